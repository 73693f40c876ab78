"""fx_offline_analyse_files / fx_offline_set_nyquists (include/fx.h) without a GPU: the tests' model of the files entry
(tests/offline_files_model.py) against the model of the one-length entry, its widening against the project's WAV reader, the header against
the binding, and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np

import offline_analyse_model as model
import offline_files_model as files_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fx_offline_analyse_files", "fx_offline_set_nyquists", "fx_offline_get_nyquists")


def same(a, b):
    """bit for bit; a NaN equals a NaN whatever its sign and payload"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.tobytes() == b.tobytes():
        return True
    if a.dtype.kind != "f":
        return False
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


def test_model_on_equal_lengths_is_the_one_length_model(oracle):
    N, C, S, D, rate, nyq = 256, 3, 1500, 6, 48000, 24000.0
    rng = np.random.default_rng(11)
    t = np.arange(S) / float(rate)
    audio = np.stack([0.2 * np.sin(2 * np.pi * 1500.0 * t) + rng.normal(0, 0.01, S), np.zeros(S), rng.normal(0, 0.1, S)]).astype(np.float32)
    state, states = model.State(C), files_model.States(C)
    for call in range(2):                                           # the second call starts from the first one's state
        want = model.analyse(oracle, state, audio, D, N, rate, nyq)
        got = files_model.analyse(oracle, states, audio.reshape(-1), [S] * C, files_model.F32, D, N, rate, nyq)
        for g, w in zip(got, want):
            assert same(g, w), call
        assert same(states.previous_f0, state.previous_f0) and same(states.previous_bins, state.previous_bins)
    assert state.previous_f0[0] > 0 and state.previous_bins[2].any()


def test_widening_is_the_wav_readers(fx, tmp_path):
    rng = np.random.default_rng(12)
    x = np.concatenate([rng.uniform(-1.2, 1.2, 997), [-1.0, 1.0, 0.0, -2.0 ** -23, 2.0 ** -15, 1.0 - 2.0 ** -23]])
    for fmt, name in ((files_model.S16, "pcm16"), (files_model.S24, "pcm24"), (files_model.F32, "float32")):
        path = str(tmp_path / (name + ".wav"))
        fx.wav.write_wav(path, 48000, x, name)
        _, decoded, _ = fx.wav.read_wav(path)
        payload = open(path, "rb").read()[44:44 + x.shape[0] * files_model.BYTES[fmt]]
        raw = np.frombuffer(payload, files_model.DTYPE[fmt])
        assert same(files_model.widen(raw, fmt), decoded[:, 0]), name
        assert same(files_model.quantise(x, fmt), raw), name        # (the tests' quantiser writes what the WAV writer writes)
    h = rng.uniform(-1, 1, 100).astype(np.float16)
    assert same(files_model.widen(h, files_model.F16).astype(np.float16), h)
    assert [files_model.F32, files_model.F16, files_model.S16, files_model.S24] == [fx.capi.SAMPLE_F32, fx.capi.SAMPLE_F16, fx.capi.SAMPLE_S16,
                                                                                   fx.capi.SAMPLE_S24]


def test_split_starts_each_file_where_the_ones_before_it_end():
    lengths = [5, 1, 9]
    bank = files_model.quantise(np.linspace(-0.9, 0.9, 15), files_model.S24)
    files = files_model.split(bank, lengths, files_model.S24)
    assert [f.shape[0] for f in files] == [15, 3, 27] and same(np.concatenate(files), bank)
    assert same(files_model.widen(files[2], files_model.S24), files_model.widen(bank, files_model.S24)[6:])


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(fx.capi.EXPORTS)
    lib = fx.load_library()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6 and "#define FX_ABI_VERSION 6" in text
    for method in ("perform_spectral_analysis_files", "set_nyquists"):
        assert callable(getattr(fx.offline.AudioAnalyser, method))
    assert isinstance(fx.offline.AudioAnalyser.nyquists, property)


def test_entries_refuse_a_null_handle_before_device_use(fx):
    lib = fx.load_library()
    f = (ctypes.c_float * 4096)()
    p = ctypes.cast(f, ctypes.c_void_p)
    lengths, rates, nyq = (ctypes.c_longlong * 1)(4096), (ctypes.c_int * 1)(48000), (ctypes.c_double * 1)(24000.0)
    assert lib.fx_offline_analyse_files(None, p, lengths, fx.capi.SAMPLE_F32, 1, 1024, rates, 63, p, None, p, None,
                                        fx.capi.MEM_HOST) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"null argument" in lib.fx_last_error()
    assert lib.fx_offline_set_nyquists(None, nyq) == fx.capi.FX_ERR_INVALID_ARGUMENT and b"null argument" in lib.fx_last_error()
    assert lib.fx_offline_get_nyquists(None, nyq) == fx.capi.FX_ERR_INVALID_ARGUMENT and b"null argument" in lib.fx_last_error()


def test_feature_buffer_carries_each_files_length_and_rate(fx):
    C, D = 3, 4
    feat = np.zeros((10, C, D), np.float32)
    buf = fx.offline.ConcatenatedFeatureBuffer(feat, np.zeros((C, D), np.float32), None, None, D, [44100, 48000, 44100], num_samples=[8, 9, 300])
    assert buf.sample_rate.tolist() == [44100, 48000, 44100] and buf.num_samples.tolist() == [8, 9, 300]
    one = fx.offline.ConcatenatedFeatureBuffer(feat, np.zeros((C, D), np.float32), None, None, D, 44100)
    assert one.sample_rate == 44100 and one.num_samples is None
