"""A library of files of different lengths in one call (include/fx.h, fx_offline_analyse_files) and each channel's own nyquist
(fx_offline_set_nyquists) on the GPU.  Every file's results against a one-channel analyser given fx_offline_analyse on that file alone, bit
for bit, and against the tests' model (tests/offline_files_model.py); the wire formats against the fp32 entry on the widened floats, with
file starts at every alignment; the uncentred single frame; equal lengths against fx_offline_analyse; the seams between chunks of the
scratch; the nyquists against analysers created at each value; the refusals."""
import ctypes

import numpy as np
import pytest

import offline_analyse_model as model
import offline_files_model as files_model

pytestmark = pytest.mark.gpu

EXACT_ROWS = [model.CENTROID, model.FLUX, model.SLOPE, model.ZERO_CROSSES, model.F0, model.HER, model.INHARMONICITY, model.AUDIO]
PIECE_ROWS = [r for r in range(model.FEATURE_ROWS) if r != model.AUDIO]


def same(a, b):
    """bit for bit; a NaN equals a NaN whatever its sign and payload (tests/test_gpu_offline_analyse.py)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.tobytes() == b.tobytes():
        return True
    if a.dtype.kind != "f":
        return False
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def ragged_files(lengths, seed, fundamental, silent, sample_rate=48000):
    """one float32 file per length: harmonics of the fundamental plus noise at a level of its own; file `silent` is all zeros"""
    rng = np.random.default_rng(seed)
    files = []
    for c, S in enumerate(lengths):
        t = np.arange(S) / float(sample_rate)
        tone = sum(np.sin(2 * np.pi * fundamental * h * t) / h for h in range(1, 7))
        level = 0.25 / (1 + c % 3)
        files.append((level * tone + rng.normal(0, 0.05 * level, S)).astype(np.float32) if c != silent else np.zeros(S, np.float32))
    return files


def device_bank(files, fmt):
    """the files back to back in one CUDA tensor that ends where the last file ends, with their lengths"""
    import torch
    per = 3 if fmt == files_model.S24 else 1
    bank = torch.from_numpy(np.concatenate(files)).cuda()
    return bank, [f.shape[0] // per for f in files]


def through_files(an, files, fmt, D, N, rates, device, **flags):
    if device:
        return an.perform_spectral_analysis_files(device_bank(files, fmt), D, N, rates, keep_fft=True, sample_format=fmt, **flags)
    return an.perform_spectral_analysis_files(files, D, N, rates, keep_fft=True, sample_format=fmt, **flags)


def assert_same_results(got, want, where):
    """two ConcatenatedFeatureBuffers (or a buffer and a (features, energy, lat, mags) tuple), every output bit for bit"""
    if not isinstance(want, tuple):
        want = (want.feature_buffer, want.energy_envelope, want.estimated_log_attack_time, want.magnitudes)
    assert same(got.magnitudes, want[3]), where
    assert same(got.energy_envelope, want[1]), where
    assert same(got.estimated_log_attack_time, want[2]), (where, got.estimated_log_attack_time, want[2])
    for r in range(model.FEATURE_ROWS):
        assert same(got.feature_buffer[r], want[0][r]), (where, r, got.feature_buffer[r], want[0][r])


def assert_equals_the_model(got, want, where):
    features, energy, lat, mags = want
    assert same(got.magnitudes, mags) and same(got.energy_envelope, energy) and same(got.estimated_log_attack_time, lat), where
    for r in EXACT_ROWS:
        assert same(got.feature_buffer[r], features[r]), (where, r, got.feature_buffer[r], features[r])
    for r in (model.SPREAD, model.FLATNESS):                        # pow() is rounded independently on the device: tests/test_offline.py's budget
        np.testing.assert_allclose(got.feature_buffer[r], features[r], rtol=2e-7, atol=0)


class Alone:
    """one one-channel analyser per file, each given fx_offline_analyse on its file alone"""

    def __init__(self, gpu_fx, nyquists):
        self.each = [gpu_fx.offline.AudioAnalyser(1, float(v)) for v in nyquists]

    def analyse(self, floats, D, N, rates, **flags):
        parts = [an.perform_spectral_analysis(f[None, :], D, N, int(r), keep_fft=True, **flags) for an, f, r in zip(self.each, floats, rates)]
        return (np.concatenate([p.feature_buffer for p in parts], axis=1), np.concatenate([p.energy_envelope for p in parts], axis=0),
                np.concatenate([p.estimated_log_attack_time for p in parts]), np.concatenate([p.magnitudes for p in parts], axis=1))

    def reset(self):
        for an in self.each:
            an.reset()

    @property
    def previous_f0(self):
        return np.concatenate([an.previous_f0 for an in self.each])

    @property
    def previous_bin_magnitudes(self):
        return np.concatenate([an.previous_bin_magnitudes for an in self.each])


# ---- 1. ragged equals alone ----
RAGGED = dict(N=256, D=8, lengths=[8, 9, 300, 777, 2049, 4100], rates=[48000, 44100, 48000, 44100, 22050, 96000], seed=1, silent=3)
_ragged = {}


def ragged_case(oracle):
    if not _ragged:                                                 # (the model runs once; nothing changes what it returned)
        k = RAGGED
        files = ragged_files(k["lengths"], k["seed"], 1500.0, k["silent"])
        states = files_model.States(len(files))
        want = files_model.analyse(oracle, states, np.concatenate(files), k["lengths"], files_model.F32, k["D"], k["N"], k["rates"], 24000.0)
        for a in files + list(want):
            a.setflags(write=False)
        _ragged.update(files=files, want=want, f0=states.previous_f0, bins=states.previous_bins)
    return _ragged


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_ragged_files_equal_each_file_alone_and_the_model(gpu_fx, oracle, device):
    k, case = RAGGED, ragged_case(oracle)
    files, want, N, D, C = case["files"], case["want"], RAGGED["N"], RAGGED["D"], len(RAGGED["lengths"])
    # the case is what it is meant to be, by the model alone: a pitch is found in some file, the silent file passes no gate and its attack time
    # is log10 (0), the length-8 file has step = spb = 1 and nearly all of every window is padding
    assert (want[0][model.F0] > 0).any() and not want[0][PIECE_ROWS][:, k["silent"]].any() and np.isneginf(want[2][k["silent"]])
    assert np.isfinite(want[2][:3]).all() and len(set(want[2][:3].tolist())) == 3 and k["lengths"][0] // D == 1 and k["lengths"][3] % D and k["lengths"][4] == 2049
    an, alone = gpu_fx.offline.AudioAnalyser(C, 24000.0), Alone(gpu_fx, [24000.0] * C)
    got = through_files(an, files, files_model.F32, D, N, k["rates"], device)
    assert got.magnitudes.shape == (D, C, N // 2 + 1) and got.num_samples.tolist() == k["lengths"] and got.sample_rate.tolist() == k["rates"]
    assert_same_results(got, alone.analyse(files, D, N, k["rates"]), "alone")
    assert same(an.previous_f0, alone.previous_f0) and same(an.previous_bin_magnitudes, alone.previous_bin_magnitudes)
    assert_equals_the_model(got, want, "model")
    assert same(an.previous_f0, case["f0"]) and same(an.previous_bin_magnitudes, case["bins"])
    raw = through_files(gpu_fx.offline.AudioAnalyser(C), files, files_model.F32, D, N, k["rates"], device, spectral=False, harmonic=False,
                        zero_crosses=False, normalise=False, log_attack=False)
    assert same(raw.feature_buffer[model.AUDIO][0], files[0]) and same(raw.feature_buffer[model.AUDIO], model_audio_rows(files, D))
    assert not raw.feature_buffer[:model.AUDIO].any() and raw.estimated_log_attack_time is None


def model_audio_rows(files, D):
    return np.concatenate([model.rms_row(f[None, :], D) for f in files])


# ---- 2. the same at 1024 points; the state goes from call to call ----
def test_two_calls_with_other_lengths_carry_each_files_state_and_reset_restores_it(gpu_fx, oracle):
    N, D, C, rates, nyq = 1024, 20, 4, [48000, 44100, 48000, 32000], 24000.0
    calls = [ragged_files([11003, 12000, 12345, 13001], 31, 220.0, 2), ragged_files([12500, 11111, 13000, 12001], 32, 330.0, 2)]
    an, alone, states = gpu_fx.offline.AudioAnalyser(C, nyq), Alone(gpu_fx, [nyq] * C), files_model.States(C)
    first = None
    for call, files in enumerate(calls):                            # the second call starts from the first one's state
        got = through_files(an, files, files_model.F32, D, N, rates, device=bool(call))
        assert_same_results(got, alone.analyse(files, D, N, rates), call)
        assert same(an.previous_f0, alone.previous_f0) and same(an.previous_bin_magnitudes, alone.previous_bin_magnitudes), call
        want = files_model.analyse(oracle, states, np.concatenate(files), [f.shape[0] for f in files], files_model.F32, D, N, rates, nyq)
        assert_equals_the_model(got, want, call)
        assert same(an.previous_f0, states.previous_f0) and same(an.previous_bin_magnitudes, states.previous_bins), call
        assert (got.feature_buffer[model.F0][[0, 1, 3]] > 0).any() and not got.feature_buffer[PIECE_ROWS][:, 2].any()
        first = got if first is None else first
    assert an.previous_f0[[0, 1, 3]].all()
    again = through_files(an, calls[0], files_model.F32, D, N, rates, device=False)
    assert not same(again.feature_buffer[model.FLUX], first.feature_buffer[model.FLUX])           # (the state matters ...)
    an.reset()
    assert_same_results(through_files(an, calls[0], files_model.F32, D, N, rates, device=False), first, "after reset")   # ... and reset restores it


# ---- 3. the wire formats, with file starts at every alignment ----
FORMAT_LENGTHS = [9, 13, 301, 777, 2049, 4101]      # all = 1 (mod 4): S24 files start at bytes 0, 3, 2, 1 (mod 4); all odd: every other 16-bit file starts off a 4-byte boundary


@pytest.mark.parametrize("fmt", [files_model.F16, files_model.S16, files_model.S24], ids=["f16", "s16", "s24"])
def test_formats_equal_the_fp32_entry_on_the_widened_floats(gpu_fx, fmt):
    N, D, C, rates = 256, 8, len(FORMAT_LENGTHS), RAGGED["rates"]
    starts = np.concatenate([[0], np.cumsum(FORMAT_LENGTHS)[:-1]]) * files_model.BYTES[fmt]
    assert all(s % 4 == 1 for s in FORMAT_LENGTHS) and (set(starts % 4) == {0, 1, 2, 3} if fmt == files_model.S24 else set(starts % 4) == {0, 2})
    wire = [files_model.quantise(f, fmt) for f in ragged_files(FORMAT_LENGTHS, 3, 1500.0, 3)]
    floats = [files_model.widen(w, fmt) for w in wire]
    assert wire[0].dtype == files_model.DTYPE[fmt] and any(not same(a, b) for a, b in zip(floats, ragged_files(FORMAT_LENGTHS, 3, 1500.0, 3)))
    want_an = gpu_fx.offline.AudioAnalyser(C)
    want = through_files(want_an, floats, files_model.F32, D, N, rates, device=False)
    assert (want.feature_buffer[model.F0] > 0).any() and want.feature_buffer[model.AUDIO].any()
    for device in (False, True):
        an = gpu_fx.offline.AudioAnalyser(C)
        assert_same_results(through_files(an, wire, fmt, D, N, rates, device), want, (fmt, device))
        assert same(an.previous_f0, want_an.previous_f0) and same(an.previous_bin_magnitudes, want_an.previous_bin_magnitudes)


# ---- 4. one downsample: the uncentred single frame ----
def test_one_downsample_is_the_uncentred_frame_of_each_file(gpu_fx, oracle):
    N, lengths, rates = 256, [256, 300, 1000], [48000, 44100, 48000]
    files = ragged_files(lengths, 4, 1500.0, -1)
    an, alone = gpu_fx.offline.AudioAnalyser(3), Alone(gpu_fx, [24000.0] * 3)
    got = through_files(an, files, files_model.F32, 1, N, rates, device=True)
    assert_same_results(got, alone.analyse(files, 1, N, rates), "alone")
    assert_equals_the_model(got, files_model.analyse(oracle, files_model.States(3), np.concatenate(files), lengths, files_model.F32, 1, N, rates, 24000.0), "model")
    assert same(got.magnitudes, model.magnitude_frames(oracle, np.stack([f[:N] for f in files]), 1, N)[0])     # from sample 0, not centred
    short = [files[0], files[1][:255], files[2]]
    with pytest.raises(gpu_fx.capi.FxError) as e:
        through_files(an, short, files_model.F32, 1, N, rates, device=False)
    assert "file 1" in str(e.value) and "window_size 256" in str(e.value) and "255" in str(e.value)


# ---- 5. equal lengths: the new entry is the old ----
def test_equal_lengths_equal_fx_offline_analyse(gpu_fx):
    N, C, S, D, rate = 512, 4, 3001, 10, 44100
    files = ragged_files([S] * C, 5, 440.0, 1, rate)
    old, new = gpu_fx.offline.AudioAnalyser(C, 22050.0), gpu_fx.offline.AudioAnalyser(C, 22050.0)
    for call in range(2):
        want = old.perform_spectral_analysis(np.stack(files), D, N, rate, keep_fft=True)
        assert_same_results(through_files(new, files, files_model.F32, D, N, rate, device=bool(call)), want, call)
        assert same(new.previous_f0, old.previous_f0) and same(new.previous_bin_magnitudes, old.previous_bin_magnitudes)
    assert (want.feature_buffer[model.F0] > 0).any()


# ---- 6. the seams between chunks of the scratch ----
def test_chunks_of_the_scratch_leave_the_same_bits(gpu_fx):
    """C = 32, N = 4096: F = (16 << 20) div (4 * 32 * 2049) = 63 frames fit the scratch (tests/test_gpu_offline_analyse.py), so the 70 frames
    are cut after frame 62.  GPU against GPU: with the magnitudes kept nothing is cut."""
    import torch
    C, N, D, rate = 32, 4096, 70, 48000
    assert max(1, model.SCRATCH_BYTES // (4 * C * (N // 2 + 1))) == 63
    lengths = np.linspace(4480, 9000, C).astype(np.int64)
    assert lengths[0] == 4480 and len(set(lengths.tolist())) == C
    rng = np.random.default_rng(6)
    bank = torch.from_numpy(np.concatenate([rng.normal(0, 0.3, S) * np.linspace(0.2, 1.0, S) for S in lengths]).astype(np.float32)).cuda()
    only = dict(harmonic=False, zero_crosses=False, audio_rms=False, normalise=False, log_attack=False)
    kept_an, cut_an = gpu_fx.offline.AudioAnalyser(C), gpu_fx.offline.AudioAnalyser(C)
    kept = kept_an.perform_spectral_analysis_files((bank, lengths), D, N, rate, keep_fft=True, **only)
    cut = cut_an.perform_spectral_analysis_files((bank, lengths), D, N, rate, keep_fft=False, **only)
    assert same(cut.feature_buffer, kept.feature_buffer) and same(cut.energy_envelope, kept.energy_envelope)
    assert same(cut_an.previous_bin_magnitudes, kept_an.previous_bin_magnitudes) and same(cut_an.previous_f0, kept_an.previous_f0)
    assert kept.feature_buffer[model.FLUX][:, [62, 63, D - 1]].all() and kept.feature_buffer[model.CENTROID].all() and cut.magnitudes is None


# ---- 7. each channel's own nyquist ----
def test_nyquists_are_each_channels_own(gpu_fx):
    N, D, C, B, rates = 256, 8, 3, 129, [44100, 48000, 22050]
    values = np.array([22050.0, 24000.0, 11025.0])
    files = ragged_files([2049, 777, 4100], 7, 1500.0, -1)
    mags = np.abs(np.random.default_rng(7).normal(0, 1, (C, B))).astype(np.float32)
    mags[:, 20::20] += 30.0                                         # peaks for the histogram
    data = np.random.default_rng(8).normal(0, 1, (C, 64, 2)).astype(np.float32)
    an = gpu_fx.offline.AudioAnalyser(C, 24000.0)
    assert same(an.nyquists, np.full(C, 24000.0))                   # before the first set: the creation value
    an.perform_spectral_analysis(np.stack([f[:700] for f in files]), D, N, 48000)
    f0, bins = an.previous_f0, an.previous_bin_magnitudes
    an.set_nyquists(values)
    assert same(an.nyquists, values) and same(an.previous_f0, f0) and same(an.previous_bin_magnitudes, bins)      # the state is left alone
    an.reset()
    alone = Alone(gpu_fx, values)
    # the per-frame entries
    assert same(an.calculate_spectral_characteristics(mags), np.concatenate([a.calculate_spectral_characteristics(mags[c:c + 1]) for c, a in enumerate(alone.each)]))
    got3 = an.calculate_harmonic_characteristics(mags)
    assert same(got3, np.concatenate([a.calculate_harmonic_characteristics(mags[c:c + 1]) for c, a in enumerate(alone.each)])) and (got3[:, 0] > 0).all()
    got_ac = an.analyse_auto_correlation(data)
    for c, a in enumerate(alone.each):
        want_ac = a.analyse_auto_correlation(data[c:c + 1])
        assert same(got_ac[0][c:c + 1], want_ac[0]) and same(got_ac[1][c:c + 1], want_ac[1]) and same(got_ac[2][c:c + 1], want_ac[2])
    assert len(set(got3[:, 0].tolist())) == C                       # (the values matter: the same magnitudes, three pitches)
    an.reset()
    alone.reset()
    # fx_offline_analyse and the files entry
    same_length = [f[:700] for f in files]
    assert_same_results(an.perform_spectral_analysis(np.stack(same_length), D, N, 48000, keep_fft=True), alone.analyse(same_length, D, N, [48000] * C), "analyse")
    assert_same_results(through_files(an, files, files_model.F32, D, N, rates, device=True), alone.analyse(files, D, N, rates), "files")
    assert same(an.previous_f0, alone.previous_f0) and same(an.previous_bin_magnitudes, alone.previous_bin_magnitudes)
    # an object set to its creation value in every channel is an object never set
    never, set_same = gpu_fx.offline.AudioAnalyser(C, 22050.0), gpu_fx.offline.AudioAnalyser(C, 22050.0)
    set_same.set_nyquists([22050.0] * C)
    assert_same_results(through_files(set_same, files, files_model.F32, D, N, rates, device=False), through_files(never, files, files_model.F32, D, N, rates, device=False), "never set")
    assert same(never.nyquists, np.full(C, 22050.0))


# ---- 8. refusals ----
def test_refusals_come_before_any_launch_copy_or_state_change(gpu_fx):
    import torch
    capi = gpu_fx.capi
    C, N, D = 2, 256, 8
    lengths, rates = np.array([2000, 1500], np.int64), np.array([48000, 44100], np.int32)
    files = ragged_files(lengths, 5, 1500.0, -1)
    bank = np.concatenate(files)
    an = gpu_fx.offline.AudioAnalyser(C, 24000.0)
    an.set_nyquists([24000.0, 22050.0])
    an.perform_spectral_analysis_files(files, D, N, rates)
    f0, bins, nyq = an.previous_f0, an.previous_bin_magnitudes, an.nyquists
    assert f0.any() and bins.shape == (C, N // 2 + 1) and bins.any()
    lib, h = an._lib, an._h
    CANARY = np.float32(-1234.5)
    features = np.full((model.FEATURE_ROWS, C, D), CANARY)
    energy, lat, mags = np.full((C, D), CANARY), np.full(C, CANARY), np.full((D, C, 4096 // 2 + 1), CANARY)

    def refused(status, *words):
        assert status == capi.FX_ERR_INVALID_ARGUMENT, status
        message = lib.fx_last_error().decode()
        for w in words:
            assert str(w) in message, (w, message)
        assert same(an.previous_f0, f0) and same(an.previous_bin_magnitudes, bins) and same(an.nyquists, nyq), message
        for out in (features, energy, lat, mags):
            assert (out == CANARY).all(), message

    def analyse(bank=bank, lengths=lengths, fmt=capi.SAMPLE_F32, D=D, N=N, rates=rates, what=model.DO_ALL, features=features, lat=lat, kind=capi.MEM_HOST):
        lp = None if lengths is None else np.ascontiguousarray(lengths, np.int64).ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
        rp = None if rates is None else np.ascontiguousarray(rates, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        return lib.fx_offline_analyse_files(h, vp(bank), lp, fmt, D, N, rp, what, vp(features), vp(energy), vp(lat), vp(mags), kind)

    # what fx_offline_analyse refuses that still applies
    refused(analyse(bank=None), "null argument")
    refused(analyse(features=None), "null argument")
    refused(analyse(D=0), "num_downsamples 0")
    for n in (0, 128, 1000, 8192, -256):
        refused(analyse(N=n), "window_size %d" % n)
    refused(analyse(kind=7), "memory kind 7")
    refused(analyse(what=model.DO_NORMALISE_AUDIO | model.DO_SPECTRAL), "FX_OFFLINE_DO_NORMALISE_AUDIO", model.DO_NORMALISE_AUDIO | model.DO_SPECTRAL)
    refused(analyse(lat=None), "log_attack_time")
    refused(analyse(N=512), "129 bins", "257")                     # previousBinMagnitudes has this analyser's window size
    # the files entry's own
    refused(analyse(lengths=None), "null argument")
    refused(analyse(lengths=[2000, 0]), "file 1", "num_samples 0")
    refused(analyse(lengths=[-3, 1500]), "file 0", "num_samples -3")
    refused(analyse(lengths=[2000, 1 << 31]), "file 1", "num_samples %d" % (1 << 31))
    refused(analyse(lengths=[2000, 7]), "file 1", "num_downsamples 8", "num_samples 7")
    refused(analyse(lengths=[255, 1500], D=1), "file 0", "window_size 256", "255")
    for fmt in (-1, 4, 99):
        refused(analyse(fmt=fmt), "sample format %d" % fmt)
    refused(analyse(rates=None), "sample_rates")
    refused(analyse(rates=[48000, 999]), "file 1", "sample_rate 999")
    d_bank = torch.from_numpy(np.concatenate([np.zeros(1, np.int16), files_model.quantise(bank, files_model.S16)])).cuda()
    torch.cuda.synchronize()
    d_out = torch.full((model.FEATURE_ROWS * C * D,), float(CANARY), dtype=torch.float32, device="cuda")
    assert d_bank.data_ptr() % 4 == 0
    status = lib.fx_offline_analyse_files(h, ctypes.c_void_p(d_bank.data_ptr() + 2), np.ascontiguousarray(lengths).ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)),
                                          capi.SAMPLE_S16, D, N, None, 0, vp(d_out), None, None, None, capi.MEM_DEVICE)
    refused(status, "4-byte boundary")
    capi.check(lib.fx_offline_sync(h))
    assert (d_out.cpu().numpy() == CANARY).all()
    # the setter: per entry what fx_offline_create refuses, naming the channel, changing nothing
    for bad in (0.0, -24000.0, float("nan")):
        refused(lib.fx_offline_set_nyquists(h, np.array([22050.0, bad]).ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "channel 1", "nyquist")
    refused(lib.fx_offline_set_nyquists(h, None), "null argument")
    # and what is not refused: the sample rates are the log attack time's alone, the window size is the spectral analysis's
    assert analyse(rates=None, what=model.DO_ALL & ~model.DO_LOG_ATTACK) == capi.FX_OK
    assert analyse(N=512, what=model.DO_ALL & ~model.DO_SPECTRAL) == capi.FX_OK
    assert not (features == CANARY).any() and same(an.previous_bin_magnitudes, bins)
