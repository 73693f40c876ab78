"""The offline driver (include/fx.h, fx_offline_frames / fx_offline_analyse) without a GPU: the tests' model of it
(tests/offline_analyse_model.py) against what the reference's own headers produced (tests/golden/offline/feature_buffer.npz, made by
tests/golden/make_feature_buffer_cases.py through tools/refdiff/refdiff_buffer.cpp from the unmodified AudioAnalysis.h / AudioFeatures.h),
bit for bit -- the windowed input of each case's last frame, and the Audio row before and after normalising --, the header against the
binding, and the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import offline_analyse_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_feature_buffer_cases import feature_buffer_inputs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "offline", "feature_buffer.npz")
ENTRIES = ("fx_offline_frames", "fx_offline_analyse")


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


def test_model_frames_equal_the_reference_headers_windowed_input(oracle):
    g, cases = np.load(GOLDEN), feature_buffer_inputs()
    assert "AudioAnalysis.h" in str(g["source"]) and "AudioFeatures.h" in str(g["source"]) and "refdiff_buffer.cpp" in str(g["source"])
    assert sorted(n for _, _, n in cases["frames"])[0] == 256 and {n for _, _, n in cases["frames"]} == set(model.WINDOWS)
    for k, (audio, nd, n) in enumerate(cases["frames"]):
        assert same(model.windowed(oracle, audio, nd, n)[-1], g["fftin_%d" % k]), k
    # the cases show what they are meant to: zero padding in front of and behind the audio, the uncentred single frame, inf * 0 = NaN
    last = len(cases["frames"]) - 1
    assert np.isnan(g["fftin_%d" % last][0]) and np.isnan(g["fftin_%d" % last][8]) and np.isneginf(g["fftin_%d" % last][9])
    both = g["fftin_11"]                                            # 200 samples, 2 downsamples, window 256: frame 1 covers samples -28 .. 227
    assert cases["frames"][11][1:] == (2, 256) and not both[:28].any() and both[28:228].all() and not both[228:].any()
    behind = g["fftin_8"]                                           # 700 samples, 20 downsamples, window 1024: frame 19 starts at sample 153
    assert behind[1:700 - 153].all() and not behind[700 - 153:].any()
    audio, nd, n = cases["frames"][5]                               # one frame: the audio from sample 0, not centred
    assert nd == 1 and same(g["fftin_5"], (audio[:n] * model.windowed(oracle, np.ones(n, np.float32), 1, n)[0]).astype(np.float32))


def test_model_audio_row_equals_the_reference_headers(oracle):
    g, cases = np.load(GOLDEN), feature_buffer_inputs()
    for k, (audio, nd) in enumerate(cases["rows"]):
        raw = model.rms_row(audio[None, :], nd)
        assert same(raw[0], g["audio_%d_raw" % k]), k
        assert same(model.normalise_row(raw)[0], g["audio_%d_norm" % k]), k
    assert same(g["audio_0_raw"], cases["rows"][0][0][:200])                             # one sample per step: the samples themselves
    assert g["audio_4_raw"].min() == -3.0 and g["audio_4_norm"].min() == -1.0          # the maximum came from |lo|
    assert not g["audio_5_raw"].any() and np.isnan(g["audio_5_norm"]).all()              # silence: 0 * (1 / 0)
    assert np.isnan(g["audio_6_norm"]).all()                                            # a NaN at row[0] stays the range's both ends
    n7 = g["audio_7_norm"]
    assert np.isnan(n7[7]) and np.isfinite(np.delete(n7, 7)).all() and np.abs(np.delete(n7, 7)).max() == 1.0    # a NaN elsewhere is stepped over


def _refdiff():
    sys.path.insert(0, os.path.join(ROOT, "tools", "refdiff"))
    import refdiff
    return refdiff


@pytest.mark.skipif(not _refdiff().legacy_available(), reason="the reference sources are not in this container (the fixture is checked above)")
def test_harness_reproduces_the_fixture():
    refdiff = _refdiff()
    g, cases = np.load(GOLDEN), feature_buffer_inputs()
    assert len(g.files) == 1 + len(cases["frames"]) + 2 * len(cases["rows"])
    for k, (audio, nd, n) in enumerate(cases["frames"]):
        assert same(refdiff.buffer_last_frame(audio, nd, n), g["fftin_%d" % k]), k
    for k, (audio, nd) in enumerate(cases["rows"]):
        raw, norm = refdiff.buffer_audio_row(audio, nd)
        assert same(raw, g["audio_%d_raw" % k]) and same(norm, g["audio_%d_norm" % k]), k


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", code)))
    assert declared == sorted(fx.capi.EXPORTS)
    lib = fx.load_library()
    for name in ENTRIES:
        assert name in declared and hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    rows = re.search(r"enum \{ (FX_OFFLINE_CENTROID = 0,.*?FX_OFFLINE_FEATURE_ROWS) \}", text, re.S).group(1)
    names = [n.strip().split(" ")[0] for n in rows.split(",")]
    assert names == ["FX_OFFLINE_" + n for n in ("CENTROID", "SLOPE", "SPREAD", "FLATNESS", "FLUX", "ZERO_CROSSES", "F0", "HER", "INHARMONICITY",
                                                 "AUDIO", "FEATURE_ROWS")]
    c = fx.capi
    assert [getattr(c, n[3:]) for n in names] == list(range(11)) == [model.CENTROID, model.SLOPE, model.SPREAD, model.FLATNESS, model.FLUX,
                                                                     model.ZERO_CROSSES, model.F0, model.HER, model.INHARMONICITY, model.AUDIO,
                                                                     model.FEATURE_ROWS]
    assert ("enum { FX_OFFLINE_DO_SPECTRAL = 1, FX_OFFLINE_DO_HARMONIC = 2, FX_OFFLINE_DO_ZERO_CROSSES = 4, FX_OFFLINE_DO_AUDIO = 8,\n"
            "       FX_OFFLINE_DO_NORMALISE_AUDIO = 16, FX_OFFLINE_DO_LOG_ATTACK = 32 };") in text
    assert (c.OFFLINE_DO_SPECTRAL, c.OFFLINE_DO_HARMONIC, c.OFFLINE_DO_ZERO_CROSSES, c.OFFLINE_DO_AUDIO, c.OFFLINE_DO_NORMALISE_AUDIO,
            c.OFFLINE_DO_LOG_ATTACK) == (1, 2, 4, 8, 16, 32)
    assert "#define FX_OFFLINE_SCRATCH_BYTES (16u << 20)" in text and c.OFFLINE_SCRATCH_BYTES == 16 << 20 == model.SCRATCH_BYTES
    assert c.OFFLINE_WINDOWS == model.WINDOWS
    for method in ("magnitude_frames", "perform_spectral_analysis"):
        assert callable(getattr(fx.offline.AudioAnalyser, method))
    for method in ("get_feature_buffer", "get_feature_sample", "get_feature_range", "get_average_feature_sample", "fft_bins"):
        assert callable(getattr(fx.offline.ConcatenatedFeatureBuffer, method))


def test_entries_refuse_a_null_handle_before_device_use(fx):
    lib = fx.load_library()
    f = (ctypes.c_float * 4096)()
    p = ctypes.cast(f, ctypes.c_void_p)
    assert lib.fx_offline_frames(None, p, 1024, 1, 1024, p, None, fx.capi.MEM_HOST) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"null argument" in lib.fx_last_error()
    assert lib.fx_offline_analyse(None, p, 1024, 1, 1024, 48000, 63, p, None, p, None, fx.capi.MEM_HOST) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"null argument" in lib.fx_last_error()


def test_feature_buffer_carries_the_reference_names(fx):
    """ConcatenatedFeatureBuffer is host arithmetic: the layout (ref AudioFeatures.h:124-140), findMinMax over every channel's row (:208-213),
    the serial float average (:266-275) and the [bin][downsample] view of setFFTBinsForSample (:142-156)."""
    rng = np.random.default_rng(3)
    C, D, B = 3, 7, 5
    feat = rng.normal(0, 1, (10, C, D)).astype(np.float32)
    mags = rng.normal(0, 1, (D, C, B)).astype(np.float32)
    buf = fx.offline.ConcatenatedFeatureBuffer(feat, np.zeros((C, D), np.float32), np.zeros(C, np.float32), mags, D, 44100)
    flat = feat.reshape(-1)
    for r, c, i in ((0, 0, 0), (4, 2, 6), (9, 1, 3)):
        assert buf.get_feature_sample(r, c, i) == flat[r * D * C + c * D + i]           # arrayStartIndex + index
    assert same(buf.get_feature_buffer(fx.capi.OFFLINE_FLUX), feat[4])
    assert buf.get_feature_range(2) == (feat[2].min(), feat[2].max())
    av = np.float32(0.0)
    for c in range(C):
        av = np.float32(av + feat[6, c, 2])
    assert buf.get_average_feature_sample(6, 2) == np.float32(av / np.float32(C))
    assert buf.fft_bins(1).shape == (B, D) and buf.fft_bins(1)[3, 5] == mags[5, 1, 3]
    assert buf.num_downsamples == D and buf.sample_rate == 44100
