"""Analysis taps (include/fx.h, fx_request_taps / fx_get_taps) without a GPU: the committed fixtures -- the reference's display buffers
read through its own getters (tests/golden/taps/make_taps.py) -- are the oracle's arithmetic bit for bit, the C ABI declares and
exports both entry points, and they refuse bad arguments before any device use."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest

import taps_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = os.path.join(ROOT, "tests", "golden", "taps")
FIXTURES = sorted(glob.glob(os.path.join(TAPS, "*.npz")))


def _captures(path):
    d = np.load(path)
    N, gain = int(d["window_size"]), np.float32(d["gain"])
    hops = d["hops"]
    for i, k in enumerate(d["captures"]):
        tail = hops[k - 1] * gain if k > 0 else np.zeros(N // 2, np.float32)
        window = np.concatenate([tail, hops[k] * gain]).astype(np.float32)
        yield int(k), window, {f: d[f][i] for f in taps_model.FIELDS}


def test_fixtures_cover_the_issue():
    sizes = set()
    gains, first = [], False
    for p in FIXTURES:
        d = np.load(p)
        sizes.add(int(d["window_size"]))
        gains.append(float(d["gain"]))
        first |= 0 in d["captures"]
        assert "refdiff_taps.cpp" in str(d["source"])
    assert len(FIXTURES) >= 7 and {256, 1024, 2048, 4096} <= sizes and first and any(g != 1.0 for g in gains)
    assert sum(os.path.getsize(p) for p in FIXTURES) < 4 << 20


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fixture_is_the_oracle_bit_for_bit(oracle, path):
    for k, window, ref in _captures(path):
        N = window.shape[0]
        what = "%s hop %d" % (os.path.basename(path), k)
        # the overlapped window: the previous hop and this one, both times the gain
        assert np.array_equal(ref["window"], window, equal_nan=True), what
        # the spectra: fxo_forward_real after fxo_bartlett, and after fxo_lowpass + fxo_bartlett
        spectrum = oracle.forward_real(oracle.bartlett(window))
        pitch = oracle.forward_real(oracle.bartlett(oracle.lowpass(window)))
        assert np.array_equal(ref["spectrum"], spectrum, equal_nan=True), what
        assert np.array_equal(ref["pitch_spectrum"], pitch, equal_nan=True), what
        # CND and lag: fxo_estimate_pitch
        _, lag, cnd2n = oracle.estimate_pitch(pitch)
        assert np.array_equal(ref["cnd"], cnd2n[:N], equal_nan=True), what
        x = ref["lag_position"][0]
        if x >= 0:
            assert x * np.float32(2 * N) == np.float32(lag), (what, x, lag)
            assert ref["lag_position"][1] == cnd2n[int(lag)], what
        else:
            assert x == np.float32(-1.0) / np.float32(2 * N) and ref["lag_position"][1] == np.float32(100.0), what
        assert np.array_equal(ref["lag_position"], taps_model.lag_position(cnd2n, N), equal_nan=True), what
        # the autocorrelation, restated from fxo_fft_complex(inverse) x 1.0f / N; its running sum reproduces the oracle's CND
        v = taps_model.autocorrelation(oracle, pitch)
        assert np.array_equal(ref["autocorrelation"], v[:N], equal_nan=True), what
        assert np.array_equal(taps_model.cnd_from(v), cnd2n, equal_nan=True), what
        # and the whole model agrees
        taps_model.assert_taps_equal(ref, taps_model.oracle_taps(oracle, window), what)


def test_fixtures_exercise_every_lag_outcome():
    found, missed, nonfinite = False, False, False
    for p in FIXTURES:
        for _, window, ref in _captures(p):
            found |= ref["lag_position"][0] >= 0
            missed |= ref["lag_position"][0] < 0
            nonfinite |= not all(np.isfinite(ref[f]).all() for f in taps_model.FIELDS)
    assert found and missed and nonfinite


def _refdiff():
    sys.path.insert(0, os.path.join(ROOT, "tools", "refdiff"))
    sys.path.insert(0, TAPS)
    import refdiff
    import make_taps
    return refdiff, make_taps


@pytest.mark.skipif(not _refdiff()[0].available(), reason="the reference sources are not in this container (fixtures are checked above)")
def test_driver_reproduces_the_fixtures():
    _, make_taps = _refdiff()
    cases = make_taps.cases()
    assert sorted(cases) == sorted(os.path.basename(p)[:-4] for p in FIXTURES)
    for name, (N, hops, captures, gain) in cases.items():
        d = np.load(os.path.join(TAPS, name + ".npz"))
        assert np.array_equal(d["hops"], hops) and list(d["captures"]) == captures and np.float32(d["gain"]) == np.float32(gain), name
        got = make_taps.run(hops, N, captures, gain)
        for f in taps_model.FIELDS:
            assert np.array_equal(got[f], d[f], equal_nan=True), (name, f)


def test_header_declares_and_library_exports_the_taps(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read()
    assert "#define FX_MAX_TAP_CHANNELS 64" in text
    for name in ("fx_request_taps", "fx_get_taps"):
        assert name + "(" in text.replace(" (", "(")
        assert name in fx.capi.EXPORTS
        assert hasattr(fx.load_library(), name)
    assert fx.capi.LAUNCH_KINDS[9] == "taps" and fx.capi.MAX_TAP_CHANNELS == 64


def test_taps_refuse_a_null_context_before_device_use(fx):
    lib = fx.load_library()
    ch = (ctypes.c_int * 2)(0, 1)
    f = (ctypes.c_float * 8)()
    assert lib.fx_request_taps(None, ch, 2) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"null context" in lib.fx_last_error()
    assert lib.fx_get_taps(None, 0, f, f, f, f, f, f, None) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"null context" in lib.fx_last_error()
