"""The level cases (tests/level_cases.py) on the CPU: the oracle's answer is defined at every kept level, the inputs can tell an
implementation that flushes subnormals from one that does not, the oracle equals the reference's own headers across the sweep (recorded
in tests/golden/levels/cases.npz by tests/golden/make_level_cases.py), a gain reaches the same place as samples scaled beforehand, and
the case holds the regimes of the lag search.  tests/test_gpu_levels.py holds the kernels to the oracle on the same cases."""
import ctypes
import os
import platform
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import level_cases as lc  # noqa: E402
from rate_cases import same_bits  # noqa: E402
from refdiff_record import Replay  # noqa: E402

refdiff = Replay(os.path.join(ROOT, "tests", "golden", "levels", "cases.npz"))

RMS, F0 = 1, 2
GAIN_LEVELS = (-9.0, -11.0, -13.0)


@pytest.mark.parametrize("N", lc.SIZES)
def test_inputs_are_the_recorded_ones(N):
    assert lc.hops(N).shape == (len(lc.labels(N)), lc.T, N // 2) and lc.crc(N) == lc.CRC[N]


@pytest.mark.parametrize("N", lc.SIZES)
def test_no_undefined_answers(oracle, N):
    """Raw and smoothed output finite and raw f0 > 0 (no lag -1: the reference would index out of bounds, HarmonicCharacteristics.h:205)
    for every kept channel; everything below full scale is kept; what is dropped is loud and really is not finite."""
    kept = lc.labels(N)
    for b in lc.BASES:
        for e in lc.NORMAL + lc.BAND + lc.BELOW + lc.SUBNORMAL:
            assert (b, e) in kept, (b, e)
    assert all(e in lc.LOUD for _, e in lc.DROPPED[N])
    raw, sm = lc.oracle_run(oracle, N)
    for i, label in enumerate(kept):
        assert np.isfinite(raw[i]).all() and np.isfinite(sm[i]).all(), (N, lc.label_id(label))
        assert (raw[i, :, F0] > 0).all(), (N, lc.label_id(label))
    for b, e in lc.DROPPED[N]:
        out = oracle.push_hops(lc.scaled(lc.full_scale(N, b), e)[None], N)
        assert not (np.isfinite(out[0]).all() and np.isfinite(out[1]).all()), (N, b, e)
        assert (out[0][0, :, F0] > 0).all(), (N, b, e)                 # (never the out-of-bounds lag: only the flatness overflows)


@pytest.fixture(scope="module")
def flush_mode(tmp_path_factory):
    """fx_test_flush_mode (tests/cpp/flush_mode.cpp): flush-to-zero and denormals-are-zero for the calling thread"""
    if platform.machine() not in ("x86_64", "AMD64"):
        pytest.skip("MXCSR's flush bits: x86-64 only")
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    so = str(tmp_path_factory.mktemp("flush") / "libflush_mode.so")
    p = subprocess.run(["g++", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "flush_mode.cpp"), "-o", so], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lib = ctypes.CDLL(so)
    lib.fx_test_flush_mode.argtypes, lib.fx_test_flush_mode.restype = [ctypes.c_uint], ctypes.c_uint

    def flushed(fn, *args, **kwargs):
        lib.fx_test_flush_mode(1)
        try:
            return fn(*args, **kwargs)
        finally:
            assert lib.fx_test_flush_mode(0) == 1
    return flushed


@pytest.mark.parametrize("N", lc.SIZES)
def test_the_cases_can_tell_a_flushing_implementation(oracle, flush_mode, N):
    """A condition on the inputs, by the oracle alone: evaluated with subnormals flushed (operands and results), the e = -11 channel of
    every base signal answers another raw f0 in at least half of its frames (measured: at least 10 of 12), and no other slot moves.

    The all-subnormal channels (e = -39, -42) cannot differ from silence in any slot at gain 1, flushed or not: the RMS slot,
    log10(1 + 9 rms) in fp32, is exactly 0 below about 1e-8, and below the band every v = ac * ac * s is 0, so the lag is silence's
    (2: f0 = 4.8).  That is held here as it is.  They differ from silence -- in f0 -- under the gain that lifts them into the band
    (10^(-9 - e), a float): there an implementation that flushes subnormal samples on ingest answers silence's f0 and the oracle
    the signal's, and the flushed evaluation shows it.  tests/test_gpu_levels.py runs the kernels on both."""
    hops = lc.hops(N)
    raw = lc.oracle_run(oracle, N)[0]
    flushed = flush_mode(oracle.push_hops, hops, N)[0]
    others = [k for k in range(12) if k != F0]
    for b in lc.BASES:
        (i,) = lc.channels(N, b, -11.0)
        differ = int((raw[i, :, F0] != flushed[i, :, F0]).sum())
        print("N=%d %s@1e-11: raw f0 differs in %d of %d frames with subnormals flushed" % (N, b, differ, lc.T))
        assert differ >= lc.T // 2, (N, b, differ)
    assert same_bits(raw[:, :, others], flushed[:, :, others]).all()
    silence = oracle.push_hops(np.zeros((1, lc.T, N // 2), np.float32), N)[0][0]
    for b in lc.BASES:
        for e in (-39.0, -42.0):
            (i,) = lc.channels(N, b, e)
            assert np.abs(hops[i]).max() < np.finfo(np.float32).tiny and np.count_nonzero(hops[i]) > hops[i].size // 2
            assert same_bits(raw[i], silence).all()                                                  # gain 1: silence's slots
            gain = float(np.float32(10.0 ** (-9.0 - e)))
            lifted = oracle.push_hops(hops[i:i + 1], N, gain=gain)[0][0]
            differ = int((lifted[:, F0] != silence[:, F0]).sum())
            print("N=%d %s@1e%g under gain %g: raw f0 differs from silence's in %d of %d frames" % (N, b, e, gain, differ, lc.T))
            assert differ >= lc.T // 2, (N, b, e, differ)
            assert same_bits(flush_mode(oracle.push_hops, hops[i:i + 1], N, gain=gain)[0][0], silence).all()


@pytest.mark.parametrize("N", lc.SIZES)
def test_oracle_is_bit_identical_to_the_reference_headers_at_every_level(oracle, N):
    """the reference's own headers (tools/refdiff, log10(float) correctly rounded) on the level cases: every raw and smoothed value"""
    raw, sm = refdiff.run(np.ascontiguousarray(lc.hops(N)), N, mode="cr")
    oraw, osm = lc.oracle_run(oracle, N)
    assert same_bits(raw, oraw).all(), "raw differs at %s" % (np.argwhere(~same_bits(raw, oraw))[:5],)
    assert same_bits(sm, osm).all(), "smoothed differs at %s" % (np.argwhere(~same_bits(sm, osm))[:5],)


@pytest.mark.parametrize("N", lc.SIZES)
def test_gain_reaches_the_same_place(oracle, N):
    """full-scale samples under gain 10^e (a float) equal the samples scaled beforehand under gain 1, bit for bit: the overlapper's
    product (RealTimeAnalyser.h) is the same single fp32 multiplication"""
    for b in lc.BASES:
        full = lc.full_scale(N, b)[None]
        for e in GAIN_LEVELS:
            (i,) = lc.channels(N, b, e)
            got = oracle.push_hops(full, N, gain=float(np.float32(10.0 ** e)))
            want = lc.oracle_run(oracle, N)
            for k in (0, 1):
                assert same_bits(got[k][0], want[k][i]).all(), (N, b, e, ("raw", "smoothed")[k])


def test_lag_search_regimes_of_the_1024_point_case(oracle):
    """The 1024-point kernel takes the cnd 64 samples at a time and fetches blocks 2 and 3, and then the rest past sample 255, only if
    the search gets there: the level case holds frames decided in each of those parts, band-level frames among them.

    The global-minimum fallback (no cnd below 0.01 in [2, N)) is not among them and no band-level channel of the low tones supplies it
    at 1024 points (every channel of low_tones at 8 to 24 channels and every signal of tests/signals.py was tried at full scale and at
    every band level): with a smooth autocorrelation cnd[s] is about 2 / s, below the threshold from s = 200 on, so only a 256-point
    window can end there.  The 256-point case does, and the fallback's code (LagSearch::finish) is the same at every size.
    (tests/golden/make_lag_cases.py looked again, over four families of synthetic frames and short decaying bursts: still no fallback at
    512 points or more -- lag_cases.UNREACHED says so per size.)

    These regimes are the coarse view.  The seams between them -- `first` and `stop` on lanes 62, 63, 0 and 1 of every 64-sample block
    up to block 7, samples 126-129 and 254-257 on both sides, the walk to N-1 that is decided against cnd[N] -- are held by the frames
    of tests/lag_cases.py (tests/test_lag_cases_cpu.py, tests/test_gpu_lag_cases.py); lag_regime shares its classification."""
    def regimes(N, chans):
        hops = lc.hops(N)
        return {(i, t): lc.lag_regime(oracle, w) for i in chans for t, w in enumerate(lc.windows(hops[i]))}

    band = [i for e in lc.BAND for i in lc.channels(1024, None, e)]
    at_1024 = regimes(1024, range(len(lc.labels(1024))))
    for r in lc.LAG_REGIMES[:3]:
        where = [k for k, v in at_1024.items() if v == r]
        print("N=1024 %s: %d frames, %d of them at band level" % (r, len(where), sum(i in band for i, _ in where)))
        assert where and any(i in band for i, _ in where), r
    assert "fallback" not in at_1024.values()
    at_256 = regimes(256, range(len(lc.labels(256))))
    where = [k for k, v in at_256.items() if v == "fallback"]
    print("N=256 fallback: %d frames" % len(where))
    assert where
