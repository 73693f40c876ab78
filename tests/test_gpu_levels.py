"""Every kernel family from full scale down to subnormal samples, and through the band (1e-9 .. 1e-13 of full scale) where the raw F0 slot
rests on IEEE gradual underflow (tests/level_cases.py; the CPU side -- the oracle's answer is defined there, the inputs can tell an
implementation that flushes subnormals, the oracle equals the reference's headers -- is tests/test_levels_cpu.py).  The bar is the
suite's: onset and f0 exact, every other slot within its ulp budget (oracle/ulp.py), every path the batch path's bits.  All tests here
need a real MI355X.

With FX_LEVELS_ULP_OUT set to a file name, the largest ulp distance seen per family, level and slot is written there when the module is
done (the record profiles/levels_ulp.txt was made that way)."""
import os

import numpy as np
import pytest

import level_cases as lc
import path_runs
import signals
import taps_model
from rate_cases import same_bits
from test_gpu_rates import PATHS

pytestmark = pytest.mark.gpu

RATE = 48000.0
FUSED_CALLS = ((0, 5), (5, 8), (8, 12))         # the fused tail's frame-per-lane form: calls of 5, 3 and 4 frames
GAIN_LEVELS = (-9.0, -11.0, -13.0)
ULP_SEEN = {}                                   # (family, level) -> largest distance per slot


@pytest.fixture(scope="module", autouse=True)
def _ulp_record():
    yield
    path = os.environ.get("FX_LEVELS_ULP_OUT")
    if path and ULP_SEEN:
        with open(path, "w") as f:
            f.write("largest fp32 ulp distance from the oracle, raw and smoothed, over the level cases and every path of tests/test_gpu_levels.py\n")
            f.write("%-12s %-10s %s\n" % ("family", "level", " ".join("%-8s" % s for s in signals.SLOTS)))
            for (family, _, level), d in sorted(ULP_SEEN.items()):
                f.write("%-12s %-10s %s\n" % (family, level, " ".join("%-8d" % v for v in d)))


def _level_key(label):
    """(sort key, name) of a channel's level: the scaled levels from loud to quiet, then the fades and the other inputs"""
    kind, e = label
    return (0, -e, "1e%g" % e) if e is not None else (1, 0.0, kind)


def close(got, want, family, labels, what):
    """both vectors [C][T][12] within the family's budget; the maxima per level (labels: one (kind, e) per channel) are kept for the record"""
    from oracle import fx_oracle as fo
    for k, name in ((0, "raw"), (1, "smoothed")):
        signals.assert_features_within(got[k], want[k], signals.ulp_budget(family), fo.FEATURE_NAMES, "%s %s" % (what, name))
        d = signals.ulp_distance(np.asarray(got[k], np.float32).reshape(-1, 12), np.asarray(want[k], np.float32).reshape(-1, 12))
        d = d.reshape(len(labels), -1, 12).max(axis=1)
        for i, label in enumerate(labels):
            a, b, level = _level_key(label)
            key = (family, (a, b), level)
            ULP_SEEN[key] = np.maximum(ULP_SEEN.get(key, np.zeros(12, np.int64)), d[i])


def same(got, want, what):
    for k in (0, 1):
        assert np.array_equal(got[k], want[k], equal_nan=True), "%s: %s differs at %s" % (what, ("raw", "smoothed")[k], np.argwhere(~same_bits(got[k], want[k]))[:5])


def run_path(gpu_fx, path, N):
    return path_runs.run_path(gpu_fx, path, N, RATE, lc.hops(N), fused_calls=FUSED_CALLS)


_BATCH = {}


def batch(gpu_fx, N, low=False):
    """the batch path's result on the size's case, computed once per (size, family) and shared"""
    if (N, low) not in _BATCH:
        _BATCH[N, low] = run_path(gpu_fx, "pair" if low else "batch", N)
    return _BATCH[N, low]


# ---- parity of the batch kernels, every size ----
@pytest.mark.parametrize("N", lc.SIZES)
def test_batch_frame_kernel_matches_oracle(gpu_fx, oracle, N):
    close(batch(gpu_fx, N), lc.oracle_run(oracle, N), "default", lc.labels(N), "batch N=%d" % N)


@pytest.mark.parametrize("N", [2048, 4096])
def test_pair_kernel_matches_oracle(gpu_fx, oracle, N):
    got = batch(gpu_fx, N, low=True)
    close(got, lc.oracle_run(oracle, N), "low_latency", lc.labels(N), "pair N=%d" % N)
    ref = batch(gpu_fx, N)
    for k in (0, 1):                                              # the discrete decisions are the default family's
        assert np.array_equal(got[k][:, :, [0, 2]], ref[k][:, :, [0, 2]], equal_nan=True)


# ---- every other path: the oracle's values within the budget, and the batch path's bits ----
@pytest.mark.parametrize("path,N", PATHS, ids=["%s-%d" % p for p in PATHS])
def test_every_path_matches_oracle_and_equals_the_batch_path_bitwise(gpu_fx, oracle, path, N):
    low = path in ("hop_pair", "ring_hop_pair")
    got = run_path(gpu_fx, path, N)
    close(got, lc.oracle_run(oracle, N), "low_latency" if low else "default", lc.labels(N), "%s N=%d" % (path, N))
    same(got, batch(gpu_fx, N, low), "%s N=%d against the batch path" % (path, N))


@pytest.mark.parametrize("which,mask,N", [("harmonic", 2, 2048), ("spectral", 1, 512)])
def test_single_analyser_modes(gpu_fx, oracle, which, mask, N):
    hops = lc.hops(N)
    an = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, analysers=which)
    whole = an.push_hops(hops)
    close(whole, lc.oracle_run(oracle, N, analysers=mask), "default", lc.labels(N), "%s N=%d" % (which, N))
    one = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, analysers=which)
    same(path_runs._calls(one, hops, 1, ("frame", "epilogue")), whole, "%s N=%d one frame per call" % (which, N))
    if which == "harmonic":                                       # the harmonic slots are those of the full bundle
        assert np.array_equal(whole[0][:, :, [2, 9, 10, 11]], batch(gpu_fx, N)[0][:, :, [2, 9, 10, 11]], equal_nan=True)
    an.close(); one.close()


# ---- the 1024-point kernel's lazily fetched lag blocks ----
def test_1024_point_lag_blocks_in_every_regime(gpu_fx, oracle):
    """The 1024-point kernel fetches lag blocks 2 and 3, and then the rest past sample 255, only if the search gets there.  By the
    oracle's own cnd the band-level channels hold frames decided in each of those parts (this test stops if they no longer do), and the
    raw F0 of every such frame is the oracle's bit for bit on the batch path and on the one-hop kernel."""
    N = 1024
    hops = lc.hops(N)
    band = [i for e in lc.BAND for i in lc.channels(N, None, e)]
    regime = {(i, t): lc.lag_regime(oracle, w) for i in band for t, w in enumerate(lc.windows(hops[i]))}
    want = lc.oracle_run(oracle, N)[0]
    for got in (batch(gpu_fx, N)[0], run_path(gpu_fx, "hop", N)[0]):
        for r in lc.LAG_REGIMES[:3]:
            where = [k for k, v in regime.items() if v == r]
            assert where, "no band-level frame of the 1024-point case is decided in %s any more" % r
            bad = [k for k in where if not same_bits(got[k][2], want[k][2])]
            assert not bad, "%s: raw f0 differs at (channel, frame) %s" % (r, bad[:5])


# ---- gain: full-scale samples of every format lowered into the band by the context's gain and by the per-track table ----
def _as_format(gpu_fx, x, fmt):
    """x [..][n] float32 at full scale -> (what the analyser is fed, the floats it stands for)"""
    if fmt == "f32":
        return x, x
    if fmt == "f16":
        h = x.astype(np.float16)
        return h, h.astype(np.float32)
    if fmt == "s16":
        v = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        return v, v.astype(np.float32) / np.float32(32768.0)
    v = np.clip(np.round(x.astype(np.float64) * 8388608.0), -2 ** 23, 2 ** 23 - 1).astype(np.int32)
    return gpu_fx.pack_s24(v), v.astype(np.float32) / np.float32(8388608.0)


def _full_scale(N):
    """the three base signals at full scale, [3][12][N/2], brought under 1 so that the PCM formats hold them"""
    x = np.stack([lc.full_scale(N, b) for b in lc.BASES])
    return (x / np.float32(max(1.0, np.abs(x).max() * 1.001))).astype(np.float32)


@pytest.mark.parametrize("N", lc.SIZES)
@pytest.mark.parametrize("fmt", ["f32", "f16", "s16", "s24"])
def test_gain_routes_reach_the_band(gpu_fx, oracle, fmt, N):
    base = _full_scale(N)
    B, H, per = len(lc.BASES), N // 2, 3 if fmt == "s24" else 1
    fed, floats = _as_format(gpu_fx, base, fmt)
    gains = [float(np.float32(10.0 ** e)) for e in GAIN_LEVELS]
    want = {e: oracle.push_hops(floats, N, gain=g) for e, g in zip(GAIN_LEVELS, gains)}
    # route 1: the context's gain, whole hops and 480-sample blocks
    for e, g in zip(GAIN_LEVELS, gains):
        level = [(b, e) for b in lc.BASES]
        an = gpu_fx.BatchAnalyser(B, N, RATE)
        an.set_gain(g)
        whole = an.push_hops(fed, sample_format=fmt)
        close(whole, want[e], "default", level, "context gain 1e%g, %s N=%d, push_hops" % (e, fmt, N))
        an.close()
        an = gpu_fx.BatchAnalyser(B, N, RATE)
        an.set_gain(g)
        flat = np.asarray(fed).reshape(B, -1)
        parts = [an.push_samples(np.ascontiguousarray(flat[:, at:at + 480 * per]), sample_format=fmt) for at in range(0, flat.shape[1], 480 * per)]
        blocks = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
        assert blocks[0].shape[1] == lc.T and an.pending_samples() == 0
        close(blocks, want[e], "default", level, "context gain 1e%g, %s N=%d, push_samples" % (e, fmt, N))
        same(blocks, whole, "context gain 1e%g, %s N=%d: blocks against whole hops" % (e, fmt, N))
        an.close()
        if fmt == "f32":                                          # the samples scaled beforehand: the same bits (tests/test_levels_cpu.py)
            an = gpu_fx.BatchAnalyser(B, N, RATE)
            same(an.push_hops(lc.scaled(base, e)), whole, "f32 N=%d: scaled beforehand against gain 1e%g" % (N, e))
            an.close()
    # route 2: the per-track table, neighbouring tracks at different exponents
    tracks = [(b, e) for b in range(B) for e in GAIN_LEVELS]
    an = gpu_fx.BatchAnalyser(len(tracks), N, RATE)
    an.set_channel_gains([np.float32(10.0 ** e) for _, e in tracks])
    got = an.push_hops(np.ascontiguousarray(np.asarray(fed)[[b for b, _ in tracks]]), sample_format=fmt)
    an.close()
    expect = tuple(np.stack([want[e][k][b] for b, e in tracks]) for k in (0, 1))
    close(got, expect, "default", [(lc.BASES[b], e) for b, e in tracks], "per-track gains, %s N=%d" % (fmt, N))


@pytest.mark.parametrize("N", lc.SIZES)
def test_subnormal_samples_lifted_into_the_band_by_gain(gpu_fx, oracle, N):
    """The all-subnormal channels (e = -39, -42) equal silence in every slot at gain 1; under the per-track gain that lifts them to 1e-9
    the oracle answers the signal's f0, and a kernel that flushed subnormal samples on ingest would answer silence's."""
    pairs = [(b, e) for b in lc.BASES for e in (-39.0, -42.0)]
    hops = np.ascontiguousarray(lc.hops(N)[[lc.channels(N, b, e)[0] for b, e in pairs]])
    gains = [np.float32(10.0 ** (-9.0 - e)) for _, e in pairs]
    an = gpu_fx.BatchAnalyser(len(pairs), N, RATE)
    an.set_channel_gains(gains)
    got = an.push_hops(hops)
    an.close()
    want = [oracle.push_hops(hops[i:i + 1], N, gain=float(g)) for i, g in enumerate(gains)]
    want = tuple(np.concatenate([w[k] for w in want]) for k in (0, 1))
    close(got, want, "default", [("lifted", e) for _, e in pairs], "subnormal samples under gain, N=%d" % N)


# ---- fp16 ingest of subnormal halves ----
def _windows(hops):
    C, T, H = hops.shape
    x = np.concatenate([np.zeros((C, 1, H), hops.dtype), hops], axis=1)
    return np.ascontiguousarray(np.concatenate([x[:, :-1], x[:, 1:]], axis=2))


@pytest.mark.parametrize("N", [512, 1024, 2048, 4096])
def test_fp16_subnormal_halves(gpu_fx, oracle, N):
    """tone and noise whose halves lie between 6e-8 and 6e-5, mostly subnormal: against the oracle on the decoded floats, through push_hops
    and process_frames (512, 1024, 4096 points) and through a ring of fp16 slots (2048 points)"""
    halves = lc.f16_subnormal(N)
    C = halves.shape[0]
    want = oracle.push_hops(halves.astype(np.float32), N)
    labels = [("f16 %g" % p, None) for p in lc.F16_SUBNORMAL_PEAKS]
    an = gpu_fx.BatchAnalyser(C, N, RATE)
    if N == 2048:
        st = gpu_fx.HopStream(an, 1, slots=3, dtype=np.float16)
        got = []
        for t in range(lc.T):
            if st.in_flight() == 2:
                got.append(st.collect())
            st.push(halves[:, t:t + 1])
        while st.in_flight():
            got.append(st.collect())
        st.close()
        close(tuple(np.concatenate([g[k] for g in got], axis=1) for k in (0, 1)), want, "default", labels, "fp16 ring N=%d" % N)
    else:
        whole = an.push_hops(halves)
        close(whole, want, "default", labels, "fp16 push_hops N=%d" % N)
        frames = gpu_fx.BatchAnalyser(C, N, RATE)
        same(frames.process_frames(_windows(halves)), whole, "fp16 process_frames N=%d against push_hops" % N)
        frames.close()
    an.close()


# ---- taps: one armed band-level channel, so that a mismatch can be traced to a stage ----
@pytest.mark.parametrize("N,low", [(1024, False), (2048, True)])
def test_taps_of_a_band_level_channel(gpu_fx, oracle, N, low):
    hops = lc.hops(N)
    (c,) = lc.channels(N, "tone", -11.0)
    an = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, low_latency=low)
    an.push_hops(hops[:, :2])
    an.request_taps([c])
    an.push_hops(hops[:, 2:3])
    assert an.last_launches()[0]["kind"] == "taps"
    got = an.taps(c)
    an.close()
    assert got["frame_index"] == 2
    taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, np.concatenate([hops[c, 1], hops[c, 2]])), "N=%d tone@1e-11" % N)
