"""Every implementation of the pitch lag search on the frames of tests/lag_cases.py: `first` and `stop` on lanes 62, 63, 0 and 1 of the
kernels' 64-sample blocks, on both sides of the 1024-point kernel's stage seams (samples 126-129 and 254-257), the walk to sample N-1
that is decided against cnd[N], the walk that does not move, the fallback (tests/test_lag_cases_cpu.py holds, by the oracle alone, that
the frames are of these classes).  Raw f0 is an exact slot and f0 = sample_rate / lag, so a wrong hand-over between two blocks shows as
another f0: a failure names the frame's class, `first`, `stop`, and the oracle's and the kernel's lag.  The bar is the suite's: onset
and f0 exact, every other slot within its ulp budget, raw and smoothed.  Where a test forces a path it asserts the launches too.

The frames go in as frames (fx_process_frames, twelve per channel, in one call and one frame per call) and as hops (channel c streams
both halves of its frames one after the other: every second window is a chosen frame and the junctions between two are compared as
well).  All tests here need a real MI355X."""
import numpy as np
import pytest

import lag_cases as lg
import path_runs
import taps_model
from rate_cases import same_bits

pytestmark = pytest.mark.gpu

RATE = 48000.0
F0 = 2
SPLIT = (1024, 2048, 4096)                      # the sizes with a hop kernel and a one-launch form
MAX_TAPS = 64

_WANT = {}


def want_frames(oracle, N, **settings):
    """the oracle on the batch layout, computed once per (size, settings) and shared (read-only)"""
    key = ("frames", N, tuple(sorted(settings.items())))
    if key not in _WANT:
        _WANT[key] = oracle.process_frames(lg.batch_layout(N)[0], N, **settings)
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def want_hops(oracle, N):
    if ("hops", N) not in _WANT:
        _WANT["hops", N] = oracle.push_hops(lg.hop_layout(N)[0], N)
        for a in _WANT["hops", N]:
            a.setflags(write=False)
    return _WANT["hops", N]


def kinds(an):
    return [l["kind"] for l in an.last_launches()]


def frame_by_frame(an, B, expect):
    """fx_process_frames one frame per call, every call's launches `expect`"""
    outs = []
    for t in range(B.shape[1]):
        outs.append(an.process_frames(np.ascontiguousarray(B[:, t:t + 1])))
        assert kinds(an) == list(expect), (t, an.last_launches())
    return tuple(np.concatenate([o[k] for o in outs], axis=1) for k in (0, 1))


# ---- as frames, twelve per channel: the batch kernels ----
@pytest.mark.parametrize("N", lg.SIZES)
def test_batch_kernel(gpu_fx, oracle, N):
    B, _ = lg.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE)
    got = an.process_frames(B)
    assert kinds(an) == ["frame", "epilogue"]
    an.close()
    lg.assert_held(oracle, got, want_frames(oracle, N), B, "default", "batch N=%d" % N)


@pytest.mark.parametrize("N", lg.SIZES)
def test_harmonic_only_kernel(gpu_fx, oracle, N):
    B, _ = lg.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE, analysers="harmonic")
    got = an.process_frames(B)
    assert [(l["kind"], l["analysers"]) for l in an.last_launches()] == [("frame", 2), ("epilogue", 2)]
    an.close()
    lg.assert_held(oracle, got, want_frames(oracle, N, analysers=2), B, "default", "harmonic N=%d" % N)


@pytest.mark.parametrize("shape,planned", [((3, 2), (3, 2)), ((2, 8), (1, 8)), ((2, 4), (2, 4))])
def test_1024_point_workgroup_shapes(gpu_fx, oracle, monkeypatch, shape, planned):
    """other channels per workgroup x waves per channel (tests/test_gpu_parity.py, test_workgroup_shapes_give_the_same_bits): the
    buffers the search's later blocks are read from sit at other LDS offsets.  (A call of twelve frames keeps a workgroup within eight
    wavefronts, so that test's 2 x 8 is planned as 1 x 8 here; 2 x 4 is the shape of two channels that is launched as asked.)"""
    N = 1024
    B, _ = lg.batch_layout(N)
    monkeypatch.setenv("FX_CHANNELS_PER_WG", str(shape[0]))
    monkeypatch.setenv("FX_WAVES", str(shape[1]))
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE)
    got = an.process_frames(B)
    rec = an.last_launches()
    an.close()
    assert [l["kind"] for l in rec] == ["frame", "epilogue"] and (rec[0]["ch_per_wg"], rec[0]["waves_per_ch"]) == planned, rec
    lg.assert_held(oracle, got, want_frames(oracle, N), B, "default", "batch N=1024, %d channels x %d waves per workgroup" % shape)


# ---- as hops ----
@pytest.mark.parametrize("N", lg.SIZES)
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_hop_streams(gpu_fx, oracle, fmt, N):
    """every second window is a chosen frame, the others are junctions of two; the s16 samples are the same numbers exactly"""
    H, _ = lg.hop_layout(N)
    an = gpu_fx.BatchAnalyser(H.shape[0], N, RATE)
    got = an.push_hops(lg.as_s16(H) if fmt == "s16" else H)
    assert kinds(an) == ["frame", "epilogue"]
    an.close()
    lg.assert_held(oracle, got, want_hops(oracle, N), lg.hop_windows(H), "default", "%s hops N=%d" % (fmt, N))


# ---- one frame per call ----
ONE_FRAME = [("direct", 256), ("direct", 512)] + [(p, N) for N in SPLIT for p in ("hop", "frame_tail", "direct")]


@pytest.mark.parametrize("path,N", ONE_FRAME, ids=["%s-%d" % p for p in ONE_FRAME])
def test_one_frame_per_call(gpu_fx, oracle, path, N):
    B, _ = lg.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE)
    if path != "hop" and N >= 1024:
        an.set_tuning(one_hop_kernel=0)
    if path == "direct" and N >= 1024:
        an.set_test_hooks(path_runs.HOOK_TAIL_NEVER_FUSED)
    expect = {"hop": ("hop",), "frame_tail": ("frame_tail",), "direct": ("frame", "epilogue")}[path]
    try:
        got = frame_by_frame(an, B, expect)
        if path == "direct":
            assert an.last_launches()[0]["direct_state"] == 1
    finally:
        an.close()
    lg.assert_held(oracle, got, want_frames(oracle, N), B, "default", "%s N=%d, one frame per call" % (path, N))


# ---- the low-latency family: a frame on a pair of wavefronts, the search over LDS ----
@pytest.mark.parametrize("N", [2048, 4096])
def test_pair_kernel(gpu_fx, oracle, N):
    B, _ = lg.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE, low_latency=True)
    got = an.process_frames(B)
    assert kinds(an) == ["pair", "epilogue"]
    an.close()
    lg.assert_held(oracle, got, want_frames(oracle, N), B, "low_latency", "pair N=%d" % N)


@pytest.mark.parametrize("N", [2048, 4096])
def test_hop_pair_kernel(gpu_fx, oracle, N):
    H, _ = lg.hop_layout(N)
    got = path_runs.run_path(gpu_fx, "hop_pair", N, RATE, H, fused_calls=())
    lg.assert_held(oracle, got, want_hops(oracle, N), lg.hop_windows(H), "low_latency", "hop_pair N=%d, one hop per call" % N)


# ---- taps: the cnd the search walked, and where it ended ----
def spread(oracle, N):
    """up to MAX_TAPS of the chosen frames: the first frame of every class that is no cell, then the others at even steps through the
    table (which is ordered by block, roughly)"""
    cls = [lg.classes(N, *k) for k in lg.classified(oracle, N)]
    seen, pick = set(), []
    for i, c in enumerate(cls):
        new = {q for q in c if q[0] != "cell"} - seen
        if new:
            pick.append(i)
            seen |= new
    rest = [i for i in range(len(cls)) if i not in pick]
    room = max(0, min(MAX_TAPS - len(pick), len(rest)))
    pick += [rest[j] for j in sorted({int(round(q)) for q in np.linspace(0, len(rest) - 1, room)})] if room else []
    return sorted(pick)


@pytest.mark.parametrize("N,low", [(256, False), (1024, False), (2048, True), (4096, False)])
def test_taps_of_the_chosen_frames(gpu_fx, oracle, N, low):
    """fx_get_taps' cnd and lag position of the chosen frames, armed before the call that analyses them: the oracle's cnd[:N] and
    (lag / 2N, cnd[lag]) bit for bit, and the lag position gives the same call's raw f0"""
    B, where = lg.batch_layout(N)
    armed = {}
    for i in spread(oracle, N):
        armed.setdefault(where[i][1], []).append(i)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE, low_latency=low)
    try:
        for t in range(lg.T):
            if t in armed:
                an.request_taps([where[i][0] for i in armed[t]])
            raw, _ = an.process_frames(np.ascontiguousarray(B[:, t:t + 1]))
            assert (kinds(an)[0] == "taps") == (t in armed)
            for i in armed.get(t, ()):
                c = where[i][0]
                kind, first, stop, lag = lg.classified(oracle, N)[i]
                what = "N=%d frame %d (%s)" % (N, i, lg.describe(N, kind, first, stop, lag))
                got = an.taps(c)
                assert got["frame_index"] == t, what
                taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, B[c, t]), what)
                x, y = got["lag_position"]
                if kind == "fallback":                                     # the display holds no lag then (PitchAnalyser.h:187)
                    assert x < 0, what
                    continue
                cnd = lg.oracle_cnd(oracle, B[c, t])[1]
                assert same_bits(np.float32(x), np.float32(lag) / np.float32(2 * N)) and same_bits(np.float32(y), cnd[lag]), (what, x, y)
                slot = np.float32(RATE / float(np.float32(x) * np.float32(2 * N)) / 5000.0)
                assert same_bits(slot, raw[c, 0, F0]), "%s: the taps say lag %d, the same call's f0 says %s" % (what, lag, lg.lag_of(raw[c, 0, F0]))
    finally:
        an.close()
