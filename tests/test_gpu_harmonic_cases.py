"""Every implementation of part 2 of the harmonic analyser on the frames of tests/harmonic_cases.py: peaks tied exactly with a neighbour
that lies in another lane (and, in the pair kernel, in the other wavefront), flat spectra where the last bit of the reference's serial sum
makes every bin a peak or none, the gate, the clipped windows of the first and last bins, probes exactly on bin edges, on bins 0 and 1 and
at and past bin M, both clamps, and every skip of the inharmonicity loop over peak lists of up to 3M/4 entries
(tests/test_harmonic_cases_cpu.py holds, by the oracle alone, that the frames are of these classes and tell every single-decision mutant
of the model apart).  HER, OER and inharmonicity are exact slots: a failure names the frame's classes.  The bar is the suite's: onset and
f0 exact, every other slot within its ulp budget, raw and smoothed.  Where a test forces a path it asserts the launches too.

The frames go in as frames (fx_process_frames, twelve per channel, in one call and one frame per call), as hops (channel c streams both
halves of its frames one after the other: every second window is a chosen frame and the junctions between two are compared as well) and
as one stream of samples cut into blocks.  All tests here need a real MI355X."""
import numpy as np
import pytest

import harmonic_cases as hc
import path_runs

pytestmark = pytest.mark.gpu

RATE = 48000.0
HOOK_FRAME_TAIL = 8                             # csrc/fx_kernels.h, bit 3: one-frame calls always finish the tail in the frame kernel
SPLIT = (1024, 2048, 4096)                      # the sizes with a hop kernel and a one-launch form

_WANT = {}


def want_frames(oracle, N, rate=RATE, **settings):
    """the oracle on the batch layout, computed once per (size, rate, settings) and shared (read-only)"""
    key = ("frames", N, rate, tuple(sorted(settings.items())))
    if key not in _WANT:
        _WANT[key] = oracle.process_frames(hc.batch_layout(N)[0], N, rate, **settings)
        for a in _WANT[key]:
            a.setflags(write=False)
    return _WANT[key]


def want_hops(oracle, N, only_s16=False):
    if ("hops", N, only_s16) not in _WANT:
        _WANT["hops", N, only_s16] = oracle.push_hops(hc.hop_layout(N, only_s16)[0], N)
        for a in _WANT["hops", N, only_s16]:
            a.setflags(write=False)
    return _WANT["hops", N, only_s16]


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
@pytest.mark.parametrize("N", hc.SIZES)
def test_batch_kernel(gpu_fx, oracle, N):
    B, _ = hc.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE)
    got = an.process_frames(B)
    assert kinds(an) == ["frame", "epilogue"]
    an.close()
    hc.assert_held(oracle, got, want_frames(oracle, N), B, "default", "batch N=%d" % N)


@pytest.mark.parametrize("N", [1024, 4096])
def test_batch_kernel_at_44100(gpu_fx, oracle, N):
    """nyquist / M is exact at this rate too and its reciprocal is not: the probes' bins and the ratios of the inharmonicity loop.
    At 4096 points the windowed spectrum of frame 4, ('sp', ((0, -999), (1024, -333), (3072, -333), (2048, -666))), has period 4 and
    an exact centroid of 11019.61669921875 Hz, exactly half way between two floats: the reference's serial sums
    (SpectralCharacteristics.h:86, :95) end just below it, the moments just above, and the kernel has to follow the reference."""
    B, _ = hc.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, 44100.0)
    got = an.process_frames(B)
    assert kinds(an) == ["frame", "epilogue"]
    an.close()
    hc.assert_held(oracle, got, want_frames(oracle, N, 44100.0), B, "default", "batch N=%d at 44.1 kHz" % N, rate=44100.0)


@pytest.mark.parametrize("N", hc.SIZES)
def test_harmonic_only_kernel(gpu_fx, oracle, N):
    B, _ = hc.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE, analysers="harmonic")
    got = an.process_frames(B)
    assert [(l["kind"], l["analysers"]) for l in an.last_launches()] == [("frame", 2), ("epilogue", 2)]
    an.close()
    hc.assert_held(oracle, got, want_frames(oracle, N, analysers=2), B, "default", "harmonic N=%d" % N)


@pytest.mark.parametrize("shape", [(3, 2), (2, 4)])
def test_1024_point_workgroup_shapes(gpu_fx, oracle, monkeypatch, shape):
    """other channels per workgroup x waves per channel: the batch form takes the neighbours of a lane's first and last bins by the
    per-lane images it keeps across frames, the same kernel's other forms by the bins image; both shapes are launched as asked"""
    N = 1024
    B, _ = hc.batch_layout(N)
    want = want_frames(oracle, N)
    again = np.arange(max(B.shape[0], shape[0])) % B.shape[0]                  # (a workgroup holds no more channels than the call has:
    B, want = np.ascontiguousarray(B[again]), tuple(w[again] for w in want)    # the first channels once more, channels are independent)
    monkeypatch.setenv("FX_CHANNELS_PER_WG", str(shape[0]))
    monkeypatch.setenv("FX_WAVES", str(shape[1]))
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE)
    got = an.process_frames(B)
    rec = an.last_launches()
    an.close()
    assert [l["kind"] for l in rec] == ["frame", "epilogue"] and (rec[0]["ch_per_wg"], rec[0]["waves_per_ch"]) == shape, rec
    hc.assert_held(oracle, got, want, B, "default", "batch N=1024, %d channels x %d waves per workgroup" % shape)


# ---- as hops ----
@pytest.mark.parametrize("N", hc.SIZES)
@pytest.mark.parametrize("fmt", ["f32", "s16"])
def test_hop_streams(gpu_fx, oracle, fmt, N):
    """every second window is a chosen frame, the others are junctions of two; in s16 the frames that are exact in that format"""
    H, _ = hc.hop_layout(N, fmt == "s16")
    an = gpu_fx.BatchAnalyser(H.shape[0], N, RATE)
    got = an.push_hops(hc.as_s16(H) if fmt == "s16" else H)
    assert kinds(an) == ["frame", "epilogue"]
    an.close()
    hc.assert_held(oracle, got, want_hops(oracle, N, fmt == "s16"), hc.hop_windows(H), "default", "%s hops N=%d" % (fmt, N))


def test_push_samples_in_blocks_of_several_hops(gpu_fx, oracle):
    """one stream of samples cut every 2000 samples: every call holds three or four hops of 512 and is one launch of the block-fed
    batch form, which reads its windows from [pending | block]"""
    N = 1024
    H, _ = hc.hop_layout(N)
    flat = H.reshape(H.shape[0], -1)
    an = gpu_fx.BatchAnalyser(H.shape[0], N, RATE)
    parts = []
    try:
        for at in range(0, flat.shape[1], 2000):
            parts.append(an.push_samples(np.ascontiguousarray(flat[:, at:at + 2000])))
            f = parts[-1][0].shape[1]
            if f > 2:
                assert [(l["kind"], l["block_mode"], l["T"]) for l in an.last_launches()] == [("frame", 1, f), ("epilogue", 0, 0)], (at, an.last_launches())
        assert an.pending_samples() == 0 and sum(p[0].shape[1] > 2 for p in parts) >= 6
    finally:
        an.close()
    got = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
    hc.assert_held(oracle, got, want_hops(oracle, N), hc.hop_windows(H), "default", "push_samples N=1024, blocks of 2000 samples")


# ---- one frame per call ----
ONE_FRAME = [("direct", 256), ("direct", 512)] + [(p, N) for N in SPLIT for p in ("hop", "frame_tail", "direct")]


@pytest.mark.parametrize("path,N", ONE_FRAME, ids=["%s-%d" % p for p in ONE_FRAME])
def test_one_frame_per_call(gpu_fx, oracle, path, N):
    B, _ = hc.batch_layout(N)
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
    hc.assert_held(oracle, got, want_frames(oracle, N), B, "default", "%s N=%d, one frame per call" % (path, N))


ONE_FRAME_44100 = [(e, p) for e in ("frames", "samples") for p in ("frame_tail", "direct")]


@pytest.mark.parametrize("entry,path", ONE_FRAME_44100, ids=["%s-%s" % q for q in ONE_FRAME_44100])
def test_one_frame_per_call_at_44100_and_4096_points(gpu_fx, oracle, entry, path):
    """the frame whose centroid lies half way between two floats (test_batch_kernel_at_44100) through the one-frame forms of the
    4096-point kernels, which redo the reference's serial sums with their registers full: as frames, and as samples one hop per call,
    where the block-fed forms read the window from [pending | block]"""
    N, rate = 4096, 44100.0
    expect = {"frame_tail": ["frame_tail"], "direct": ["frame", "epilogue"]}[path]
    B, _ = hc.batch_layout(N)
    H, _ = hc.hop_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, rate)
    an.set_tuning(one_hop_kernel=0)
    an.set_test_hooks(path_runs.HOOK_TAIL_NEVER_FUSED if path == "direct" else HOOK_FRAME_TAIL)
    try:
        if entry == "frames":
            got = frame_by_frame(an, B, expect)
            want, windows = want_frames(oracle, N, rate), B
        else:
            parts, flat, at = [], H.reshape(H.shape[0], -1), 0
            for n in [100] + [N // 2] * (H.shape[1] - 1) + [N // 2 - 100]:         # (100 samples pending: every later call completes one hop)
                parts.append(an.push_samples(np.ascontiguousarray(flat[:, at:at + n])))
                at += n
                rec = an.last_launches()
                assert parts[-1][0].shape[1] == (at > 100), (at, parts[-1][0].shape)
                assert at == 100 or ([l["kind"] for l in rec] == expect and rec[0]["block_mode"] == 1), (at, rec)
            assert an.pending_samples() == 0
            got = tuple(np.concatenate([q[k] for q in parts], axis=1) for k in (0, 1))
            if ("hops", N, rate) not in _WANT:
                _WANT["hops", N, rate] = oracle.push_hops(H, N, rate)
            want, windows = _WANT["hops", N, rate], hc.hop_windows(H)
    finally:
        an.close()
    hc.assert_held(oracle, got, want, windows, "default", "%s N=4096 at 44.1 kHz, one %s per call" % (path, entry[:-1]), rate=rate)


# ---- the low-latency family: a frame on a pair of wavefronts, the peak list and the serial sum handed from wave to wave ----
@pytest.mark.parametrize("N", hc.PAIR_SIZES)
def test_pair_kernel(gpu_fx, oracle, N):
    B, _ = hc.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, RATE, low_latency=True)
    got = an.process_frames(B)
    assert kinds(an) == ["pair", "epilogue"]
    an.close()
    hc.assert_held(oracle, got, want_frames(oracle, N), B, "low_latency", "pair N=%d" % N)


def test_pair_kernel_at_44100(gpu_fx, oracle):
    """the period-4 frames whose centroid lies exactly half way between two floats at this rate (test_batch_kernel_at_44100), where
    the pair's two wavefronts hand the reference's serial sums from one to the other"""
    N = 4096
    B, _ = hc.batch_layout(N)
    an = gpu_fx.BatchAnalyser(B.shape[0], N, 44100.0, low_latency=True)
    got = an.process_frames(B)
    assert kinds(an) == ["pair", "epilogue"]
    an.close()
    hc.assert_held(oracle, got, want_frames(oracle, N, 44100.0), B, "low_latency", "pair N=%d at 44.1 kHz" % N, rate=44100.0)


@pytest.mark.parametrize("N", hc.PAIR_SIZES)
def test_hop_pair_kernel(gpu_fx, oracle, N):
    H, _ = hc.hop_layout(N)
    got = path_runs.run_path(gpu_fx, "hop_pair", N, RATE, H, fused_calls=())
    hc.assert_held(oracle, got, want_hops(oracle, N), hc.hop_windows(H), "low_latency", "hop_pair N=%d, one hop per call" % N)
