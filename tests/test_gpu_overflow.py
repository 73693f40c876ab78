"""Every kernel family on overflowing and non-finite samples (tests/overflow_cases.py: the ladder from 1e2 to 1e38 of full scale, the walks
through the overflow band, hops that hold NaN, inf and near-overflow samples; the CPU side -- the regimes exist, the oracle equals the
reference's headers wherever those define an answer -- is tests/test_overflow_cpu.py).  The bar is the suite's: onset and f0 exact, every
other slot within its ulp budget (oracle/ulp.py), applied through the mask of slot-frames the reference does not define (HER, OER and
inharmonicity of a frame whose raw f0 is not > 0: it reads out of bounds there); every path the batch path's bits on every slot-frame,
masked ones included.  All tests here need a real MI355X.

With FX_OVERFLOW_ULP_OUT set to a file name, the largest ulp distance seen per family, level and slot (defined slot-frames only) is written
there when the module is done (the record profiles/overflow_ulp.txt was made that way)."""
import os

import numpy as np
import pytest

import overflow_cases as oc
import path_runs
import signals
import taps_model
from test_gpu_rates import PATHS

pytestmark = pytest.mark.gpu

RATE = 48000.0
FUSED_CALLS = ((0, 8), (8, 16), (16, 21), (21, 24))
GAIN_LEVELS = (8.0, 9.5, 19.0, 36.0)
ULP_SEEN = {}                                   # (family, level) -> largest distance per slot


@pytest.fixture(scope="module", autouse=True)
def _ulp_record():
    yield
    path = os.environ.get("FX_OVERFLOW_ULP_OUT")
    if path and ULP_SEEN:
        with open(path, "w") as f:
            f.write("largest fp32 ulp distance from the oracle, raw and smoothed, over the overflow cases and every path of tests/test_gpu_overflow.py\n")
            f.write("(slot-frames the reference defines; HER, OER and inharmonicity of frames whose f0 is not > 0 are not compared)\n")
            f.write("%-12s %-22s %s\n" % ("family", "level", " ".join("%-8s" % s for s in signals.SLOTS)))
            for (family, _, level), d in sorted(ULP_SEEN.items()):
                f.write("%-12s %-22s %s\n" % (family, level, " ".join("%-8d" % v for v in d)))


def _level_key(label):
    """(sort key, name) of a channel's level: the ladder from quiet to loud, then the other kinds by name"""
    kind, e = label
    return (0, e, "1e%g" % e) if isinstance(e, float) else (1, 0.0, kind if e is None or kind.startswith("clean") else "%s %s" % (kind, e))


def close(got, want, family, labels, what, masked=True):
    """both vectors [C][T][12] within the family's budget wherever the reference defines an answer (masked=False: everywhere); the
    maxima per level (labels: one (kind, e) per channel) are kept for the record"""
    masks = oc.defined(want[0]) if masked else (None, None)
    for k, name in ((0, "raw"), (1, "smoothed")):
        oc.assert_within(got[k], want[k], signals.ulp_budget(family), masks[k], "%s %s" % (what, name))
        d = signals.ulp_distance(np.asarray(got[k], np.float32).reshape(-1, 12), np.asarray(want[k], np.float32).reshape(-1, 12))
        if masks[k] is not None:
            d = np.where(masks[k].reshape(-1, 12), d, 0)
        d = d.reshape(len(labels), -1, 12).max(axis=1)
        for i, label in enumerate(labels):
            a, b, level = _level_key(label)
            key = (family, (a, b), level)
            ULP_SEEN[key] = np.maximum(ULP_SEEN.get(key, np.zeros(12, np.int64)), d[i])


def same(got, want, what):
    """bit for bit on every slot-frame (a NaN is a NaN)"""
    for k in (0, 1):
        ok = oc_same_bits(got[k], want[k])
        assert ok.all(), "%s: %s differs at %s" % (what, ("raw", "smoothed")[k], np.argwhere(~ok)[:5])


def oc_same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


RING_HOP_BYTES = 1024 * 1024                     # csrc/fx_stream.cpp: the ring runs the one-hop kernels on up to 1 MiB of hops per call


def run_path(gpu_fx, path, N, hops=None):
    hops = oc.hops(N) if hops is None else hops
    per_ring = RING_HOP_BYTES // (4 * (N // 2))
    if path.startswith("ring") and hops.shape[0] > per_ring:      # more channels than one ring takes: two rings, half the channels each
        half = (hops.shape[0] + 1) // 2
        assert half <= per_ring
        parts = [path_runs.run_path(gpu_fx, path, N, RATE, np.ascontiguousarray(h), fused_calls=FUSED_CALLS) for h in (hops[:half], hops[half:])]
        return tuple(np.concatenate([p[k] for p in parts]) for k in (0, 1))
    return path_runs.run_path(gpu_fx, path, N, RATE, hops, fused_calls=FUSED_CALLS)


_BATCH = {}


def batch(gpu_fx, N, low=False):
    """the batch path's result on the size's case, computed once per (size, family) and shared"""
    if (N, low) not in _BATCH:
        _BATCH[N, low] = run_path(gpu_fx, "pair" if low else "batch", N)
    return _BATCH[N, low]


# ---- parity of the batch kernels, every size ----
@pytest.mark.parametrize("N", oc.SIZES)
def test_batch_frame_kernel_matches_oracle(gpu_fx, oracle, N):
    close(batch(gpu_fx, N), oc.oracle_run(oracle, N), "default", oc.labels(N), "batch N=%d" % N)


@pytest.mark.parametrize("N", [2048, 4096])
def test_pair_kernel_matches_oracle(gpu_fx, oracle, N):
    got = batch(gpu_fx, N, low=True)
    close(got, oc.oracle_run(oracle, N), "low_latency", oc.labels(N), "pair N=%d" % N)
    ref = batch(gpu_fx, N)
    for k in (0, 1):                                              # the discrete decisions are the default family's, on all frames
        assert oc_same_bits(got[k][:, :, [0, 2]], ref[k][:, :, [0, 2]]).all()


# ---- every other path: the oracle's values through the mask, and the batch path's bits everywhere ----
@pytest.mark.parametrize("path,N", PATHS, ids=["%s-%d" % p for p in PATHS])
def test_every_path_matches_oracle_and_equals_the_batch_path_bitwise(gpu_fx, oracle, path, N):
    low = path in ("hop_pair", "ring_hop_pair")
    got = run_path(gpu_fx, path, N)
    close(got, oc.oracle_run(oracle, N), "low_latency" if low else "default", oc.labels(N), "%s N=%d" % (path, N))
    same(got, batch(gpu_fx, N, low), "%s N=%d against the batch path" % (path, N))


# ---- single-analyser contexts ----
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_spectral_only_contexts_have_no_undefined_slot(gpu_fx, oracle, N):
    """the spectral analyser reads nothing out of bounds: every slot of every frame is held, with no mask"""
    hops = oc.hops(N)
    an = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, analysers="spectral")
    whole = an.push_hops(hops)
    an.close()
    close(whole, oc.oracle_run(oracle, N, analysers=1), "default", oc.labels(N), "spectral N=%d" % N, masked=False)
    one = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, analysers="spectral")
    same(path_runs._calls(one, hops, 1), whole, "spectral N=%d one frame per call" % N)
    one.close()


@pytest.mark.parametrize("N", [512, 2048])
def test_harmonic_only_contexts(gpu_fx, oracle, N):
    hops = oc.hops(N)
    an = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, analysers="harmonic")
    whole = an.push_hops(hops)
    an.close()
    want = oc.oracle_run(oracle, N, analysers=2)
    assert oc_same_bits(want[0][:, :, 2], oc.oracle_run(oracle, N)[0][:, :, 2]).all()            # (the mask is the full bundle's)
    close(whole, want, "default", oc.labels(N), "harmonic N=%d" % N)
    for k in (0, 1):                                              # the harmonic slots are the full bundle's, raw and smoothed
        assert oc_same_bits(whole[k][:, :, [2, 9, 10, 11]], batch(gpu_fx, N)[k][:, :, [2, 9, 10, 11]]).all()


# ---- the tail's discrete decisions: order modes, onset types and windows, on the batch path and one hop per call ----
def _tail_channels(N):
    """the channels whose histories meet non-finite values: the walks, the transients and the clean channels around them"""
    lo = oc.channels(N, "fade_in")[0]
    return list(range(lo, len(oc.labels(N))))


@pytest.mark.parametrize("window", [5, 32])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_order_modes_and_onset_types(gpu_fx, oracle, N, order, window):
    idx = _tail_channels(N)
    hops = np.ascontiguousarray(oc.hops(N)[idx])
    labels = [oc.labels(N)[i] for i in idx]
    for onset_type in (0, 1, 2):
        want = oracle.push_hops(hops, N, order=order, onset_type=onset_type, onset_sensitivity=0.2, onset_window=window)
        runs = {}
        for per in (oc.T, 1):
            an = gpu_fx.BatchAnalyser(len(idx), N, RATE, order=order)
            an.set_onset_detection_type(onset_type)
            an.set_onset_detection_sensitivity(0.2)
            an.set_onset_window_length(window)
            runs[per] = path_runs._calls(an, hops, per)
            an.close()
            what = "order %d type %d window %d N=%d, %d hops per call" % (order, onset_type, window, N, per)
            close(runs[per], want, "default", labels, what)
            for k in (0, 1):                                      # said once more: the onset column and the RMS are exact
                assert oc_same_bits(runs[per][k][:, :, [0, 1]], want[k][:, :, [0, 1]]).all(), what
        same(runs[1], runs[oc.T], "order %d type %d window %d N=%d: one hop per call against the batch path" % (order, onset_type, window, N))
    # one bad sample keeps the smoothed RMS non-finite for 6 frames where the analysers share their features (both write the RMS slot:
    # its 10-entry history holds 5 frames) and for 11 where they do not (tests/test_overflow_cpu.py holds it of the oracle)
    i = labels.index(("tone_bad", "nan@first"))
    for per in (oc.T, 1):
        assert np.array_equal(np.flatnonzero(~np.isfinite(runs[per][1][i, :, 1])), np.arange(6 if order == 1 else 11))


# ---- isolation: a clean channel beside poisoned ones is the clean channel alone ----
@pytest.mark.parametrize("N", oc.SIZES)
def test_clean_channels_are_untouched(gpu_fx, N):
    alone = run_path(gpu_fx, "batch", N, oc.clean(N))
    got = batch(gpu_fx, N)
    for k, idx in enumerate(oc.clean_channels(N).values()):
        for i in idx:
            same(tuple(g[i] for g in got), tuple(a[k] for a in alone), "N=%d clean channel %d" % (N, i))


# ---- routes: fp16 ingest, gains on every sample format, device blocks ----
def _f16_case(N):
    """[6][24][N/2] float16: a tone with NaN, +inf, -inf, 65504 and -65504 at sample 17 of the bad hops, and the tone itself"""
    tone = (oc.clean(N)[0] * np.float32(0.5)).astype(np.float16)
    rows = []
    for v in (np.nan, np.inf, -np.inf, 65504.0, -65504.0):
        x = tone.copy()
        for t in oc.BAD_HOPS:
            x[t, 17] = np.float16(v)
        rows.append(x)
    return np.ascontiguousarray(np.stack(rows + [tone]))


def _ring(gpu_fx, N, hops, low):
    an = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, low_latency=low)
    st = gpu_fx.HopStream(an, 1, slots=3, dtype=hops.dtype.type)
    got = []
    try:
        for t in range(hops.shape[1]):
            if st.in_flight() == 2:
                got.append(st.collect())
            st.push(hops[:, t:t + 1])
        while st.in_flight():
            got.append(st.collect())
    finally:
        st.close()
        an.close()
    return tuple(np.concatenate([g[k] for g in got], axis=1) for k in (0, 1))


@pytest.mark.parametrize("N,route", [(1024, "batch"), (2048, "pair"), (4096, "ring")])
def test_fp16_hops_with_non_finite_halves_equal_their_fp32_twins(gpu_fx, oracle, N, route):
    halves = _f16_case(N)
    floats = halves.astype(np.float32)
    assert np.isnan(floats[0]).sum() == 2 and np.isinf(floats[1:3]).sum() == 4 and np.abs(floats[3:5]).max() == 65504.0
    if route == "ring":
        got, twin = _ring(gpu_fx, N, halves, False), _ring(gpu_fx, N, floats, False)
    else:
        out = []
        for x in (halves, floats):
            an = gpu_fx.BatchAnalyser(halves.shape[0], N, RATE, low_latency=route == "pair")
            out.append(an.push_hops(x))
            an.close()
        got, twin = out
    same(got, twin, "fp16 %s N=%d against the fp32 twin" % (route, N))
    labels = [("f16 %s" % v, None) for v in ("nan", "+inf", "-inf", "65504", "-65504", "clean")]
    close(got, oracle.push_hops(floats, N), "low_latency" if route == "pair" else "default", labels, "fp16 %s N=%d" % (route, N))


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


@pytest.mark.parametrize("N", [512, 1024, 4096])
@pytest.mark.parametrize("fmt", ["f32", "f16", "s16", "s24"])
def test_a_gain_reaches_the_band_and_beyond(gpu_fx, oracle, fmt, N):
    """set_gain(10^e) on full-scale samples of every format equals the fp32 samples scaled beforehand, bit for bit, and the oracle"""
    x = np.stack([oc.full_scale(N, b) for b in oc.BASES])
    base = (x / np.float32(max(1.0, np.abs(x).max() * 1.001))).astype(np.float32)
    fed, floats = _as_format(gpu_fx, base, fmt)
    for e in GAIN_LEVELS:
        g = float(np.float32(10.0 ** e))
        an = gpu_fx.BatchAnalyser(len(oc.BASES), N, RATE)
        an.set_gain(g)
        got = an.push_hops(fed, sample_format=fmt)
        an.close()
        an = gpu_fx.BatchAnalyser(len(oc.BASES), N, RATE)
        before = an.push_hops(oc.scaled(floats, e))
        an.close()
        same(got, before, "%s N=%d: gain 1e%g against samples scaled beforehand" % (fmt, N, e))
        close(got, oracle.push_hops(floats, N, gain=g), "default", [(b, e) for b in oc.BASES], "gain 1e%g, %s N=%d" % (e, fmt, N))


@pytest.mark.parametrize("N", [512, 2048])
def test_device_blocks_of_the_transient_channels(gpu_fx, N):
    idx = oc.transients(N)
    hops = np.ascontiguousarray(oc.hops(N)[idx])
    blocks = run_path(gpu_fx, "blocks", N, hops)
    whole = run_path(gpu_fx, "batch", N, hops)
    same(blocks, whole, "N=%d: 480-sample blocks against whole hops" % N)
    same(whole, tuple(b[idx] for b in batch(gpu_fx, N)), "N=%d: the transient channels alone against the whole case" % N)


# ---- recovery by reset ----
@pytest.mark.parametrize("per", [1, 12])
@pytest.mark.parametrize("N", [1024, 2048])
def test_reset_after_the_bad_hops_leaves_fresh_tracks(gpu_fx, oracle, N, per):
    """After the second bad hop the poisoned tracks are reset: from there on they are a fresh context's tracks fed the remaining hops,
    nothing non-finite is left in them, and every other track goes on as if nothing had happened; reset_state does it for all tracks."""
    lo = oc.channels(N, "tone_bad")[0]
    idx = list(range(lo - 1, len(oc.labels(N))))                  # the transients, with the clean channels before, among and behind them
    labels = [oc.labels(N)[i] for i in idx]
    hops = np.ascontiguousarray(oc.hops(N)[idx])
    bad = [k for k, (kind, _) in enumerate(labels) if kind in ("tone_bad", "bursts_bad")]
    good = [k for k in range(len(idx)) if k not in bad]
    at = 12
    assert at > oc.BAD_HOPS[-1] + 1 and len(good) >= 3 and all(labels[k][0].startswith("clean") for k in good)

    def context():
        return gpu_fx.BatchAnalyser(len(idx), N, RATE)

    an = context()
    head = path_runs._calls(an, hops[:, :at], per)
    assert not np.isfinite(head[1][bad][:, :, 1]).all()           # (there was something to recover from)
    an.reset_channels(bad)
    tail = path_runs._calls(an, hops[:, at:], per)
    latest = an.get_features()
    an.close()
    fresh_an = context()
    fresh = path_runs._calls(fresh_an, hops[:, at:], per)
    fresh_latest = fresh_an.get_features()
    fresh_an.close()
    straight = context()
    through = path_runs._calls(straight, hops, per)
    straight.close()
    same(tuple(t[bad] for t in tail), tuple(f[bad] for f in fresh), "N=%d per %d: reset tracks against fresh tracks" % (N, per))
    assert oc_same_bits(latest[bad], fresh_latest[bad]).all()
    want = oracle.push_hops(hops[bad][:, at:], N)                 # a fresh oracle track fed the remaining hops: finite, f0 > 0
    assert all(np.isfinite(w).all() for w in want) and (want[0][:, :, 2] > 0).all()
    close(tuple(t[bad] for t in tail), want, "default", [labels[k] for k in bad], "N=%d per %d: reset tracks against a fresh oracle" % (N, per))
    for rows in (tail[0][bad], tail[1][bad], latest[bad]):
        assert np.isfinite(rows).all()
    same(tuple(np.concatenate([h[good], t[good]], axis=1) for h, t in zip(head, tail)), tuple(s[good] for s in through), "N=%d per %d: the other tracks" % (N, per))
    an = context()
    path_runs._calls(an, hops[:, :at], per)
    an.reset_state()
    same(path_runs._calls(an, hops[:, at:], per), fresh, "N=%d per %d: reset_state against a fresh context" % (N, per))
    an.close()


# ---- taps: the display buffers of a band-level channel, of +inf under Bartlett weight 0 and of a transform-overflow channel ----
# (tests/test_overflow_cpu.py holds that tests/taps_model.py reproduces the oracle's own buffers for these windows)
@pytest.mark.parametrize("N,low", [(1024, False), (4096, False), (4096, True)])
def test_taps_of_overflowing_and_non_finite_windows(gpu_fx, oracle, N, low):
    hops = oc.hops(N)
    chans, TAP_FRAME = oc.tap_channels(N), oc.TAP_FRAME
    an = gpu_fx.BatchAnalyser(hops.shape[0], N, RATE, low_latency=low)
    an.push_hops(hops[:, :TAP_FRAME])
    an.request_taps(chans)
    an.push_hops(hops[:, TAP_FRAME:TAP_FRAME + 1])
    assert an.last_launches()[0]["kind"] == "taps"
    got = [an.taps(c) for c in chans]
    an.close()
    for c, g in zip(chans, got):
        assert g["frame_index"] == TAP_FRAME
        taps_model.assert_taps_equal(g, taps_model.oracle_taps(oracle, oc.tap_window(N, c)), "N=%d %s" % (N, oc.label_id(oc.labels(N)[c])))
