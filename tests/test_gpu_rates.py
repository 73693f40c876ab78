"""Every kernel family at sample rates beyond 48 / 44.1 kHz, on inputs that sit on the rate's rounding edges (tests/rate_cases.py; the CPU
side -- the inputs really are on the edges, the oracle equals the reference's headers there -- is tests/test_rates_cpu.py).  The bar is the
suite's: onset and f0 exact, every other slot within its ulp budget (oracle/ulp.py), every path the batch path's bits, a power-of-two
change of rate invisible but for F0.  All tests here need a real MI355X.

With FX_RATES_ULP_OUT set to a file name, the largest ulp distance seen per family, rate and slot is written there when the module is
done (the record profiles/rates_ulp.txt was made that way)."""
import os

import numpy as np
import pytest

import path_runs
import rate_cases as rc
import signals
import taps_model

pytestmark = pytest.mark.gpu
_calls = path_runs._calls

RATE_IDS = [rc.rate_id(r) for r in rc.RATES]
ULP_SEEN = {}                                   # (family, rate) -> largest distance per slot


@pytest.fixture(scope="module", autouse=True)
def _ulp_record():
    yield
    path = os.environ.get("FX_RATES_ULP_OUT")
    if path and ULP_SEEN:
        with open(path, "w") as f:
            f.write("largest fp32 ulp distance from the oracle, raw and smoothed, over the rate cases and every path of tests/test_gpu_rates.py\n")
            f.write("%-12s %-10s %s\n" % ("family", "rate", " ".join("%-8s" % s for s in signals.SLOTS)))
            for (family, rate), d in sorted(ULP_SEEN.items()):
                f.write("%-12s %-10s %s\n" % (family, rate, " ".join("%-8d" % v for v in d)))


def close(got, want, family, rate, what):
    """both vectors within the family's budget; the maxima are kept for the record"""
    from oracle import fx_oracle as fo
    for k, name in ((0, "raw"), (1, "smoothed")):
        d = signals.assert_features_within(got[k], want[k], signals.ulp_budget(family), fo.FEATURE_NAMES, "%s at %s %s" % (what, rate if isinstance(rate, str) else rc.rate_id(rate), name))
        key = (family, rate if isinstance(rate, str) else rc.rate_id(rate))
        ULP_SEEN[key] = np.maximum(ULP_SEEN.get(key, np.zeros(12, np.int64)), d)


def same(got, want, what):
    for k in (0, 1):
        assert np.array_equal(got[k], want[k], equal_nan=True), "%s: %s differs at %s" % (what, ("raw", "smoothed")[k], np.argwhere(~rc.same_bits(got[k], want[k]))[:5])


def run_path(gpu_fx, path, N, rate):
    """(raw, smoothed) of the size's whole case through one dispatch path (the fused tail in calls of 8, 8, 5 and 3 frames)"""
    return path_runs.run_path(gpu_fx, path, N, rate, rc.hops(N), fused_calls=((0, 8), (8, 16), (16, 21), (21, 24)))


_BATCH = {}


def batch(gpu_fx, N, rate, low=False):
    """the batch path's result, computed once per (size, rate, family) and shared"""
    key = (N, rate, low)
    if key not in _BATCH:
        _BATCH[key] = run_path(gpu_fx, "pair" if low else "batch", N, rate)
    return _BATCH[key]


# ---- parity of the batch kernels, every size and rate ----
@pytest.mark.parametrize("N", rc.SIZES)
@pytest.mark.parametrize("rate", rc.RATES, ids=RATE_IDS)
def test_batch_frame_kernel_matches_oracle(gpu_fx, oracle, rate, N):
    close(batch(gpu_fx, N, rate), rc.oracle_run(oracle, N, rate), "default", rate, "batch N=%d" % N)


@pytest.mark.parametrize("N", [2048, 4096])
@pytest.mark.parametrize("rate", rc.RATES, ids=RATE_IDS)
def test_pair_kernel_matches_oracle(gpu_fx, oracle, rate, N):
    got = batch(gpu_fx, N, rate, low=True)
    close(got, rc.oracle_run(oracle, N, rate), "low_latency", rate, "pair N=%d" % N)
    ref = batch(gpu_fx, N, rate)
    for k in (0, 1):                                              # the discrete decisions are the default family's
        assert np.array_equal(got[k][:, :, [0, 2]], ref[k][:, :, [0, 2]], equal_nan=True)


# ---- every other path: the oracle's values within the budget, and the batch path's bits ----
PATHS = ([("fused_tail", N) for N in rc.SIZES] + [("direct", N) for N in rc.SIZES]
         + [(p, N) for p in ("frame_tail", "hop", "ring_hop") for N in (1024, 2048, 4096)]
         + [(p, N) for p in ("hop_pair", "ring_hop_pair") for N in (2048, 4096)] + [("blocks", 1024)])


@pytest.mark.parametrize("path,N", PATHS, ids=["%s-%d" % p for p in PATHS])
def test_every_path_matches_oracle_and_equals_the_batch_path_bitwise(gpu_fx, oracle, path, N):
    low = path in ("hop_pair", "ring_hop_pair")
    for rate in rc.RATES:
        got = run_path(gpu_fx, path, N, rate)
        close(got, rc.oracle_run(oracle, N, rate), "low_latency" if low else "default", rate, "%s N=%d" % (path, N))
        same(got, batch(gpu_fx, N, rate, low), "%s N=%d at %s against the batch path" % (path, N, rc.rate_id(rate)))


@pytest.mark.parametrize("which,mask,N", [("harmonic", 2, 2048), ("spectral", 1, 512)])
def test_single_analyser_modes(gpu_fx, oracle, which, mask, N):
    hops = rc.hops(N)
    for rate in rc.RATES:
        an = gpu_fx.BatchAnalyser(rc.C, N, rate, analysers=which)
        whole = an.push_hops(hops)
        close(whole, rc.oracle_run(oracle, N, rate, analysers=mask), "default", rate, "%s N=%d" % (which, N))
        one = gpu_fx.BatchAnalyser(rc.C, N, rate, analysers=which)
        same(_calls(one, hops, 1, ("frame", "epilogue")), whole, "%s N=%d one frame per call at %s" % (which, N, rc.rate_id(rate)))
        if which == "harmonic":                                   # the harmonic slots are those of the full bundle
            full = batch(gpu_fx, N, rate)
            assert np.array_equal(whole[0][:, :, [2, 9, 10, 11]], full[0][:, :, [2, 9, 10, 11]], equal_nan=True)
        an.close(); one.close()


# ---- a power of two times the rate: the same bits, F0 exactly scaled ----
@pytest.mark.parametrize("N", rc.SIZES)
def test_power_of_two_invariance(gpu_fx, N):
    rc.assert_power_of_two_invariant(lambda rate: batch(gpu_fx, N, rate), "batch N=%d" % N)
    if N >= 1024:
        rc.assert_power_of_two_invariant(lambda rate: run_path(gpu_fx, "hop", N, rate), "hop kernel N=%d" % N)


@pytest.mark.parametrize("N", [2048, 4096])
def test_power_of_two_invariance_low_latency(gpu_fx, N):
    rc.assert_power_of_two_invariant(lambda rate: batch(gpu_fx, N, rate, low=True), "pair N=%d" % N)
    rc.assert_power_of_two_invariant(lambda rate: run_path(gpu_fx, "hop_pair", N, rate), "hop pair N=%d" % N)


# ---- the rate changed mid-stream, to a non-dyadic rate and back ----
CHANGES = [(8, rc.MID_STREAM_RATE), (16, 48000.0)]                # (before hop, rate): the event list of the reference's record


def _with_changes(an, at):
    for hop, rate in CHANGES:
        if hop == at:
            an.sample_rate_changed(rate)


@pytest.mark.parametrize("N", [512, 1024, 4096])
def test_rate_changed_mid_stream_push_hops(gpu_fx, oracle, N):
    hops = rc.hops(N)
    want = rc.oracle_with_rate_events(oracle, hops, N, CHANGES)
    results = {}
    for per in (1, 2, 8):                                         # one-frame kernels, two launches / the two-frame form, the batch kernels
        an = gpu_fx.BatchAnalyser(rc.C, N)
        outs = []
        for t in range(0, rc.T, per):
            _with_changes(an, t)
            outs.append(an.push_hops(hops[:, t:t + per]))
        results[per] = tuple(np.concatenate([o[k] for o in outs], axis=1) for k in (0, 1))
        close(results[per], want, "default", "mid-stream", "mid-stream N=%d, %d hops per call" % (N, per))
        same(results[per], results[1], "mid-stream N=%d, %d hops per call against one" % (N, per))
        an.close()


@pytest.mark.parametrize("per", [1, 2])
@pytest.mark.parametrize("graph", ["0", "1"])
def test_rate_changed_mid_stream_through_the_ring(gpu_fx, oracle, monkeypatch, graph, per):
    """The ring's hop-kernel route (one hop per batch) and its captured step (two: with FX_STREAM_GRAPH=1 nyquist travels through
    device memory and frpb, 1 / nyquist and the bin deviation are derived again on the device; =0: plain launches)."""
    monkeypatch.setenv("FX_STREAM_GRAPH", graph)
    N = 1024
    hops = rc.hops(N)
    want = rc.oracle_with_rate_events(oracle, hops, N, CHANGES)
    ref = gpu_fx.BatchAnalyser(rc.C, N)
    plain = []
    for t in range(0, rc.T, per):
        _with_changes(ref, t)
        plain.append(ref.push_hops(hops[:, t:t + per]))
    plain = tuple(np.concatenate([o[k] for o in plain], axis=1) for k in (0, 1))
    an = gpu_fx.BatchAnalyser(rc.C, N)
    st = gpu_fx.HopStream(an, per, slots=3)
    got = []
    for t in range(0, rc.T, per):
        _with_changes(an, t)                                      # a setter applies to the batches submitted after it
        if st.in_flight() == 3:
            got.append(st.collect())
        st.push(hops[:, t:t + per])
    while st.in_flight():
        got.append(st.collect())
    got = tuple(np.concatenate([g[k] for g in got], axis=1) for k in (0, 1))
    close(got, want, "default", "mid-stream", "ring graph=%s, %d hops per batch" % (graph, per))
    same(got, plain, "ring graph=%s, %d hops per batch against fx_push_hops" % (graph, per))
    assert np.array_equal(an.get_features(), ref.get_features(), equal_nan=True)
    st.close(); an.close(); ref.close()


# ---- taps: the display buffers do not know the rate ----
@pytest.mark.parametrize("N,low", [(512, False), (1024, False), (4096, False), (2048, True)])
def test_taps_are_rate_free(gpu_fx, oracle, N, low):
    """window, spectra, autocorrelation, CND and the lag position (a fraction of the window) hold no frequency: a capture at any rate
    equals the capture at 48 kHz bit for bit, and that one the taps model"""
    hops = rc.hops(N, frames=4)
    chans = [0, rc.C - 1]

    def capture(rate):
        an = gpu_fx.BatchAnalyser(rc.C, N, rate, low_latency=low)
        an.push_hops(hops[:, :2])
        an.request_taps(chans)
        an.push_hops(hops[:, 2:3])
        assert an.last_launches()[0]["kind"] == "taps"
        out = [an.taps(c) for c in chans]
        an.close()
        return out

    want = capture(48000.0)
    for c, w in zip(chans, want):
        taps_model.assert_taps_equal(w, taps_model.oracle_taps(oracle, np.concatenate([hops[c, 1], hops[c, 2]])), "N=%d channel %d at 48000" % (N, c))
    for rate in rc.RATES:
        for c, g, w in zip(chans, capture(rate), want):
            assert g["frame_index"] == w["frame_index"] == 2
            for k in taps_model.FIELDS:
                assert np.array_equal(g[k], w[k], equal_nan=True), "N=%d channel %d %s at %s" % (N, c, k, rc.rate_id(rate))
