"""tests/tail_model.py, pinned: the model of the reference's tail equals, bit for bit, the oracle's smoothed vectors and onset
column over every signal, window size, order mode, analyser set and onset setting, settings changed and state reset in
mid-stream, and the smoothed vectors of every fixture the reference's own headers made.  The sweep must fire onsets and put
onset candidates on both sides of the detector's 0.01 amplitude gate, or an exact onset column proves nothing.  Also the
ulp helpers of oracle/ulp.py and tests/signals.py."""
import glob
import os
import sys

import numpy as np
import pytest

import signals
import tail_model as tm
from oracle import fx_oracle as fo

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "*.npz")))
MASKS = {"both": 3, "spectral": 1, "harmonic": 2}
WINDOWS = (1, 2, 3, 4, 5, 8, 16, 21, 31, 32)
SENSITIVITIES = (0.0, 0.7, 5.0)                 # none, the reference's default (multiplier 1.7), a large one


def oracle_timeline(hops, N, order, mask, events):
    """the oracle, one fxo_channel per channel, with the events' per-channel setters between the hops they separate"""
    C, T = hops.shape[0], hops.shape[1]
    raw = np.empty((C, T, 12), np.float32)
    sm = np.empty((C, T, 12), np.float32)
    cuts = sorted(set([0, T] + [e[0] for e in events if e[0] < T]))
    for c in range(C):
        ch = fo.Channel(N, order=order)
        ch.set_analysers(mask)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            for e in events:
                if e[0] != lo:
                    continue
                if e[1] == "onset_window":
                    ch.set_onset_window(e[2])
                elif e[1] == "sensitivity":
                    ch.set_onset_sensitivity(e[2])
                elif e[1] == "onset_type":
                    ch.set_onset_type(e[2])
                elif e[1] == "reset":
                    ch.reset()
                elif e[1] == "gain":
                    ch.set_gain(e[2])
                elif e[1] == "sample_rate":
                    ch.set_sample_rate(e[2])
            raw[c, lo:hi], sm[c, lo:hi] = ch.push_hops(hops[c, lo:hi])
    return raw, sm


def onset_stream(C, T, N, seed):
    """tone bursts over exact silence, quiet noise and impulses of random height: amplitude and flux jumps, and quiet frames
    below the 0.01 gate"""
    rng = np.random.default_rng(seed)
    x = signals.bursts(C, T, N, seed=seed)
    quiet = rng.random((C, T)) < 0.2
    x[quiet] = rng.normal(0, 1e-3, (int(quiet.sum()), N // 2)).astype(np.float32)
    hit = rng.random((C, T)) < 0.12
    for c, t in zip(*np.nonzero(hit)):
        x[c, t, rng.integers(0, N // 2)] += np.float32(rng.uniform(0.1, 0.9))
    for c in range(C):                          # stretches of silence long enough for the smoothed RMS to fall below the gate
        for at in rng.integers(0, max(1, T - 16), 2):
            x[c, at:at + 14] = 0.0
    return x.astype(np.float32)


def sweep_events(otype):
    """every onset window of WINDOWS, held long enough to fill and detect, each sensitivity, a gain and a sample-rate change
    (no effect on the tail) and a reset in mid-stream"""
    ev, t = [(0, "onset_type", otype)], 0
    for k, w in enumerate(WINDOWS):
        ev.append((t, "onset_window", w))
        ev.append((t, "sensitivity", SENSITIVITIES[k % 3]))
        t += w + 6
    ev += [(9, "gain", 0.5), (30, "sample_rate", 44100.0), (60, "reset"), (60, "onset_window", 5), (140, "reset")]
    return ev, t


def run_model(raw, events, order, mask):
    tail = tm.Tail(raw.shape[0], order, mask)
    sm, onset = tm.run(raw, events, order, mask, tail=tail)
    cand = np.concatenate(tail.detector.candidates) if tail.detector.candidates else np.zeros(0, np.float32)
    return sm, onset, cand


def assert_same(sm, onset, raw, osm, what):
    assert np.array_equal(onset, raw[..., 0]), "%s: onset column, model %d onsets, oracle %d" % (what, onset.sum(), raw[..., 0].sum())
    same = (sm.view(np.uint32) == osm.view(np.uint32)) | (np.isnan(sm) & np.isnan(osm))
    assert same.all(), "%s: smoothed differs at %s: model %r oracle %r" % (what, np.argwhere(~same)[0], sm[~same][0], osm[~same][0])


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("sig", sorted(signals.ALL))
def test_model_equals_oracle_on_every_signal(sig, N):
    hops = signals.ALL[sig](3, 16, N)
    raw, sm = fo.push_hops(hops, N)
    msm, mon, _ = run_model(raw, (), 0, 3)
    assert_same(msm, mon, raw, sm, "%s N=%d" % (sig, N))


CONTEXTS = [(o, a, t) for o in range(3) for a in MASKS for t in range(3)]
FIRED = {}


@pytest.mark.parametrize("order,analysers,otype", CONTEXTS, ids=["order%d-%s-type%d" % c for c in CONTEXTS])
def test_model_equals_oracle_with_settings_timeline(order, analysers, otype):
    ev, T = sweep_events(otype)
    hops = onset_stream(8, T, 256, seed=order * 3 + otype)
    mask = MASKS[analysers]
    raw, sm = oracle_timeline(hops, 256, order, mask, ev)
    msm, mon, cand = run_model(raw, ev, order, mask)
    assert_same(msm, mon, raw, sm, "order %d %s type %d" % (order, analysers, otype))
    if mask & 1:
        assert mon.sum() >= 1, "order %d %s type %d: no onset" % (order, analysers, otype)
        assert (cand < 0.01).any() and (cand >= 0.01).any(), (int((cand < 0.01).sum()), int((cand >= 0.01).sum()))
    else:
        assert not mon.any() and np.isnan(msm[..., [tm.CENTROID, tm.FLUX, tm.ONSET]]).all()


@pytest.mark.parametrize("otype,least", [(tm.ONSET_SPECTRAL, 150), (tm.ONSET_AMPLITUDE, 150), (tm.ONSET_COMBINATION, 20)])
def test_sweep_fires_onsets_of_every_type(otype, least):
    """over the three order modes with both analysers: a floor on the onsets, and candidates on both sides of the gate"""
    ev, T = sweep_events(otype)
    fired, low, high = 0, 0, 0
    for order in range(3):
        raw, _ = oracle_timeline(onset_stream(8, T, 256, seed=order * 3 + otype), 256, order, 3, ev)
        _, mon, cand = run_model(raw, ev, order, 3)
        fired += int(mon.sum())
        low += int((cand < 0.01).sum())
        high += int((cand >= 0.01).sum())
    assert fired >= least, (otype, fired)
    assert low >= 20 and high >= 20, (otype, low, high)


@pytest.mark.parametrize("window", WINDOWS)
def test_model_equals_oracle_at_every_onset_window(window):
    ev = [(0, "onset_type", tm.ONSET_COMBINATION), (0, "onset_window", window), (0, "sensitivity", 0.0)]
    hops = onset_stream(4, 3 * window + 24, 512, seed=window)
    raw, sm = oracle_timeline(hops, 512, 1, 3, ev)
    msm, mon, _ = run_model(raw, ev, 1, 3)
    assert_same(msm, mon, raw, sm, "window %d" % window)


def test_rms_inserts_and_the_amplitude_the_detector_sees():
    """both analysers on one AudioFeatures: RMS goes in twice per frame; the detector reads it after two inserts
    (harmonic then spectral) or one (spectral then harmonic); isolated or one analyser: once"""
    raw = np.zeros((1, 3, 12), np.float32)
    raw[0, :, tm.RMS] = [0.1, 0.4, 0.7]
    for order, mask, recorded in [(0, 3, 6), (1, 3, 6), (2, 3, 3), (0, 1, 3), (0, 2, 3)]:
        tail = tm.Tail(1, order, mask)
        tm.run(raw, (), order, mask, tail=tail)
        assert tail.fs.hist[tm.RMS].recorded == recorded, (order, mask)
    seen = {}
    for order in (0, 1):
        tail = tm.Tail(1, order, 3)
        tm.run(raw[:, :1], (), order, 3, tail=tail)
        seen[order] = tail.detector.amp.h[0, -1]
    assert seen[1] == np.float32(0.1) and seen[0] == np.float32(0.1)          # one frame: the mean of 0.1 (twice) or 0.1 (once)
    for order in (0, 1):
        tail = tm.Tail(1, order, 3)
        tm.run(raw[:, :2], (), order, 3, tail=tail)
        seen[order] = tail.detector.amp.h[0, -1]
    f = np.float32
    assert seen[0] == (f(0.1) + f(0.1) + f(0.4)) / f(3) and seen[1] == (f(0.1) + f(0.1) + f(0.4) + f(0.4)) / f(4), seen


def test_onset_window_empties_the_onset_histories_only_and_reset_empties_all():
    raw = np.random.default_rng(0).random((2, 9, 12)).astype(np.float32)
    tail = tm.Tail(2)
    tm.run(raw, [(8, "onset_window", 3)], tail=tail)
    assert tail.detector.amp.recorded == 1 and tail.detector.amp.h.shape == (2, 3)
    assert tail.fs.hist[tm.CENTROID].recorded == 9
    tm.run(raw[:, :1], [(0, "reset")], tail=tail)
    assert tail.detector.amp.recorded == 1 and tail.detector.amp.h.shape == (2, 3) and tail.fs.hist[tm.CENTROID].recorded == 1
    sm, _ = tm.run(raw[:, :1], (), 0, 2)
    assert np.isnan(sm[:, 0, [tm.ONSET, tm.CENTROID, tm.FLUX, tm.SLOPE]]).all() and not np.isnan(sm[:, 0, [tm.RMS, tm.F0]]).any()


# ---- against the reference's own output ----
@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
def test_model_reproduces_golden_fixture(path):
    g = np.load(path)
    sm, onset, _ = run_model(g["raw"], (), int(g["order"]), 3)
    assert_same(sm, onset, g["raw"], g["smoothed"], os.path.basename(path))


def test_model_reproduces_random_reference_cases():
    import test_oracle
    fired = 0
    for k, p, hops, raw, sm in test_oracle._random_reference_cases():
        ev = [(0, "onset_type", p["onset_type"]), (0, "sensitivity", p["sensitivity"]), (0, "onset_window", p["onset_window"])]
        msm, mon, _ = run_model(raw, ev, p["order"], 3)
        assert_same(msm, mon, raw, sm, "random case %d" % k)
        fired += int(mon.sum())
    assert fired >= 20, fired


def test_model_reproduces_block_fixtures():
    """tests/golden/blocks: the runtime setters at hop boundaries (blocks of one hop) map to frame indices; gain and
    clearBuffer change no tail value wherever they fall"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import block_cases
    import startup_cases
    d = np.load(os.path.join(HERE, "golden", "blocks", "cases.npz"))
    fired = 0
    for name, N, C, hops, extra, block, order, events in block_cases.CASES:
        ev = []
        for e in events:
            if e[1] in ("gain", "clear"):
                continue
            assert e[0] % (N // 2) == 0, (name, e)
            ev.append((e[0] // (N // 2),) + tuple(e[1:]))
        sm, onset, _ = run_model(d[name + "_raw"], ev, order, 3)
        assert_same(sm, onset, d[name + "_raw"], d[name + "_smoothed"], name)
        fired += int(onset.sum())
    s = np.load(os.path.join(HERE, "golden", "blocks", "startup.npz"))
    for name, N, C, total, block, order in startup_cases.CASES:
        sm, onset, _ = run_model(s[name + "_raw"], (), order, 3)
        assert_same(sm, onset, s[name + "_raw"], s[name + "_smoothed"], name)
        fired += int(onset.sum())
    assert fired >= 20, fired


# ---- the ulp helper ----
def test_ulp_distance_edges():
    f = np.float32
    d = signals.ulp_distance
    tiny = np.float32(1.4e-45)                              # the smallest subnormal
    big = np.finfo(np.float32).max
    assert d(f(0.0), f(-0.0)) == 0
    assert d(f(1.0), np.nextafter(f(1.0), f(2))) == 1 and d(f(1.0), np.nextafter(f(1.0), f(0))) == 1
    assert d(tiny, f(0.0)) == 1 and d(-tiny, tiny) == 2 and d(tiny * f(3), f(0.0)) == 3
    assert d(np.finfo(np.float32).tiny, np.nextafter(np.finfo(np.float32).tiny, f(0))) == 1      # normal to subnormal
    assert d(f(-1.0), f(1.0)) == 2 * int(np.float32(1.0).view(np.int32))
    assert d(big, np.nextafter(big, f(0))) == 1
    assert d(f(np.nan), f(np.nan)) == 0 and d(f(np.nan), f(1.0)) >= signals.ULP_INFINITE and d(f(0.0), f(np.nan)) >= signals.ULP_INFINITE
    assert d(f(np.inf), f(np.inf)) == 0 and d(f(-np.inf), f(-np.inf)) == 0
    assert d(f(np.inf), big) >= signals.ULP_INFINITE and d(f(np.inf), f(-np.inf)) >= signals.ULP_INFINITE
    assert d(f(np.nan), f(np.inf)) >= signals.ULP_INFINITE
    x = np.array([1.0, -2.5, 3e-40], np.float32)
    assert list(d(x, x)) == [0, 0, 0]


def test_assert_features_within():
    w = np.random.default_rng(1).random((2, 3, 12)).astype(np.float32)
    w[..., 0] = [[0, 1, 0], [1, 0, 0]]
    w[0, 0, 5] = np.nan
    w[1, 2, 7] = np.inf
    budget = signals.ulp_budget("default")
    assert signals.assert_features_within(w.copy(), w, budget).max() == 0
    g = w.copy()
    g[0, 1, 4] = np.nextafter(g[0, 1, 4], np.float32(9), dtype=np.float32)       # 1 ulp
    signals.assert_features_within(g, w, np.maximum(budget, 1) * (np.arange(12) > 0))
    with pytest.raises(AssertionError):
        signals.assert_features_within(g, w, np.zeros(12, np.int64))
    g = w.copy()
    g[1, 0, 0] = 0
    with pytest.raises(AssertionError, match="onset"):
        signals.assert_features_within(g, w, np.full(12, 0))
    g = w.copy()
    g[0, 0, 5] = 0.5
    with pytest.raises(AssertionError):
        signals.assert_features_within(g, w, np.array([0] + [1000] * 11))
    g = w.copy()
    g[1, 2, 7] = np.finfo(np.float32).max
    with pytest.raises(AssertionError):
        signals.assert_features_within(g, w, np.array([0] + [1000] * 11))


def test_budget_table():
    for fam in ("default", "low_latency"):
        b = signals.ulp_budget(fam)
        assert b.shape == (12,) and b[tm.ONSET] == 0 and b[tm.F0] == 0 and (b >= 0).all()
