"""The tail on the device, bit for bit: the smoothed vectors and the onset column every tail form delivers are what the
reference's own tail (tests/tail_model.py) makes of the raw stream the device delivered.  One context per order mode x
analysers x onset type, over a stream of bursts and impulses more than three history rings (HLEN = 48) long, fed in ragged
calls of 1, 2, 7, 8, 9, 47, 48 and 49 frames (both sides of FUSED_TAIL_MAX_FRAMES = 8 and of the ring's wrap), while the
onset window steps through 1 .. 32, the sensitivity changes and the state is reset once.  The default family at 1024
points, FX_LOW_LATENCY at 2048 and 4096, one hop per call (the hop kernels) and a HopStream ring with the settings changed
between submissions (the captured step's per-call parameters)."""
import numpy as np
import pytest

import signals
import tail_model

pytestmark = pytest.mark.gpu

C = 6
SHORT = (1, 2, 7, 8, 9)
LONG = (49, 1, 48, 2, 47, 8, 9, 7)
HELD = (1, 2, 3, 4, 5, 8, 16, 21, 31, 32)            # windows held long enough to fill and detect; the others pass in one frame
SENSITIVITY = {1: 0.0, 5: 0.7, 8: 2.5, 21: 0.0, 32: 0.3}
MASKS = {"both": 3, "spectral": 1, "harmonic": 2}


def timeline():
    """(events [(frame, name, value)], call lengths): phase A steps the onset window through 1 .. 32 in short calls cut at
    the events; phase B runs the long calls with a sensitivity change and one reset between them"""
    ev, cuts, t = [], [], 0
    for w in range(1, 33):
        ev.append((t, "onset_window", w))
        if w in SENSITIVITY:
            ev.append((t, "sensitivity", SENSITIVITY[w]))
        cuts.append(t)
        t += w + 5 if w in HELD else 1
    ev.append((t, "onset_window", 5))
    cuts.append(t)
    b = t
    for n in LONG:
        t += n
        cuts.append(t)
    ev.append((b + 49, "sensitivity", 1.2))
    ev.append((b + 49 + 1 + 48, "reset"))
    ev.append((b + 49 + 1 + 48, "onset_window", 3))
    lengths, k = [], 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        while lo < hi:
            n = min(SHORT[k % len(SHORT)], hi - lo) if lo < b else hi - lo
            lengths.append(n)
            lo += n
            k += 1
    return ev, lengths


def stream(T, N, seed=0):
    """bursts of a tone with noise over exact silence, and impulses of random height: the flux and the amplitude jump"""
    rng = np.random.default_rng(seed)
    x = signals.bursts(C, T, N, seed=seed + 4)
    hit = rng.random((C, T)) < 0.15
    for c, t in zip(*np.nonzero(hit)):
        x[c, t, rng.integers(0, N // 2)] += np.float32(rng.uniform(0.2, 0.95))
    return x.astype(np.float32)


def apply(an, e):
    if e[1] == "onset_window":
        an.set_onset_window_length(e[2])
    elif e[1] == "sensitivity":
        an.set_onset_detection_sensitivity(e[2])
    elif e[1] == "onset_type":
        an.set_onset_detection_type(e[2])
    elif e[1] == "reset":
        an.reset_state()
    else:
        raise ValueError(e)


def run_calls(an, hops, ev, lengths):
    outs, t = [], 0
    for n in lengths:
        for e in ev:
            if e[0] == t:
                apply(an, e)
        outs.append(an.push_hops(hops[:, t:t + n]))
        t += n
    assert t == hops.shape[1]
    return np.concatenate([o[0] for o in outs], 1), np.concatenate([o[1] for o in outs], 1)


def check(raw, sm, ev, order, mask, what):
    fired = tail_model.assert_tail_exact(raw, sm, ev, order, mask, what)
    if mask & 1:
        assert fired > 0, "%s: the stream fired no onset; the onset column proves nothing" % what
    return fired


CONTEXTS = [(o, a, t) for o in range(3) for a in MASKS for t in range(3)]


@pytest.fixture(scope="module")
def plan():
    ev, lengths = timeline()
    T = sum(lengths)
    assert T > 3 * 48 and set(SHORT + LONG) <= set(lengths), (T, sorted(set(lengths)))
    return ev, lengths, T


@pytest.mark.parametrize("order,analysers,otype", CONTEXTS, ids=["order%d-%s-type%d" % c for c in CONTEXTS])
def test_default_family_tail_equals_model(gpu_fx, plan, order, analysers, otype):
    ev, lengths, T = plan
    N = 1024
    hops = stream(T, N, seed=order * 9 + otype)
    an = gpu_fx.BatchAnalyser(C, N, order=order, analysers=analysers)
    an.set_onset_detection_type(otype)
    raw, sm = run_calls(an, hops, ev, lengths)
    an.close()
    check(raw, sm, [(0, "onset_type", otype)] + ev, order, MASKS[analysers], "N=%d order %d %s type %d" % (N, order, analysers, otype))


LL = [(N, o, t) for N in (2048, 4096) for o in range(3) for t in range(3)]


@pytest.mark.parametrize("N,order,otype", LL, ids=["%d-order%d-type%d" % c for c in LL])
def test_low_latency_tail_equals_model(gpu_fx, plan, N, order, otype):
    ev, lengths, T = plan
    hops = stream(T, N, seed=N + order * 3 + otype)
    an = gpu_fx.BatchAnalyser(C, N, order=order, low_latency=True)
    an.set_onset_detection_type(otype)
    raw, sm = run_calls(an, hops, ev, lengths)
    an.close()
    check(raw, sm, [(0, "onset_type", otype)] + ev, order, 3, "low latency N=%d order %d type %d" % (N, order, otype))


@pytest.mark.parametrize("order,otype", [(0, 1), (1, 2)])
def test_hop_by_hop_tail_equals_model(gpu_fx, plan, order, otype):
    """one hop per call: the hop kernel's own one-frame tail"""
    ev, lengths, T = plan
    N = 2048
    hops = stream(T, N, seed=77 + order)
    an = gpu_fx.BatchAnalyser(C, N, order=order)
    an.set_onset_detection_type(otype)
    raw, sm = run_calls(an, hops, ev, [1] * T)
    assert [k["kind"] for k in an.last_launches()] == ["hop"], an.last_launches()
    an.close()
    check(raw, sm, [(0, "onset_type", otype)] + ev, order, 3, "hop by hop order %d type %d" % (order, otype))


@pytest.mark.parametrize("graph", ["0", "1"])
def test_hop_stream_tail_equals_model(gpu_fx, monkeypatch, graph):
    """the ring, settings changed between submissions: with FX_STREAM_GRAPH=1 they reach the replayed step as its per-call
    parameters in device memory"""
    monkeypatch.setenv("FX_STREAM_GRAPH", graph)
    N, B, nb = 1024, 4, 40
    ev = [(0, "onset_type", 2), (0, "onset_window", 3), (8, "sensitivity", 0.0), (16, "onset_window", 1), (20, "onset_window", 8),
          (40, "onset_type", 1), (48, "sensitivity", 2.0), (60, "onset_window", 32), (100, "reset"), (100, "onset_window", 4),
          (112, "onset_type", 0), (124, "sensitivity", 0.5), (140, "onset_window", 2)]
    hops = stream(B * nb, N, seed=5)
    an = gpu_fx.BatchAnalyser(C, N)
    st = gpu_fx.HopStream(an, B, slots=3)
    got = []
    for b in range(nb):
        for e in ev:
            if e[0] == b * B:
                apply(an, e)
        if st.in_flight() == 3:
            got.append(st.collect())
        st.push(hops[:, b * B:(b + 1) * B])
    while st.in_flight():
        got.append(st.collect())
    st.close()
    an.close()
    raw = np.concatenate([g[0] for g in got], 1)
    sm = np.concatenate([g[1] for g in got], 1)
    check(raw, sm, ev, 0, 3, "ring, graph=%s" % graph)
