"""Per-track gain and onset settings inside one context (fx_set_channel_gains / fx_set_channel_onset / fx_get_channel_settings).

The rule under test: a context on which no per-track setter was ever called runs exactly the code it ran before, and a track with
per-track settings produces, bit for bit, what it produces in a context that has those settings context-wide.  Every track of a mixed
context is held to the oracle's Channel given that track's settings (values within test_gpu_parity's ulp BUDGET) and to the
reference's tail (tests/tail_model.py, bit for bit, with that track's events), through every entry point and kernel family."""
import numpy as np
import pytest

import dispatch_paths as dp
import signals
import tail_model
import taps_model
from test_gpu_parity import BUDGET

pytestmark = pytest.mark.gpu

C = 8
GAINS = np.array([1.0, 0.0, -0.7, 0.5, 2.0, 0.25, 1.5, 0.9], np.float32)
SENS = np.array([0.7, 0.3, 0.0, 0.2, 0.5, 0.1, 0.15, 0.3], np.float32)
WINDOWS = np.array([1, 3, 5, 21, 32, 5, 3, 21], np.int32)
TYPES = np.array([0, 1, 2, 1, 0, 2, 1, 0], np.int32)
MASKS = {"both": 3, "spectral": 1, "harmonic": 2}


def _mixed(an):
    an.set_channel_gains(GAINS)
    an.set_channel_onset(SENS, WINDOWS, TYPES)


def _events(c, at=0):
    return [(at, "gain", float(GAINS[c])), (at, "onset_window", int(WINDOWS[c])), (at, "sensitivity", float(SENS[c])), (at, "onset_type", int(TYPES[c]))]


def _oracle_tracks(oracle, N, analysers=3):
    chans = [oracle.Channel(N) for _ in range(C)]
    for c, ch in enumerate(chans):
        ch.set_analysers(analysers)
        ch.set_gain(float(GAINS[c]))
        ch.set_onset_sensitivity(float(SENS[c]))
        ch.set_onset_window(int(WINDOWS[c]))
        ch.set_onset_type(int(TYPES[c]))
    return chans


def _push_all(chans, hops):
    outs = [ch.push_hops(hops[c]) for c, ch in enumerate(chans)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def _check(raw, sm, oraw, osm, events_of, analysers, what, need_onsets=False):
    signals.assert_features_within(raw, oraw, BUDGET, signals.SLOTS, what + " raw")
    signals.assert_features_within(sm, osm, BUDGET, signals.SLOTS, what + " smoothed")
    onsets = [tail_model.assert_tail_exact(raw[c:c + 1], sm[c:c + 1], events_of(c), analysers=analysers, what="%s track %d" % (what, c))
              for c in range(raw.shape[0])]
    if need_onsets:
        types = {int(TYPES[c]) for c in range(C) if onsets[c] > 0}
        assert len(types) >= 2, "%s: onsets per track %s: the case must contain onsets on tracks of different types" % (what, onsets)
    return onsets


def _feed(gpu_fx, an, entry, hops, per):
    """the whole stream through one entry point, `per` hops (samples for 'samples') per call -> (raw, smoothed) of the frames analysed"""
    outs = []
    if entry == "hops":
        for t in range(0, hops.shape[1], per):
            outs.append(an.push_hops(np.ascontiguousarray(hops[:, t:t + per])))
    elif entry == "samples":
        flat = hops.reshape(hops.shape[0], -1)
        for at in range(0, flat.shape[1], per):
            outs.append(an.push_samples(np.ascontiguousarray(flat[:, at:at + per])))
    else:
        st = gpu_fx.HopStream(an, per, slots=3, dtype=hops.dtype)
        for t in range(0, hops.shape[1], per):
            if st.in_flight() == 2:
                outs.append(st.collect())
            st.push(np.ascontiguousarray(hops[:, t:t + per]))
        while st.in_flight():
            outs.append(st.collect())
        st.close()
    return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1)


# id, N, entry, per call, hops in the stream, analyser kwargs, tuning
CASES = [("hops-1-%d" % N, N, "hops", 1, 56, {}, {}) for N in (256, 1024, 2048, 4096)]
CASES += [("hops-2-%d" % N, N, "hops", 2, 56, {}, {}) for N in (256, 1024, 2048, 4096)]
CASES += [("hops-14-%d" % N, N, "hops", 14, 56, {}, {}) for N in (256, 1024, 2048, 4096)]
CASES += [
    ("frame-tail-1024", 1024, "hops", 1, 56, {}, {"one_hop_kernel": 0}),
    ("frame-tail-4096", 4096, "hops", 1, 56, {}, {"one_hop_kernel": 0}),
    ("cut-in-time-1024", 1024, "hops", 300, 300, {}, {}),
    ("cut-in-time-2048", 2048, "hops", 130, 130, {}, {}),
    ("blocks-480-1024", 1024, "samples", 480, 56, {}, {}),
    ("blocks-480-2048", 2048, "samples", 480, 56, {}, {}),
    ("blocks-1000-1024", 1024, "samples", 1000, 56, {}, {}),
    ("blocks-2500-1024", 1024, "samples", 2500, 56, {}, {}),
    ("low-latency-14-2048", 2048, "hops", 14, 56, {"low_latency": True}, {}),
    ("low-latency-14-4096", 4096, "hops", 14, 56, {"low_latency": True}, {}),
    ("low-latency-1-2048", 2048, "hops", 1, 56, {"low_latency": True}, {}),
    ("low-latency-1-4096", 4096, "hops", 1, 56, {"low_latency": True}, {}),
    ("spectral-only-14-1024", 1024, "hops", 14, 56, {"analysers": "spectral"}, {}),
    ("spectral-only-1-2048", 2048, "hops", 1, 56, {"analysers": "spectral"}, {}),
    ("ring-graph-1024", 1024, "ring", 1, 56, {}, {"stream_hop_kernel": 0}),
    ("ring-graph-4-512", 512, "ring", 4, 56, {}, {}),
    ("ring-hop-1024", 1024, "ring", 1, 56, {}, {}),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mixed_tracks_match_the_oracle(gpu_fx, oracle, case):
    name, N, entry, per, T, kw, tuning = case
    hops = signals.bursts(C, T, N, seed=41)
    an = gpu_fx.BatchAnalyser(C, N, **kw)
    if tuning:
        an.set_tuning(**tuning)
    _mixed(an)
    raw, sm = _feed(gpu_fx, an, entry, hops, per)
    an.close()
    frames = raw.shape[1]
    assert frames == T
    mask = MASKS[kw.get("analysers", "both")]
    oraw, osm = _push_all(_oracle_tracks(oracle, N, mask), hops[:, :frames])
    _check(raw, sm, oraw, osm, _events, mask, name, need_onsets=True)


@pytest.mark.parametrize("N,per,kw", [(1024, 1, {}), (1024, 14, {}), (256, 3, {}), (4096, 1, {}), (2048, 14, {"low_latency": True}),
                                      (2048, 1, {"low_latency": True}), (1024, 14, {"analysers": "spectral"})])
def test_each_track_is_bit_identical_to_a_context_with_its_settings_context_wide(gpu_fx, N, per, kw):
    T = 42
    hops = signals.bursts(C, T, N, seed=43)
    an = gpu_fx.BatchAnalyser(C, N, **kw)
    _mixed(an)
    raw, sm = _feed(gpu_fx, an, "hops", hops, per)
    an.close()
    for c in range(C):
        one = gpu_fx.BatchAnalyser(C, N, **kw)
        one.set_gain(float(GAINS[c]))
        one.set_onset_detection_sensitivity(float(SENS[c]))
        one.set_onset_window_length(int(WINDOWS[c]))
        one.set_onset_detection_type(int(TYPES[c]))
        wraw, wsm = _feed(gpu_fx, one, "hops", hops, per)
        one.close()
        assert np.array_equal(raw[c].view(np.uint32), wraw[c].view(np.uint32)), "raw of track %d" % c
        assert np.array_equal(sm[c].view(np.uint32), wsm[c].view(np.uint32)), "smoothed of track %d" % c


@pytest.mark.parametrize("N,entry,per", [(1024, "hops", 1), (1024, "hops", 14), (2048, "samples", 480), (512, "ring", 4)])
def test_defaults_per_track_are_bit_identical_to_no_call(gpu_fx, N, entry, per):
    hops = signals.bursts(C, 56, N, seed=44)
    plain = gpu_fx.BatchAnalyser(C, N)
    want = _feed(gpu_fx, plain, entry, hops, per)
    defaults = plain.channel_settings()
    plain.close()
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_channel_gains(defaults["gain"])
    an.set_channel_onset(defaults["sensitivity"], defaults["window"], defaults["type"])
    got = _feed(gpu_fx, an, entry, hops, per)
    an.close()
    assert np.array_equal(defaults["gain"], np.ones(C, np.float32)) and np.array_equal(defaults["window"], np.full(C, 5))
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("N,per", [(1024, 1), (1024, 6), (2048, 2)])
def test_per_track_settings_changed_mid_stream(gpu_fx, oracle, N, per):
    """test_gpu_parity.test_settings_changed_mid_stream per track: two tracks' windows (track 3 to the length it already has: its histories
    still empty), another's gain, the rest left alone (window < 0); then a context-wide set_gain overrides every track's."""
    T0, T1, T2 = 18, 36, 54
    hops = signals.bursts(C, T2, N, seed=45)
    an = gpu_fx.BatchAnalyser(C, N)
    chans = _oracle_tracks(oracle, N)
    _mixed(an)
    got, want = [], []

    def both(lo, hi):
        got.append(_feed(gpu_fx, an, "hops", hops[:, lo:hi], per))
        want.append(_push_all(chans, hops[:, lo:hi]))

    both(0, T0)
    windows = np.full(C, -1, np.int32)
    windows[3] = WINDOWS[3]
    windows[6] = 8
    gains = GAINS.copy()
    gains[5] = -1.25
    an.set_channel_onset(window=windows)
    an.set_channel_gains(gains)
    chans[3].set_onset_window(int(WINDOWS[3]))
    chans[6].set_onset_window(8)
    chans[5].set_gain(-1.25)
    s = an.channel_settings()
    assert np.array_equal(s["window"], np.where(windows > 0, windows, WINDOWS)) and np.array_equal(s["gain"], gains)
    assert np.array_equal(s["sensitivity"], SENS) and np.array_equal(s["type"], TYPES)
    both(T0, T1)
    an.set_gain(0.5)
    [ch.set_gain(0.5) for ch in chans]
    assert np.array_equal(an.channel_settings()["gain"], np.full(C, 0.5, np.float32))
    both(T1, T2)
    an.close()
    raw, sm = (np.concatenate([g[k] for g in got], axis=1) for k in (0, 1))
    oraw, osm = (np.concatenate([w[k] for w in want], axis=1) for k in (0, 1))

    def events_of(c):
        ev = _events(c)
        if c in (3, 6):
            ev.append((T0, "onset_window", int(WINDOWS[3]) if c == 3 else 8))
        return ev + [(T1, "gain", 0.5)]

    _check(raw, sm, oraw, osm, events_of, 3, "mid-stream %d/%d" % (N, per))
    # track 3's histories really were emptied: its detector cannot fire for window - 1 frames after the change
    assert not raw[3, T0:T0 + int(WINDOWS[3]) - 1, 0].any()


def test_ring_graph_route_sees_the_table_appear_and_change(gpu_fx, oracle):
    """The captured step (hipGraph) of a ring: per-track settings made after the step was captured, then changed again, reach the
    replayed step in stream order."""
    N, T = 1024, 60
    hops = signals.bursts(C, T, N, seed=46)
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_tuning(stream_hop_kernel=0)
    chans = [oracle.Channel(N) for _ in range(C)]
    st = gpu_fx.HopStream(an, 1, slots=3, dtype=hops.dtype)
    outs, want = [], []

    def push(lo, hi):
        want.append(_push_all(chans, hops[:, lo:hi]))       # the oracle's tracks, with the settings they have now
        for t in range(lo, hi):
            if st.in_flight() == 2:
                outs.append(st.collect())
            st.push(np.ascontiguousarray(hops[:, t:t + 1]))
        assert [l["kind"] for l in an.last_launches()] == ["frame", "epilogue"]      # the captured step's launches

    push(0, 20)
    _mixed(an)
    for c, ch in enumerate(chans):
        ch.set_gain(float(GAINS[c])), ch.set_onset_sensitivity(float(SENS[c])), ch.set_onset_window(int(WINDOWS[c])), ch.set_onset_type(int(TYPES[c]))
    push(20, 40)
    gains = GAINS[::-1].copy()
    an.set_channel_gains(gains)
    [ch.set_gain(float(gains[c])) for c, ch in enumerate(chans)]
    push(40, T)
    while st.in_flight():
        outs.append(st.collect())
    st.close()
    an.close()
    raw, sm = (np.concatenate([o[k] for o in outs], axis=1) for k in (0, 1))
    oraw, osm = (np.concatenate([w[k] for w in want], axis=1) for k in (0, 1))
    _check(raw, sm, oraw, osm, lambda c: _events(c, 20) + [(40, "gain", float(gains[c]))], 3, "ring graph route")


@pytest.mark.parametrize("N,per", [(1024, 1), (1024, 14), (4096, 2)])
def test_a_change_on_one_track_leaves_the_others_bit_identical(gpu_fx, N, per):
    T, k = 28, 3
    hops = signals.bursts(C, T, N, seed=47)
    a = gpu_fx.BatchAnalyser(C, N)
    _mixed(a)
    base = _feed(gpu_fx, a, "hops", hops, per)
    a.close()
    for gain_k in (3.0, np.nan, np.inf, -np.inf):
        b = gpu_fx.BatchAnalyser(C, N)
        _mixed(b)
        gains, sens, windows, types = GAINS.copy(), SENS.copy(), WINDOWS.copy(), TYPES.copy()
        gains[k], sens[k], windows[k], types[k] = gain_k, 0.05, 2, 2
        b.set_channel_gains(gains)
        b.set_channel_onset(sens, windows, types)
        got = _feed(gpu_fx, b, "hops", hops, per)
        b.close()
        others = [c for c in range(C) if c != k]
        for g, w in zip(got, base):
            assert np.array_equal(g[others].view(np.uint32), w[others].view(np.uint32)), gain_k
        assert not np.array_equal(got[0][k], base[0][k], equal_nan=True)
        if not np.isfinite(gain_k):
            assert np.isnan(got[0][k, :, 1]).any()                      # the poisoned track's RMS is NaN, as in the reference


@pytest.mark.parametrize("N,entry", [(1024, "hops"), (2048, "hops"), (1024, "samples")])
def test_taps_show_the_armed_tracks_own_gain(gpu_fx, oracle, N, entry):
    H = N // 2
    hops = signals.tone_vibrato_noise(C, 6, N, seed=48)
    an = gpu_fx.BatchAnalyser(C, N)
    _mixed(an)
    armed = [2, 4, 7]
    if entry == "hops":
        an.push_hops(hops[:, :3])
        an.request_taps(armed)
        an.push_hops(np.ascontiguousarray(hops[:, 3:4]))
    else:
        flat = hops.reshape(C, -1)
        an.push_samples(np.ascontiguousarray(flat[:, :3 * H + 100]))
        an.request_taps(armed)
        an.push_samples(np.ascontiguousarray(flat[:, 3 * H + 100:4 * H + 50]))
    for c in armed:
        got = an.taps(c)
        assert got["frame_index"] == 3
        window = np.concatenate([hops[c, 2] * GAINS[c], hops[c, 3] * GAINS[c]]).astype(np.float32)
        taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, window), "track %d" % c)
    an.close()


def test_osc_datagrams_of_a_mixed_context(gpu_fx):
    N = 1024
    hops = signals.bursts(C, 30, N, seed=49)
    an = gpu_fx.BatchAnalyser(C, N)
    _mixed(an)
    raw, sm = an.push_hops(hops)
    d, n = an.osc_datagrams("/Audio/A", 0)
    an.close()
    for c in range(C):
        assert bytes(d[c, :n[c]]) == gpu_fx.capi.osc_encode("/Audio/A%d" % c, sm[c, -1]), c


DISPATCH_ROWS = ["batch-1024", "hop-1024", "frame-tail-2048", "two-hop-4096", "fused-tail-256", "cut-default-1024", "frames-1024",
                 "block-batch-1024-f32", "reblock-1-1024-f32", "ring-hop-1024", "ring-graph-1024", "ring-queues-12-2048", "cut-pair-2048",
                 "spectral-256"]


@pytest.mark.parametrize("rid", DISPATCH_ROWS)
def test_launch_sequences_are_the_dispatch_tables_with_per_track_settings(gpu_fx, rid):
    import torch
    import test_gpu_dispatch as tgd
    if torch.cuda.get_device_properties(0).multi_processor_count != dp.CUS:
        pytest.skip("the table's launch sequences are written for %d CUs" % dp.CUS)
    r = [x for x in dp.ROWS if x.id == rid][0]
    _, pieces = tgd._plan(r)
    an = tgd._analyser(gpu_fx, r)
    rng = np.random.default_rng(5)
    an.set_channel_gains(rng.uniform(-2, 2, r.C).astype(np.float32))
    an.set_channel_onset(rng.uniform(0, 1, r.C).astype(np.float32), rng.integers(1, 33, r.C).astype(np.int32), rng.integers(0, 3, r.C).astype(np.int32))
    if r.entry == "ring":
        outs, records = tgd._run_ring(gpu_fx, an, r, pieces)
    else:
        outs, records, _ = tgd._run_calls(gpu_fx, an, r, pieces)
    an.close()
    tgd._check_launches(r, records, [o[0].shape[1] for o in outs])


def test_channel_settings_round_trip(gpu_fx):
    an = gpu_fx.BatchAnalyser(C, 1024)
    s = an.channel_settings()
    assert np.array_equal(s["gain"], np.ones(C, np.float32)) and np.array_equal(s["sensitivity"], np.full(C, 0.7, np.float32))
    assert np.array_equal(s["window"], np.full(C, 5)) and np.array_equal(s["type"], np.full(C, 1))
    an.set_onset_detection_sensitivity(0.25)            # context-wide, before any table exists
    assert np.array_equal(an.channel_settings()["sensitivity"], np.full(C, 0.25, np.float32))
    _mixed(an)
    s = an.channel_settings()
    assert np.array_equal(s["gain"], GAINS) and np.array_equal(s["sensitivity"], SENS)
    assert np.array_equal(s["window"], WINDOWS) and np.array_equal(s["type"], TYPES)
    an.set_channel_onset(window=np.full(C, -1, np.int32))           # leaves everything alone
    assert np.array_equal(an.channel_settings()["window"], WINDOWS)
    # a bad entry names its track and changes nothing
    bad = WINDOWS.copy()
    bad[5] = 33
    with pytest.raises(gpu_fx.FxError, match="track 5"):
        an.set_channel_onset(SENS * 2, bad, TYPES)
    with pytest.raises(gpu_fx.FxError, match="track 2"):
        an.set_channel_onset(np.where(np.arange(C) == 2, np.nan, SENS).astype(np.float32))
    with pytest.raises(gpu_fx.FxError, match="track 7"):
        an.set_channel_onset(type=np.where(np.arange(C) == 7, 3, TYPES).astype(np.int32))
    assert np.array_equal(an.channel_settings()["sensitivity"], SENS)
    # the context-wide setters set every track
    an.set_gain(0.5)
    an.set_onset_window_length(7)
    an.set_onset_detection_type(2)
    an.set_onset_detection_sensitivity(0.1)
    s = an.channel_settings()
    assert np.array_equal(s["gain"], np.full(C, 0.5, np.float32)) and np.array_equal(s["sensitivity"], np.full(C, 0.1, np.float32))
    assert np.array_equal(s["window"], np.full(C, 7)) and np.array_equal(s["type"], np.full(C, 2))
    an.reset_state()                                    # settings are kept
    assert np.array_equal(an.channel_settings()["window"], np.full(C, 7))
    an.close()


def test_reset_state_keeps_per_track_settings_and_restarts_the_histories(gpu_fx, oracle):
    N, T = 1024, 30
    hops = signals.bursts(C, T, N, seed=50)
    an = gpu_fx.BatchAnalyser(C, N)
    _mixed(an)
    first = an.push_hops(hops)
    an.reset_state()
    again = an.push_hops(hops)
    an.close()
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
