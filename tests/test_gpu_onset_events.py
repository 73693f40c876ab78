"""The onset event list on the device (include/fx.h, fx_enable_onset_events / fx_get_onset_events).

The expected list is never taken from the list itself: it is the (frame, channel) order of the ones in column 0 of the call's own
raw output and, independently, of the oracle's Channel.push_hops per track (tests/onset_events_model.py turns either into the
list).  Onset is a discrete slot: the comparison is exact, every field, in order.

Main setup: signals.bursts(C, T, N); even tracks spectral type, sensitivity 0.2, window 3 (fx_set_channel_onset), odd tracks at the
defaults; C = 200 / 130 cross 64-lane groups and leave a ragged last group.  Before any case looks at the GPU it asserts that the
expected list is worth looking at: at least 100 events, events in at least half of the frames, a frame with events in two different
64-channel groups."""
import numpy as np
import pytest

import dispatch_paths as dp
import onset_events_model as om
import signals

pytestmark = pytest.mark.gpu

SHAPES = [(1024, 200, 56), (2048, 130, 40), (256, 200, 120)]          # N, C, T
BIG = 1 << 20


def _track_settings(C):
    even = np.arange(C) % 2 == 0
    return (np.where(even, 0.2, 0.7).astype(np.float32), np.where(even, 3, 5).astype(np.int32), np.where(even, 0, 1).astype(np.int32))


def _mixed(an):
    an.set_channel_onset(*_track_settings(an.num_channels))


_ORACLE = {}


def _oracle_flags(oracle, N, C, T, all_spectral=False):
    """[C][T] onset column of the oracle, one Channel per track with that track's settings"""
    key = (N, C, T, all_spectral)
    if key not in _ORACLE:
        hops = signals.bursts(C, T, N)
        sens, window, types = _track_settings(C)
        flags = np.empty((C, T), np.float32)
        for c in range(C):
            ch = oracle.Channel(N)
            k = 0 if all_spectral else c
            ch.set_onset_sensitivity(float(sens[k]))
            ch.set_onset_window(int(window[k]))
            ch.set_onset_type(int(types[k]))
            flags[c] = ch.push_hops(hops[c])[0][:, 0]
        _ORACLE[key] = flags
    return _ORACLE[key]


def _worth_looking_at(events, T, what):
    """the issue's three conditions on an EXPECTED list"""
    assert len(events) >= 100, "%s: only %d events expected" % (what, len(events))
    frames = {}
    for f, c, _ in events:
        frames.setdefault(f, set()).add(c // 64)
    assert 2 * len(frames) >= T, "%s: events in %d of %d frames" % (what, len(frames), T)
    assert any(len(g) >= 2 for g in frames.values()), "%s: no frame has events in two 64-channel groups" % what


def _windows(hops):
    C, T, H = hops.shape
    x = np.concatenate([np.zeros((C, 1, H), hops.dtype), hops], axis=1)
    return np.ascontiguousarray(np.concatenate([x[:, :-1], x[:, 1:]], axis=2))


def _pieces(hops, entry, per):
    """the stream cut into the calls of one path: per = hops (frames) per call, or samples per block"""
    C, T, H = hops.shape
    if entry == "hops":
        return [np.ascontiguousarray(hops[:, t:t + per]) for t in range(0, T, per)]
    if entry == "frames":
        w = _windows(hops)
        return [np.ascontiguousarray(w[:, t:t + per]) for t in range(0, T, per)]
    flat = hops.reshape(C, -1)
    cut = [np.ascontiguousarray(flat[:, at:at + per]) for at in range(0, flat.shape[1], per)]
    return [np.ascontiguousarray(p.T) for p in cut] if entry == "interleaved" else cut


def _call(an, entry, piece, device, want_raw):
    if device:
        import torch
        piece = torch.from_numpy(piece).cuda()
    fn = {"hops": an.push_hops, "frames": an.process_frames, "samples": an.push_samples, "interleaved": an.push_interleaved}[entry]
    raw, sm = fn(piece, want_raw=want_raw)
    if device:
        raw, sm = (None if raw is None else raw.cpu().numpy()), sm.cpu().numpy()
    return raw, sm


def _run(an, entry, pieces, device=False, want_raw=True, drain_each=False):
    """-> (raw or None, smoothed, drains [(events as tuples, dropped)], frames per call)"""
    raws, sms, drains, frames = [], [], [], []
    for piece in pieces:
        raw, sm = _call(an, entry, piece, device, want_raw)
        raws.append(raw), sms.append(sm), frames.append(sm.shape[1])
        if drain_each:
            ev, lost = an.onset_events()
            drains.append((om.as_tuples(ev), lost))
    if not drain_each:
        ev, lost = an.onset_events()
        drains.append((om.as_tuples(ev), lost))
    raw = np.concatenate(raws, axis=1) if want_raw else None
    return raw, np.concatenate(sms, axis=1), drains, frames


def _expected_by_call(flags, frames):
    """the list of a stream whose calls analysed `frames` frames each: call by call (call_frame restarts with every call)"""
    out, at = [], 0
    for t in frames:
        out += om.events_of_call(flags[:, at:at + t], at)
        at += t
    return out


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# entry, per call, device buffers, want_raw
PATHS = [("hops", 1, False, True), ("hops", 2, False, True), ("hops", 14, False, True), ("hops", None, False, True),
         ("hops", 1, True, True), ("hops", 14, True, True), ("hops", 2, True, False), ("hops", 14, False, False),
         ("frames", 1, False, True), ("frames", 14, False, True), ("frames", 2, True, True),
         ("samples", 480, False, True), ("samples", 480, True, True), ("samples", 480, False, False), ("samples", 480, True, False),
         ("interleaved", 480, False, True), ("interleaved", 480, True, False)]
CASES = [(N, C, T, {}) + p for (N, C, T) in SHAPES for p in PATHS]
CASES += [(2048, 130, 40, {"low_latency": True}) + p for p in [("hops", 1, False, True), ("hops", 2, True, True), ("hops", 14, False, False),
                                                                 ("samples", 480, False, True)]]


def _case_id(c):
    N, C, T, kw, entry, per, device, want_raw = c
    return "%d-%s%s-%s-%s%s" % (N, "ll-" if kw else "", entry, "all" if per is None else per, "device" if device else "host", "" if want_raw else "-noraw")


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_list_equals_the_column_and_results_are_untouched(gpu_fx, oracle, case):
    N, C, T, kw, entry, per, device, want_raw = case
    what = _case_id(case)
    hops = signals.bursts(C, T, N)
    oflags = _oracle_flags(oracle, N, C, T)
    _worth_looking_at(om.events_of_call(oflags), T, what)               # before anything runs on the GPU
    pieces = _pieces(hops, entry, T if per is None else per)

    # a context that never enabled the list, on the same stream through the same calls: the yardstick for the result bits
    plain = gpu_fx.BatchAnalyser(C, N, **kw)
    _mixed(plain)
    praws, psms = zip(*[_call(plain, entry, p, device, True) for p in pieces])
    plain_raw, plain_sm = np.concatenate(praws, axis=1), np.concatenate(psms, axis=1)
    plain_latest = plain.get_features()
    plain.close()
    assert plain_raw.shape[1] == T or entry in ("samples", "interleaved")
    frames_total = plain_raw.shape[1]

    each = gpu_fx.BatchAnalyser(C, N, **kw)
    _mixed(each)
    each.enable_onset_events(BIG)
    raw_a, sm_a, drains_a, frames = _run(each, entry, pieces, device, want_raw, drain_each=True)
    latest_a = each.get_features()
    each.close()
    once = gpu_fx.BatchAnalyser(C, N, **kw)
    _mixed(once)
    once.enable_onset_events(BIG)
    raw_b, sm_b, drains_b, frames_b = _run(once, entry, pieces, device, want_raw, drain_each=False)
    once.close()
    assert frames == frames_b and sum(frames) == frames_total

    # the expected list: from the run's own raw column (the plain context's where this one asked for none), and from the oracle
    column = (raw_a if want_raw else plain_raw)[:, :, 0]
    want = _expected_by_call(column, frames)
    want_oracle = _expected_by_call(oflags[:, :frames_total], frames)
    assert want == want_oracle, "%s: the GPU's onset column and the oracle's give different lists" % what
    _worth_looking_at(want, frames_total, what)
    got_each = [e for ev, _ in drains_a for e in ev]
    assert got_each == want, "%s: drained after every call" % what
    assert drains_b[0][0] == want, "%s: drained once at the end" % what
    assert all(lost == 0 for _, lost in drains_a + drains_b)
    # per call: a drain after call k holds exactly call k's events
    at = 0
    for (ev, _), t in zip(drains_a, frames):
        assert ev == om.events_of_call(column[:, at:at + t], at), "%s: call at frame %d" % (what, at)
        at += t

    # results are untouched, bit for bit
    if want_raw:
        assert _same_bits(raw_a, plain_raw) and _same_bits(raw_b, plain_raw), what
    assert _same_bits(sm_a, plain_sm) and _same_bits(sm_b, plain_sm), what
    assert _same_bits(latest_a, plain_latest), what


def test_frame_is_the_taps_frame_index(gpu_fx, oracle):
    N, C, T = SHAPES[0]
    hops = signals.bursts(C, T, N)
    want = om.events_of_call(_oracle_flags(oracle, N, C, T))
    f, c, _ = [e for e in want if e[0] >= 10][0]
    an = gpu_fx.BatchAnalyser(C, N)
    _mixed(an)
    an.enable_onset_events(BIG)
    an.push_hops(np.ascontiguousarray(hops[:, :f]))
    an.onset_events()
    an.request_taps([c])
    an.push_hops(np.ascontiguousarray(hops[:, f:f + 3]))
    assert [l["kind"] for l in an.last_launches()][0] == "taps" and an.last_launches()[-1]["kind"] == "onset_events"
    ev, _ = an.onset_events()
    frame_index = an.taps(c)["frame_index"]
    an.close()
    mine = [e for e in om.as_tuples(ev) if e[1] == c]
    assert frame_index == f and mine[0] == (f, c, 0), (frame_index, mine[:2])


# ---- nothing moves when it is off; exactly one more launch when it is on ----
PLAIN_TOO = {"batch-1024", "hop-1024", "frame-tail-2048", "two-hop-4096", "fused-tail-256", "cut-default-1024", "frames-1024",
             "block-batch-1024-f32", "reblock-1-1024-f32", "block-hop-1024-f32", "block-two-hop-2048-s16", "pair-2048", "harmonic-1024",
             "direct-256", "two-hop-direct-1024"}
CALL_ROWS = [r for r in dp.ROWS if r.entry != "ring"]


@pytest.mark.parametrize("r", CALL_ROWS, ids=[r.id for r in CALL_ROWS])
def test_launches_with_the_list_off_and_on(gpu_fx, r):
    import torch
    import test_gpu_dispatch as tgd
    if torch.cuda.get_device_properties(0).multi_processor_count != dp.CUS:
        pytest.skip("the table's launch sequences are written for %d CUs" % dp.CUS)
    _, pieces = tgd._plan(r)
    if r.id in PLAIN_TOO:
        an = tgd._analyser(gpu_fx, r)
        outs, records, _ = tgd._run_calls(gpu_fx, an, r, pieces)
        an.close()
        tgd._check_launches(r, records, [o[0].shape[1] for o in outs])            # what it is today
    an = tgd._analyser(gpu_fx, r)
    an.enable_onset_events(BIG)
    outs, records, _ = tgd._run_calls(gpu_fx, an, r, pieces)
    ev, lost = an.onset_events()
    an.close()
    frames = [o[0].shape[1] for o in outs]
    stripped = []
    for rec, t in zip(records, frames):
        if t == 0:
            assert all(l["kind"] != "onset_events" for l in rec), (r.id, rec)       # a call that completes no hop launches nothing more
            stripped.append(rec)
            continue
        assert [l["kind"] for l in rec].count("onset_events") == 1 and rec[-1]["kind"] == "onset_events", (r.id, rec)
        last = rec[-1]
        assert last["T"] == t and last["window"] == r.N, (r.id, last)
        assert all(v == 0 for k, v in last.items() if k not in ("kind", "T", "window")), (r.id, last)
        stripped.append(rec[:-1])
    tgd._check_launches(r, stripped, frames)
    raw = np.concatenate([o[0] for o in outs], axis=1)
    assert lost == 0 and om.as_tuples(ev) == _expected_by_call(raw[:, :, 0], frames), r.id
    if r.analysers == "harmonic":
        assert len(ev) == 0, "%s: a FX_HARMONIC_ONLY context produced %d events" % (r.id, len(ev))


def test_harmonic_only_produces_no_event(gpu_fx):
    N, C, T = SHAPES[0]
    an = gpu_fx.BatchAnalyser(C, N, analysers="harmonic")
    an.enable_onset_events(BIG)
    for per in (1, 2, 14):
        an.push_hops(np.ascontiguousarray(signals.bursts(C, per, N)), want_raw=False)
    an.push_hops(signals.bursts(C, T, N))
    ev, lost = an.onset_events()
    an.close()
    assert len(ev) == 0 and lost == 0


def test_the_ring_produces_no_events(gpu_fx):
    N, C = 1024, 8
    hops = signals.bursts(C, 30, N)
    an = gpu_fx.BatchAnalyser(C, N)
    an.enable_onset_events(BIG)
    st = gpu_fx.HopStream(an, 1, slots=3, dtype=hops.dtype)
    outs = []
    for t in range(hops.shape[1]):
        if st.in_flight() == 2:
            outs.append(st.collect())
        st.push(np.ascontiguousarray(hops[:, t:t + 1]))
        assert all(l["kind"] != "onset_events" for l in an.last_launches())
    while st.in_flight():
        outs.append(st.collect())
    st.close()
    ev, lost = an.onset_events()
    an.close()
    assert np.concatenate([o[0] for o in outs], axis=1)[:, :, 0].sum() > 0          # there were onsets to miss
    assert len(ev) == 0 and lost == 0


# ---- overflow, partial drains, resize, reset ----
def test_overflow_and_partial_drains(gpu_fx, oracle):
    N, C, T = SHAPES[0]
    hops = signals.bursts(C, T, N)
    flags = _oracle_flags(oracle, N, C, T, all_spectral=True)
    want = om.events_of_call(flags)
    assert len([e for e in want if e[0] < 8]) > 64, "the spectral case must overflow 64 within the first few frames"

    def analyser(capacity):
        an = gpu_fx.BatchAnalyser(C, N)
        an.set_onset_detection_type(gpu_fx.ONSET_SPECTRAL)
        an.set_onset_detection_sensitivity(0.2)
        an.set_onset_window_length(3)
        an.enable_onset_events(capacity)
        return an

    for per in (1, 14, T):
        an = analyser(64)
        model = om.EventList(64)
        for t in range(0, T, per):
            raw, _ = an.push_hops(np.ascontiguousarray(hops[:, t:t + per]))
            assert np.array_equal(raw[:, :, 0], flags[:, t:t + per])
            model.call(flags[:, t:t + per])
        ev, lost = an.onset_events()
        mev, mlost = model.drain()
        assert om.as_tuples(ev) == mev and lost == mlost, per
        assert len(ev) == 64 and lost == len(want) - 64 and [e[:2] for e in mev] == [e[:2] for e in want[:64]], per
        ev, lost = an.onset_events()
        assert len(ev) == 0 and lost == 0, "a second drain must find nothing stored and nothing dropped"
        # the list has room again: the next calls' events are stored from its start, partial drains return consecutive slices
        an.reset_state()
        model.reset()
        for t in range(0, 6, 2):
            an.push_hops(np.ascontiguousarray(hops[:, t:t + 2]), want_raw=False)
            model.call(flags[:, t:t + 2])
            for _ in range(2):
                ev, lost = an.onset_events(10)
                assert (om.as_tuples(ev), lost) == model.drain(10), (per, t)
        rest, lost = an.onset_events()
        assert (om.as_tuples(rest), lost) == model.drain(None)
        an.close()

    # cap = 10, the stream fed three times over without a reset: consecutive slices, in order, while the ring goes round (and
    # overflows when the drains fall behind).  The model is driven by the calls' own raw column here: the oracle's stream ended.
    an = analyser(300)
    model = om.EventList(300)
    got = 0
    for rounds in range(3):
        for t in range(0, T, 7):
            raw, _ = an.push_hops(np.ascontiguousarray(hops[:, t:t + 7]))
            model.call(raw[:, :, 0])
            for _ in range(2):
                ev, lost = an.onset_events(10)
                assert (om.as_tuples(ev), lost) == model.drain(10), (rounds, t)
                got += len(ev)
        while True:
            ev, lost = an.onset_events(10)
            assert (om.as_tuples(ev), lost) == model.drain(10), rounds
            got += len(ev)
            if len(ev) < 10:
                break
    assert got > 2 * 300                         # the ring went round
    an.reset_state()
    # resizing drops what is stored; the stream's frame count goes on
    raw, _ = an.push_hops(np.ascontiguousarray(hops[:, :35]))
    assert raw[:, :, 0].sum() > 300
    an.enable_onset_events(5000)
    ev, lost = an.onset_events()
    assert len(ev) == 0 and lost == 0
    raw, _ = an.push_hops(np.ascontiguousarray(hops[:, 35:42]))
    ev, lost = an.onset_events()
    assert om.as_tuples(ev) == om.events_of_call(raw[:, :, 0], 35) and lost == 0 and len(ev) > 0
    # fx_reset_state empties the list, zeroes dropped and restarts `frame` at 0; the list stays enabled at its capacity
    an.enable_onset_events(64)
    an.push_hops(hops, want_raw=False)
    an.reset_state()
    raw, _ = an.push_hops(np.ascontiguousarray(hops[:, :4]))
    ev, lost = an.onset_events()
    fresh = om.events_of_call(raw[:, :, 0], 0)          # only this call's events, frames from 0; the overflow count is this call's own
    assert om.as_tuples(ev) == fresh[:64] and lost == max(0, len(fresh) - 64)
    # disabled: the entry refuses, analysis calls go on
    an.enable_onset_events(0)
    with pytest.raises(gpu_fx.FxError, match="not enabled"):
        an.onset_events()
    an.push_hops(np.ascontiguousarray(hops[:, 4:5]))
    assert all(l["kind"] != "onset_events" for l in an.last_launches())
    an.close()


def test_scale_once(gpu_fx, oracle):
    """65 536 tracks, one hop per call, 12 calls: count and (frame, channel) order against the column"""
    N, C, calls, base = 1024, 65536, 12, 256
    hops = signals.bursts(base, calls, N)
    per_tile = 0
    for k in range(base):
        ch = oracle.Channel(N)
        ch.set_onset_window(3)
        per_tile += int((ch.push_hops(hops[k])[0][:, 0] == 1).sum())
    assert per_tile >= 100, "the oracle finds %d onsets in one tile of %d tracks" % (per_tile, base)
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_onset_window_length(3)
    an.enable_onset_events(1 << 22)
    column = np.empty((C, calls), np.float32)
    for t in range(calls):
        raw, _ = an.push_hops(np.ascontiguousarray(np.tile(hops[:, t:t + 1], (C // base, 1, 1))))
        column[:, t] = raw[:, 0, 0]
        assert an.last_launches()[-1]["kind"] == "onset_events"
    ev, lost = an.onset_events()
    an.close()
    t, c = np.nonzero((column == 1).T)
    assert len(t) == per_tile * (C // base), "the column holds %d onsets, the oracle's tile times %d is %d" % (len(t), C // base, per_tile * (C // base))
    assert lost == 0 and len(ev) == len(t)
    assert np.array_equal(ev["frame"], t) and np.array_equal(ev["channel"], c) and not ev["call_frame"].any()
    order = ev["frame"].astype(np.int64) * C + ev["channel"]
    assert np.all(np.diff(order) > 0)
