"""Per-track reset and clear (fx_reset_channels / fx_clear_pending_channels / fx_get_channel_frames).

The two properties under test, both bit for bit (float bits compared as uint32, so NaN slots count):
  - after fx_reset_channels a listed track produces what the same track of a freshly created context with the same settings
    produces when that context is first given fx_pending_samples() zeros and then the same input;
  - every track not listed produces what it produces in a context where the call was never made.
They are held through every entry point, window size, analyser flag and call length, with resets at frame 0, inside the first ten
frames, inside an onset window's worth of frames of another reset and after the 48-row history ring has lapped, one track reset twice
and a list with a duplicate.  Reset tracks are also held to the CPU: their frames after the reset to a fresh oracle.Channel within
test_gpu_parity's ulp BUDGET, their whole raw / smoothed sequence to the reference's tail (tests/tail_model.py) with a "reset" event.

Worst figures seen: the bitwise comparisons have none (they are equal or the test fails); the oracle comparison uses
test_gpu_parity.BUDGET unchanged."""
import numpy as np
import pytest

import signals
import tail_model
from test_gpu_parity import BUDGET

pytestmark = pytest.mark.gpu

C = 6
GAINS = np.array([1.0, 0.5, -0.7, 2.0, 1.5, 0.25], np.float32)
SENS = np.array([0.7, 0.3, 0.1, 0.2, 0.5, 0.15], np.float32)
WINDOWS = np.array([5, 3, 1, 8, 21, 5], np.int32)
TYPES = np.array([1, 0, 2, 1, 0, 1], np.int32)
MASKS = {"both": 3, "spectral": 1, "harmonic": 2}
# frame position -> tracks: frame 0, inside the first ten frames, a second reset of track 1 nine frames after its first (inside its own
# onset / smoothing histories' fill), and after the ring has lapped (with a duplicate in the list).  Tracks 4 and 5 are never reset.
RESETS = {0: [0], 4: [1], 13: [2, 1], 55: [3, 3]}
NEVER = [4, 5]
# signals.bursts seed of the cases below, picked on the CPU with the oracle alone: with it every case that runs the spectral analyser has
# onsets after the last reset on at least two of the reset tracks (fresh oracle.Channel per track, fed the track's stream from its reset)
SEED = 85


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), "%s: %d of %d values differ" % (what, int((_bits(a) != _bits(b)).sum()), a.size)


def _plan(per, total, resets=RESETS, unit=1):
    """calls of `per` (hops, or samples when unit is the hop length) up to `total` hops, each reset placed at the first call boundary
    at or after its frame position"""
    plan, todo, at = [], sorted(resets.items()), 0
    while at < total * unit:
        while todo and todo[0][0] * unit <= at:
            plan.append(("reset", todo.pop(0)[1]))
        n = min(per, total * unit - at)
        plan.append(n)
        at += n
    return plan


class Feeder:
    """one context fed through one entry point; keeps a ring open across resets so that its captured step is replayed after them"""

    def __init__(self, fx, N, entry, kw, tuning, mixed, events=True):
        self.fx, self.N, self.H, self.entry = fx, N, N // 2, entry
        self.an = fx.BatchAnalyser(C, N, **kw)
        if tuning:
            self.an.set_tuning(**tuning)
        if mixed:
            self.an.set_channel_gains(GAINS)
            self.an.set_channel_onset(SENS, WINDOWS, TYPES)
        if events:
            self.an.enable_onset_events(1 << 16)
        self.ring = fx.HopStream(self.an, 1, slots=3) if entry == "ring" else None
        self.outs, self.calls = [], []          # per call: (raw, smoothed); frames per call

    def _keep(self, out):
        self.outs.append(out)
        self.calls.append(out[0].shape[1])

    def zeros(self, n):
        if n:
            out = self.an.push_samples(np.zeros((C, n), np.float32))
            assert out[0].shape[1] == 0

    def feed(self, x):
        """x [C][n] samples (whole hops unless the entry takes blocks)"""
        e, H = self.entry, self.H
        if e == "samples":
            self._keep(self.an.push_samples(np.ascontiguousarray(x)))
        elif e == "interleaved":
            self._keep(self.an.push_interleaved(np.ascontiguousarray(x.T)))
        elif e == "hops":
            self._keep(self.an.push_hops(np.ascontiguousarray(x.reshape(C, -1, H))))
        elif e == "ring":
            for t in range(x.shape[1] // H):
                self.ring.push(np.ascontiguousarray(x[:, t * H:(t + 1) * H]).reshape(C, 1, H))
                self._keep(self.ring.collect())
        else:
            raise ValueError(e)

    def feed_frames(self, frames):
        self._keep(self.an.process_frames(np.ascontiguousarray(frames)))

    def result(self):
        return np.concatenate([o[0] for o in self.outs], axis=1), np.concatenate([o[1] for o in self.outs], axis=1)

    def close(self):
        if self.ring:
            self.ring.close()
        self.an.close()


def _frames_of(hops):
    """assembled windows [C][T][N] of a hop stream (the overlapper starts with a zero tail)"""
    Cn, T, H = hops.shape
    prev = np.concatenate([np.zeros((Cn, 1, H), np.float32), hops[:, :-1]], axis=1)
    return np.ascontiguousarray(np.concatenate([prev, hops], axis=2))


def _run_plan(fx, N, entry, kw, tuning, mixed, flat, plan, frames=None, start=0, zeros=0, resets=True, stop=None):
    """feed flat[:, start:] (or frames[:, start:]) call by call as `plan` says, from plan position `start` (in samples; frames for the
    frames entry); resets=False skips them (the context where the call was never made).  Returns the feeder, closed, and per reset
    (plan index, samples fed before it, frames analysed before it, pending, tracks)."""
    f = Feeder(fx, N, entry, kw, tuning, mixed)
    f.zeros(zeros)
    at, marks, frames_done, H = 0, [], 0, N // 2
    pending = zeros
    for i, step in enumerate(plan):
        if isinstance(step, tuple):
            if at < start:
                continue
            if resets:
                before = f.an.channel_settings()
                f.an.reset_channels(step[1])
                after = f.an.channel_settings()
                assert all(before[k].tobytes() == after[k].tobytes() for k in before), "a reset changed a setting"
                assert f.an.pending_samples() == pending
            marks.append((i, at, frames_done, pending, list(step[1])))
            continue
        if at >= start:
            if entry == "frames":
                f.feed_frames(frames[:, at:at + step])
                frames_done += step
            else:
                f.feed(flat[:, at:at + step])
                frames_done += (pending + step) // H
                pending = (pending + step) % H
        at += step
        if stop is not None and at >= stop:
            break
    return f, marks


def _track_events(c, mixed, extra=()):
    ev = [(0, "gain", float(GAINS[c])), (0, "onset_window", int(WINDOWS[c])), (0, "sensitivity", float(SENS[c])), (0, "onset_type", int(TYPES[c]))] if mixed else []
    return ev + list(extra)


def _oracle_track(oracle, N, c, mixed, analysers, order):
    ch = oracle.Channel(N, order=order)
    ch.set_analysers(analysers)
    if mixed:
        ch.set_gain(float(GAINS[c])), ch.set_onset_sensitivity(float(SENS[c])), ch.set_onset_window(int(WINDOWS[c])), ch.set_onset_type(int(TYPES[c]))
    return ch


def _expected_events(raw, calls, first):
    """the list the contract promises from the raw onset column: earlier calls first, then call_frame, then channel; `first`
    [C][T] = the first frame of the track's stream at each global frame"""
    out, g0 = [], 0
    for n in calls:
        for t in range(n):
            for c in range(raw.shape[0]):
                if raw[c, g0 + t, 0] == 1.0:
                    out.append((g0 + t - first[c, g0 + t], c, t))
        g0 += n
    return out


def _check_case(fx, oracle, N, entry, kw, tuning, mixed, plan, total, seed=SEED):
    H = N // 2
    hops = signals.bursts(C, total, N, seed=seed)
    flat = np.ascontiguousarray(hops.reshape(C, -1))
    frames = _frames_of(hops) if entry == "frames" else None
    what = "%s N=%d %s %s" % (entry, N, kw, "mixed" if mixed else "plain")

    a, marks = _run_plan(fx, N, entry, kw, tuning, mixed, flat, plan, frames)
    raw, sm = a.result()
    got_events, dropped = a.an.onset_events()
    got_frames = a.an.channel_frames()
    calls = list(a.calls)
    a.close()
    T = raw.shape[1]
    assert dropped == 0 and T == (total if entry == "frames" else flat.shape[1] // H)

    # ---- tracks not listed: the context where the call was never made ----
    b, _ = _run_plan(fx, N, entry, kw, tuning, mixed, flat, plan, frames, resets=False)
    braw, bsm = b.result()
    b.close()
    first_reset = {}
    for _, _, fr, _, tracks in marks:
        for c in tracks:
            first_reset.setdefault(c, fr)
    for c in range(C):
        upto = first_reset.get(c, T)
        _same(raw[c, :upto], braw[c, :upto], "%s: raw of track %d before any reset of it" % (what, c))
        _same(sm[c, :upto], bsm[c, :upto], "%s: smoothed of track %d before any reset of it" % (what, c))
    assert all(c not in first_reset for c in NEVER)

    # ---- listed tracks: a fresh context given `pending` zeros, then the same input ----
    first = np.zeros((C, T), np.int64)
    resets_of = {c: [] for c in range(C)}
    for k, (i, at, fr, pending, tracks) in enumerate(marks):
        fresh, _ = _run_plan(fx, N, entry, kw, tuning, mixed, flat, plan, frames, start=at, zeros=pending, resets=False)
        fraw, fsm = fresh.result()
        fresh.close()
        assert fraw.shape[1] == T - fr, (what, fraw.shape, T, fr)
        for c in set(tracks):
            later = [m[2] for m in marks[k + 1:] if c in m[4]]
            end = later[0] if later else T
            _same(raw[c, fr:end], fraw[c, :end - fr], "%s: raw of track %d after its reset at frame %d" % (what, c, fr))
            _same(sm[c, fr:end], fsm[c, :end - fr], "%s: smoothed of track %d after its reset at frame %d" % (what, c, fr))
            first[c, fr:] = fr
            resets_of[c].append((fr, pending, at))

    # ---- frame counts and the event list ----
    assert np.array_equal(got_frames, T - first[:, -1] if T else np.zeros(C)), (what, got_frames)
    want_events = _expected_events(raw, calls, first) if entry != "ring" else []       # (the ring produces no events: include/fx.h)
    assert [(int(e["frame"]), int(e["channel"]), int(e["call_frame"])) for e in got_events] == want_events, what

    # ---- the CPU: a fresh oracle track per stream, the reference's tail with a "reset" event ----
    mask = MASKS[kw.get("analysers", "both")]
    order = int(kw.get("order", 0))
    onsets_after = 0
    for c in range(C):
        ev = _track_events(c, mixed, [(fr, "reset") for fr, _, _ in resets_of[c]])
        n = tail_model.assert_tail_exact(raw[c:c + 1], sm[c:c + 1], ev, order=order, analysers=mask, what="%s track %d" % (what, c))
        if resets_of[c]:
            fr = resets_of[c][-1][0]
            onsets_after += int(raw[c, fr:, 0].sum() > 0)
        if not resets_of[c]:
            continue
        fr, pending, at = resets_of[c][-1]
        ch = _oracle_track(oracle, N, c, mixed, mask, order)
        if entry == "frames":
            oraw, osm = ch.process_frames(frames[c, fr:])
        else:
            stream = np.concatenate([np.zeros(pending, np.float32), flat[c, at:]])
            oraw, osm = ch.push_hops(stream[:(stream.size // H) * H].reshape(-1, H))
        signals.assert_features_within(raw[c:c + 1, fr:], oraw[None], BUDGET, signals.SLOTS, "%s track %d raw after its last reset" % (what, c))
        signals.assert_features_within(sm[c:c + 1, fr:], osm[None], BUDGET, signals.SLOTS, "%s track %d smoothed after its last reset" % (what, c))
    return onsets_after


def _case(cid, N, entry, per, total=80, kw=None, tuning=None, mixed=False, plan=None):
    return (cid, N, entry, per, total, kw or {}, tuning or {}, mixed, plan)


LONG = [("reset", [0]), 130, ("reset", [1]), 7, ("reset", [2, 1]), 130, ("reset", [3, 3]), 3]       # 130: cut into work units, laps the ring
LL = {"low_latency": True}
CASES = [_case("hops-1-%d" % N, N, "hops", 1, mixed=N in (512, 2048)) for N in (256, 512, 1024, 2048, 4096)]
CASES += [_case("hops-2-%d" % N, N, "hops", 2, mixed=N == 1024) for N in (256, 1024, 4096)]
CASES += [_case("hops-7-%d" % N, N, "hops", 7, mixed=N == 512) for N in (512, 2048)]
CASES += [_case("hops-long-%d" % N, N, "hops", 0, total=270, plan=LONG, mixed=N == 1024) for N in (256, 1024, 2048)]
CASES += [
    _case("frame-tail-1024", 1024, "hops", 1, tuning={"one_hop_kernel": 0}, mixed=True),
    _case("harmonic-first-1-1024", 1024, "hops", 1, kw={"order": 1}),
    _case("harmonic-first-7-1024", 1024, "hops", 7, kw={"order": 1}, mixed=True),
    _case("isolated-2-2048", 2048, "hops", 2, kw={"order": 2}, mixed=True),
    _case("isolated-7-512", 512, "hops", 7, kw={"order": 2}),
    _case("spectral-only-1-256", 256, "hops", 1, kw={"analysers": "spectral"}, mixed=True),
    _case("spectral-only-7-1024", 1024, "hops", 7, kw={"analysers": "spectral"}),
    _case("harmonic-only-1-1024", 1024, "hops", 1, kw={"analysers": "harmonic"}),
    _case("harmonic-only-7-4096", 4096, "hops", 7, kw={"analysers": "harmonic"}, mixed=True),
    _case("low-latency-1-2048", 2048, "hops", 1, kw=LL, mixed=True),
    _case("low-latency-2-4096", 4096, "hops", 2, kw=LL),
    _case("low-latency-7-4096", 4096, "hops", 7, kw=LL, mixed=True),
    _case("low-latency-long-2048", 2048, "hops", 0, total=270, plan=LONG, kw=LL),
    _case("frames-1-1024", 1024, "frames", 1, mixed=True),
    _case("frames-2-256", 256, "frames", 2),
    _case("frames-7-2048", 2048, "frames", 7),
    _case("frames-long-1024", 1024, "frames", 0, total=270, plan=LONG),
    _case("samples-441-1024", 1024, "samples", 441, mixed=True),
    _case("samples-480-1024", 1024, "samples", 480),
    _case("samples-441-2048", 2048, "samples", 441),
    _case("samples-480-2048", 2048, "samples", 480, mixed=True),
    _case("samples-441-256", 256, "samples", 441, mixed=True),
    _case("samples-480-512", 512, "samples", 480),
    _case("samples-480-4096", 4096, "samples", 480),
    _case("samples-480-low-latency-2048", 2048, "samples", 480, kw=LL, mixed=True),
    _case("samples-441-spectral-1024", 1024, "samples", 441, kw={"analysers": "spectral"}),
    _case("interleaved-480-1024", 1024, "interleaved", 480, mixed=True),
    _case("interleaved-441-512", 512, "interleaved", 441),
    _case("ring-hop-1024", 1024, "ring", 1, mixed=True),
    _case("ring-hop-2048", 2048, "ring", 1),
    _case("ring-graph-1024", 1024, "ring", 1, tuning={"stream_hop_kernel": 0}),
    _case("ring-graph-4096", 4096, "ring", 1, tuning={"stream_hop_kernel": 0}, mixed=True),
    _case("ring-graph-low-latency-2048", 2048, "ring", 1, kw=LL, tuning={"stream_hop_kernel": 0}),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reset_tracks_are_fresh_and_the_others_untouched(gpu_fx, oracle, case):
    cid, N, entry, per, total, kw, tuning, mixed, plan = case
    H = N // 2
    # plans are in samples (in frames for fx_process_frames); `per` is hops per call for the hop entries
    unit = 1 if entry == "frames" else H
    step = per if entry in ("frames", "samples", "interleaved") else per * H
    plan = _plan(step, total, unit=unit) if plan is None else [s if isinstance(s, tuple) else s * unit for s in plan]
    onsets_after = _check_case(gpu_fx, oracle, N, entry, kw, tuning, mixed, plan, total)
    if MASKS[kw.get("analysers", "both")] & 1:
        assert onsets_after >= 2, "%s: the case must contain onsets after the reset on at least two tracks (%d)" % (cid, onsets_after)


def test_reset_of_every_track_is_reset_state_but_for_the_pending_count(gpu_fx):
    N, H = 1024, 512
    flat = np.ascontiguousarray(signals.bursts(C, 60, N, seed=72).reshape(C, -1))
    a = gpu_fx.BatchAnalyser(C, N)
    b = gpu_fx.BatchAnalyser(C, N)
    for an in (a, b):
        an.set_channel_gains(GAINS)
        an.push_hops(flat[:, :20 * H].reshape(C, 20, H))
    a.reset_channels(np.arange(C))
    b.reset_state()
    assert np.array_equal(a.channel_frames(), np.zeros(C)) and np.array_equal(b.channel_frames(), np.zeros(C))
    _same(a.get_features(), b.get_features(), "latest after the reset")
    for x, y in zip(a.push_hops(flat[:, 20 * H:].reshape(C, 40, H)), b.push_hops(flat[:, 20 * H:].reshape(C, 40, H))):
        _same(x, y, "all tracks reset against fx_reset_state")
    # with samples pending: the count stays (fx_reset_state drops it), the samples are zeros
    a.push_samples(flat[:, :700])
    assert a.pending_samples() == 188
    a.reset_channels(list(range(C)))
    assert a.pending_samples() == 188
    b.reset_state()
    b.push_samples(np.zeros((C, 188), np.float32))
    for x, y in zip(a.push_samples(flat[:, 700:4000]), b.push_samples(flat[:, 700:4000])):
        _same(x, y, "all tracks reset with samples pending")
    a.reset_state()
    assert np.array_equal(a.channel_frames(), np.zeros(C)) and a.pending_samples() == 0
    a.push_hops(flat[:, :3 * H].reshape(C, 3, H))
    assert np.array_equal(a.channel_frames(), np.full(C, 3))
    a.close(), b.close()


@pytest.mark.parametrize("mixed", [False, True], ids=["no-table", "table"])
def test_latest_vectors_datagrams_taps_and_frame_counts_right_after_a_reset(gpu_fx, mixed):
    N, H = 1024, 512
    hops = signals.bursts(C, 30, N, seed=73)
    an = gpu_fx.BatchAnalyser(C, N)
    new = gpu_fx.BatchAnalyser(C, N)
    if mixed:
        for x in (an, new):
            x.set_channel_gains(GAINS)
            x.set_channel_onset(SENS, WINDOWS, TYPES)
    settings = an.channel_settings()
    an.push_hops(hops[:, :17])
    before = an.get_features()
    d0, n0 = an.osc_datagrams("/Audio/A", 0)
    assert np.array_equal(an.channel_frames(), np.full(C, 17))
    an.reset_channels([1, 4])
    after, fresh = an.get_features(), new.get_features()
    d1, n1 = an.osc_datagrams("/Audio/A", 0)
    dn, nn = new.osc_datagrams("/Audio/A", 0)
    for c in range(C):
        listed = c in (1, 4)
        _same(after[c], fresh[c] if listed else before[c], "latest of track %d" % c)
        assert bytes(d1[c, :n1[c]]) == (bytes(dn[c, :nn[c]]) if listed else bytes(d0[c, :n0[c]])), c
    assert not np.array_equal(_bits(before[1]), _bits(fresh[1]))          # (the reset did change something)
    assert np.array_equal(an.channel_frames(), [17, 0, 17, 17, 0, 17])
    now = an.channel_settings()
    for k in settings:
        assert np.array_equal(settings[k], now[k]), k                      # settings kept; on a context without a table they are the defaults
    # taps: the reset track's frame index starts again, its window's carried half is a new track's zeros
    an.request_taps([1, 2])
    an.push_hops(np.ascontiguousarray(hops[:, 17:20]))
    t1, t2 = an.taps(1), an.taps(2)
    assert t1["frame_index"] == 0 and t2["frame_index"] == 17
    gain = GAINS if mixed else np.ones(C, np.float32)
    assert not t1["window"][:H].any() and np.array_equal(t1["window"][H:], hops[1, 17] * gain[1])
    assert np.array_equal(t2["window"][:H], hops[2, 16] * gain[2])
    assert np.array_equal(an.channel_frames(), [20, 3, 20, 20, 3, 20])
    an.reset_channels([1])                                                  # a capture keeps the index it was made with
    assert an.taps(1)["frame_index"] == 0
    an.reset_channels([])                                                   # nothing listed: nothing happens
    assert np.array_equal(an.channel_frames(), [20, 0, 20, 20, 3, 20])
    with pytest.raises(ValueError, match="entry 1"):
        an.reset_channels([0, C])
    lib = gpu_fx.load_library()
    import ctypes
    bad = (ctypes.c_int * 2)(2, C)
    assert lib.fx_reset_channels(an._h, bad, 2) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT and b"entry 1" in lib.fx_last_error()
    assert lib.fx_clear_pending_channels(an._h, bad, 2) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT
    assert np.array_equal(an.channel_frames(), [20, 0, 20, 20, 3, 20])
    an.close(), new.close()


def test_event_frames_restart_for_the_reset_track_and_the_order_is_by_call(gpu_fx):
    """bursts make onsets on both sides of the reset: the reset track's `frame` restarts, the others' continue, and the list is in
    (call, call_frame, channel) order -- no longer sorted by frame once a track was reset on its own"""
    N, per, T, R = 1024, 6, 96, 48
    hops = signals.bursts(C, T, N, seed=76)
    an = gpu_fx.BatchAnalyser(C, N)
    an.enable_onset_events(1 << 14)
    raws, calls = [], []
    for t in range(0, T, per):
        if t == R:
            an.reset_channels([0, 1])
        raws.append(an.push_hops(np.ascontiguousarray(hops[:, t:t + per]))[0])
        calls.append(per)
    ev, dropped = an.onset_events()
    an.close()
    raw = np.concatenate(raws, axis=1)
    first = np.zeros((C, T), np.int64)
    first[[0, 1], R:] = R
    assert dropped == 0
    assert [(int(e["frame"]), int(e["channel"]), int(e["call_frame"])) for e in ev] == _expected_events(raw, calls, first)
    for c in (0, 1):
        mine = ev[ev["channel"] == c]
        assert (raw[c, :R, 0] == 1).any() and (raw[c, R:, 0] == 1).any(), "track %d needs onsets on both sides of the reset" % c
        assert np.array_equal(mine["frame"], np.concatenate([np.flatnonzero(raw[c, :R, 0] == 1), np.flatnonzero(raw[c, R:, 0] == 1)]))
    other = ev[ev["channel"] == 2]
    assert np.array_equal(other["frame"], np.flatnonzero(raw[2, :, 0] == 1)) and (other["frame"] >= R).any()


@pytest.mark.parametrize("N,entry", [(1024, "samples"), (2048, "samples"), (256, "samples"), (1024, "interleaved")])
def test_clear_pending_channels_zeroes_the_listed_tracks_pending_samples_only(gpu_fx, N, entry):
    H = N // 2
    flat = np.ascontiguousarray(signals.bursts(C, 40, N, seed=75).reshape(C, -1)) + np.float32(0.01)
    cuts = [0, H + H // 3, 3 * H + 7, 40 * H]
    listed = [1, 3, 3]
    zeroed = flat.copy()
    p0 = (cuts[1] // H) * H                                     # what is pending after the first block: samples p0 .. cuts[1]
    zeroed[[1, 3], p0:cuts[1]] = 0.0
    outs = []
    for stream, clear in ((flat, True), (zeroed, False)):
        an = gpu_fx.BatchAnalyser(C, N)
        an.set_channel_gains(GAINS)
        got = []
        for k in range(3):
            x = np.ascontiguousarray(stream[:, cuts[k]:cuts[k + 1]])
            got.append(an.push_samples(x) if entry == "samples" else an.push_interleaved(np.ascontiguousarray(x.T)))
            if k == 0:
                pending = an.pending_samples()
                assert pending == cuts[1] - p0 and pending > 0
                frames = an.channel_frames()
                latest = an.get_features()
                if clear:
                    an.clear_pending_channels(listed)
                assert an.pending_samples() == pending and np.array_equal(an.channel_frames(), frames)
                _same(an.get_features(), latest, "latest vectors across the clear")
        an.close()
        outs.append([np.concatenate([g[i] for g in got], axis=1) for i in (0, 1)])
    _same(outs[0][0], outs[1][0], "raw: cleared tracks against tracks whose pending samples were zeros, the others untouched")
    _same(outs[0][1], outs[1][1], "smoothed")
    assert not np.array_equal(flat[1, p0:cuts[1]], zeroed[1, p0:cuts[1]])


@pytest.mark.parametrize("tuning", [{}, {"stream_hop_kernel": 0}], ids=["ring-hop", "ring-graph"])
def test_a_reset_is_ordered_after_the_batches_in_flight(gpu_fx, tuning):
    """two batches of the ring are outstanding when the reset is made: they are analysed before it (the call waits for the stream), the
    batches submitted after it see it, and nothing is lost from the ring"""
    N, H, T, R = 1024, 512, 40, 17
    hops = signals.bursts(C, T, N, seed=SEED)

    def run(reset, start=0):
        an = gpu_fx.BatchAnalyser(C, N)
        if tuning:
            an.set_tuning(**tuning)
        st = gpu_fx.HopStream(an, 1, slots=3)
        outs = []
        for t in range(start, T):
            if t == R and reset:
                assert st.in_flight() == 2
                an.reset_channels([1, 4])
                assert st.in_flight() == 2
            if st.in_flight() == 2:
                outs.append(st.collect())
            st.push(np.ascontiguousarray(hops[:, t:t + 1]))
        while st.in_flight():
            outs.append(st.collect())
        frames = an.channel_frames()
        st.close()
        an.close()
        return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1), frames

    raw, sm, frames = run(True)
    braw, bsm, _ = run(False)
    fraw, fsm, _ = run(False, start=R)
    assert np.array_equal(frames, [T, T - R, T, T, T - R, T])
    for c in range(C):
        if c in (1, 4):
            _same(raw[c, :R], braw[c, :R], "raw of track %d before the reset, the two batches in flight included" % c)
            _same(raw[c, R:], fraw[c], "raw of track %d after the reset" % c)
            _same(sm[c, R:], fsm[c], "smoothed of track %d after the reset" % c)
        else:
            _same(raw[c], braw[c], "raw of track %d" % c)
            _same(sm[c], bsm[c], "smoothed of track %d" % c)
