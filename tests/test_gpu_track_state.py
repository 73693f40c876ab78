"""Moving tracks between contexts (fx_track_state_bytes / fx_export_channels / fx_import_channels).

Everything is compared as uint32 bits, NaN slots included: the yardstick is the library itself on a track that never moved (the other
suites hold that track to the oracle), so there is no tolerance -- the values are equal or the test fails.

The main property: context A (6 tracks) is fed k frames, tracks [1, 3, 3] are exported, records 0 and 1 go into slots [2, 0] of a
context B with another channel count that has analysed another number of frames (0, 31, 100: other ring rows, a negative first_frame,
a lapped ring), and both slots are fed the rest of the tracks' input while B's other tracks get input of their own.  Then
  - B's raw and smoothed output of the moved slots is that of a copy of A that simply kept going,
  - B's other tracks are those of a B where no import happened,
  - A's later output is that of the copy: the export changed nothing.
k is 0 (a track never analysed), 4 and 13 (histories filling; with per-track settings the onset window was set three frames before,
so the move falls inside it) and 55 (ring lapped); after the import every window size, entry point, call length, order mode, analyser
flag and kernel family runs.

The bitwise comparisons have no worst figure (they are equal or the test fails).  Wall time on an MI355X: the cases of the main
property take at most 0.21 s each (ring-graph-4096-k13), the whole file a few seconds."""
import ctypes

import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu

CA = 6
EXPORTED = [1, 3, 3]            # a duplicate is allowed on export
SLOTS = [2, 0]                  # records 0 and 1 (tracks 1 and 3) go here
MOVED = [1, 3]
GAINS = np.array([1.0, 0.5, -0.7, 2.0, 1.5, 0.25], np.float32)
SENS = np.array([0.7, 0.3, 0.1, 0.2, 0.5, 0.15], np.float32)
WINDOWS = np.array([5, 3, 1, 8, 21, 5], np.int32)
TYPES = np.array([1, 0, 2, 1, 0, 1], np.int32)
MASKS = {"both": 3, "spectral": 1, "harmonic": 2}
# signals.bursts seed of A's input, picked on the CPU with the oracle alone (oracle.Channel per moved track, fed the track's whole
# stream with the case's settings): with it every case below that runs the spectral analyser has an onset after the move on at least
# one of the two moved tracks.  B's own input uses the next seed.
SEED = 90


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(_bits(a), _bits(b)), "%s: %d of %d values differ" % (what, int((_bits(a) != _bits(b)).sum()), a.size)


def _frames_of(hops):
    """assembled windows [C][T][N] of a hop stream (the overlapper starts with a zero tail)"""
    Cn, T, H = hops.shape
    prev = np.concatenate([np.zeros((Cn, 1, H), hops.dtype), hops[:, :-1]], axis=1)
    return np.ascontiguousarray(np.concatenate([prev, hops], axis=2))


class Ctx:
    """one context and, for the ring entry, the ring that stays open across the import (its captured step is replayed after it)"""

    def __init__(self, fx, C, N, entry, kw, tuning, settings=None):
        self.C, self.N, self.H, self.entry = C, N, N // 2, entry
        self.an = fx.BatchAnalyser(C, N, **kw)
        if tuning:
            self.an.set_tuning(**tuning)
        if settings is not None:
            gains, sens, windows, types = settings
            self.an.set_channel_gains(gains)
            self.an.set_channel_onset(sens, windows, types)
        self.ring = fx.HopStream(self.an, 1, slots=3) if entry == "ring" else None

    def feed(self, x, per):
        """x: [C][n] samples (whole hops unless the entry takes blocks) or, for the frames entry, [C][T][N]; calls of `per` hops,
        frames or samples.  Returns (raw, smoothed) of all of it."""
        e, H, outs = self.entry, self.H, []
        if e == "frames":
            for t in range(0, x.shape[1], per):
                outs.append(self.an.process_frames(np.ascontiguousarray(x[:, t:t + per])))
        elif e in ("samples", "interleaved"):
            for s in range(0, x.shape[1], per):
                blk = np.ascontiguousarray(x[:, s:s + per])
                outs.append(self.an.push_samples(blk) if e == "samples" else self.an.push_interleaved(np.ascontiguousarray(blk.T)))
        elif e == "hops":
            for s in range(0, x.shape[1], per * H):
                outs.append(self.an.push_hops(np.ascontiguousarray(x[:, s:s + per * H].reshape(self.C, -1, H))))
        elif e == "ring":
            for s in range(0, x.shape[1], H):
                self.ring.push(np.ascontiguousarray(x[:, s:s + H]).reshape(self.C, 1, H))
                outs.append(self.ring.collect())
        else:
            raise ValueError(e)
        if not outs:
            z = np.zeros((self.C, 0, 12), np.float32)
            return z, z
        return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1)

    def close(self):
        if self.ring:
            self.ring.close()
        self.an.close()


def source_input(N, total, fmt="f32", seed=SEED):
    """A's hops [6][total][H]: float32, or the same as 16-bit PCM"""
    hops = signals.bursts(CA, total, N, seed=seed)
    if fmt == "s16":
        hops = np.clip(np.rint(hops * 16384.0), -32768, 32767).astype(np.int16)
    return hops


def pre_move_plan(N, entry, per, k):
    """how A reaches the move: (samples fed, frames analysed, pending) -- k whole hops, or for the block entries the fewest blocks of
    `per` samples that complete k frames"""
    H = N // 2
    if entry in ("samples", "interleaved"):
        blocks = -(-k * H // per)
        return blocks * per, blocks * per // H, blocks * per % H
    return k * H, k, 0


def _case(cid, N, entry, per, k, dst, kw=None, tuning=None, mixed=False, post=None, fmt="f32"):
    return (cid, N, entry, per, k, dst, kw or {}, tuning or {}, mixed, post if post is not None else 80 - k, fmt)


LL = {"low_latency": True}
GRAPH = {"stream_hop_kernel": 0}
CASES = [
    _case("hops-1-256-k0", 256, "hops", 1, 0, (4, 0)),
    _case("hops-1-512-k4", 512, "hops", 1, 4, (9, 31), mixed=True),
    _case("hops-1-1024-k13", 1024, "hops", 1, 13, (4, 100), mixed=True),
    _case("hops-1-2048-k55", 2048, "hops", 1, 55, (9, 0), mixed=True),
    _case("hops-1-4096-k4", 4096, "hops", 1, 4, (4, 31)),
    _case("hops-2-256-k13", 256, "hops", 2, 13, (9, 100)),
    _case("hops-2-1024-k55", 1024, "hops", 2, 55, (4, 31), mixed=True),
    _case("hops-2-4096-k0", 4096, "hops", 2, 0, (9, 100)),
    _case("hops-7-512-k55", 512, "hops", 7, 55, (4, 100), mixed=True),
    _case("hops-7-2048-k13", 2048, "hops", 7, 13, (9, 31)),
    _case("hops-long-1024-k4", 1024, "hops", 130, 4, (9, 100), mixed=True, post=130),       # 130: cut into work units, laps the ring
    _case("frame-tail-1024-k13", 1024, "hops", 1, 13, (4, 31), tuning={"one_hop_kernel": 0}, mixed=True),
    _case("harmonic-first-1-1024-k4", 1024, "hops", 1, 4, (9, 100), kw={"order": 1}),
    _case("harmonic-first-7-1024-k55", 1024, "hops", 7, 55, (4, 0), kw={"order": 1}, mixed=True),
    _case("isolated-2-2048-k13", 2048, "hops", 2, 13, (9, 31), kw={"order": 2}, mixed=True),
    _case("spectral-only-1-256-k13", 256, "hops", 1, 13, (4, 100), kw={"analysers": "spectral"}, mixed=True),
    _case("spectral-only-7-1024-k4", 1024, "hops", 7, 4, (9, 31), kw={"analysers": "spectral"}),
    _case("harmonic-only-1-1024-k55", 1024, "hops", 1, 55, (4, 31), kw={"analysers": "harmonic"}),
    _case("harmonic-only-7-4096-k13", 4096, "hops", 7, 13, (9, 100), kw={"analysers": "harmonic"}, mixed=True),
    _case("low-latency-1-2048-k13", 2048, "hops", 1, 13, (4, 100), kw=LL, mixed=True),
    _case("low-latency-2-4096-k55", 4096, "hops", 2, 55, (9, 31), kw=LL),
    _case("low-latency-7-4096-k4", 4096, "hops", 7, 4, (4, 0), kw=LL, mixed=True),
    _case("frames-1-1024-k13", 1024, "frames", 1, 13, (9, 31), mixed=True),
    _case("frames-7-2048-k4", 2048, "frames", 7, 4, (4, 100)),
    _case("samples-441-1024-k13", 1024, "samples", 441, 13, (4, 31), mixed=True),
    _case("samples-480-1024-k55", 1024, "samples", 480, 55, (9, 100)),
    _case("samples-441-2048-k4", 2048, "samples", 441, 4, (9, 31)),
    _case("samples-480-512-k13-s16", 512, "samples", 480, 13, (4, 100), mixed=True, fmt="s16"),
    _case("samples-480-low-latency-2048-k4", 2048, "samples", 480, 4, (9, 0), kw=LL, mixed=True),
    _case("interleaved-480-1024-k4", 1024, "interleaved", 480, 4, (9, 100), mixed=True),
    _case("interleaved-441-512-k55", 512, "interleaved", 441, 55, (4, 31)),
    _case("ring-hop-1024-k13", 1024, "ring", 1, 13, (9, 31), mixed=True),
    _case("ring-hop-2048-k4", 2048, "ring", 1, 4, (4, 100)),
    _case("ring-graph-1024-k55", 1024, "ring", 1, 55, (4, 31), tuning=GRAPH),
    _case("ring-graph-4096-k13", 4096, "ring", 1, 13, (9, 100), tuning=GRAPH, mixed=True),
    _case("ring-graph-low-latency-2048-k4", 2048, "ring", 1, 4, (9, 31), kw=LL, tuning=GRAPH),
]


def feed_source_to_the_move(a, hops, N, entry, per, k, mixed):
    """A's (or its copy's) way to the move.  With per-track settings and k >= 4 the onset windows are set again three frames before
    it, so the tracks leave inside an onset window's fill."""
    H = N // 2
    fed, frames, pending = pre_move_plan(N, entry, per, k)
    if entry == "frames":
        fr = _frames_of(hops)
        a.feed(fr[:, :max(k - 3, 0)], 8)
        if mixed and k >= 4:
            a.an.set_channel_onset(None, WINDOWS, None)
        a.feed(fr[:, max(k - 3, 0):k], 8)
        return fed
    flat = np.ascontiguousarray(hops.reshape(CA, -1))
    if entry in ("samples", "interleaved"):
        first = (max(frames - 3, 0) * H // per) * per          # whole blocks: the last of them ends at most three frames before the move
        a.feed(flat[:, :first], per)
        if mixed and k >= 4:
            a.an.set_channel_onset(None, WINDOWS, None)
        a.feed(flat[:, first:fed], per)
    else:
        cut = max(k - 3, 0) * H
        if cut:
            a.an.push_hops(np.ascontiguousarray(flat[:, :cut].reshape(CA, -1, H)))
        if mixed and k >= 4:
            a.an.set_channel_onset(None, WINDOWS, None)
        if fed > cut:
            a.an.push_hops(np.ascontiguousarray(flat[:, cut:fed].reshape(CA, -1, H)))
    assert a.an.pending_samples() == pending and np.array_equal(a.an.channel_frames(), np.full(CA, frames))
    return fed


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_a_moved_track_goes_on_as_if_it_had_stayed(gpu_fx, case):
    cid, N, entry, per, k, (CB, dst_frames), kw, tuning, mixed, post, fmt = case
    fx, H = gpu_fx, N // 2
    total = k + post
    hops = source_input(N, total + 2, fmt)
    flat = np.ascontiguousarray(hops.reshape(CA, -1))
    settings = (GAINS, SENS, WINDOWS, TYPES) if mixed else None
    fed, frames_a, pending = pre_move_plan(N, entry, per, k)
    end = total * H

    # ---- A exports and goes on; its copy never exports ----
    outs = {}
    for name in ("A", "copy"):
        a = Ctx(fx, CA, N, entry, kw, tuning, settings)
        feed_source_to_the_move(a, hops, N, entry, per, k, mixed)
        if name == "A":
            before = a.an.export_tracks(list(range(CA)))
            state = a.an.export_tracks(EXPORTED)
            assert state.shape == (3, a.an.track_state_bytes()) and state.dtype == np.uint8
            assert np.array_equal(state[1], state[2]) and np.array_equal(state[0], before[1]) and np.array_equal(state[1], before[3])
            assert np.array_equal(a.an.export_tracks(list(range(CA))), before)
        if entry == "frames":
            outs[name] = a.feed(_frames_of(hops)[:, k:total], per)
        else:
            outs[name] = a.feed(flat[:, fed:end], per)
        a.close()
    for i, part in enumerate(("raw", "smoothed")):
        _same(outs["A"][i], outs["copy"][i], "%s: %s of A after its export against a copy that never exported" % (cid, part))
    T = outs["copy"][0].shape[1]
    assert T == (total - k if entry == "frames" else (end - fed + pending) // H) and T > 0

    # ---- B, with tracks of its own, takes records 0 and 1 into slots 2 and 0; a second B takes nothing ----
    own = source_input(N, dst_frames + total + 2, fmt, seed=SEED + 1)
    own = np.concatenate([own, own[:3]], axis=0)[:CB] if CB > CA else own[:CB]
    own_flat = np.ascontiguousarray(own.reshape(CB, -1))
    # half the destinations have a per-track table of their own
    b_settings = tuple(np.resize(v[::-1], CB) for v in (GAINS, SENS, WINDOWS, TYPES)) if CB == 9 else None
    got = {}
    for name in ("B", "untouched"):
        b = Ctx(fx, CB, N, entry, kw, tuning, b_settings)
        # B's own past: dst_frames frames, then (block entries) blocks of the same lengths as A's, so that the pending counts agree
        if entry == "frames":
            own_frames = _frames_of(own)
            b.feed(own_frames[:, :dst_frames], 8)
            at = dst_frames
            x = np.ascontiguousarray(own_frames[:, at:at + T])
            if name == "B":
                src = _frames_of(hops)
                for slot, track in zip(SLOTS, MOVED):
                    x[slot] = src[track, k:total]
        else:
            if entry in ("samples", "interleaved"):
                b.feed(own_flat[:, :dst_frames * H], max(dst_frames * H, 1))
                b.feed(own_flat[:, dst_frames * H:dst_frames * H + fed], per)
            else:
                b.feed(own_flat[:, :dst_frames * H], 1 if entry == "ring" else 8)
            at = dst_frames * H + fed
            x = np.ascontiguousarray(own_flat[:, at:at + end - fed])
            if name == "B":
                for slot, track in zip(SLOTS, MOVED):
                    x[slot] = flat[track, fed:end]
        assert b.an.pending_samples() == pending
        if name == "B":
            others = [c for c in range(CB) if c not in SLOTS]
            kept = b.an.export_tracks(others)
            b.an.import_tracks(SLOTS, state[:2])
            assert np.array_equal(b.an.export_tracks(others), kept), "%s: the import changed a track it did not list" % cid
            assert np.array_equal(b.an.export_tracks(SLOTS), state[:2]), "%s: the slots do not export what was imported" % cid
            frames_b = b.an.channel_frames()
            own_frames_b = dst_frames + (frames_a if entry in ("samples", "interleaved") else 0)
            assert frames_b[2] == frames_a and frames_b[0] == frames_a and all(frames_b[c] == own_frames_b for c in others), frames_b
        got[name] = b.feed(x, per)
        b.close()
    for i, part in enumerate(("raw", "smoothed")):
        for slot, track in zip(SLOTS, MOVED):
            _same(got["B"][i][slot], outs["copy"][i][track], "%s: %s of track %d in slot %d of B against the track that stayed" % (cid, part, track, slot))
        for c in range(CB):
            if c not in SLOTS:
                _same(got["B"][i][c], got["untouched"][i][c], "%s: %s of B's own track %d" % (cid, part, c))
    assert not np.array_equal(_bits(got["B"][0][2]), _bits(got["untouched"][0][2]))          # (the import did change something)
    if MASKS[kw.get("analysers", "both")] & 1:
        onsets = int((outs["copy"][0][MOVED, :, 0] == 1.0).sum())
        assert onsets > 0, "%s: the case must contain an onset after the move on a moved track" % cid


def _moved_pair(fx, N=1024, k=17, CB=4, dst_frames=31, mixed=True, seed=SEED):
    """A fed k hops and B fed dst_frames hops of its own, both open; (a, b, hops of A, hops of B)"""
    hops = signals.bursts(CA, k + 40, N, seed=seed)
    own = signals.bursts(CB, dst_frames + 40, N, seed=seed + 1)
    a = fx.BatchAnalyser(CA, N)
    b = fx.BatchAnalyser(CB, N)
    if mixed:
        a.set_channel_gains(GAINS)
        a.set_channel_onset(SENS, WINDOWS, TYPES)
    if k:
        a.push_hops(np.ascontiguousarray(hops[:, :k]))
    if dst_frames:
        b.push_hops(np.ascontiguousarray(own[:, :dst_frames]))
    return a, b, hops, own


def test_records_are_canonical_bytes(gpu_fx):
    fx = gpu_fx
    a, b, hops, own = _moved_pair(fx)
    size = a.track_state_bytes()
    assert size == 2432 + 6 * 1024 and size % 16 == 0 and b.track_state_bytes() == size
    host = a.export_tracks(EXPORTED)
    dev = a.export_tracks(EXPORTED, device=True)
    assert dev.is_cuda and tuple(dev.shape) == (3, size)
    assert np.array_equal(dev.cpu().numpy(), host), "host and device buffers"
    # through B and back: B has another channel count, frame index and ring position, the slot is another
    b.import_tracks(SLOTS, dev[:2])
    assert np.array_equal(b.export_tracks(SLOTS), host[:2]), "after a round trip through a device buffer"
    assert np.array_equal(b.export_tracks(SLOTS, device=True).cpu().numpy(), host[:2])
    c = fx.BatchAnalyser(3, 1024)
    c.push_hops(np.ascontiguousarray(own[:3, :7]))
    c.import_tracks([1], np.frombuffer(b.export_tracks([2]).tobytes(), np.uint8))          # a read-only flat copy imports the same
    assert np.array_equal(c.export_tracks([1])[0], host[0]), "after a second move, from plain bytes"
    assert np.array_equal(a.export_tracks(EXPORTED), host), "the source after its exports"
    # the header says what it should (little-endian words as include/fx.h lists them)
    words = host[0][:80].view(np.uint32)
    assert words[2] == 1024 and words[3] == 0 and words[4] == 1 and words[5] == 0 and words[7] == WINDOWS[1]
    assert host[0][32:48].view(np.int64).tolist() == [17, 17] and words[16] == size
    assert host[0][48:60].view(np.float32).tolist() == [GAINS[1], SENS[1], np.float32(1.0) + SENS[1]] and words[15] == TYPES[1]
    for an in (a, b, c):
        an.close()


@pytest.mark.parametrize("pending", [0, 441])
def test_a_fresh_track_and_a_reset_track_export_the_same_bytes(gpu_fx, pending):
    fx, N = gpu_fx, 1024
    hops = signals.bursts(CA, 60, N, seed=SEED)
    fresh = fx.BatchAnalyser(CA, N)
    used = fx.BatchAnalyser(4, N)
    used.push_hops(np.ascontiguousarray(hops[:4, :55]))                   # ring lapped: the reset clears none of its rows
    if pending:
        fresh.push_samples(np.zeros((CA, pending), np.float32))
        used.push_samples(np.ascontiguousarray(hops[:4, 55].reshape(4, -1)[:, :pending]))
    used.reset_channels([2])
    want = fresh.export_tracks([5])
    assert np.array_equal(used.export_tracks([2]), want)
    assert not np.array_equal(used.export_tracks([1]), want)
    assert not want[0][80:].any()                                          # all of a new track's state is zeros
    fresh.close(), used.close()


@pytest.mark.parametrize("mixed", [False, True], ids=["no-table", "table"])
def test_what_travels_and_what_does_not(gpu_fx, mixed):
    fx, N, H, k, dst_frames, CB = gpu_fx, 1024, 512, 17, 31, 4
    a, b, hops, own = _moved_pair(fx, N, k, CB, dst_frames, mixed)
    b.set_osc_addresses(["/B/slot%d" % c for c in range(CB)])
    cmap = [3, 2, 1, 0]
    b.set_channel_map(cmap)
    b.enable_onset_events(1 << 12)
    b.import_tracks(SLOTS, a.export_tracks(MOVED))
    # ---- right after the import ----
    fa, fb = a.get_features(), b.get_features()
    sa, sb = a.channel_settings(), b.channel_settings()
    for slot, track in zip(SLOTS, MOVED):
        _same(fb[slot], fa[track], "latest vector of slot %d" % slot)
        da, na = a.osc_datagrams("/Audio/A", slot)                         # the same address for the track there and the slot here
        db, nb = b.osc_datagrams("/Audio/A", track)
        assert bytes(da[track, :na[track]]) == bytes(db[slot, :nb[slot]])
        for key in sa:
            assert sa[key][track].tobytes() == sb[key][slot].tobytes(), (key, slot)
    assert np.array_equal(b.channel_frames(), [k, dst_frames, k, dst_frames])
    dgrams, lens = b.osc_datagrams(addressed=True)
    for c in range(CB):
        assert bytes(dgrams[c, :lens[c]]).startswith(b"/B/slot%d\0" % c)       # the address is the slot's
    # ---- the next call: taps and events count the moved tracks' own frames; the channel map is B's ----
    a.request_taps(MOVED)
    b.request_taps([0, 1, 2])
    n = 20
    x = np.ascontiguousarray(own[:, dst_frames:dst_frames + n]).reshape(CB, -1)
    for slot, track in zip(SLOTS, MOVED):
        x[slot] = hops[track, k:k + n].reshape(-1)
    block = np.empty((n * H, CB), np.float32)
    for c in range(CB):
        block[:, cmap[c]] = x[c]                                            # track c collects source channel cmap[c]
    raw_b, sm_b = b.push_interleaved(block)
    raw_a, sm_a = a.push_hops(np.ascontiguousarray(hops[:, k:k + n]))
    for slot, track in zip(SLOTS, MOVED):
        _same(raw_b[slot], raw_a[track], "raw of slot %d through B's channel map" % slot)
        _same(sm_b[slot], sm_a[track], "smoothed of slot %d" % slot)
        ta, tb = a.taps(track), b.taps(slot)
        assert ta["frame_index"] == k and tb["frame_index"] == k
        assert np.array_equal(_bits(ta["window"]), _bits(tb["window"]))
    assert b.taps(1)["frame_index"] == dst_frames
    ev, dropped = b.onset_events()
    assert dropped == 0
    for slot in range(CB):
        mine = ev[ev["channel"] == slot]
        first = k if slot in SLOTS else dst_frames
        assert np.array_equal(mine["frame"], first + np.flatnonzero(raw_b[slot, :, 0] == 1.0)), slot
    # (picked with the oracle: with the per-track settings both moved tracks have onsets in these 20 frames, with the defaults neither)
    assert (raw_b[SLOTS, :, 0] == 1.0).any() == mixed, "the moved tracks need an onset after the move"
    a.close(), b.close()


@pytest.mark.parametrize("tuning", [{}, {"stream_hop_kernel": 0}], ids=["ring-hop", "ring-graph"])
def test_an_import_is_ordered_after_the_batches_in_flight(gpu_fx, tuning):
    """two batches of B's ring are outstanding when the import is made: they are analysed before it (the call waits for the stream),
    the batches submitted after it see it, and nothing is lost from the ring"""
    fx, N, H, T, R, k, CB = gpu_fx, 1024, 512, 40, 17, 13, 4
    hops = signals.bursts(CA, k + T, N, seed=SEED)
    own = signals.bursts(CB, T, N, seed=SEED + 1)
    a = fx.BatchAnalyser(CA, N)
    if tuning:
        a.set_tuning(**tuning)
    a.push_hops(np.ascontiguousarray(hops[:, :k]))
    state = a.export_tracks(MOVED)
    ring, outs = fx.HopStream(a, 1, slots=3), []
    for t in range(k, k + T - R):                                           # the tracks that stayed, through the same one-hop step
        ring.push(np.ascontiguousarray(hops[:, t:t + 1]))
        outs.append(ring.collect())
    stayed = [np.concatenate([o[i] for o in outs], axis=1) for i in (0, 1)]
    ring.close()
    a.close()

    def run(move):
        an = fx.BatchAnalyser(CB, N)
        if tuning:
            an.set_tuning(**tuning)
        st = fx.HopStream(an, 1, slots=3)
        outs = []
        for t in range(T):
            if t == R and move:
                assert st.in_flight() == 2
                an.import_tracks(SLOTS, state)
                assert st.in_flight() == 2
            if st.in_flight() == 2:
                outs.append(st.collect())
            x = np.ascontiguousarray(own[:, t:t + 1])
            if t >= R and move:
                for slot, track in zip(SLOTS, MOVED):
                    x[slot] = hops[track, k + t - R]
            st.push(x)
        while st.in_flight():
            outs.append(st.collect())
        frames = an.channel_frames()
        st.close()
        an.close()
        return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=1), frames

    raw, sm, frames = run(True)
    braw, bsm, _ = run(False)
    assert np.array_equal(frames, [k + T - R, T, k + T - R, T])
    for c in range(CB):
        if c in SLOTS:
            track = MOVED[SLOTS.index(c)]
            _same(raw[c, :R], braw[c, :R], "raw of slot %d before the import, the two batches in flight included" % c)
            _same(raw[c, R:], stayed[0][track], "raw of slot %d after the import" % c)
            _same(sm[c, R:], stayed[1][track], "smoothed of slot %d after the import" % c)
        else:
            _same(raw[c], braw[c], "raw of track %d" % c)
            _same(sm[c], bsm[c], "smoothed of track %d" % c)


def test_refusals_leave_every_bit_of_the_destination(gpu_fx):
    fx = gpu_fx
    lib = fx.load_library()
    inv = fx.capi.FX_ERR_INVALID_ARGUMENT
    N, CB = 1024, 4
    hops = signals.bursts(CA, 30, N, seed=SEED)
    b = fx.BatchAnalyser(CB, N)
    b.set_channel_gains(GAINS[:CB])
    b.push_hops(np.ascontiguousarray(hops[:CB, :9]))
    good_src = fx.BatchAnalyser(CA, N)
    good_src.push_hops(np.ascontiguousarray(hops[:, :5]))
    good = good_src.export_tracks(MOVED)
    everything = b.export_tracks(list(range(CB)))
    size = b.track_state_bytes()

    def refused(channels, state, match, device=False):
        if device:
            import torch
            state = torch.from_numpy(np.ascontiguousarray(state)).to("cuda:%d" % b.device)
        with pytest.raises(fx.capi.FxError, match=match) as e:
            b.import_tracks(channels, state)
        assert e.value.code == inv
        assert np.array_equal(b.export_tracks(list(range(CB))), everything), "a refused import changed the destination (%s)" % match

    def records_of(an, prepare=None):
        if prepare:
            prepare(an)
        s = an.export_tracks(MOVED)
        an.close()
        return s

    for device in (False, True):
        refused(SLOTS, records_of(fx.BatchAnalyser(CA, 2048)), "record 0: (window size|record size)", device)
        refused(SLOTS, records_of(fx.BatchAnalyser(CA, N, order=1)), "record 0: create flags", device)
        refused(SLOTS, records_of(fx.BatchAnalyser(CA, N, analysers="spectral")), "record 0: create flags", device)
        refused(SLOTS, records_of(fx.BatchAnalyser(CA, N), lambda an: an.push_samples(np.zeros((CA, 100), np.float32))), "record 0: pending count", device)
        bad = good.copy()
        bad[1, 2] ^= 0x40
        refused(SLOTS, bad, "record 1: not a track record", device)
        bad = good.copy()
        bad[0, 4] = 9
        refused(SLOTS, bad, "record 0: layout version", device)
        refused([1, 1], good, "entry 1: channel 1 is listed twice", device)
    # the kernel family: 2048 points, pairs of wavefronts against single ones
    b2 = fx.BatchAnalyser(CB, 2048)
    pairs = records_of(fx.BatchAnalyser(CA, 2048, low_latency=True))
    with pytest.raises(fx.capi.FxError, match="record 0: kernel family"):
        b2.import_tracks(SLOTS, pairs)
    fresh = fx.BatchAnalyser(CB, 2048)
    assert np.array_equal(b2.export_tracks(list(range(CB))), fresh.export_tracks(list(range(CB))))
    b2.close(), fresh.close()
    # the carry format while samples are pending: 100 samples of s16 against 100 of f32
    b3 = fx.BatchAnalyser(CB, N)
    b3.push_samples(np.zeros((CB, 100), np.float32))
    s16 = records_of(fx.BatchAnalyser(CA, N), lambda an: an.push_samples(np.zeros((CA, 100), np.int16)))
    kept = b3.export_tracks(list(range(CB)))
    with pytest.raises(fx.capi.FxError, match="record 0: carry format"):
        b3.import_tracks(SLOTS, s16)
    assert np.array_equal(b3.export_tracks(list(range(CB))), kept)
    b3.close()
    # the list and the buffer, through the C ABI (the Python wrapper checks the list itself, with fx_reset_channels' messages)
    with pytest.raises(ValueError, match=r"entry 1: track 4 out of range \[0,4\)"):
        b.import_tracks([0, CB], good)
    with pytest.raises(ValueError, match="entry 0: track -1"):
        b.export_tracks([-1])
    ptr = good.ctypes.data_as(ctypes.c_void_p)
    out_of_range = (ctypes.c_int * 2)(2, CB)
    slots = (ctypes.c_int * 2)(*SLOTS)
    twice = (ctypes.c_int * 2)(3, 3)
    assert lib.fx_import_channels(b._h, out_of_range, 2, ptr, good.size, fx.capi.MEM_HOST) == inv and b"entry 1" in lib.fx_last_error()
    assert lib.fx_export_channels(b._h, out_of_range, 2, ptr, good.size, fx.capi.MEM_HOST) == inv and b"entry 1" in lib.fx_last_error()
    assert lib.fx_import_channels(b._h, twice, 2, ptr, good.size, fx.capi.MEM_HOST) == inv and b"entry 1" in lib.fx_last_error()
    assert lib.fx_import_channels(b._h, slots, 2, ptr, 2 * size - 1, fx.capi.MEM_HOST) == inv and b"record buffer holds" in lib.fx_last_error()
    assert lib.fx_export_channels(b._h, slots, 2, ptr, 2 * size - 1, fx.capi.MEM_HOST) == inv
    assert lib.fx_import_channels(b._h, slots, 2, None, 2 * size, fx.capi.MEM_HOST) == inv and b"null record buffer" in lib.fx_last_error()
    import torch
    dev = torch.zeros(2 * size + 16, dtype=torch.uint8, device="cuda:%d" % b.device)
    dev[8:8 + 2 * size] = torch.from_numpy(good.reshape(-1)).to(dev.device)
    torch.cuda.synchronize()
    misaligned = ctypes.c_void_p(dev.data_ptr() + 8)
    assert lib.fx_import_channels(b._h, slots, 2, misaligned, 2 * size, fx.capi.MEM_DEVICE) == inv and b"16-byte aligned" in lib.fx_last_error()
    assert lib.fx_export_channels(b._h, slots, 2, misaligned, 2 * size, fx.capi.MEM_DEVICE) == inv
    assert lib.fx_import_channels(b._h, slots, 0, None, 0, fx.capi.MEM_HOST) == fx.capi.FX_OK          # nothing listed: nothing happens
    assert np.array_equal(b.export_tracks(list(range(CB))), everything)
    assert np.array_equal(good_src.export_tracks(MOVED), good)
    # ... and the same records are welcome once nothing is wrong with them
    b.import_tracks(SLOTS, good)
    assert np.array_equal(b.export_tracks(SLOTS), good)
    b.close(), good_src.close()


@pytest.mark.parametrize("where", ["side-stream", "library-stream"])
def test_an_import_reads_a_device_buffer_after_its_producer_on_another_stream(gpu_fx, where):
    """The staging tensor holds an EARLIER batch's records (valid ones: other tracks, other frame counts and gains) when, on a stream
    that is not the default one, a long stretch of work and then the copy of the new records are queued, and import_tracks is called
    at once.  Headers and rows must both be the new batch's: the header read is ordered on the context's stream like the scatter."""
    import torch
    fx = gpu_fx
    a, b, hops, own = _moved_pair(fx)
    a.push_hops(np.ascontiguousarray(hops[:, 17:20]))
    old = a.export_tracks([0, 4], device=True)                             # 20 frames, gains 1.0 and 1.5
    a.push_hops(np.ascontiguousarray(hops[:, 20:29]))
    new = a.export_tracks(MOVED, device=True)                              # 29 frames, gains 0.5 and 2.0
    want = new.cpu().numpy()
    dev = torch.device("cuda", b.device)
    staging = old.clone()
    ballast = torch.ones(1 << 27, dtype=torch.float32, device=dev)         # 512 MB: each pass over it is a fraction of a millisecond
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev) if where == "side-stream" else b.torch_stream()
    with torch.cuda.stream(stream):
        for _ in range(40):
            ballast.mul_(1.0001)
        staging.copy_(new, non_blocking=True)
        b.import_tracks(SLOTS, staging)
    torch.cuda.synchronize()
    assert np.array_equal(staging.cpu().numpy(), want)
    assert np.array_equal(b.export_tracks(SLOTS), want), "the import took headers or rows of the staging buffer's earlier contents"
    assert np.array_equal(b.channel_frames(), [29, 31, 29, 31])
    assert np.array_equal(b.channel_settings()["gain"][SLOTS], GAINS[MOVED])
    a.close(), b.close()


def test_host_buffers_move_through_the_scratch_in_chunks(gpu_fx):
    """fx_set_tuning_internal bit 6: two records a chunk instead of 32 MB -- five records are three chunks, same bytes, same state"""
    fx = gpu_fx
    a, b, hops, own = _moved_pair(fx, CB=9)
    tracks, slots = [5, 1, 3, 3, 0], [8, 2, 0, 4, 6]
    whole = a.export_tracks(tracks)
    a.set_test_hooks(64), b.set_test_hooks(64)
    chunked = a.export_tracks(tracks)
    assert np.array_equal(chunked, whole) and np.array_equal(a.export_tracks(tracks, device=True).cpu().numpy(), whole)
    kept = b.export_tracks([1, 3, 5, 7])
    b.import_tracks(slots, whole)
    b.set_test_hooks(0)
    assert np.array_equal(b.export_tracks(slots), whole) and np.array_equal(b.export_tracks([1, 3, 5, 7]), kept)
    a.close(), b.close()
