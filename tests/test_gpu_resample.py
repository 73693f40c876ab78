"""Clips at their own sample rate on the GPU (include/fx.h, "CLIPS AT THEIR OWN RATE"): context A runs push_sources with rated clips,
its twin B is given push_samples(the fp32 planar block of tests/resample_model.py, which renders with the table read from the
library) and clear_pending_channels at the model's points.  After every tick raw, smoothed, frame counts and pending_samples() are
equal bit for bit, the launch record is "sources", "resample" (T = n each) followed by the twin's record, and transport_state() is
the model's table; get_features() and the display are compared where a case ends.

Tracks per context.  The kinds a context must mix (an INPUT track, an unrated fp32 loop, rated loops of five lengths, a rated one-shot
that ends inside a tick, a rated paused, a stopped and a no-file track) are eleven, so the contexts that mix them have 14 tracks; the
same blocks also run through two contexts of 6 tracks that hold one half of the kinds each."""
import functools
import os
import subprocess

import numpy as np
import pytest

import clip_model as cm
import interleave_model as im
import resample_model as rm
import signals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 48000.0
RATIOS = [147 / 160, 160 / 147, 2.0, 1 / 2, 8.0, 1 / 8, 1.5]
BLOCKS = [1, 63, 257, 441, 480, 1000, 4097]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _torch(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(r):
    return None if r is None else (r.cpu().numpy() if hasattr(r, "cpu") else r)


@functools.lru_cache(maxsize=None)
def _tape():
    """one long stretch of audio: clips and live rows are cut from it"""
    return signals.tone_vibrato_noise(1, 400, 1024, seed=23).reshape(-1).astype(np.float32)


def _cut(fmt, k, L):
    """clip number k: L samples of the tape from a place of its own, as the bytes of `fmt`"""
    at = (k * 7919) % (_tape().size - L)
    return cm.raw(im.encode(_tape()[None, at:at + L], fmt))[0].copy()


def _live(C, total):
    room = _tape().size - total
    return np.stack([_tape()[(c * 4099) % room:(c * 4099) % room + total] for c in range(C)])


class Rig:
    """a sources context, its twin and the model between them; clips are named (format, number in that format's bank)"""

    def __init__(self, gpu_fx, C, N, device, sample_rate=RATE):
        self.fx, self.C, self.N, self.device = gpu_fx, C, N, device
        self.an, self.twin = gpu_fx.BatchAnalyser(C, N, sample_rate), gpu_fx.BatchAnalyser(C, N, sample_rate)
        for a in (self.an, self.twin):
            a.set_gain(0.75)
        self.m = rm.Model(C, gpu_fx.capi.resampler_table()[0], sample_rate)
        self.first, self.clips, self.rates = {}, {}, {}

    def close(self):
        assert same(self.an.get_features(), self.twin.get_features())
        self.an.close(); self.twin.close()

    def _arr(self, x):
        return _torch(x) if self.device else np.ascontiguousarray(x)

    def bank(self, fmt, clips, rates):
        """the clips back to back in ONE bank of their format (so 16- and 24-bit clips start at odd addresses), the rates given with it"""
        self.first[fmt] = self.an.create_clips(self._arr(cm.typed(np.concatenate(clips), fmt)), lengths=[c.size // cm.BYTES[fmt] for c in clips],
                                               sample_format=fmt, sample_rates=rates)
        self.clips[fmt], self.rates[fmt] = clips, [float(r) for r in rates]

    def clip_id(self, key):
        return -1 if key is None else self.first[key[0]] + key[1]

    def set_rates(self, keys, rates):
        self.an.set_clip_rates([self.clip_id(k) for k in keys], rates)
        for k, r in zip(keys, rates):
            self.rates[k[0]][k[1]] = float(r)

    def _cleared(self, tracks):
        if tracks:
            self.twin.clear_pending_channels(tracks)

    def load(self, channels, keys, loop=None):
        self.an.load_clips(channels, [self.clip_id(k) for k in keys], loop)
        self._cleared(self.m.load(channels, [None if k is None else self.clips[k[0]][k[1]] for k in keys], loop,
                                  ["f32" if k is None else k[0] for k in keys], [0.0 if k is None else self.rates[k[0]][k[1]] for k in keys]))

    def sources(self, channels, types):
        self.an.set_sources(channels, types)
        self._cleared(self.m.set_sources(channels, types))

    def transport(self, channels, command):
        self.an.transport(channels, command)
        self._cleared(self.m.transport(channels, command))

    def check_table(self):
        got, want = self.an.transport_state(), self.m.table()
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, got[k], want[k])

    def tick(self, live, n, table=True):
        """one tick: `live` float32 [C][n] or None"""
        resampled = any(p.source == cm.FILE and p.rated for p in self.m.players)
        planar = self.m.tick(live, n)
        if live is None:
            got = self.an.push_sources(None, n, device=self.device)         # "f32" by default
        else:
            got = self.an.push_sources(self._arr(live))
        want = self.twin.push_samples(self._arr(planar))
        g, w = [_host(x) for x in got], [_host(x) for x in want]
        assert g[0].shape == w[0].shape and same(g[0], w[0]) and same(g[1], w[1])
        assert self.an.pending_samples() == self.twin.pending_samples()
        rec, twin_rec = self.an.last_launches(), self.twin.last_launches()
        head = ["sources", "resample"] if resampled else ["sources"]
        assert [r["kind"] for r in rec[:len(head)]] == head and all(r["T"] == n for r in rec[:len(head)]), rec
        assert rec[len(head):] == twin_rec, (rec, twin_rec)
        if table:
            self.check_table()
        return g[0].shape[1]

    def both(self, call):
        return call(self.an), call(self.twin)


def _kinds(n):
    """the tracks a context mixes, as (kind, clip length in samples; for the one-shot in outputs)"""
    lengths = [L for L in dict.fromkeys([1, 5, 7, n - 1, 100003]) if L >= 1]
    return ([("input", 0), ("plain", 1000)] + [("loop", L) for L in lengths] +
            [("oneshot", n + n // 2 + 1), ("paused", 50), ("stopped", 50), ("nofile", 0)])


def _run_mix(gpu_fx, C, N, device, n, kinds, ticks, turn):
    rig = Rig(gpu_fx, C, N, device)
    track_kind = [kinds[t % len(kinds)] for t in range(C)]
    # every track with a file gets a clip of its own; the rated ones walk the ratios and the formats (7 and 4: every pair in turn)
    key, per_fmt, rates, loops = {}, {f: [] for f in cm.FORMATS}, {f: [] for f in cm.FORMATS}, {}
    rated = 0
    for t, (kind, L) in enumerate(track_kind):
        if kind in ("input", "nofile"):
            continue
        if kind == "plain":
            fmt, rate = "f32", 0.0
        else:
            fmt, ratio = cm.FORMATS[(rated + turn) % 4], RATIOS[(rated + turn) % 7]
            rate = RATE * ratio
            rated += 1
            if kind == "oneshot":
                L = max(1, int(L * ratio))              # it ends inside the second tick: after n + n / 2 + 1 outputs
        key[t] = (fmt, len(per_fmt[fmt]))
        per_fmt[fmt].append(_cut(fmt, t + 7 * turn, L))
        rates[fmt].append(rate)
        loops[t] = 0 if kind == "oneshot" else 1
    for fmt in cm.FORMATS:
        if per_fmt[fmt]:
            rig.bank(fmt, per_fmt[fmt], rates[fmt])
    with_clip = sorted(key)
    rig.load(with_clip, [key[t] for t in with_clip], [loops[t] for t in with_clip])
    files = [t for t in range(C) if track_kind[t][0] != "input"]
    rig.sources(files, [cm.FILE] * len(files))
    rig.transport([t for t in with_clip if track_kind[t][0] != "stopped"], cm.PLAY)
    rig.both(lambda a: a.enable_display(64, 256))
    paused = [t for t in range(C) if track_kind[t][0] == "paused"]
    live = _live(C, n * ticks)
    frames = 0
    for k in range(ticks):
        frames += rig.tick(np.ascontiguousarray(live[:, k * n:(k + 1) * n]), n, table=(k % 64 == 0 or k == ticks - 1))
        if k == 0 and paused:
            rig.transport(paused, cm.PAUSE)             # with k that is not 0, and (n < hop) samples pending
    assert frames == (n * ticks) // (N // 2) >= 3
    state = rig.m.table()["state"]
    for c in range(C):
        want = {"paused": cm.PAUSED, "stopped": cm.STOPPED, "nofile": cm.NO_FILE, "loop": cm.PLAYING, "plain": cm.PLAYING}.get(track_kind[c][0])
        assert want is None or state[c] == want, (c, track_kind[c])
        if track_kind[c][0] == "oneshot" and ticks >= 2:
            assert state[c] == cm.FINISHED
        if track_kind[c][0] == "paused":
            assert rig.m.players[c].k == n
    g, w = rig.both(lambda a: a.display())
    assert g.shape == w.shape and same(g, w) and np.abs(g).max() > 0
    rig.close()


@pytest.mark.parametrize("part", ["all", "first", "second"])
@pytest.mark.parametrize("i,n", list(enumerate(BLOCKS)))
def test_rated_sources_equal_the_planar_twin(gpu_fx, i, n, part):
    N = (256, 1024)[i % 2]
    H = N // 2
    ticks = max(3, -(-(3 * H + (77 if n > 1 else 0)) // n))
    kinds = _kinds(n)
    half = (len(kinds) + 1) // 2
    if part == "all":
        _run_mix(gpu_fx, 14, N, bool(i % 2), n, kinds, ticks, i)
    else:
        _run_mix(gpu_fx, 6, N, not i % 2, n, kinds[:half] if part == "first" else kinds[half:], ticks, i + 3)


def _small_rig(gpu_fx, device, C=8, N=1024, sample_rate=RATE):
    rig = Rig(gpu_fx, C, N, device, sample_rate)
    rig.bank("f32", [_cut("f32", k, L) for k, L in enumerate([700, 333, 1500])], [44100.0, 0.0, 96000.0])
    rig.bank("s16", [_cut("s16", 10 + k, L) for k, L in enumerate([700, 50, 2000])], [44100.0, 96000.0, 22050.0])
    rig.bank("s24", [_cut("s24", 20, 901)], [0.0])
    return rig


@pytest.mark.parametrize("device", [False, True])
def test_commands_mid_stream(gpu_fx, device):
    rig = _small_rig(gpu_fx, device)
    C, n = rig.C, 480
    live = _live(C, n * 40)
    at = [0]

    def tick(count=1):
        for _ in range(count):
            rig.tick(np.ascontiguousarray(live[:, at[0] * n:(at[0] + 1) * n]), n)
            at[0] += 1

    tick()                                                      # every track on its input: no resampler launch
    rig.load([0, 1, 2, 3], [("s16", 0), ("f32", 2), ("s16", 2), ("s16", 1)], [1, 0, 1, 0])     # 1 and 3 are one-shots (1500 @ 96k, 50 @ 96k)
    rig.sources([0, 1, 2, 3, 4], [cm.FILE] * 5)                 # track 4 has no file
    rig.check_table()
    tick()                                                      # all stopped: the launch is made, every row stays silent
    rig.transport([0, 1, 2, 3], cm.PLAY)
    tick()                                                      # 3 finishes inside the tick (25 outputs), 1 plays on (750 outputs)
    assert rig.m.players[3].state == cm.FINISHED and rig.m.players[1].state == cm.PLAYING
    rig.transport([0], cm.PAUSE)
    tick()                                                      # 1 finishes
    assert rig.m.players[1].state == cm.FINISHED and rig.m.players[0].k == n
    rig.transport([0], cm.PLAY)                                 # from PAUSED: the phase is kept
    tick()
    assert rig.m.players[0].k == 2 * n
    rig.transport([0, 1], cm.PLAY)                              # playing stays; from FINISHED: from the top
    assert rig.m.players[1].k == 0
    rig.check_table()
    tick()
    rig.transport([2, 3], cm.RESTART)                           # a playing loop goes back and plays on; FINISHED becomes STOPPED
    assert rig.m.players[2].k == 0
    rig.check_table()
    tick()
    rig.transport([2], cm.STOP)
    rig.check_table()
    tick()
    rig.transport([2, 2], cm.PLAY)
    tick(2)
    rig.transport([0], cm.PAUSE)
    rig.transport([0], cm.RESTART)                              # restart while paused: k 0, still paused
    assert (rig.m.players[0].state, rig.m.players[0].k) == (cm.PAUSED, 0)
    tick()
    rig.transport([0], cm.PLAY)
    tick()
    rig.sources([2, 5], [cm.INPUT, cm.FILE])                    # 2 back to its input (its player stops, k 0), 5 to no file
    tick()
    rig.sources([2], [cm.FILE])
    rig.transport([2], cm.PLAY)
    tick()
    rig.load([0, 2], [("f32", 2), ("f32", 1)], [1, 1])          # a clip replaced by one of another rate (44.1k -> 96k), and by an unrated one
    rig.transport([0, 2], cm.PLAY)
    tick(2)
    # a rate changed on a clip nobody has loaded, then loaded; on a loaded clip the change is refused with nothing changed
    rig.set_rates([("f32", 0), ("s24", 0)], [32000.0, 88200.0])
    before = rig.an.transport_state()
    with pytest.raises(gpu_fx.FxError, match="track 0"):
        rig.an.set_clip_rates([rig.clip_id(("s24", 0)), rig.clip_id(("f32", 2))], [44100.0, 44100.0])
    assert rig.rates["s24"][0] == 88200.0
    after = rig.an.transport_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    rig.load([5, 6], [("f32", 0), ("s24", 0)], [1, 0])
    rig.sources([6], [cm.FILE])
    rig.transport([5, 6], cm.PLAY)
    assert rig.m.players[6].r == 88200.0 / RATE and rig.m.players[5].r == 32000.0 / RATE        # (not 44100: the refused call set nothing)
    tick(3)
    assert rig.m.players[6].state == cm.FINISHED
    rig.load([0], [None])                                       # the file taken away
    rig.check_table()
    tick()
    rig.close()


def test_refusals_change_nothing(gpu_fx):
    rig = _small_rig(gpu_fx, False, C=4)
    C, n = rig.C, 441
    live = _live(C, n * 12)
    rig.load([0, 1], [("f32", 0), ("s16", 1)], [1, 1])          # 44.1k fp32 and 96k s16
    rig.sources([0, 1, 2], [cm.FILE] * 3)
    rig.transport([0], cm.PLAY)                                 # track 1 stays stopped: its clip counts all the same
    rig.tick(np.ascontiguousarray(live[:, :n]), n)
    assert rig.an.pending_samples() == 441
    before = rig.an.transport_state()
    Err = gpu_fx.FxError

    def unchanged():
        assert rig.an.pending_samples() == 441 and rig.an.last_launches() == []
        after = rig.an.transport_state()
        for k in before:
            assert np.array_equal(before[k], after[k]), k

    # a tick that is not fp32 while a rated clip is loaded on a FILE track, whatever its state
    for fmt_block in (np.zeros((C, n), np.float16), np.zeros((C, n), np.int16)):
        with pytest.raises(Err, match="track 0"):
            rig.an.push_sources(fmt_block)
        unchanged()
    rig.sources([0], [cm.INPUT])
    before = rig.an.transport_state()
    with pytest.raises(Err, match="track 1"):                  # the stopped track's clip
        rig.an.push_sources(np.zeros((C, n), np.float16))
    unchanged()
    rig.sources([0], [cm.FILE])
    rig.transport([0], cm.PLAY)
    before = rig.an.transport_state()
    # r = 9
    rig.set_rates([("f32", 2)], [RATE * 9])
    with pytest.raises(Err, match="entry 1"):
        rig.an.load_clips([3, 2], [rig.clip_id(("f32", 1)), rig.clip_id(("f32", 2))])
    unchanged()
    rig.set_rates([("f32", 2)], [RATE / 8.5])
    with pytest.raises(Err, match="entry 0"):
        rig.an.load_clips([2], [rig.clip_id(("f32", 2))])
    unchanged()
    rig.check_table()
    rig.tick(np.ascontiguousarray(live[:, n:2 * n]), n)
    # the context's rate changes: the loaded clips' ratios are stale, and a tick is refused until they are loaded again
    pending = rig.an.pending_samples()
    rig.both(lambda a: a.sample_rate_changed(44100.0))
    rig.m.sample_rate = 44100.0
    before = rig.an.transport_state()
    with pytest.raises(Err, match="track 0"):
        rig.an.push_sources(np.ascontiguousarray(live[:, 2 * n:3 * n]))
    assert rig.an.pending_samples() == pending and rig.an.last_launches() == []
    after = rig.an.transport_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    rig.load([0], [("f32", 0)])                                 # at 44.1k in a 44.1k context: not rated any more
    with pytest.raises(Err, match="track 1"):
        rig.an.push_sources(np.ascontiguousarray(live[:, 2 * n:3 * n]))
    rig.load([1], [("s16", 1)])
    assert not rig.m.players[0].rated and rig.m.players[1].r == 96000.0 / 44100.0
    rig.transport([0, 1], cm.PLAY)
    for k in range(2, 8):
        rig.tick(np.ascontiguousarray(live[:, k * n:(k + 1) * n]), n)
    rig.close()


@pytest.mark.parametrize("device", [False, True])
def test_a_clip_at_the_contexts_own_rate_is_the_byte_path(gpu_fx, device):
    rig = Rig(gpu_fx, 5, 1024, device)
    rig.bank("f32", [_cut("f32", k, L) for k, L in enumerate([700, 5, 1500])], [RATE, 48000.0, 0.0])
    rig.load([0, 1, 2], [("f32", 0), ("f32", 1), ("f32", 2)], [1, 1, 0])
    rig.sources([0, 1, 2, 3], [cm.FILE] * 4)
    rig.transport([0, 1, 2], cm.PLAY)
    assert not any(p.rated for p in rig.m.players)
    live = _live(5, 480 * 6)
    for k in range(6):
        rig.tick(np.ascontiguousarray(live[:, k * 480:(k + 1) * 480]), 480)            # records "sources" + the twin's, no "resample"
        assert [r["kind"] for r in rig.an.last_launches()].count("resample") == 0
    assert rig.m.players[2].state == cm.FINISHED and rig.m.players[0].laps == 4
    rig.close()


def test_rated_clips_in_a_bank_past_2_to_the_31_bytes(gpu_fx):
    """one borrowed s16 device bank of more than 2^31 bytes: the rated tracks play short clips that start past byte 2^31, so every
    address the resampler reads is past it.  The model is fed those slices only."""
    import torch
    C, N, n = 8, 1024, 1000
    lengths = [(1 << 30) + 1, 50001, 7, 1, 30011, 1200]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    assert starts[1] * 2 > 1 << 31
    bank = torch.randint(-12000, 12000, (int(sum(lengths)),), dtype=torch.int16, device="cuda")
    rig = Rig(gpu_fx, C, N, True)
    rates = [0.0, 44100.0, 96000.0, 6000.0, RATE * 8, 72000.0]
    rig.first["s16"] = rig.an.create_clips(bank, lengths=lengths, borrow=True, sample_rates=rates)
    rig.clips["s16"] = [None] + [cm.raw(bank[int(starts[k]):int(starts[k]) + lengths[k]].cpu().numpy()[None, :])[0] for k in range(1, len(lengths))]
    rig.rates["s16"] = rates
    clip = [1 + t % 5 for t in range(C)]
    rig.load(list(range(C)), [("s16", k) for k in clip], [0 if k == 5 else 1 for k in clip])
    rig.sources(list(range(C)), [cm.FILE] * C)
    rig.transport(list(range(C)), cm.PLAY)
    for _ in range(4):
        rig.tick(None, n)
    t = rig.m.table()
    assert t["state"][4] == cm.FINISHED and t["laps"][1] > 100 and t["position"][0] == int(np.floor(4 * n * (44100.0 / RATE)))
    first = rig.first["s16"]
    rig.load(list(range(C)), [None] * C)
    rig.an.destroy_clips(first)
    rig.close()


def test_cpp_clip_rates_mirror(gpu_fx, tmp_path):
    gpu_fx.load_library()
    exe = str(tmp_path / "clip_rates_mirror")
    lib_dir = os.path.dirname(gpu_fx.library_path())
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "clip_rates_mirror.cpp"), "-o", exe, "-L", lib_dir, "-lfx_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "clip_rates_mirror: ok" in out.stdout
