"""File sources on the GPU (include/fx.h, fx_create_clips .. fx_push_sources): context A runs sources, its twin B is given
push_samples(the model's planar block) and clear_pending_channels at the model's points (tests/clip_model.py).  After every tick raw,
smoothed, frame counts and pending_samples() are equal bit for bit, the launch record is "sources" (T = n) followed by the twin's
record, and transport_state() is the model's table; get_features() is compared where a case ends.

Tracks per context.  The kinds a context must mix (an INPUT track, looping clips of seven lengths, a one-shot that ends inside a tick,
a paused, a stopped and a no-file track) are twelve, so the contexts that mix them have 14 tracks (70 for two of the block lengths: a
partial second group of 64); the same blocks also run through two contexts of 6 tracks that hold one half of the kinds each, where the
whole staging buffer is a handful of 16-byte pieces (12 bytes for one 16-bit sample per track)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import clip_model as cm
import interleave_model as im
import signals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [1, 63, 441, 480, 512, 1000, 4097]
NS = [256, 1024, 2048, 4096]
# every (format, block) pair once; window size and memory kind walk their own cycles, so each value of each axis is met
CASES = [(NS[i % 4], fmt, bool(i % 2), block) for i, (fmt, block) in enumerate((f, b) for f in cm.FORMATS for b in BLOCKS)]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _torch(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(r):
    return None if r is None else (r.cpu().numpy() if hasattr(r, "cpu") else r)


@functools.lru_cache(maxsize=None)
def _tape(fmt):
    """one long stretch of audio in `fmt`, as bytes: clips and live rows are cut from it"""
    x = signals.tone_vibrato_noise(1, 400, 1024, seed=21).reshape(-1).astype(np.float32)
    return cm.raw(im.encode(x[None, :], fmt))[0]


def _cut(fmt, k, L):
    """clip number k: L samples of the tape from a place of its own"""
    B = cm.BYTES[fmt]
    at = (k * 7919) % (_tape(fmt).size // B - L)
    return _tape(fmt)[at * B:(at + L) * B].copy()


def _live(fmt, C, total):
    B = cm.BYTES[fmt]
    room = _tape(fmt).size // B - total
    return np.stack([_tape(fmt)[((c * 4099) % room) * B:((c * 4099) % room + total) * B] for c in range(C)])


class Rig:
    """a sources context, its twin and the model between them"""

    def __init__(self, gpu_fx, C, N, fmt, device):
        self.fx, self.C, self.N, self.fmt, self.B, self.device = gpu_fx, C, N, fmt, cm.BYTES[fmt], device
        self.an, self.twin = gpu_fx.BatchAnalyser(C, N), gpu_fx.BatchAnalyser(C, N)
        for a in (self.an, self.twin):
            a.set_gain(0.75)
        self.m = cm.Model(C, fmt)
        self.clips, self.first = [], None

    def close(self):
        assert same(self.an.get_features(), self.twin.get_features())
        self.an.close(); self.twin.close()

    def _arr(self, block):
        t = cm.typed(block, self.fmt)
        return _torch(t) if self.device else t

    def bank(self, clips):
        """the clips back to back in ONE bank (so 16- and 24-bit clips start at odd addresses): clip k of the rig is self.first + k"""
        assert self.first is None
        self.clips = clips
        self.first = self.an.create_clips(self._arr(np.concatenate(clips)), lengths=[c.size // self.B for c in clips], sample_format=self.fmt)
        return self.first

    def _cleared(self, tracks):
        if tracks:
            self.twin.clear_pending_channels(tracks)

    def load(self, channels, keys, loop=None):
        self.an.load_clips(channels, [-1 if k is None else self.first + k for k in keys], loop)
        self._cleared(self.m.load(channels, [None if k is None else self.clips[k] for k in keys], loop))

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
        """one tick: `live` uint8 [C][n * B] or None"""
        planar = self.m.tick(live, n)
        if live is None:
            got = self.an.push_sources(None, n, sample_format=self.fmt, device=self.device)
        else:
            got = self.an.push_sources(self._arr(live), sample_format=self.fmt)
        want = self.twin.push_samples(self._arr(planar), sample_format=self.fmt)
        g, w = [_host(x) for x in got], [_host(x) for x in want]
        assert g[0].shape == w[0].shape and same(g[0], w[0]) and same(g[1], w[1])
        assert self.an.pending_samples() == self.twin.pending_samples()
        rec, twin_rec = self.an.last_launches(), self.twin.last_launches()
        assert rec[0]["kind"] == "sources" and rec[0]["T"] == n
        assert rec[1:] == twin_rec, (rec, twin_rec)
        if table:
            self.check_table()
        return g[0].shape[1]

    def both(self, call):
        """the same call on both contexts (what is not part of the feature: resets, taps, the display)"""
        return call(self.an), call(self.twin)


def _kinds(n):
    """the tracks a context mixes, as (kind, clip length)"""
    lengths = [L for L in dict.fromkeys([1, 5, 7, n - 1, n, n + 1, 100003]) if L >= 1]
    return ([("input", 0)] + [("loop", L) for L in lengths] +
            [("oneshot", n + n // 2 + 1), ("paused", 50), ("stopped", 50), ("nofile", 0)])


def _run_mix(gpu_fx, C, N, fmt, device, n, kinds, ticks):
    rig = Rig(gpu_fx, C, N, fmt, device)
    track_kind = [kinds[t % len(kinds)] for t in range(C)]
    with_clip = [t for t in range(C) if track_kind[t][1]]
    rig.bank([_cut(fmt, t, track_kind[t][1]) for t in with_clip])
    rig.load(with_clip, list(range(len(with_clip))), [0 if track_kind[t][0] == "oneshot" else 1 for t in with_clip])
    files = [t for t in range(C) if track_kind[t][0] != "input"]
    rig.sources(files, [cm.FILE] * len(files))
    rig.transport([t for t in with_clip if track_kind[t][0] != "stopped"], cm.PLAY)
    paused = [t for t in range(C) if track_kind[t][0] == "paused"]
    live = _live(fmt, C, n * ticks)
    frames = 0
    for k in range(ticks):
        frames += rig.tick(np.ascontiguousarray(live[:, k * n * rig.B:(k + 1) * n * rig.B]), n, table=(k % 64 == 0 or k == ticks - 1))
        if k == 0 and paused:
            rig.transport(paused, cm.PAUSE)        # with a position that is not 0, and (n < hop) samples pending
    assert frames == (n * ticks) // (N // 2)
    t = rig.m.table()
    if ticks >= 2:
        for c in range(C):
            want = {"oneshot": cm.FINISHED, "paused": cm.PAUSED, "stopped": cm.STOPPED, "nofile": cm.NO_FILE, "loop": cm.PLAYING}.get(track_kind[c][0])
            assert want is None or t["state"][c] == want, (c, track_kind[c])
    rig.close()


@pytest.mark.parametrize("N,fmt,device,n", CASES)
def test_sources_equal_the_planar_twin(gpu_fx, N, fmt, device, n):
    H = N // 2
    total = H + 5 if n == 1 else 3 * H + 77
    ticks = max(3, -(-total // n))
    kinds = _kinds(n)
    _run_mix(gpu_fx, 70 if n in (441, 4097) else 14, N, fmt, device, n, kinds, ticks)
    half = (len(kinds) + 1) // 2
    for part in (kinds[:half], kinds[half:]):
        _run_mix(gpu_fx, 6, N, fmt, device, n, part, ticks)


def _small_rig(gpu_fx, fmt, device, C=8, N=1024):
    rig = Rig(gpu_fx, C, N, fmt, device)
    rig.bank([_cut(fmt, k, L) for k, L in enumerate([700, 333, 1500, 50, 2000])])
    return rig


@pytest.mark.parametrize("fmt,device", [("f32", False), ("s24", True), ("s16", False)])
def test_commands_mid_stream(gpu_fx, fmt, device):
    rig = _small_rig(gpu_fx, fmt, device)
    C, n, B = rig.C, 480, rig.B
    live = _live(fmt, C, n * 40)
    at = [0]

    def tick(count=1):
        for _ in range(count):
            rig.tick(np.ascontiguousarray(live[:, at[0] * n * B:(at[0] + 1) * n * B]), n)
            at[0] += 1

    tick()                                                      # every track on its input; 480 samples pending
    rig.load([0, 1, 2, 3], [1, 0, 2, 3], [1, 0, 1, 0])          # 1 and 3 are one-shots (700 and 50 samples)
    rig.sources([0, 1, 2, 3, 4], [cm.FILE] * 5)                 # track 4 has no file
    rig.check_table()
    tick()                                                      # all stopped: silence
    rig.transport([0, 1, 2, 3], cm.PLAY)
    tick()                                                      # 3 finishes inside the tick, 1 plays on
    assert rig.m.players[3].state == cm.FINISHED and rig.m.players[1].state == cm.PLAYING
    rig.transport([0], cm.PAUSE)
    tick()                                                      # 1 finishes (700 < 960)
    rig.transport([0], cm.RESTART)                              # restart while paused: position 0, still paused
    assert (rig.m.players[0].state, rig.m.players[0].position) == (cm.PAUSED, 0)
    rig.check_table()
    tick()
    rig.transport([0, 1], cm.PLAY)                              # play from PAUSED and from FINISHED (position 0 again)
    rig.check_table()
    tick()
    rig.transport([2, 3], cm.RESTART)                           # a playing loop goes back and plays on; FINISHED becomes STOPPED
    rig.check_table()
    tick()
    rig.transport([2], cm.STOP)
    rig.transport([2, 2], cm.PLAY)                              # a duplicate in the list
    tick(2)
    assert rig.m.players[0].state == cm.PLAYING
    rig.sources([0, 0], [cm.INPUT, cm.FILE])                    # the last entry of a track wins: the type does not change, the player
    assert rig.m.players[0].state == cm.PLAYING                 # plays on, and the pending samples are zeroed all the same
    rig.check_table()
    tick()
    rig.sources([0, 5], [cm.INPUT, cm.FILE])                    # a switch both ways: 0 back to its input (its player stops), 5 to no file
    assert (rig.m.players[0].state, rig.m.players[0].position) == (cm.STOPPED, 0)
    tick()
    rig.sources([0], [cm.FILE])                                 # and back to the file: stopped at 0 until it is played
    rig.check_table()
    tick()
    rig.transport([0], cm.PLAY)
    tick()
    rig.load([0, 2], [4, 0], [1, 1])                            # a clip replaced; clip 0 now loops on track 2 and plays once on track 1
    rig.transport([0, 2], cm.PLAY)
    tick(2)
    rig.load([1], [0], [1])                                     # `loop` changed on track 1
    rig.transport([1], cm.PLAY)
    tick(5)
    assert rig.m.players[1].laps >= 3
    rig.load([2], [None])                                       # the file taken away
    rig.check_table()
    tick()
    rig.close()


def test_refused_lists_change_nothing(gpu_fx):
    rig = _small_rig(gpu_fx, "f32", False)
    C, n, B = rig.C, 441, rig.B
    live = _live("f32", C, n * 8)
    rig.load([0, 1], [0, 1])
    rig.sources([0, 1, 2], [cm.FILE] * 3)
    rig.transport([0, 1], cm.PLAY)
    rig.tick(np.ascontiguousarray(live[:, :n * B]), n)
    assert rig.an.pending_samples() == 441
    before = rig.an.transport_state()
    Err = gpu_fx.FxError
    # a bad entry, through the C ABI (the binding refuses it before): every entry is checked before anything changes
    bad = (ctypes.c_int * 2)(0, 99)
    assert rig.an._lib.fx_transport(rig.an._h, bad, 2, cm.STOP) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"entry 1" in rig.an._lib.fx_last_error()
    for call in (lambda a: a.transport([0, 2], "play"),                         # track 2 has no file
                 lambda a: a.transport([0], 7),
                 lambda a: a.load_clips([0, 1], [rig.first, rig.first + 99]),
                 lambda a: a.set_sources([0, 1], [1, 5]),
                 lambda a: a.push_sources(None, n, sample_format="f32"),        # tracks 3.. listen to the input
                 lambda a: a.push_sources(np.ascontiguousarray(cm.typed(live[:, :n * B], "f32")).astype(np.float16))):   # pending samples are f32
        with pytest.raises(Err):
            call(rig.an)
        assert rig.an.pending_samples() == 441
    assert rig.an.last_launches() == []
    after = rig.an.transport_state()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    rig.check_table()
    # and the next valid calls are the ones that would have followed: the pending samples are those of before
    for k in range(1, 5):
        rig.tick(np.ascontiguousarray(live[:, k * n * B:(k + 1) * n * B]), n)
    rig.close()


def test_format_of_a_loaded_clip_must_be_the_calls(gpu_fx):
    rig = _small_rig(gpu_fx, "s16", False, C=3)
    rig.load([1], [0])
    rig.sources([1], [cm.FILE])                                 # stopped: its clip would not even be read
    with pytest.raises(gpu_fx.FxError, match="track 1"):
        rig.an.push_sources(np.zeros((3, 64), np.float32))
    assert rig.an.last_launches() == [] and rig.an.pending_samples() == 0
    rig.check_table()
    rig.tick(_live("s16", 3, 64), 64)
    rig.close()


def test_plain_calls_between_ticks_ignore_the_table(gpu_fx):
    rig = _small_rig(gpu_fx, "f32", True)
    C, B = rig.C, rig.B
    rig.load([0, 1, 2], [0, 1, 2], [1, 0, 1])
    rig.sources([0, 1, 2], [cm.FILE] * 3)
    rig.transport([0, 1, 2], cm.PLAY)
    live = _live("f32", C, 6000)
    at = 0
    for i, n in enumerate([480, 441, 1000, 63, 512, 2000, 1]):
        piece = np.ascontiguousarray(live[:, at * B:(at + n) * B])
        if i % 2:
            g, w = rig.both(lambda a: a.push_samples(rig._arr(piece)))      # the plain call: the live block on every track
            assert same(_host(g[0]), _host(w[0])) and same(_host(g[1]), _host(w[1]))
            assert rig.an.last_launches() == rig.twin.last_launches()
            rig.check_table()                                                # no position has moved
        else:
            rig.tick(piece, n)
        at += n
    rig.close()


def test_taps_and_display_armed_before_a_tick(gpu_fx):
    rig = _small_rig(gpu_fx, "s24", False, C=5)
    n, B = 700, rig.B
    rig.load([0, 3], [2, 4])
    rig.sources([0, 3, 4], [cm.FILE] * 3)
    rig.transport([0, 3], cm.PLAY)
    live = _live("s24", 5, 3 * n)
    rig.both(lambda a: a.enable_display(64, 256))
    rig.tick(np.ascontiguousarray(live[:, :n * B]), n)
    rig.both(lambda a: a.request_taps([0, 1, 4]))
    rig.tick(np.ascontiguousarray(live[:, n * B:2 * n * B]), n)
    rig.tick(np.ascontiguousarray(live[:, 2 * n * B:]), n)
    for ch in (0, 1, 4):
        g, w = rig.an.taps(ch), rig.twin.taps(ch)
        assert g["frame_index"] == w["frame_index"]
        for k in g:
            assert same(g[k], w[k]), (ch, k)
    g, w = rig.both(lambda a: a.display())
    assert g.shape == w.shape and same(g, w) and np.abs(g[0]).max() > 0
    rig.close()


@pytest.mark.parametrize("device", [False, True])
def test_all_tracks_on_files_need_no_live_block(gpu_fx, device):
    rig = _small_rig(gpu_fx, "f16", device, C=5)
    rig.load([0, 1, 2, 3], [0, 1, 2, 3], [1, 0, 1, 1])
    rig.sources([0, 1, 2, 3], [cm.FILE] * 4)
    rig.transport([0, 1, 2, 3], cm.PLAY)
    # one track still listens to the input: a tick without a live block is refused with nothing changed
    with pytest.raises(gpu_fx.FxError, match="track 4"):
        rig.an.push_sources(None, 480, sample_format="f16", device=device)
    assert rig.an.last_launches() == [] and rig.an.pending_samples() == 0
    rig.check_table()
    rig.sources([4], [cm.FILE])
    for n in (480, 480, 1, 2000, 512):
        rig.tick(None, n)
    rig.close()


def test_bank_past_2_to_the_31_bytes(gpu_fx):
    """one borrowed device bank of more than 2^31 bytes: the clips that play start past byte 2^31, so every address the gather reads is
    past it, and the first clip is longer than 2^31 bytes by itself.  The twin is fed slices of the same tensor."""
    import torch
    C, N, n = 64, 1024, 30000
    lengths = [(1 << 30) + 1, 100003, 7, 50001, 1, 250001]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    assert starts[1] * 2 > 1 << 31
    bank = torch.randint(-12000, 12000, (int(sum(lengths)),), dtype=torch.int16, device="cuda")
    an, twin = gpu_fx.BatchAnalyser(C, N), gpu_fx.BatchAnalyser(C, N)
    first = an.create_clips(bank, lengths=lengths, borrow=True)
    clip = [[1, 2, 3, 4, 5, 0][t % 6] for t in range(C)]
    loop = [0 if clip[t] == 3 else 1 for t in range(C)]
    an.load_clips(list(range(C)), [first + k for k in clip], loop)
    an.set_sources(list(range(C)), "file")
    an.transport(list(range(C)), "play")
    position, laps, state = np.zeros(C, np.int64), np.zeros(C, np.int64), np.full(C, cm.PLAYING, np.int32)
    i = torch.arange(n, device="cuda", dtype=torch.int64)
    for tick in range(4):
        rows = []
        for t in range(C):
            L, s = lengths[clip[t]], int(starts[clip[t]])
            if state[t] != cm.PLAYING:
                rows.append(torch.zeros(n, dtype=torch.int16, device="cuda"))
            elif loop[t]:
                rows.append(bank[s + (position[t] + i) % L])
                laps[t] += (position[t] + n) // L
                position[t] = (position[t] + n) % L
            else:
                x = position[t] + i
                rows.append(torch.where(x < L, bank[s + torch.clamp(x, max=L - 1)], torch.zeros((), dtype=torch.int16, device="cuda")))
                if position[t] + n >= L:
                    state[t] = cm.FINISHED
                position[t] = min(position[t] + n, L)
        planar = torch.stack(rows).contiguous()
        got = an.push_sources(None, n, sample_format="s16", device=True)
        want = twin.push_samples(planar)
        assert got[0].shape == (C, (tick + 1) * n // 512 - tick * n // 512, 12)
        assert torch.equal(got[0].nan_to_num(1e30), want[0].nan_to_num(1e30)) and torch.equal(got[1].nan_to_num(1e30), want[1].nan_to_num(1e30))
        assert an.pending_samples() == twin.pending_samples()
        rec = an.last_launches()
        assert rec[0]["kind"] == "sources" and rec[1:] == twin.last_launches()
        tab = an.transport_state()
        assert np.array_equal(tab["position"], position) and np.array_equal(tab["laps"], laps) and np.array_equal(tab["state"], state)
    assert state[2] == cm.FINISHED and laps[1] > 1000 and position[5] == 4 * n
    assert same(an.get_features(), twin.get_features())
    an.load_clips(list(range(C)), -1)
    an.destroy_clips(first)
    an.close(); twin.close()


def test_bank_lifetime_and_resets_leave_the_transport_alone(gpu_fx):
    rig = _small_rig(gpu_fx, "f32", False, C=4)
    n, B = 480, rig.B
    live = _live("f32", 4, n * 8)
    second = rig.an.create_clips([cm.typed(_cut("f32", 9, 100), "f32"), cm.typed(_cut("f32", 10, 20), "f32")])
    assert second == rig.first + 5
    rig.load([0, 1], [0, 1], [1, 0])
    rig.sources([0, 1, 2], [cm.FILE] * 3)
    rig.transport([0, 1], cm.PLAY)
    rig.tick(np.ascontiguousarray(live[:, :n * B]), n)
    with pytest.raises(gpu_fx.FxError, match="track 0"):
        rig.an.destroy_clips(rig.first)
    with pytest.raises(gpu_fx.FxError, match="no bank"):
        rig.an.destroy_clips(rig.first + 1)             # not the first id of a bank
    rig.an.destroy_clips(second)                        # nobody plays from it
    with pytest.raises(gpu_fx.FxError, match="unknown clip id"):
        rig.an.load_clips([3], [second])
    rig.check_table()
    rig.tick(np.ascontiguousarray(live[:, n * B:2 * n * B]), n)
    # the resets are the analysers': the players go on where they were
    rig.both(lambda a: a.reset_channels([0, 3]))
    rig.check_table()
    rig.tick(np.ascontiguousarray(live[:, 2 * n * B:3 * n * B]), n)
    rig.both(lambda a: a.reset_state())
    assert rig.an.pending_samples() == 0
    rig.check_table()
    rig.tick(np.ascontiguousarray(live[:, 3 * n * B:4 * n * B]), n)
    rig.tick(np.ascontiguousarray(live[:, 4 * n * B:5 * n * B]), n)
    assert rig.m.players[0].position > 0 and rig.m.players[1].state == cm.FINISHED
    rig.load([0, 1], [None, None])
    rig.an.destroy_clips(rig.first)
    rig.tick(np.ascontiguousarray(live[:, 5 * n * B:6 * n * B]), n)
    rig.close()


def test_cpp_file_player_mirror(gpu_fx, tmp_path):
    gpu_fx.load_library()
    exe = str(tmp_path / "clip_mirror")
    lib_dir = os.path.dirname(gpu_fx.library_path())
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "clip_mirror.cpp"),
                           "-o", exe, "-L", lib_dir, "-lfx_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "clip_mirror: ok" in out.stdout
