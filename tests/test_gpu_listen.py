"""Listening tracks on the GPU (include/fx.h, "LISTENING TRACKS": fx_set_channel_listen / fx_get_channel_listen).  The method is the
twin method of tests/test_gpu_clips.py and tests/test_gpu_monitor.py: context A runs push_sources with a monitor and tracks that
listen to its outputs, its plain twin B is given push_samples(listen_model.heard(the model's block, the model's mix, the listens)).
After every tick raw, smoothed, frame counts and pending_samples() are the twin's bit for bit, get_monitor() is monitor_model.mix of
the UNMODIFIED block, and the launch record is sources, resample if any, monitor, listen if anybody listens (T = n each), then the
twin's record.  Every stream ends with a tick that completes a hop, so what the last ticks left pending is compared as well.

run_case() also runs without a GPU (fx None): tests/test_listen_cpu.py uses that to show that THIS data tells a listening track from
a track that hears itself, and the left output from the right one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clip_model as cm
import listen_model as lm
import monitor_model as mm
import test_gpu_clips as tc
import test_gpu_monitor as tg
import test_gpu_resample as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACKS = [6, 64, 70, 130]
# rows at every dword alignment (n % 4 = 1, 3, 3, 1, 0, 0, 0, 1), tails of 1 and 3 dwords, rows shorter than one 16-byte piece, the
# last row's end, more than one 512-sample tile, and a hop (512 samples at 1024 points) completed inside one tick
BLOCKS = [1, 3, 63, 441, 480, 512, 1000, 4097]
LAST = 100                  # the last common tick: 6597 samples are 12 hops and 453 pending, 100 more complete the thirteenth
N = 1024
NAMES = {"self": lm.SELF, "left": lm.LEFT, "right": lm.RIGHT}


class Listening:
    """what a rig of test_gpu_monitor needs to hold listening tracks to the model: the listens, and a tick whose twin hears the mix"""

    def start_listen(self):
        self.listen = np.zeros(self.C, np.int32)
        self.heard = []                     # (n, the block the analysers get, the tracks' own block, the mix, the listens) per tick
        self.got_mixes, self.last = [], None

    def listens(self, channels, values):
        self.an.set_listen(channels, values)
        per_entry = values if isinstance(values, (list, tuple, np.ndarray)) else [values] * len(channels)
        for c, v in zip(channels, per_entry):       # in list order: the last entry of a track wins
            self.listen[c] = NAMES.get(v, v)
        self._cleared(list(channels))               # toggleCollectInput clears the collector, whichever way it is switched

    def check_listens(self):
        if not self.dry:
            got = self.an.listens()
            assert got.dtype == np.int32 and np.array_equal(got, self.listen), (got, self.listen)

    def tick(self, live, n, table=True):
        resampled = any(p.source == cm.FILE and getattr(p, "rated", False) for p in self.m.players)
        planar = self.m.tick(live, n)
        want, x = self.expected(planar)             # the mix of every track's OWN row
        block = lm.heard(x, want, self.listen)
        self.mixes.append((n, want, x, (self.on.copy(), self.left.copy(), self.right.copy())))
        self.heard.append((n, block, x, want, self.listen.copy()))
        if self.dry:
            return 0
        if live is None:
            got = self.an.push_sources(None, n, sample_format="f32", device=self.device)
        else:
            got = self.an.push_sources(self._arr(live), sample_format="f32")
        twin = self.twin.push_samples(tc._torch(block) if self.device else block)
        g, w = [tc._host(r) for r in got], [tc._host(r) for r in twin]
        assert g[0].shape == w[0].shape and tc.same(g[0], w[0]) and tc.same(g[1], w[1]), np.flatnonzero((g[0] != w[0]).any(axis=(1, 2)))
        assert self.an.pending_samples() == self.twin.pending_samples()
        rec, twin_rec = self.an.last_launches(), self.twin.last_launches()
        head = ["sources"] + (["resample"] if resampled else []) + ["monitor"] + (["listen"] if self.listen.any() else [])
        assert [r["kind"] for r in rec[:len(head)]] == head and all(r["T"] == n for r in rec[:len(head)]), rec
        assert rec[len(head):] == twin_rec[:self.fx.capi.LAUNCH_RECORD_CAP - len(head)], (rec, twin_rec)
        self.check_monitor(want)
        self.got_mixes.append(self.an.get_monitor())
        if table:
            self.check_table()
        self.last = g
        return g[0].shape[1]


class ClipRig(Listening, tg.ClipRig):
    def __init__(self, fx, C, device, N=N):
        tg.ClipRig.__init__(self, fx, C, N, "f32", device)
        self.start_listen()


class RatedRig(Listening, tg.RatedRig):
    def __init__(self, fx, C, device):
        tg.RatedRig.__init__(self, fx, C, N, device)
        self.start_listen()


def case_listens(C):
    """SELF / LEFT / RIGHT interleaved: every second track listens, to the left and the right output in turn, so that every listener has
    a track that hears itself on each side; track 0 and track C - 1 listen (and C - 2, the last one's neighbour, does not)"""
    listen = np.zeros(C, np.int32)
    listen[0::4], listen[2::4] = lm.LEFT, lm.RIGHT
    listen[C - 2], listen[C - 1] = lm.SELF, lm.RIGHT
    return listen


def run_case(fx, C, device, blocks, listening=True):
    """one context over ticks of `blocks` samples and the last common tick -> the rig; fx None: the models alone"""
    rig = ClipRig(fx, C, device)
    kinds = tg._kinds(C)
    track_kind = [kinds[(t + C) % len(kinds)] for t in range(C)]
    with_clip = [t for t in range(C) if track_kind[t][1]]
    rig.bank([tg._cut("f32", t, track_kind[t][1]) for t in with_clip])
    rig.load(with_clip, list(range(len(with_clip))), [0 if track_kind[t][0] == "oneshot" else 1 for t in with_clip])
    files = [t for t in range(C) if track_kind[t][0] != "input"]
    rig.sources(files, [cm.FILE] * len(files))
    rig.transport([t for t in with_clip if track_kind[t][0] != "stopped"], cm.PLAY)
    paused = [t for t in range(C) if track_kind[t][0] == "paused"]
    rig.sends(list(range(C)), *tg.case_sends(C, 100 * C + 7))
    if listening:
        rig.listens(list(range(C)), case_listens(C))
    rig.check_listens()
    ticks = list(blocks) + [LAST]
    live = tg._live("f32", C, sum(ticks))
    at = 0
    for k, n in enumerate(ticks):
        rig.tick(np.ascontiguousarray(live[:, at * 4:(at + n) * 4]), n, table=(k == len(ticks) - 1))
        at += n
        if k == 0:
            rig.transport(paused, cm.PAUSE)
        if k == 3 and listening:
            # a listen changed between ticks is in force at the next one; of a track listed twice the last entry wins
            rig.listens([2, 2], [lm.SELF, lm.LEFT])               # (track 2 heard the right output so far)
            rig.check_listens()
    rig.check_listens()
    rig.check_sends()
    rig.close()
    return rig


@pytest.mark.parametrize("C", TRACKS)
def test_listeners_hear_the_mix_and_nobody_else_changes(gpu_fx, C):
    device = C in (64, 130)
    rig = run_case(gpu_fx, C, device, BLOCKS)
    assert [n for n, *_ in rig.heard] == BLOCKS + [LAST]
    assert rig.listen[0] and rig.listen[C - 1] and all(np.abs(m).max(axis=1).min() > 0 for _, _, _, m, _ in rig.heard)
    # the mix of a tick is the same bits whether anybody listens or not -- and a context in which nobody listens records what the
    # parent recorded (sources, monitor, then the twin's record; test_no_listener_makes_the_parents_launches holds the same with
    # test_gpu_monitor's own rig)
    nobody = run_case(gpu_fx, C, device, BLOCKS, listening=False)
    assert not nobody.listen.any() and len(nobody.got_mixes) == len(rig.got_mixes)
    for a, b in zip(rig.got_mixes, nobody.got_mixes):
        assert mm.bits_same(a, b)


def test_no_listener_makes_the_parents_launches(gpu_fx):
    """test_gpu_monitor's rig, which expects sources, monitor and then the twin's record: enabled monitor, listens all SELF (set and
    unset again), every tick's record is what it was before there were listens"""
    rig = tg.ClipRig(gpu_fx, 70, N, "f32", False)
    rig.sends(list(range(70)), *tg.case_sends(70, 3))
    rig.an.set_listen([0, 69], ["left", "right"])
    rig.an.set_listen([0, 69], "self")
    for a in (rig.an, rig.twin):
        a.clear_pending_channels([0, 69])
    live = tg._live("f32", 70, 480 + 441)
    rig.tick(np.ascontiguousarray(live[:, :480 * 4]), 480)
    rig.tick(np.ascontiguousarray(live[:, 480 * 4:]), 441)
    assert [r["kind"] for r in rig.an.last_launches()[:2]] == ["sources", "monitor"] and "listen" not in [r["kind"] for r in rig.an.last_launches()]
    rig.close()


def test_a_rated_clip_is_heard_through_the_resampler(gpu_fx):
    C = 6
    rig = RatedRig(gpu_fx, C, True)
    rig.bank("f32", [tr._cut("f32", 0, 700), tr._cut("f32", 1, 1500)], [0.0, 44100.0])
    rig.load([1, 2], [("f32", 0), ("f32", 1)], [1, 1])
    rig.sources([1, 2], [cm.FILE] * 2)
    rig.transport([1, 2], cm.PLAY)
    rig.sends([0, 1, 2], True, left=[0.25, 0.5, -1.5], right=[0.0, 1.0, 2.0])
    rig.listens([3, 5], ["left", "right"])                      # 4 hears itself between them
    total = 480 + 441 + 63 + 1000
    live = tr._live(C, total) * np.float32(0.01) + mm.data(C, total, 3)
    at = 0
    for n in (480, 441, 63, 1000):
        rig.tick(np.ascontiguousarray(live[:, at:at + n]), n)
        at += n
        assert [r["kind"] for r in rig.an.last_launches()[:4]] == ["sources", "resample", "monitor", "listen"]
    # the rated track really played, and its resampled row is in what track 5 heard (right gain 2: the largest term there)
    _, block, x, want, _ = rig.heard[0]
    assert np.abs(x[2]).max() > 0 and mm.bits_same(block[5], want[1]) and mm.bits_same(block[3], want[0]) and mm.bits_same(block[4], x[4])
    without = mm.mix(np.where(np.arange(C)[:, None] == 2, np.float32(0), x), rig.on, rig.left, rig.right)
    assert not mm.bits_same(without, want)
    rig.close()


def test_non_finite_samples_are_heard_only_through_a_send_that_is_on(gpu_fx):
    C, n = 70, 512                                              # a hop a tick: every tick returns a frame
    rig = ClipRig(gpu_fx, C, False)
    on, left, right = tg.case_sends(C, 5)
    on[[5, 6, 7, 8, 66]] = [0, 1, 1, 1, 1]
    rig.sends(list(range(C)), on, left, right)
    listeners = [9, 11, 69]
    rig.listens(listeners, ["left", "right", "left"])
    x = mm.data(C, 3 * n, 77)
    bad = x.copy()
    bad[5, [3, 100, 479]] = [np.inf, np.nan, -np.inf]
    rig.tick(cm.raw(bad[:, :n]), n)                             # the track that carries them is off: neither the mix nor the listeners
    assert np.isfinite(rig.heard[-1][3]).all() and np.isfinite(rig.an.get_monitor()).all()
    # (a first frame's features may hold an inf of their own, so the mark of a sample that is not finite is the NaN)
    assert not np.isnan(rig.last[0][listeners]).any() and np.isnan(rig.last[0][5]).any()
    rig.sends([5], True)
    bad[5, [n + 3, n + 100, n + 479]] = [np.inf, np.nan, -np.inf]
    rig.tick(cm.raw(bad[:, n:2 * n]), n)                        # on: the listeners' features are the twin's, which was fed the NaNs
    _, block, _, want, _ = rig.heard[-1]
    assert np.isnan(want[:, 100]).all() and np.isinf(want[:, 3]).all() and np.isnan(block[9, 100]) and np.isnan(block[11, 100])
    for t in listeners:
        assert np.isnan(rig.last[0][t]).any(), t
    assert not np.isnan(rig.last[0][10]).any()                  # the neighbour that hears itself
    rig.an.close(); rig.twin.close()                            # (the analysers' features are NaN from here on, on both sides alike)


def test_the_listeners_gain_is_applied_to_what_it_hears(gpu_fx):
    C = 8
    rig = ClipRig(gpu_fx, C, True)
    rig.sends(list(range(C)), *tg.case_sends(C, 11))
    rig.listens([2, 5], ["right", "left"])
    gains = np.linspace(0.5, 1.2, C).astype(np.float32)
    gains[2], gains[5] = 0.3, -1.75
    rig.both(lambda a: a.set_channel_gains(gains))
    live = tg._live("f32", C, 600 + 441 + 1000)
    at = 0
    for n in (600, 441, 1000):
        rig.tick(np.ascontiguousarray(live[:, at * 4:(at + n) * 4]), n)        # (the mix is the model's, which knows no gain)
        at += n
    heard = rig.last[0].copy()
    # and the gain matters: the same stream with the listeners' gains at 1 gives them other features
    other = ClipRig(gpu_fx, C, True)
    other.sends(list(range(C)), *tg.case_sends(C, 11))
    other.listens([2, 5], ["right", "left"])
    gains[2], gains[5] = 1.0, 1.0
    other.both(lambda a: a.set_channel_gains(gains))
    at = 0
    for n in (600, 441, 1000):
        other.tick(np.ascontiguousarray(live[:, at * 4:(at + n) * 4]), n)
        at += n
    for a, b in zip(rig.got_mixes, other.got_mixes):
        assert mm.bits_same(a, b)
    assert not tc.same(heard[2], other.last[0][2]) and not tc.same(heard[5], other.last[0][5]) and tc.same(heard[3], other.last[0][3])
    rig.close(); other.close()


def test_lifecycle_and_refusals(gpu_fx):
    C, n = 8, 512
    rig = ClipRig(gpu_fx, C, False)
    an, Err = rig.an, gpu_fx.FxError
    live = tg._live("f32", C, 12 * n)
    piece = lambda k, m=n: np.ascontiguousarray(live[:, k * n * 4:(k * n + m) * 4])      # noqa: E731
    rig.check_listens()                                         # SELF when the monitor is made
    rig.sends(list(range(C)), True, *mm.gains(C, 2))
    rig.listens([3, 6], ["left", "right"])
    rig.both(lambda a: a.enable_onset_events(4096))
    rig.both(lambda a: a.enable_display(64, 256))
    rig.tick(piece(0), n)
    # a tick that is not fp32 is refused before any launch, names the first listener and changes nothing
    before, held = an.transport_state(), an.get_monitor()
    assert an.pending_samples() == 0
    with pytest.raises(Err, match="track 3 listens"):
        an.push_sources(np.zeros((C, 64), np.int16))
    with pytest.raises(Err, match="track 3 listens"):
        an.push_sources(np.zeros((C, 64), np.float16))
    assert an.last_launches() == [] and an.pending_samples() == 0
    after = an.transport_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert an.get_monitor().shape == (2, n) and mm.bits_same(an.get_monitor(), held)
    an.push_sources(np.zeros((C, 0), np.float32))              # a tick of no samples does nothing
    assert an.last_launches() == [] and mm.bits_same(an.get_monitor(), held)
    # the monitor is not freed under a listener; nothing changes
    with pytest.raises(Err, match="track 3 listens"):
        an.enable_monitor(False)
    rig.check_listens(); rig.check_sends()
    assert mm.bits_same(an.get_monitor(), held)
    # the setter zeroes the pending samples, also where the value does not change; a duplicate: the last entry wins
    rig.tick(piece(1, 300), 300)
    assert an.pending_samples() == 300
    rig.listens([3], ["left"])                                  # unchanged, and cleared all the same (the twin clears track 3)
    rig.listens([6, 6, 0], ["self", "left", "right"])
    rig.check_listens()
    assert list(rig.listen[[0, 3, 6]]) == [lm.RIGHT, lm.LEFT, lm.LEFT]
    rig.both(lambda a: a.request_taps([0, 3, 4]))
    rig.tick(live[:, (n + 300) * 4:(2 * n + 88) * 4].copy(), n - 212)       # completes the hop: 300 pending, of which some tracks' are zeros
    assert rig.last[0].shape[1] == 1
    for ch in (0, 3, 4):
        g, w = rig.an.taps(ch), rig.twin.taps(ch)
        assert g["frame_index"] == w["frame_index"]
        for k in g:
            assert tc.same(g[k], w[k]), (ch, k)
    # a refused list changes nothing, and names the entry
    lib = an._lib
    assert lib.fx_set_channel_listen(an._h, (ctypes.c_int * 2)(1, 2), 2, (ctypes.c_int * 2)(0, 3)) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"entry 1" in lib.fx_last_error() and b"unknown listen 3" in lib.fx_last_error()
    assert lib.fx_set_channel_listen(an._h, (ctypes.c_int * 2)(1, 99), 2, (ctypes.c_int * 2)(1, 1)) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"entry 1" in lib.fx_last_error()
    rig.check_listens()
    # the listens belong to the slot: resets and a track's move leave them
    rig.both(lambda a: a.reset_channels([0, 3]))
    rig.both(lambda a: a.import_tracks([4], a.export_tracks([6])))
    rig.check_listens()
    rig.tick(piece(3), n)
    rig.both(lambda a: a.reset_state())
    rig.check_listens()
    rig.tick(piece(4), n)
    rig.tick(piece(5, 1000), 1000)
    # the plain calls do not consult the listens
    g, w = rig.both(lambda a: a.push_samples(cm.typed(piece(7), "f32")))
    assert tc.same(g[0], w[0]) and an.last_launches() == rig.twin.last_launches()
    rig.tick(piece(8), n)
    # display and onset events of the listening tracks are the twin's
    g, w = rig.both(lambda a: a.display())
    assert g.shape == w.shape and tc.same(g, w) and np.abs(g[3]).max() > 0
    (ge, gd), (we, wd) = rig.both(lambda a: a.onset_events())
    assert gd == wd and np.array_equal(ge, we)
    # nobody listens any more: the monitor may go, and the record is the one of before
    rig.listens([0, 3, 6], "self")
    an.enable_monitor(False)
    with pytest.raises(Err, match="not enabled"):
        an.set_listen([0], "left")
    with pytest.raises(Err, match="not enabled"):
        an.listens()
    got, want = an.push_sources(cm.typed(piece(9), "f32")), rig.twin.push_samples(cm.typed(piece(9), "f32"))
    assert tc.same(got[0], want[0]) and [r["kind"] for r in an.last_launches()][:1] == ["sources"] and an.last_launches()[1:] == rig.twin.last_launches()
    rig.close()


def test_rows_past_2_to_the_31_bytes(gpu_fx):
    """65 536 tracks x 8193 samples: the planar block is 2 147 745 792 bytes and track 65 535's row starts 2 147 713 020 bytes in, so
    a 32-bit offset anywhere in the kernel lands somewhere else.  Every track plays a clip of one bank (no live block); tracks 0,
    65 534 and 65 535 listen; they and 65 533, which hears itself, are compared with a 4-track twin."""
    import torch
    C, n = 65536, 8193
    assert (C - 1) * n * 4 == 2147713020 and (C - 1) * n * 4 > 1 << 31
    lengths = [100003, 7, 5000, 33331, 20000, 8193, 12345, 3]
    clips = [mm.data(1, L, 900 + k)[0] for k, L in enumerate(lengths)]
    an, twin = gpu_fx.BatchAnalyser(C, N), gpu_fx.BatchAnalyser(4, N)
    first = an.create_clips(np.concatenate(clips), lengths=lengths, sample_format="f32")
    tracks = np.arange(C)
    an.load_clips(tracks, first + tracks % len(lengths))
    an.set_sources(tracks, "file")
    an.transport(tracks, "play")
    an.enable_monitor()
    on = [0, 1, 77, 40000, 65533, 65535]
    left = dict(zip(on, np.float32([0.5, -1.0, 0.25, 1.5, -0.75, 1.0])))
    right = dict(zip(on, np.float32([1.0, 0.5, -2.0, 0.0, 0.3, -1.25])))
    an.set_monitor(on, True, [left[t] for t in on], [right[t] for t in on])
    compared = [0, 65533, 65534, 65535]
    an.set_listen([0, 65534, 65535], ["left", "right", "left"])
    row = lambda t: clips[t % len(lengths)][np.arange(n) % lengths[t % len(lengths)]]        # noqa: E731
    want = lm.sparse_mix({t: row(t) for t in on}, left, right, n)
    block = np.stack([want[0], row(65533), want[1], want[0]])
    got = an.push_sources(None, n, sample_format="f32", device=True)
    ref = twin.push_samples(block)
    kinds = [r["kind"] for r in an.last_launches()]
    assert kinds[:3] == ["sources", "monitor", "listen"]
    assert mm.bits_same(an.get_monitor(), want)
    idx = torch.tensor(compared, device=got[0].device)
    assert got[0].shape == (C, n // 512, 12)
    assert tc.same(got[0][idx].cpu().numpy(), ref[0]) and tc.same(got[1][idx].cpu().numpy(), ref[1])
    # and the listeners really heard something else than their own clips
    own = gpu_fx.BatchAnalyser(4, N)
    mine = own.push_samples(np.stack([row(t) for t in compared]))
    assert tc.same(mine[0][1], ref[0][1]) and not tc.same(mine[0][0], ref[0][0]) and not tc.same(mine[0][3], ref[0][3])
    own.close()
    assert np.array_equal(np.flatnonzero(an.listens()), [0, 65534, 65535])
    an.close(); twin.close()


def test_cpp_listen_mirror(gpu_fx, tmp_path):
    gpu_fx.load_library()
    exe = str(tmp_path / "listen_mirror")
    lib_dir = os.path.dirname(gpu_fx.library_path())
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "listen_mirror.cpp"), "-o", exe, "-L", lib_dir, "-lfx_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "listen_mirror: ok" in out.stdout
