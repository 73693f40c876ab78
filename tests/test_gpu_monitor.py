"""The monitor mix on the GPU (include/fx.h, fx_enable_monitor .. fx_get_monitor).  The rig is that of tests/test_gpu_clips.py: context A
runs push_sources with the monitor enabled, its plain twin B is given push_samples(the model's planar block); clip_model.Model (or
resample_model.Model) forms that block, resample_model.widen and monitor_model.mix the expected output.  After every tick
get_monitor() is the model's mix bit for bit in host and in device memory (NaNs equal), raw, smoothed, frame counts and
pending_samples() are the twin's, and the launch record is sources, resample if any, monitor (T = n), then the twin's record.

A context runs ticks of every block length one after another, so every (tracks, format, block length) triple is met in 16 pairs of
contexts.  Tracks: 6, 64, 70, 130 -- below a group, exactly one, a partial second, a partial third; block lengths 1, 63, 441, 480,
512, 1000 (and 4097 once): rows at odd byte offsets, a ragged last piece, rows shorter than one 16-byte piece.  run_case() also runs
without a GPU (fx None): tests/test_monitor_cpu.py uses that to show that THIS data tells the specified order from a flat sum."""
import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import clip_model as cm
import interleave_model as im
import monitor_model as mm
import resample_model as rm
import test_gpu_clips as tc
import test_gpu_resample as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRACKS = [6, 64, 70, 130]
BLOCKS = [480, 1, 63, 441, 512, 1000]
NS = [256, 1024, 2048, 4096]
# every (tracks, format) pair once; window size and memory kind walk their own cycles, so each value of each axis meets each format
CASES = [(C, fmt, NS[(i + i // 4) % 4], bool((i + i // 4) % 2)) for i, (C, fmt) in enumerate(itertools.product(TRACKS, cm.FORMATS))]


class _Dry:
    """stands in for a context where there is no GPU: every call does nothing and returns 0"""
    def __getattr__(self, name):
        return lambda *a, **k: 0


class _DryFx:
    @staticmethod
    def BatchAnalyser(*a, **k):
        return _Dry()


@functools.lru_cache(maxsize=None)
def _tape(fmt):
    """one long stretch of four-decade data in `fmt`, as bytes: clips and live rows are cut from it"""
    return cm.raw(im.encode(mm.data(1, 300000, 31), fmt))[0]


def _cut(fmt, k, L):
    B = cm.BYTES[fmt]
    at = (k * 7919) % (_tape(fmt).size // B - L)
    return _tape(fmt)[at * B:(at + L) * B].copy()


def _live(fmt, C, total):
    B = cm.BYTES[fmt]
    room = _tape(fmt).size // B - total
    return np.stack([_tape(fmt)[((c * 4099) % room) * B:((c * 4099) % room + total) * B] for c in range(C)])


class Monitored:
    """what a rig of test_gpu_clips / test_gpu_resample needs to hold the monitor to the model: the sends, and a tick that knows the
    monitor's launch record and checks the mix"""

    def start_monitor(self, fmt):
        self.fmt, self.dry = fmt, isinstance(self.an, _Dry)
        self.an.enable_monitor()
        self.monitor = True
        self.default_sends()
        self.mixes = []                     # (n, the model's mix, the widened block, the sends in force) of every tick

    def default_sends(self):
        self.on, self.left, self.right = np.zeros(self.C, np.int32), np.ones(self.C, np.float32), np.ones(self.C, np.float32)

    def sends(self, channels, on=True, left=None, right=None):
        self.an.set_monitor(channels, on, left, right)
        for i, c in enumerate(channels):            # in list order: the last entry of a track wins
            self.on[c] = int(bool(on[i] if isinstance(on, (list, tuple, np.ndarray)) else on))
            for mine, given in ((self.left, left), (self.right, right)):
                if given is not None:
                    mine[c] = np.float32(given[i] if isinstance(given, (list, tuple, np.ndarray)) else given)

    def check_sends(self):
        if not self.dry:
            got = self.an.monitor_sends()
            assert np.array_equal(got["on"], self.on) and mm.bits_same(got["left"], self.left) and mm.bits_same(got["right"], self.right)

    def expected(self, planar):
        x = planar if planar.dtype == np.float32 else np.stack([rm.widen(row, self.fmt) for row in planar])
        return mm.mix(x, self.on, self.left, self.right), x

    def check_monitor(self, want):
        if self.dry:
            return
        host, dev = self.an.get_monitor(), self.an.get_monitor(device=True)
        assert host.dtype == np.float32 and host.shape == want.shape, (host.shape, want.shape)
        assert mm.bits_same(host, want), np.flatnonzero(host.view(np.uint32) != want.view(np.uint32))[:8]
        assert mm.bits_same(dev.cpu().numpy(), want)

    def tick(self, live, n, table=True):
        """one tick: `live` [C] rows as the rig's model takes them, or None"""
        resampled = any(p.source == cm.FILE and getattr(p, "rated", False) for p in self.m.players)
        planar = self.m.tick(live, n)
        want, x = self.expected(planar)
        self.mixes.append((n, want, x, (self.on.copy(), self.left.copy(), self.right.copy())))
        if self.dry:
            return 0
        give = self._arr
        if live is None:
            got = self.an.push_sources(None, n, sample_format=self.fmt, device=self.device)
        else:
            got = self.an.push_sources(give(live), sample_format=self.fmt)
        twin = self.twin.push_samples(give(planar), sample_format=self.fmt)
        g, w = [tc._host(r) for r in got], [tc._host(r) for r in twin]
        assert g[0].shape == w[0].shape and tc.same(g[0], w[0]) and tc.same(g[1], w[1])
        assert self.an.pending_samples() == self.twin.pending_samples()
        rec, twin_rec = self.an.last_launches(), self.twin.last_launches()
        head = ["sources"] + (["resample"] if resampled else []) + (["monitor"] if self.monitor else [])
        assert [r["kind"] for r in rec[:len(head)]] == head and all(r["T"] == n for r in rec[:len(head)]), rec
        assert rec[len(head):] == twin_rec, (rec, twin_rec)
        if self.monitor:
            self.check_monitor(want)
        if table:
            self.check_table()
        return g[0].shape[1]


class ClipRig(Monitored, tc.Rig):
    def __init__(self, fx, C, N, fmt, device):
        tc.Rig.__init__(self, fx if fx is not None else _DryFx, C, N, fmt, device)
        self.start_monitor(fmt)


class RatedRig(Monitored, tr.Rig):
    def __init__(self, fx, C, N, device):
        tr.Rig.__init__(self, fx, C, N, device)
        self.start_monitor("f32")


def _kinds(C):
    """the tracks a context mixes, as (kind, clip length): the kinds of test_gpu_clips.py around a 480-sample tick"""
    if C < 12:
        return [("input", 0), ("loop", 5), ("loop", 481), ("oneshot", 721), ("paused", 50), ("nofile", 0)]
    return ([("input", 0)] + [("loop", L) for L in (1, 5, 7, 479, 480, 481, 100003)] +
            [("oneshot", 721), ("paused", 50), ("stopped", 50), ("nofile", 0)])


def case_sends(C, seed):
    """(on, left, right): about 80 % of the tracks on -- at 130 tracks the whole second group off --, gains in [-2, 2] and among them
    0, 1, -1 and one that makes subnormal products (1e-36 times samples of 1e-4 .. 1)"""
    rng = np.random.default_rng(seed)
    on = (rng.random(C) < 0.8).astype(np.int32)
    on[0] = 1
    if C == 130:
        on[64:128], on[128:] = 0, 1                 # (the two tracks of the third group both on: its partial sum is a sum)
    left, right = mm.gains(C, seed + 1)
    left[[1, 2, 3, 4]] = [0.0, 1.0, -1.0, 1e-36]
    right[[1, 2, 3, 5]] = [-1.0, 0.0, 1e-36, 1.0]
    on[[2, 3, 4, 5]] = 1
    return on, left, right


def run_case(fx, C, fmt, N, device, blocks):
    """one context over ticks of `blocks` samples -> the rig's (n, mix, widened block, sends) per tick; fx None: the models alone"""
    rig = ClipRig(fx, C, N, fmt, device)
    kinds = _kinds(C)
    # (turned by C: the last group's tracks are loops at 70 and at 130 tracks, so that its partial sum has several terms that sound)
    track_kind = [kinds[(t + C) % len(kinds)] for t in range(C)]
    with_clip = [t for t in range(C) if track_kind[t][1]]
    rig.bank([_cut(fmt, t, track_kind[t][1]) for t in with_clip])
    rig.load(with_clip, list(range(len(with_clip))), [0 if track_kind[t][0] == "oneshot" else 1 for t in with_clip])
    files = [t for t in range(C) if track_kind[t][0] != "input"]
    rig.sources(files, [cm.FILE] * len(files))
    rig.transport([t for t in with_clip if track_kind[t][0] != "stopped"], cm.PLAY)
    paused = [t for t in range(C) if track_kind[t][0] == "paused"]
    on, left, right = case_sends(C, 100 * C + len(blocks) + cm.FORMATS.index(fmt))
    rig.sends(list(range(C)), on, left, right)
    rig.check_sends()
    live = _live(fmt, C, sum(blocks))
    at = 0
    for k, n in enumerate(blocks):
        rig.tick(np.ascontiguousarray(live[:, at * rig.B:(at + n) * rig.B]), n, table=(k == len(blocks) - 1))
        at += n
        if k == 0:
            rig.transport(paused, cm.PAUSE)
        if k == 1:
            # sends changed between ticks are in force at the next one; of a track listed twice the last entry wins, right gains stay
            other = min(10, C - 1)
            rig.sends([0, 3, 3, other], on=[1, 0, 1, 1 - int(rig.on[other])], left=[0.5, 9.0, -1.5, 2.0])
    rig.check_sends()
    if not rig.dry:
        state = rig.m.table()["state"]
        for c in range(C):
            want = {"oneshot": cm.FINISHED, "paused": cm.PAUSED, "stopped": cm.STOPPED, "nofile": cm.NO_FILE, "loop": cm.PLAYING}.get(track_kind[c][0])
            assert want is None or state[c] == want, (c, track_kind[c])
    rig.close()
    return rig.mixes


@pytest.mark.parametrize("C,fmt,N,device", CASES)
def test_monitor_is_the_model_and_the_analysis_the_twins(gpu_fx, C, fmt, N, device):
    blocks = BLOCKS + [4097] if (C, fmt) == (70, "s24") else BLOCKS
    mixes = run_case(gpu_fx, C, fmt, N, device, blocks)
    assert [n for n, *_ in mixes] == blocks and all(np.abs(m).max() > 0 for _, m, *_ in mixes)


def _input_rig(gpu_fx, C, N=1024, device=False):
    """every track on its input, fp32"""
    return ClipRig(gpu_fx, C, N, "f32", device)


def test_non_finite_samples_reach_the_output_only_through_a_send_that_is_on(gpu_fx):
    C, n = 70, 480
    rig = _input_rig(gpu_fx, C)
    on, left, right = case_sends(C, 5)
    on[[5, 6, 7, 8, 66]] = [0, 1, 1, 1, 1]
    left[[6, 7, 8]], right[[6, 7, 8]] = [2.0, 1.0, 1.0], [0.5, 1.0, 1.0]
    rig.sends(list(range(C)), on, left, right)
    x = mm.data(C, 3 * n, 77)
    bad = x.copy()
    bad[5, [3, 100, 479]] = [np.inf, np.nan, -np.inf]
    rig.tick(cm.raw(bad[:, :n]), n)                             # the track that carries them is off
    assert np.isfinite(rig.mixes[-1][1]).all() and np.isfinite(rig.an.get_monitor()).all()
    rig.sends([5], True)
    bad[6, n + 10] = 3e38                                       # times 2: inf on the left, finite on the right
    bad[7, n + 20], bad[8, n + 20] = np.inf, -np.inf            # inf - inf
    bad[5, [n + 3, n + 100, n + 479]] = [np.inf, np.nan, -np.inf]
    rig.tick(cm.raw(bad[:, n:2 * n]), n)
    want = rig.mixes[-1][1]
    got = rig.an.get_monitor()
    assert np.isposinf(want[0, 10]) == np.isposinf(got[0, 10]) and np.isinf(got[0, 10]) and np.isfinite(got[1, 10])
    assert np.isnan(got[:, 20]).all() and np.isnan(got[:, 100]).all() and np.isinf(got[:, 3]).all() and np.isinf(got[:, 479]).all()
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    rig.sends([5, 6, 7, 8], False)
    rig.tick(cm.raw(bad[:, 2 * n:]), n)                         # the next tick is clean again: nothing is carried
    assert np.isfinite(rig.an.get_monitor()).all()
    rig.an.close(); rig.twin.close()                            # (the analysers' features are NaN from here on, on both sides alike)


def test_rated_clips_are_mixed_after_the_resampler(gpu_fx):
    C = 70
    rig = RatedRig(gpu_fx, C, 1024, True)
    rig.bank("f32", [tr._cut("f32", k, L) for k, L in enumerate([700, 1500])], [0.0, 96000.0])
    rig.bank("s16", [tr._cut("s16", 10, 900)], [44100.0])
    rig.bank("f16", [tr._cut("f16", 20, 333)], [22050.0])
    tracks = [1, 2, 3, 66]
    rig.load(tracks, [("f32", 0), ("f32", 1), ("s16", 0), ("f16", 0)], [1, 1, 1, 0])
    rig.sources(tracks, [cm.FILE] * 4)
    rig.transport(tracks, cm.PLAY)
    on, left, right = case_sends(C, 9)
    on[tracks] = 1
    rig.sends(list(range(C)), on, left, right)
    live = tr._live(C, 480 + 441 + 63) * np.float32(0.01) + mm.data(C, 480 + 441 + 63, 3)
    at = 0
    for n in (480, 441, 63):
        rig.tick(np.ascontiguousarray(live[:, at:at + n]), n)
        at += n
    assert [r["kind"] for r in rig.an.last_launches()[:3]] == ["sources", "resample", "monitor"]
    assert all(np.abs(x[tracks]).max(axis=1).min() > 0 for _, _, x, _ in rig.mixes[:1])     # every rated track really played
    rig.close()


def test_lifecycle(gpu_fx):
    C, n = 8, 480
    rig = _input_rig(gpu_fx, C)
    an, lib = rig.an, rig.an._lib
    rig.load([1, 2], [None, None])                              # (no bank: two FILE tracks without a file play silence)
    rig.sources([1, 2], [cm.FILE] * 2)
    live = cm.raw(mm.data(C, 8 * n, 11))
    piece = lambda k: np.ascontiguousarray(live[:, k * n * 4:(k + 1) * n * 4])     # noqa: E731
    # enabled, no send set: the defaults, no tick yet, and a tick's output is all +0
    rig.check_sends()
    assert an.get_monitor().shape == (2, 0) and an.get_monitor(device=True).shape == (2, 0)
    rig.tick(piece(0), n)
    assert not an.get_monitor().view(np.uint32).any()
    rig.sends(list(range(C)), True, *mm.gains(C, 2))
    rig.tick(piece(1), n)
    held = an.get_monitor()
    assert np.abs(held).max() > 0
    # what does not feed the monitor leaves the last mix alone
    rig.both(lambda a: a.push_sources(np.zeros((C, 0), np.float32)))
    assert an.last_launches() == []
    rig.both(lambda a: a.push_samples(cm.typed(piece(2), "f32")))
    rig.both(lambda a: a.push_interleaved(np.ascontiguousarray(cm.typed(piece(3), "f32").T)))
    assert mm.bits_same(an.get_monitor(), held)
    # the sends belong to the slot: resets and a track's move leave them
    rig.both(lambda a: a.reset_channels([0, 3]))
    rig.both(lambda a: a.reset_state())
    rig.both(lambda a: a.import_tracks([4], a.export_tracks([5])))
    rig.check_sends()
    assert mm.bits_same(an.get_monitor(), held)
    rig.tick(piece(4), n)
    # a refused tick (no live block while tracks listen to the input) changes neither the table nor the monitor
    held = an.get_monitor()
    with pytest.raises(gpu_fx.FxError, match="track 0"):
        an.push_sources(None, 1000, sample_format="f32")
    assert an.last_launches() == [] and mm.bits_same(an.get_monitor(), held)
    rig.check_sends(); rig.check_table()
    # too little room is refused with both numbers, and the count is reported all the same
    buf, got = (ctypes.c_float * (2 * n))(), ctypes.c_int(-1)
    assert lib.fx_get_monitor(an._h, buf, n - 1, ctypes.byref(got), gpu_fx.capi.MEM_HOST) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"479" in lib.fx_last_error() and b"480" in lib.fx_last_error() and got.value == n
    assert lib.fx_set_channel_monitor(an._h, (ctypes.c_int * 2)(0, 99), 2, None, None, None) == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"entry 1" in lib.fx_last_error()
    rig.check_sends()
    # enabling an enabled monitor keeps the sends and the mix
    an.enable_monitor()
    rig.check_sends()
    assert mm.bits_same(an.get_monitor(), held)
    # disabled: the record is the twin's with "sources" in front, and there is nothing to get
    an.enable_monitor(False)
    rig.monitor = False
    rig.tick(piece(5), n)
    for call in (an.get_monitor, an.monitor_sends, lambda: an.set_monitor([0])):
        with pytest.raises(gpu_fx.FxError, match="not enabled"):
            call()
    # enabled again: no tick yet, the sends back at their defaults
    an.enable_monitor()
    rig.monitor = True
    rig.default_sends()
    rig.check_sends()
    assert an.get_monitor().shape == (2, 0)
    rig.tick(piece(6), n)
    assert not an.get_monitor().view(np.uint32).any()
    rig.sends([7, 0], [1, 1], left=[-1.0, 0.25])
    rig.tick(piece(7), n)
    rig.close()


def test_cpp_monitor_mirror(gpu_fx, tmp_path):
    gpu_fx.load_library()
    exe = str(tmp_path / "monitor_mirror")
    lib_dir = os.path.dirname(gpu_fx.library_path())
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "monitor_mirror.cpp"), "-o", exe, "-L", lib_dir, "-lfx_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "monitor_mirror: ok" in out.stdout
