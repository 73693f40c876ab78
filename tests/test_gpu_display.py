"""Audio display levels on the device (include/fx.h, fx_enable_display / fx_set_display_samples_per_block / fx_clear_display_channels /
fx_get_display).

Every case drives a context and, beside it, one display_model.Track per track with the gained float32 hops the test forms itself --
the input widened as the load stage widens it (f16 exactly, s16 x / 32768, s24 x / 2^23), times the gain in force when the hop is
analysed -- and compares the uint32 view of fx_get_display with the model's drawing order after every call.  No tolerance: a level
is one of the samples."""
import numpy as np
import pytest

import dispatch_paths as dp
import display_model as dm

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---- input in each sample format, and the floats the load stage makes of it ----
def _signal(C, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.6 * np.sin(2 * np.pi * t[None, :] * (0.003 + 0.002 * np.arange(C)[:, None])) + 0.25 * rng.standard_normal((C, n))
    return np.clip(x, -0.999, 0.999).astype(F32)


def _as_format(x, fmt, fx):
    """-> (what the entry point is given, the float32 samples the kernels make of it)"""
    if fmt == "f32":
        return x, x
    if fmt == "f16":
        h = x.astype(np.float16)
        return h, h.astype(F32)
    if fmt == "s16":
        v = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        return v, v.astype(F32) * F32(1.0 / 32768.0)
    v = np.clip(np.round(x.astype(np.float64) * 8388608.0), -8388608, 8388607).astype(np.int32)
    return fx.pack_s24(v), v.astype(F32) * F32(1.0 / 8388608.0)         # (24 significant bits: exact)


class Driver:
    """a context with the display enabled, and the model beside it"""

    def __init__(self, fx, C, N, spb, L, tracks=None, **kw):
        self.fx, self.C, self.N, self.H, self.L = fx, C, N, N // 2, L
        self.an = fx.BatchAnalyser(C, N, **kw)
        self.an.enable_display(spb, L)
        self.model = [dm.Track(spb, L) for _ in range(C)]
        self.gain = np.ones(C, F32)
        self.pending = np.zeros((C, 0), F32)
        self.tracks = list(range(C)) if tracks is None else tracks      # the tracks the model follows (all are compared where it does)

    def close(self):
        self.an.close()

    def _show(self, hops, gained=True):
        """hops [C][T][H] float32 as analysed"""
        for c in self.tracks:
            x = hops[c].ravel()
            if gained and self.gain[c] != 1.0:
                x = x * self.gain[c]
            self.model[c].push(x)

    def push_hops(self, x, fmt="f32", device=False):
        given, floats = _as_format(x, fmt, self.fx)
        self._call(self.an.push_hops, given, device, fmt)
        self._show(floats.reshape(self.C, -1, self.H))

    def process_frames(self, frames):
        self._call(self.an.process_frames, frames, False)
        self._show(frames[:, :, self.H:], gained=False)

    def _take(self, floats):
        have = np.concatenate([self.pending, floats], axis=1)
        hops = have.shape[1] // self.H
        if hops:
            self._show(have[:, :hops * self.H].reshape(self.C, hops, self.H))
        self.pending = have[:, hops * self.H:]
        return hops

    def push_samples(self, x, fmt="f32", device=False):
        given, floats = _as_format(x, fmt, self.fx)
        out = self._call(self.an.push_samples, given, device, fmt)
        assert out[1].shape[1] == self._take(floats)

    def push_interleaved(self, block, channel_map, fmt="f32"):
        """block [n][K] float32"""
        given, floats = _as_format(block, fmt, self.fx)
        out = self.an.push_interleaved(given)
        assert out[1].shape[1] == self._take(np.ascontiguousarray(floats.T[channel_map]))

    def _call(self, fn, given, device, fmt="f32"):
        given = np.ascontiguousarray(given)
        if device:
            import torch
            given = torch.from_numpy(given).cuda()
        return fn(given, **({"sample_format": "s24"} if fmt == "s24" else {}))      # (uint8 is packed 24-bit PCM only when the caller says so)

    def set_gains(self, gains):
        self.gain = np.asarray(gains, F32)
        self.an.set_channel_gains(self.gain)

    def set_gain(self, g):
        self.gain = np.full(self.C, g, F32)
        self.an.set_gain(float(g))

    def set_spb(self, n):
        self.an.set_display_samples_per_block(n)
        for t in self.model:
            t.set_samples_per_block(n)

    def reset_channels(self, channels):
        self.an.reset_channels(channels)
        for c in channels:
            self.model[c] = dm.Track(self.model[c].spb, self.L)
            # (the track's pending samples become zeros; the pending COUNT is the context's and stays)
            self.pending[c] = 0

    def clear(self, channels):
        self.an.clear_display(channels)
        for c in channels:
            self.model[c].clear()

    def reset_state(self):
        self.an.reset_state()
        self.model = [dm.Track(t.spb, self.L) for t in self.model]
        self.pending = np.zeros((self.C, 0), F32)

    def check(self, what="", device=False):
        got = self.an.display(device=device)
        if device:
            got = got.cpu().numpy()
        assert got.shape == (self.C, self.L, 2) and got.dtype == F32
        for c in self.tracks:
            want = self.model[c].draw_order()
            same = dm.bits(got[c]) == dm.bits(want)
            assert same.all(), "%s: track %d, first difference at level %d: got %s, model %s" % (
                what, c, int(np.flatnonzero(~same.all(axis=1))[0]), got[c][~same.all(axis=1)][:3], want[~same.all(axis=1)][:3])
        # a listed get returns the same rows
        some = [self.tracks[-1], self.tracks[0], self.tracks[-1]]
        listed = self.an.display(some)
        assert np.array_equal(dm.bits(listed), dm.bits(got[some])), what


def _spbs(N):
    return sorted({1, 7, N // 2, 256, 300, N // 2 + 1, 5000})


HOP_CASES = [(N, spb, L) for N in (256, 1024) for spb in _spbs(N) for L in (4, 1024)]


@pytest.mark.parametrize("N,spb,L", HOP_CASES, ids=["%d-spb%d-L%d" % c for c in HOP_CASES])
def test_push_hops_calls_of_1_2_5(gpu_fx, N, spb, L):
    """T = 1, 2, 5 on one stream: `sub` carries from call to call; spb 1 / 7 publish more than L = 4 entries in a single call,
    spb 5000 exceeds a whole call, 300 and N/2 + 1 straddle hop boundaries"""
    C, H = 3, N // 2
    x = _signal(C, 8 * H, seed=N + spb).reshape(C, 8, H)
    d = Driver(gpu_fx, C, N, spb, L)
    d.check("new")                                      # all zero
    at = 0
    for T in (1, 2, 5):
        d.push_hops(np.ascontiguousarray(x[:, at:at + T]))
        at += T
        assert [l["kind"] for l in d.an.last_launches()].count("display") == 1
        d.check("after T = %d" % T)
    if spb <= 7 and L == 4:
        assert 5 * H // spb > L                         # a single call did publish more than L entries
    d.close()


def test_a_call_that_publishes_exactly_L_entries(gpu_fx):
    d = Driver(gpu_fx, 3, 256, 32, 4)                   # 128 samples from a new component: publications at 0, 32, 64, 96
    d.push_hops(_signal(3, 128, seed=1).reshape(3, 1, 128))
    assert all(t.next == 4 for t in d.model)
    d.check("exactly L")
    d.push_hops(_signal(3, 128, seed=2).reshape(3, 1, 128))
    d.check("and L more")
    d.close()


@pytest.mark.parametrize("N,kw", [(2048, {"low_latency": True}), (1024, {"analysers": "spectral"})], ids=["2048-low-latency", "1024-spectral-only"])
def test_the_display_does_not_depend_on_the_analysers(gpu_fx, N, kw):
    C, H = 3, N // 2
    x = _signal(C, 8 * H, seed=N).reshape(C, 8, H)
    d = Driver(gpu_fx, C, N, 300, 1024, **kw)
    at = 0
    for T in (1, 2, 5):
        d.push_hops(np.ascontiguousarray(x[:, at:at + T]))
        at += T
        d.check("after T = %d" % T)
    d.close()


def test_65_channels_once(gpu_fx):
    C, N = 65, 256
    x = _signal(C, 5 * 128, seed=65).reshape(C, 5, 128)
    d = Driver(gpu_fx, C, N, 7, 4)
    d.set_gains(np.linspace(0.5, 2.0, C))
    d.push_hops(x[:, :2].copy())
    d.reset_channels([64, 3])                           # phases differ per track from here on
    d.push_hops(x[:, 2:].copy())
    d.check("65 channels")
    d.close()


BLOCK_CASES = [(1024, f) for f in ("f32", "f16", "s16", "s24")] + [(256, f) for f in ("f32", "f16", "s16", "s24")] + [(2048, "f32")]


@pytest.mark.parametrize("N,fmt", BLOCK_CASES, ids=["%d-%s" % c for c in BLOCK_CASES])
def test_push_samples_blocks(gpu_fx, N, fmt):
    """blocks of 100, 480, 777 and 3 N/2 + 5: the block-fed kernels (1024 points and up), two-hop calls and the re-blocked path;
    a call that completes no hop changes nothing"""
    C, H = 3, N // 2
    blocks = [100, 480, 777, 3 * H + 5, 100, 480, 777, 3 * H + 5]
    x = _signal(C, sum(blocks), seed=N + len(fmt))
    d = Driver(gpu_fx, C, N, 300, 4 if fmt == "s16" else 1024)
    at = 0
    for i, n in enumerate(blocks):
        before = d.an.display()
        d.push_samples(np.ascontiguousarray(x[:, at:at + n]), fmt, device=(i % 2 == 1))
        at += n
        d.check("block %d of %d samples" % (i, n))
        if at < H:                                      # no hop yet: nothing published, nothing launched
            assert np.array_equal(dm.bits(before), dm.bits(d.an.display()))
            assert all(l["kind"] != "display" for l in d.an.last_launches())
    d.close()


def test_a_call_that_completes_no_hop_changes_nothing(gpu_fx):
    C, N = 3, 1024
    x = _signal(C, 2000, seed=3)
    d = Driver(gpu_fx, C, N, 7, 1024)
    d.push_samples(x[:, :600].copy())                   # one hop, 88 pending
    before = d.an.display()
    assert before.any()
    d.push_samples(x[:, 600:700].copy())                # 188 pending: no hop
    assert all(l["kind"] != "display" for l in d.an.last_launches())
    assert np.array_equal(dm.bits(before), dm.bits(d.an.display()))
    d.push_samples(x[:, 700:1100].copy())
    d.check("after the hop completed")
    d.close()


def test_push_interleaved_with_a_permuted_map(gpu_fx):
    C, N, K = 3, 1024, 5
    cmap = [4, 0, 2]
    x = _signal(K, 3 * 480, seed=11)
    d = Driver(gpu_fx, C, N, 256, 1024)
    d.an.set_channel_map(cmap)
    for i in range(3):
        d.push_interleaved(np.ascontiguousarray(x[:, i * 480:(i + 1) * 480].T), cmap)
        d.check("interleaved block %d" % i)
    d.close()


def test_process_frames_shows_second_halves_without_gain(gpu_fx):
    C, N = 3, 256
    frames = _signal(C, 6 * N, seed=12).reshape(C, 6, N)
    d = Driver(gpu_fx, C, N, 7, 1024)
    d.set_gain(3.0)                                     # hops would be scaled; frames are shown as given
    d.process_frames(np.ascontiguousarray(frames[:, :1]))
    d.check("one frame")
    d.process_frames(np.ascontiguousarray(frames[:, 1:]))
    d.check("five frames")
    d.close()


def test_per_track_gains_and_a_gain_change_while_samples_are_pending(gpu_fx):
    C, N = 3, 1024
    x = _signal(C, 3000, seed=13)
    d = Driver(gpu_fx, C, N, 256, 1024)
    d.set_gains([0.5, 2.0, -1.5])
    d.push_samples(x[:, :812].copy())                   # one hop at the first gains, 300 pending
    d.check("first gains")
    d.set_gains([1.0, 0.25, 3.0])                       # the pending samples are shown with the gain in force when their hop completes
    d.push_samples(x[:, 812:1300].copy())
    d.check("changed while pending")
    d.set_gain(0.75)                                    # the context-wide setter writes every row
    d.push_samples(x[:, 1300:3000].copy())
    d.check("context-wide gain")
    d.close()


def test_phase_changes(gpu_fx):
    C, N, H = 3, 256, 128
    x = _signal(C, 40 * H, seed=14).reshape(C, 40, H)
    d = Driver(gpu_fx, C, N, 300, 4)
    d.push_hops(x[:, 0:3].copy())
    d.set_spb(64)                                       # in mid-block: the running block keeps its count
    d.push_hops(x[:, 3:5].copy())
    d.check("samples per block 300 -> 64")
    d.set_spb(1000)
    d.push_hops(x[:, 5:6].copy())
    d.check("64 -> 1000")
    d.reset_channels([1])
    d.check("track 1 reset")
    d.push_hops(x[:, 6:15].copy())                      # track 1 runs at another phase now
    d.check("after the reset")
    assert len({(t.sub, t.next) for t in d.model}) > 1
    d.clear([0, 2])
    d.check("tracks 0 and 2 cleared")
    d.push_hops(x[:, 15:22].copy())
    d.check("after the clear")
    assert d.model[0].next != 0 or d.model[0].levels.any()
    d.reset_state()
    d.check("reset_state")
    d.push_hops(x[:, 22:30].copy())
    d.check("after reset_state")
    d.close()


def test_special_samples(gpu_fx):
    C, N, H, spb = 3, 256, 128, 64
    x = _signal(C, 6 * H, seed=15).reshape(C, -1)
    x[0, 20] = np.nan                                   # NaN in mid-block
    x[0, 63] = np.nan                                   # NaN as a block's last sample (the new component's first block ends at 63)
    x[0, 127] = np.nan                                  # and as the last sample of a call
    x[1, 70] = np.inf
    x[1, 90] = -np.inf
    x[1, 200] = np.nan
    x[1, 201] = np.inf
    x[2, 128:192] = np.where(np.arange(64) % 3 == 0, -0.0, 0.0)         # a block of mixed zeros ...
    x[2, 192:256] = np.where(np.arange(64) % 2 == 0, 0.0, -0.0)         # ... ending on either sign
    x[2, 300:364] = -0.0
    for L in (4, 1024):
        d = Driver(gpu_fx, C, N, spb, L)
        hops = x.reshape(C, 6, H)
        d.push_hops(hops[:, :1].copy())
        d.check("first hop, L = %d" % L)
        d.push_hops(hops[:, 1:3].copy())
        d.check("two hops, L = %d" % L)
        d.push_hops(hops[:, 3:].copy())
        d.check("three hops, L = %d" % L)
        d.close()
    # the model did see what the case is about
    t = dm.Track(spb, 1024)
    t.push(x[0])
    assert np.isnan(t.levels[:t.next]).any(axis=1).sum() >= 2
    t = dm.Track(spb, 1024)
    t.push(x[2])
    assert (dm.bits(t.levels[:t.next]) == 0x80000000).any()


def test_host_and_device_destinations(gpu_fx):
    C, N = 3, 1024
    x = _signal(C, 5 * 512, seed=16).reshape(C, 5, 512)
    d = Driver(gpu_fx, C, N, 7, 1024)
    d.push_hops(x, device=True)
    d.check("host", device=False)
    d.check("device", device=True)
    import torch
    some = d.an.display([2, 0], device=True)
    assert some.is_cuda and tuple(some.shape) == (2, 1024, 2)
    assert np.array_equal(dm.bits(some.cpu().numpy()), dm.bits(d.an.display()[[2, 0]]))
    torch.cuda.synchronize()
    d.close()


def test_results_are_the_disabled_twins_bits(gpu_fx):
    C, N = 5, 1024
    x = _signal(C, 7000, seed=17)
    outs = {}
    for enabled in (False, True):
        an = gpu_fx.BatchAnalyser(C, N)
        if enabled:
            an.enable_display(300, 1024)
        got = [an.push_hops(np.ascontiguousarray(x[:, :2560].reshape(C, 5, 512)))]
        got += [an.push_samples(np.ascontiguousarray(x[:, a:b])) for a, b in ((2560, 3040), (3040, 4040), (4040, 7000))]
        got.append((an.get_features(),))
        outs[enabled] = got
        an.close()
    for a, b in zip(outs[False], outs[True]):
        for p, q in zip(a, b):
            assert p.shape == q.shape and np.array_equal(p.view(np.uint32), q.view(np.uint32))


# ---- nothing moves when it is off; exactly one more launch when it is on ----
LAUNCH_ROWS = [r for r in dp.ROWS if r.id in {"batch-1024", "hop-1024", "frame-tail-2048", "two-hop-4096", "fused-tail-256", "frames-1024",
                                                "block-batch-1024-f32", "reblock-1-1024-f32", "block-hop-1024-f32", "block-two-hop-2048-s16",
                                                "pair-2048", "harmonic-1024", "reblock-three-hops-2048-s16"}]


@pytest.mark.parametrize("r", LAUNCH_ROWS, ids=[r.id for r in LAUNCH_ROWS])
def test_launches_with_the_display_off_and_on(gpu_fx, r):
    import torch
    import test_gpu_dispatch as tgd
    if torch.cuda.get_device_properties(0).multi_processor_count != dp.CUS:
        pytest.skip("the table's launch sequences are written for %d CUs" % dp.CUS)
    hops, pieces = tgd._plan(r)
    an = tgd._analyser(gpu_fx, r)
    outs, records, _ = tgd._run_calls(gpu_fx, an, r, pieces)
    an.close()
    tgd._check_launches(r, records, [o[0].shape[1] for o in outs])            # never enabled: what it is at the parent commit
    an = tgd._analyser(gpu_fx, r)
    an.enable_display(300, 64)
    outs_on, records, _ = tgd._run_calls(gpu_fx, an, r, pieces)
    levels = an.display()
    an.close()
    frames = [o[0].shape[1] for o in outs_on]
    stripped = []
    for rec, t in zip(records, frames):
        if t == 0:
            assert all(l["kind"] != "display" for l in rec), (r.id, rec)
            stripped.append(rec)
            continue
        assert [l["kind"] for l in rec].count("display") == 1 and rec[-1]["kind"] == "display", (r.id, rec)
        last = rec[-1]
        assert last["T"] == t and last["window"] == r.N, (r.id, last)
        assert all(v == 0 for k, v in last.items() if k not in ("kind", "T", "window")), (r.id, last)
        stripped.append(rec[:-1])
    tgd._check_launches(r, stripped, frames)
    for a, b in zip(outs, outs_on):
        for p, q in zip(a, b):
            assert np.array_equal(p.view(np.uint32), q.view(np.uint32)), r.id
    # and the levels are the model's, on two tracks: the analysed hops as floats (frames rows show them without gain: gain is 1 here)
    total = sum(frames)
    floats = tgd._floats(hops[:, :total], r.fmt)
    for c in (0, r.C - 1):
        t = dm.Track(300, 64)
        t.push(np.asarray(floats[c], F32))
        assert np.array_equal(dm.bits(levels[c]), dm.bits(t.draw_order())), (r.id, c)
