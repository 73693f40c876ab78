"""Listening tracks (include/fx.h, "LISTENING TRACKS") without a GPU: the C ABI declares and exports the entries and the bindings know
them, each refuses bad arguments before any device use, the launch record knows the copy, the host model (tests/listen_model.py)
equals its own word-by-word loop -- and the data the GPU test runs tells a track that hears the mix from one that hears itself, and
the left output from the right one."""
import ctypes
import os

import numpy as np
import pytest

import listen_model as lm
import monitor_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fx_set_channel_listen", "fx_get_channel_listen")


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in text
        assert name in fx.capi.EXPORTS
        assert hasattr(lib, name)
    assert "enum { FX_LISTEN_SELF = 0, FX_LISTEN_LEFT = 1, FX_LISTEN_RIGHT = 2 };" in text
    assert (fx.capi.LISTEN_SELF, fx.capi.LISTEN_LEFT, fx.capi.LISTEN_RIGHT) == (0, 1, 2) == (lm.SELF, lm.LEFT, lm.RIGHT)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    for method in ("set_listen", "listens"):
        assert callable(getattr(fx.BatchAnalyser, method))
    mirror = open(os.path.join(ROOT, "include", "fx_realtime.hpp")).read()
    for name in ENTRIES + ("void setListen", "void toggleCollectInput"):
        assert name + " (" in mirror, name
    assert "std::vector<int> getListens() const" in mirror
    # the two sentences that said this was left out point here now
    assert "not carried over" not in text and "tracks hearing each\n * other's players. */" not in text


def test_launch_kind_and_build_lists(fx):
    assert fx.capi.LAUNCH_KINDS[18] == "listen" and fx.capi.LAUNCH_KINDS[17] == "monitor" and fx.capi.LAUNCH_RECORD_CAP == 8
    csrc = os.path.join(ROOT, "feature-extractor_amd", "csrc")
    text = open(os.path.join(csrc, "fx_kernels.h")).read()
    assert "FX_LAUNCH_LISTEN = 18" in text and "FX_LAUNCH_RECORD_CAP = 8" in text
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_monitor.hip" in build.SOURCES and "fx_monitor.hip" not in build.HOST_SOURCES
    # the shim's host units refer to the unit through the context's hooks only
    for source in build.HOST_SOURCES:
        body = open(os.path.join(csrc, source)).read()
        for name in ENTRIES + ("fx_monitor_listen_kernel",):
            assert name not in body, (source, name)
    unit = open(os.path.join(csrc, "fx_monitor.hip")).read()
    assert "fx_monitor_listen_kernel" in unit and unit.index("launch_monitor_kernels(p, m->d_part") < unit.index("launch_listen_kernel(lp")
    clips = open(os.path.join(csrc, "fx_clips.hip")).read()
    assert not any(name in clips for name in ENTRIES)
    assert "monitor_prepare(c, num_samples, sample_format)" in clips


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID = fx.capi.FX_ERR_INVALID_ARGUMENT
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                      # noqa: E731
    # A zeroed block stands in for a context (no tracks, no monitor): each refusal below comes before the entry touches a device.
    fake = ctypes.create_string_buffer(1 << 16)

    def refused(status, *why):
        assert status == INVALID, (status, why, lib.fx_last_error())
        for w in why:
            assert w in lib.fx_last_error(), (why, lib.fx_last_error())

    refused(lib.fx_set_channel_listen(None, ints(0), 1, ints(1)), b"null context")
    refused(lib.fx_get_channel_listen(None, ints(0)), b"null context")
    refused(lib.fx_set_channel_listen(fake, ints(0), -1, ints(1)), b"negative channel count -1")
    refused(lib.fx_set_channel_listen(fake, None, 2, ints(1, 1)), b"null channel list")
    refused(lib.fx_set_channel_listen(fake, ints(0, 0), 2, None), b"null listen list")
    # a value outside {0, 1, 2}, at a named entry (the call's own values come before the range of its entries)
    refused(lib.fx_set_channel_listen(fake, ints(0, 0, 0), 3, ints(0, 2, 3)), b"entry 2", b"unknown listen 3")
    refused(lib.fx_set_channel_listen(fake, ints(0, 0), 2, ints(-1, 7)), b"entry 0", b"unknown listen -1")
    # a track out of range (the stand-in has no tracks: track 0 is out of range already), and the entry is named
    refused(lib.fx_set_channel_listen(fake, ints(0, 0), 2, ints(1, 2)), b"entry 0", b"out of range")
    refused(lib.fx_set_channel_listen(fake, ints(-3), 1, ints(0)), b"entry 0", b"channel -3")
    # no monitor
    refused(lib.fx_set_channel_listen(fake, None, 0, None), b"monitor is not enabled", b"fx_enable_monitor")
    refused(lib.fx_get_channel_listen(fake, ints(0)), b"monitor is not enabled", b"fx_enable_monitor")
    refused(lib.fx_get_channel_listen(fake, None), b"null output")
    # freeing a monitor that does not exist is still nothing to do
    assert lib.fx_enable_monitor(fake, 0) == fx.capi.FX_OK


class _NoLibrary:
    """stands in for the library: any use of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the binding used the library (%s) before refusing its arguments" % name)


def test_binding_refuses_before_any_library_use(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)          # no context: the refusals come first
    an.num_channels, an.window_size, an.device, an._lib, an._h = 4, 1024, 0, _NoLibrary(), None
    with pytest.raises(ValueError, match="out of range"):
        an.set_listen([4], "left")
    with pytest.raises(ValueError, match="out of range"):
        an.set_listen([0, -1], [1, 1])
    with pytest.raises(ValueError, match="holds integers"):
        an.set_listen([0.5], 1)
    with pytest.raises(ValueError, match="one value per listed track"):
        an.set_listen([0, 1, 2], [1, 0])
    with pytest.raises(ValueError, match="entry 1: unknown listen 3"):
        an.set_listen([0, 1], [2, 3])
    with pytest.raises(ValueError, match="entry 0: unknown listen -1"):
        an.set_listen([2], -1)
    with pytest.raises(ValueError, match="expected integers or one of left, right, self"):
        an.set_listen([2], "centre")
    with pytest.raises(ValueError, match="expected integers"):
        an.set_listen([2], 1.0)


@pytest.mark.parametrize("C", [1, 6, 70])
def test_model_equals_its_naive_loop(C):
    n = 37
    x = mm.data(C, n, C)
    x.view(np.uint32)[0, [1, 2]] = [0x80000000, 0x7fc12345]         # a -0 and a NaN with a payload: moved as words
    rng = np.random.default_rng(C)
    listen = rng.integers(0, 3, C)
    mix = mm.mix(x, np.ones(C, np.int32), *mm.gains(C, C + 1))
    mix.view(np.uint32)[1, 4] = 0xffc00001
    a, b = lm.heard(x, mix, listen), lm.heard_naive(x, mix, listen)
    assert a.dtype == np.float32 and a.shape == (C, n) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for c in range(C):
        want = x[c] if listen[c] == lm.SELF else mix[listen[c] - 1]
        assert np.array_equal(a[c].view(np.uint32), want.view(np.uint32))
    # nobody listens: the block, every byte
    assert np.array_equal(lm.heard(x, mix, np.zeros(C, np.int32)).view(np.uint32), x.view(np.uint32))


def test_sparse_mix_is_the_mix():
    C, n = 200, 53
    x = mm.data(C, n, 8)
    left, right = mm.gains(C, 9)
    on_tracks = [0, 1, 63, 64, 130, 199]
    on = np.zeros(C, np.int32)
    on[on_tracks] = 1
    got = lm.sparse_mix({t: x[t] for t in on_tracks}, dict(enumerate(left)), dict(enumerate(right)), n)
    assert mm.bits_same(got, mm.mix(x, on, left, right))


def test_minus_zero_is_heard_as_plus_zero_through_one_send():
    """the documented difference (fx.h): one send on at gains (1, 0), the track listening to the left output hears its own samples,
    except that -0 arrives as +0"""
    x = np.array([[1.5, -0.0, 0.0, -2.0]], np.float32)
    mix = mm.mix(x, [1], np.float32([1.0]), np.float32([0.0]))
    got = lm.heard(x, mix, [lm.LEFT])
    assert np.array_equal(got, x) and list(got.view(np.uint32)[0]) == [0x3fc00000, 0, 0, 0xc0000000]


@pytest.mark.parametrize("C", [6, 64, 70, 130])
def test_the_data_can_tell(oracle, C):
    """What tests/test_gpu_listen.py feeds its contexts of C tracks, run dry on the models, then through the oracle: over the whole
    stream every listening track's features differ from those of its own rows, no other track's differ, and with the two outputs
    exchanged every listening track's features differ again.  So a kernel that does nothing, one that writes a neighbour's row, or
    one that takes the left output for the right cannot pass the GPU test, which holds all tracks to the twin bit for bit.  (The
    stream is analysed here in one piece: the clears a command makes on both contexts alike are left out.)"""
    import test_gpu_listen as tl
    rig = tl.run_case(None, C, False, tl.BLOCKS)
    assert [n for n, *_ in rig.heard] == tl.BLOCKS + [tl.LAST]
    listening = np.flatnonzero(np.all([l != lm.SELF for *_, l in rig.heard], axis=0))
    selfs = np.flatnonzero(np.all([l == lm.SELF for *_, l in rig.heard], axis=0))
    assert 0 in listening and C - 1 in listening and listening.size + selfs.size == C and selfs.size >= C // 2 - 1
    for t in listening:                                     # a track that hears itself on each side, where there is a side
        assert all(u in selfs for u in (t - 1, t + 1) if 0 <= u < C), t
    swapped = {lm.SELF: lm.SELF, lm.LEFT: lm.RIGHT, lm.RIGHT: lm.LEFT}
    streams = {"heard": np.concatenate([b for _, b, *_ in rig.heard], axis=1), "own": np.concatenate([x for _, _, x, *_ in rig.heard], axis=1),
               "swapped": np.concatenate([lm.heard(x, m, [swapped[int(v)] for v in l]) for _, _, x, m, l in rig.heard], axis=1)}
    hops = streams["heard"].shape[1] // 512
    assert hops == 13
    raw = {k: oracle.push_hops(v[:, :hops * 512].reshape(C, hops, 512), tl.N, onset_sensitivity=0.5)[0] for k, v in streams.items()}
    for t in range(C):
        differs = not np.array_equal(raw["heard"][t], raw["own"][t], equal_nan=True)
        assert differs == (t in listening), t
        if t in listening:
            assert not np.array_equal(raw["heard"][t], raw["swapped"][t], equal_nan=True), t
    # and tick by tick the listeners' rows differ from their own in most words, and nobody else's in any
    for n, block, x, m, l in rig.heard:
        for t in np.flatnonzero(l):
            assert (block[t].view(np.uint32) != x[t].view(np.uint32)).mean() > 0.9 or n < 4, (n, t)
        assert np.array_equal(block[l == 0].view(np.uint32), x[l == 0].view(np.uint32))
