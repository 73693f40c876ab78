"""The monitor mix (include/fx.h, fx_enable_monitor .. fx_get_monitor) without a GPU: the C ABI declares and exports the entries and the
binding knows them, each refuses bad arguments before any device use, the launch record knows the mix, the host model
(tests/monitor_model.py) equals its own sample-by-sample loop -- and the data the GPU test mixes tells the specified summation order
from the orders a kernel might take instead."""
import ctypes
import os

import numpy as np
import pytest

import monitor_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fx_enable_monitor", "fx_set_channel_monitor", "fx_get_channel_monitor", "fx_get_monitor")
BLOCKS = [63, 441, 480, 512, 1000, 4097]            # the GPU test's block lengths from 63 on


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in text
        assert name in fx.capi.EXPORTS
        assert hasattr(lib, name)
    assert "#define FX_MONITOR_GROUP 64" in text and fx.capi.MONITOR_GROUP == 64 == mm.GROUP
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    for method in ("enable_monitor", "set_monitor", "monitor_sends", "get_monitor"):
        assert callable(getattr(fx.BatchAnalyser, method))
    mirror = open(os.path.join(ROOT, "include", "fx_realtime.hpp")).read()
    for name in ENTRIES:
        assert name + " (" in mirror, name


def test_launch_kind_and_build_lists(fx):
    assert fx.capi.LAUNCH_KINDS[17] == "monitor"
    text = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", "fx_kernels.h")).read()
    assert "FX_LAUNCH_MONITOR = 17" in text
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_monitor.hip" in build.SOURCES and any(u[0] == "fx_monitor.hip" for u in build.UNITS)
    assert "fx_monitor.hip" not in build.HOST_SOURCES
    # the shim's host units refer to the unit through the context's hooks only
    csrc = os.path.join(ROOT, "feature-extractor_amd", "csrc")
    for source in build.HOST_SOURCES:
        body = open(os.path.join(csrc, source)).read()
        for name in ENTRIES:
            assert name not in body, (source, name)
    assert "monitor_release" in open(os.path.join(csrc, "fx_capi.cpp")).read()
    # and the tick reaches it through them too
    clips = open(os.path.join(csrc, "fx_clips.hip")).read()
    assert "monitor_prepare" in clips and "monitor_launch" in clips and not any(name in clips for name in ENTRIES)
    assert clips.index("monitor_prepare(c") < clips.index("launch_clip_gather_kernel(p, esz") < clips.index("monitor_launch(c") < clips.index("st = fx_push_block(")


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID, OK, HOST, DEVICE = fx.capi.FX_ERR_INVALID_ARGUMENT, fx.capi.FX_OK, fx.capi.MEM_HOST, fx.capi.MEM_DEVICE
    buf = (ctypes.c_float * 64)()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                      # noqa: E731
    floats = lambda *v: (ctypes.c_float * len(v))(*v)                  # noqa: E731
    got = ctypes.c_int(7)
    # A zeroed block stands in for a context (no tracks, no monitor): each refusal below comes before the entry touches a device.
    fake = ctypes.create_string_buffer(1 << 16)

    def refused(status, *why):
        assert status == INVALID, (status, why, lib.fx_last_error())
        for w in why:
            assert w in lib.fx_last_error(), (why, lib.fx_last_error())

    # null context
    refused(lib.fx_enable_monitor(None, 1), b"null context")
    refused(lib.fx_set_channel_monitor(None, ints(0), 1, None, None, None), b"null context")
    refused(lib.fx_get_channel_monitor(None, None, None, None), b"null context")
    refused(lib.fx_get_monitor(None, buf, 32, ctypes.byref(got), HOST), b"null context")
    assert got.value == 0
    # a negative count, a null list
    refused(lib.fx_set_channel_monitor(fake, ints(0), -1, None, None, None), b"negative channel count -1")
    refused(lib.fx_set_channel_monitor(fake, None, 2, None, None, None), b"null channel list")
    # a list entry out of range (the stand-in has no tracks: track 0 is out of range already), and the entry is named
    refused(lib.fx_set_channel_monitor(fake, ints(0, 0), 2, None, None, None), b"entry 0", b"out of range")
    refused(lib.fx_set_channel_monitor(fake, ints(-3), 1, ints(1), floats(1.0), floats(1.0)), b"entry 0", b"channel -3")
    # a gain that is NaN or infinite, at a named entry (the call's own values come before the range of its entries)
    nan, inf = float("nan"), float("inf")
    refused(lib.fx_set_channel_monitor(fake, ints(0, 0, 0), 3, None, floats(1.0, 0.5, nan), None), b"entry 2", b"left gain")
    refused(lib.fx_set_channel_monitor(fake, ints(0, 0), 2, ints(1, 0), floats(1.0, 0.5), floats(2.0, -inf)), b"entry 1", b"right gain")
    refused(lib.fx_set_channel_monitor(fake, ints(0, 0), 2, None, floats(inf, nan), floats(nan, 1.0)), b"entry 0", b"left gain")
    # the mix: a null out, an unknown memory kind
    got.value = 7
    refused(lib.fx_get_monitor(fake, None, 32, ctypes.byref(got), HOST), b"null output")
    assert got.value == 0
    refused(lib.fx_get_monitor(fake, buf, 32, ctypes.byref(got), 7), b"unknown memory kind 7")
    refused(lib.fx_get_monitor(fake, buf, 32, None, -1), b"unknown memory kind -1")
    # no monitor
    for status in (lib.fx_get_monitor(fake, buf, 32, ctypes.byref(got), HOST), lib.fx_get_monitor(fake, buf, 32, ctypes.byref(got), DEVICE),
                   lib.fx_get_channel_monitor(fake, None, None, None), lib.fx_set_channel_monitor(fake, None, 0, None, None, None)):
        refused(status, b"monitor is not enabled", b"fx_enable_monitor")
    # freeing a monitor that does not exist is nothing to do
    assert lib.fx_enable_monitor(fake, 0) == OK


class _NoLibrary:
    """stands in for the library: any use of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the binding used the library (%s) before refusing its arguments" % name)


def test_binding_refuses_before_any_library_use(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)          # no context: the refusals come first
    an.num_channels, an.window_size, an.device, an._lib, an._h = 4, 1024, 0, _NoLibrary(), None
    with pytest.raises(ValueError, match="out of range"):
        an.set_monitor([4])
    with pytest.raises(ValueError, match="out of range"):
        an.set_monitor([0, -1], on=[1, 1])
    with pytest.raises(ValueError, match="holds integers"):
        an.set_monitor([0.5])
    with pytest.raises(ValueError, match="one value per listed track"):
        an.set_monitor([0, 1, 2], on=[1, 0])
    with pytest.raises(ValueError, match="one left gain per listed track"):
        an.set_monitor([0, 1, 2], left=[1.0, 0.5])
    with pytest.raises(ValueError, match="entry 1: the right gain"):
        an.set_monitor([0, 1], right=[1.0, float("nan")])
    with pytest.raises(ValueError, match="entry 0: the left gain"):
        an.set_monitor([2], left=float("inf"))


@pytest.mark.parametrize("C", [1, 6, 64, 65, 70, 130])
def test_model_equals_its_naive_loop(C):
    n = 37
    x = mm.data(C, n, C)
    rng = np.random.default_rng(C)
    on = (rng.random(C) < 0.8).astype(np.int32)
    left, right = mm.gains(C, C + 1)
    left[0], right[C - 1] = 0.0, 1e-36                        # a zero gain, subnormal products
    x[C // 2, [3, 5]] = [np.inf, np.nan]                      # in a track that is on or off, as the draw has it
    a, b = mm.mix(x, on, left, right), mm.mix_naive(x, on, left, right)
    assert a.dtype == np.float32 and a.shape == (2, n) and mm.bits_same(a, b)
    # off tracks contribute nothing at all: whatever they carry
    x[on == 0] = np.nan
    x[C // 2, [3, 5]] = 1.0
    assert np.isfinite(mm.mix(x, on, left, right)).all()
    # no track on: every word is +0
    assert not mm.mix(x, np.zeros(C, np.int32), left, right).view(np.uint32).any()


@pytest.mark.parametrize("C", [70, 130])
def test_the_data_tells_the_summation_orders_apart(C):
    """a kernel that sums flat, in groups of 32 or in fp64 cannot pass the GPU test: on data of four decades and gains in [-2, 2] each
    of those orders differs from the specified one in some sample of every block length of 63 and more (in 44-92 % of them)"""
    on = np.ones(C, np.int32)
    left, right = mm.gains(C, 3)
    for n in BLOCKS:
        x = mm.data(C, n, 1000 * C + n)
        want = mm.mix(x, on, left, right)
        for name, other in (("flat", mm.mix(x, on, left, right, group=C)), ("groups of 32", mm.mix(x, on, left, right, group=32)),
                            ("fp64", mm.mix_f64(x, on, left, right))):
            differ = (want.view(np.uint32) != other.view(np.uint32)).mean()
            assert differ > 0.2, (C, n, name, differ)
            assert np.abs(want - other).max() < 1e-4, (C, n, name)        # (and they are the same sum all the same)


@pytest.mark.parametrize("C", [6, 64, 65])
def test_up_to_65_tracks_the_specified_order_is_the_flat_sum(C):
    """the second group holds at most one track there, and +0 + x is x: nobody should mistake these sizes for a test of the order"""
    on = np.ones(C, np.int32)
    left, right = mm.gains(C, 4)
    x = mm.data(C, 480, C)
    assert mm.bits_same(mm.mix(x, on, left, right), mm.mix(x, on, left, right, group=C))


def test_the_gpu_tests_own_ticks_tell_the_orders_apart():
    """the same for what tests/test_gpu_monitor.py really mixes -- clips, silent tracks, sends off, one whole group off at 130 tracks,
    every format: its contexts of 70 and 130 tracks run here on the models alone"""
    import test_gpu_monitor as tg
    seen = 0
    for C, fmt, N, _ in tg.CASES:
        if C not in (70, 130):
            continue
        for n, want, x, (on, left, right) in tg.run_case(None, C, fmt, N, False, tg.BLOCKS):
            assert want.shape == (2, n) and x.shape == (C, n)
            if n >= 63:
                flat = mm.mix(x, on, left, right, group=C)
                assert (want.view(np.uint32) != flat.view(np.uint32)).any(), (C, fmt, n)
                seen += 1
    assert seen == 2 * 4 * 5
