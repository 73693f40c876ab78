"""Audio display levels (include/fx.h, fx_enable_display / fx_set_display_samples_per_block / fx_clear_display_channels /
fx_get_display) without a GPU: the C ABI declares, exports and binds the four entries, the ABI number is unchanged, every refusal
comes before any device use and names its argument, the unit attaches through hooks only, the segment-summary combine folds any split
of a run to the sequential model's bits, and the model (tests/display_model.py) is held to cases written out by hand."""
import ctypes
import os
import re

import numpy as np
import pytest

import display_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fx_enable_display", "fx_set_display_samples_per_block", "fx_clear_display_channels", "fx_get_display")
F32 = np.float32


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in text
        assert name in fx.capi.EXPORTS
        assert hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    # every entry cites the reference
    for cite in ("AnalyserTrackController.h:74-78", "AudioDataCollector.h:88-91", "AnalyserTrack.h:148-157", "AnalyserTrack.h:27-29",
                 "AnalyserTrackController.h:154-158", "AnalyserTrackController.h:105,114"):
        assert cite.replace(" (", "(") in text, cite
    for method in ("enable_display", "set_display_samples_per_block", "clear_display", "display"):
        assert callable(getattr(fx.BatchAnalyser, method))
    rt = open(os.path.join(ROOT, "include", "fx_realtime.hpp")).read()
    for method in ("enableDisplay", "setSamplesPerBlock", "clearDisplay", "getDisplayLevels"):
        assert re.search(r"\b%s\s*\(" % method, rt), method


def test_launch_kind(fx):
    assert fx.capi.LAUNCH_KINDS[14] == "display"
    text = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", "fx_kernels.h")).read()
    assert "constexpr int FX_LAUNCH_DISPLAY = 14;" in text
    assert "constexpr int FX_LAUNCH_OSC_BUNDLE = 13;" in text               # the kinds before it are as they were


def test_the_unit_attaches_through_hooks_only():
    """The shim's host units refer to no symbol of fx_display.hip (the fake-HIP host builds compile them without the unit)"""
    import importlib
    build = importlib.import_module("feature-extractor_amd.build")
    for source in build.HOST_SOURCES:
        shim = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", source)).read()
        assert not re.search(r"fx_(enable|get)_display\s*\(|fx_set_display_samples_per_block\s*\(|fx_clear_display_channels\s*\(", shim), source
        assert "FX_LAUNCH_DISPLAY" not in shim and "fx_display_kernel" not in shim, source
    assert "fx_display.hip" in build.SOURCES and any(u[0] == "fx_display.hip" for u in build.UNITS)


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID = fx.capi.FX_ERR_INVALID_ARGUMENT
    out = (ctypes.c_float * 64)()
    lst = (ctypes.c_int * 4)(0, 0, 0, 0)
    assert lib.fx_enable_display(None, 256, 1024) == INVALID and b"null context" in lib.fx_last_error()
    assert lib.fx_set_display_samples_per_block(None, 256) == INVALID and b"null context" in lib.fx_last_error()
    assert lib.fx_clear_display_channels(None, lst, 1) == INVALID and b"null context" in lib.fx_last_error()
    assert lib.fx_get_display(None, lst, 1, out, 0) == INVALID and b"null context" in lib.fx_last_error()
    # A zeroed block stands in for a context (of no channels): each refusal below comes before the entry touches a device.
    fake = ctypes.create_string_buffer(1 << 16)
    for length in (-1, 4097, 2 ** 31 - 1):
        assert lib.fx_enable_display(fake, 256, length) == INVALID, length
        assert b"buffer_size" in lib.fx_last_error(), lib.fx_last_error()
    for spb in (0, -1, 65537, 2 ** 31 - 1):
        assert lib.fx_enable_display(fake, spb, 1024) == INVALID, spb
        assert b"samples_per_block" in lib.fx_last_error(), lib.fx_last_error()
        assert lib.fx_set_display_samples_per_block(fake, spb) == INVALID, spb
        assert b"samples_per_block" in lib.fx_last_error(), lib.fx_last_error()
    # disabling a display that was never enabled is nothing to do
    assert lib.fx_enable_display(fake, 256, 0) == fx.capi.FX_OK
    # a context without a display
    assert lib.fx_set_display_samples_per_block(fake, 256) == INVALID and b"not enabled" in lib.fx_last_error()
    assert lib.fx_clear_display_channels(fake, None, 0) == INVALID and b"not enabled" in lib.fx_last_error()
    assert lib.fx_get_display(fake, None, 0, out, 0) == INVALID and b"not enabled" in lib.fx_last_error()
    # bad lists: the entry is named (the stand-in has no channels, so entry 0 is already out of range)
    assert lib.fx_clear_display_channels(fake, lst, 2) == INVALID and b"entry 0" in lib.fx_last_error()
    assert lib.fx_get_display(fake, lst, 2, out, 0) == INVALID and b"entry 0" in lib.fx_last_error()
    assert lib.fx_clear_display_channels(fake, lst, -1) == INVALID and b"negative" in lib.fx_last_error()
    assert lib.fx_get_display(fake, lst, -1, out, 0) == INVALID and b"negative" in lib.fx_last_error()
    assert lib.fx_clear_display_channels(fake, None, 3) == INVALID and b"null channel list" in lib.fx_last_error()
    assert lib.fx_get_display(fake, None, 3, out, 0) == INVALID and b"null channel list" in lib.fx_last_error()
    assert lib.fx_get_display(fake, None, 0, out, 7) == INVALID and b"memory kind" in lib.fx_last_error()
    assert bytes(fake.raw) == bytes(1 << 16)          # and none of them wrote to the context


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU error path")
def test_a_well_formed_enable_needs_a_device(fx):
    lib = fx.load_library()
    fake = ctypes.create_string_buffer(1 << 16)
    assert lib.fx_enable_display(fake, 256, 1024) == fx.capi.FX_ERR_NO_DEVICE
    assert bytes(fake.raw) == bytes(1 << 16)


def test_binding_refuses_before_the_library(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)
    an.num_channels, an.window_size, an.device, an._h = 4, 1024, 0, None
    an._lib = fx.load_library()
    with pytest.raises(fx.FxError, match="null context"):
        an.enable_display()
    with pytest.raises(fx.FxError, match="null context"):
        an.set_display_samples_per_block(64)
    with pytest.raises(ValueError, match="out of range"):
        an.clear_display([4])
    with pytest.raises(ValueError, match="out of range"):
        an.display([-1])
    with pytest.raises(fx.FxError, match="null context"):
        an.display()
    an._h = None            # (nothing to destroy)


# ---- the combine rule against the sequential model ----
SPECIAL = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1.0, -1.0, -1.0, 3.5, -3.5]


def _runs():
    rng = np.random.default_rng(20240607)
    for n in list(range(1, 41)) + [40] * 20:
        x = rng.standard_normal(n).astype(F32)
        # seeded with NaN, +-inf, +0 / -0 and repeated extremes
        k = rng.integers(0, n + 1)
        at = rng.integers(0, n, size=k)
        x[at] = rng.choice(np.array(SPECIAL, F32), size=k)
        if n > 3 and rng.random() < 0.5:
            x[rng.integers(0, n, size=3)] = x.max() if not np.isnan(x.max()) else F32(7.0)      # a repeated extreme
        yield x
    yield np.array([0.0, -0.0, 0.0, -0.0], F32)
    yield np.array([-0.0, 0.0], F32)
    yield np.array([np.nan], F32)
    yield np.array([1.0, np.nan], F32)
    yield np.array([np.nan, np.nan, 2.0, -0.0, 0.0], F32)


def test_folding_any_split_equals_the_sequential_model():
    checked = 0
    for x in _runs():
        for carried in ((F32(0.0), F32(0.0)), (F32(-2.0), F32(0.5)), (F32(np.nan), F32(np.nan)), (F32(-0.0), F32(-0.0))):
            want = dm.sequential_value(carried, x)
            whole = dm.combine((carried[0], carried[1], False), dm.fold(x))
            assert dm.bits(whole[:2]).tolist() == dm.bits(want).tolist(), (x, carried)
            for cut in range(1, len(x)):
                # [carried | left] folded first, then the right run; and the right run folded on its own first (associativity)
                left = dm.combine((carried[0], carried[1], False), dm.fold(x[:cut]))
                got = dm.combine(left, dm.fold(x[cut:]))
                assert dm.bits(got[:2]).tolist() == dm.bits(want).tolist(), (x, carried, cut)
                checked += 1
        # a block's first sample starts from (x, x): no carried value
        t = dm.Track(len(x) + 5, 4)
        t.push(x)
        assert dm.bits(t.value).tolist() == dm.bits(dm.fold(x)[:2]).tolist(), x
    assert checked > 5000


def test_three_way_splits_are_associative():
    rng = np.random.default_rng(5)
    for _ in range(300):
        x = rng.choice(np.array(SPECIAL + [0.25, -0.25], F32), size=9)
        a, b = sorted(rng.integers(1, 9, size=2))
        if a == b:
            continue
        A, B, C = dm.fold(x[:a]), dm.fold(x[a:b]), dm.fold(x[b:])
        l = dm.combine(dm.combine(A, B), C)
        r = dm.combine(A, dm.combine(B, C))
        assert dm.bits(l[:2]).tolist() == dm.bits(r[:2]).tolist() and l[2] == r[2], x


# ---- the model against cases written out by hand ----
def _pairs(a):
    return [tuple(float(v) for v in row) for row in np.asarray(a)]


def test_first_entry_is_zero_and_a_block_is_published_one_sample_late():
    t = dm.Track(3, 4)
    t.push([5, 1, 2])
    # the first sample published the new component's (0, 0); the block (1, 5) is complete but not yet out
    assert t.next == 1 and _pairs(t.levels) == [(0, 0), (0, 0), (0, 0), (0, 0)] and t.value == (1, 5) and t.sub == 1
    t.push([7])
    assert t.next == 2 and _pairs(t.levels)[1] == (1, 5) and t.value == (7, 7) and t.sub == 3
    assert _pairs(t.draw_order()) == [(0, 0), (0, 0), (0, 0), (1, 5)]


def test_samples_per_block_one():
    t = dm.Track(1, 3)
    t.push([4, -1, 9, 2, 6])
    # every sample publishes the one before it; the ring holds the last three publications: 9, 2 and -1 ...
    assert _pairs(t.draw_order()) == [(-1, -1), (9, 9), (2, 2)] and t.value == (6, 6)
    assert t.next == 2 and t.sub == 1


def test_clear_keeps_next():
    t = dm.Track(2, 4)
    t.push([1, 2, 3, 4, 5])
    assert t.next == 3
    t.clear()
    assert t.next == 3 and t.sub == 0 and t.value == (0, 0) and not t.levels.any()
    t.push([8, 9, 7])
    # the first entry after a clear is (0, 0), stored at the slot the ring had reached
    assert _pairs(t.levels) == [(8, 9), (0, 0), (0, 0), (0, 0)] and t.next == 1
    assert _pairs(t.draw_order()) == [(0, 0), (0, 0), (0, 0), (8, 9)]


def test_samples_per_block_change_in_mid_block():
    t = dm.Track(4, 8)
    t.push([1, 2])                      # (0, 0) out; the running block has two of its four samples
    t.set_samples_per_block(2)
    t.push([3, 4, 5, 6, 7])             # the running block still ends after four; the ones after it after two
    assert _pairs(t.levels)[:4] == [(0, 0), (1, 4), (5, 6), (0, 0)] and t.value == (7, 7) and t.sub == 2
    t.set_samples_per_block(5)
    t.push([0, 1, 2, 3, 4, 5])          # (7, 7) runs to two samples; the next block takes five
    assert _pairs(t.levels)[3] == (0, 7) and t.value == (1, 5) and t.sub == 1


def test_ties_take_the_newer_sample_and_nan_is_replaced():
    t = dm.Track(10, 4)
    t.push([0.0, -0.0])
    assert dm.bits(t.value).tolist() == dm.bits([-0.0, -0.0]).tolist()
    t.push([0.0])
    assert dm.bits(t.value).tolist() == dm.bits([0.0, 0.0]).tolist()
    t.push([-3, np.nan])
    assert np.isnan(t.value[0]) and np.isnan(t.value[1])
    t.push([2.5])
    assert t.value == (2.5, 2.5)
