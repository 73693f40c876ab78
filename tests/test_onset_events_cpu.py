"""The onset event list (include/fx.h, fx_enable_onset_events / fx_get_onset_events) without a GPU: the C ABI declares and exports
both entries, the ABI number is unchanged, the Python structure is the C one, every refusal comes before any device use and names
its argument, the launch record knows the step, and the model of the contract (tests/onset_events_model.py) is held to cases
written out by hand."""
import ctypes
import os

import numpy as np
import pytest

import onset_events_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fx_enable_onset_events", "fx_get_onset_events")


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in text
        assert name in fx.capi.EXPORTS
        assert hasattr(lib, name)
    assert "typedef struct fx_onset_event { long long frame; int channel; int call_frame; } fx_onset_event;" in text
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    # the header cites the reference's callback and says what the ring does not do
    assert "RealTimeAnalyser.h:228-229" in text and "AnalyserTrackController.h:80-84" in text
    assert "ring does not produce events" in text


def test_structure_and_launch_kind(fx):
    assert ctypes.sizeof(fx.capi.OnsetEvent) == 16
    assert [f[0] for f in fx.capi.OnsetEvent._fields_] == ["frame", "channel", "call_frame"]
    assert fx.capi.ONSET_EVENT_DTYPE.itemsize == 16 and fx.capi.ONSET_EVENT_DTYPE == om.EVENT_DTYPE
    assert fx.capi.ONSET_EVENT_DTYPE.fields["channel"][1] == 8 and fx.capi.ONSET_EVENT_DTYPE.fields["call_frame"][1] == 12
    assert fx.capi.LAUNCH_KINDS[11] == "onset_events"
    text = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", "fx_kernels.h")).read()
    assert "constexpr int FX_LAUNCH_ONSET_EVENTS = 11;" in text
    assert "FX_LAUNCH_TAPS, FX_LAUNCH_DEINTERLEAVE }" in text           # the enum itself is as it was


def test_the_unit_attaches_through_hooks_only():
    """The shim's host units refer to no symbol of fx_events.hip (the sanitised host builds compile them without the unit)"""
    import importlib
    import re
    build = importlib.import_module("feature-extractor_amd.build")
    for source in build.HOST_SOURCES:
        shim = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", source)).read()
        assert not re.search(r"fx_(enable|get)_onset_events\s*\(", shim), source
        assert "FX_LAUNCH_ONSET_EVENTS" not in shim, source
    assert "fx_events.hip" in build.SOURCES and any(u[0] == "fx_events.hip" for u in build.UNITS)


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID = fx.capi.FX_ERR_INVALID_ARGUMENT
    ev = (fx.capi.OnsetEvent * 4)()
    n, lost = ctypes.c_int(7), ctypes.c_longlong(7)
    assert lib.fx_enable_onset_events(None, 16) == INVALID
    assert b"null context" in lib.fx_last_error()
    assert lib.fx_get_onset_events(None, ev, 4, ctypes.byref(n), ctypes.byref(lost)) == INVALID
    assert b"null context" in lib.fx_last_error() and n.value == 0 and lost.value == 0
    # A zeroed block stands in for a context: each refusal below comes before the entry touches a device (this machine has none).
    fake = ctypes.create_string_buffer(1 << 16)
    for capacity in (-1, -(1 << 30), (1 << 26) + 1, 2 ** 31 - 1):
        assert lib.fx_enable_onset_events(fake, capacity) == INVALID, capacity
        assert b"capacity" in lib.fx_last_error(), lib.fx_last_error()
    # disabling a list that was never enabled is nothing to do
    assert lib.fx_enable_onset_events(fake, 0) == fx.capi.FX_OK
    cases = [((ev, -1), b"negative cap"),
             ((None, 4), b"null out"),
             ((ev, 4), b"not enabled"),
             ((None, 0), b"not enabled")]
    for (out, cap), why in cases:
        n.value, lost.value = 7, 7
        assert lib.fx_get_onset_events(fake, out, cap, ctypes.byref(n), ctypes.byref(lost)) == INVALID, why
        assert why in lib.fx_last_error() and n.value == 0 and lost.value == 0, (why, lib.fx_last_error())
    assert bytes(fake.raw) == bytes(1 << 16)          # and none of them wrote to the context


def test_binding_refuses_before_the_library(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)
    an.num_channels, an.window_size, an.device, an._h = 4, 1024, 0, None
    an._lib = fx.load_library()
    with pytest.raises(fx.FxError, match="null context"):
        an.enable_onset_events(16)
    with pytest.raises(fx.FxError, match="null context"):
        an.onset_events()
    an._h = None            # (nothing to destroy)


def test_sharded_gather_offsets_each_shards_channels(fx):
    import importlib
    sh = importlib.import_module("feature-extractor_amd.sharded")
    # 10 channels over 3 ranks: shards [0,4) [4,8) [8,10)
    parts = [om.as_array([(0, 3, 0), (2, 0, 0)]), om.as_array([(0, 0, 0), (1, 3, 1)]), om.as_array([(0, 1, 0)])]
    got = om.as_tuples(sh.gather_onset_events(parts, 10))
    assert got == [(0, 3, 0), (0, 4, 0), (0, 9, 0), (1, 7, 1), (2, 0, 0)]
    assert parts[1]["channel"].tolist() == [0, 3]                       # the inputs are left as they were
    with pytest.raises(ValueError, match="reported channel"):
        sh.gather_onset_events([om.as_array([(0, 4, 0)]), om.as_array([]), om.as_array([])], 10)


# ---- the model against cases written out by hand ----
def _flags(C, T, ones):
    f = np.zeros((C, T), np.float32)
    for c, t in ones:
        f[c, t] = 1.0
    return f


def test_model_order_is_frame_then_channel():
    f = _flags(5, 3, [(4, 0), (1, 0), (0, 2), (3, 1), (2, 2)])
    assert om.events_of_call(f) == [(0, 1, 0), (0, 4, 0), (1, 3, 1), (2, 0, 2), (2, 2, 2)]
    assert om.events_of_call(f, frames_before=10) == [(10, 1, 0), (10, 4, 0), (11, 3, 1), (12, 0, 2), (12, 2, 2)]
    # only 1 counts: NaN (a slot nobody wrote), 0.5 and 2 are not events
    g = np.array([[np.nan, 0.5], [2.0, 1.0]], np.float32)
    assert om.events_of_call(g) == [(1, 1, 1)]


def test_model_overflow_in_the_middle_of_a_frame():
    # frame 0 has three events, frame 1 two; room for four: the list ends inside frame 1
    f = _flags(4, 2, [(0, 0), (1, 0), (3, 0), (1, 1), (2, 1)])
    (ev, lost), = om.simulate([f], 4, {0: None})
    assert ev == [(0, 0, 0), (0, 1, 0), (0, 3, 0), (1, 1, 1)] and lost == 1
    # the next call's events go behind a list that is still full: all of them are lost; a drain makes room again
    lst = om.EventList(4)
    lst.call(f)
    lst.call(_flags(4, 1, [(0, 0), (2, 0)]))
    assert lst.count() == 4
    assert lst.drain() == ([(0, 0, 0), (0, 1, 0), (0, 3, 0), (1, 1, 1)], 3)
    lst.call(_flags(4, 1, [(2, 0)]))
    assert lst.drain() == ([(3, 2, 0)], 0)


def test_model_partial_drain_keeps_the_rest():
    a = _flags(3, 2, [(0, 0), (2, 0), (1, 1)])
    b = _flags(3, 1, [(0, 0), (1, 0)])
    got = om.simulate([a, b], 16, {0: 2, 1: None})
    assert got[0] == ([(0, 0, 0), (0, 2, 0)], 0)
    assert got[1] == ([(1, 1, 1), (2, 0, 0), (2, 1, 0)], 0)
    lst = om.EventList(16)
    lst.call(a)
    assert lst.drain(0) == ([], 0) and lst.count() == 3
    assert lst.drain(1) == ([(0, 0, 0)], 0)
    assert lst.drain(5) == ([(0, 2, 0), (1, 1, 1)], 0)
    assert lst.drain(5) == ([], 0)


def test_model_dropped_is_reported_once():
    lst = om.EventList(1)
    lst.call(_flags(2, 2, [(0, 0), (1, 0), (1, 1)]))
    assert lst.drain(0) == ([], 2)              # a drain of nothing still reports and clears the count
    assert lst.drain() == ([(0, 0, 0)], 0)


def test_model_reset_and_disable_reenable():
    lst = om.EventList(2)
    lst.call(_flags(2, 3, [(0, 0), (1, 1), (0, 2)]))
    lst.reset()
    assert lst.count() == 0 and lst.capacity == 2
    lst.call(_flags(2, 1, [(1, 0)]))
    assert lst.drain() == ([(0, 1, 0)], 0)      # frames count from 0 again, nothing dropped carried over
    # disabled: calls go by, the frame count goes on; re-enabled: an empty list that picks up at the stream's frame
    lst.enable(0)
    lst.call(_flags(2, 4, [(0, 0), (1, 3)]))
    with pytest.raises(ValueError):
        lst.drain()
    lst.enable(8)
    lst.call(_flags(2, 1, [(0, 0)]))
    assert lst.drain() == ([(5, 0, 0)], 0)
    # a resize drops what is stored
    lst.call(_flags(2, 1, [(0, 0), (1, 0)]))
    lst.enable(4)
    assert lst.count() == 0 and lst.drain() == ([], 0)
    with pytest.raises(ValueError):
        lst.enable(-1)
    with pytest.raises(ValueError):
        lst.enable((1 << 26) + 1)
