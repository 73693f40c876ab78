"""File sources (include/fx.h, fx_create_clips .. fx_push_sources) without a GPU: the C ABI declares and exports every entry and the
binding knows them, each refuses bad arguments before any device use, the launch record knows the gather, and the host model of a
tick (tests/clip_model.py) equals its own sample-by-sample loop."""
import ctypes
import os

import numpy as np
import pytest

import clip_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fx_create_clips", "fx_destroy_clips", "fx_set_channel_clips", "fx_set_channel_sources", "fx_transport", "fx_get_transport",
           "fx_push_sources")


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in text
        assert name in fx.capi.EXPORTS
        assert hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6
    for method in ("create_clips", "destroy_clips", "load_clips", "set_sources", "transport", "transport_state", "push_sources"):
        assert callable(getattr(fx.BatchAnalyser, method))


def test_header_and_binding_agree_on_the_constants(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read()
    c = fx.capi
    assert "enum { FX_SOURCE_INPUT = 0, FX_SOURCE_FILE = 1 };" in text and (c.SOURCE_INPUT, c.SOURCE_FILE) == (0, 1)
    assert ("enum { FX_TRANSPORT_NO_FILE = 0, FX_TRANSPORT_PLAYING = 1, FX_TRANSPORT_PAUSED = 2, FX_TRANSPORT_STOPPED = 3, "
            "FX_TRANSPORT_FINISHED = 4 };") in text
    assert (c.TRANSPORT_NO_FILE, c.TRANSPORT_PLAYING, c.TRANSPORT_PAUSED, c.TRANSPORT_STOPPED, c.TRANSPORT_FINISHED) == (0, 1, 2, 3, 4)
    assert "enum { FX_PLAY = 0, FX_PAUSE = 1, FX_STOP = 2, FX_RESTART = 3 };" in text and (c.PLAY, c.PAUSE, c.STOP, c.RESTART) == (0, 1, 2, 3)
    assert "enum { FX_CLIP_BORROW = 1 };" in text and c.CLIP_BORROW == 1
    # the model speaks the same numbers
    assert (cm.INPUT, cm.FILE) == (c.SOURCE_INPUT, c.SOURCE_FILE) and (cm.PLAY, cm.PAUSE, cm.STOP, cm.RESTART) == (c.PLAY, c.PAUSE, c.STOP, c.RESTART)
    assert (cm.NO_FILE, cm.PLAYING, cm.PAUSED, cm.STOPPED, cm.FINISHED) == (0, 1, 2, 3, 4)


def test_launch_kind_and_build_lists(fx):
    assert fx.capi.LAUNCH_KINDS[15] == "sources"
    text = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", "fx_kernels.h")).read()
    assert "FX_LAUNCH_SOURCES = 15" in text
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_clips.hip" in build.SOURCES and any(u[0] == "fx_clips.hip" for u in build.UNITS)
    assert "fx_clips.hip" not in build.HOST_SOURCES
    # the shim's host units refer to the unit through the context's hook only
    csrc = os.path.join(ROOT, "feature-extractor_amd", "csrc")
    for source in build.HOST_SOURCES:
        body = open(os.path.join(csrc, source)).read()
        for name in ENTRIES:
            assert name not in body, (source, name)
    assert "clips_release" in open(os.path.join(csrc, "fx_capi.cpp")).read()


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID, F32, HOST, DEVICE = fx.capi.FX_ERR_INVALID_ARGUMENT, fx.capi.SAMPLE_F32, fx.capi.MEM_HOST, fx.capi.MEM_DEVICE
    buf = (ctypes.c_float * 64)()
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                      # noqa: E731
    lens = lambda *v: (ctypes.c_longlong * len(v))(*v)                 # noqa: E731
    first, got = ctypes.c_int(7), ctypes.c_int(7)
    # A zeroed block stands in for a context (no tracks, no banks): each refusal below comes before the entry touches a device.
    fake = ctypes.create_string_buffer(1 << 16)
    misaligned = ctypes.c_void_p(ctypes.addressof(buf) + 2)

    def refused(status, *why):
        assert status == INVALID, (status, why, lib.fx_last_error())
        for w in why:
            assert w in lib.fx_last_error(), (why, lib.fx_last_error())

    # null context
    refused(lib.fx_create_clips(None, buf, lens(4), 1, F32, HOST, 0, ctypes.byref(first)), b"null context")
    refused(lib.fx_destroy_clips(None, 0), b"null context")
    refused(lib.fx_set_channel_clips(None, ints(0), 1, ints(0), None), b"null context")
    refused(lib.fx_set_channel_sources(None, ints(0), 1, ints(0)), b"null context")
    refused(lib.fx_transport(None, ints(0), 1, fx.capi.PLAY), b"null context")
    refused(lib.fx_get_transport(None, None, None, None, None), b"null context")
    refused(lib.fx_push_sources(None, buf, 4, F32, HOST, None, None, ctypes.byref(got)), b"null context")
    assert got.value == 0
    # negative counts
    refused(lib.fx_create_clips(fake, buf, lens(4), -1, F32, HOST, 0, ctypes.byref(first)), b"-1 clips")
    assert first.value == -1
    refused(lib.fx_create_clips(fake, buf, lens(4), 0, F32, HOST, 0, ctypes.byref(first)), b"0 clips")
    refused(lib.fx_set_channel_clips(fake, ints(0), -1, ints(0), None), b"negative channel count")
    refused(lib.fx_set_channel_sources(fake, ints(0), -2, ints(0)), b"negative channel count")
    refused(lib.fx_transport(fake, ints(0), -1, fx.capi.STOP), b"negative channel count")
    got.value = 7
    refused(lib.fx_push_sources(fake, buf, -1, F32, HOST, None, None, ctypes.byref(got)), b"negative sample count")
    assert got.value == 0
    # a list entry out of range (the stand-in has no tracks: track 0 is out of range already), and the entry is named
    refused(lib.fx_set_channel_clips(fake, ints(0, 0), 2, ints(-1, -1), None), b"entry 0", b"out of range")
    refused(lib.fx_set_channel_sources(fake, ints(-3), 1, ints(1)), b"entry 0", b"channel -3")
    refused(lib.fx_transport(fake, ints(5), 1, fx.capi.PAUSE), b"entry 0", b"channel 5")
    refused(lib.fx_set_channel_clips(fake, None, 2, ints(-1, -1), None), b"null channel list")
    # unknown command, source, clip id
    for command in (-1, 4, 99):
        refused(lib.fx_transport(fake, ints(0), 1, command), b"unknown transport command %d" % command)
    refused(lib.fx_set_channel_sources(fake, ints(0, 0), 2, ints(1, 2)), b"entry 1", b"unknown source 2")
    refused(lib.fx_set_channel_clips(fake, ints(0, 0), 2, ints(-1, 3), None), b"entry 1", b"unknown clip id 3")
    refused(lib.fx_set_channel_clips(fake, ints(0), 1, ints(-2), None), b"entry 0", b"unknown clip id -2")
    refused(lib.fx_destroy_clips(fake, 0), b"no bank starts at clip id 0")
    # clips: a length below 1, a borrowed host bank, unknown format / kind / flags, a misaligned device bank
    refused(lib.fx_create_clips(fake, buf, lens(4, 0, 4), 3, F32, HOST, 0, ctypes.byref(first)), b"lengths[1] = 0")
    refused(lib.fx_create_clips(fake, buf, lens(-4), 1, F32, HOST, 0, ctypes.byref(first)), b"lengths[0] = -4")
    refused(lib.fx_create_clips(fake, buf, lens(4), 1, F32, HOST, fx.capi.CLIP_BORROW, ctypes.byref(first)), b"FX_CLIP_BORROW")
    refused(lib.fx_create_clips(fake, buf, lens(4), 1, 99, HOST, 0, ctypes.byref(first)), b"unknown sample format")
    refused(lib.fx_create_clips(fake, buf, lens(4), 1, F32, 7, 0, ctypes.byref(first)), b"unknown memory kind")
    refused(lib.fx_create_clips(fake, buf, lens(4), 1, F32, HOST, 6, ctypes.byref(first)), b"unknown flags")
    refused(lib.fx_create_clips(fake, None, lens(4), 1, F32, HOST, 0, ctypes.byref(first)), b"null argument")
    refused(lib.fx_create_clips(fake, misaligned, lens(4), 1, F32, DEVICE, fx.capi.CLIP_BORROW, ctypes.byref(first)), b"4-byte aligned")
    assert first.value == -1
    # a tick: unknown format / kind, a misaligned device block
    for args, why in [((buf, 4, 99, HOST), b"unknown sample format"), ((buf, 4, F32, 7), b"unknown memory kind"),
                      ((misaligned, 4, F32, DEVICE), b"4-byte aligned")]:
        got.value = 7
        refused(lib.fx_push_sources(fake, *args, None, None, ctypes.byref(got)), why)
        assert got.value == 0
    # nothing to do is no error
    OK = fx.capi.FX_OK
    assert lib.fx_push_sources(fake, buf, 0, F32, HOST, None, None, None) == OK
    assert lib.fx_set_channel_clips(fake, None, 0, None, None) == OK and lib.fx_set_channel_sources(fake, None, 0, None) == OK
    assert lib.fx_transport(fake, None, 0, fx.capi.PLAY) == OK


class _NoLibrary:
    """stands in for the library: any use of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the binding used the library (%s) before refusing its arguments" % name)


def test_binding_refuses_before_any_library_use(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)          # no context: the refusals come first
    an.num_channels, an.window_size, an.device, an._lib, an._h = 4, 1024, 0, _NoLibrary(), None
    with pytest.raises(ValueError, match="out of range"):
        an.load_clips([4], 0)
    with pytest.raises(ValueError, match="out of range"):
        an.transport([-1], "play")
    with pytest.raises(ValueError, match="one of"):
        an.transport([0], "rewind")
    with pytest.raises(ValueError, match="integers or one of"):
        an.set_sources([0], "tape")
    with pytest.raises(ValueError, match="one value per listed track"):
        an.load_clips([0, 1, 2], [0, 1])
    with pytest.raises(ValueError, match="add up"):
        an.create_clips(np.zeros(10, np.float32), lengths=[4, 5])
    with pytest.raises(ValueError, match="lengths"):
        an.create_clips(np.zeros(10, np.float32))
    with pytest.raises(ValueError, match="borrowed"):
        an.create_clips(np.zeros(10, np.float32), lengths=[10], borrow=True)
    with pytest.raises(ValueError, match="multiple of 3"):
        an.create_clips(np.zeros(10, np.uint8), lengths=[3], sample_format="s24")
    with pytest.raises(ValueError, match="num_samples"):
        an.push_sources()
    with pytest.raises(ValueError, match="multiple of the channel count"):
        an.push_sources(np.zeros(10, np.float32))


LENGTHS = [1, 5, 7, 479, 480, 481, 1000]
TICKS = [1, 63, 441, 480, 512, 1000]


def _clip(L, B, seed):
    return np.random.default_rng(seed).integers(0, 256, L * B, dtype=np.uint8)


@pytest.mark.parametrize("fmt", cm.FORMATS)
def test_model_equals_its_naive_loop(fmt):
    B = cm.BYTES[fmt]
    for L in LENGTHS:
        clip = _clip(L, B, L)
        for n in TICKS:
            for loop in (1, 0):
                for start in sorted({0, L // 3, L - 1, max(L - n, 0)}):
                    p = cm.Player()
                    p.source, p.state, p.loop, p.clip, p.L, p.position, p.laps = cm.FILE, cm.PLAYING, loop, clip, L, start, 2
                    q = p.copy()
                    for tick in range(3):           # a few ticks in a row: wraps and the end are met from every phase
                        a, b = cm.render(p, n, B), cm.render_naive(q, n, B)
                        assert a[0].dtype == np.uint8 and a[0].shape == (n * B,)
                        assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:], (fmt, L, n, loop, start, tick)
                        (_, p.position, p.laps, p.state), (_, q.position, q.laps, q.state) = a, b


@pytest.mark.parametrize("fmt", cm.FORMATS)
def test_one_shot_that_ends_exactly_with_the_tick_is_finished_and_all_real(fmt):
    B = cm.BYTES[fmt]
    for L in LENGTHS:
        clip = _clip(L, B, 100 + L)
        for n in [t for t in TICKS if t <= L]:
            p = cm.Player()
            p.source, p.state, p.loop, p.clip, p.L, p.position = cm.FILE, cm.PLAYING, 0, clip, L, L - n
            out, position, laps, state = cm.render(p, n, B)
            assert out.tobytes() == clip[(L - n) * B:].tobytes() and (position, laps, state) == (L, 0, cm.FINISHED)
            naive = cm.render_naive(p, n, B)
            assert naive[0].tobytes() == out.tobytes() and naive[1:] == (position, laps, state)
            if n > 1:                               # one sample short of the end: still playing
                p.position = L - n
                assert cm.render(p, n - 1, B)[1:] == (L - 1, 0, cm.PLAYING)


def test_model_commands_follow_the_contract():
    m = cm.Model(5, "s16")
    clip = _clip(10, 2, 1)
    assert m.load([0, 1, 2], [clip, clip, None], [1, 0, 1]) == [0, 1, 2]
    assert m.set_sources([0, 1, 2, 3], [cm.FILE] * 4) == [0, 1, 2, 3]
    assert list(m.table()["state"]) == [cm.STOPPED, cm.STOPPED, cm.NO_FILE, cm.NO_FILE, cm.NO_FILE]
    with pytest.raises(cm.Refused):
        m.transport([0, 2], cm.PLAY)                # track 2 has no file: the whole list is refused
    assert list(m.table()["state"])[:2] == [cm.STOPPED, cm.STOPPED]
    with pytest.raises(cm.Refused):
        m.tick(None, 4)                             # track 4 listens to the input
    assert m.transport([0, 1, 1], cm.PLAY) == [0, 1, 1]
    live = np.arange(5 * 8 * 2, dtype=np.uint8).reshape(5, 16)
    out = m.tick(live, 8)
    assert out[0].tobytes() == clip[:16].tobytes() and out[4].tobytes() == live[4].tobytes() and not out[2].any() and not out[3].any()
    out = m.tick(live, 8)                           # the loop wraps, the one-shot ends after two samples
    assert out[0].tobytes() == (clip[16:].tobytes() + clip[:12].tobytes())
    assert out[1].tobytes() == clip[16:].tobytes() + bytes(12)
    t = m.table()
    assert list(t["position"][:2]) == [6, 10] and list(t["laps"][:2]) == [1, 0] and list(t["state"][:2]) == [cm.PLAYING, cm.FINISHED]
    assert m.transport([1], cm.RESTART) == [] and m.players[1].state == cm.STOPPED and m.players[1].position == 0
    m.transport([0], cm.PAUSE)
    assert m.transport([0], cm.RESTART) == [] and m.players[0].state == cm.PAUSED and m.players[0].position == 0
    m.transport([1], cm.PLAY); m.tick(np.zeros((5, 20), np.uint8), 10)
    assert m.players[1].state == cm.FINISHED
    m.transport([1], cm.PLAY)
    assert (m.players[1].state, m.players[1].position) == (cm.PLAYING, 0)
    m.set_sources([1], [cm.INPUT])
    assert (m.players[1].source, m.players[1].state, m.players[1].position) == (cm.INPUT, cm.STOPPED, 0)
    m.transport([0, 1, 2], cm.STOP)
    assert list(m.table()["state"][:3]) == [cm.STOPPED, cm.STOPPED, cm.NO_FILE]
