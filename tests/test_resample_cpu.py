"""Clips at their own sample rate (include/fx.h, fx_set_clip_rates / fx_get_resampler_table) without a GPU: header, exports and binding
agree, the library's table is the formula's, the rate setter refuses bad arguments before any device use, the host model of a rated
tick (tests/resample_model.py) equals its own tap-by-tap loop and does not depend on how a stream is cut into ticks, and the
specification itself -- Z = 16, P = 512, beta = 9 -- resamples a sine as well as the issue that chose it measured."""
import ctypes
import functools
import os

import numpy as np
import pytest

import resample_model as rm
from signals import ulp_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("fx_set_clip_rates", "fx_get_resampler_table")
RATIOS = [147 / 160, 160 / 147, 2.0, 1.5, 1 / 8, 8.0]


@functools.lru_cache(maxsize=None)
def _table(fx):
    table, z, p = fx.capi.resampler_table()
    assert (z, p) == (rm.Z, rm.P)
    return table


def test_header_exports_and_binding_agree(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in text and name in fx.capi.EXPORTS and hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6 and "#define FX_ABI_VERSION 6" in text
    assert fx.capi.LAUNCH_KINDS[16] == "resample" and fx.capi.LAUNCH_KINDS[15] == "sources"
    kernels = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", "fx_kernels.h")).read()
    assert "FX_LAUNCH_RESAMPLE = 16" in kernels
    assert callable(fx.BatchAnalyser.set_clip_rates)
    assert "sample_rates" in fx.BatchAnalyser.create_clips.__code__.co_varnames
    assert (fx.capi.RESAMPLER_ZERO_CROSSINGS, fx.capi.RESAMPLER_PHASES) == (rm.Z, rm.P)
    # the shim's host units still know nothing of the unit
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    for source in build.HOST_SOURCES:
        body = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", source)).read()
        for name in ENTRIES:
            assert name not in body, (source, name)


def test_table_is_the_formula(fx):
    table, want = _table(fx), rm.table_formula()
    assert table.dtype == np.float32 and table.shape == (rm.TABLE_SIZE,) == want.shape
    # host libm and numpy may differ in the last fp64 bits of I0 and sinc: that moves an fp32 rounding by one step and no more
    assert int(ulp_distance(table, want).max()) <= 1
    assert table[0] == 1.0
    assert table[-2:].tobytes() == np.zeros(2, np.float32).tobytes()           # +0, both
    assert np.all(np.abs(table[1:]) < 1.0)
    # the zero crossings of the sinc: at whole multiples of P the entries are rounding noise
    assert np.all(np.abs(table[rm.P:rm.Z * rm.P:rm.P]) < 1e-15)


def test_table_entry_refuses_a_small_capacity(fx):
    lib = fx.load_library()
    INVALID = fx.capi.FX_ERR_INVALID_ARGUMENT
    fp = ctypes.POINTER(ctypes.c_float)
    guard = np.full(rm.TABLE_SIZE + 4, 7.0, np.float32)
    z, p = ctypes.c_int(0), ctypes.c_int(0)
    for capacity in (0, 1, rm.TABLE_SIZE - 1, -5):
        assert lib.fx_get_resampler_table(guard.ctypes.data_as(fp), capacity, ctypes.byref(z), ctypes.byref(p)) == INVALID
        assert b"capacity" in lib.fx_last_error() and np.all(guard == 7.0)
        assert (z.value, p.value) == (rm.Z, rm.P)                               # what a caller sizes its buffer by
    assert lib.fx_get_resampler_table(None, rm.TABLE_SIZE, None, None) == INVALID
    assert lib.fx_get_resampler_table(guard.ctypes.data_as(fp), rm.TABLE_SIZE, None, None) == fx.capi.FX_OK
    assert np.all(guard[rm.TABLE_SIZE:] == 7.0) and guard[0] == 1.0


def test_rate_setter_refuses_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID, OK = fx.capi.FX_ERR_INVALID_ARGUMENT, fx.capi.FX_OK
    ints = lambda *v: (ctypes.c_int * len(v))(*v)                               # noqa: E731
    rates = lambda *v: (ctypes.c_double * len(v))(*v)                           # noqa: E731
    # A zeroed block stands in for a context (no tracks, no banks): each refusal below comes before the entry touches a device.
    fake = ctypes.create_string_buffer(1 << 16)

    def refused(status, *why):
        assert status == INVALID, (status, why, lib.fx_last_error())
        for w in why:
            assert w in lib.fx_last_error(), (why, lib.fx_last_error())

    refused(lib.fx_set_clip_rates(None, ints(0), 1, rates(44100.0)), b"null context")
    refused(lib.fx_set_clip_rates(fake, ints(0), -1, rates(44100.0)), b"negative clip count")
    refused(lib.fx_set_clip_rates(fake, None, 2, rates(44100.0, 0.0)), b"null clip id list")
    refused(lib.fx_set_clip_rates(fake, ints(0, 1), 2, None), b"null sample rate list")
    refused(lib.fx_set_clip_rates(fake, ints(0), 1, rates(44100.0)), b"entry 0", b"unknown clip id 0")
    refused(lib.fx_set_clip_rates(fake, ints(-1), 1, rates(0.0)), b"entry 0", b"unknown clip id -1")
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -44100.0):
        refused(lib.fx_set_clip_rates(fake, ints(0, 1), 2, rates(48000.0, bad)), b"entry 1", b"sample rate")
    assert lib.fx_set_clip_rates(fake, None, 0, None) == OK                     # nothing to do is no error


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the binding used the library (%s) before refusing its arguments" % name)


def test_binding_refuses_before_any_library_use(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)
    an.num_channels, an.window_size, an.device, an._lib, an._h = 4, 1024, 0, _NoLibrary(), None
    with pytest.raises(ValueError, match="one sample rate per clip"):
        an.set_clip_rates([0, 1, 2], [44100.0, 48000.0])
    with pytest.raises(ValueError, match="one sample rate per clip"):
        an.create_clips(np.zeros(10, np.float32), lengths=[4, 6], sample_rates=[1.0, 2.0, 3.0])


def test_rate_params_are_the_hosts(fx):
    assert rm.rate_params(0, 48000.0) is None and rm.rate_params(48000.0, 48000.0) is None
    assert rm.rate_params(44100.0, 48000.0) == (44100.0 / 48000.0, 1.0, 16)
    assert rm.rate_params(96000.0, 48000.0) == (2.0, 0.5, 32)
    assert rm.rate_params(384000.0, 48000.0) == (8.0, 0.125, 128) and rm.rate_params(6000.0, 48000.0) == (0.125, 1.0, 16)
    r, rho, J = rm.rate_params(72000.0, 48000.0)
    assert (r, rho) == (1.5, 1.0 / 1.5) and J == int(np.ceil(16 / (1.0 / 1.5)))
    for bad in (48000.0 * 9, 48000.0 / 9, 5999.0):
        with pytest.raises(rm.Refused):
            rm.rate_params(bad, 48000.0)


def _samples(L, seed):
    return np.random.default_rng(seed).uniform(-1, 1, L).astype(np.float32)


def _player(L, r, loop, k=0, seed=None):
    rho = min(1.0, 1.0 / r)
    return rm.rated_player(_samples(L, L if seed is None else seed), r, rho, int(np.ceil(rm.Z / rho)), loop, k)


@pytest.mark.parametrize("r", RATIOS)
def test_model_equals_its_naive_loop(fx, r):
    T = _table(fx)
    for L in (1, 5, 7, 1000):
        for loop in (1, 0):
            # a one-shot starts where its end falls inside the tick, so that real taps, taps past the end and forced zeros all occur
            n = 24
            k = 0 if loop else max(0, int((L - 8 * r) / r))
            p, q = _player(L, r, loop, k), _player(L, r, loop, k)
            for tick in range(2):
                a, b = rm.render(p, n, T), rm.render_naive(q, n, T)
                assert a[0].dtype == np.float32 and a[0].shape == (n,)
                assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:], (r, L, loop, tick)
                (_, p.position, p.laps, p.state, p.k), (_, q.position, q.laps, q.state, q.k) = a, b
            assert loop or p.state == rm.FINISHED


@pytest.mark.parametrize("r", RATIOS)
def test_any_cut_into_ticks_gives_the_same_samples(fx, r):
    T = _table(fx)
    for L, loop in ((1000, 1), (7, 1), (1500, 0)):
        whole = rm.render(_player(L, r, loop), 2000, T)
        p, parts = _player(L, r, loop), []
        for n in (441, 1, 1558):
            out, p.position, p.laps, p.state, p.k = rm.render(p, n, T)
            parts.append(out)
        assert np.concatenate(parts).tobytes() == whole[0].tobytes()
        assert (p.position, p.laps, p.state) == whole[1:4]
        assert p.k == whole[4] or p.state == rm.FINISHED         # (a finished track's hidden k stops with it; PLAY sets it to 0)


def test_widening_is_the_load_stages():
    import interleave_model as im
    x = np.array([[0.0, 0.5, -0.5, 0.999, -1.0, 1e-3, 3.0517578125e-05]], np.float32)
    import clip_model as cm
    for fmt in cm.FORMATS:
        enc = im.encode(x, fmt)
        got = rm.widen(cm.raw(enc)[0], fmt)
        want = {"f32": x[0], "f16": x[0].astype(np.float16).astype(np.float32),
                "s16": np.clip(np.round(x[0] * 32768.0), -32768, 32767).astype(np.float32) / np.float32(32768.0),
                "s24": (np.clip(np.round(x[0].astype(np.float64) * 8388608.0), -8388608, 8388607) / 8388608.0).astype(np.float32)}[fmt]
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), fmt


def test_model_commands_set_k_as_the_contract_says(fx):
    T = _table(fx)
    m = rm.Model(3, T, 48000.0)
    clip = _samples(300, 3).view(np.uint8)
    m.load([0, 1], [clip, clip], [1, 0], ["f32", "f32"], [44100.0, 96000.0])
    assert m.players[0].rated and m.players[1].rated and (m.players[1].r, m.players[1].J) == (2.0, 32)
    m.set_sources([0, 1], [rm.FILE, rm.FILE])
    m.transport([0, 1], rm.PLAY)
    live = np.zeros((3, 100), np.float32)
    m.tick(live, 100)
    assert m.players[0].k == 100 and m.table()["position"][0] == int(np.floor(100 * (44100.0 / 48000.0)))
    m.transport([0], rm.PAUSE)
    assert m.players[0].k == 100 and not m.tick(live, 100)[0].any() and m.players[0].k == 100     # paused: silence, the phase kept
    m.transport([0], rm.PLAY)
    m.tick(live, 100)
    assert m.players[0].k == 200 and m.players[1].state == rm.FINISHED and m.table()["position"][1] == 300
    m.transport([1], rm.PLAY)                                                    # from FINISHED: from the top
    assert (m.players[1].k, m.players[1].position, m.players[1].state) == (0, 0, rm.PLAYING)
    m.transport([0], rm.RESTART)
    assert (m.players[0].k, m.players[0].position, m.players[0].state) == (0, 0, rm.PLAYING)
    m.tick(live[:, :10], 10)
    m.transport([0], rm.STOP)
    assert m.players[0].k == 0
    m.transport([0], rm.PLAY); m.tick(live[:, :10], 10)
    m.set_sources([0], [rm.INPUT])
    assert m.players[0].k == 0
    with pytest.raises(rm.Refused):
        m.load([2], [clip], None, ["f32"], [48000.0 * 9])
    assert m.players[2].clip is None
    m.load([0], [clip], None, ["f32"], [48000.0])                               # the context's own rate: not rated
    assert not m.players[0].rated


# ---- the quality of the specification: properties of Z, P and beta, not of any kernel ----
QUALITY = [(44100, 48000, 997), (44100, 48000, 15000), (48000, 44100, 997), (96000, 48000, 997), (22050, 48000, 5000),
           (48000, 16000, 3000), (192000, 48000, 997), (8000, 48000, 997)]


def _resampled_tone(T, source, target, tone, outputs=4800, k=1000):
    """a 0.5-amplitude sine in a one-second looping clip at `source` Hz, played into a context at `target` Hz: (rendered, ideal, clip)"""
    clip = (0.5 * np.sin(2.0 * np.pi * tone * np.arange(source, dtype=np.float64) / source)).astype(np.float32)
    r, rho, J = rm.rate_params(float(source), float(target))
    p = rm.rated_player(clip, r, rho, J, 1, k)
    out = rm.render(p, outputs, T)[0]
    x = (k + np.arange(outputs, dtype=np.float64)) * r
    return out.astype(np.float64), 0.5 * np.sin(2.0 * np.pi * tone * x / source), clip


@pytest.mark.parametrize("source,target,tone", QUALITY)
def test_a_resampled_sine_is_within_90_db_of_the_ideal(fx, source, target, tone):
    out, ideal, _ = _resampled_tone(_table(fx), source, target, tone)
    snr = 10.0 * np.log10(np.sum(ideal ** 2) / np.sum((out - ideal) ** 2))
    print("%d -> %d Hz, %d Hz tone: SNR %.1f dB" % (source, target, tone, snr))
    assert snr >= 90.0


def test_a_tone_above_the_new_nyquist_is_gone(fx):
    out, _, clip = _resampled_tone(_table(fx), 96000, 48000, 30000)
    level = 10.0 * np.log10(np.mean(out ** 2) / np.mean(clip.astype(np.float64) ** 2))
    print("30 kHz through 96k -> 48k: %.1f dB re input" % level)
    assert level <= -90.0
