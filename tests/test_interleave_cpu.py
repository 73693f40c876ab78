"""Interleaved input through a channel map (include/fx.h, fx_set_channel_map / fx_push_interleaved) without a GPU: the C ABI declares
and exports both entries, they refuse bad arguments before any device use, the Python binding refuses blocks that are not whole
frames, the launch record knows the de-interleave, and the host model of the planar block is the byte-level definition."""
import ctypes
import os

import numpy as np
import pytest

import interleave_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entries(fx):
    text = open(os.path.join(ROOT, "include", "fx.h")).read().replace(" (", "(")
    lib = fx.load_library()
    for name in ("fx_set_channel_map", "fx_push_interleaved"):
        assert name + "(" in text
        assert name in fx.capi.EXPORTS
        assert hasattr(lib, name)
    assert fx.capi.ABI_VERSION == 6 and lib.fx_abi_version() == 6


def test_launch_kind_of_the_deinterleave(fx):
    assert fx.capi.LAUNCH_KINDS[10] == "deinterleave"
    text = open(os.path.join(ROOT, "feature-extractor_amd", "csrc", "fx_kernels.h")).read()
    assert "FX_LAUNCH_TAPS, FX_LAUNCH_DEINTERLEAVE }" in text


def test_entries_refuse_bad_arguments_before_device_use(fx):
    lib = fx.load_library()
    INVALID = fx.capi.FX_ERR_INVALID_ARGUMENT
    m = (ctypes.c_int * 4)(0, 1, 2, 3)
    buf = (ctypes.c_float * 64)()
    got = ctypes.c_int(7)
    assert lib.fx_set_channel_map(None, m) == INVALID
    assert b"null context" in lib.fx_last_error()
    assert lib.fx_push_interleaved(None, buf, 4, 4, fx.capi.SAMPLE_F32, fx.capi.MEM_HOST, None, None, ctypes.byref(got)) == INVALID
    assert b"null context" in lib.fx_last_error() and got.value == 0
    # A zeroed block stands in for a context: each refusal below comes before the entry reads any field of it or touches a device.
    fake = ctypes.create_string_buffer(1 << 16)
    cases = [((buf, -1, 4, fx.capi.SAMPLE_F32, fx.capi.MEM_HOST), b"negative sample count"),
             ((buf, 4, 0, fx.capi.SAMPLE_F32, fx.capi.MEM_HOST), b"source channels"),
             ((buf, 4, -2, fx.capi.SAMPLE_F32, fx.capi.MEM_HOST), b"source channels"),
             ((buf, 4, 4, 99, fx.capi.MEM_HOST), b"unknown sample format"),
             ((buf, 4, 4, fx.capi.SAMPLE_F32, 7), b"unknown memory kind"),
             ((None, 4, 4, fx.capi.SAMPLE_F32, fx.capi.MEM_HOST), b"null input buffer"),
             ((ctypes.c_void_p(ctypes.addressof(buf) + 2), 4, 4, fx.capi.SAMPLE_F32, fx.capi.MEM_DEVICE), b"4-byte aligned")]
    for args, why in cases:
        got.value = 7
        assert lib.fx_push_interleaved(fake, *args, None, None, ctypes.byref(got)) == INVALID, why
        assert why in lib.fx_last_error() and got.value == 0, (why, lib.fx_last_error())
    # nothing to do is no error
    assert lib.fx_push_interleaved(fake, buf, 0, 4, fx.capi.SAMPLE_F32, fx.capi.MEM_HOST, None, None, None) == fx.capi.FX_OK


def test_binding_refuses_blocks_of_partial_frames(fx):
    dims = fx.analyser.interleaved_dims
    S16, S24 = fx.capi.SAMPLE_S16, fx.capi.SAMPLE_S24
    assert dims((480, 6), 480 * 6, S16) == (480, 6)
    assert dims((480, 18), 480 * 18, S24) == (480, 6)
    assert dims((2880,), 2880, S16, 6) == (480, 6)
    assert dims((0, 6), 0, S16) == (0, 6)
    with pytest.raises(ValueError, match="multiple of 3"):
        dims((480, 10), 4800, S24)
    with pytest.raises(ValueError, match="not a multiple"):
        dims((2881,), 2881, S16, 6)
    with pytest.raises(ValueError, match="not a multiple"):
        dims((30,), 30, S24, 4)
    with pytest.raises(ValueError, match="num_source_channels"):
        dims((2880,), 2880, S16)
    with pytest.raises(ValueError, match="at least one"):
        dims((2880,), 2880, S16, 0)


class _NoLibrary:
    """stands in for the library: any use of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("push_interleaved used the library (%s) before refusing the block" % name)


def test_push_interleaved_refuses_partial_frames_before_device_use(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)          # no context: the refusals come first
    an.num_channels, an.window_size, an.device, an._lib, an._h = 4, 1024, 0, _NoLibrary(), None
    with pytest.raises(ValueError, match="multiple of 3"):
        an.push_interleaved(np.zeros((480, 10), np.uint8), sample_format="s24")
    with pytest.raises(ValueError, match="not a multiple"):
        an.push_interleaved(np.zeros(2881, np.int16), num_source_channels=6)
    with pytest.raises(ValueError, match="not a multiple"):
        an.push_interleaved(np.zeros(30, np.uint8), sample_format="s24", num_source_channels=4)
    with pytest.raises(ValueError, match="num_source_channels"):
        an.push_interleaved(np.zeros(2880, np.float32))
    with pytest.raises(ValueError, match="at least one"):
        an.push_interleaved(np.zeros(2880, np.float32), num_source_channels=0)


@pytest.mark.parametrize("fmt", im.FORMATS)
def test_model_is_the_byte_level_definition(fmt):
    rng = np.random.default_rng(3)
    for C, K, n in [(5, 5, 7), (4, 7, 13), (6, 12, 1), (3, 1, 9)]:
        sources = rng.standard_normal((K, n)).astype(np.float32) * 0.3
        block = im.interleave(sources, fmt)
        bps = 3 if fmt == "s24" else block.itemsize
        assert block.shape == ((n, 3 * K) if fmt == "s24" else (n, K))
        # the interleaved block holds source k's samples at frame i, sample k
        enc = im.encode(sources, fmt)
        assert im.planar_bytes(block.tobytes(), n, K, range(K), bps) == enc.tobytes()
        kinds = im.maps(C, K, seed=C + K) if K >= C else {"all from one source": np.zeros(C, np.int64)}
        for name, cmap in kinds.items():
            assert len(cmap) == C and cmap.min() >= 0 and cmap.max() < K, name
            got = im.planar(block, cmap, fmt)
            assert got.dtype == block.dtype and got.flags.c_contiguous
            assert got.tobytes() == im.planar_bytes(block.tobytes(), n, K, cmap, bps), (fmt, C, K, name)


def test_s24_packing_is_little_endian_twos_complement():
    x = np.array([[0.5, -0.5, 1.0 / 8388608.0, -1.0]], np.float32)
    b = im.encode(x, "s24").reshape(-1, 3)
    v = b[:, 0].astype(np.int32) | (b[:, 1].astype(np.int32) << 8) | (b[:, 2].astype(np.int32) << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    assert list(v) == [4194304, -4194304, 1, -8388608]


def test_maps_cover_the_kinds():
    m = im.maps(8, 16)
    assert list(m["identity"]) == list(range(8)) and list(m["reversed"]) == list(range(8))[::-1]
    assert len(set(m["random"])) < 8
    assert list(m["strided"]) == list(range(0, 16, 2))
