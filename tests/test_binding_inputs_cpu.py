"""What the Python binding hands to the C ABI for every accepted input, and what it refuses, without a GPU: a BatchAnalyser made with
__new__ (no context) over a stand-in library that records the calls of fx_push_hops, fx_process_frames, fx_push_samples and
fx_push_interleaved.  Everything asserted through the public methods holds before and after the binding's input description
(analyser._describe_input) was gathered into one function; the tests named `..._describe_input...` hold that function itself."""
import ctypes

import numpy as np
import pytest

C, N = 3, 256
H = N // 2
SAMPLE_BYTES = {0: 4, 1: 2, 2: 2, 3: 3}          # FX_SAMPLE_F32, _F16, _S16, _S24
ENTRIES = ("push_hops", "process_frames", "push_samples", "push_interleaved")


def _null(p):
    return p is None or p.value is None


class _Recorder:
    """stands in for the library: the four analysis entries store what they were given (and the bytes behind the input pointer, read
    while the call holds them alive), write `frames` through frames_out and return FX_OK; fx_pending_samples returns `pending`"""

    def __init__(self, pending=0, frames=0):
        self.pending, self.frames, self.calls = pending, frames, []

    def _record(self, name, h, ptr, counts, samples, fmt, mem, raw, sm, frames_out=None):
        data = ctypes.string_at(ptr.value, samples * SAMPLE_BYTES[fmt]) if samples else b""
        self.calls.append(dict(name=name, h=h, counts=counts, fmt=fmt, mem=mem, raw_null=_null(raw), sm_null=_null(sm), data=data))
        if frames_out is not None:
            frames_out._obj.value = self.frames
        return 0

    def fx_push_hops(self, h, ptr, T, fmt, mem, raw, sm):
        return self._record("fx_push_hops", h, ptr, (T,), C * T * H, fmt, mem, raw, sm)

    def fx_process_frames(self, h, ptr, T, fmt, mem, raw, sm):
        return self._record("fx_process_frames", h, ptr, (T,), C * T * N, fmt, mem, raw, sm)

    def fx_push_samples(self, h, ptr, n, fmt, mem, raw, sm, frames_out):
        return self._record("fx_push_samples", h, ptr, (n,), C * n, fmt, mem, raw, sm, frames_out)

    def fx_push_interleaved(self, h, ptr, n, K, fmt, mem, raw, sm, frames_out):
        return self._record("fx_push_interleaved", h, ptr, (n, K), n * K, fmt, mem, raw, sm, frames_out)

    def fx_pending_samples(self, h):
        return self.pending


class _NoLibrary:
    """stands in for the library: any call into it fails the test"""
    def __getattr__(self, name):
        def used(*args):
            raise AssertionError("the binding called the library (%s) before refusing its input" % name)
        return used


def _analyser(fx, lib):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)          # no context
    an.num_channels, an.window_size, an.device, an._lib, an._h = C, N, 0, lib, None
    return an


def _shape(entry, T):
    """the input shape of `entry` that completes T hops from nothing pending (in samples: s24 triples the last axis)"""
    return {"push_hops": (C, T, H), "process_frames": (C, T, N), "push_samples": (C, T * H), "push_interleaved": (T * H, C)}[entry]


def _floats(shape, seed=0):
    return (np.random.default_rng(seed).standard_normal(shape) * 0.25).astype(np.float32)


def _s24(fx, shape, seed=0):
    return fx.analyser.pack_s24(np.random.default_rng(seed).integers(-(1 << 23), 1 << 23, shape, dtype=np.int32))


def _forms(fx, shape):
    """(name, input, sample_format, expected format code, expected bytes) of every accepted numpy form of one block"""
    capi = fx.capi
    f32 = _floats(shape)
    f64 = _floats(shape, 1).astype(np.float64) + 1e-12
    i32 = np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape) % 7 - 3
    s16 = (f32 * 32768).astype(np.int16)
    packed = _s24(fx, shape)
    plain = np.array(packed.view(np.ndarray))                 # the same bytes, untagged
    wide = _floats(shape[:-1] + (2 * shape[-1],), 2)
    view = wide[..., ::2]
    assert not view.flags.c_contiguous and type(plain) is np.ndarray
    return [("float32", f32, None, capi.SAMPLE_F32, f32.tobytes()),
            ("float32 named", f32, "f32", capi.SAMPLE_F32, f32.tobytes()),
            ("float64", f64, None, capi.SAMPLE_F32, f64.astype(np.float32).tobytes()),
            ("int32", i32, None, capi.SAMPLE_F32, i32.astype(np.float32).tobytes()),
            ("float16", f32.astype(np.float16), None, capi.SAMPLE_F16, f32.astype(np.float16).tobytes()),
            ("int16", s16, None, capi.SAMPLE_S16, s16.tobytes()),
            ("int16 named", s16, "s16", capi.SAMPLE_S16, s16.tobytes()),
            ("PackedS24", packed, None, capi.SAMPLE_S24, packed.tobytes()),
            ("uint8 named s24", plain, "s24", capi.SAMPLE_S24, plain.tobytes()),
            ("non-contiguous view", view, None, capi.SAMPLE_F32, np.ascontiguousarray(view).tobytes())]


@pytest.mark.parametrize("entry", ENTRIES)
def test_accepted_numpy_inputs_reach_the_library_as_described(fx, entry):
    T = 2
    for name, x, sample_format, fmt, data in _forms(fx, _shape(entry, T)):
        lib = _Recorder(pending=0, frames=T)
        an = _analyser(fx, lib)
        raw, sm = getattr(an, entry)(x, sample_format=sample_format)
        assert len(lib.calls) == 1, name
        call = lib.calls[0]
        assert call["name"] == "fx_" + entry and call["h"] is None, name
        assert call["fmt"] == fmt and call["mem"] == fx.capi.MEM_HOST, name
        assert call["counts"] == {"push_hops": (T,), "process_frames": (T,), "push_samples": (T * H,), "push_interleaved": (T * H, C)}[entry], name
        assert call["data"] == data, name
        assert not call["raw_null"] and not call["sm_null"], name
        for r in (raw, sm):
            assert isinstance(r, np.ndarray) and r.dtype == np.float32 and r.shape == (C, T, 12) and r.flags.c_contiguous, name


@pytest.mark.parametrize("entry", ENTRIES)
def test_want_flags_decide_which_result_pointers_are_null(fx, entry):
    x = _floats(_shape(entry, 1))
    for want_raw, want_smoothed in ((True, True), (True, False), (False, True), (False, False)):
        lib = _Recorder(frames=1)
        raw, sm = getattr(_analyser(fx, lib), entry)(x, want_raw=want_raw, want_smoothed=want_smoothed)
        assert (lib.calls[0]["raw_null"], lib.calls[0]["sm_null"]) == (not want_raw, not want_smoothed)
        assert (raw is None, sm is None) == (not want_raw, not want_smoothed)
        for r in (raw, sm):
            assert r is None or r.shape == (C, 1, 12)


@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_length_blocks(fx, entry):
    lib = _Recorder(pending=100, frames=0)
    raw, sm = getattr(_analyser(fx, lib), entry)(np.zeros(_shape(entry, 0), np.float32))
    call = lib.calls[0]
    assert call["counts"][0] == 0 and call["fmt"] == fx.capi.SAMPLE_F32 and call["mem"] == fx.capi.MEM_HOST and call["data"] == b""
    assert raw.shape == (C, 0, 12) and sm.shape == (C, 0, 12) and raw.dtype == np.float32
    if entry == "push_interleaved":
        assert call["counts"] == (0, C)
    if entry in ("push_samples", "push_interleaved"):
        assert call["raw_null"] and call["sm_null"]


def test_a_block_that_completes_no_hop_gives_empty_results_and_null_pointers(fx):
    """pending 100 + 27 samples < a hop of 128: raw [C][0][12], and the library is given no result pointer"""
    for entry, x in (("push_samples", _floats((C, 27))), ("push_interleaved", _floats((27, C)))):
        lib = _Recorder(pending=100, frames=0)
        raw, sm = getattr(_analyser(fx, lib), entry)(x)
        call = lib.calls[0]
        assert call["counts"][0] == 27 and call["raw_null"] and call["sm_null"] and call["data"] == x.tobytes()
        assert raw.shape == (C, 0, 12) and sm.shape == (C, 0, 12)
    # one sample more completes the hop: a frame, and pointers
    lib = _Recorder(pending=100, frames=1)
    raw, sm = _analyser(fx, lib).push_samples(_floats((C, 28)))
    assert raw.shape == (C, 1, 12) and not lib.calls[0]["raw_null"] and not lib.calls[0]["sm_null"]
    # pending samples count towards the frames of a long block too
    lib = _Recorder(pending=100, frames=3)
    raw, sm = _analyser(fx, lib).push_interleaved(_floats((2 * H + 28, C)), want_smoothed=False)
    assert raw.shape == (C, 3, 12) and sm is None and lib.calls[0]["counts"] == (2 * H + 28, C)


def test_interleaved_source_channel_counts(fx):
    """K is the last axis of a 2-D block (a third of it for s24) or num_source_channels; it need not be the track count"""
    K = 5
    x = _floats((40, K))
    lib = _Recorder(frames=0)
    an = _analyser(fx, lib)
    an.push_interleaved(x)
    an.push_interleaved(x.ravel(), num_source_channels=K)
    an.push_interleaved(_s24(fx, (40, K)))
    an.push_interleaved(np.array(_s24(fx, (40, K)).view(np.ndarray)).ravel(), sample_format="s24", num_source_channels=K)
    assert [c["counts"] for c in lib.calls] == [(40, K)] * 4
    assert [c["fmt"] for c in lib.calls] == [fx.capi.SAMPLE_F32] * 2 + [fx.capi.SAMPLE_S24] * 2
    assert lib.calls[0]["data"] == lib.calls[1]["data"] == x.tobytes() and len(lib.calls[2]["data"]) == 40 * K * 3


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_come_before_any_use_of_the_library(fx, entry):
    call = getattr(_analyser(fx, _NoLibrary()), entry)
    shape = _shape(entry, 1)
    with pytest.raises(ValueError, match="uint8"):
        call(np.zeros(shape[:-1] + (3 * shape[-1],), np.uint8))                   # never s24 on dtype alone
    with pytest.raises(ValueError, match="does not describe"):
        call(np.zeros(shape, np.float32), sample_format="s16")
    with pytest.raises(ValueError, match="does not describe"):
        call(np.zeros(shape, np.int16), sample_format="s24")
    with pytest.raises(ValueError, match="does not describe"):
        call(_s24(fx, shape), sample_format="f32")
    with pytest.raises(ValueError, match="sample_format must be one of f16, f32, s16, s24"):
        call(np.zeros(shape, np.float32), sample_format="s32")
    with pytest.raises(ValueError, match="not a multiple"):
        call(np.zeros(int(np.prod(shape)) + 1, np.float32), **({"num_source_channels": C} if entry == "push_interleaved" else {}))
    with pytest.raises(ValueError, match="not a multiple"):                        # whole frames of bytes, but not of 3-byte samples
        call(np.zeros(C * (H if entry == "push_hops" else N if entry == "process_frames" else 4), np.uint8), sample_format="s24",
             **({"num_source_channels": C} if entry == "push_interleaved" else {}))


def test_interleaved_dims_and_its_refusals_through_push_interleaved(fx):
    dims = fx.analyser.interleaved_dims
    S16, S24 = fx.capi.SAMPLE_S16, fx.capi.SAMPLE_S24
    assert dims((480, 6), 480 * 6, S16) == (480, 6)
    assert dims((480, 18), 480 * 18, S24) == (480, 6)
    assert dims((2880,), 2880, S16, 6) == (480, 6)
    assert dims((0, 6), 0, S16) == (0, 6)
    an = _analyser(fx, _NoLibrary())
    for match, shape, dtype, kw in (("multiple of 3", (480, 10), np.uint8, {"sample_format": "s24"}),
                                    ("not a multiple", (2881,), np.int16, {"num_source_channels": 6}),
                                    ("not a multiple", (30,), np.uint8, {"sample_format": "s24", "num_source_channels": 4}),
                                    ("num_source_channels", (2880,), np.float32, {}),
                                    ("at least one", (2880,), np.float32, {"num_source_channels": 0})):
        with pytest.raises(ValueError, match=match):
            an.push_interleaved(np.zeros(shape, dtype), **kw)
        with pytest.raises(ValueError, match=match):
            dims(shape, int(np.prod(shape)), S24 if dtype == np.uint8 else S16, kw.get("num_source_channels"))


def test_a_cpu_tensor_is_refused(fx):
    import torch
    an = _analyser(fx, _NoLibrary())
    for entry in ENTRIES:
        with pytest.raises(ValueError):
            getattr(an, entry)(torch.zeros(_shape(entry, 1)))
    for entry in ("push_hops", "process_frames"):
        with pytest.raises(ValueError, match="must live on the GPU"):
            getattr(an, entry)(torch.zeros(_shape(entry, 1)))


def test_a_frames_out_that_disagrees_fails_the_call(fx):
    """the library reports another frame count than (pending + n) // (N/2): an AssertionError, not a result of the wrong shape"""
    for entry, x in (("push_samples", _floats((C, H))), ("push_interleaved", _floats((H, C)))):
        with pytest.raises(AssertionError):
            getattr(_analyser(fx, _Recorder(pending=0, frames=2)), entry)(x)
        with pytest.raises(AssertionError):
            getattr(_analyser(fx, _Recorder(pending=100, frames=1)), entry)(x[..., :27] if entry == "push_samples" else x[:27])
        raw, _ = getattr(_analyser(fx, _Recorder(pending=0, frames=1)), entry)(x)
        assert raw.shape == (C, 1, 12)


# ---- the one description of an input (new with the function) ----
def test_describe_input_numpy(fx):
    describe, capi = fx.analyser._describe_input, fx.capi
    for name, x, sample_format, fmt, data in _forms(fx, (C, 2, H)):
        ptr, got_fmt, mem, count, keep, device = describe(x, sample_format, 0)
        assert isinstance(ptr, ctypes.c_void_p) and got_fmt == fmt and mem == capi.MEM_HOST and device is None, name
        assert count == C * 2 * H, name                                            # samples, not bytes: a third of the bytes of s24
        assert isinstance(keep, np.ndarray) and keep.flags.c_contiguous and keep.ctypes.data == ptr.value, name
        assert ctypes.string_at(ptr.value, len(data)) == data, name
    f32 = _floats((C, H))
    assert describe(f32, None, 0)[4] is f32                                        # no copy of what is already right
    assert describe(np.zeros((C, 0), np.int16), None, 0)[3] == 0
    for x, sample_format, match in ((np.zeros(6, np.uint8), None, "uint8"), (f32, "s16", "does not describe a float32 array"),
                                    (f32, "wav", "sample_format must be one of"), (np.zeros(7, np.uint8), "s24", "not a multiple of 3")):
        with pytest.raises(ValueError, match=match):
            describe(x, sample_format, 0)


def test_describe_input_refuses_a_cpu_tensor_for_every_entry_point(fx):
    import torch
    with pytest.raises(ValueError, match="must live on the GPU"):
        fx.analyser._describe_input(torch.zeros(C, H), None, 0)
    an = _analyser(fx, _NoLibrary())
    for entry in ENTRIES:
        with pytest.raises(ValueError, match="must live on the GPU"):
            getattr(an, entry)(torch.zeros(_shape(entry, 1)))


def test_hop_stream_takes_its_formats_from_the_same_table(fx):
    class _Stream:
        def fx_stream_create(self, h, hops, slots, fmt, out):
            self.fmt = fmt
            return 0
    for dtype, fmt in ((np.float32, fx.capi.SAMPLE_F32), (np.float16, fx.capi.SAMPLE_F16), (np.int16, fx.capi.SAMPLE_S16), (np.uint8, fx.capi.SAMPLE_S24)):
        an = _analyser(fx, _Stream())
        s = fx.analyser.HopStream(an, 4, dtype=dtype)
        assert an._lib.fmt == fmt and s._shape == (C, 4, H * (3 if dtype == np.uint8 else 1))
        s._h = None
    with pytest.raises(ValueError, match="HopStream samples are float32, float16, int16"):
        fx.analyser.HopStream(_analyser(fx, _NoLibrary()), 4, dtype=np.float64)


# ---- capi: one prototype table ----
def test_every_export_has_a_prototype_and_the_library_carries_it(fx):
    capi = fx.capi
    names = [p[0] for p in capi.PROTOTYPES]
    assert names == capi.EXPORTS and len(set(names)) == len(names)
    internal = [p[0] for p in capi.INTERNAL_PROTOTYPES]
    assert internal == ["fx_set_tuning_internal", "fx_last_launches_internal"] and not set(internal) & set(names)
    lib = fx.load_library()
    for name, argtypes, restype in capi.PROTOTYPES + capi.INTERNAL_PROTOTYPES:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype, name
    default = ctypes.CDLL(None).getpid.restype                                     # ctypes' default restype: int
    for name, _, restype in capi.PROTOTYPES:
        if name in ("fx_tuning_defaults", "fx_tuning_from_env", "fx_pack_osc12", "fx_pack_osc10"):
            assert restype is None, name
        elif name == "fx_last_error":
            assert restype is ctypes.c_char_p
        else:
            assert restype is default, name


def test_the_internal_entries_are_bound_once_at_load(fx):
    lib = fx.load_library()
    an = _analyser(fx, lib)                                   # a null context: both entries refuse it, after the binding did its part
    hooks, launches = lib.fx_set_tuning_internal, lib.fx_last_launches_internal
    before = (hooks.argtypes, launches.argtypes)
    assert before[0] is not None and before[1] is not None
    with pytest.raises(fx.FxError):
        an.set_test_hooks(0)
    assert an.last_launches() == []                           # a zero-launch record
    assert lib.fx_set_tuning_internal.argtypes is before[0] and lib.fx_last_launches_internal.argtypes is before[1]
