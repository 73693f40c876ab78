"""The Python binding's device inputs on the GPU: what it refuses of a tensor it refuses before the context sees anything; host and
device input of the same samples give the same bits through every entry point and sample format; calls made on the library's
stream give what calls on torch's default stream give."""
import numpy as np
import pytest

import interleave_model as im
import signals

pytestmark = pytest.mark.gpu

C, N, T = 2, 256, 3
H = N // 2
ENTRIES = ("push_hops", "process_frames", "push_samples", "push_interleaved")
CUTS = (0, 200, T * H)                      # the block entry points get the stream in two blocks: 200 samples stay partly pending


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def hops():
    x = (signals.loud_noise(C, T, N) * 0.2).astype(np.float32)
    x.setflags(write=False)
    return x


def _torch(x):
    import torch
    return torch.from_numpy(np.array(x, order="C")).cuda()           # (a copy: the shared fixture is read-only)


def _host(r):
    return r.cpu().numpy() if hasattr(r, "cpu") else r


def _inputs(entry, hops, fmt):
    """the three hops as the calls `entry` takes them in, encoded in `fmt` (s24: uint8, the last axis three times as long)"""
    if entry == "push_hops":
        return [im.encode(hops, fmt)]
    if entry == "process_frames":
        prev = np.concatenate([np.zeros((C, 1, H), np.float32), hops[:, :-1]], axis=1)
        return [im.encode(np.concatenate([prev, hops], axis=2), fmt)]
    flat = hops.reshape(C, T * H)
    if entry == "push_samples":
        return [im.encode(flat[:, a:b], fmt) for a, b in zip(CUTS, CUTS[1:])]
    return [im.interleave(flat[:, a:b], fmt) for a, b in zip(CUTS, CUTS[1:])]


def _feed(an, entry, blocks, fmt, device, **kw):
    sf = "s24" if fmt == "s24" else None
    out = [getattr(an, entry)(_torch(b) if device else b, sample_format=sf, **kw) for b in blocks]
    return [np.concatenate([_host(o[k]) for o in out], axis=1) for k in (0, 1)]


@pytest.mark.parametrize("fmt", im.FORMATS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_host_and_device_input_give_the_same_bits(gpu_fx, hops, entry, fmt):
    blocks = _inputs(entry, hops, fmt)
    want = _feed(gpu_fx.BatchAnalyser(C, N), entry, blocks, fmt, device=False)
    got = _feed(gpu_fx.BatchAnalyser(C, N), entry, blocks, fmt, device=True)
    assert want[0].shape == (C, T, 12) and np.isfinite(want[1]).any()
    assert same(got[0], want[0]) and same(got[1], want[1])


@pytest.mark.parametrize("entry", ["push_hops", "process_frames"])
def test_caller_provided_result_tensors_are_the_results(gpu_fx, hops, entry):
    import torch
    blocks = _inputs(entry, hops, "f32")
    want = _feed(gpu_fx.BatchAnalyser(C, N), entry, blocks, "f32", device=False)
    r = torch.full((C, T, 12), -7.0, dtype=torch.float32, device="cuda")
    s = torch.full((C, T, 12), -7.0, dtype=torch.float32, device="cuda")
    raw, sm = getattr(gpu_fx.BatchAnalyser(C, N), entry)(_torch(blocks[0]), out_raw=r, out_smoothed=s)
    assert raw is r and sm is s
    assert same(r.cpu().numpy(), want[0]) and same(s.cpu().numpy(), want[1])


def _offset_view(x, items):
    """the values of x in a tensor that starts `items` elements into its allocation"""
    import torch
    flat = _torch(x).reshape(-1)
    view = torch.zeros(x.size + items, dtype=flat.dtype, device="cuda")[items:]
    view.copy_(flat)
    return view.reshape(x.shape)


def test_device_inputs_are_refused_before_the_context_sees_them(gpu_fx, hops):
    import torch
    an, fresh = gpu_fx.BatchAnalyser(C, N), gpu_fx.BatchAnalyser(C, N)
    got = [an.push_hops(_torch(hops[:, :1]))]
    state = (an.pending_samples(), an.channel_frames().copy())
    assert state[0] == 0 and list(state[1]) == [1] * C
    shapes = {"push_hops": (C, 1, H), "process_frames": (C, 1, N), "push_samples": (C, H), "push_interleaved": (H, C)}

    def refused(match, call, *args, **kw):
        with pytest.raises(ValueError, match=match):
            call(*args, **kw)
        assert an.pending_samples() == state[0] and np.array_equal(an.channel_frames(), state[1]), match

    for entry in ("push_hops", "process_frames"):             # a view 4 bytes into an allocation: not the 16-byte boundary whole hops need
        v = _offset_view(np.ones(shapes[entry], np.float32), 1)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        refused("16-byte boundary", getattr(an, entry), v)
    for entry in ("push_samples", "push_interleaved"):        # ... a block needs 4 bytes: 2 bytes into an int16 allocation is refused
        v = _offset_view(np.ones(shapes[entry], np.int16), 1)
        assert v.is_contiguous() and v.data_ptr() % 4 == 2
        refused("4-byte boundary", getattr(an, entry), v)
    for entry in ENTRIES:
        shape = shapes[entry]
        refused("contiguous", getattr(an, entry), torch.zeros(shape[::-1], device="cuda").permute(*range(len(shape))[::-1]))
        refused("float32, float16, int16", getattr(an, entry), torch.zeros(shape, dtype=torch.float64, device="cuda"))
        refused('sample_format="s24"', getattr(an, entry), torch.zeros(shape[:-1] + (3 * shape[-1],), dtype=torch.uint8, device="cuda"))
    for entry in ("push_hops", "process_frames"):
        x = torch.zeros(shapes[entry], device="cuda")
        refused("out_raw must be", getattr(an, entry), x, out_raw=torch.empty((C, 2, 12), device="cuda"))
        refused("out_smoothed must be", getattr(an, entry), x, out_smoothed=torch.empty((C, 1, 11), device="cuda"))
    # the context is what it was: the rest of the stream gives what a context gives that never met a refusal
    got.append(an.push_hops(_torch(hops[:, 1:])))
    want = fresh.push_hops(hops)
    for k in (0, 1):
        assert same(np.concatenate([_host(g[k]) for g in got], axis=1), want[k]), k
    assert same(an.get_features(), fresh.get_features())


def test_a_block_may_start_on_any_4_byte_boundary(gpu_fx, hops):
    """the view push_hops refuses (4 bytes into its allocation) is a legal device block for push_samples and push_interleaved"""
    flat = hops.reshape(C, T * H)
    for entry, block in (("push_samples", flat), ("push_interleaved", np.ascontiguousarray(flat.T))):
        v = _offset_view(block, 1)
        assert v.data_ptr() % 16 == 4
        want = getattr(gpu_fx.BatchAnalyser(C, N), entry)(block)
        got = getattr(gpu_fx.BatchAnalyser(C, N), entry)(v)
        assert want[0].shape == (C, T, 12) and same(_host(got[0]), want[0]) and same(_host(got[1]), want[1])


@pytest.mark.parametrize("entry", ["push_samples", "push_interleaved"])
def test_blocks_on_the_library_stream_give_the_same_bits(gpu_fx, hops, entry):
    import torch
    blocks = _inputs(entry, hops, "f32")
    want = _feed(gpu_fx.BatchAnalyser(C, N), entry, blocks, "f32", device=True)
    an = gpu_fx.BatchAnalyser(C, N)
    with torch.cuda.stream(an.torch_stream()):
        assert torch.cuda.current_stream().cuda_stream == an.torch_stream().cuda_stream
        out = [getattr(an, entry)((_torch(b) * 1.0).contiguous()) for b in blocks]       # produced on the library's stream, right before the call
        got = [np.concatenate([_host(o[k]) for o in out], axis=1) for k in (0, 1)]
    assert same(got[0], want[0]) and same(got[1], want[1])
