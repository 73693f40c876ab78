"""fx_set_channel_map / fx_push_interleaved on the GPU: every result equals, bit for bit, a twin context fed fx_push_samples with the
planar block the map makes of each interleaved block (tests/interleave_model.py) -- raw, smoothed, frames, pending samples and the
latest features -- and the call's launches are the de-interleave followed by the twin's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import interleave_model as im
import signals

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = [1, 63, 441, 480, 512, 1000, 4097]
NS = [256, 1024, 2048, 4096]
KS = ["C", "C+3", "2C"]
MAPS = ["identity", "reversed", "random", "strided"]
# every (format, block) pair once; window size, memory kind, K and map walk their own cycles, so each value of each axis is met
CASES = [(NS[i % 4], fmt, bool(i % 2), block, KS[i % 3], MAPS[(i // 2) % 4])
         for i, (fmt, block) in enumerate((f, b) for f in im.FORMATS for b in BLOCKS)]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _k(kind, C):
    return {"C": C, "C+3": C + 3, "2C": 2 * C}[kind]


def _sources(K, N, total, seed):
    H = N // 2
    T = -(-total // H)
    return signals.tone_vibrato_noise(K, T, N, seed=seed).reshape(K, -1)[:, :total].astype(np.float32)


def _torch(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(r):
    return None if r is None else (r.cpu().numpy() if hasattr(r, "cpu") else r)


def _pair(gpu_fx, C, N, cmap):
    an, twin = gpu_fx.BatchAnalyser(C, N), gpu_fx.BatchAnalyser(C, N)
    for a in (an, twin):
        a.set_gain(0.75)
    if cmap is not None:
        an.set_channel_map(cmap)
    return an, twin


def _step(an, twin, block, cmap, fmt, device):
    """one interleaved block into `an`, its planar form into `twin`; every output compared"""
    sf = "s24" if fmt == "s24" else None
    pl = im.planar(block, cmap, fmt)
    got = an.push_interleaved(_torch(block) if device else block, sample_format=sf)
    want = twin.push_samples(_torch(pl) if device else pl, sample_format=sf)
    g, w = [_host(x) for x in got], [_host(x) for x in want]
    assert g[0].shape == w[0].shape and same(g[0], w[0]) and same(g[1], w[1])
    assert an.pending_samples() == twin.pending_samples()
    return g[0].shape[1]


def _feed(an, twin, sources, block_len, cmap, fmt, device):
    K, total = sources.shape
    block = im.interleave(sources, fmt)
    frames = 0
    for at in range(0, total, block_len):
        frames += _step(an, twin, np.ascontiguousarray(block[at:at + block_len]), cmap, fmt, device)
    assert same(an.get_features(), twin.get_features())
    return frames


@pytest.mark.parametrize("N,fmt,device,block,kkind,mapkind", CASES)
def test_interleaved_blocks_equal_the_planar_twin(gpu_fx, N, fmt, device, block, kkind, mapkind):
    C = 70 if block in (441, 4097) else 6             # (70 tracks: two workgroups of tracks, one of them partial)
    K = _k(kkind, C)
    cmap = im.maps(C, K, seed=N + block)[mapkind]
    H = N // 2
    total = H + 5 if block == 1 else 3 * H + 77
    sources = _sources(K, N, total, seed=block)
    an, twin = _pair(gpu_fx, C, N, None if mapkind == "identity" else cmap)
    frames = _feed(an, twin, sources, block, cmap, fmt, device)
    assert frames == total // H
    an.close(); twin.close()


@pytest.mark.parametrize("fmt", ["s16", "s24", "f32"])
def test_blocks_at_the_tiles_seams(gpu_fx, fmt):
    """65 tracks and 65 samples: the smallest shape with a second workgroup in tracks (one row of its tile) and a second in positions
    (one sample), after a block of exactly one tile's 64 samples; every byte width the tile carries"""
    C = K = 65
    N = 256                                           # (the smallest window: the analysis behind the blocks is cheap)
    cmap = im.maps(C, K, seed=65)["reversed"]
    block = im.interleave(_sources(K, N, 64 + 65, seed=65), fmt)
    an, twin = _pair(gpu_fx, C, N, cmap)
    frames = _step(an, twin, np.ascontiguousarray(block[:64]), cmap, fmt, True)
    frames += _step(an, twin, np.ascontiguousarray(block[64:]), cmap, fmt, True)
    assert frames == (64 + 65) // (N // 2)
    assert same(an.get_features(), twin.get_features())
    an.close(); twin.close()


def test_interleaved_and_planar_calls_alternate(gpu_fx):
    C, K, N = 5, 9, 1024
    cmap = im.maps(C, K, seed=1)["random"]
    src = _sources(K, N, 6000, seed=11)
    block = im.interleave(src, "f32")
    an, twin = _pair(gpu_fx, C, N, cmap)
    at, i = 0, 0
    for n in [480, 441, 1000, 63, 512, 2000, 1]:
        piece = np.ascontiguousarray(block[at:at + n])
        pl = im.planar(piece, cmap, "f32")
        if i % 2:
            g, w = an.push_samples(pl), twin.push_samples(pl)
            assert same(g[0], w[0]) and same(g[1], w[1])
        else:
            _step(an, twin, piece, cmap, "f32", device=bool(i % 4))
        at += n; i += 1
    assert an.pending_samples() == twin.pending_samples() and same(an.get_features(), twin.get_features())


@pytest.mark.parametrize("device", [False, True])
def test_map_change_mid_stream_switches_source_at_the_block_boundary(gpu_fx, device):
    C, K, N = 6, 8, 1024
    src = _sources(K, N, 5000, seed=5)
    block = im.interleave(src, "s16")
    first, second = im.maps(C, K, seed=2)["reversed"], im.maps(C, K, seed=3)["random"]
    an, twin = _pair(gpu_fx, C, N, first)
    _step(an, twin, np.ascontiguousarray(block[:700]), first, "s16", device)
    assert an.pending_samples() > 0                  # the change comes while samples are pending: they are kept
    an.set_channel_map(second)
    _step(an, twin, np.ascontiguousarray(block[700:1500]), second, "s16", device)
    an.set_channel_map(None)                         # back to the identity
    _step(an, twin, np.ascontiguousarray(block[1500:3000]), np.arange(C), "s16", device)
    an.reset_state(); twin.reset_state()             # the map is a setting: reset keeps it
    an.set_channel_map(second)
    an.reset_state()
    _step(an, twin, np.ascontiguousarray(block[3000:]), second, "s16", device)
    assert same(an.get_features(), twin.get_features())


def test_rejected_calls_change_nothing(gpu_fx):
    import torch
    C, K, N = 4, 6, 1024
    src = _sources(K, N, 4000, seed=9)
    block = im.interleave(src, "f32")
    cmap = np.array([5, 0, 3, 3])
    an, twin = _pair(gpu_fx, C, N, cmap)
    lib = an._lib
    _step(an, twin, np.ascontiguousarray(block[:300]), cmap, "f32", False)
    pend = an.pending_samples()
    # a map entry >= K: source 5 of a block of 5 channels
    narrow = np.ascontiguousarray(block[300:800, :5])
    with pytest.raises(gpu_fx.FxError):
        an.push_interleaved(narrow)
    assert an.last_launches() == [] and an.pending_samples() == pend
    # a format change while samples are pending
    with pytest.raises(gpu_fx.FxError):
        an.push_interleaved(im.encode(block[300:800], "s16"))
    assert an.last_launches() == [] and an.pending_samples() == pend
    # a device pointer misaligned by 2 (through the C ABI: the binding refuses it before)
    d = torch.zeros(500 * K + 1, dtype=torch.float32, device="cuda")
    d[1:] = torch.from_numpy(np.ascontiguousarray(block[300:800]).ravel()).cuda()
    torch.cuda.synchronize()
    frames = ctypes.c_int(5)
    st = lib.fx_push_interleaved(an._h, ctypes.c_void_p(d.data_ptr() + 2), 500, K, gpu_fx.capi.SAMPLE_F32, gpu_fx.capi.MEM_DEVICE,
                                 None, None, ctypes.byref(frames))
    assert st == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT and frames.value == 0 and an.pending_samples() == pend
    # and the next valid call is the one that would have followed
    _step(an, twin, np.ascontiguousarray(block[300:2500]), cmap, "f32", False)
    _step(an, twin, np.ascontiguousarray(block[2500:]), cmap, "f32", True)
    assert same(an.get_features(), twin.get_features())


@pytest.mark.parametrize("N,blocks", [(1024, [512]), (1024, [300, 724]), (1024, [5 * 512 + 77]), (2048, [3 * 1024 + 5]), (1024, [100])])
@pytest.mark.parametrize("device", [False, True])
def test_launch_record_is_the_deinterleave_then_the_twins(gpu_fx, N, blocks, device):
    """one hop, two hops, a long block read by the batch kernel's block feed (1024 points), a long block re-blocked (2048), no hop"""
    C, K = 6, 7
    cmap = im.maps(C, K, seed=4)["random"]
    src = _sources(K, N, sum(blocks), seed=N)
    block = im.interleave(src, "f32")
    an, twin = _pair(gpu_fx, C, N, cmap)
    at = 0
    for n in blocks:
        _step(an, twin, np.ascontiguousarray(block[at:at + n]), cmap, "f32", device)
        at += n
        got, want = an.last_launches(), twin.last_launches()
        assert got[0]["kind"] == "deinterleave" and got[0]["T"] == n
        assert got[1:] == want, (got, want)


def test_taps_before_an_interleaved_call(gpu_fx):
    C, K, N = 5, 8, 1024
    cmap = im.maps(C, K, seed=6)["strided"]
    src = _sources(K, N, 3000, seed=6)
    block = im.interleave(src, "s24")
    an, twin = _pair(gpu_fx, C, N, cmap)
    _step(an, twin, np.ascontiguousarray(block[:700]), cmap, "s24", False)
    for a in (an, twin):
        a.request_taps([0, 3])
    _step(an, twin, np.ascontiguousarray(block[700:1600]), cmap, "s24", True)
    for ch in (0, 3):
        g, w = an.taps(ch), twin.taps(ch)
        assert g["frame_index"] == w["frame_index"]
        for k in g:
            assert same(g[k], w[k]), (ch, k)


def test_block_larger_than_2_to_the_31_bytes(gpu_fx):
    import torch
    C = K = 4096
    n, N = 131584, 1024
    assert n * K * 4 > 1 << 31
    g = torch.Generator(device="cuda").manual_seed(7)
    x = (torch.rand((n, K), generator=g, device="cuda") - 0.5) * 0.5
    cmap = np.arange(C)[::-1].copy()
    an, twin = _pair(gpu_fx, C, N, cmap)
    got = an.push_interleaved(x)
    planar = x.flip(1).t().contiguous()
    del x
    want = twin.push_samples(planar)
    del planar
    assert got[0].shape == (C, n // (N // 2), 12)
    assert torch.equal(got[0].nan_to_num(1e30), want[0].nan_to_num(1e30)) and torch.equal(got[1].nan_to_num(1e30), want[1].nan_to_num(1e30))
    assert same(got[0][::97].cpu().numpy(), want[0][::97].cpu().numpy())
    assert an.pending_samples() == twin.pending_samples() and same(an.get_features(), twin.get_features())


def _records(path):
    b = open(path, "rb").read()
    out, pos = [], 0
    while pos < len(b):
        n = int.from_bytes(b[pos:pos + 4], "little")
        out.append(b[pos + 4:pos + 4 + n])
        pos += 4 + n
    return out


def _build(gpu_fx, tmp_path, src, name, extra=()):
    gpu_fx.load_library()
    exe = str(tmp_path / name)
    lib_dir = os.path.dirname(gpu_fx.library_path())
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, *src), "-o", exe,
                           "-L", lib_dir, "-lfx_hip", "-Wl,-rpath," + lib_dir] + list(extra))
    return exe


def test_wav_to_osc_all_channels(gpu_fx, tmp_path):
    exe = _build(gpu_fx, tmp_path, ("examples", "wav_to_osc.cpp"), "wav_to_osc")
    wav = str(tmp_path / "six.wav")
    x = gpu_fx.synth.samples(6, 48000 + 333, first_channel=2).T
    gpu_fx.wav.write_wav(wav, 48000, x, "pcm16")
    for direct in ([], ["--pcm16-direct"]):
        for mode in (["--batch", "7"], ["--device-block", "480"]):
            dump = str(tmp_path / "all.bin")
            out = subprocess.run([exe, wav, "--window", "1024", "--gain", "0.5", "--all-channels", "--dump", dump] + mode + direct,
                                 capture_output=True, text=True)
            assert out.returncode == 0, out.stdout + out.stderr
            every = _records(dump)
            for k in range(6):
                one = str(tmp_path / ("one%d.bin" % k))
                out = subprocess.run([exe, wav, "--window", "1024", "--gain", "0.5", "--channel", str(k), "--address", "/Audio/A%d" % k,
                                      "--dump", one, "--batch", "7"] + direct, capture_output=True, text=True)
                assert out.returncode == 0, out.stdout + out.stderr
                mine = [r for r in every if r.split(b"\0", 1)[0] == b"/Audio/A%d" % k]
                want = _records(one)
                assert len(want) == (48000 + 333) // 512 and mine == want, (k, direct, mode)
            assert len(every) == 6 * len(want)


def test_cpp_collector_mirror(gpu_fx, tmp_path):
    exe = _build(gpu_fx, tmp_path, ("tests", "cpp", "interleave_mirror.cpp"), "interleave_mirror", ["-pthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "interleave_mirror: ok" in out.stdout
