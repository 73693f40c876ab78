"""Host model of fx_push_interleaved's input (include/fx.h): interleaved blocks [n][K] (packed s24: uint8 [n][3K]) and the planar block
[C][n] a channel map makes of them, [c][i] = block[i][map[c]] -- what fx_push_samples is given in the twin runs of
tests/test_gpu_interleave.py."""
import numpy as np

FORMATS = ("f32", "f16", "s16", "s24")


def encode(x, fmt):
    """float samples [..][n] -> the format's array: f32 / f16 / s16 as they are, s24 as uint8 [..][3n] (little endian)"""
    x = np.asarray(x, np.float32)
    if fmt == "f32":
        return x.copy()
    if fmt == "f16":
        return x.astype(np.float16)
    if fmt == "s16":
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    v = np.clip(np.round(x.astype(np.float64) * 8388608.0), -8388608, 8388607).astype(np.int32)
    b = np.stack([(v >> (8 * i)) & 0xFF for i in range(3)], axis=-1).astype(np.uint8)
    return b.reshape(x.shape[:-1] + (3 * x.shape[-1],))


def interleave(sources, fmt):
    """sources [K][n] of floats -> the interleaved block [n][K] in `fmt` (uint8 [n][3K] for s24)"""
    planar = encode(sources, fmt)
    K = planar.shape[0]
    if fmt == "s24":
        n = planar.shape[1] // 3
        return np.ascontiguousarray(planar.reshape(K, n, 3).transpose(1, 0, 2).reshape(n, 3 * K))
    return np.ascontiguousarray(planar.T)


def planar(block, channel_map, fmt):
    """the planar block [C][n] (uint8 [C][3n] for s24) of an interleaved one: row c is source channel_map[c]"""
    m = np.asarray(channel_map, np.int64)
    if fmt == "s24":
        n, K = block.shape[0], block.shape[1] // 3
        return np.ascontiguousarray(block.reshape(n, K, 3)[:, m, :].transpose(1, 0, 2).reshape(len(m), 3 * n))
    return np.ascontiguousarray(block[:, m].T)


def planar_bytes(data, n, K, channel_map, sample_bytes):
    """the same, byte by byte from a flat byte string of n frames of K samples: the definition the model above is held to"""
    out = bytearray()
    for src in channel_map:
        for i in range(n):
            at = (i * K + src) * sample_bytes
            out += data[at:at + sample_bytes]
    return bytes(out)


def maps(C, K, seed=0):
    """the channel maps the tests use: identity, reversed, random with duplicates, a strided subset"""
    rng = np.random.default_rng(seed)
    rand = rng.integers(0, K, C)
    rand[-1] = rand[0]                                   # (a duplicate, whatever the draw)
    stride = max(1, K // C)
    return {"identity": np.arange(C), "reversed": np.arange(C)[::-1].copy(), "random": rand,
            "strided": (np.arange(C) * stride + (K - 1 - (C - 1) * stride) // 2) % K}
