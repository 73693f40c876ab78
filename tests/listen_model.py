"""Host model of listening tracks (include/fx.h, "LISTENING TRACKS"): what the analysers of a tick get once the tracks that listen to a
monitor output have had their rows replaced by the mix.  heard() is the statement vectorised over the samples, heard_naive() the same
one sample at a time, the definition heard() is held to (tests/test_listen_cpu.py).  The mix itself is monitor_model.mix of the
UNMODIFIED block: a listening track's send contributes its own source, so nothing feeds back.  sparse_mix() is monitor_model.mix for
a context of which only a few tracks are on, given those tracks' rows alone (65 536 tracks x 8193 samples are 2 GB as one array)."""
import numpy as np

import monitor_model as mm

SELF, LEFT, RIGHT = 0, 1, 2


def heard(block_f32, mix, listen):
    """block_f32 float32 [C][n], the tick's own rows; mix float32 [2][n]; listen [C] of SELF / LEFT / RIGHT -> float32 [C][n], bit
    for bit: row c is mix[listen[c] - 1] where the track listens, its own row (every byte) where it does not"""
    block = np.ascontiguousarray(block_f32, np.float32)
    mix = np.ascontiguousarray(mix, np.float32)
    listen = np.asarray(listen)
    assert block.ndim == 2 and mix.shape == (2, block.shape[1]) and listen.shape == (block.shape[0],)
    assert np.isin(listen, (SELF, LEFT, RIGHT)).all()
    out = block.copy()
    for output in (LEFT, RIGHT):
        out.view(np.uint32)[listen == output] = mix.view(np.uint32)[output - 1]
    return out


def heard_naive(block_f32, mix, listen):
    """the same, one 32-bit word at a time"""
    block, words = np.ascontiguousarray(block_f32, np.float32).view(np.uint32), np.ascontiguousarray(mix, np.float32).view(np.uint32)
    C, n = block.shape
    out = np.empty((C, n), np.uint32)
    for c in range(C):
        for i in range(n):
            out[c, i] = block[c, i] if listen[c] == SELF else words[int(listen[c]) - 1, i]
    return out.view(np.float32)


def sparse_mix(rows, left, right, n):
    """monitor_model.mix of a context in which exactly the tracks of `rows` ({track: float32 [n]}) are on, with gains left / right
    ({track: gain}): the groups' partial sums in track order, then the groups ascending.  A group with no track on adds +0, which
    changes no bit (the accumulators start at +0 and are never -0), so it is left out."""
    out = np.zeros((2, n), np.float32)
    with np.errstate(all="ignore"):
        for ch, gain in enumerate((left, right)):
            total = np.zeros(n, np.float32)
            for g in sorted({t // mm.GROUP for t in rows}):
                part = np.zeros(n, np.float32)
                for t in sorted(t for t in rows if t // mm.GROUP == g):
                    part = part + np.float32(gain[t]) * np.asarray(rows[t], np.float32)
                total = total + part
            out[ch] = total
    return out
