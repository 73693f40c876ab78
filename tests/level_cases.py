"""Hop streams from full scale down to subnormal samples, and through the band where f0 rests on IEEE gradual underflow.

Every parity input of the rest of the suite lies between about 1e-5 and 31 of full scale.  Below 1e-8 the pitch path (oracle/fx_oracle.c,
estimate_pitch: re * re in fp32, the inverse transform, ac * ac * s, the serial fp32 running sum and v / sum) leaves the normal fp32
range, and between 1e-9 and 1e-13 the raw F0 slot -- an exact slot -- depends on subnormal arithmetic being done as IEEE 754 has it: an
implementation that flushes subnormals answers another lag there (tests/test_levels_cpu.py holds that of these inputs, by the oracle
alone).  Below the band every v underflows to 0, every cnd is 0 and the search stops at lag 2 -- what silence gives; the RMS slot,
log10(1 + 9 rms) in fp32, is exactly 0 from about 1e-8 down, so from there on F0 is the only slot that tells a level from silence.

Per window size one case [C][12][N/2]: three base signals of tests/signals.py (the tone with vibrato and noise, one mid channel of the low
tones, the loud noise), each multiplied in fp32 by 10^e for every e of LEVELS, then one tone fading out from 1 to 1e-14 over the twelve
frames and its mirror fading in, so that a stream walks through the band with the low-pass, flux, history and onset state carried.
No file I/O; everything follows from the seeds, and CRC holds the bytes the committed reference record was made from."""
import zlib

import numpy as np

import lag_cases
import signals

T = 12
SIZES = (256, 512, 1024, 2048, 4096)
BASES = ("tone", "low_tones", "loud_noise")

NORMAL = (-2.0, -4.0, -6.0, -8.0)
BAND = (-9.0, -9.5, -10.0, -10.5, -11.0, -11.5, -12.0, -12.5, -13.0)          # f0 depends on gradual underflow here
BELOW = (-15.0, -20.0, -30.0, -36.0)                                           # (-36: the samples are partly subnormal)
SUBNORMAL = (-39.0, -42.0, -45.0)                                              # all subnormal; at -45 partly zero
LOUD = (1.0, 3.0, 5.0)
# Loud levels, overflow and non-finite samples are held by tests/overflow_cases.py; here a loud level is kept only where the oracle's output
# is finite with f0 > 0.  Every (base, e) dropped here is dropped for one reason: the
# serial flatness product (SpectralCharacteristics.h:89-94) overflows to inf, so the raw flatness slot is inf and its smoothed value
# inf or NaN.  (f0 > 0 holds at all three loud levels at every size: the lag is never -1 and the reference does not index out of bounds;
# that overflow is what tests/signals.py's `levels` covers.)  tests/test_levels_cpu.py holds that exactly these are not finite.
_ALL_LOUD = tuple((b, e) for b in BASES for e in LOUD)
DROPPED = {256: tuple(p for p in _ALL_LOUD if p not in (("tone", 1.0), ("low_tones", 1.0))),
           512: tuple(p for p in _ALL_LOUD if p != ("tone", 1.0)),
           1024: _ALL_LOUD, 2048: _ALL_LOUD, 4096: _ALL_LOUD}
LEVELS = NORMAL + BAND + BELOW + SUBNORMAL + LOUD
FADE_FLOOR = 1e-14
LOW_TONES_CHANNELS, LOW_TONES_MID = 8, 4
LAG_REGIMES = ("blocks 0-1", "blocks 2-3", "past 255", "fallback")

# zlib.crc32 of hops(N)'s bytes: what the committed reference record (tests/golden/levels/cases.npz) was made from
CRC = {256: 2812705679, 512: 79302845, 1024: 1623121958, 2048: 3310669289, 4096: 1212814380}

_CACHE = {}


def _base(name, N):
    if name == "tone":
        return signals.tone_vibrato_noise(1, T, N, seed=N + 1)[0]
    if name == "low_tones":
        return signals.low_tones(LOW_TONES_CHANNELS, T, N, seed=N + 2)[LOW_TONES_MID]
    return signals.loud_noise(1, T, N, seed=N + 3)[0]


def scaled(x, e):
    """x * 10^e in fp32 (one rounding of the factor, one per product: what a float gain does)"""
    return (np.asarray(x, np.float32) * np.float32(10.0 ** e)).astype(np.float32)


def labels(N):
    """(kind, e) per channel: kind one of BASES, or "fade_out" / "fade_in" (e None)"""
    out = [(b, e) for b in BASES for e in LEVELS if (b, e) not in DROPPED[N]]
    return out + [("fade_out", None), ("fade_in", None)]


def label_id(label):
    return label[0] if label[1] is None else "%s@1e%g" % label


def channels(N, kind=None, e=None):
    """indices of the channels of one kind and / or level"""
    return [i for i, (k, le) in enumerate(labels(N)) if (kind is None or k == kind) and (e is None or le == e)]


def hops(N):
    """[C][12][N/2] float32, one channel per entry of labels(N) (read-only: shared between tests)"""
    if N not in _CACHE:
        H = N // 2
        rows = []
        for kind, e in labels(N):
            if kind in BASES:
                rows.append(scaled(_base(kind, N), e))
            else:
                tone = signals.tone_vibrato_noise(1, T, N, seed=N + 4)[0].reshape(-1)
                env = np.exp(np.log(FADE_FLOOR) * np.arange(T * H) / (T * H - 1.0))
                if kind == "fade_in":
                    env = env[::-1]
                rows.append((tone * env.astype(np.float32)).astype(np.float32).reshape(T, H))
        out = np.ascontiguousarray(np.stack(rows), np.float32)
        out.setflags(write=False)
        _CACHE[N] = out
    return _CACHE[N]


def crc(N):
    return zlib.crc32(hops(N).tobytes())


def full_scale(N, kind):
    """the base signal of a scaled kind at full scale, [12][N/2] (for the gain routes: gain 10^e on these)"""
    return np.ascontiguousarray(_base(kind, N))


F16_SUBNORMAL_PEAKS = (5e-5, 1.5e-5, 2e-6, 5e-7)       # a half is subnormal below 6.1e-5 and counts in steps of 6e-8


def f16_subnormal(N):
    """[4][12][N/2] float16: a tone and a noise whose halves are mostly subnormal, and both again 25 / 30 times quieter, where a sample is
    a few steps of the smallest half -- ordinary levels for a fading fp16 stream"""
    tone = signals.tone_vibrato_noise(1, T, N, seed=N + 5)[0]
    noise = signals.loud_noise(1, T, N, seed=N + 6)[0]
    a, b, c, d = F16_SUBNORMAL_PEAKS
    return np.stack([tone * np.float32(a), noise * np.float32(b), tone * np.float32(c), noise * np.float32(d)]).astype(np.float16)


_ORACLE = {}


def oracle_run(oracle, N, **settings):
    """(raw, smoothed) of the CPU oracle on the size's case, computed once and shared (read-only)"""
    key = (N, tuple(sorted(settings.items())))
    if key not in _ORACLE:
        out = oracle.push_hops(hops(N), N, **settings)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def windows(h):
    """[T][N/2] hops of one channel -> the [T][N] overlapped windows the analysers read (the first one starts with silence)"""
    x = np.concatenate([np.zeros((1, h.shape[1]), np.float32), h])
    return np.concatenate([x[:-1], x[1:]], axis=1)


def lag_regime(oracle, window):
    """which part of the lag search (PitchAnalyser.h:161-190) decides this window, by the oracle's own cnd (fxo_estimate_pitch): the 64-sample
    block in which the walk from the first cnd < 0.01 stops falling -- where a kernel that takes the cnd block by block may stop -- or the
    global-minimum fallback.  -> one of LAG_REGIMES; the lag the walk gives is checked against the oracle's.  (The classification is
    tests/lag_cases.py's, which holds a frame for every seam between the blocks; these regimes are the coarse view of it.)"""
    lag, cnd = lag_cases.oracle_cnd(oracle, window)
    kind, _, s, mine = lag_cases.classify_cnd(cnd, len(window))
    if kind == "fallback":
        return "fallback"
    assert lag == mine, (lag, s)
    return "blocks 0-1" if s + 1 < 128 else "blocks 2-3" if s + 1 < 256 else "past 255"
