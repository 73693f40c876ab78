"""Hop streams that sit on the sample rate's rounding edges, and the rates they are run at.

The rate enters the analysis only where rounding decides.  The sharpest such place is the inharmonicity's `floor(rs) != floor(re)` test
(ref HarmonicCharacteristics.h:212-244): rs = (bin * fr) / f0 with fr = nyquist / M and f0 = 2 nyquist / lag is bin * lag / N in exact
arithmetic, an exact integer whenever N divides bin * lag -- and which side of that integer the double lands on depends on the rate.  A
spectral peak at bin b uses both b and b + 1, so a sinusoid at the exact bin centre b / N cycles per sample with N | (b + 1) * lag is
counted at one rate and skipped at another.

Each case is a low sinusoid that fixes the lag estimate, cosines at such bin centres and a little noise, so that frames differ.  The
reference's lag estimator is not predicted here (it answers about a quarter of the period for these tones, PitchAnalyser.h:110-190):
the parameters below were found by search with the CPU oracle -- lags whose edges move with the rate (multiples of 31, 29, 11, 79 ...
times a power of two: no factor of the usual rates), base frequencies that land on them, and the bins whose floor test differs from
48 kHz at some rate -- and tests/test_rates_cpu.py holds the outcome: at every size from 512 points and every non-dyadic rate some
frame's inharmonicity differs from the 48 kHz run while its lag is the same.  No file I/O; everything follows from the seeds."""
import numpy as np

C, T = 8, 24
SIZES = (256, 512, 1024, 2048, 4096)
EDGE_SIZES = (512, 1024, 2048, 4096)                 # where the selection condition is held (256 points: a case, no condition)

# scaling by a power of two is exact in every expression the rate enters: these give the bits of 48 kHz, F0 apart
DYADIC = (24000.0, 48000.0, 96000.0)
# 192 kHz = 4 x 48 kHz belongs to that family as well, whatever list it is written in: the invariance is held for it too
NON_DYADIC = (44100.0, 32000.0, 8000.0, 11025.0, 192000.0, 48000.0 * 1000.0 / 1001.0, 12345.678)
POWER_OF_TWO_OF_48K = DYADIC + (192000.0,)
EDGE_RATES = tuple(r for r in NON_DYADIC if r not in POWER_OF_TWO_OF_48K)
RATES = DYADIC + NON_DYADIC
MID_STREAM_RATE = float(np.float32(12345.678))      # (the reference harness hands a changed rate over as a float)

BASE_AMPLITUDE, TONE_AMPLITUDE, NOISE_SIGMA = 0.5, 0.02, 1e-3

# per window size: seed, per channel (the lag aimed at, the factor on the base frequency N / (4 lag) that lands on it) and the bins of the
# added cosines
PARAMS = {
    256: dict(seed=256,
              base=[(64, 1.06), (60, 1.045), (32, 1.0), (56, 1.0325), (40, 1.0), (2, 1.0), (10, 1.0), (11, 1.0)],
              tones=[[43, 107, 59], [63], [87, 119], [95], [95], [], [], []]),
    512: dict(seed=512,
              base=[(124, 1.0575), (116, 1.0425), (128, 1.065), (64, 1.0025), (120, 1.05), (60, 1.0), (112, 1.035), (80, 1.005)],
              tones=[[127], [127], [107, 43, 187], [87, 215, 119], [63, 127], [127], [95, 191, 223], [95, 191]]),
    1024: dict(seed=1024,
               base=[(248, 1.0575), (176, 1.01), (124, 1.005), (232, 1.0425), (116, 1.0025), (256, 1.065), (128, 1.005), (240, 1.05)],
               tones=[[127, 255], [319], [255], [127, 255, 383], [255], [403, 107, 187], [215, 87, 375], [63, 127, 255]]),
    2048: dict(seed=2048,
               base=[(352, 1.01), (248, 1.005), (316, 1.01), (124, 1.0), (176, 1.0), (348, 1.01), (352, 1.01), (248, 1.005)],
               tones=[[319, 575, 639], [255, 511], [511], [511], [639], [511], [319, 575, 639], [255, 511]]),
    4096: dict(seed=4096,
               base=[(496, 1.0075), (352, 1.0025), (632, 1.01), (248, 1.0), (696, 1.01), (496, 1.0075), (352, 1.0025), (632, 1.01)],
               tones=[[255, 511, 1023], [639, 1151, 1279], [511, 1023, 1535], [511, 1023], [511, 1023, 1535], [255, 511, 1023],
                      [639, 1151, 1279], [511, 1023, 1535]]),
}

_CACHE = {}


def hops(N, channels=C, frames=T):
    """[channels][frames][N/2] float32: the first channels / frames of the size's case (read-only: shared between tests)"""
    assert channels <= C and frames <= T
    if N not in _CACHE:
        p = PARAMS[N]
        rng = np.random.default_rng(p["seed"])
        n = np.arange(T * N // 2)
        x = np.empty((C, n.size))
        for c, (lag, factor) in enumerate(p["base"]):
            k0 = N / (4.0 * lag) * factor
            x[c] = BASE_AMPLITUDE * np.sin(2 * np.pi * k0 * n / N + 0.3 * c) + rng.normal(0, NOISE_SIGMA, n.size)
        for c, bins in enumerate(p["tones"]):
            for b in bins:
                x[c] += TONE_AMPLITUDE * np.cos(2 * np.pi * b * n / N)
        out = x.astype(np.float32).reshape(C, T, N // 2)
        out.setflags(write=False)
        _CACHE[N] = out
    return _CACHE[N][:channels, :frames]


def lags(raw, rate):
    """the integer lag of every frame from its raw F0 slot, f0 / 5000 = rate / lag / 5000 (PitchAnalyser.h:57, RealTimeAnalyser.h:165-166)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.rint(rate / (np.asarray(raw)[..., 2].astype(np.float64) * 5000.0))


def rate_id(rate):
    return ("%.3f" % rate).rstrip("0").rstrip(".")


_ORACLE = {}


def oracle_run(oracle, N, rate, **settings):
    """(raw, smoothed) of the CPU oracle on the size's case at one rate, computed once and shared (read-only)"""
    key = (N, rate, tuple(sorted(settings.items())))
    if key not in _ORACLE:
        out = oracle.push_hops(hops(N), N, sample_rate=rate, **settings)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """bit-identical, except that a NaN is a NaN whatever its sign / payload"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_power_of_two_invariant(run, what):
    """run(rate) -> (raw, smoothed): at every power of two times 48 kHz the bits of 48 kHz, slot F0 exactly scaled"""
    want = run(48000.0)
    for rate in POWER_OF_TWO_OF_48K:
        got = run(rate)
        scale = np.float32(rate / 48000.0)
        for k, name in ((0, "raw"), (1, "smoothed")):
            g, w = np.array(got[k]), np.array(want[k])
            assert same_bits(g[:, :, 2], w[:, :, 2] * scale).all(), "%s %s F0 at %s" % (what, name, rate_id(rate))
            g[:, :, 2] = w[:, :, 2]
            assert same_bits(g, w).all(), "%s %s at %s differs at %s" % (what, name, rate_id(rate), np.argwhere(~same_bits(g, w))[:5])


def oracle_with_rate_events(oracle, hops, N, events, rate=48000.0, **settings):
    """the oracle over hops [C][T][N/2] with set_sample_rate(value) before hop `at` for every (at, value) in events"""
    chans = [oracle.Channel(N, rate) for _ in range(hops.shape[0])]
    for ch in chans:
        oracle._apply(ch, settings)
    cuts = [0] + [at for at, _ in events] + [hops.shape[1]]
    raws, sms = [], []
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        if i:
            [ch.set_sample_rate(events[i - 1][1]) for ch in chans]
        out = [ch.push_hops(hops[c, lo:hi]) for c, ch in enumerate(chans)]
        raws.append(np.stack([o[0] for o in out]))
        sms.append(np.stack([o[1] for o in out]))
    return np.concatenate(raws, 1), np.concatenate(sms, 1)
