"""Hop streams from full scale up to overflow, and hops that hold NaN, inf and near-overflow samples: the loud mirror of tests/level_cases.py.

DESIGN section 1: "NaN / inf / values > 1 are the reference's, not fixed".  By the CPU oracle (tests/test_overflow_cpu.py holds each line, at
every size):
  1e2 .. 1e7     every slot as at full scale, except that the serial flatness product is inf (the low tones' crosses that edge between
                 1e2 and 1e3); f0 is the full-scale channel's but for a few near-ties of the low tones' lag search
  1e7 .. 1e10.5  the overflow band: re * re, ac * ac * s and the running fp32 sum of the pitch path (oracle/fx_oracle.c, estimate_pitch)
                 overflow one after the other, and the raw F0 slot -- an exact slot -- moves while it stays > 0, until lag -1 takes over
  >= 1e11        every cnd is NaN or inf, the lag is -1 and f0 = -2 nyquist / 5000 (at 1e11 a single frame may still keep a lag)
  ~ 1e19         the RMS product overflows in fp32 (as JUCE's sample * sample does): the RMS slot is inf
  1e25 .. 1e36   the flux is inf
  1e36 .. 1e38   bins overflow inside the transforms (inf - inf): centroid, spread, LER and slope are NaN
  one bad sample the two frames that see it: RMS NaN or inf, f0 = -2 nyquist / 5000, spectral slots 0 (the gate) or NaN; the smoothed values
                 are non-finite for as long as their histories hold it, then recover

Where the reference defines an answer: HarmonicCharacteristics.h:161-166,205 indexes with floor(f0 / range), which is negative for
f0 <= 0, so in a frame whose raw f0 is not > 0 the reference reads out of bounds and HER, OER and inharmonicity (slots 9..11) have no
reference value -- `defined` masks exactly those slot-frames (and the smoothed ones whose 10-entry history holds one), by the oracle's f0
alone.  Everything else is defined for every input, and so is every slot of a spectral-only context.

Per window size one case [C][24][N/2]; `labels` lists the channels: the ladder (level_cases' three base signals times 10^e), two walks
(a tone fading in from 1 to 1e12 over the 24 frames and its mirror), the transients (one bad value in hop BAD_HOPS[0] and again in hop
BAD_HOPS[1] of a clean tone and of signals.bursts) and, behind every three of them and every group, a clean channel -- one of the two of
`clean`, which a test runs alone as well.  No file I/O; everything follows from the seeds, and CRC holds the bytes the committed reference record was made from."""
import zlib

import numpy as np

import signals

T = 24
SIZES = (256, 512, 1024, 2048, 4096)
BASES = ("tone", "low_tones", "loud_noise")
F0, RMS, FLATNESS, FLUX = 2, 1, 5, 7
HARMONIC_SLOTS = (9, 10, 11)
HISTORY = 10                                    # ValueHistory entries of a smoothed slot (RealTimeAudioAnalysis.h)

LOUD = (2.0, 3.0, 5.0, 7.0)
BAND = (7.0, 7.5, 8.0, 8.5, 9.0, 9.5, 10.0, 10.5, 11.0)
RMS_EDGE = (18.5, 19.0, 19.5)
HIGH = (25.0, 30.0)
TRANSFORM = (34.0, 35.0, 36.0, 37.0, 38.0)
LEVELS = tuple(sorted(set(LOUD + BAND + RMS_EDGE + HIGH + TRANSFORM)))
FADE_CEILING = 1e12
LOW_TONES_CHANNELS, LOW_TONES_MID = 8, 4

# The hops that hold the bad value.  A harmonic slot's smoothed value is masked while its history holds an undefined frame, that is for
# 9 frames after the two that see the bad hop: with the second bad hop at 9 the smoothed slots 9..11 are defined again from frame 20 on,
# so that four frames of recovery are observed within the 24 (with bad hops 3 and 13 the smoothed slots would stay masked to the end).
# BURSTS_SEED: the signals.bursts(1, T, N, seed) whose onset column, for each onset type at sensitivity 0.2, both gains an onset and
# loses one under these hops -- under the combined type the clean stream must have an onset to lose, which few seeds give.  Found by
# search with the oracle over seeds N + 9 .. N + 400 and first hops 1 .. 4, second hops 7 .. 9; tests/test_overflow_cpu.py holds it.
BAD_HOPS = (1, 9)
BURSTS_SEED = {256: 256 + 128, 512: 512 + 24, 1024: 1024 + 26, 2048: 2048 + 48, 4096: 4096 + 84}

NEG_NAN_PAYLOAD = 0xFFC12345
BAD_VALUES = (("nan", float("nan")), ("-nan", None), ("+inf", float("inf")), ("-inf", float("-inf")), ("3e38", 3e38), ("-3e38", -3e38),
              ("1e12", 1e12))
POSITIONS = ("0", "17", "last")                  # sample 0, sample 17 and sample N/2 - 1 of the hop
# every value at every position (under the combined onset type only 1e12 at the hop's last sample creates an onset); a whole hop of +inf
# and of 1e20; a NaN in the stream's very first sample
TRANSIENTS = tuple((v, p) for v, _ in BAD_VALUES for p in POSITIONS) + (("+inf", "hop"), ("1e20", "hop"), ("nan", "first"))
# No four neighbouring channels without a clean one, so that a one-frame form that packs 4 to 8 channels into a workgroup always mixes
# clean channels with poisoned or ladder ones
CLEAN_EVERY = 3

# zlib.crc32 of hops(N)'s bytes: what the committed reference record (tests/golden/overflow/cases.npz) was made from
CRC = {256: 2349981045, 512: 3912328260, 1024: 3731403678, 2048: 2933320367, 4096: 3955177259}

_CACHE, _BASE, _LABELS = {}, {}, {}


def _base(name, N):
    if (name, N) not in _BASE:
        if name == "tone":
            x = signals.tone_vibrato_noise(1, T, N, seed=N + 1)[0]
        elif name == "low_tones":
            x = signals.low_tones(LOW_TONES_CHANNELS, T, N, seed=N + 2)[LOW_TONES_MID]
        elif name == "loud_noise":
            x = signals.loud_noise(1, T, N, seed=N + 3)[0]
        elif name == "clean_tone":
            x = signals.tone_vibrato_noise(1, T, N, seed=N + 7)[0]
        else:
            x = signals.bursts(1, T, N, seed=BURSTS_SEED[N])[0]
        x = np.ascontiguousarray(x, np.float32)
        x.setflags(write=False)
        _BASE[name, N] = x
    return _BASE[name, N]


def scaled(x, e):
    """x * 10^e in fp32 (one rounding of the factor, one per product: what a float gain does); an overflowing product is inf"""
    with np.errstate(over="ignore"):
        return (np.asarray(x, np.float32) * np.float32(10.0 ** e)).astype(np.float32)


def full_scale(N, kind):
    """the base signal of a ladder kind at full scale, [24][N/2] (read-only)"""
    return _base(kind, N)


def overflowing(N):
    """the (base, e) whose scaled samples are not all finite: the only ladder channels that are dropped"""
    return tuple((b, e) for b in BASES for e in LEVELS if not np.isfinite(scaled(_base(b, N), e)).all())


def _clean(kind, N):
    return _base(kind, N)


def bad_value(name):
    if name == "-nan":
        return np.array([NEG_NAN_PAYLOAD], np.uint32).view(np.float32)[0]
    if name == "1e20":
        return np.float32(1e20)
    return np.float32(dict(BAD_VALUES)[name])


def poisoned(x, value, position, hops=BAD_HOPS):
    """x [T][N/2] with the bad value written into the hops' sample (position: one of POSITIONS), over the whole hop ("hop") or into the
    stream's very first sample only ("first")"""
    out = np.array(x, np.float32)
    v = bad_value(value)
    if position == "first":
        out[0, 0] = v
        return out
    for t in hops:
        if position == "hop":
            out[t, :] = v
        else:
            out[t, {"0": 0, "17": 17, "last": out.shape[1] - 1}[position]] = v
    return out


def last_bad_frame(label):
    """the last frame whose window holds the channel's bad value (the hop and the frame after it)"""
    return 1 if label[1].endswith("@first") else BAD_HOPS[-1] + 1


def labels(N):
    """(kind, e) per channel: kind one of BASES with its exponent e; "fade_in" / "fade_out" (e None); "clean_tone" / "clean_bursts" (e: the
    channel it follows); "tone_bad" / "bursts_bad" with e = "<value>@<position>" """
    if N in _LABELS:
        return _LABELS[N]
    dropped = overflowing(N)
    out = _LABELS[N] = []
    groups = [[(b, e) for e in LEVELS if (b, e) not in dropped] for b in BASES] + [[("fade_in", None), ("fade_out", None)]]
    groups += [[(kind, "%s@%s" % vp) for vp in TRANSIENTS] for kind in ("tone_bad", "bursts_bad")]
    for group in groups:                                            # a clean channel behind every CLEAN_EVERY channels and every group
        for k, label in enumerate(group):
            out.append(label)
            if k % CLEAN_EVERY == CLEAN_EVERY - 1 or k == len(group) - 1:
                cleans = sum(kind.startswith("clean") for kind, _ in out)
                out.append(("clean_bursts" if cleans % 2 else "clean_tone", "after " + label_id(label)))
    return out


def label_id(label):
    return label[0] if label[1] is None else "%s@1e%g" % label if label[0] in BASES else "%s %s" % label


def channels(N, kind=None, e=None):
    """indices of the channels of one kind and / or level"""
    return [i for i, (k, le) in enumerate(labels(N)) if (kind is None or k == kind) and (e is None or le == e)]


def transients(N):
    return channels(N, "tone_bad") + channels(N, "bursts_bad")


# taps: the bad hop's sample 0 is the window's sample 0 in the frame after it -- Bartlett weight 0, so the window holds 0 * inf
TAP_FRAME = BAD_HOPS[0] + 1


def tap_channels(N):
    """an overflow-band channel, +inf under Bartlett weight 0 (in frame TAP_FRAME) and a channel whose bins overflow inside the transforms"""
    return [channels(N, "tone", 8.5)[0], channels(N, "tone_bad", "+inf@0")[0], channels(N, "tone", 36.0)[0]]


def tap_window(N, c):
    h = hops(N)
    return np.concatenate([h[c, TAP_FRAME - 1], h[c, TAP_FRAME]])


def clean_channels(N):
    """{kind: indices} of the clean channels of the case; clean(N) holds one of each kind, in this order"""
    return {k: channels(N, k) for k in ("clean_tone", "clean_bursts")}


def clean(N):
    """[2][24][N/2]: the two clean channels alone"""
    out = np.ascontiguousarray(np.stack([_clean("clean_tone", N), _clean("clean_bursts", N)]), np.float32)
    out.setflags(write=False)
    return out


def hops(N):
    """[C][24][N/2] float32, one channel per entry of labels(N) (read-only: shared between tests)"""
    if N not in _CACHE:
        H = N // 2
        rows = []
        for kind, e in labels(N):
            if kind in BASES:
                rows.append(scaled(_base(kind, N), e))
            elif kind in ("fade_in", "fade_out"):
                tone = signals.tone_vibrato_noise(1, T, N, seed=N + 4)[0].reshape(-1)
                env = np.exp(np.log(FADE_CEILING) * np.arange(T * H) / (T * H - 1.0))
                if kind == "fade_out":
                    env = env[::-1]
                rows.append((tone * env.astype(np.float32)).astype(np.float32).reshape(T, H))
            elif kind in ("clean_tone", "clean_bursts"):
                rows.append(_clean(kind, N))
            else:
                value, position = e.split("@")
                rows.append(poisoned(_clean("clean_tone" if kind == "tone_bad" else "clean_bursts", N), value, position))
        out = np.ascontiguousarray(np.stack(rows), np.float32)
        out.setflags(write=False)
        _CACHE[N] = out
    return _CACHE[N]


def crc(N):
    return zlib.crc32(hops(N).tobytes())


_ORACLE = {}


def oracle_run(oracle, N, which="case", **settings):
    """(raw, smoothed) of the CPU oracle on the size's case (or on clean(N)), computed once and shared (read-only)"""
    key = (N, which, tuple(sorted(settings.items())))
    if key not in _ORACLE:
        out = oracle.push_hops(hops(N) if which == "case" else clean(N), N, **settings)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def defined(raw_oracle):
    """(raw, smoothed) boolean [C][T][12]: where the reference defines an answer.  Slots 9, 10, 11 of frame t are undefined raw iff the
    oracle's raw f0 at t is not > 0, and undefined smoothed iff that holds for any frame of [t - 9, t] (the slot's own 10-entry
    ValueHistory: the reference carries nothing else out of an undefined frame).  Slots 0..8 are always defined.  From the oracle alone."""
    raw_oracle = np.asarray(raw_oracle)
    with np.errstate(invalid="ignore"):
        bad = ~(raw_oracle[..., F0] > 0)                                       # [C][T]
    held = bad.copy()
    for k in range(1, HISTORY):
        held[:, k:] |= bad[:, :-k]
    raw = np.ones(raw_oracle.shape, bool)
    sm = np.ones(raw_oracle.shape, bool)
    for s in HARMONIC_SLOTS:
        raw[..., s] = ~bad
        sm[..., s] = ~held
    return raw, sm


def assert_within(got, want, budget, mask=None, what=""):
    """every defined slot-frame within its ulp budget (signals.assert_features_within: onset exact, NaN == NaN whatever its sign or
    payload, inf == inf of the same sign); mask: boolean like got, False where the reference defines no answer -- those and nothing else
    are ignored.  Returns the largest distance per slot over what was compared."""
    return signals.assert_features_within(got, want, budget, what=what, defined=mask)
