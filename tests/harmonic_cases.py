"""Frames that put part 2 of the harmonic analyser (HarmonicCharacteristics.h:46-244; FrameWave::harmonic_tail and PairWave::harmonic_tail
in csrc/) on its ties, seams and bin edges.

The kernels hold U = M/64 bins per lane (the pair kernel U2 = M/128 per lane of two wavefronts), take the neighbours of a lane's first
and last bins from other lanes, ignore bin M-1 seen from bin M-2, and redo the sum over the bins in the reference's serial order only
when a bin sits within rounding distance of the mean.  Noise never puts two neighbouring bins at exactly equal |re|, a probe frequency
exactly on a bin edge, or a whole spectrum on its mean.  The frames here do: sparse impulses and impulse trains of exact amplitudes
(s16 steps, or fp32 given by its bits where the rounding of the serial sum is the point), whose spectra are exact sums of a few terms.
No sin or cos of the host decides a frame.  No file I/O: everything follows from the parameters, CRC holds the bytes.

analyse() restates the reference for one raw spectrum and one lag in the reference's own serial order and records which operand decided;
classes() names what a frame holds; model() is analyse() with one decision changed (MUTANTS), so that tests/test_harmonic_cases_cpu.py can
hold, by the oracle alone, that the frames tell every such slip apart.  tests/golden/make_harmonic_cases.py is the search that chose the
frames; CASES is its table, UNREACHED what it looked for and did not find, UNTOLD the mutants no chosen frame tells apart (none).  tests/test_gpu_harmonic_cases.py runs the frames through
every implementation."""
import math
import zlib

import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
T = 12                                                                         # frames per channel of the batch layout
MAX_FRAMES = 96
RATES = (48000.0, 44100.0)
PAIR_SIZES = (2048, 4096)                                                      # the sizes with a pair kernel (two wavefronts per frame)
HER, OER, INHARM = 9, 10, 11
f32, f64 = np.float32, np.float64


# ---- the families ----
def synth(N, case):
    """one frame [N] float32 of a table entry:
    ("sp", ((n, k), ...))                   x[n] = k / 32768 (n < 0 counts from the end): sparse impulses, s16-exact
    ("fb", ((n, bits), ...))                x[n] = the fp32 with these bits
    ("train", period, phase, ka, kb, dc)    x[phase + i period] = ka (i even) or kb (i odd), on a constant dc; all in s16 steps
    ("mix", case, case)                     the sum of two s16-exact entries"""
    x = np.zeros(N, f32)
    fam = case[0]
    if fam == "sp":
        for n, k in case[1]:
            x[n % N] = f32(k) / f32(32768.0)
    elif fam == "fb":
        for n, bits in case[1]:
            x[n % N] = np.array([bits], np.uint32).view(f32)[0]
    elif fam == "train":
        _, period, phase, ka, kb, dc = case
        v = np.full(N, dc, np.int64)
        at = np.arange(phase, N, period)
        v[at] += np.where(np.arange(at.size) % 2 == 0, ka, kb)
        assert np.abs(v).max() <= 32767
        x = v.astype(f32) / f32(32768.0)
    elif fam == "mix":
        x = synth(N, case[1]) + synth(N, case[2])
        assert s16_exact(case) and np.array_equal(as_s16(x).astype(f32) / f32(32768.0), x)
    else:
        raise KeyError(fam)
    return x


def s16_exact(case):
    return case[0] != "fb" and (case[0] != "mix" or (s16_exact(case[1]) and s16_exact(case[2])))


# ---- what the analyser is given: the oracle's raw spectrum and the oracle's lag ----
def oracle_inputs(oracle, window, rate=48000.0):
    """(re [M+1] float32: the real parts of bins 0 .. M of the raw window's transform (forward_real; the analyser reads bins 0 .. M-1, bin M
    is what a window that is not clipped would read), the lag of the oracle's pitch path lowpass -> bartlett -> forward_real ->
    estimate_pitch)"""
    window = np.ascontiguousarray(window, f32)
    M = window.shape[0] // 2
    re = oracle.forward_real(window)[0:2 * M + 2:2].copy()
    _, lag, _ = oracle.estimate_pitch(oracle.forward_real(oracle.bartlett(oracle.lowpass(window))), rate / 2.0)
    return re, float(lag)


# ---- the restatement, with one decision changed on demand ----
# name: (what is changed, whether it depends on the bins-per-lane geometry)
MUTANTS = {
    "ge_l2": ("bin-2 rejects on >= (:141)", False),
    "ge_l1": ("bin-1 rejects on >= (:141)", False),
    "ge_r1": ("bin+1 rejects on >= (:141)", False),
    "wrong_l2_j0": ("a lane's first bin takes bin-1 for bin-2", True),
    "wrong_l2_j1": ("a lane's second bin takes bin-3 for bin-2", True),
    "wrong_l1_j0": ("a lane's first bin takes bin-2 for bin-1", True),
    "wrong_r1_jlast": ("a lane's last bin takes bin+2 for bin+1", True),
    "seam_l2_0": ("bin M/2 takes bin-1 for bin-2 (the pair kernel's wave seam)", False),
    "seam_l2_1": ("bin M/2+1 takes bin-3 for bin-2 (the wave seam)", False),
    "seam_l1_0": ("bin M/2 takes bin-2 for bin-1 (the wave seam)", False),
    "seam_r1_last": ("bin M/2-1 takes bin+2 for bin+1 (the wave seam)", False),
    "m1_not_ignored": ("bin M-2 is compared with bin M-1 (:137)", False),
    "last_window_unclipped": ("bin M-1 is compared with bin M (:137)", False),
    "tree_sum": ("the sum over the bins taken per lane and then pairwise, not serially (:61-66)", True),
    "ge_mean": ("mag >= mean passes (:132)", False),
    "recip_fr": ("freq * (1 / fr) for freq / fr (:248)", False),
    "recip_f0": ("x * (1 / f0) for x / f0 in the ratios (:258)", False),
    "hb_gt": ("hb > M breaks, not hb >= M (:174)", False),
    "no_f0_skip": ("a peak in f0's bin is not skipped (:220)", False),
    "no_fs0": ("bin 0's start frequency stays 0 (:225)", False),
    "floors_lt": ("floor(start) < floor(end) skips, not != (:232)", False),
    "her_clamp": ("HER is not clamped at 1 (:187)", False),
}
SEAM_MUTANTS = ("seam_l2_0", "seam_l2_1", "seam_l1_0", "seam_r1_last")         # 2048 and 4096 points only
# Mutants that change no slot for any lag the search can answer (2 .. N), at either rate: no frame can tell them apart, and
# tests/test_harmonic_cases_cpu.py holds that by going through every lag
EQUIVALENT = {
    "recip_fr": "floor(freq * (1 / fr)) is floor(freq / fr) for all 18 probe frequencies of every lag 2 .. N at 48 kHz and 44.1 kHz",
    "no_fs0": "bin 0 adds nothing either way: with fs = fr / 2 the floors of f0 / (fr / 2) = 2 N / lag and f0 / fr = N / lag differ for "
              "every lag <= N, and with fs = 0 the ratio is infinite and its floor differs from every other",
}
# Single decisions of the same code that the model does not take as mutants, because no frame can show them in a slot:
NOT_OBSERVABLE = {
    "gate_le": "magnitudeSum <= 0.005 for < (:88) differs only at a serial sum of exactly 0.005 (UNREACHED: ('gate', 'equal'))",
    "oer_clamp": "the OER slot receives HER (RealTimeAnalyser.h:171): nothing computed from the odd and even energies reaches a slot",
    "her_floor": "HER < 0 (:188) needs a negative normalised magnitude",
}


def _serial(a):
    return float(np.add.accumulate(np.asarray(a, f64))[-1]) if len(a) else 0.0


def _tree(a, U):
    """the sum as a wavefront takes it: every lane its own U bins in order, then the lanes pairwise"""
    lanes = np.asarray(a, f64).reshape(-1, U)
    s = np.zeros(lanes.shape[0])
    for j in range(U):
        s = s + lanes[:, j]
    while s.size > 1:
        s = s[0::2] + s[1::2]
    return float(s[0])


def analyse(re, lag, nyquist, mutant=None, U=None):
    """HarmonicCharacteristics.h:46-244 on re [M+1] (oracle_inputs) with f0 = 2 nyquist / lag (PitchAnalyser.h:57), sums in the
    reference's serial order.  U: bins per lane, for the mutants that depend on it (default M/64).  Returns a dict:
    slots (HER, OER, inharmonicity raw slots as float32; the OER slot receives HER, RealTimeAnalyser.h:171), and what decided:
    mag_sum, mean, gated, peaks [bins], ties [(bin, offset)], rejected {bin: offset}, probes [(kind, index, bin, exact edge?)], her, oer
    (before the clamps), terms [(bin, kind)] of the inharmonicity loop."""
    assert mutant is None or mutant in MUTANTS, mutant
    M = len(re) - 1
    U = U or M // 64
    v = np.asarray(re, f32).astype(f64)
    magx = v * v                                                               # :63-65, exact
    mag = magx[:M]
    mag_sum = _tree(mag, U) if mutant == "tree_sum" else _serial(mag)          # :66
    max_mag = float(mag.max())                                                 # :67-68
    out = {"mag_sum": mag_sum, "mean": mag_sum / M, "gated": True, "peaks": [], "ties": [], "rejected": {}, "probes": [], "her": 0.0,
           "oer": 0.0, "terms": [], "slots": (f32(0), f32(0), f32(0)), "tree_sum": _tree(mag, U), "flat": bool(mag.min() == max_mag), "mag0": mag[0],
           "f0_bin": None, "M": M, "re_last": (abs(float(v[M - 2])), abs(float(v[M - 1]))),     # |re| of bins M-2 and M-1
           "where": None}                                                      # (classify: where the frame's one impulse is)
    if mag_sum < 0.005:                                                        # :88-89
        return out
    out["gated"] = False
    with np.errstate(over="ignore"):
        normed_d = magx / max_mag                                              # :75
        normed = normed_d.astype(f32)                                          # :76
    sum_normed = _serial(normed_d[:M])                                         # :77
    mean = mag_sum / M                                                         # :86

    # binIsPeak :127-145: above the mean, none of bins -2, -1, +1 larger; the last two bins have no +1 neighbour (:137)
    idx = np.arange(M)
    P = np.full(M + 8, -1.0)
    P[4:4 + M] = mag
    o2, o1, r1 = np.full(M, -2), np.full(M, -1), np.full(M, 1)
    j = idx % U
    if mutant == "wrong_l2_j0": o2[j == 0] = -1
    if mutant == "wrong_l2_j1": o2[j == 1] = -3
    if mutant == "wrong_l1_j0": o1[j == 0] = -2
    if mutant == "wrong_r1_jlast": r1[j == U - 1] = 2
    if mutant == "seam_l2_0": o2[M // 2] = -1
    if mutant == "seam_l2_1": o2[M // 2 + 1] = -3
    if mutant == "seam_l1_0": o1[M // 2] = -2
    if mutant == "seam_r1_last": r1[M // 2 - 1] = 2
    use_r1 = idx < M - 2
    if mutant == "m1_not_ignored": use_r1[M - 2] = True
    if mutant == "last_window_unclipped":
        use_r1[M - 1] = True
        P[4 + M] = magx[M]
    n2, n1, nr = P[4 + idx + o2], P[4 + idx + o1], P[4 + idx + r1]
    above = mag >= mean if mutant == "ge_mean" else mag > mean
    rej2 = n2 >= mag if mutant == "ge_l2" else n2 > mag
    rej1 = n1 >= mag if mutant == "ge_l1" else n1 > mag
    rejr = use_r1 & (nr >= mag if mutant == "ge_r1" else nr > mag)
    peak = above & ~rej2 & ~rej1 & ~rejr
    peaks = np.flatnonzero(peak)
    out["peaks"] = peaks.tolist()
    out["on_mean"] = int(np.count_nonzero(mag == mean))
    if mutant is None:                                                         # the records are the reference's own
        for off, nb, used in ((-2, n2, idx >= 2), (-1, n1, idx >= 1), (1, nr, use_r1)):
            out["ties"] += [(int(b), off) for b in np.flatnonzero(peak & used & (nb == mag))]
        first = np.where(rej2, -2, np.where(rej1, -1, 1))
        out["rejected"] = {int(b): int(first[b]) for b in np.flatnonzero(above & ~peak)}

    # calculateHarmonicEnergyCharacteristics :147-198
    f0 = (nyquist * 2.0) / lag
    fr = nyquist / M                                                           # :93
    r_fr = 1.0 / fr

    def bin_of(freq):                                                          # :246-249
        return int(math.floor(freq * r_fr if mutant == "recip_fr" else freq / fr))

    def nb_max(c):                                                             # :200-210
        if c < 0:
            return 0.0
        lo = c - 2 if c - 2 >= 0 else 0
        hi = c + 2 if c + 2 < M else M
        m_ = normed[c]
        for q in range(lo, hi):
            if normed[q] > m_:
                m_ = normed[q]
        return float(m_)

    N = 2 * M
    ilag = int(lag)
    f0_bin = bin_of(f0)
    out["f0_bin"] = f0_bin
    score = even_e = odd_e = 0.0
    for k in range(1, 16):
        lb = bin_of(f0 / 2.0 ** k)
        exact = ilag > 0 and N % (ilag << k) == 0
        if lb == f0_bin:
            out["probes"].append(("sub_skipped", k, lb, exact))
            continue
        out["probes"].append(("sub", k, lb, exact))
        score += nb_max(lb)
    for h in range(1, 4):
        hb = bin_of(f0 * h)
        exact = ilag > 0 and (N * h) % ilag == 0
        if (hb > M) if mutant == "hb_gt" else (hb >= M):
            out["probes"].append(("break", h, hb, exact))
            break
        bm = nb_max(hb)
        out["probes"].append(("harm", h, hb, exact))
        if h % 2 == 0:
            even_e += bm
        else:
            odd_e += bm
        score += bm
    her = score / sum_normed
    out["her"] = her
    if her > 1.0 and mutant != "her_clamp":
        her = 1.0
    if her < 0.0:
        her = 0.0
    oer = even_e / odd_e if odd_e > 0.0 else 1.0
    out["oer"], out["odd_e"] = oer, odd_e
    her_d = float(f32(her))

    # calculateInharmonicity :212-244
    inh = 0.0
    if f0 > 0.0 and peaks.size:
        b = peaks if mutant == "no_f0_skip" else peaks[peaks != f0_bin]
        fs = b * fr
        if mutant != "no_fs0":
            fs = np.where(fs == 0.0, fr * 0.5, fs)
        fe = (b + 1.0) * fr
        with np.errstate(divide="ignore", invalid="ignore"):
            def ratio(f):                                                      # :251-259
                up = f > f0
                hi = np.where(up, f, f0)
                lo = np.where(up, f0, f)
                q = np.where(up & (mutant == "recip_f0"), hi * (1.0 / f0), hi / lo)
                return np.where(f == f0, 1.0, q)
            rs, re_ = ratio(fs), ratio(fe)
            skip = np.floor(rs) < np.floor(re_) if mutant == "floors_lt" else np.floor(rs) != np.floor(re_)
            r = np.where(rs < re_, rs, re_)
            terms = (r - np.floor(r)) * (mag[b] / mag_sum)
        inh = _serial(terms[~skip])
        if mutant is None:
            for bb, sk, s_, e_ in zip(b.tolist(), skip.tolist(), fs.tolist(), fe.tolist()):
                if sk:
                    kind = ("floor_skip_exact" if ((bb + 1) * ilag) % N == 0 and (bb + 1) * ilag // N >= 2 else
                            "below_exact" if bb >= 1 and N % (bb * ilag) == 0 else "floor_skip")
                elif e_ <= f0:
                    kind = "below"
                else:
                    kind = "above" if s_ >= f0 else "straddle"
                out["terms"].append((bb, kind))
    with np.errstate(invalid="ignore"):
        her_s = f32(math.log10(her_d * 9.0 + 1.0)) if her_d == her_d else f32(np.nan)
        inh_s = f32(math.log10(inh * 9.0 + 1.0)) if inh == inh and inh * 9.0 + 1.0 > 0 else f32(np.nan)
    out["slots"] = (her_s, her_s, inh_s)
    return out


def model(re, lag, nyquist, mutant=None, U=None):
    """(HER, OER, inharmonicity) raw slots of one raw spectrum and lag, with one decision changed (a key of MUTANTS) or none"""
    return analyse(re, lag, nyquist, mutant, U)["slots"]


def same_slots(a, b):
    return np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))


# ---- the classes ----
def j_labels(j, U):
    """where bin j of a lane's U bins sits: 0, 1, "U-2", "U-1" (at U = 2 the two bins are both pairs), "in" for the interior"""
    out = {lab for lab, at in ((0, 0), (1, 1), ("U-2", U - 2), ("U-1", U - 1)) if j == at}
    return out or {"in"}


def classes(a, lag, rate=48000.0):
    """the classes of one analysed frame (a = analyse(...) with no mutant), as a set of tuples.  The probe and inharmonicity classes carry
    the rate, the others do not depend on it."""
    M = a["M"]
    U = M // 64
    N = 2 * M
    out = set()
    rel = a["mag_sum"] / 0.005 - 1.0
    if abs(rel) < 1e-6:                                                        # within a few fp32 steps of the amplitude
        out.add(("gate", "below" if a["gated"] else "above"))
    if a["gated"]:
        return out
    peaks = set(a["peaks"])
    if a["flat"]:
        out.add(("flat", "every bin a peak" if len(peaks) == M else "no peak"))
        if a["tree_sum"] != a["mag_sum"]:
            out.add(("flat", "serial != tree"))
        if a["where"] is not None:                                             # one impulse, at sample 0 or at N/2
            out.add(("flat", "impulse at %s" % a["where"]))
            out.add(("flat", "impulse at %s" % a["where"], "every bin a peak" if len(peaks) == M else "no peak"))
        if not peaks and a["mean"] != float(a["mag0"]):
            out.add(("flat", "no peak, the serial sum puts the mean above the bins"))
    for b, off in a["ties"]:
        for lab in j_labels(b % U, U):
            out.add(("tie", off, lab))
        lane_seam = (b + off) // U != b // U
        if lane_seam:
            out.add(("tie across lanes", off))
        if N in PAIR_SIZES and (b < M // 2) != (b + off < M // 2):
            out.add(("tie across the wave seam", off, b - M // 2))
    if 0 in peaks:
        out.add(("end", "bin 0 a peak"))
    if (1, -1) in a["ties"]:
        out.add(("end", "bin 1 a peak tied with bin 0"))
    if M - 2 in peaks and a["re_last"][1] > a["re_last"][0]:
        out.add(("end", "bin M-2 a peak under a larger bin M-1"))
    if M - 1 in peaks:
        out.add(("end", "bin M-1 a peak"))
    if a["rejected"].get(M - 1) == -2:
        out.add(("end", "bin M-1 rejected by bin M-3"))
    r = int(rate)
    for kind, i, b, exact in a["probes"]:
        if kind == "harm":
            if exact:
                out.add(("probe", "harmonic %d on a bin edge" % i, r))
            if b in (0, 1):
                out.add(("probe", "at bin %d" % b, r))
        elif kind == "break":
            out.add(("probe", "hb == M" if (N * i) == M * int(lag) else "hb > M", r))
            if i == 1:
                out.add(("probe", "break at h = 1", r))
        elif kind == "sub":
            if exact:
                out.add(("probe", "sub-harmonic on a bin edge", r))
            if b in (0, 1):
                out.add(("probe", "at bin %d" % b, r))
    if a["odd_e"] > 0.0:
        out.add(("oer", "clamped" if a["oer"] > 1.0 else "not clamped", r))
    out.add(("her", "clamped" if a["her"] > 1.0 else "not clamped", r))
    kinds = dict((k, b) for b, k in a["terms"])
    if 0 in peaks and a["f0_bin"] != 0:
        out.add(("inh", "peak at bin 0", r))
    if a["f0_bin"] in peaks:
        out.add(("inh", "peak at f0_bin skipped", r))
    for k, name in (("floor_skip_exact", "bin end an exact multiple of f0, skipped"), ("below_exact", "f0 an exact multiple of the bin start, skipped"),
                    ("above", "peak above f0"), ("below", "peak below f0")):
        if k in kinds:
            out.add(("inh", name, r))
    if len(peaks) > 64:
        out.add(("inh", "more than 64 peaks", r))
    if len(peaks) > M // 2:
        out.add(("inh", "more than M/2 peaks", r))
    return out


def classify(oracle, window, rate=48000.0):
    """(analyse's record, the lag, the classes) of one window at one rate"""
    re, lag = oracle_inputs(oracle, window, rate)
    a = analyse(re, lag, rate / 2.0)
    N = len(window)
    at = np.flatnonzero(window)
    if at.size == 1 and int(at[0]) in (0, N // 2):                             # (a flat spectrum has other sources too: the period-4 frames)
        a["where"] = "0" if at[0] == 0 else "N/2"
    return a, lag, classes(a, lag, rate)


def describe(cls):
    """what a failure message says of a frame: its classes"""
    return "; ".join(" ".join(str(p) for p in c) for c in sorted(cls, key=repr)) or "no class"


REQUIRED_TIES = (("tie across lanes", -2), ("tie across lanes", -1), ("tie across lanes", 1),
                 ("tie", -1, 0), ("tie", -2, 0), ("tie", -2, 1), ("tie", 1, "U-1"))
TIE_CELLS = tuple(("tie", off, lab) for off in (-2, -1, 1) for lab in (0, 1, "U-2", "U-1", "in"))
RATE_CLASSES = (
    ("probe", "harmonic 1 on a bin edge"), ("probe", "harmonic 2 on a bin edge"), ("probe", "harmonic 3 on a bin edge"),
    ("probe", "hb == M"), ("probe", "hb > M"), ("probe", "break at h = 1"), ("oer", "clamped"), ("oer", "not clamped"),
    ("her", "clamped"), ("her", "not clamped"), ("probe", "sub-harmonic on a bin edge"), ("probe", "at bin 0"), ("probe", "at bin 1"),
    ("inh", "peak at bin 0"), ("inh", "peak at f0_bin skipped"), ("inh", "bin end an exact multiple of f0, skipped"),
    ("inh", "f0 an exact multiple of the bin start, skipped"), ("inh", "peak above f0"), ("inh", "peak below f0"),
    ("inh", "more than 64 peaks"), ("inh", "more than M/2 peaks"),
)


FLAT_WANTED = tuple(("flat", "impulse at %s" % w, o) for w in ("0", "N/2") for o in ("every bin a peak", "no peak")) + (
    ("flat", "no peak, the serial sum puts the mean above the bins"),)


def required(N):
    """every class the table has to hold at size N"""
    out = {("gate", "below"), ("gate", "above"), ("flat", "every bin a peak"), ("flat", "no peak"), ("flat", "serial != tree"),
           ("flat", "impulse at 0"), ("flat", "impulse at N/2"), ("end", "bin 0 a peak"), ("end", "bin 1 a peak tied with bin 0"),
           ("end", "bin M-2 a peak under a larger bin M-1"), ("end", "bin M-1 a peak"), ("end", "bin M-1 rejected by bin M-3")}
    out |= set(REQUIRED_TIES)
    if N in PAIR_SIZES:
        out |= {("tie across the wave seam", off, d) for off, d in ((-2, 0), (-2, 1), (-1, 0), (1, -1))}
    out |= {c + (int(r),) for c in RATE_CLASSES for r in RATES}
    return out


def wanted(N):
    """what the search looks for: the required classes, every (offset, j) cell, and both outcomes of a flat spectrum's tie for an
    impulse at either place, one of them with the mean strictly above the bins"""
    return required(N) | set(TIE_CELLS) | set(FLAT_WANTED)


def mutant_targets(N):
    """[(mutant, U)]: every mutant at the frame kernel's U = M/64, the geometry-dependent ones and the wave seam's also at the pair
    kernel's U2 = M/128 where there is a pair kernel"""
    M = N // 2
    out = [(m, M // 64) for m in MUTANTS if m not in SEAM_MUTANTS and m not in EQUIVALENT]
    if N in PAIR_SIZES:
        out += [(m, M // 128) for m, (_, geo) in MUTANTS.items() if geo or m in SEAM_MUTANTS]
    return out


# ---- the table: tests/golden/make_harmonic_cases.py prints it ----
# What UNREACHED lists, and why it is believed to stay out of reach of frames like these:
#   ("gate", "equal")                a serial sum of squares of exactly 0.005, whose double has a full mantissa: adjacent fp32 amplitudes of
#                                    one impulse move the sum by 1.2e-7 of itself
#   ("level", "upper on the mean")   a spectrum of two levels has its mean below the upper one by (upper - lower) times the lower level's
#                                    share, at least 1.2e-7 / M of the upper level: 1e7 times the rounding of the serial sum
#   ("mean", "within rounding, not flat")  the same distance holds for any bin of a spectrum that is not flat
#   ("probe", "at bin M-2 or M-1")   a harmonic's bin is floor(N h / lag), which is M or more for lag <= 2 h and at most 2 M / 3 = M - M/3
#                                    for the next lag; sub-harmonics lie below f0's bin
#   ("probe", "lb == f0_bin skip")   needs f0 < fr, a lag above N; the search ends at N
#   ("flat", "no peak, the serial sum ...")  at 256 and 512 points none of 1200 full-mantissa amplitudes made the serial sum of 128 or 256
#                                    equal squares round above M times the square; there "no peak" comes from sums that are exact
#   ("tie", offset, "in")           at 256 and 512 points a lane holds two and four bins: 0, 1, U-2 and U-1 are all there are
# BEGIN TABLE
CASES = {
    256: (
        ('sp', ((0, -999), (64, -999), (192, -999), (128, -999))), ('sp', ((0, -999), (64, -999), (192, -999), (128, -333))),
        ('sp', ((0, -999), (64, -999), (192, -999), (128, 999))), ('sp', ((0, -999), (64, -666), (192, -666), (128, 666))),
        ('sp', ((0, -999), (64, -666), (192, -666), (128, 999))), ('sp', ((0, -999), (128, -999))), ('sp', ((0, -999),)),
        ('sp', ((128, -999),)), ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -450), (-2, -450))),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -150), (-2, -150))), ('sp', ((0, 1000), (1, -750), (-1, -750), (2, 150), (-2, 150))),
        ('sp', ((0, 1000), (1, -150), (-1, -150), (2, 600), (-2, 600))), ('train', 1, 0, 3000, 3000, 0), ('train', 4, 0, 3000, -1500, 0),
        ('sp', ((0, -666), (64, -999), (192, -999), (128, 333))), ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -600), (-2, -600))),
        ('train', 33, 16, 3000, 1000, 0), ('train', 67, 0, 3000, -3000, 400), ('fb', ((0, 1003277517),)), ('fb', ((0, 1003277516),)),
        ('fb', ((128, 1003277517),)),
    ),
    512: (
        ('sp', ((0, -999), (128, -999), (384, -999), (256, -999))), ('sp', ((0, -999), (128, -999), (384, -999), (256, -333))),
        ('sp', ((0, -999), (128, -999), (384, -999), (256, 999))), ('sp', ((0, -999), (128, -666), (384, -666), (256, -999))),
        ('sp', ((0, -999), (128, -666), (384, -666), (256, 666))), ('sp', ((0, -999), (256, -999))), ('sp', ((0, -999),)),
        ('sp', ((0, -999), (128, 333), (384, 333), (256, 333))), ('sp', ((0, -666), (128, -999), (384, -999), (256, -999))),
        ('sp', ((256, -999),)), ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -450), (-2, -450))),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -150), (-2, -150))), ('sp', ((0, 1000), (1, -750), (-1, -750), (2, 150), (-2, 150))),
        ('sp', ((0, 1000), (1, -150), (-1, -150), (2, 600), (-2, 600))), ('train', 1, 0, 3000, 3000, 0), ('train', 4, 0, 3000, -1500, 0),
        ('sp', ((0, -666), (128, 999), (384, 999), (256, 333))), ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -600), (-2, -600))),
        ('sp', ((0, 1000), (1, -600), (-1, -600), (2, -450), (-2, -450))), ('train', 63, 1, 3000, -1500, 0),
        ('mix', ('train', 1, 0, 20, 20, 0), ('sp', ((0, -2002), (128, -1001), (384, -1001), (256, 1001)))), ('fb', ((0, 999346371),)),
        ('fb', ((0, 999346370),)), ('fb', ((256, 999346371),)),
    ),
    1024: (
        ('sp', ((0, -999), (256, -999), (768, -999), (512, -999))), ('sp', ((0, -999), (256, -999), (768, -999), (512, -666))),
        ('sp', ((0, -999), (256, -999), (768, -999), (512, 999))), ('sp', ((0, -999), (256, -666), (768, -666), (512, 666))),
        ('sp', ((0, -999), (256, -333), (768, -333), (512, 333))), ('sp', ((0, -999), (512, -999))), ('sp', ((0, -999),)),
        ('sp', ((0, -999), (256, 333), (768, 333), (512, 333))), ('sp', ((0, -999), (256, 666), (768, 666))), ('sp', ((512, -999),)),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -450), (-2, -450))),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -150), (-2, -150))), ('sp', ((0, 1000), (1, -750), (-1, -750), (2, 150), (-2, 150))),
        ('sp', ((0, 1000), (1, -150), (-1, -150), (2, 600), (-2, 600))), ('train', 1, 0, 3000, 3000, 0), ('train', 4, 0, 3000, -1500, 0),
        ('sp', ((0, -666), (256, 999), (768, 999), (512, 333))), ('sp', ((0, 1000), (1, -600), (-1, -600), (2, -450), (-2, -450))),
        ('sp', ((0, 1000), (2, -600), (-2, -600))), ('train', 123, 61, 3000, 1000, 0),
        ('mix', ('train', 1, 0, 20, 20, 0), ('sp', ((0, 1001), (512, -1001)))), ('fb', ((0, 994888909),)), ('fb', ((0, 994888908),)),
        ('fb', ((0, 994888910),)), ('fb', ((512, 994888910),)),
    ),
    2048: (
        ('sp', ((0, -999), (512, -999), (1536, -999), (1024, -999))), ('sp', ((0, -999), (512, -999), (1536, -999))),
        ('sp', ((0, -999), (512, -999), (1536, -999), (1024, 999))), ('sp', ((0, -999), (512, -666), (1536, -666), (1024, 666))),
        ('sp', ((0, -999), (1024, -999))), ('sp', ((0, -999),)), ('sp', ((0, -999), (512, 333), (1536, 333))),
        ('sp', ((0, -999), (512, 333), (1536, 333), (1024, 333))), ('sp', ((1024, -999),)),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -450), (-2, -450))),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -150), (-2, -150))), ('sp', ((0, 1000), (1, -750), (-1, -750), (2, 150), (-2, 150))),
        ('sp', ((0, 1000), (1, -150), (-1, -150), (2, 600), (-2, 600))), ('train', 1, 0, 3000, 3000, 0), ('train', 4, 0, 3000, -1500, 0),
        ('sp', ((0, -666), (512, 999), (1536, 999), (1024, 333))), ('sp', ((0, 1000), (1, -750), (-1, -750), (2, -600), (-2, -600))),
        ('sp', ((0, 1000), (2, -600), (-2, -600))), ('sp', ((0, 1000), (1, 150), (-1, 150), (2, -300), (-2, -300))),
        ('train', 15, 0, 3000, -1500, 0),
        ('mix', ('train', 1, 0, 20, 20, 0), ('sp', ((0, -2002), (512, 1001), (1536, 1001), (1024, 1001)))),
        ('sp', ((0, -333), (896, -666), (960, -666))),
        ('sp', ((416, 333), (672, 666), (1184, 333), (1408, 999), (1696, -666), (1920, 333), (1952, -333))),
        ('sp', ((471, -2247), (719, -1730), (930, 236), (1481, -1715), (1624, 1990), (2024, -231))),
        ('sp', ((71, 308), (561, -2053), (866, -509), (1152, 209), (1230, -1791), (2003, 2100))), ('fb', ((0, 990957763),)),
        ('fb', ((0, 990957762),)), ('fb', ((0, 1050647505),)), ('fb', ((1024, 1051218778),)),
    ),
    4096: (
        ('sp', ((0, -999), (1024, -999), (3072, -999), (2048, -999))), ('sp', ((0, -999), (1024, -999), (3072, -999), (2048, -333))),
        ('sp', ((0, -999), (1024, -999), (3072, -999), (2048, 999))), ('sp', ((0, -999), (1024, -666), (3072, -666), (2048, 666))),
        ('sp', ((0, -999), (1024, -333), (3072, -333), (2048, -666))), ('sp', ((0, -999), (2048, -999))), ('sp', ((0, -999),)),
        ('sp', ((0, -999), (1024, 333), (3072, 333), (2048, 333))), ('sp', ((2048, -999),)),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -450), (-2, -450))),
        ('sp', ((0, 1000), (1, -900), (-1, -900), (2, -150), (-2, -150))), ('sp', ((0, 1000), (1, -750), (-1, -750), (2, 150), (-2, 150))),
        ('sp', ((0, 1000), (1, -150), (-1, -150), (2, 600), (-2, 600))), ('train', 1, 0, 3000, 3000, 0), ('train', 4, 0, 3000, -1500, 0),
        ('sp', ((0, -666), (1024, 999), (3072, 999), (2048, 333))), ('sp', ((0, 1000), (1, -750), (-1, -750), (2, -600), (-2, -600))),
        ('sp', ((0, 1000), (2, -600), (-2, -600))), ('train', 35, 1, 3000, 3000, 0),
        ('mix', ('train', 1, 0, 3, 3, 0), ('sp', ((0, 333), (2048, -333)))), ('sp', ((2624, 333), (2688, -333))),
        ('sp', ((239, 2595), (1360, -2536), (1550, -674), (1666, -1513), (1754, 1747), (2984, 554))),
        ('sp', ((120, 1891), (809, 2850), (1308, 2472), (2061, -692), (2726, 1296), (3217, -2771))),
        ('sp', ((4, 2928), (2655, 1866), (3516, 243))), ('fb', ((0, 986500301),)), ('fb', ((0, 986500300),)), ('fb', ((0, 986500302),)),
        ('fb', ((2048, 986500302),)),
    ),
}
UNREACHED = {
    256: (
        ('flat', 'no peak, the serial sum puts the mean above the bins'), ('tie', -1, 'in'), ('tie', -2, 'in'), ('tie', 1, 'in'),
        ('gate', 'equal'), ('level', 'upper on the mean'), ('mean', 'within rounding, not flat'), ('probe', 'at bin M-2 or M-1'),
        ('probe', 'lb == f0_bin skip'),
    ),
    512: (
        ('flat', 'no peak, the serial sum puts the mean above the bins'), ('tie', -1, 'in'), ('tie', -2, 'in'), ('tie', 1, 'in'),
        ('gate', 'equal'), ('level', 'upper on the mean'), ('mean', 'within rounding, not flat'), ('probe', 'at bin M-2 or M-1'),
        ('probe', 'lb == f0_bin skip'),
    ),
    1024: (
        ('gate', 'equal'), ('level', 'upper on the mean'), ('mean', 'within rounding, not flat'), ('probe', 'at bin M-2 or M-1'),
        ('probe', 'lb == f0_bin skip'),
    ),
    2048: (
        ('gate', 'equal'), ('level', 'upper on the mean'), ('mean', 'within rounding, not flat'), ('probe', 'at bin M-2 or M-1'),
        ('probe', 'lb == f0_bin skip'),
    ),
    4096: (
        ('gate', 'equal'), ('level', 'upper on the mean'), ('mean', 'within rounding, not flat'), ('probe', 'at bin M-2 or M-1'),
        ('probe', 'lb == f0_bin skip'),
    ),
}
UNTOLD = {
    256: (
    ),
    512: (
    ),
    1024: (
    ),
    2048: (
    ),
    4096: (
    ),
}
CRC = {256: 860377023, 512: 839137435, 1024: 3435775128, 2048: 4215608639, 4096: 3841401943}
# END TABLE

_CACHE = {}


def frames(N):
    """[K][N] float32, one frame per entry of CASES[N], the s16-exact ones first (read-only: shared between tests)"""
    if N not in _CACHE:
        out = np.ascontiguousarray(np.stack([synth(N, c) for c in CASES[N]]), f32)
        out.setflags(write=False)
        _CACHE[N] = out
    return _CACHE[N]


def crc(N):
    return zlib.crc32(frames(N).tobytes())


def num_s16(N):
    """the table holds the s16-exact frames first: how many"""
    k = sum(s16_exact(c) for c in CASES[N])
    assert all(s16_exact(c) for c in CASES[N][:k]) and not any(s16_exact(c) for c in CASES[N][k:])
    return k


def as_s16(x):
    """the int16 samples of s16-exact frames"""
    v = np.asarray(x, f32) * f32(32768.0)
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 32767
    return v.astype(np.int16)


def batch_layout(N, only_s16=False):
    """([C][12][N] frames, [K] (channel, frame) of every chosen frame): the K frames (only_s16: the s16-exact ones) laid out twelve per
    channel, the last channel filled up with the first frames again"""
    F = frames(N)
    K = num_s16(N) if only_s16 else F.shape[0]
    C = -(-K // T)
    idx = np.arange(C * T) % K
    return np.ascontiguousarray(F[idx].reshape(C, T, N)), [(k // T, k % T) for k in range(K)]


def hop_layout(N, only_s16=False):
    """([C][24][N/2] hops, [K] (channel, hop) of every chosen frame): channel c streams both halves of its twelve frames one after the
    other, so that every second window is a chosen frame and the windows in between are junctions of two of them"""
    B, where = batch_layout(N, only_s16)
    C = B.shape[0]
    return np.ascontiguousarray(B.reshape(C, 2 * T, N // 2)), [(c, 2 * t + 1) for c, t in where]


def hop_windows(hops):
    """[C][T][N/2] -> the [C][T][N] windows analysed (the first one starts with silence)"""
    C, T_, H = hops.shape
    x = np.concatenate([np.zeros((C, 1, H), hops.dtype), hops], axis=1)
    return np.concatenate([x[:, :-1], x[:, 1:]], axis=2)


_CLASSIFIED = {}


def classified(oracle, N, rate=48000.0):
    """[K] (record, lag, classes) of the chosen frames at one rate, computed once"""
    if (N, rate) not in _CLASSIFIED:
        _CLASSIFIED[N, rate] = [classify(oracle, w, rate) for w in frames(N)]
    return _CLASSIFIED[N, rate]


def held(oracle, N):
    """every class the chosen frames hold, at both rates"""
    out = set()
    for rate in RATES:
        for _, _, cls in classified(oracle, N, rate):
            out |= cls
    return out


# ---- the comparison: the harmonic slots first, with a message that names the frame's classes ----
def assert_held(oracle, got, want, windows, family, what, rate=48000.0):
    """got, want: (raw, smoothed) [C][T][12]; windows [C][T][N]: what every frame analysed.  First the raw HER, OER and inharmonicity of
    every frame, which are exact slots (oracle/ulp.py) -- a failure names the frame's classes -- then the suite's bar on all of it: onset
    and f0 exact, every other slot within the family's ulp budget, raw and smoothed."""
    import signals
    from oracle import fx_oracle as fo
    assert got[0].shape == want[0].shape == windows.shape[:2] + (12,), (got[0].shape, want[0].shape, windows.shape)
    budget = signals.ulp_budget(family)
    d = signals.ulp_distance(got[0][:, :, HER:INHARM + 1], want[0][:, :, HER:INHARM + 1])
    bad = np.argwhere((d > budget[None, None, HER:INHARM + 1]).any(axis=2))
    if bad.size:
        lines = []
        for c, t in bad[:6]:
            _, lag, cls = classify(oracle, windows[c, t], rate)
            lines.append("channel %d frame %d (lag %d): %s -- the oracle's HER, OER, inharmonicity %s, the kernel's %s" % (
                c, t, lag, describe(cls), want[0][c, t, HER:INHARM + 1].tolist(), got[0][c, t, HER:INHARM + 1].tolist()))
        raise AssertionError("%s: raw harmonic slots differ in %d of %d frames\n  %s" % (
            what, len(bad), windows.shape[0] * windows.shape[1], "\n  ".join(lines)))
    for k, name in ((0, "raw"), (1, "smoothed")):
        signals.assert_features_within(got[k], want[k], budget, fo.FEATURE_NAMES, "%s %s" % (what, name))
