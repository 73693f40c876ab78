"""The tests' model of what the library derives from a feature buffer (include/fx.h: fx_offline_feature_ranges, fx_offline_feature_distribution,
fx_offline_smoothing / fx_offline_smooth_rows) and of fx::FeatureSpace: the reference's arithmetic (ref AudioFeatures.h:208-240, :319-349,
:356-421) restated in numpy -- serial np.float32 sums, np.sort on an integer key -- and held to the reference's unmodified header by
tests/golden/offline/feature_stats.npz (tests/test_offline_stats_cpu.py)."""
import numpy as np

SORT_CHUNK = 8192
SCRATCH_BYTES = 16 << 20
SMOOTHED = 9                    # AudioFeature::NumFeatures - 2 (ref :360)
MAX_DEPTH = 64
F32 = np.float32


def same(a, b):
    """bit for bit; a NaN equals a NaN whatever its sign and payload"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.tobytes() == b.tobytes():
        return True
    if a.dtype.kind != "f":
        return False
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


# ---- getFeatureRange (ref :208-213) with the stand-in's findMinMax ----
def feature_range(row):
    row = np.asarray(row, F32)
    lo = hi = row[0]
    for v in row[1:]:
        if v < lo:
            lo = v
        if v > hi:
            hi = v
    return np.array([lo, hi], F32)


def feature_ranges(rows):
    """rows [R][C][D] -> [R][C][2]"""
    rows = np.asarray(rows, F32)
    out = np.empty(rows.shape[:2] + (2,), F32)
    for r in range(rows.shape[0]):
        for c in range(rows.shape[1]):
            out[r, c] = feature_range(rows[r, c])
    return out


# ---- getDiscreteFeatureDistribution (ref :215-240) ----
def sort_keys(values):
    """the float's bits made monotonic: b ^ 0x80000000 for b >= 0, ~b for b < 0, 0xFFFFFFFF for a NaN"""
    v = np.ascontiguousarray(values, F32)
    b = v.view(np.uint32)
    keys = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    keys[np.isnan(v)] = np.uint32(0xFFFFFFFF)
    return keys


def values_of(keys):
    keys = np.ascontiguousarray(keys, np.uint32)
    return np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32).view(F32)


def sorted_rows(rows):
    """ascending along the last axis, by key"""
    return values_of(np.sort(sort_keys(rows), axis=-1, kind="stable"))


def serial_sums(terms):
    """fl32 sums along the last axis in index order from +0.0f (np.add.accumulate adds one term after the other)"""
    terms = np.asarray(terms, F32)
    lead = np.zeros(terms.shape[:-1] + (1,), F32)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([lead, terms], axis=-1), axis=-1, dtype=F32)[..., -1]


def pairwise_sums(terms):
    """the same terms summed as a balanced tree: what the library must NOT compute"""
    t = np.asarray(terms, F32)
    with np.errstate(all="ignore"):
        while t.shape[-1] > 1:
            if t.shape[-1] & 1:
                t = np.concatenate([t, np.zeros(t.shape[:-1] + (1,), F32)], axis=-1)
            t = (t[..., 0::2] + t[..., 1::2]).astype(F32)
    return t[..., 0] if t.shape[-1] else np.zeros(t.shape[:-1], F32)


def distributions(rows, num_brackets, sums=serial_sums):
    """rows [...][D] -> [...][num_brackets]"""
    rows = np.asarray(rows, F32)
    D, nb = rows.shape[-1], int(num_brackets)
    step = D // nb
    s = sorted_rows(rows)[..., :nb * step].reshape(rows.shape[:-1] + (nb, step))
    with np.errstate(all="ignore"):
        return (sums(s) / F32(step)).astype(F32)


# ---- SmoothedFeatures (ref :356-421), one per channel ----
class Smoothers:
    def __init__(self, num_channels, depth):
        self.C, self.depth = int(num_channels), int(depth)
        self.current = np.zeros((SMOOTHED, self.C), F32)
        self.history = np.zeros((SMOOTHED, self.C, self.depth), F32)

    def update(self, new):
        """new [9][C]: updateValues of every channel's smoother -> current [9][C]"""
        with np.errstate(all="ignore"):
            self.history[..., :-1] = self.history[..., 1:].copy()          # updateHistory, :399-409
            self.history[..., -1] = self.current
            av = serial_sums(self.history)                                  # :413-417
            av = (av / F32(F32(self.depth) + F32(1))).astype(F32)           # :418
            self.current = (av + ((np.asarray(new, F32) - av).astype(F32) * F32(0.5)).astype(F32)).astype(F32)      # :389-393
        return self.current.copy()

    def smooth_rows(self, rows, first=0, count=None):
        """rows [R >= 9][C][D] -> [9][C][count]"""
        rows = np.asarray(rows, F32)
        count = rows.shape[2] - first if count is None else count
        out = np.empty((SMOOTHED, self.C, count), F32)
        for k in range(count):
            out[:, :, k] = self.update(rows[:SMOOTHED, :, first + k])
        return out


# ---- Range<float> as tools/refdiff/juce_standin.h:55-66 states it, and FeatureSpace (ref :319-349) ----
class Range:
    def __init__(self, start=0.0, end=0.0):
        s, e = F32(start), F32(end)
        self.start, self.end = s, (s if e < s else e)

    def set_start(self, s):
        self.start = F32(s)
        if self.end < s:
            self.end = F32(s)

    def set_end(self, e):
        self.end = F32(e)
        if e < self.start:
            self.start = F32(e)

    def pair(self):
        return [self.start, self.end]


class FeatureSpace:
    def __init__(self, attack=None, centroid=None, slope=None, crosses=None):
        self.attack_range = Range() if attack is None else Range(attack, 0.0)               # :331
        self.spectral_centroid_range = centroid or Range()
        self.spectral_slope_range = slope or Range()
        self.zero_crosses_range = crosses or Range()

    @staticmethod
    def compare_and_update_ranges(existing, new):                                           # :337-343
        if new.start < existing.start:
            existing.set_start(new.start)
        if new.end < existing.end:
            existing.set_end(new.end)

    def ranges(self):
        return [self.attack_range, self.spectral_centroid_range, self.spectral_slope_range, self.zero_crosses_range]

    def fold(self, other):
        for mine, theirs in zip(self.ranges(), other.ranges()):
            FeatureSpace.compare_and_update_ranges(mine, theirs)

    def flat(self):
        return np.array([v for r in self.ranges() for v in r.pair()], F32)


def feature_space_folds(spaces):
    """spaces [n][7] (attack, three (start, end)) -> [n][8]: space 0 as constructed and after folding in each later one"""
    spaces = np.asarray(spaces, F32).reshape(-1, 7)
    make = lambda p: FeatureSpace(p[0], Range(p[1], p[2]), Range(p[3], p[4]), Range(p[5], p[6]))
    existing = make(spaces[0])
    out = [existing.flat()]
    for p in spaces[1:]:
        existing.fold(make(p))
        out.append(existing.flat())
    return np.array(out, F32)
