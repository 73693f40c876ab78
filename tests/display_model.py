"""The audio display's contract (include/fx.h, fx_enable_display) as plain Python: JUCE 4.2.3's AudioVisualiserComponent::ChannelInfo,
one object per track, restated sample by sample -- and, as a second function, the segment-summary combine a parallel form folds with.

Every comparison below is a float32 comparison and every result is one of the operands (no arithmetic), so the bits of a published
level are the bits of a sample: NaN payloads and the sign of a zero included."""
import numpy as np

F32 = np.float32


class Track:
    """levels[L] of (lo, hi), value (lo, hi), sub, next: all zero in a new component"""

    def __init__(self, samples_per_block, length):
        assert 1 <= length and 1 <= samples_per_block
        self.spb = int(samples_per_block)
        self.L = int(length)
        self.levels = np.zeros((self.L, 2), F32)
        self.value = (F32(0.0), F32(0.0))
        self.sub = 0
        self.next = 0

    def push_sample(self, x):
        x = F32(x)
        self.sub -= 1
        if self.sub <= 0:
            self.next %= self.L
            self.levels[self.next, 0], self.levels[self.next, 1] = self.value
            self.next += 1
            self.sub = self.spb
            self.value = (x, x)
        else:
            lo, hi = self.value
            lo2 = lo if lo < x else x               # jmin (x, lo)
            t = hi if x < hi else x                 # jmax (x, hi)
            hi2 = t if lo2 < t else lo2             # Range's constructor
            self.value = (lo2, hi2)

    def push(self, samples):
        with np.errstate(invalid="ignore"):
            for x in np.asarray(samples, F32).ravel():
                self.push_sample(x)

    def clear(self):
        self.levels[:] = 0
        self.value = (F32(0.0), F32(0.0))
        self.sub = 0                                # next stays

    def set_samples_per_block(self, n):
        self.spb = int(n)                           # the running block keeps its sub

    def draw_order(self):
        """[L][2], oldest first: levels[(next + k) % L]"""
        idx = (self.next + np.arange(self.L)) % self.L
        return self.levels[idx].copy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


# ---- the parallel form: a run of samples as (lo, hi, holds a NaN) ----
def single(x):
    x = F32(x)
    return (x, x, bool(np.isnan(x)))


def combine(left, right):
    """the summary of [left run | right run]"""
    if right[2]:
        return right
    with np.errstate(invalid="ignore"):
        lo = left[0] if left[0] < right[0] else right[0]
        hi = left[1] if right[1] < left[1] else right[1]
    return (lo, hi, left[2])


def fold(samples):
    """left-to-right fold of a non-empty run's single samples"""
    s = single(samples[0])
    for x in samples[1:]:
        s = combine(s, single(x))
    return s


def sequential_value(value, samples):
    """`value` after the else-branch of push_sample has taken every sample of the run"""
    t = Track(1 << 30, 1)
    t.value = (F32(value[0]), F32(value[1]))
    t.sub = 1 << 30
    t.push(samples)
    return t.value
