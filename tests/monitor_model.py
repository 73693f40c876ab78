"""Host model of the monitor mix (include/fx.h, "THE MIX"): the specification in numpy, one IEEE fp32 operation at a time (numpy fuses
nothing).  mix() is a tick's output vectorised over the samples, sequential over a group's tracks and then over the groups;
mix_naive() the same one sample and one float32 scalar at a time, the definition mix() is held to (tests/test_monitor_cpu.py).  The
other summation orders (`group` other than 64, mix_f64) exist so that the tests can show that their data tells them apart: a kernel
that sums in another order cannot pass.  data() and gains() make that data: magnitudes over four decades, gains in [-2, 2]."""
import numpy as np

GROUP = 64


def mix(x, on, left, right, group=GROUP):
    """x float32 [C][n], the tick's widened samples; on [C]; left, right float32 [C] -> float32 [2][n].  group: tracks per partial sum
    (the specification's is 64; C or more makes the sum flat)."""
    x = np.asarray(x, np.float32)
    C, n = x.shape
    out = np.zeros((2, n), np.float32)
    with np.errstate(all="ignore"):
        for ch, gain in enumerate((np.asarray(left, np.float32), np.asarray(right, np.float32))):
            total = np.zeros(n, np.float32)
            for first in range(0, C, group):
                part = np.zeros(n, np.float32)
                for c in range(first, min(first + group, C)):
                    if on[c]:
                        part = part + gain[c] * x[c]
                total = total + part
            assert total.dtype == np.float32
            out[ch] = total
    return out


def mix_naive(x, on, left, right):
    """the same, one sample at a time with float32 scalars"""
    x = np.asarray(x, np.float32)
    C, n = x.shape
    out = np.zeros((2, n), np.float32)
    with np.errstate(all="ignore"):
        for ch, gain in enumerate((left, right)):
            for i in range(n):
                total = np.float32(0.0)
                for first in range(0, C, GROUP):
                    part = np.float32(0.0)
                    for c in range(first, min(first + GROUP, C)):
                        if on[c]:
                            part = np.float32(part + np.float32(np.float32(gain[c]) * x[c, i]))
                    total = np.float32(total + part)
                out[ch, i] = total
    return out


def mix_f64(x, on, left, right):
    """fl32 of the sum carried in fp64 (products of two floats are exact there): what a "more accurate" kernel would return"""
    x = np.asarray(x, np.float32).astype(np.float64)
    keep = np.asarray(on).astype(bool)
    with np.errstate(all="ignore"):
        return np.stack([(np.asarray(g, np.float32).astype(np.float64)[keep, None] * x[keep]).sum(axis=0) for g in (left, right)]).astype(np.float32)


def data(C, n, seed):
    """float32 [C][n]: random signs, magnitudes 10^u with u uniform in [-4, 0] -- four decades, so that a sum's roundings depend on its order"""
    rng = np.random.default_rng(seed)
    return (rng.choice(np.array([-1.0, 1.0]), (C, n)) * 10.0 ** rng.uniform(-4.0, 0.0, (C, n))).astype(np.float32)


def gains(C, seed):
    """(left, right) float32 [C], uniform in [-2, 2]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, C).astype(np.float32), rng.uniform(-2.0, 2.0, C).astype(np.float32)


def bits_same(a, b):
    """bit for bit, NaNs comparing equal (a NaN's sign and payload are the adder's own)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))
