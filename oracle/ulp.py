"""Per-slot ulp budgets of the GPU features against the oracle / the reference's fixtures, and the fp32 ulp distance they
are counted in.  TEST INFRASTRUCTURE ONLY, like the rest of oracle/: tests/signals.py and tools/stress_parity.py judge by
this one table."""
import numpy as np

# Distances in fp32 ulp (ulp_distance); one budget per slot holds for raw and smoothed values alike.  Measured with
# tools/stress_parity.py (profiles/r07_ulp_stress.txt, 2.3e7 frames, every path and window size): only spread ever
# differed.  "default": the one-wavefront kernels; "low_latency": FX_LOW_LATENCY pairs (include/fx.h: sums over bins in
# another order).  Onset and f0 are discrete decisions and exact.  The budget is a regression guard: BASELINE.json's
# 1e-5 relative stays the contract.
SLOTS = ("onset", "rms", "f0", "centroid", "spread", "flatness", "ler", "flux", "slope", "her", "oer", "inharm")
ULP_BUDGET = {
    #              onset rms f0 centroid spread flatness ler flux slope her oer inharm
    "default":     (0,   0,  0, 0,       2,     0,       0,  0,   0,    0,  0,  0),   # spread: raw 1, smoothed 2 ulp measured
    "low_latency": (0,   0,  0, 0,       4,     0,       0,  0,   0,    0,  0,  0),   # spread: raw 1, smoothed 4 ulp measured
}


def ulp_budget(family="default"):
    return np.asarray(ULP_BUDGET[family], np.int64)


ULP_INFINITE = np.int64(1) << 40


def ulp_distance(a, b):
    """fp32 ulp distance, elementwise: the number of representable floats between a and b (+0 and -0 are the same point,
    subnormals count one step each, a sign change counts the steps through zero).  NaN vs NaN and inf vs the same inf are 0;
    NaN vs anything else and inf vs anything else are ULP_INFINITE, beyond every budget."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    oa = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ob = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(oa - ob)
    na, nb = np.isnan(a), np.isnan(b)
    d = np.where(na | nb, np.where(na & nb, 0, ULP_INFINITE), d)
    ia_inf, ib_inf = np.isinf(a), np.isinf(b)
    d = np.where((ia_inf | ib_inf) & ~(na | nb), np.where(a == b, 0, ULP_INFINITE), d)
    return d
