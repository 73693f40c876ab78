"""Frames that put the pitch lag search (PitchAnalyser.h:161-190; LagSearch, LazyLag and the pair kernel in csrc/) on its seams.

The kernels take the cumulative normalised difference 64 samples -- one wavefront -- at a time and hand the running sum, the previous
sample's cnd and `first` from block to block; the 1024-point kernel fetches blocks 2-3 and everything past sample 255 only on demand.
A wrong hand-over shows only when `first` (the first cnd < 0.01 from sample 2 on) or `stop` (where the walk from there stops falling)
sits on lane 62, 63, 0 or 1 of a block, or on sample N-1, where the decision is taken against cnd[N].  Per window size this module holds
one frame per such class, chosen by the oracle alone (tests/golden/make_lag_cases.py is the search; CASES is its table) from four
families of synthetic signals.  Every sample is rounded to s16, so that a last-bit difference of sin between machines cannot move a frame
and the same frames are exact in the s16 sample format.  No file I/O; everything follows from the parameters and seeds, CRC holds the
bytes, and UNREACHED the classes the search looked for and did not find.  tests/test_lag_cases_cpu.py holds the table to its floors;
tests/test_gpu_lag_cases.py runs the frames through every implementation of the search."""
import zlib

import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
T = 12                                                                         # frames per channel of the batch layout
RESIDUES = (62, 63, 0, 1)
THRESHOLD = np.float32(0.01)


# ---- the families ----
def _noise(seed, N):
    return np.random.default_rng(seed).standard_normal(N)


def synth(N, case):
    """one frame [N] float32 of a table entry (family, parameters...): computed in double, rounded to s16, divided by 32768 in fp32"""
    n = np.arange(N, dtype=np.float64)
    fam = case[0]
    if fam == "sine":                                                          # 0.6 sin(2 pi n / P + 0.2) + dc
        _, P, dc = case
        x = 0.6 * np.sin(2.0 * np.pi * n / P + 0.2) + dc
    elif fam == "harm":                                                        # a tone, its octave and noise of sigma 10^e
        _, P, phi, a, e, seed = case
        x = 0.5 * np.sin(2.0 * np.pi * n / P + phi) + a * np.sin(4.0 * np.pi * n / P) + 10.0 ** e * _noise(seed, N)
    elif fam == "long":                                                        # a slow tone (up to 64 windows per period) and a little noise
        _, P, phi, seed = case
        x = 0.6 * np.sin(2.0 * np.pi * n / P + phi) + 1e-3 * _noise(seed, N)
    elif fam == "decay":                                                       # Gaussian noise under exp(-n / tau)
        _, tau, seed = case
        x = 0.25 * _noise(seed, N) * np.exp(-n / tau)
    else:
        raise KeyError(fam)
    v = np.clip(np.rint(x * 32768.0), -32768, 32767)
    return v.astype(np.float32) / np.float32(32768.0)


# ---- the classification, by the oracle's own cnd ----
def oracle_cnd(oracle, window):
    """(the oracle's lag, its cnd [2N]) of one window (lowpass -> bartlett -> forward_real -> estimate_pitch)"""
    window = np.ascontiguousarray(window, np.float32)
    _, lag, cnd = oracle.estimate_pitch(oracle.forward_real(oracle.bartlett(oracle.lowpass(window))))
    return int(lag), cnd


def classify_cnd(cnd, N):
    """(kind, first, stop, lag) of getLagEstimateFromCumulativeDifference (PitchAnalyser.h:161-190, :192-203) on cnd[0 .. N]:
    kind "walk": first = the first s in [2, N) with cnd[s] < 0.01, stop = the first s' >= first with not cnd[s'+1] < cnd[s'], stop < N-1;
    kind "end": the walk ran to stop = N-1 (:178, sample + 1 < numSamples) and is decided against cnd[N];
    either way lag = stop if cnd[stop] <= cnd[stop+1] else stop + 1.
    kind "fallback": no cnd below the threshold; first is None, stop = lag = the first global minimum over [2, N)."""
    below = np.flatnonzero(cnd[2:N] < THRESHOLD)
    if below.size == 0:
        lag = 2 + int(np.argmin(cnd[2:N]))
        return "fallback", None, lag, lag
    first = 2 + int(below[0])
    rising = np.flatnonzero(~(cnd[first + 1:N] < cnd[first:N - 1]))
    stop = first + int(rising[0]) if rising.size else N - 1
    lag = stop if cnd[stop] <= cnd[stop + 1] else stop + 1
    return ("end" if stop == N - 1 else "walk"), first, stop, lag


def classify(oracle, window):
    """classify_cnd of the oracle's cnd of one window [N]"""
    return classify_cnd(oracle_cnd(oracle, window)[1], len(window))


def classes(N, kind, first, stop, lag):
    """the classes of one classified frame, as a set of tuples:
    ("cell", residue, block)  stop = 64 * block + residue with the residue one of RESIDUES (the walk to N-1 is the cell (63, N/64 - 1))
    ("first63",)              first on lane 63 and stop in a later block: the kernel's walk mask is empty in first's block (k0 >= 64)
    ("first0",)               first on lane 0 (k0 = 1)
    ("first2",)               first = 2, the first sample the search may take (block 0's own mask)
    ("stop=first",)           the walk does not move
    ("cross", 0 | 1 | 2)      block boundaries between first and stop; 2 stands for two or more
    ("end", lag)              the walk to N-1, lag N-1 or N
    ("fallback", block)       the global-minimum fallback, with the block that holds the minimum"""
    if kind == "fallback":
        return {("fallback", stop // 64)}
    out = {("cross", min(2, stop // 64 - first // 64))}
    if stop % 64 in RESIDUES:
        out.add(("cell", stop % 64, stop // 64))
    if first % 64 == 63 and stop // 64 > first // 64:
        out.add(("first63",))
    if first % 64 == 0:
        out.add(("first0",))
    if first == 2:
        out.add(("first2",))
    if stop == first:
        out.add(("stop=first",))
    if kind == "end":
        out.add(("end", lag))
    return out


def all_cells(N):
    return {("cell", r, b) for b in range(N // 64) for r in RESIDUES}


def describe(N, kind, first, stop, lag):
    """what a failure message says of a frame"""
    if kind == "fallback":
        return "fallback, minimum at lane %d of block %d (lag %d)" % (stop % 64, stop // 64, lag)
    return "%s, first %d (lane %d of block %d), stop %d (lane %d of block %d), lag %d" % (
        kind, first, first % 64, first // 64, stop, stop % 64, stop // 64, lag)


# ---- the table: tests/golden/make_lag_cases.py prints it ----
# What UNREACHED lists, and why it is believed to stay out of reach of frames like these:
#   ("end", N-1)       v[N] is N times the square of imag[0] of the inverse transform of a real sequence, which is exactly 0 (only unit
#                      twiddles meet at output 0), so cnd[N] is 0 on every frame and the walk to N-1 answers N unless cnd[N-1] is 0 too --
#                      an exact zero of the autocorrelation at N-1 reached by a strictly falling cnd.  Not found among s16 frames; the
#                      subnormal levels of tests/level_cases.py, where v underflows, are where it could happen.
#   ("fallback", None) no fallback at all at 512 points and more: cnd[s] is about 2 / s for a smooth autocorrelation and passes the
#                      threshold near s = 200 (tests/test_levels_cpu.py); the short bursts tried here do not keep it up either.
#   the high cells     the walk has to fall without a break from `first` (near 200 at the latest) to the tone's period; in the
#                      highest blocks no candidate did (what breaks the fall there first was not looked into).
CASES = {
    256: (
        ('sine', 8.0, 0.0), ('sine', 8.0, 0.3), ('sine', 37.0, 0.3), ('sine', 42.0, 0.3), ('sine', 43.0, 0.3), ('sine', 82.0, 0.3),
        ('sine', 121.0, 0.3), ('sine', 134.0, 0.3), ('sine', 140.0, 0.3), ('sine', 141.0, 0.3), ('sine', 143.0, 0.3), ('sine', 146.0, 0.3),
        ('sine', 224.0, 0.3), ('sine', 234.0, 0.3), ('sine', 251.0, 0.3), ('sine', 253.0, 0.3), ('sine', 268.0, 0.3), ('sine', 287.0, 0.3),
        ('sine', 333.0, 0.0), ('harm', 264.773, 0.009, 0.171, -3.94, 650),
    ),
    512: (
        ('sine', 8.0, 0.0), ('sine', 8.0, 0.3), ('sine', 27.0, 0.3), ('sine', 51.0, 0.3), ('sine', 57.0, 0.3), ('sine', 74.0, 0.3),
        ('sine', 84.0, 0.3), ('sine', 101.0, 0.3), ('sine', 124.0, 0.3), ('sine', 125.0, 0.3), ('sine', 139.0, 0.3), ('sine', 159.0, 0.3),
        ('sine', 166.0, 0.3), ('sine', 168.0, 0.3), ('sine', 182.0, 0.3), ('sine', 256.0, 0.0), ('sine', 270.0, 0.3), ('sine', 286.0, 0.3),
        ('sine', 287.0, 0.3), ('sine', 468.0, 0.3), ('sine', 644.0, 0.0), ('sine', 648.0, 0.0), ('sine', 651.0, 0.0),
        ('harm', 1566.132, 3.722, 0.359, -3.55, 428), ('harm', 640.808, 5.125, 0.329, -3.03, 1722),
        ('harm', 845.757, 0.395, 0.448, -3.32, 2367), ('harm', 1973.004, 3.28, 0.378, -1.81, 3032),
        ('harm', 1371.745, 4.658, 0.185, -3.25, 5875),
    ),
    1024: (
        ('sine', 8.0, 0.0), ('sine', 8.0, 0.3), ('sine', 45.0, 0.3), ('sine', 51.0, 0.3), ('sine', 54.0, 0.3), ('sine', 85.0, 0.3),
        ('sine', 126.0, 0.3), ('sine', 127.0, 0.3), ('sine', 132.0, 0.3), ('sine', 164.0, 0.3), ('sine', 169.0, 0.3), ('sine', 184.0, 0.3),
        ('sine', 205.0, 0.3), ('sine', 212.0, 0.3), ('sine', 218.0, 0.3), ('sine', 241.0, 0.3), ('sine', 250.0, 0.3), ('sine', 337.0, 0.3),
        ('sine', 339.0, 0.3), ('sine', 364.0, 0.3), ('sine', 460.0, 0.3), ('sine', 483.0, 0.3), ('sine', 503.0, 0.0), ('sine', 544.0, 0.3),
        ('sine', 573.0, 0.3), ('sine', 645.0, 0.3), ('sine', 960.0, 0.0), ('sine', 961.0, 0.3), ('sine', 1035.0, 0.3),
        ('sine', 1047.0, 0.3), ('sine', 1132.0, 0.0), ('sine', 1135.0, 0.0), ('sine', 1293.0, 0.0), ('sine', 1295.0, 0.0),
        ('sine', 1297.0, 0.0), ('sine', 1300.0, 0.0), ('sine', 1413.0, 0.0), ('sine', 1415.0, 0.0), ('sine', 1416.0, 0.0),
        ('sine', 1417.0, 0.0), ('harm', 1728.972, 0.159, 0.449, -2.38, 567), ('harm', 3573.971, 4.463, 0.301, -3.93, 701),
        ('harm', 1848.329, 5.02, 0.477, -3.14, 842), ('harm', 3129.244, 4.334, 0.37, -2.78, 1956),
        ('harm', 2967.421, 2.633, 0.181, -3.55, 2677), ('harm', 2887.616, 3.053, 0.43, -1.8, 4255),
        ('harm', 2800.942, 4.499, 0.252, -2.0, 5583),
    ),
    2048: (
        ('sine', 8.0, 0.0), ('sine', 8.0, 0.3), ('sine', 36.0, 0.3), ('sine', 42.0, 0.3), ('sine', 85.0, 0.3), ('sine', 86.0, 0.3),
        ('sine', 108.0, 0.3), ('sine', 127.0, 0.3), ('sine', 130.0, 0.3), ('sine', 155.0, 0.3), ('sine', 159.0, 0.3), ('sine', 208.0, 0.3),
        ('sine', 230.0, 0.3), ('sine', 253.0, 0.3), ('sine', 293.0, 0.3), ('sine', 339.0, 0.3), ('sine', 368.0, 0.3), ('sine', 438.0, 0.3),
        ('sine', 484.0, 0.3), ('sine', 501.0, 0.3), ('sine', 636.0, 0.3), ('sine', 643.0, 0.3), ('sine', 646.0, 0.3), ('sine', 650.0, 0.3),
        ('sine', 678.0, 0.3), ('sine', 679.0, 0.3), ('sine', 727.0, 0.3), ('sine', 757.0, 0.0), ('sine', 919.0, 0.3), ('sine', 966.0, 0.3),
        ('sine', 967.0, 0.3), ('sine', 968.0, 0.3), ('sine', 1015.0, 0.0), ('sine', 1081.0, 0.3), ('sine', 1084.0, 0.3),
        ('sine', 1097.0, 0.3), ('sine', 1121.0, 0.3), ('sine', 1144.0, 0.3), ('sine', 1231.0, 0.3), ('sine', 1284.0, 0.3),
        ('sine', 1290.0, 0.3), ('sine', 1674.0, 0.3), ('sine', 1676.0, 0.3), ('sine', 1677.0, 0.3), ('sine', 1900.0, 0.3),
        ('sine', 1901.0, 0.3), ('sine', 1922.0, 0.3), ('sine', 1959.0, 0.3), ('sine', 1960.0, 0.3), ('sine', 1962.0, 0.3),
        ('sine', 1963.0, 0.3), ('sine', 2063.0, 0.3), ('sine', 2067.0, 0.3), ('sine', 2083.0, 0.3), ('sine', 2094.0, 0.3),
        ('sine', 2099.0, 0.0), ('sine', 2120.0, 0.3), ('sine', 2121.0, 0.3), ('sine', 2270.0, 0.0), ('sine', 2273.0, 0.0),
        ('sine', 2278.0, 0.0), ('sine', 2437.0, 0.0), ('sine', 2439.0, 0.0), ('sine', 2442.0, 0.0), ('sine', 2444.0, 0.0),
        ('sine', 2591.0, 0.0), ('sine', 2593.0, 0.0), ('sine', 2595.0, 0.0), ('sine', 2597.0, 0.0), ('sine', 2725.0, 0.0),
        ('sine', 2727.0, 0.0), ('sine', 2728.0, 0.0), ('sine', 2730.0, 0.0), ('sine', 2829.0, 0.0), ('sine', 2831.0, 0.0),
        ('sine', 2832.0, 0.0), ('sine', 2834.0, 0.0), ('sine', 2896.0, 0.0), ('sine', 2897.0, 0.0), ('sine', 2898.0, 0.0),
        ('harm', 5708.66, 3.122, 0.396, -3.53, 17), ('sine', 1088.1, 0.3), ('sine', 1088.2, 0.3), ('sine', 1088.3, 0.3),
        ('sine', 1088.4, 0.3),
    ),
    4096: (
        ('sine', 8.0, 0.0), ('sine', 8.0, 0.3), ('sine', 47.0, 0.3), ('sine', 84.0, 0.3), ('sine', 98.0, 0.3), ('sine', 129.0, 0.3),
        ('sine', 138.0, 0.3), ('sine', 148.0, 0.3), ('sine', 158.0, 0.3), ('sine', 229.0, 0.3), ('sine', 259.0, 0.0), ('sine', 260.0, 0.3),
        ('sine', 292.0, 0.3), ('sine', 293.0, 0.3), ('sine', 310.0, 0.3), ('sine', 324.0, 0.3), ('sine', 342.0, 0.3), ('sine', 383.0, 0.3),
        ('sine', 402.0, 0.3), ('sine', 411.0, 0.3), ('sine', 416.0, 0.3), ('sine', 454.0, 0.3), ('sine', 461.0, 0.3), ('sine', 507.0, 0.3),
        ('sine', 541.0, 0.3), ('sine', 657.0, 0.3), ('sine', 680.0, 0.3), ('sine', 736.0, 0.3), ('sine', 770.0, 0.0), ('sine', 785.0, 0.3),
        ('sine', 811.0, 0.3), ('sine', 819.0, 0.3), ('sine', 820.0, 0.3), ('sine', 838.0, 0.3), ('sine', 894.0, 0.3), ('sine', 896.0, 0.3),
        ('sine', 939.0, 0.3), ('sine', 968.0, 0.3), ('sine', 1003.0, 0.3), ('sine', 1004.0, 0.3), ('sine', 1013.0, 0.3),
        ('sine', 1028.0, 0.3), ('sine', 1068.0, 0.3), ('sine', 1073.0, 0.3), ('sine', 1252.0, 0.3), ('sine', 1282.0, 0.3),
        ('sine', 1288.0, 0.3), ('sine', 1293.0, 0.3), ('sine', 1297.0, 0.3), ('sine', 1332.0, 0.3), ('sine', 1358.0, 0.3),
        ('sine', 1454.0, 0.3), ('sine', 1455.0, 0.3), ('sine', 1523.0, 0.0), ('sine', 1527.0, 0.0), ('sine', 1530.0, 0.3),
        ('sine', 1589.0, 0.3), ('sine', 1812.0, 0.3), ('sine', 1839.0, 0.3), ('sine', 1855.0, 0.3), ('sine', 1864.0, 0.3),
        ('sine', 1877.0, 0.3), ('sine', 1878.0, 0.3), ('sine', 1880.0, 0.3), ('sine', 1881.0, 0.3), ('sine', 1934.0, 0.3),
        ('sine', 1935.0, 0.3), ('sine', 1959.0, 0.3), ('sine', 1960.0, 0.3), ('sine', 1973.0, 0.3), ('sine', 1981.0, 0.3),
        ('sine', 2027.0, 0.0), ('sine', 2030.0, 0.0), ('sine', 2130.0, 0.3), ('sine', 2165.0, 0.3), ('sine', 2172.0, 0.3),
        ('sine', 2177.0, 0.3), ('sine', 2194.0, 0.3), ('sine', 2214.0, 0.3), ('sine', 2223.0, 0.3), ('sine', 2241.0, 0.3),
        ('sine', 2289.0, 0.3), ('sine', 2495.0, 0.3), ('sine', 2497.0, 0.3), ('sine', 2575.0, 0.3), ('sine', 3245.0, 0.0),
        ('sine', 3351.0, 0.3), ('sine', 3353.0, 0.3), ('sine', 3448.0, 0.0), ('sine', 3470.0, 0.3), ('sine', 3801.0, 0.3),
        ('sine', 3828.0, 0.3), ('sine', 3841.0, 0.0), ('sine', 3844.0, 0.3), ('sine', 3854.0, 0.3), ('sine', 3921.0, 0.3),
        ('sine', 3922.0, 0.3), ('sine', 3924.0, 0.3), ('sine', 3925.0, 0.3), ('sine', 4003.0, 0.3), ('sine', 4004.0, 0.3),
        ('sine', 4005.0, 0.3), ('sine', 4006.0, 0.3), ('sine', 4151.0, 0.3), ('sine', 4155.0, 0.3), ('sine', 4160.0, 0.3),
        ('sine', 4175.0, 0.3), ('sine', 4188.0, 0.3), ('sine', 4201.0, 0.0), ('sine', 4208.0, 0.3), ('sine', 4240.0, 0.3),
        ('sine', 4241.0, 0.3), ('sine', 4242.0, 0.3), ('sine', 4302.0, 0.3), ('sine', 4303.0, 0.3), ('sine', 4379.0, 0.0),
        ('sine', 4549.0, 0.0), ('sine', 4554.0, 0.0), ('sine', 4715.0, 0.0), ('sine', 4717.0, 0.0), ('sine', 4723.0, 0.0),
        ('sine', 4879.0, 0.0), ('sine', 4881.0, 0.0), ('sine', 4884.0, 0.0), ('sine', 5037.0, 0.0), ('sine', 5039.0, 0.0),
        ('sine', 5041.0, 0.0), ('sine', 5044.0, 0.0), ('sine', 5186.0, 0.0), ('sine', 5189.0, 0.0), ('sine', 5191.0, 0.0),
        ('sine', 5193.0, 0.0), ('sine', 5326.0, 0.0), ('sine', 5328.0, 0.0), ('sine', 5333.0, 0.0), ('sine', 5454.0, 0.0),
        ('sine', 5456.0, 0.0), ('sine', 5457.0, 0.0), ('sine', 5459.0, 0.0), ('sine', 5566.0, 0.0), ('sine', 5568.0, 0.0),
        ('sine', 5570.0, 0.0), ('sine', 5571.0, 0.0), ('sine', 5662.0, 0.0), ('sine', 5663.0, 0.0), ('sine', 5665.0, 0.0),
        ('sine', 5666.0, 0.0), ('sine', 5738.0, 0.0), ('sine', 5739.0, 0.0), ('sine', 5740.0, 0.0), ('sine', 5741.0, 0.0),
        ('sine', 5795.0, 0.0), ('sine', 5796.0, 0.0), ('sine', 5828.0, 0.0), ('harm', 6780.697, 5.876, 0.455, -3.04, 418),
        ('harm', 11758.265, 3.871, 0.395, -3.28, 920), ('long', 5828.241, 6.095, 868), ('sine', 2176.7, 0.3), ('sine', 2176.8, 0.3),
        ('sine', 2176.9, 0.3),
    ),
}
UNREACHED = {
    256: (
        ('cell', 62, 3), ('end', 255), ('fallback', 0), ('fallback', 1),
    ),
    512: (
        ('cell', 0, 7), ('cell', 1, 5), ('cell', 1, 7), ('cell', 62, 4), ('cell', 62, 6), ('cell', 62, 7), ('cell', 63, 6), ('end', 511),
        ('fallback', None),
    ),
    1024: (
        ('cell', 0, 10), ('cell', 0, 12), ('cell', 0, 13), ('cell', 0, 14), ('cell', 0, 15), ('cell', 1, 10), ('cell', 1, 14),
        ('cell', 1, 15), ('cell', 1, 9), ('cell', 62, 10), ('cell', 62, 12), ('cell', 62, 13), ('cell', 62, 14), ('cell', 62, 15),
        ('cell', 62, 9), ('cell', 63, 11), ('cell', 63, 12), ('cell', 63, 13), ('cell', 63, 14), ('cell', 63, 8), ('end', 1023),
        ('fallback', None),
    ),
    2048: (
        ('cell', 0, 18), ('cell', 0, 19), ('cell', 0, 20), ('cell', 0, 26), ('cell', 0, 27), ('cell', 0, 28), ('cell', 0, 29),
        ('cell', 0, 30), ('cell', 0, 31), ('cell', 1, 15), ('cell', 1, 17), ('cell', 1, 18), ('cell', 1, 19), ('cell', 1, 20),
        ('cell', 1, 21), ('cell', 1, 24), ('cell', 1, 26), ('cell', 1, 27), ('cell', 1, 28), ('cell', 1, 29), ('cell', 1, 30),
        ('cell', 1, 31), ('cell', 62, 16), ('cell', 62, 17), ('cell', 62, 18), ('cell', 62, 19), ('cell', 62, 20), ('cell', 62, 22),
        ('cell', 62, 23), ('cell', 62, 25), ('cell', 62, 26), ('cell', 62, 27), ('cell', 62, 28), ('cell', 62, 29), ('cell', 62, 30),
        ('cell', 62, 31), ('cell', 63, 20), ('cell', 63, 22), ('cell', 63, 23), ('cell', 63, 25), ('cell', 63, 26), ('cell', 63, 27),
        ('cell', 63, 28), ('cell', 63, 29), ('cell', 63, 30), ('end', 2047), ('fallback', None),
    ),
    4096: (
        ('cell', 0, 30), ('cell', 0, 34), ('cell', 0, 37), ('cell', 0, 38), ('cell', 0, 39), ('cell', 0, 40), ('cell', 0, 41),
        ('cell', 0, 42), ('cell', 0, 43), ('cell', 0, 45), ('cell', 0, 46), ('cell', 0, 47), ('cell', 0, 48), ('cell', 0, 49),
        ('cell', 0, 52), ('cell', 0, 53), ('cell', 0, 54), ('cell', 0, 55), ('cell', 0, 56), ('cell', 0, 57), ('cell', 0, 58),
        ('cell', 0, 59), ('cell', 0, 60), ('cell', 0, 61), ('cell', 0, 62), ('cell', 0, 63), ('cell', 1, 35), ('cell', 1, 36),
        ('cell', 1, 38), ('cell', 1, 39), ('cell', 1, 40), ('cell', 1, 42), ('cell', 1, 43), ('cell', 1, 45), ('cell', 1, 46),
        ('cell', 1, 47), ('cell', 1, 48), ('cell', 1, 49), ('cell', 1, 52), ('cell', 1, 53), ('cell', 1, 54), ('cell', 1, 55),
        ('cell', 1, 56), ('cell', 1, 57), ('cell', 1, 58), ('cell', 1, 59), ('cell', 1, 60), ('cell', 1, 61), ('cell', 1, 62),
        ('cell', 1, 63), ('cell', 62, 30), ('cell', 62, 34), ('cell', 62, 35), ('cell', 62, 36), ('cell', 62, 37), ('cell', 62, 38),
        ('cell', 62, 39), ('cell', 62, 41), ('cell', 62, 42), ('cell', 62, 44), ('cell', 62, 45), ('cell', 62, 46), ('cell', 62, 47),
        ('cell', 62, 48), ('cell', 62, 51), ('cell', 62, 52), ('cell', 62, 53), ('cell', 62, 54), ('cell', 62, 55), ('cell', 62, 56),
        ('cell', 62, 57), ('cell', 62, 58), ('cell', 62, 59), ('cell', 62, 60), ('cell', 62, 61), ('cell', 62, 62), ('cell', 62, 63),
        ('cell', 63, 34), ('cell', 63, 35), ('cell', 63, 36), ('cell', 63, 37), ('cell', 63, 41), ('cell', 63, 44), ('cell', 63, 46),
        ('cell', 63, 47), ('cell', 63, 48), ('cell', 63, 51), ('cell', 63, 52), ('cell', 63, 53), ('cell', 63, 54), ('cell', 63, 55),
        ('cell', 63, 56), ('cell', 63, 57), ('cell', 63, 58), ('cell', 63, 59), ('cell', 63, 60), ('cell', 63, 61), ('cell', 63, 62),
        ('end', 4095), ('fallback', None),
    ),
}
CRC = {256: 2457589269, 512: 844087989, 1024: 1387446063, 2048: 2820420811, 4096: 595866662}

_CACHE = {}


def frames(N):
    """[K][N] float32, one frame per entry of CASES[N] (read-only: shared between tests)"""
    if N not in _CACHE:
        out = np.ascontiguousarray(np.stack([synth(N, c) for c in CASES[N]]), np.float32)
        out.setflags(write=False)
        _CACHE[N] = out
    return _CACHE[N]


def crc(N):
    return zlib.crc32(frames(N).tobytes())


def as_s16(x):
    """the int16 samples the frames were rounded to (exact)"""
    v = np.asarray(x, np.float32) * np.float32(32768.0)
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 32768
    return v.astype(np.int16)


def batch_layout(N):
    """([C][12][N] frames, [K] (channel, frame) of every chosen frame): the K frames laid out twelve per channel, the last channel filled
    up with the first frames again"""
    F = frames(N)
    K = F.shape[0]
    C = -(-K // T)
    idx = np.arange(C * T) % K
    return np.ascontiguousarray(F[idx].reshape(C, T, N)), [(k // T, k % T) for k in range(K)]


def hop_layout(N):
    """([C][24][N/2] hops, [K] (channel, hop) of every chosen frame): channel c streams both halves of its twelve frames one after the
    other, so that every second window is a chosen frame and the windows in between are junctions of two of them"""
    B, where = batch_layout(N)
    C = B.shape[0]
    return np.ascontiguousarray(B.reshape(C, 2 * T, N // 2)), [(c, 2 * t + 1) for c, t in where]


def hop_windows(hops):
    """[C][T][N/2] -> the [C][T][N] windows analysed (the first one starts with silence)"""
    C, T, H = hops.shape
    x = np.concatenate([np.zeros((C, 1, H), hops.dtype), hops], axis=1)
    return np.concatenate([x[:, :-1], x[:, 1:]], axis=2)


# ---- the comparison: raw f0 first, with a message that says where the search went ----
F0 = 2


def lag_of(slot, rate=48000.0):
    """the lag behind a raw f0 slot (f0 / 5000 with f0 = sample_rate / lag), None if the slot holds none"""
    slot = float(slot)
    return int(round(rate / (slot * 5000.0))) if np.isfinite(slot) and slot > 0 else None


def assert_held(oracle, got, want, windows, family, what):
    """got, want: (raw, smoothed) [C][T][12]; windows [C][T][N]: what every frame analysed.  First the raw f0 of every frame -- a
    failure names the frame's class, first, stop, and the oracle's and the kernel's lag -- then the suite's bar on all of it: onset and
    f0 exact, every other slot within the family's ulp budget, raw and smoothed."""
    import signals
    from oracle import fx_oracle as fo
    from rate_cases import same_bits
    N = windows.shape[-1]
    assert got[0].shape == want[0].shape == windows.shape[:2] + (12,), (got[0].shape, want[0].shape, windows.shape)
    bad = np.argwhere(~same_bits(got[0][:, :, F0], want[0][:, :, F0]))
    if bad.size:
        lines = ["channel %d frame %d: %s -- the oracle's lag %s, the kernel answered %s" % (
            c, t, describe(N, *classify(oracle, windows[c, t])), lag_of(want[0][c, t, F0]), lag_of(got[0][c, t, F0])) for c, t in bad[:6]]
        raise AssertionError("%s: raw f0 differs in %d of %d frames\n  %s" % (what, len(bad), windows.shape[0] * windows.shape[1], "\n  ".join(lines)))
    for k, name in ((0, "raw"), (1, "smoothed")):
        signals.assert_features_within(got[k], want[k], signals.ulp_budget(family), fo.FEATURE_NAMES, "%s %s" % (what, name))


_CLASSIFIED = {}


def classified(oracle, N):
    """[K] (kind, first, stop, lag) of the chosen frames, computed once"""
    if N not in _CLASSIFIED:
        _CLASSIFIED[N] = [classify(oracle, w) for w in frames(N)]
    return _CLASSIFIED[N]
