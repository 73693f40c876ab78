"""Inputs that put the legacy offline analyser (ref AudioAnalysis.h; csrc/fx_offline.hip, oracle/fx_offline.c) on the edges of its discrete
decisions: both sides of every gate and threshold, equal maxima and equal weights (the first must win), and non-finite values wherever
a comparison meets them.  tests/test_offline.py holds the arithmetic of ordinary inputs; this file holds the decisions.

No file I/O; everything follows from seeds and constants.  Every case is a dict with a `label`, the inputs, and the claim it is built
for -- which side of which comparison it lands on, or which index must win -- written down from the reference's text, not from any
implementation's output.  tests/test_offline_edges_cpu.py asserts every claim with the oracle; the expected outputs themselves are the
reference header's (tests/golden/offline/edge_cases.npz, made by tests/golden/make_offline_edge_cases.py).

Sizes are the smallest at which the kernels' structure shows: 256 threads a block, 64 lanes a wave, serial sums in batches of eight; bin
counts and envelope lengths from 1, 4, 5, 63-65, 255-257, 513, 1025, and one 4097-bin case for each kernel with dynamic LDS."""
import numpy as np

F32 = np.float32
NAN, INF = float("nan"), float("inf")
MAX_BINS = 4097


def up(x):
    return np.nextafter(F32(x), F32(INF))


def down(x):
    return np.nextafter(F32(x), F32(-INF))


def serial_sum(values):
    """the reference's sum: doubles added in index order from 0.0"""
    s = 0.0
    for v in values:
        s += float(v)
    return s


def serial_product(values):
    p = 1.0
    for v in values:
        p *= float(v)
    return p


def gate_terms(target=0.001):
    """float32 magnitudes whose serial fp64 sum sits one fp64 step under `target`, exactly on it, and one step over it: each term is the
    remainder so far rounded down to a float32, so every partial sum is exact.  -> (under, on, over), three float32 vectors."""
    def exactly(total):
        terms, rest = [], total
        while rest > 0.0:
            t = F32(rest)
            if float(t) > rest:
                t = np.nextafter(t, F32(0))
            terms.append(t)
            rest -= float(t)
        assert serial_sum(terms) == total
        return np.array(terms, F32)
    return exactly(float(np.nextafter(target, 0.0))), exactly(target), exactly(float(np.nextafter(target, INF)))


def sparse(num_bins, bins):
    """zeros but for {bin: magnitude}"""
    m = np.zeros(num_bins, F32)
    for b, v in bins.items():
        m[b] = v
    return m


# ---- zero crossings (ref :517-541): a pair counts if first > 0 and (first - second) > first, or first < 0 and (first - second) < first ----
# (first, second, counted) -- fp32 arithmetic as written: 1 + 2^-24 is a tie and rounds to the even 1.0, 1 + 2^-23 is the next float
ZC_PAIRS = [
    (1.0, -2.0 ** -25, 0), (1.0, -2.0 ** -24, 0), (1.0, -2.0 ** -23, 1),
    (-1.0, 2.0 ** -25, 0), (-1.0, 2.0 ** -24, 0), (-1.0, 2.0 ** -23, 1),
    (1.0, 0.0, 0), (1.0, -0.0, 0), (-1.0, 0.0, 0), (-1.0, -0.0, 0),               # first - 0 == first: not greater
    (0.0, -1.0, 0), (-0.0, 1.0, 0), (0.0, 1.0, 0), (-0.0, -1.0, 0),               # a zero is neither > 0 nor < 0
    (2.0 ** -149, -2.0 ** -149, 1), (-2.0 ** -149, 2.0 ** -149, 1),               # subnormals are not flushed: 2^-148 > 2^-149
    (2.0 ** -149, 2.0 ** -149, 0), (2.0 ** -140, -2.0 ** -149, 1), (-2.0 ** -127, 2.0 ** -130, 1),
    (INF, 1.0, 0), (INF, -1.0, 0), (INF, -INF, 0), (INF, INF, 0),                 # inf - x is inf (or NaN): never > inf
    (-INF, 1.0, 0), (-INF, INF, 0), (-INF, -INF, 0),
    (1.0, -INF, 1), (1.0, INF, 0), (-1.0, INF, 1), (-1.0, -INF, 0),
    (NAN, 1.0, 0), (NAN, -1.0, 0), (1.0, NAN, 0), (-1.0, NAN, 0), (NAN, NAN, 0),
    (1.0, -1.0, 1), (-1.0, 1.0, 1), (1.0, 0.5, 0), (-1.0, -0.5, 0),
]
ZC_STEPS = (1, 2, 256, 257, 258)
ZC_DOWNSAMPLES = 3


def zero_cross_cases():
    """-> [{label, audio [C][S], num_downsamples, counts [C][num_downsamples] (the pairs that count in each step)}]"""
    cases = []
    pairs = np.array([[a, b] for a, b, _ in ZC_PAIRS], F32).reshape(1, -1)          # step 2: every step is one pair
    cases.append(dict(label="pairs", audio=pairs, num_downsamples=len(ZC_PAIRS), counts=np.array([[c for _, _, c in ZC_PAIRS]])))
    for step in ZC_STEPS:
        nd, left = ZC_DOWNSAMPLES, 2                                               # num_samples = nd * step + 2: the int division drops the two
        S = nd * step + left
        s = np.arange(nd * step)
        straddle = np.where((s // step) % 2 == 0, 1.0, -1.0)                       # the sign changes between steps only: never counted
        last_pair = np.where(s % step == step - 1, -1.0, 1.0)                      # (+1, -1) on s = step - 2 counts; (-1, +1) straddles the boundary
        every = np.where(s % 2 == 0, 1.0, -1.0)                                    # every pair inside a step counts: step - 1
        audio = np.full((3, S), NAN, F32)                                          # the leftover samples hold NaNs: never read into a count
        audio[:, :nd * step] = np.stack([straddle, last_pair, every])
        counts = np.array([[0] * nd, [1 if step >= 2 else 0] * nd, [step - 1] * nd])
        cases.append(dict(label="step %d" % step, audio=audio, num_downsamples=nd, counts=counts))
    return cases


# ---- log attack time (ref :611-622): the first index holding the envelope's maximum; the maximum starts from envelope[0] and moves on `>` only ----
def attack_cases():
    """-> [{label, env [n], num_input_samples, num_downsamples, sample_rate, index (the i of :616-618; n when no entry equals the maximum)}]"""
    rng = np.random.default_rng(20261019)
    cases = []

    def add(label, env, index, rate=(441, 44100)):
        env = np.asarray(env, F32)
        n = env.shape[0]
        cases.append(dict(label=label, env=env, num_input_samples=n * rate[0], num_downsamples=n, sample_rate=rate[1], index=index))

    def base(n):
        return (rng.random(n) * 4.0 + 0.5).astype(F32)                             # everything in [0.5, 4.5)

    for n in (1, 255, 256, 257, 513):
        e = base(n); e[0] = 50.0
        add("n %d max at 0" % n, e, 0)
        e = base(n); e[n - 1] = 50.0
        add("n %d max at n-1" % n, e, n - 1, rate=(48, 48000))
    for at in (255, 256):
        e = base(513); e[at] = 50.0
        add("n 513 max at %d" % at, e, at)
    for k in (3, 200):
        for gap in (1, 64, 256):                                                    # another lane, another wave, the same thread's next stride
            e = base(513); e[k] = e[k + gap] = 50.0
            add("equal maxima at %d and %d" % (k, k + gap), e, k)
    for t, n in ((5, 513), (1, 513), (255, 513), (5, 1025)):                        # a NaN early in a thread's stride must not hide the maximum behind it
        e = base(n); e[t] = NAN; e[t + 256] = 50.0
        add("n %d NaN at %d max at %d" % (n, t, t + 256), e, t + 256)
    e = base(1025); e[5] = NAN; e[5 + 512] = 50.0
    add("n 1025 NaN at 5 max at 517", e, 517)
    e = base(513); e[1:256] = NAN; e[300] = 50.0; e[400] = 50.0
    add("NaNs at 1..255 max at 300 and 400", e, 300)
    e = base(257); e[0] = NAN; e[100] = 50.0
    add("NaN at 0", e, 257)                                                        # the maximum stays NaN and equals nothing: i = n
    e = np.full(1, NAN, F32)
    add("n 1 NaN", e, 1)
    e = np.full(257, NAN, F32); e[0] = 2.0
    add("all NaN but entry 0", e, 0)
    e = np.full(257, NAN, F32); e[7] = 2.0
    add("all NaN but entry 7", e, 257)
    add("all -inf", np.full(257, -INF, F32), 0)
    e = np.full(257, -INF, F32); e[256] = -3.0
    add("-inf then a finite last entry", e, 256)
    e = np.full(513, -0.0, F32); e[300] = 0.0
    add("-0.0 with one +0.0", e, 0)                                                # +0.0 > -0.0 is false, -0.0 == +0.0 is true: index 0
    e = np.full(513, 0.0, F32); e[0] = -0.0
    add("+0.0 behind a -0.0", e, 0)
    e = base(513); e[70] = e[70 + 256] = INF
    add("+inf twice", e, 70)
    e = base(513); e[9] = -INF; e[100] = NAN; e[356] = INF
    add("-inf, NaN and +inf", e, 356)
    return cases


def attack_index(value, case):
    """the index i that setLogAttackTime's result stands for: log10 (i * samplesPerStep * msPerSample) undone (values of i are whole
    numbers at most 1025: their logarithms lie thousands of float steps apart)"""
    sps = case["num_input_samples"] // case["num_downsamples"]
    ms = float(F32(1.0 / (case["sample_rate"] // 1000)))
    return int(round(10.0 ** float(value) / (sps * ms)))


# ---- FFT-LBP (ref :543-564): bit = |cur - prev| > 0.1f in fp32; highest = the last bin with the bit; activity = the bits' count ----
THRESHOLD = F32(0.1)


def lbp_rounding_triples():
    """Operands of opposite sign, so that the fp32 subtraction rounds: pairs whose exact difference is over the threshold and whose
    fp32 difference is the threshold (bit 0), under it and rounded onto it (0), and between it and the next float but rounded to that
    float (1).  Found by search in fp32, the first of each kind from either sign."""
    T, U = float(THRESHOLD), float(up(THRESHOLD))
    found = {}
    a0 = F32(0.09)                                                                  # (0.09 - -0.01: the small operand's steps are an eighth of the threshold's)
    for j in range(0, 64):
        a = F32(a0 + j * np.spacing(a0))
        for k in range(-8, 9):
            b = F32(-(F32(T - float(a)) + k * np.spacing(F32(0.01))))
            exact, d = float(a) - float(b), float(F32(a - b))
            kind = None
            if exact > T and d == T: kind = "over, rounds onto"
            elif exact < T and d == T: kind = "under, rounds onto"
            elif T < exact < U and d == U: kind = "between, rounds up"
            if kind and kind not in found:
                found[kind] = (a, b, int(d > T))
    assert len(found) == 3, found
    out = []
    for kind in ("over, rounds onto", "under, rounds onto", "between, rounds up"):
        a, b, bit = found[kind]
        out += [(a, b, bit), (b, a, bit)]                                          # and from the other sign: |b - a|
    return out


def lbp_cases():
    """-> [{label, cur [C][B], prev [C][B], bits [C][B], highest [C] (the last bin with the bit, 0 without one), count [C]}]"""
    T, U, D = THRESHOLD, up(THRESHOLD), down(THRESHOLD)
    triples = [(T, 0, 0), (U, 0, 1), (D, 0, 0), (0, T, 0), (0, U, 1), (0, D, 0), (-T, 0, 0), (-U, 0, 1), (-D, 0, 0), (0, -U, 1), (0, -T, 0),
               (F32(1.0) + T, 1.0, int(F32(F32(1.0) + T) - F32(1.0) > T)), (0.5, F32(0.5) - T, int(F32(0.5) - F32(F32(0.5) - T) > T)),
               (INF, INF, 0), (-INF, -INF, 0), (INF, 0, 1), (0, INF, 1), (-INF, 0, 1), (INF, -INF, 1),
               (NAN, 0, 0), (0, NAN, 0), (NAN, NAN, 0), (NAN, INF, 0), (1.0, NAN, 0)] + lbp_rounding_triples()
    B = 65
    cur, prev, bits = np.zeros((1, B), F32), np.zeros((1, B), F32), np.zeros((1, B), np.uint8)
    assert len(triples) <= B
    for i, (a, b, bit) in enumerate(triples):
        cur[0, i], prev[0, i], bits[0, i] = a, b, bit
    cases = [dict(label="threshold", cur=cur, prev=prev, bits=bits)]
    for B in (1, 255, 256, 257):
        cur, prev, bits = np.zeros((4, B), F32), np.full((4, B), D, F32), np.zeros((4, B), np.uint8)       # every bin one step under the threshold
        prev[0, 0] = U; bits[0, 0] = 1                                             # only bin 0
        prev[1, B - 1] = U; bits[1, B - 1] = 1                                     # only the last bin
        prev[3] = U; bits[3] = 1                                                   # (channel 2: no bin) every bin
        cases.append(dict(label="bins %d" % B, cur=cur, prev=prev, bits=bits))
    for c in cases:
        c["count"] = c["bits"].sum(axis=1)
        c["highest"] = np.array([np.flatnonzero(r)[-1] if r.any() else 0 for r in c["bits"]])
    return cases


# ---- histogram F0 (ref :253-303).  nyquist = 10 * bins makes a bin 10 Hz wide exactly: an interval of d bins is the candidate 10 d, and its
# harmonics fall on the bins d, 2 d, ... exactly ----
def harmonic_cases():
    """-> [{label, frames [T][C][B], nyquist, f0 [T][C] (the F0 each frame must return), gated [T][C] (the `sum < 0.001` return: zeros, previousF0
    untouched), previous [T][C] (previousF0 after each frame), her {(t, c): the harmonic energy ratio, where the case is built for it}}]"""
    cases = []

    def add(label, channels, f0, gated=None, nyquist=None, her=None):
        """channels: per channel the list of its frames"""
        frames = np.stack([np.stack(ch) for ch in channels], axis=1).astype(F32)     # [T][C][B]
        T, C, B = frames.shape
        f0 = np.array(f0, np.float64).T.reshape(T, C)                               # given per channel
        gated = np.zeros((T, C), bool) if gated is None else np.array(gated, bool).T.reshape(T, C)
        previous = np.zeros((T, C))
        for t in range(T):
            previous[t] = np.where(gated[t], previous[t - 1] if t else 0.0, f0[t])
        cases.append(dict(label=label, frames=frames, nyquist=10.0 * B if nyquist is None else nyquist, f0=f0, gated=gated, previous=previous, her=her or {}))

    def pair(B, d, level=1.0):
        return sparse(B, {d: level, 2 * d: level})                                 # two peaks d bins apart: F0 = 10 d, every harmonic on a peak: ratio 1

    under, on, over = gate_terms()
    assert len(on) <= 4
    def padded(v, B):
        m = np.zeros(B, F32); m[:len(v)] = v
        return m
    nan_frame = sparse(5, {0: 1.0, 2: NAN, 4: 1.0})
    # `sum < 0.001` (:273): under it zeros are returned and previousF0 stays; on it (and over it) the frame goes on: its one peak gives no
    # interval, so F0 = 0 and previousF0 becomes 0.  A NaN sum is not < 0.001: it goes on as well (every weight is NaN, nothing is taken).
    add("gate", [[sparse(5, {0: 1.0, 2: 1.0}), padded(v, 5)] for v in (under, on, over)] + [[sparse(5, {0: 1.0, 2: 1.0}), nan_frame]],
        f0=[[20.0, 0.0]] * 4, gated=[[0, 1], [0, 0], [0, 0], [0, 0]])
    # a flat spectrum: the mean equals every bin exactly (0.5 B / B), `m <= mean` holds everywhere: no peaks; after a previous F0 over 10 the
    # octave rule sees the ratio inf (inf - floor (inf) is NaN: not < 0.1) and lets the 0 through
    for B in (5, 257):
        add("flat %d" % B, [[pair(B, 2 if B == 5 else 60), np.full(B, 0.5, F32)]], f0=[[20.0 if B == 5 else 600.0, 0.0]])
    # equal neighbours are both peaks (`>` rejects, equality does not); the window is [bin - 2, bin + 2): a larger bin at bin + 2 is not looked at,
    # a larger one at bin - 2 is
    add("neighbours", [[sparse(65, {10: 1.0, 11: 1.0})], [sparse(65, {20: 1.0, 22: 2.0})], [sparse(65, {20: 2.0, 22: 1.0})]], f0=[[10.0], [20.0], [0.0]])
    # peaks at bins 0, 1, B - 2, B - 1 (equal magnitudes): the intervals enter as 1 | B-2, B-3 | B-1, B-2, 1; interval 1 and interval B - 2 both
    # weigh 2 x 1/4 (one harmonic each on a peak), and 1 entered first
    for B in (64, 65):
        add("edge peaks %d" % B, [[sparse(B, {0: 1.0, 1: 1.0, B - 2: 1.0, B - 1: 1.0})]], f0=[[10.0]], her={(0, 0): 0.25})
    # the smallest frames
    add("bins 4", [[sparse(4, {0: 1.0, 3: 1.0})]], f0=[[30.0]], her={(0, 0): 0.5})
    add("bins 5", [[sparse(5, {0: 1.0, 1: 1.0, 3: 1.0, 4: 1.0})]], f0=[[10.0]], her={(0, 0): 0.75})
    # an exact tie of count x ratio between two intervals whose histogram order is not their numeric order: peaks at a, 2a, 2a + 2a/3 with
    # magnitudes 1, 2, 1 enter the intervals a, 5a/3, 2a/3; interval a sums the peaks at a and 2a (1 + 2), interval 2a/3 those at 2a and 8a/3
    # (2 + 1): both 3/4 with count 1.  The first in histogram order, a, wins -- the larger one.  The two intervals fall to lanes of one wave
    # (30, 20), to different waves (150, 100) and to a thread's second stride (300, 200).
    for a, B in ((30, 257), (150, 513), (300, 1025)):
        add("tie %d" % a, [[sparse(B, {a: 1.0, 2 * a: 2.0, 2 * a + 2 * a // 3: 1.0})]], f0=[[10.0 * a]], her={(0, 0): 0.75})
    # the 15th harmonic of interval 17 is bin 255: the last bin of 256 (added: all three magnitudes are on harmonics, ratio 1) and one past
    # the end of 255 bins (`bin >= numBins` ends the loop before it is read)
    add("harmonic 15 on the last bin", [[sparse(256, {17: 1.0, 34: 1.0, 255: 1.0})]], f0=[[170.0]], her={(0, 0): 1.0})
    add("harmonic 15 past the end", [[sparse(255, {17: 1.0, 34: 1.0})]], f0=[[170.0]], her={(0, 0): 1.0})
    # the octave rule (:279-297) over consecutive frames of one analyser
    flat = np.full(257, 0.5, F32)
    P = lambda d: pair(257, d)
    add("octave rule",
        [[P(10), P(20), P(20)],      # ratio exactly 2.0: not > 2.0, the new F0 stands; then previous == new: nothing to decide
         [P(10), P(30), P(21)],      # exactly 3.0: the fraction 0 < 0.1 keeps the previous F0; then 210 / 100: 2.1 - 2 is above 0.1 in fp64, the new one stands
         [P(20), P(41), flat],       # 2.05: the fraction is under 0.1, kept; then no peaks after a previous F0 over 10: ratio inf, F0 = 0
         [P(20), P(10), P(30)]],     # the previous on top: 200 / 100 = 2.0, not > 2.0; then 300 / 100 keeps 100
        f0=[[100.0, 200.0, 200.0], [100.0, 100.0, 210.0], [200.0, 200.0, 0.0], [200.0, 100.0, 100.0]])
    # `previousF0 > 10.0`: a previous F0 of exactly 10.0 (4 bins, nyquist 40) does not arm the rule, one fp64 step over it does (the ratio is 3)
    step_over = float(np.nextafter(10.0, INF))
    add("previous 10.0", [[sparse(4, {0: 1.0, 1: 1.0}), sparse(4, {0: 1.0, 3: 1.0})]], f0=[[10.0, 30.0]])
    add("previous over 10.0", [[sparse(4, {0: 1.0, 1: 1.0}), sparse(4, {0: 1.0, 3: 1.0})]], f0=[[step_over, step_over]], nyquist=4.0 * step_over)
    # non-finite magnitudes: +inf makes the mean inf (`m <= mean` everywhere: no peaks); -inf makes the sum -inf (< 0.001: the gate); both make it
    # NaN, and so does a NaN between two peaks (the frame goes on, every weight is NaN, nothing is taken)
    first = pair(65, 2)
    add("non-finite", [[first, sparse(65, {7: INF, 20: 1.0, 40: 1.0})], [first, sparse(65, {7: -INF, 20: 1.0, 40: 1.0})],
                       [first, sparse(65, {7: INF, 9: -INF, 20: 1.0, 40: 1.0})], [first, sparse(65, {20: 1.0, 30: NAN, 40: 1.0})]],
        f0=[[20.0, 0.0]] * 4, gated=[[0, 0], [0, 1], [0, 0], [0, 0]])
    # the LDS maximum
    add("bins 4097", [[sparse(MAX_BINS, {1000: 1.0, 2000: 1.0})], [sparse(MAX_BINS, {2048: 3.0, 4096: 3.0})]], f0=[[10000.0], [20480.0]])
    return cases


# ---- the full-spectrum characteristics (ref :463-515): `! (sum > 0.001)` returns zeros and leaves previousBinMagnitudes alone ----
def spectral_cases():
    """-> [{label, frames [T][C][B], nyquist, gated [T][C], flux {(t, c): the flux the frame must return}, flatness {(t, c): its flatness, where
    the product decides it without pow()}}]"""
    rng = np.random.default_rng(20261020)
    cases = []

    def add(label, channels, gated=None, flux=None, flatness=None, nyquist=24000.0):
        frames = np.stack([np.stack(ch) for ch in channels], axis=1).astype(F32)
        T, C, B = frames.shape
        gated = np.zeros((T, C), bool) if gated is None else np.array(gated, bool).T.reshape(T, C)
        cases.append(dict(label=label, frames=frames, nyquist=nyquist, gated=gated, flux=flux or {}, flatness=flatness or {}))

    under, on, over = gate_terms()
    def padded(v, B=5):
        m = np.zeros(B, F32); m[:len(v)] = v
        return m
    first, third = np.array([1, 2, 3, 2, 1], F32), np.full(5, 2.0, F32)
    # the gate between two ordinary frames: under 0.001, on it (not > 0.001) and with a NaN in the middle (not > anything) the four outputs
    # are +0.0 and the third frame's flux is taken against the FIRST frame (1 + 0 + 0 + 0 + 1); over it the frame is analysed and the third
    # frame's flux is taken against it
    nan_mid = np.array([1, 2, NAN, 2, 1], F32)
    add("gate", [[first, padded(under), third], [first, padded(on), third], [first, padded(over), third], [first, nan_mid, third]],
        gated=[[0, 1, 0], [0, 1, 0], [0, 0, 0], [0, 1, 0]],
        flux={(2, 0): 2.0, (2, 1): 2.0, (2, 3): 2.0, (2, 2): serial_sum([2.0 - float(v) for v in padded(over)]), (0, 0): 9.0})
    # the first frame of an analyser: flux = the sum of |m|; the same frame again: +0.0; the same magnitudes with other signs: +0.0 again
    # (the flux compares absolute values); then a louder frame
    for B in (64, 257):
        m = (rng.random(B) * 1.5 + 0.5).astype(F32)
        flipped = m.copy(); flipped[3] = -m[3]; flipped[B - 2] = -m[B - 2]
        add("flux %d" % B, [[m, m, flipped, (m * F32(2.0)).astype(F32)]],
            flux={(0, 0): serial_sum(m), (1, 0): 0.0, (2, 0): 0.0, (3, 0): serial_sum(m)})
    # the product: a zero bin makes it 0 and a -0.0 bin -0.0 (the flatness is +0.0 both times: pow (-0.0, 1/65) is +0.0); 65 bins of 1e30
    # overflow it to inf (flatness inf); 64 bins of 1e-30 around one of 1.0 underflow it to exactly 0 (1e-300, then 0: never a subnormal)
    m = (rng.random(65) * 1.5 + 0.5).astype(F32)
    zero, negzero = m.copy(), m.copy()
    zero[31], negzero[31] = 0.0, -0.0
    tiny = np.full(65, 1e-30, F32); tiny[32] = 1.0
    add("product", [[zero], [negzero], [np.full(65, 1e30, F32)], [tiny]], flatness={(0, 0): 0.0, (0, 1): 0.0, (0, 2): INF, (0, 3): 0.0})
    # a frame of +inf passes the gate and the buffer becomes inf; the finite frame behind it has flux +0.0 (|m| - inf is not > 0) and
    # replaces the buffer; the third frame's flux is an ordinary one again
    a, b = (rng.random(65) + 0.5).astype(F32), (rng.random(65) + 0.5).astype(F32)
    add("inf frame", [[np.full(65, INF, F32), a, b]],
        flux={(0, 0): INF, (1, 0): 0.0, (2, 0): serial_sum([max(0.0, float(y) - float(x)) for x, y in zip(a, b)])})
    # the LDS maximum: magnitudes around 1, so that the product of 4097 of them stays a normal number
    add("bins 4097", [[(rng.random(MAX_BINS) * 0.2 + 0.9).astype(F32)] * 2], flux={(1, 0): 0.0})
    return cases


# ---- the legacy slope (ref :566-609): `! (magnitude > 0.0001)` returns 0 ----
def slope_cases():
    """-> [{label, mags [C][B], gated [C] (the peak is not > 0.0001: +0.0), nan [C] (the result must be a NaN), finite [C]}]"""
    rng = np.random.default_rng(20261021)
    cases = []

    def add(label, rows, gated, nan=None, finite=None):
        mags = np.stack(rows).astype(F32)
        C = mags.shape[0]
        cases.append(dict(label=label, mags=mags, gated=np.array(gated, bool), nan=np.array(nan if nan is not None else [0] * C, bool),
                          finite=np.array(finite if finite is not None else [0] * C, bool)))

    E = F32(1e-4)
    peaks = [down(E), E, up(E)]
    sides = [not (float(p) > 0.0001) for p in peaks]                                # the fp32 peak widened to fp64 against the fp64 constant
    assert sides[0] and not sides[2]
    add("peak around 1e-4", [np.array([0, p, 0, p / F32(2), 0], F32) for p in peaks] + [np.array([0, 0, 0, -p, 0], F32) for p in peaks],
        gated=sides + sides, finite=[not s for s in sides + sides])
    add("one bin", [np.array([3.0], F32), np.array([-3.0], F32), np.array([0.0], F32)], gated=[0, 0, 1], nan=[1, 1, 0])       # (bins - 1.0f) is 0: 0.5 / 0 times a deviation of 0
    base = (rng.random(65) + 0.5).astype(F32)
    rows = []
    for v in (INF, -INF):
        r = base.copy(); r[20] = v; rows.append(r)                                  # x / inf is 0 and inf / inf NaN: the sums are NaN
    r = base.copy(); r[20] = NAN; rows.append(r)                                    # the peak scan skips a NaN, the sums do not
    r = base.copy(); r[64] = NAN; rows.append(r)
    add("non-finite", rows, gated=[0] * 4, nan=[1] * 4)
    r = (base * F32(0.1)).astype(F32); r[7] = -3.0
    add("negative peak", [r, -base], gated=[0, 0], finite=[1, 1])
    for B in (255, 256, 257):
        add("flat and silent %d" % B, [np.full(B, 0.3, F32), np.full(B, 1e-5, F32), np.zeros(B, F32), np.full(B, -0.0, F32)],
            gated=[0, 1, 1, 1])                                                     # (flat: the energy deviation is 0 or a rounding residue: NaN, 0 or finite, as the reference has it)
    add("bins 4097", [np.exp(-np.arange(MAX_BINS) / 800.0).astype(F32), (rng.random(MAX_BINS)).astype(F32)], gated=[0, 0], finite=[1, 1])
    return cases


# ---- auto-correlation (ref :623-665): the first item holding the largest real part of item x conj (item); getMaxIndex starts from item 0 ----
def autocorrelation_cases():
    """-> [{label, data [C][n][2], nyquist, peak [C]}]"""
    rng = np.random.default_rng(20261022)
    cases = []
    for n in (5, 257, 513):
        data = rng.normal(0, 1, (6, n, 2)).astype(F32)
        data[0, 3, 0], data[0, 4, 0] = -INF, INF                                    # both squares are +inf: the first
        data[1, n - 1, 0] = INF
        data[2, :, 0] = NAN; data[2, 0, 0] = 2.0                                    # every real part NaN but item 0's
        data[3, :, 0] = NAN; data[3, 2, 0] = 2.0                                    # ... but item 2's: item 0's NaN stays the maximum, bin 0
        data[4, 1, 1] = INF                                                         # an infinite imaginary part: (r * r) - (i * -i) is +inf
        data[5, :, 0] *= F32(0.1)
        data[5, 2, 0], data[5, 2, 1] = INF, NAN                                     # a NaN product: skipped
        data[5, 4, 0] = 9.0
        cases.append(dict(label="items %d" % n, data=data, nyquist=1000.0, peak=np.array([3, n - 1, 0, 0, 1, 4])))
    one = np.array([[[3.0, 4.0]], [[NAN, 1.0]], [[-INF, 0.0]], [[0.0, -0.0]]], F32)
    cases.append(dict(label="one item", data=one, nyquist=24000.0, peak=np.array([0, 0, 0, 0])))
    return cases
