"""The search behind tests/harmonic_cases.py: prints CASES, UNREACHED, UNTOLD and CRC, the block between BEGIN TABLE and END TABLE of
that module (--write puts it there).

    python tests/golden/make_harmonic_cases.py [--write] [N ...]

Per window size the candidates of the families (harmonic_cases.synth) are generated in a fixed order and classified by the oracle alone
(harmonic_cases.classify, at 48 kHz and at 44.1 kHz).  First pass: the first candidate found for each class that is wanted is kept.
Second pass: for every mutant (and bins-per-lane geometry) that none of the kept frames tells apart, the first candidate that does is
kept.  The s16-exact frames are listed first.  What is not found is listed in UNREACHED (classes) and UNTOLD (mutants).  About three
minutes for the five sizes; needs only numpy and the oracle."""
import itertools
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import harmonic_cases as hc  # noqa: E402
from oracle import fx_oracle  # noqa: E402

ALWAYS_UNREACHED = (("gate", "equal"), ("level", "upper on the mean"), ("mean", "within rounding, not flat"),
                    ("probe", "at bin M-2 or M-1"), ("probe", "lb == f0_bin skip"))


def sp(pairs):
    return ("sp", tuple((int(n), int(k)) for n, k in pairs if k))


def candidates(N):
    M = N // 2
    q = N // 4
    # four impulses on the quarters: spectra of period 4 with exact ties (only unit twiddles meet)
    for s in (333, 1001):
        for x0, x1, x2 in itertools.product(range(-3, 4), repeat=3):
            if (x0, x1, x2) != (0, 0, 0):
                yield sp(((0, x0 * s), (q, x1 * s), (3 * q, x1 * s), (2 * q, x2 * s)))
    # the spectrum's ends: re[k] = a + 2 b cos(2 pi k / N) + 2 c cos(4 pi k / N), not periodic
    for a in (1000, 2000):
        for b in range(-900, 901, 150):
            for c in range(-600, 601, 150):
                if b or c:
                    yield sp(((0, a), (1, b), (-1, b), (2, c), (-2, c)))
    # impulse trains: N h / lag and N / (lag 2^k) on integers, hb == M at lags 2, 4 and 6, the DC-heavy frames
    for period in range(1, 129):
        for phase in sorted({0, 1, period // 2}):
            for ka, kb in ((3000, 3000), (3000, -1500), (3000, 1000), (3000, -3000), (3000, 2700), (3000, 2400), (3000, 2000)):
                for dc in (0, 400, 1500):
                    if phase < period:
                        yield ("train", period, phase, ka, kb, dc)
    # a small constant under the end and quarter frames: the constant draws the lag out to a hundred samples and more
    for dc in (20, 50, 100, 200, 3, 5):
        for b in range(-900, 901, 300):
            for c in (-600, 0, 600):
                if b or c:
                    yield ("mix", ("train", 1, 0, dc, dc, 0), sp(((0, 2000), (1, b), (-1, b), (2, c), (-2, c))))
        for x0, x1, x2 in itertools.product(range(-2, 3), repeat=3):
            for s in (1001, 333):
                if (x0, x1, x2) != (0, 0, 0):
                    yield ("mix", ("train", 1, 0, dc, dc, 0), sp(((0, x0 * s), (q, x1 * s), (3 * q, x1 * s), (2 * q, x2 * s))))
    # sparse impulses on multiples of N/8 .. N/64
    rng = np.random.default_rng(7000 + N)
    for D in (8, 16, 32, 64):
        for _ in range(250):
            at = np.flatnonzero(rng.random(D) < min(0.6, 5.0 / D))
            ks = rng.integers(-3, 4, at.size) * int(rng.choice((333, 1001, 2500)))
            if np.any(ks):
                yield sp(zip((at * (N // D)).tolist(), ks.tolist()))
    # a few impulses anywhere: spectra without structure, for the neighbours taken from the wrong bin
    for _ in range(1200):
        at = rng.integers(0, N, int(rng.integers(2, 7)))
        ks = rng.integers(-3000, 3001, at.size)
        yield sp(sorted(dict(zip(at.tolist(), ks.tolist())).items()))
    # one impulse of a full-mantissa amplitude at sample 0 or N/2: the flat spectra, and the gate
    a0 = np.array([np.sqrt(0.005 / M)], np.float32).view(np.uint32)[0]
    for n in (0, N // 2):
        for d in (0, -1, 1, -2, 2):                                              # (adjacent amplitudes on both sides of the gate)
            yield ("fb", ((n, int(a0) + d),))
        for _ in range(600):
            yield ("fb", ((n, int(0x3D800000 + rng.integers(0, 1 << 25))),))


def told(re, lag, ref, mutant, U):
    return not hc.same_slots(hc.model(re, lag, 24000.0, mutant, U), ref)


def search(N):
    t0 = time.time()
    pool = []
    for case in candidates(N):
        w = hc.synth(N, case)
        cls = set()
        for rate in hc.RATES:
            cls |= hc.classify(fx_oracle, w, rate)[2]
        pool.append((case, w, cls))
    held, chosen = set(), []
    want = hc.wanted(N)
    for case, w, cls in pool:
        if (cls & want) - held:
            chosen.append(case)
            held |= cls
    # the mutants
    targets = hc.mutant_targets(N)
    inputs = {}

    def inp(case, w):
        if case not in inputs:
            re, lag = hc.oracle_inputs(fx_oracle, w)
            inputs[case] = (re, lag, hc.model(re, lag, 24000.0))
        return inputs[case]

    by_case = {case: w for case, w, _ in pool}
    untold = [t for t in targets if not any(told(*inp(c, by_case[c]), *t) for c in chosen)]
    for case, w, cls in pool:
        if not untold:
            break
        now = [t for t in untold if told(*inp(case, w), *t)]
        if now and case not in chosen:
            chosen.append(case)
            held |= cls
            untold = [t for t in untold if t not in now]
    chosen = [c for c in chosen if hc.s16_exact(c)] + [c for c in chosen if not hc.s16_exact(c)]
    unreached = sorted(want - held, key=repr) + list(ALWAYS_UNREACHED)
    sys.stderr.write("N=%d: %d candidates, %d frames, %d classes unreached, %d mutants untold, %.0f s\n" % (
        N, len(pool), len(chosen), len(unreached), len(untold), time.time() - t0))
    return chosen, unreached, untold


def block(name, table, sizes):
    out = ["%s = {" % name]
    for N in sizes:
        out.append("    %d: (" % N)
        line = "       "
        for c in table[N]:
            s = " %r," % (c,)
            if len(line) + len(s) > 140 and line.strip():
                out.append(line)
                line = "       "
            line += s
        if line.strip():
            out.append(line)
        out.append("    ),")
    out.append("}")
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--write"]
    sizes = [int(a) for a in args] or list(hc.SIZES)
    cases, unreached, untold, crcs = {}, {}, {}, {}
    for N in sizes:
        cases[N], unreached[N], untold[N] = search(N)
        crcs[N] = zlib.crc32(np.stack([hc.synth(N, c) for c in cases[N]]).astype(np.float32).tobytes())
    lines = block("CASES", cases, sizes) + block("UNREACHED", unreached, sizes) + block("UNTOLD", untold, sizes)
    lines.append("CRC = {%s}" % ", ".join("%d: %d" % (N, crcs[N]) for N in sizes))
    text = "\n".join(lines) + "\n"
    if "--write" in sys.argv[1:] and sizes == list(hc.SIZES):
        path = os.path.join(ROOT, "tests", "harmonic_cases.py")
        src = open(path).read()
        head, rest = src.split("# BEGIN TABLE\n")
        _, tail = rest.split("# END TABLE\n")
        open(path, "w").write(head + "# BEGIN TABLE\n" + text + "# END TABLE\n" + tail)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
