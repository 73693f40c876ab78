"""The search behind tests/lag_cases.py: prints CASES, UNREACHED and CRC to paste into that module.

    python tests/golden/make_lag_cases.py [N ...]

Per window size the candidates of four families (lag_cases.synth) are generated in a fixed order, rounded to s16 and classified by the
oracle alone (lag_cases.classify); the first candidate found for each class is kept.  After the families one try is made at what is still
missing: a fine sweep of the period of a plain and of a lightly noisy tone around every missing cell's lag and around N-1 (for the walk
to the end with lag N-1), and short decaying bursts for the fallback.  What is not found then is listed in UNREACHED.  About a minute and
a half for the five sizes; needs only numpy and the oracle."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lag_cases as lg  # noqa: E402
from oracle import fx_oracle  # noqa: E402

RANDOM_PER_FAMILY = {256: 6000, 512: 6000, 1024: 6000, 2048: 4000, 4096: 3000}


def r(x, d=3):
    return round(float(x), d)


def family_candidates(N):
    top = 6000 if N == 1024 else 8 * N
    for P in range(8, top + 1):
        for dc in (0.0, 0.3):
            yield ("sine", float(P), dc)
    rng = np.random.default_rng(1000 + N)
    M = RANDOM_PER_FAMILY[N]
    for k in range(M):                                                         # P in [8, 4N] (log-uniform), a in [0, 0.5], sigma 10^[-4, -1]
        yield ("harm", r(np.exp(rng.uniform(np.log(8.0), np.log(4.0 * N)))), r(rng.uniform(0, 2 * np.pi)), r(rng.uniform(0, 0.5)),
               r(rng.uniform(-4, -1), 2), k)
    for k in range(M // 2):                                                    # P in [N/4, 64N]
        yield ("long", r(np.exp(rng.uniform(np.log(N / 4.0), np.log(64.0 * N)))), r(rng.uniform(0, 2 * np.pi)), k)
    for k in range(M // 2):                                                    # tau in [2, N]
        yield ("decay", r(np.exp(rng.uniform(np.log(2.0), np.log(float(N))))), k)


def wanted(N):
    """every class the search looks for (fallback: every block)"""
    out = set(lg.all_cells(N)) - {("cell", 0, 0), ("cell", 1, 0)}             # stop >= 2
    out |= {("first63",), ("first0",), ("first2",), ("stop=first",), ("cross", 0), ("cross", 1), ("cross", 2), ("end", N), ("end", N - 1)}
    out |= {("fallback", b) for b in range(N // 64)}
    return out


def extra_candidates(N, missing):
    deltas = np.linspace(-1.5, 1.5, 31)
    targets = sorted({64 * c[2] + c[1] for c in missing if c[0] == "cell"} | ({N - 1, N} if ("end", N - 1) in missing else set()))
    k = 0
    for L in targets:
        for mult in (1, 2):
            for d in deltas:
                P = r(L / mult + d)
                if P < 8:
                    continue
                for dc in (0.0, 0.3):
                    yield ("sine", P, dc)
                yield ("harm", P, 0.2, 0.0, -4.0, k)
                k += 1
    if any(c[0] == "fallback" for c in missing):
        for k in range(2000):                                                  # short bursts: the flattest autocorrelations the families have
            yield ("decay", r(2.0 + 0.01 * k), 100000 + k)


def search(N):
    held, chosen = {}, []
    t0 = time.time()

    def take(cands, only=None):
        for case in cands:
            got = lg.classes(N, *lg.classify(fx_oracle, lg.synth(N, case)))
            new = [c for c in got if c not in held and (only is None or c in only)]
            if new:
                chosen.append(case)
                for c in new:
                    held[c] = len(chosen) - 1

    take(family_candidates(N))
    n_family = len(chosen)
    missing = wanted(N) - set(held)
    take(extra_candidates(N, missing), only=missing)
    missing = wanted(N) - set(held)
    if not any(c[0] == "fallback" for c in held):                              # no fallback at all: one entry, not one per block
        missing = {c for c in missing if c[0] != "fallback"} | {("fallback", None)}
    cells = sum(c[0] == "cell" for c in held)
    sys.stderr.write("N=%d: %d frames (%d from the families), %d cells of %d, %d classes unreached, %.0f s\n" % (
        N, len(chosen), n_family, cells, N // 16, len(missing), time.time() - t0))
    return chosen, sorted(missing, key=repr)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or list(lg.SIZES)
    cases, unreached, crcs = {}, {}, {}
    for N in sizes:
        cases[N], unreached[N] = search(N)
        crcs[N] = __import__("zlib").crc32(np.stack([lg.synth(N, c) for c in cases[N]]).astype(np.float32).tobytes())
    print("CASES = {")
    for N in sizes:
        print("    %d: (" % N)
        line = "       "
        for c in cases[N]:
            s = " %r," % (c,)
            if len(line) + len(s) > 140:
                print(line)
                line = "       "
            line += s
        print(line)
        print("    ),")
    print("}")
    print("UNREACHED = {")
    for N in sizes:
        print("    %d: (" % N)
        line = "       "
        for c in unreached[N]:
            s = " %r," % (c,)
            if len(line) + len(s) > 140:
                print(line)
                line = "       "
            line += s
        print(line)
        print("    ),")
    print("}")
    print("CRC = {%s}" % ", ".join("%d: %d" % (N, crcs[N]) for N in sizes))


if __name__ == "__main__":
    main()
