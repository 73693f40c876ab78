"""The lag-search cases (tests/lag_cases.py) on the CPU, by the oracle alone: the frames are the recorded ones, a fresh classification
holds every floor the table was chosen for (the seams of the kernels' 64-sample blocks and of the 1024-point kernel's three stages, the
walk to the end, the fallback), the two restatements of the reference agree on every chosen frame's lag, and what the search did not
reach is written down and really absent.  tests/test_gpu_lag_cases.py runs the frames through every implementation of the search.

The search itself is tests/golden/make_lag_cases.py; nothing here searches."""
import numpy as np
import pytest

import lag_cases as lg
from oracle import fx_numpy

CELL_FLOOR = {256: 10, 512: 16, 1024: 32, 2048: 56, 4096: 96}
MAX_FRAMES = 168                                                               # fourteen channels of twelve frames


def held(oracle, N):
    out = set()
    for k in lg.classified(oracle, N):
        out |= lg.classes(N, *k)
    return out


@pytest.mark.parametrize("N", lg.SIZES)
def test_frames_are_the_recorded_ones(N):
    F = lg.frames(N)
    assert F.shape == (len(lg.CASES[N]), N) and F.dtype == np.float32 and len(lg.CASES[N]) <= MAX_FRAMES
    assert lg.crc(N) == lg.CRC[N]
    s = lg.as_s16(F)                                                           # exact in the s16 format
    assert np.array_equal(s.astype(np.float32) / np.float32(32768.0), F)
    B, where = lg.batch_layout(N)
    assert all(np.array_equal(B[c, t], F[k]) for k, (c, t) in enumerate(where))
    H, at = lg.hop_layout(N)
    assert all(np.array_equal(np.concatenate([H[c, t - 1], H[c, t]]), F[k]) for k, (c, t) in enumerate(at))


@pytest.mark.parametrize("N", lg.SIZES)
def test_floors(oracle, N):
    """every condition the table was chosen for, from a fresh classification"""
    got = held(oracle, N)
    cells = sorted(c[1:] for c in got if c[0] == "cell")
    others = sorted((c for c in got if c[0] != "cell"), key=repr)
    print("N=%d: %d frames, cells %d / %d, classes held: %s" % (N, len(lg.CASES[N]), len(cells), N // 16, " ".join("-".join(map(str, c)) for c in others)))
    print("N=%d: UNREACHED: %s" % (N, " ".join("-".join(map(str, c)) for c in lg.UNREACHED[N])))
    assert len(cells) >= CELL_FLOOR[N], (N, len(cells))
    for c in (("end", N), ("first63",), ("first2",), ("stop=first",)):
        assert c in got, (N, c)
    if N == 1024:
        # both stage seams of the 1024-point kernel (samples 126-129 and 254-257) and every block seam up to block 7, on both sides
        for b in range(1, 8):
            for r in lg.RESIDUES:
                assert (r, b) in cells, (r, b)
        assert (62, 0) in cells and (63, 0) in cells
        assert ("cross", 2) in got
    if N == 256:
        assert ("fallback", 2) in got and ("fallback", 3) in got


@pytest.mark.parametrize("N", lg.SIZES)
def test_classification_and_both_restatements_give_the_oracles_lag(oracle, N):
    """classify's lag is fxo_estimate_pitch's, and fx_numpy's separately written search (fx_numpy.lag_search) answers the same on the
    oracle's cnd; at 256 and 512 points fx_numpy's whole pitch path (its own FFT, low-pass and running sum) does as well"""
    for k, w in enumerate(lg.frames(N)):
        lag, cnd = lg.oracle_cnd(oracle, w)
        kind, first, stop, mine = lg.classified(oracle, N)[k]
        assert mine == lag, (N, k, lg.CASES[N][k], lg.describe(N, kind, first, stop, mine), lag)
        assert 2 <= lag <= N and (kind == "end") == (first is not None and stop == N - 1)
        assert fx_numpy.lag_search(cnd, N) == float(lag), (N, k, lg.CASES[N][k])
        if N <= 512:
            fre, _ = fx_numpy.forward_real(fx_numpy.bartlett(fx_numpy.lowpass(w)))
            _, nlag, ncnd = fx_numpy.pitch(fre, 24000.0)
            assert nlag == float(lag) and np.array_equal(ncnd, cnd), (N, k, lg.CASES[N][k])


@pytest.mark.parametrize("N", lg.SIZES)
def test_unreached_is_really_absent_and_complete(oracle, N):
    """no chosen frame is of a class listed as unreached, and every cell is either held or listed: the gap is written down"""
    got = held(oracle, N)
    for c in lg.UNREACHED[N]:
        if c == ("fallback", None):
            assert not any(g[0] == "fallback" for g in got), N
        else:
            assert c not in got, (N, c)
    listed = set(lg.UNREACHED[N])
    for c in lg.all_cells(N) - {("cell", 0, 0), ("cell", 1, 0)}:               # (stop >= 2: lanes 0 and 1 of block 0 are no cells)
        assert (c in got) != (c in listed), (N, c)
    assert (("end", N - 1) in got) != (("end", N - 1) in listed)
    if N >= 512:
        assert (("fallback", None) in listed) != any(g[0] == "fallback" for g in got)


def test_a_failure_names_the_seam(oracle):
    """what tests/test_gpu_lag_cases.py reports (lag_cases.assert_held): a made-up kernel that stops one sample early where the walk
    ends on a block's last lane is told the class, first, stop, the oracle's lag and its own; the oracle's own output passes"""
    N = 1024
    B, where = lg.batch_layout(N)
    want = oracle.process_frames(B, N)
    lg.assert_held(oracle, want, want, B, "default", "the oracle itself")
    k = next(i for i, q in enumerate(lg.classified(oracle, N)) if q[0] == "walk" and q[2] % 64 == 63 and q[3] == q[2])
    _, first, stop, lag = lg.classified(oracle, N)[k]
    c, t = where[k]
    assert lg.lag_of(want[0][c, t, lg.F0]) == lag
    got = (want[0].copy(), want[1])
    got[0][c, t, lg.F0] = np.float32(48000.0 / (lag - 1) / 5000.0)
    with pytest.raises(AssertionError) as e:
        lg.assert_held(oracle, got, want, B, "default", "made up")
    said = str(e.value)
    assert "first %d " % first in said and "stop %d (lane 63 of block %d)" % (stop, stop // 64) in said, said
    assert "the oracle's lag %d, the kernel answered %d" % (lag, lag - 1) in said, said
