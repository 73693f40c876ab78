"""The harmonic cases (tests/harmonic_cases.py) on the CPU, by the oracle alone: the frames are the recorded ones; the restatement in
harmonic_cases.analyse gives the C oracle's HER, OER and inharmonicity slots bit for bit on every chosen frame, at 48 kHz and at 44.1 kHz;
a fresh classification holds every class the table was chosen for; what the search did not reach is written down and really absent; and
the frames can tell every single-decision mutant of the model apart -- for every mutant, every size and both bins-per-lane geometries at
least one frame changes a harmonic slot, all three of which are exact slots (oracle/ulp.py).  The mutants that change nothing for any
lag are shown to do so by going through every lag.  tests/test_gpu_harmonic_cases.py runs the frames through every implementation.

The search itself is tests/golden/make_harmonic_cases.py; nothing here searches, and nothing here is compared with a kernel."""
import math
from fractions import Fraction

import numpy as np
import pytest

import harmonic_cases as hc
from oracle import fx_numpy
from oracle.ulp import ulp_budget


def test_the_harmonic_slots_are_exact_slots():
    """what "beyond the slot's budget" means below: any other bit"""
    for family in ("default", "low_latency"):
        assert not ulp_budget(family)[hc.HER:hc.INHARM + 1].any()


@pytest.mark.parametrize("N", hc.SIZES)
def test_frames_are_the_recorded_ones(N):
    F = hc.frames(N)
    assert F.shape == (len(hc.CASES[N]), N) and F.dtype == np.float32 and 0 < len(hc.CASES[N]) <= hc.MAX_FRAMES
    assert hc.crc(N) == hc.CRC[N]
    k = hc.num_s16(N)                                                          # the s16-exact frames come first and are exact
    assert k >= 12 and np.array_equal(hc.as_s16(F[:k]).astype(np.float32) / np.float32(32768.0), F[:k])
    for only in (False, True):
        B, where = hc.batch_layout(N, only)
        assert B.shape[1:] == (hc.T, N) and len(where) == (k if only else len(F))
        assert all(np.array_equal(B[c, t], F[i]) for i, (c, t) in enumerate(where))
        H, at = hc.hop_layout(N, only)
        assert all(np.array_equal(np.concatenate([H[c, t - 1], H[c, t]]), F[i]) for i, (c, t) in enumerate(at))


@pytest.mark.parametrize("rate", hc.RATES)
@pytest.mark.parametrize("N", hc.SIZES)
def test_the_classifier_is_the_oracle_bit_for_bit(oracle, N, rate):
    """harmonic_cases.analyse on the oracle's raw spectrum and lag against fxo_process_frames' raw HER, OER and inharmonicity"""
    B, where = hc.batch_layout(N)
    raw, _ = oracle.process_frames(B, N, rate)
    for i, (c, t) in enumerate(where):
        a, lag, cls = hc.classified(oracle, N, rate)[i]
        assert hc.same_slots(a["slots"], raw[c, t, hc.HER:hc.INHARM + 1]), "N=%d frame %d %r (lag %d; %s): %s, the oracle %s" % (
            N, i, hc.CASES[N][i], lag, hc.describe(cls), a["slots"], raw[c, t, hc.HER:hc.INHARM + 1])
        assert np.float32(rate / lag / 5000.0) == raw[c, t, 2], (N, i, lag)      # and the lag is the frame's


@pytest.mark.parametrize("N", hc.SIZES)
def test_the_numpy_restatement_sums_serially_too(oracle, N):
    """oracle/fx_numpy.py::harmonic on the flat frames, where the last bit of the serial sum decides every bin at once"""
    seen = set()
    for i, (a, lag, cls) in enumerate(hc.classified(oracle, N)):
        if not a["flat"] or a["gated"]:
            continue
        seen |= {c for c in cls if c[0] == "flat"}
        re, _ = hc.oracle_inputs(oracle, hc.frames(N)[i])
        her, inh = fx_numpy.harmonic(np.concatenate([re[:-1], np.zeros(N // 2, np.float32)]), 48000.0 / lag, 24000.0)
        assert hc.same_slots((her, inh), (a["slots"][0], a["slots"][2])), (N, i, hc.describe(cls))
    assert ("flat", "every bin a peak") in seen and ("flat", "no peak") in seen


@pytest.mark.parametrize("N", hc.SIZES)
def test_every_required_class_is_held(oracle, N):
    """every class the table was chosen for, at both rates where the class carries one, from a fresh classification"""
    got = hc.held(oracle, N)
    print("N=%d: %d frames (%d s16-exact); held: %s" % (N, len(hc.CASES[N]), hc.num_s16(N), hc.describe(got)))
    print("N=%d: UNREACHED: %s" % (N, hc.describe(hc.UNREACHED[N])))
    missing = hc.required(N) - got
    assert not missing, (N, hc.describe(missing))
    # the flat frames take an impulse at sample 0 and one at N/2, and both outcomes of the tie
    # (full-mantissa amplitudes given by their bits: the rounding of the serial sum is the point)
    for where in (0, N // 2):
        assert any(c[0] == "fb" and len(c[1]) == 1 and c[1][0][0] == where and a["flat"] and not a["gated"]
                   for c, (a, _, _) in zip(hc.CASES[N], hc.classified(oracle, N))), (N, where)
    assert ("flat", "impulse at 0", "every bin a peak") in got and ("flat", "impulse at N/2", "every bin a peak") in got
    # the gate is straddled by adjacent fp32 amplitudes of one impulse
    one = {c[1][0]: a["gated"] for c, (a, _, _) in zip(hc.CASES[N], hc.classified(oracle, N)) if c[0] == "fb" and len(c[1]) == 1}
    assert any(one.get((n, bits + 1)) is False for (n, bits), gated in one.items() if gated), one


@pytest.mark.parametrize("N", hc.SIZES)
def test_unreached_is_really_absent_and_complete(oracle, N):
    """no chosen frame is of a class listed as unreached, and every class the search looked for is either held or listed"""
    got = hc.held(oracle, N)
    listed = set(hc.UNREACHED[N])
    assert not (listed & got), (N, hc.describe(listed & got))
    for c in hc.wanted(N):
        assert (c in got) != (c in listed), (N, c)
    if N // 128 <= 4:                                                          # U = 2 and 4: a lane has no interior bin
        assert {c for c in listed if c[0] == "tie"} == {("tie", off, "in") for off in (-2, -1, 1)}
    else:
        assert not any(c[0] == "tie" for c in listed)                          # every (offset, j) cell is held
    # what is believed out of reach: no frame holds a bin on the mean that is not part of a flat spectrum, no probe sits at M-2 or M-1,
    # and no sub-harmonic is skipped for falling into f0's bin
    M = N // 2
    for rate in hc.RATES:
        for a, lag, cls in hc.classified(oracle, N, rate):
            if a["gated"]:
                continue
            assert a["flat"] or a["on_mean"] == 0, hc.describe(cls)
            assert a["mag_sum"] != 0.005
            assert not any(kind in ("sub", "harm") and b >= M - 2 for kind, _, b, _ in a["probes"]), hc.describe(cls)
            assert not any(kind == "sub_skipped" for kind, _, _, _ in a["probes"]), hc.describe(cls)


@pytest.mark.parametrize("N", hc.SIZES)
def test_the_frames_tell_every_mutant_apart(oracle, N):
    """for every mutant, and for the frame kernel's and the pair kernel's bins per lane where it depends on them, at least one chosen
    frame's HER, OER or inharmonicity slot has other bits than the unchanged model's"""
    assert hc.UNTOLD[N] == ()
    inputs = [hc.oracle_inputs(oracle, w) for w in hc.frames(N)]
    ref = [hc.model(re, lag, 24000.0) for re, lag in inputs]
    counts = {}
    for mutant, U in hc.mutant_targets(N):
        tellers = [i for i, (re, lag) in enumerate(inputs) if not hc.same_slots(hc.model(re, lag, 24000.0, mutant, U), ref[i])]
        counts[mutant, U] = len(tellers)
        assert tellers, "N=%d: no frame tells %s (%s) apart at %d bins per lane" % (N, mutant, hc.MUTANTS[mutant][0], U)
    print("N=%d: frames that tell each mutant apart: %s" % (N, ", ".join("%s@%d %d" % (m, u, n) for (m, u), n in counts.items())))
    targets = {m for m, _ in hc.mutant_targets(N)}
    assert targets | set(hc.EQUIVALENT) | (set(hc.SEAM_MUTANTS) if N not in hc.PAIR_SIZES else set()) == set(hc.MUTANTS)


@pytest.mark.parametrize("rate", hc.RATES)
@pytest.mark.parametrize("N", hc.SIZES)
def test_the_equivalent_mutants_change_nothing_for_any_lag(N, rate):
    """harmonic_cases.EQUIVALENT, through every lag the search can answer: the reciprocal of the bin width never moves one of the 18
    probes to another bin, and bin 0 is skipped by the floors whether its start frequency is replaced or not"""
    M = N // 2
    nyquist = rate / 2.0
    fr = nyquist / M
    r_fr = 1.0 / fr
    assert Fraction(fr) * M == Fraction(nyquist) and Fraction(r_fr) * Fraction(fr) != 1                 # exact width, inexact reciprocal
    for lag in range(2, N + 1):
        f0 = (nyquist * 2.0) / float(np.float32(lag))
        for freq in [f0] + [f0 / 2.0 ** k for k in range(1, 16)] + [f0 * h for h in (1, 2, 3)]:
            assert math.floor(freq / fr) == math.floor(freq * r_fr), (N, rate, lag, freq)
        fe = fr                                                                # bin 0: start 0 -> fr / 2, end fr
        with_sub = math.floor(max(fr * 0.5, f0) / min(fr * 0.5, f0)) != math.floor(1.0 if fe == f0 else max(fe, f0) / min(fe, f0))
        assert with_sub, (N, rate, lag)                                        # skipped (:232); f0 / 0 = inf is skipped as well
    re = np.zeros(M + 1, np.float32)
    re[0], re[5] = 1.0, 0.5                                                    # and the model agrees: a peak at bin 0, nothing from it
    for lag in (2.0, 7.0, float(N)):
        assert hc.same_slots(hc.model(re, lag, nyquist), hc.model(re, lag, nyquist, "no_fs0"))
        assert hc.same_slots(hc.model(re, lag, nyquist), hc.model(re, lag, nyquist, "recip_fr"))


@pytest.mark.parametrize("rate", hc.RATES)
@pytest.mark.parametrize("N", hc.SIZES)
def test_what_no_slot_can_show(oracle, N, rate):
    """harmonic_cases.NOT_OBSERVABLE, the decisions the issue lists as mutants that the model does not take: the OER slot is the HER
    slot bit for bit in the oracle's own output (RealTimeAnalyser.h:171), so neither OER clamp reaches a slot, although the frames do
    put the odd-even ratio on both sides of 1; no frame's serial sum is 0.005, where alone `<=` at the gate differs from `<`; and no
    harmonic score is negative, where alone the clamp at 0 acts"""
    assert set(hc.NOT_OBSERVABLE) == {"gate_le", "oer_clamp", "her_floor"} and not set(hc.NOT_OBSERVABLE) & set(hc.MUTANTS)
    B, where = hc.batch_layout(N)
    raw, sm = oracle.process_frames(B, N, rate)
    for got in (raw, sm):
        assert np.array_equal(got[:, :, hc.OER].view(np.uint32), got[:, :, hc.HER].view(np.uint32))
    oers = [a["oer"] for a, _, _ in hc.classified(oracle, N, rate) if not a["gated"] and a["odd_e"] > 0.0]
    assert min(oers) < 1.0 < max(oers), oers
    for a, _, cls in hc.classified(oracle, N, rate):
        assert a["mag_sum"] != 0.005 and a["her"] >= 0.0, hc.describe(cls)


def test_a_failure_names_the_class(oracle):
    """what tests/test_gpu_harmonic_cases.py reports (harmonic_cases.assert_held): a made-up kernel whose inharmonicity of one frame is
    one ulp off is told the frame's classes; the oracle's own output passes"""
    N = 1024
    B, where = hc.batch_layout(N)
    want = oracle.process_frames(B, N)
    hc.assert_held(oracle, want, want, B, "default", "the oracle itself")
    k = next(i for i, (_, _, cls) in enumerate(hc.classified(oracle, N)) if ("tie across lanes", -2) in cls)
    c, t = where[k]
    got = (want[0].copy(), want[1])
    got[0][c, t, hc.INHARM] = np.nextafter(got[0][c, t, hc.INHARM], np.float32(2.0))
    with pytest.raises(AssertionError) as e:
        hc.assert_held(oracle, got, want, B, "default", "made up")
    said = str(e.value)
    assert "channel %d frame %d" % (c, t) in said and "tie across lanes -2" in said and "raw harmonic slots differ in" in said, said
