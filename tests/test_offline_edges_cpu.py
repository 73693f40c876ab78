"""The legacy offline analyser at its gates, ties and non-finite inputs, without a GPU: the oracle (oracle/fx_offline.c) equals what the
reference's own header returned for every case of tests/offline_cases.py (tests/golden/offline/edge_cases.npz, made by
tests/golden/make_offline_edge_cases.py from the unmodified AudioAnalysis.h), bit for bit, and every case lands where its builder says:
the side of the gate, the index that wins, the F0.  tests/test_gpu_offline_edges.py holds the HIP kernels to the same fixture."""
import os

import numpy as np
import pytest

import offline_cases as oc
from test_offline import same

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offline", "edge_cases.npz")
F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    assert "AudioAnalysis.h" in str(g["source"])
    return g


def pos_zero(a):
    a = np.asarray(a)
    return not a.any() and not np.signbit(a).any()


def test_the_fixture_holds_every_case_and_nothing_else(golden):
    want = {"source"}
    for name, cases, outs in (("zc", oc.zero_cross_cases(), ("",)), ("lat", oc.attack_cases(), ("",)), ("lbp", oc.lbp_cases(), ("_bits", "_hi", "_act")),
                              ("hc", oc.harmonic_cases(), ("_out", "_prev")), ("sc", oc.spectral_cases(), ("_out", "_prev")),
                              ("slope", oc.slope_cases(), ("",)), ("ac", oc.autocorrelation_cases(), ("_prod", "_freq"))):
        labels = [c["label"] for c in cases]
        assert len(set(labels)) == len(labels), name
        want |= {"%s_%d%s" % (name, k, o) for k in range(len(cases)) for o in outs}
    assert set(golden.files) == want
    assert os.path.getsize(GOLDEN) < 100 * 1024                       # the order of magnitude of cases.npz


def test_the_builders_keep_to_the_sizes_they_promise():
    sizes = {1, 4, 5, 63, 64, 65, 255, 256, 257, 513, 1025}
    for c in oc.attack_cases():
        assert c["env"].shape[0] in sizes, c["label"]
    for c in oc.lbp_cases():
        assert c["cur"].shape[0] <= 8 and c["cur"].shape[1] in sizes, c["label"]
    for cases, key in ((oc.harmonic_cases(), "frames"), (oc.spectral_cases(), "frames"), (oc.slope_cases(), "mags")):
        big = 0
        for c in cases:
            assert c[key].shape[-2] <= 8, c["label"]
            big += c[key].shape[-1] == oc.MAX_BINS
            assert c[key].shape[-1] in sizes | {oc.MAX_BINS}, c["label"]
        assert big == 1                                                # one case at the LDS maximum for each kernel with dynamic LDS
    for c in oc.autocorrelation_cases():
        assert c["data"].shape[0] <= 8 and c["data"].shape[1] in sizes, c["label"]
    assert {c["audio"].shape[1] // c["num_downsamples"] for c in oc.zero_cross_cases()} == {1, 2, 256, 257, 258}
    assert all(c["audio"].shape[1] % c["num_downsamples"] for c in oc.zero_cross_cases()[1:])      # leftover samples, and they are NaNs
    assert all(np.isnan(c["audio"][:, -2:]).all() for c in oc.zero_cross_cases()[1:])


def test_zero_crossings(oracle, golden):
    for k, c in enumerate(oc.zero_cross_cases()):
        got = oracle.offline_zero_crosses(c["audio"], c["num_downsamples"])
        assert same(got, golden["zc_%d" % k]), c["label"]
        step = c["audio"].shape[1] // c["num_downsamples"]
        assert same(got, (c["counts"].astype(F32) * F32(2.0) / F32(step)).astype(F32)), (c["label"], got)       # :538
    pairs = oc.ZC_PAIRS
    firsts = {(a, b) for a, b, _ in pairs}
    for s in (1.0, -1.0):                                              # what the issue asks for is there
        assert {(s, -s * 2.0 ** -25), (s, -s * 2.0 ** -24), (s, -s * 2.0 ** -23)} <= firsts
    assert F32(1.0) - F32(-2.0 ** -24) == F32(1.0) and F32(1.0) - F32(-2.0 ** -23) > F32(1.0)


def test_log_attack_time(oracle, golden):
    """A NaN in the envelope: the header's answer passes through findMinMax of the JUCE stand-in (tools/refdiff/juce_standin.h) -- a plain loop
    from p[0] on `>`, which is what the oracle restates; JUCE's own findMinMax is a SIMD loop whose treatment of NaNs this fixture does not hold."""
    cases = oc.attack_cases()
    for k, c in enumerate(cases):
        got = oracle.offline_log_attack_time(c["env"], c["num_input_samples"], c["num_downsamples"], c["sample_rate"])
        assert same(got, golden["lat_%d" % k]), c["label"]
        assert oc.attack_index(got, c) == c["index"], (c["label"], got)
        if c["index"] == 0:
            assert np.isneginf(got)
    labels = " | ".join(c["label"] for c in cases)
    for n in (1, 255, 256, 257, 513):
        assert "n %d max at 0" % n in labels and "n %d max at n-1" % n in labels
    # the suspected bug's case is what it says: a NaN at t in 1..255, the only maximum 256 further on
    c = cases[[x["label"] for x in cases].index("n 513 NaN at 5 max at 261")]
    assert np.isnan(c["env"][5]) and c["env"][261] == 50.0 and np.nanmax(np.delete(c["env"], 261)) < 5.0 and c["index"] == 261


def test_fft_lbp(oracle, golden):
    for k, c in enumerate(oc.lbp_cases()):
        bits, hi, act = oracle.offline_fft_lbp(c["cur"], c["prev"])
        assert same(bits, golden["lbp_%d_bits" % k]) and same(hi, golden["lbp_%d_hi" % k]) and same(act, golden["lbp_%d_act" % k]), c["label"]
        B = c["cur"].shape[1]
        assert same(bits, c["bits"]), (c["label"], np.flatnonzero(bits != c["bits"]))
        assert same(hi, (c["highest"].astype(F32) / F32(B)).astype(F32)) and same(act, (c["count"].astype(F32) / F32(B)).astype(F32)), c["label"]
    # the threshold row: exactly on it, one fp32 step either side, from both signs; operands whose subtraction rounds
    T = oc.THRESHOLD
    c = oc.lbp_cases()[0]
    with np.errstate(invalid="ignore"):
        d = np.abs(c["cur"][0] - c["prev"][0])                          # fp32, as the reference subtracts
        assert ((d > T) == c["bits"][0].astype(bool)).all()
    for v, bit in ((T, 0), (oc.up(T), 1), (oc.down(T), 0)):
        assert ((d == v) & (c["bits"][0] == bit)).sum() >= 2
    for a, b, bit in oc.lbp_rounding_triples():
        assert (float(a) - float(b) != float(F32(a - b))) and abs(float(F32(a - b))) in (float(T), float(oc.up(T)))


def test_harmonic_characteristics(oracle, golden):
    for k, c in enumerate(oc.harmonic_cases()):
        T, C, B = c["frames"].shape
        pf = np.zeros(C)
        for t in range(T):
            before = pf.copy()
            out = oracle.offline_harmonic_characteristics(c["frames"][t], c["nyquist"], pf)
            assert same(out, golden["hc_%d_out" % k][t]) and same(pf, golden["hc_%d_prev" % k][t]), (c["label"], t, out, golden["hc_%d_out" % k][t])
            assert same(out[:, 0], c["f0"][t].astype(F32)), (c["label"], t, out[:, 0], c["f0"][t])
            assert same(pf, c["previous"][t]), (c["label"], t, pf)
            for ch in range(C):
                if c["gated"][t, ch]:
                    assert pos_zero(out[ch]) and pf[ch] == before[ch] != 0.0, (c["label"], t, ch)
                    assert not (oc.serial_sum(c["frames"][t, ch]) >= 0.001)
                else:
                    assert not (oc.serial_sum(c["frames"][t, ch]) < 0.001), (c["label"], t, ch)
        for (t, ch), her in c["her"].items():
            assert golden["hc_%d_out" % k][t, ch, 1] == F32(her), (c["label"], t, ch)
    gate = oc.harmonic_cases()[0]
    sums = [oc.serial_sum(gate["frames"][1, ch]) for ch in range(4)]
    assert sums[0] == np.nextafter(0.001, 0.0) and sums[1] == 0.001 and sums[2] == np.nextafter(0.001, 1.0) and np.isnan(sums[3])


def test_spectral_characteristics(oracle, golden):
    tiny = float(np.finfo(np.float32).tiny)
    for k, c in enumerate(oc.spectral_cases()):
        T, C, B = c["frames"].shape
        pb = np.zeros((C, B))
        for t in range(T):
            before = pb.copy()
            out = oracle.offline_spectral_characteristics(c["frames"][t], c["nyquist"], pb)
            want = golden["sc_%d_out" % k][t]
            assert same(out, want), (c["label"], t, out, want)
            assert same(pb, golden["sc_%d_prev" % k][t].astype(np.float64)), (c["label"], t)
            for ch in range(C):
                s = oc.serial_sum(c["frames"][t, ch])
                assert bool(c["gated"][t, ch]) == (not s > 0.001), (c["label"], t, ch, s)
                if c["gated"][t, ch]:
                    assert pos_zero(out[ch]) and same(pb[ch], before[ch]) and before[ch].any(), (c["label"], t, ch)
                else:
                    assert same(pb[ch], c["frames"][t, ch].astype(np.float64)), (c["label"], t, ch)
                # spread and flatness go through pow(): either a normal number (the GPU test's rtol applies) or decided without pow's rounding
                # -- a product of 0, inf or NaN, or a NaN centroid -- never a subnormal
                p = oc.serial_product(c["frames"][t, ch])
                assert p == 0.0 or not np.isfinite(p) or abs(p) >= np.finfo(np.float64).tiny, (c["label"], t, ch, p)
                for v in out[ch, 1:3]:
                    assert v == 0.0 or not np.isfinite(v) or abs(float(v)) >= tiny, (c["label"], t, ch, v)
        for (t, ch), flux in c["flux"].items():
            assert same(golden["sc_%d_out" % k][t, ch, 3], F32(flux)), (c["label"], t, ch, golden["sc_%d_out" % k][t, ch, 3], flux)
        for (t, ch), flat in c["flatness"].items():
            assert same(golden["sc_%d_out" % k][t, ch, 2], F32(flat)), (c["label"], t, ch)
    gate = oc.spectral_cases()[0]
    sums = [oc.serial_sum(gate["frames"][1, ch]) for ch in range(4)]
    assert sums[0] == np.nextafter(0.001, 0.0) and sums[1] == 0.001 and sums[2] == np.nextafter(0.001, 1.0) and np.isnan(sums[3])


def test_spectral_slope(oracle, golden):
    for k, c in enumerate(oc.slope_cases()):
        got = oracle.offline_spectral_slope(c["mags"])
        assert same(got, golden["slope_%d" % k]), (c["label"], got, golden["slope_%d" % k])
        for ch in range(c["mags"].shape[0]):
            with np.errstate(invalid="ignore"):
                peak = np.nanmax(np.abs(c["mags"][ch]))
            assert bool(c["gated"][ch]) == (not float(peak) > 0.0001), (c["label"], ch)
            if c["gated"][ch]:
                assert pos_zero(got[ch]), (c["label"], ch)
            if c["nan"][ch]:
                assert np.isnan(got[ch]), (c["label"], ch, got[ch])
            if c["finite"][ch]:
                assert np.isfinite(got[ch]) and got[ch] != 0.0, (c["label"], ch, got[ch])
    c = oc.slope_cases()[0]
    assert c["gated"].tolist() == [True, bool(not float(F32(1e-4)) > 0.0001), False] * 2


def test_auto_correlation(oracle, golden):
    for k, c in enumerate(oc.autocorrelation_cases()):
        prod = oracle.offline_conjugate_multiplication(c["data"])
        assert same(prod, golden["ac_%d_prod" % k]), c["label"]
        peaks, freqs = oracle.offline_auto_correlation(prod, c["nyquist"])
        assert same(freqs, golden["ac_%d_freq" % k]), c["label"]
        assert np.array_equal(peaks, c["peak"]), (c["label"], peaks)
        frpb = c["nyquist"] / c["data"].shape[1]
        assert same(freqs, c["peak"] * frpb + frpb / 2.0), c["label"]
