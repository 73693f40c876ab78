"""The HIP kernels of the legacy offline analyser (csrc/fx_offline.hip) at their gates, ties and non-finite inputs: every case of
tests/offline_cases.py against what the reference's own header returned (tests/golden/offline/edge_cases.npz) and against the oracle, bit
for bit -- but for spread and flatness, which go through pow(): rtol 2e-7 as in tests/test_offline.py where the value is a normal number,
class and sign exactly where it is 0, inf or NaN (tests/test_offline_edges_cpu.py holds that no case yields a subnormal).  Then the C
ABI around the kernels: device-resident buffers, every refusal, and staging buffers that grow and are reused."""
import ctypes
import os

import numpy as np
import pytest

import offline_cases as oc
from test_offline import same

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offline", "edge_cases.npz")
F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def pow_close(got, want):
    """spread and flatness: rtol 2e-7 on normal numbers, the bits (a NaN equals a NaN) on everything else"""
    got, want = np.asarray(got), np.asarray(want)
    normal = np.isfinite(want) & (np.abs(want) >= np.finfo(np.float32).tiny)
    if not same(np.where(normal, F32(1), got), np.where(normal, F32(1), want)):
        return False
    return bool(np.all(np.abs(got[normal].astype(np.float64) - want[normal]) <= 2e-7 * np.abs(want[normal].astype(np.float64))))


def spectral_same(got, want):
    return same(got[:, [0, 3]], want[:, [0, 3]]) and pow_close(got[:, [1, 2]], want[:, [1, 2]])


def test_zero_crossings(gpu_fx, oracle, golden):
    for k, c in enumerate(oc.zero_cross_cases()):
        got = gpu_fx.offline.AudioAnalyser(c["audio"].shape[0]).analyse_normalised_zero_crosses(c["audio"], c["num_downsamples"])
        assert same(got, golden["zc_%d" % k]), (c["label"], got, golden["zc_%d" % k])
        assert same(got, oracle.offline_zero_crosses(c["audio"], c["num_downsamples"])), c["label"]


def test_log_attack_time(gpu_fx, oracle, golden):
    """Without the NaN skip in the per-thread scan (and thread 0 starting the combine from env[0]) a NaN early in a thread's stride hides the
    maximum behind it: the kernel before the fix returned index 238 for 261 on "n 513 NaN at 5 max at 261" and index 0 for 300 on "NaNs at
    1..255 max at 300 and 400"."""
    an = gpu_fx.offline.AudioAnalyser(1)
    wrong = []
    for k, c in enumerate(oc.attack_cases()):
        got = an.set_log_attack_time(c["env"], c["num_input_samples"], c["num_downsamples"], c["sample_rate"])
        want = oracle.offline_log_attack_time(c["env"], c["num_input_samples"], c["num_downsamples"], c["sample_rate"])
        if not (same(got, golden["lat_%d" % k]) and same(got, want)):
            wrong.append((c["label"], "index %d for %d" % (oc.attack_index(got, c), c["index"]), got, golden["lat_%d" % k]))
    assert not wrong, wrong


def test_fft_lbp(gpu_fx, oracle, golden):
    for k, c in enumerate(oc.lbp_cases()):
        got = gpu_fx.offline.AudioAnalyser(c["cur"].shape[0]).calculate_fft_lbp(c["cur"], c["prev"])
        for g, name in zip(got, ("bits", "hi", "act")):
            assert same(g, golden["lbp_%d_%s" % (k, name)]), (c["label"], name, g, golden["lbp_%d_%s" % (k, name)])
        assert all(same(a, b) for a, b in zip(got, oracle.offline_fft_lbp(c["cur"], c["prev"]))), c["label"]


def test_harmonic_characteristics(gpu_fx, oracle, golden):
    for k, c in enumerate(oc.harmonic_cases()):
        T, C, B = c["frames"].shape
        an = gpu_fx.offline.AudioAnalyser(C, c["nyquist"])
        pf = np.zeros(C)
        for t in range(T):
            got = an.calculate_harmonic_characteristics(c["frames"][t])
            assert same(got, golden["hc_%d_out" % k][t]), (c["label"], t, got, golden["hc_%d_out" % k][t])
            assert same(an.previous_f0, golden["hc_%d_prev" % k][t]), (c["label"], t, an.previous_f0, golden["hc_%d_prev" % k][t])
            assert same(got, oracle.offline_harmonic_characteristics(c["frames"][t], c["nyquist"], pf)) and same(an.previous_f0, pf), (c["label"], t)


def test_spectral_characteristics(gpu_fx, oracle, golden):
    for k, c in enumerate(oc.spectral_cases()):
        T, C, B = c["frames"].shape
        an = gpu_fx.offline.AudioAnalyser(C, c["nyquist"])
        pb = np.zeros((C, B))
        for t in range(T):
            got = an.calculate_spectral_characteristics(c["frames"][t])
            want = golden["sc_%d_out" % k][t]
            assert spectral_same(got, want), (c["label"], t, got, want)
            assert same(an.previous_bin_magnitudes, golden["sc_%d_prev" % k][t].astype(np.float64)), (c["label"], t)
            assert spectral_same(got, oracle.offline_spectral_characteristics(c["frames"][t], c["nyquist"], pb)) and same(an.previous_bin_magnitudes, pb), (c["label"], t)
        an.reset()                                                     # the first frame after reset() is the first frame after construction
        assert spectral_same(an.calculate_spectral_characteristics(c["frames"][0]), golden["sc_%d_out" % k][0]), c["label"]
        assert same(an.previous_bin_magnitudes, golden["sc_%d_prev" % k][0].astype(np.float64)), c["label"]


def test_spectral_slope(gpu_fx, oracle, golden):
    for k, c in enumerate(oc.slope_cases()):
        got = gpu_fx.offline.AudioAnalyser(c["mags"].shape[0]).calculate_normalised_spectral_slope(c["mags"])
        assert same(got, golden["slope_%d" % k]), (c["label"], got, golden["slope_%d" % k])
        assert same(got, oracle.offline_spectral_slope(c["mags"])), c["label"]


def test_auto_correlation(gpu_fx, oracle, golden):
    for k, c in enumerate(oc.autocorrelation_cases()):
        prod, peaks, freqs = gpu_fx.offline.AudioAnalyser(c["data"].shape[0], c["nyquist"]).analyse_auto_correlation(c["data"])
        assert same(prod, golden["ac_%d_prod" % k]) and same(freqs, golden["ac_%d_freq" % k]), (c["label"], peaks, freqs, golden["ac_%d_freq" % k])
        want_prod = oracle.offline_conjugate_multiplication(c["data"])
        wp, wf = oracle.offline_auto_correlation(want_prod, c["nyquist"])
        assert same(prod, want_prod) and same(peaks, wp) and same(freqs, wf) and np.array_equal(peaks, c["peak"]), (c["label"], peaks, wp)


# ---- the C ABI around the kernels ----
def vp(a):
    return ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data_as(ctypes.c_void_p)


def seven_inputs(rng, C, B):
    """one small input for each entry, sized by B"""
    n = max(B // 2, 1)
    env = np.abs(rng.normal(0, 1, B)).astype(F32)
    mags = np.abs(rng.normal(0, 1.0, (C, B))).astype(F32)
    if B >= 16:
        mags[:, B // 8::B // 8] += 9.0
    return dict(audio=rng.normal(0, 1, (C, 3 * B + 1)).astype(F32), nd=3, env=env, cur=np.abs(rng.normal(0, 0.3, (C, B))).astype(F32),
                prev=np.abs(rng.normal(0, 0.3, (C, B))).astype(F32), mags=mags, data=rng.normal(0, 1, (C, n, 2)).astype(F32))


def run_seven(an, x):
    """the seven entries through the binding (host buffers): every output, in a fixed order"""
    B = x["mags"].shape[1]
    out = [an.analyse_normalised_zero_crosses(x["audio"], x["nd"]), np.array([an.set_log_attack_time(x["env"], 44100, x["env"].shape[0], 44100)])]
    out += list(an.calculate_fft_lbp(x["cur"], x["prev"]))
    if B >= 4:
        out += [an.calculate_harmonic_characteristics(x["mags"]), an.previous_f0]
    out += [an.calculate_spectral_characteristics(x["mags"]), an.previous_bin_magnitudes, an.calculate_spectral_characteristics(x["cur"]), an.previous_bin_magnitudes]
    out += [an.calculate_normalised_spectral_slope(x["mags"])]
    out += list(an.analyse_auto_correlation(x["data"]))
    return out


def test_device_buffers_give_the_bits_of_the_host_calls(gpu_fx):
    import torch
    C, B, nyq = 3, 65, 24000.0
    x = seven_inputs(np.random.default_rng(5), C, B)
    host = run_seven(gpu_fx.offline.AudioAnalyser(C, nyq), x)
    an = gpu_fx.offline.AudioAnalyser(C, nyq)
    L, h, DEV, check = an._lib, an._h, gpu_fx.capi.MEM_DEVICE, gpu_fx.capi.check
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    empty = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    d = {k: dev(v) for k, v in x.items() if k != "nd"}
    zc, lat = empty((C, x["nd"]), torch.float32), empty((1,), torch.float32)
    bits, hi, act = empty((C, B), torch.uint8), empty((C,), torch.float32), empty((C,), torch.float32)
    hc, sc1, sc2, slope = empty((C, 3), torch.float32), empty((C, 4), torch.float32), empty((C, 4), torch.float32), empty((C,), torch.float32)
    peaks, freqs = empty((C,), torch.int32), empty((C,), torch.float64)
    torch.cuda.synchronize()                                           # the analyser's stream is its own: the uploads are complete before it reads
    check(L.fx_offline_zero_crosses(h, vp(d["audio"]), x["audio"].shape[1], x["nd"], vp(zc), DEV))
    check(L.fx_offline_log_attack_time(h, vp(d["env"]), B, 44100, B, 44100, vp(lat), DEV))
    check(L.fx_offline_fft_lbp(h, vp(d["cur"]), vp(d["prev"]), B, vp(bits), vp(hi), vp(act), DEV))
    check(L.fx_offline_harmonic_characteristics(h, vp(d["mags"]), B, vp(hc), DEV))
    check(L.fx_offline_sync(h))
    pf = an.previous_f0
    check(L.fx_offline_spectral_characteristics(h, vp(d["mags"]), B, vp(sc1), DEV))
    check(L.fx_offline_sync(h))
    an._bins = B
    pb1 = an.previous_bin_magnitudes
    check(L.fx_offline_spectral_characteristics(h, vp(d["cur"]), B, vp(sc2), DEV))
    check(L.fx_offline_spectral_slope(h, vp(d["mags"]), B, vp(slope), DEV))
    check(L.fx_offline_auto_correlation(h, vp(d["data"]), x["data"].shape[1], vp(peaks), vp(freqs), DEV))
    check(L.fx_offline_sync(h))                                        # results are read after fx_offline_sync
    got = [t.cpu().numpy() for t in (zc, lat, bits, hi, act, hc)] + [pf, sc1.cpu().numpy(), pb1, sc2.cpu().numpy(), an.previous_bin_magnitudes,
                                                                     slope.cpu().numpy(), d["data"].cpu().numpy(), peaks.cpu().numpy(), freqs.cpu().numpy()]
    assert len(got) == len(host)
    for i, (a, b) in enumerate(zip(got, host)):
        assert same(a, b), (i, a, b)
    assert not same(d["data"].cpu().numpy(), x["data"])                # the caller's device buffer holds the products: multiplied in place
    assert same(d["mags"].cpu().numpy(), x["mags"]) and same(d["audio"].cpu().numpy(), x["audio"])      # every other input is read only


def test_every_refusal_is_an_invalid_argument_and_leaves_the_analyser_as_it_was(gpu_fx):
    C, B, nyq = 2, 65, 24000.0
    INVALID, HOST = gpu_fx.capi.FX_ERR_INVALID_ARGUMENT, gpu_fx.capi.MEM_HOST
    x = seven_inputs(np.random.default_rng(6), C, B)
    an, twin = gpu_fx.offline.AudioAnalyser(C, nyq), gpu_fx.offline.AudioAnalyser(C, nyq)
    first = run_seven(an, x)
    assert all(same(a, b) for a, b in zip(first, run_seven(twin, x)))
    pf, pb = an.previous_f0, an.previous_bin_magnitudes
    assert pf.any() and pb.any()
    L, h = an._lib, an._h
    big = np.ones((C, oc.MAX_BINS + 1), F32)                           # (large enough for whatever a refusal that failed to refuse would read)
    out = np.zeros((C, oc.MAX_BINS + 1), F32)
    bits, ints, dbl = np.zeros((C, oc.MAX_BINS + 1), np.uint8), np.zeros(C, np.int32), np.zeros(C, np.float64)
    refusals = []
    for name in ("fx_offline_harmonic_characteristics", "fx_offline_spectral_characteristics", "fx_offline_spectral_slope"):
        for bins in (oc.MAX_BINS + 1, 0):
            refusals.append(("%s num_bins %d" % (name, bins), getattr(L, name)(h, vp(big), bins, vp(out), HOST)))
    refusals.append(("harmonic num_bins 3", L.fx_offline_harmonic_characteristics(h, vp(big), 3, vp(out), HOST)))
    refusals.append(("spectral: another frame size", L.fx_offline_spectral_characteristics(h, vp(big), B + 1, vp(out), HOST)))
    refusals.append(("zero crossings num_downsamples 0", L.fx_offline_zero_crosses(h, vp(big), 100, 0, vp(out), HOST)))
    refusals.append(("zero crossings num_downsamples num_samples + 1", L.fx_offline_zero_crosses(h, vp(big), 100, 101, vp(out), HOST)))
    refusals.append(("attack time sample_rate 999", L.fx_offline_log_attack_time(h, vp(big), 100, 100, 100, 999, vp(out), HOST)))
    refusals.append(("attack time envelope length 0", L.fx_offline_log_attack_time(h, vp(big), 0, 100, 100, 44100, vp(out), HOST)))
    refusals.append(("fft_lbp num_bins 0", L.fx_offline_fft_lbp(h, vp(big), vp(big), 0, vp(bits), vp(out), vp(out), HOST)))
    refusals.append(("auto-correlation num_items 0", L.fx_offline_auto_correlation(h, vp(big), 0, vp(ints), vp(dbl), HOST)))
    for kind in (2, -1):                                               # an unknown memory kind, at every entry
        refusals += [("zero crossings kind %d" % kind, L.fx_offline_zero_crosses(h, vp(big), 100, 4, vp(out), kind)),
                     ("attack time kind %d" % kind, L.fx_offline_log_attack_time(h, vp(big), 100, 100, 100, 44100, vp(out), kind)),
                     ("fft_lbp kind %d" % kind, L.fx_offline_fft_lbp(h, vp(big), vp(big), B, vp(bits), vp(out), vp(out), kind)),
                     ("harmonic kind %d" % kind, L.fx_offline_harmonic_characteristics(h, vp(big), B, vp(out), kind)),
                     ("spectral kind %d" % kind, L.fx_offline_spectral_characteristics(h, vp(big), B, vp(out), kind)),
                     ("slope kind %d" % kind, L.fx_offline_spectral_slope(h, vp(big), B, vp(out), kind)),
                     ("auto-correlation kind %d" % kind, L.fx_offline_auto_correlation(h, vp(big), B, vp(ints), vp(dbl), kind))]
    refusals += [("zero crossings null in", L.fx_offline_zero_crosses(h, None, 100, 4, vp(out), HOST)),
                 ("zero crossings null out", L.fx_offline_zero_crosses(h, vp(big), 100, 4, None, HOST)),
                 ("zero crossings null analyser", L.fx_offline_zero_crosses(None, vp(big), 100, 4, vp(out), HOST)),
                 ("attack time null in", L.fx_offline_log_attack_time(h, None, 100, 100, 100, 44100, vp(out), HOST)),
                 ("attack time null out", L.fx_offline_log_attack_time(h, vp(big), 100, 100, 100, 44100, None, HOST)),
                 ("fft_lbp null cur", L.fx_offline_fft_lbp(h, None, vp(big), B, vp(bits), vp(out), vp(out), HOST)),
                 ("fft_lbp null prev", L.fx_offline_fft_lbp(h, vp(big), None, B, vp(bits), vp(out), vp(out), HOST)),
                 ("fft_lbp null bits", L.fx_offline_fft_lbp(h, vp(big), vp(big), B, None, vp(out), vp(out), HOST)),
                 ("fft_lbp null highest", L.fx_offline_fft_lbp(h, vp(big), vp(big), B, vp(bits), None, vp(out), HOST)),
                 ("fft_lbp null activity", L.fx_offline_fft_lbp(h, vp(big), vp(big), B, vp(bits), vp(out), None, HOST)),
                 ("harmonic null in", L.fx_offline_harmonic_characteristics(h, None, B, vp(out), HOST)),
                 ("harmonic null out", L.fx_offline_harmonic_characteristics(h, vp(big), B, None, HOST)),
                 ("spectral null in", L.fx_offline_spectral_characteristics(h, None, B, vp(out), HOST)),
                 ("spectral null out", L.fx_offline_spectral_characteristics(h, vp(big), B, None, HOST)),
                 ("slope null in", L.fx_offline_spectral_slope(h, None, B, vp(out), HOST)),
                 ("slope null out", L.fx_offline_spectral_slope(h, vp(big), B, None, HOST)),
                 ("auto-correlation null data", L.fx_offline_auto_correlation(h, None, B, vp(ints), vp(dbl), HOST)),
                 ("auto-correlation null peak", L.fx_offline_auto_correlation(h, vp(big), B, None, vp(dbl), HOST)),
                 ("auto-correlation null frequency", L.fx_offline_auto_correlation(h, vp(big), B, vp(ints), None, HOST)),
                 ("previous f0 null out", L.fx_offline_get_previous_f0(h, None)), ("sync null analyser", L.fx_offline_sync(None)), ("reset null analyser", L.fx_offline_reset(None))]
    assert [(name, st) for name, st in refusals if st != INVALID] == []
    assert not out.any() and not bits.any() and (big == 1).all()        # nothing was written, nothing was multiplied in place
    assert same(an.previous_f0, pf) and same(an.previous_bin_magnitudes, pb)
    y = seven_inputs(np.random.default_rng(7), C, B)
    assert all(same(a, b) for a, b in zip(run_seven(an, y), run_seven(twin, y)))       # and the next good call is what it would have been


def test_one_analyser_through_growing_and_shrinking_sizes_equals_fresh_analysers(gpu_fx):
    """The staging buffers only grow: after the largest size every smaller call runs in a buffer that still holds the larger call's bytes."""
    C, nyq = 2, 24000.0
    rng = np.random.default_rng(8)
    an = gpu_fx.offline.AudioAnalyser(C, nyq)
    for B in (1, 5, 257, 1025, 1025, 257, 5, 1):
        x = seven_inputs(rng, C, B)
        an.reset()                                                     # (previousBinMagnitudes has one size per analyser; reset() keeps the staging buffers)
        got, want = run_seven(an, x), run_seven(gpu_fx.offline.AudioAnalyser(C, nyq), x)
        assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want)), B
