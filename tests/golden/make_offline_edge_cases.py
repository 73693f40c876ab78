"""Build container only: expected outputs of the reference's LEGACY offline analyser (AudioAnalysis.h, compiled unmodified against
tools/refdiff/juce_standin.h) on the edge cases of tests/offline_cases.py -> tests/golden/offline/edge_cases.npz.  The inputs are
regenerated from the builders, so the fixture holds expected outputs only (keys: <family>_<case number>[_<output>]).

    python tests/golden/make_offline_edge_cases.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "refdiff"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATH = os.path.join(ROOT, "tests", "golden", "offline", "edge_cases.npz")


def main():
    import refdiff
    import offline_cases as oc
    assert refdiff.legacy_available(), "needs the reference's headers"
    out = {"source": "AudioAnalyser (ref AudioAnalysis.h) compiled unmodified against tools/refdiff/juce_standin.h; tools/refdiff/refdiff_legacy.cpp; inputs: tests/offline_cases.py"}
    for k, c in enumerate(oc.zero_cross_cases()):
        out["zc_%d" % k] = refdiff.legacy_zero_crosses(c["audio"], c["num_downsamples"])
    for k, c in enumerate(oc.attack_cases()):
        out["lat_%d" % k] = np.float32(refdiff.legacy_log_attack_time(c["env"], c["num_input_samples"], c["num_downsamples"], c["sample_rate"]))
    for k, c in enumerate(oc.lbp_cases()):
        out["lbp_%d_bits" % k], out["lbp_%d_hi" % k], out["lbp_%d_act" % k] = refdiff.legacy_fft_lbp(c["cur"], c["prev"])
    for k, c in enumerate(oc.harmonic_cases()):
        out["hc_%d_out" % k], out["hc_%d_prev" % k] = refdiff.legacy_harmonic_characteristics(c["frames"], c["nyquist"])
    for k, c in enumerate(oc.spectral_cases()):
        # previousBinMagnitudes after EVERY frame: the harness returns it after the last one, so the frames are run as prefixes
        T = c["frames"].shape[0]
        prevs = []
        for t in range(T):
            o, pb = refdiff.legacy_spectral_characteristics(c["frames"][:t + 1], c["nyquist"])
            assert np.array_equal(pb, pb.astype(np.float32).astype(np.float64))     # widened float32 magnitudes (or the initial zeros): stored as float32
            prevs.append(pb.astype(np.float32))
        out["sc_%d_out" % k], out["sc_%d_prev" % k] = o, np.stack(prevs)
    for k, c in enumerate(oc.slope_cases()):
        out["slope_%d" % k] = refdiff.legacy_spectral_slope(c["mags"])
    for k, c in enumerate(oc.autocorrelation_cases()):
        out["ac_%d_prod" % k], out["ac_%d_freq" % k] = refdiff.legacy_auto_correlation(c["data"], c["nyquist"])
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes,", len(out) - 1, "arrays")


if __name__ == "__main__":
    main()
