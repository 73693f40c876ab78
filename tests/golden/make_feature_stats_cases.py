"""Build container only: what the reference's own header (AudioFeatures.h, compiled unmodified against tools/refdiff/juce_standin.h by
tools/refdiff/refdiff_stats.cpp) derives from seeded one-channel feature rows -> tests/golden/offline/feature_stats.npz: getFeatureRange,
getDiscreteFeatureDistribution, SmoothedFeatures::updateValues sequences and FeatureSpace folds.  Inputs are regenerated from the seed by
feature_stats_inputs() (the tests import it), so the fixture holds expected outputs only.  The distribution cases hold no NaN (std::sort is
undefined on one): where a NaN sorts is the library's own rule, held to the model alone.

    python tests/golden/make_feature_stats_cases.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "refdiff"))

F32 = np.float32
SORT_CHUNK = 8192                   # FX_OFFLINE_SORT_CHUNK


def _f(*v):
    return np.array(v, F32)


def wide_magnitudes(rng, n):
    """both signs, magnitudes from 1e-8 to 1e8: the order of a float sum shows"""
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n)).astype(F32)


def feature_stats_inputs():
    """{"ranges": [row, ...], "distributions": [(row, brackets), ...], "smoothing": [(depth, values [updates][9]), ...], "spaces": [[n][7], ...]}"""
    rng = np.random.default_rng(20260611)
    noise = rng.normal(0, 1, 3 * SORT_CHUNK).astype(F32)
    nan0 = noise[:65].copy(); nan0[0] = np.nan
    nans = noise[:65].copy(); nans[7] = np.nan; nans[64] = np.nan
    last = noise[:257].copy(); last[-1] = -100.0
    far = np.ones(1000, F32); far[70] = -0.0; far[300] = 0.0; far[999] = 0.0       # zeros as the minimum, far apart
    ranges = [noise[:257],
              nan0, nans,                                                          # a NaN at row[0]; NaNs elsewhere
              _f(0.0, -0.0, 1, 2), _f(-0.0, 0.0, 1, 2),                            # zero as the minimum, at row[0] ...
              _f(0.0, -0.0, -1, -2), _f(-0.0, 0.0, -1, -2),                        # ... and as the maximum
              _f(1, -0.0, 0.0, 3), _f(1, 0.0, -0.0, 3), _f(-1, 0.0, -0.0, -3), _f(-1, -0.0, 0.0, -3),       # ... and behind it
              far, -far,
              _f(1, -np.inf, 5, np.inf, 2), _f(np.inf, 1, -np.inf), _f(-np.inf, np.inf),
              last, _f(3.5), _f(2, 1), noise[:1000]]
    quantised = (np.floor(rng.uniform(0, 8, 257)) / 8 - 0.5).astype(F32)           # 8 levels: long runs of ties
    zeros = rng.choice(_f(0.0, -0.0, 1.0, -1.0), 64).astype(F32)
    infs = noise[:64].copy(); infs[3] = np.inf; infs[40] = -np.inf; infs[41] = np.inf
    tiny = noise[:65].copy(); tiny[::3] = (rng.integers(-200, 200, 22) * F32(1e-45)).astype(F32)      # subnormals beside normals
    distributions = [(noise[:1000], 10), (wide_magnitudes(rng, 1000), 3), (wide_magnitudes(rng, 1024), 1), (quantised, 10),
                     (np.sort(noise[:64]), 1), (np.sort(noise[:65])[::-1].copy(), 3), (zeros, 4), (infs, 1), (infs, 4), (tiny, 5),
                     (_f(3.5), 1), (_f(2, 1), 3), (noise[:7], 7), (noise[:7], 8), (noise[:7], 3),
                     (noise[:SORT_CHUNK + 3], 10), (wide_magnitudes(rng, 2 * SORT_CHUNK + 5), 3)]
    smoothing = [(depth, (rng.normal(0, 1, (25, 9)) * 10.0 ** rng.integers(-3, 4, 9)).astype(F32)) for depth in (1, 2, 10)]
    typical = np.empty((5, 7), F32)
    typical[:, 0] = _f(-0.3, 0.5, -1.2, 0.1, -0.7)                                 # attack: Range (attack, 0.0f)
    for k in (1, 3, 5):
        a, b = rng.normal(0, 1, 5), rng.normal(0, 1, 5)
        typical[:, k], typical[:, k + 1] = np.minimum(a, b), np.maximum(a, b)
    # the end moves down and drags the start (:341 with setEnd): a NaN start keeps :339 quiet, the new end lies below the existing start
    drag = np.array([[0.5, 2, 5, 1, 2, 0, 1], [np.nan, np.nan, 1, 3, 4, np.nan, -2]], F32)
    return {"ranges": ranges, "distributions": distributions, "smoothing": smoothing, "spaces": [typical, drag]}


def main():
    import refdiff
    assert refdiff.legacy_available(), "needs /root/reference"
    cases = feature_stats_inputs()
    out = {"source": "ConcatenatedFeatureBuffer::getFeatureRange / getDiscreteFeatureDistribution, SmoothedFeatures and FeatureSpace "
                     "(ref AudioFeatures.h) compiled unmodified against tools/refdiff/juce_standin.h; tools/refdiff/refdiff_stats.cpp"}
    for k, row in enumerate(cases["ranges"]):
        out["range_%d" % k] = refdiff.stats_feature_range(row)
    for k, (row, nb) in enumerate(cases["distributions"]):
        out["dist_%d" % k] = refdiff.stats_distribution(row, nb)
    for k, (depth, values) in enumerate(cases["smoothing"]):
        out["smooth_%d_current" % k], out["smooth_%d_history" % k] = refdiff.stats_smoothing(depth, values)
    for k, spaces in enumerate(cases["spaces"]):
        out["space_%d" % k] = refdiff.stats_feature_space(spaces)
    path = os.path.join(ROOT, "tests", "golden", "offline", "feature_stats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
