"""fx::FeatureSpace (include/fx_realtime.hpp) and the binding's FeatureSpace (feature-extractor_amd/offline.py) against what the reference's
own header folds (tests/golden/offline/feature_stats.npz, made through tools/refdiff/refdiff_stats.cpp from the unmodified AudioFeatures.h
:319-349), bit for bit: tests/cpp/feature_space_mirror.cpp is compiled with g++ against the header and run on the fixture's inputs.  No GPU."""
import os
import subprocess
import sys

import numpy as np

from offline_stats_model import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_feature_stats_cases import feature_stats_inputs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "offline", "feature_stats.npz")


def test_cpp_feature_space_folds_equal_the_reference_headers(fx, tmp_path):
    fx.load_library()
    exe = str(tmp_path / "feature_space_mirror")
    lib_dir = os.path.dirname(fx.library_path())
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "feature_space_mirror.cpp"), "-o", exe, "-L", lib_dir, "-lfx_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    g = np.load(GOLDEN)
    for k, spaces in enumerate(feature_stats_inputs()["spaces"]):
        fin, fout = str(tmp_path / ("in_%d.bin" % k)), str(tmp_path / ("out_%d.bin" % k))
        with open(fin, "wb") as f:
            f.write(np.int32(spaces.shape[0]).tobytes())
            f.write(np.ascontiguousarray(spaces, np.float32).tobytes())
        out = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert out.returncode == 0 and "feature_space_mirror: ok" in out.stdout, out.stdout + out.stderr
        got = np.fromfile(fout, np.float32).reshape(-1, 8)
        assert same(got[:-1], g["space_%d" % k]), k
        assert same(got[-1], g["space_%d" % k][-1]), k                  # the same folds through FeatureSpace::fromRanges


def test_python_feature_space_folds_equal_the_reference_headers(fx):
    off = fx.offline
    g = np.load(GOLDEN)
    for k, spaces in enumerate(feature_stats_inputs()["spaces"]):
        make = lambda p: off.FeatureSpace(p[0], off.Range(p[1], p[2]), off.Range(p[3], p[4]), off.Range(p[5], p[6]))
        flat = lambda s: np.array([v for r in (s.attack_range, s.spectral_centroid_range, s.spectral_slope_range, s.zero_crosses_range) for v in r], np.float32)
        existing = make(spaces[0])
        rows = [flat(existing)]
        for p in spaces[1:]:
            new = make(p)
            for mine, theirs in ((existing.attack_range, new.attack_range), (existing.spectral_centroid_range, new.spectral_centroid_range),
                                 (existing.spectral_slope_range, new.spectral_slope_range), (existing.zero_crosses_range, new.zero_crosses_range)):
                off.FeatureSpace.compare_and_update_ranges(mine, theirs)
            rows.append(flat(existing))
        assert same(np.array(rows, np.float32), g["space_%d" % k]), k
    assert same(flat(off.FeatureSpace()), np.zeros(8, np.float32))      # ref :321-325: four empty ranges


def test_feature_space_from_buffer_takes_the_channels_own_ranges(fx):
    """from_buffer: Range (attack, 0.0f) of estimated_log_attack_time[c] and the centroid, slope and zero-crossing ranges of channel c"""
    off, capi = fx.offline, fx.capi
    C, D = 3, 5
    ranges = np.arange(10 * C * 2, dtype=np.float32).reshape(10, C, 2)
    buf = off.ConcatenatedFeatureBuffer(np.zeros((10, C, D), np.float32), np.zeros((C, D), np.float32), np.array([-1.5, 0.25, np.nan], np.float32), None, D, 48000)
    s = off.FeatureSpace.from_buffer(buf, 1, ranges=ranges)
    assert tuple(s.attack_range) == (0.25, 0.25) and tuple(s.spectral_centroid_range) == tuple(ranges[capi.OFFLINE_CENTROID, 1])
    assert tuple(s.spectral_slope_range) == tuple(ranges[capi.OFFLINE_SLOPE, 1]) and tuple(s.zero_crosses_range) == tuple(ranges[capi.OFFLINE_ZERO_CROSSES, 1])
    assert tuple(off.FeatureSpace.from_buffer(buf, 0, ranges=ranges).attack_range) == (-1.5, 0.0)
    nan = off.FeatureSpace.from_buffer(buf, 2, ranges=ranges).attack_range
    assert np.isnan(nan.start) and nan.end == 0.0                        # jmax (NaN, 0) by `<`: the end stays 0
