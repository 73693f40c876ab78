"""Per-track settings without a GPU: the entries are declared, exported and bound; their host code (csrc/fx_capi.cpp, built with the rest of build.HOST_SOURCES) validates
arguments before any device use -- a null context, a bad entry names its track and changes nothing -- and, built against
tests/cpp/fake_hip/ under ASan + UBSan with every HIP call failed once (tests/cpp/channel_settings_host.cpp), a failed table upload
leaves the old settings in force and reports FX_ERR_HIP; sharded.py cuts a global per-track array by the shard's channel range."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
FAKE = os.path.join(ROOT, "tests", "cpp", "fake_hip")
ENTRIES = ("fx_set_channel_gains", "fx_set_channel_onset", "fx_get_channel_settings")


def test_entries_are_declared_exported_and_bound(fx):
    header = open(os.path.join(ROOT, "include", "fx.h")).read()
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in header and name in fx.capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.fx_abi_version() == 6                        # additive: the ABI number does not move
    for method in ("set_channel_gains", "set_channel_onset", "channel_settings"):
        assert callable(getattr(fx.BatchAnalyser, method))
    hpp = open(os.path.join(ROOT, "include", "fx_realtime.hpp")).read()
    for overload in ("setGain (int track, float", "setOnsetDetectionSensitivity (int track, float", "setOnsetWindowLength (int track, int",
                     "setOnsetDetectionType (int track, eOnsetDetectionType"):
        assert overload in hpp, overload


def test_null_context_is_refused_before_device_use(fx):
    lib = fx.load_library()
    g = (ctypes.c_float * 4)(1, 2, 3, 4)
    w = (ctypes.c_int * 4)(1, 2, 3, 4)
    assert lib.fx_set_channel_gains(None, g) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert b"null context" in lib.fx_last_error()
    assert lib.fx_set_channel_onset(None, g, w, w) == fx.capi.FX_ERR_INVALID_ARGUMENT
    assert lib.fx_get_channel_settings(None, g, g, w, w) == fx.capi.FX_ERR_INVALID_ARGUMENT


def test_python_wrappers_check_the_array_length(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)         # no context: the length check comes first
    an.num_channels = 4
    with pytest.raises(ValueError, match="one entry per track"):
        an.set_channel_gains([1.0, 2.0])
    with pytest.raises(ValueError, match="one entry per track"):
        an.set_channel_onset(window=[5] * 5)
    an._h = None


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_host_code_sanitized_with_every_hip_call_failed_once(tmp_path):
    from importlib import import_module
    build = import_module("feature-extractor_amd.build")
    exe = str(tmp_path / "channel_settings_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", FAKE, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           *[os.path.join(CSRC, s) for s in build.HOST_SOURCES], os.path.join(FAKE, "fake_hip.cpp"),
           os.path.join(ROOT, "tests", "cpp", "channel_settings_host.cpp"), "-o", exe, "-ldl", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "ok: 0 problems" in p.stdout and "each failed once" in p.stdout, p.stdout[-2000:]


def test_sharded_cuts_a_global_array_by_the_shard_range(fx):
    from importlib import import_module
    sharded = import_module("feature-extractor_amd.sharded")
    total = 37
    gains = np.arange(total, dtype=np.float32)
    for world in (1, 2, 4, 8):
        parts = [sharded.shard_slice(gains, total, r, world) for r in range(world)]
        assert np.array_equal(np.concatenate(parts), gains)
        for r, part in enumerate(parts):
            first, count = sharded.my_shard(total, r, world)
            assert np.array_equal(part, gains[first:first + count])
    assert sharded.shard_slice(None, total, 0, 2) is None
    with pytest.raises(ValueError):
        sharded.shard_slice(gains[:-1], total, 0, 2)

    class Recorder:
        def __init__(self):
            self.calls = []

        def set_channel_gains(self, g):
            self.calls.append(("gains", g))

        def set_channel_onset(self, s, w, t):
            self.calls.append(("onset", s, w, t))

    rec = Recorder()
    windows = np.arange(total, dtype=np.int32) % 32 + 1
    sharded.set_shard_channel_settings(rec, total, 1, 4, gains=gains, window=windows)
    first, count = sharded.my_shard(total, 1, 4)
    assert rec.calls[0][0] == "gains" and np.array_equal(rec.calls[0][1], gains[first:first + count])
    assert rec.calls[1][0] == "onset" and rec.calls[1][1] is None and np.array_equal(rec.calls[1][2], windows[first:first + count]) and rec.calls[1][3] is None
