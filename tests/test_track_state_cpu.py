"""Moving tracks between contexts without a GPU: the three entries are declared, exported and bound and the ABI number stays; the
Python and C++ names exist; null contexts and bad lists are refused before any device use with the entry named; the host code
(csrc/fx_track_state.hip compiled as C++ with its kernels left out, the shim's host units of build.HOST_SOURCES) built against
tests/cpp/fake_hip/ under ASan + UBSan (tests/cpp/track_state_host.cpp, a program of its own) validates before the first device call,
carries a track between contexts at different frame indices with the ring rotated and both indices translated, and keeps the unlisted
tracks' rows and the host mirror through every HIP call failed once; the unit is part of the gfx950 build and no host unit names it."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "feature-extractor_amd")
CSRC = os.path.join(PKG, "csrc")
FAKE = os.path.join(ROOT, "tests", "cpp", "fake_hip")
ENTRIES = ("fx_track_state_bytes", "fx_export_channels", "fx_import_channels")


def test_entries_are_declared_exported_and_bound(fx):
    header = open(os.path.join(ROOT, "include", "fx.h")).read()
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in header and name in fx.capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.fx_abi_version() == 6 and "#define FX_ABI_VERSION 6" in header      # additive: the ABI number does not move
    for method in ("track_state_bytes", "export_tracks", "import_tracks"):
        assert callable(getattr(fx.BatchAnalyser, method)), method
    hpp = open(os.path.join(ROOT, "include", "fx_realtime.hpp")).read()
    batch, live = hpp[hpp.index("class RealTimeBatchAnalyser"):hpp.index("class AudioDataCollector")], hpp[hpp.index("class LiveAnalyser"):]
    for text in (batch, live):
        assert "std::vector<unsigned char> exportTracks (const int* tracks, int count)" in text
        assert "void importTracks (const int* tracks, int count, const std::vector<unsigned char>& records)" in text
    assert "waitOnWorker ([&list, &records]" in live and "commands.push_back ([reply, &f]" in live       # on the worker, and the caller waits


def test_bad_arguments_are_refused_before_device_use(fx):
    lib = fx.load_library()
    inv = fx.capi.FX_ERR_INVALID_ARGUMENT
    lst = (ctypes.c_int * 3)(0, 1, 2)
    buf = (ctypes.c_ubyte * 64)()
    assert lib.fx_track_state_bytes(None) == 0
    for fn in (lib.fx_export_channels, lib.fx_import_channels):
        for kind in (fx.capi.MEM_HOST, fx.capi.MEM_DEVICE):
            assert fn(None, lst, 3, buf, 64, kind) == inv and b"null context" in lib.fx_last_error()
            assert fn(None, None, 0, None, 0, kind) == inv                  # a null context is refused even with nothing to do


def test_python_wrappers_check_the_list_first(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)             # no context: the checks come before any use of it
    an.num_channels = 4
    for call in (an.export_tracks, lambda channels: an.import_tracks(channels, np.zeros(16, np.uint8))):
        with pytest.raises(ValueError, match=r"entry 1: track 4 out of range \[0,4\)"):
            call([0, 4])
        with pytest.raises(ValueError, match="entry 0: track -1"):
            call(np.array([-1, 2]))
        with pytest.raises(ValueError, match="integers"):
            call([0.5])
    an._h = None


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_host_code_sanitized_with_every_hip_call_failed_once(tmp_path):
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    exe = str(tmp_path / "track_state_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", FAKE, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           *[os.path.join(CSRC, s) for s in build.HOST_SOURCES], os.path.join(FAKE, "fake_hip.cpp"),
           "-x", "c++", os.path.join(CSRC, "fx_tracks.hip"), os.path.join(CSRC, "fx_track_state.hip"), "-x", "none",
           os.path.join(ROOT, "tests", "cpp", "track_state_host.cpp"), "-o", exe, "-ldl", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "ok: 0 problems" in p.stdout and "each failed once" in p.stdout, p.stdout[-2000:]


def test_the_unit_is_built_for_gfx950_and_no_host_source_names_a_symbol_of_it(fx):
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_track_state.hip" in build.SOURCES and any(u[0] == "fx_track_state.hip" for u in build.UNITS)
    assert "fx_track_state.hip" not in build.HOST_SOURCES
    fx.load_library()
    blob = open(fx.library_path(), "rb").read()
    assert b"fx_pack_tracks_kernel" in blob and b"fx_unpack_tracks_kernel" in blob and b"gfx950" in blob
    for source in build.HOST_SOURCES:
        text = open(os.path.join(CSRC, source)).read()
        for name in ENTRIES + ("launch_pack_tracks_kernel", "launch_unpack_tracks_kernel", "TrackStateParams", "TrackHeader", "TrackEntry"):
            assert name not in text, (source, name)
