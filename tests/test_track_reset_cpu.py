"""Per-track reset and clear without a GPU: the three entries are declared, exported and bound and the ABI number stays; the Python
and C++ names exist; lists are refused before any device use with the entry named; the host code (csrc/fx_tracks.hip compiled as C++
with its kernel left out, the shim's host units of build.HOST_SOURCES) built against tests/cpp/fake_hip/ under ASan + UBSan with every HIP call failed once
(tests/cpp/track_reset_host.cpp) keeps the unlisted tracks' rows through every failure; the unit is part of the gfx950 build and
the source tree holds none of the scalar-store instructions the kernels must not use."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "feature-extractor_amd")
CSRC = os.path.join(PKG, "csrc")
FAKE = os.path.join(ROOT, "tests", "cpp", "fake_hip")
ENTRIES = ("fx_reset_channels", "fx_clear_pending_channels", "fx_get_channel_frames")


def test_entries_are_declared_exported_and_bound(fx):
    header = open(os.path.join(ROOT, "include", "fx.h")).read()
    lib = fx.load_library()
    for name in ENTRIES:
        assert name + "(" in header and name in fx.capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.fx_abi_version() == 6 and "#define FX_ABI_VERSION 6" in header      # additive: the ABI number does not move
    for method in ("reset_channels", "clear_pending_channels", "channel_frames"):
        assert callable(getattr(fx.BatchAnalyser, method)), method
    hpp = open(os.path.join(ROOT, "include", "fx_realtime.hpp")).read()
    for name in ("void resetTrack (int track)", "void resetTracks (const int* tracks, int count)", "void clearBuffer (int track)"):
        assert name in hpp, name
    live = hpp[hpp.index("class LiveAnalyser"):]
    assert "void resetTracks (const int* tracks, int count)" in live and "callOnWorker ([list]" in live


def test_bad_arguments_are_refused_before_device_use(fx):
    lib = fx.load_library()
    inv = fx.capi.FX_ERR_INVALID_ARGUMENT
    lst = (ctypes.c_int * 3)(0, 1, 2)
    frames = (ctypes.c_longlong * 4)()
    for fn in (lib.fx_reset_channels, lib.fx_clear_pending_channels):
        assert fn(None, lst, 3) == inv and b"null context" in lib.fx_last_error()
        assert fn(None, None, 0) == inv                         # a null context is refused even with nothing to do
    assert lib.fx_get_channel_frames(None, frames) == inv and b"null context" in lib.fx_last_error()


def test_python_wrappers_check_the_list_first(fx):
    an = fx.BatchAnalyser.__new__(fx.BatchAnalyser)             # no context: the checks come before any use of it
    an.num_channels = 4
    for call in (an.reset_channels, an.clear_pending_channels):
        with pytest.raises(ValueError, match=r"entry 1: track 4 out of range \[0,4\)"):
            call([0, 4])
        with pytest.raises(ValueError, match="entry 0: track -1"):
            call(np.array([-1, 2]))
        with pytest.raises(ValueError, match="integers"):
            call([0.5])
    an._h = None


def test_sharded_cuts_a_global_track_list_to_local_indices(fx):
    from importlib import import_module
    sharded = import_module("feature-extractor_amd.sharded")
    total = 37
    want = [36, 0, 5, 5, 18, 9, 27]
    for world in (1, 2, 4, 8):
        back = []
        for r in range(world):
            first, count = sharded.my_shard(total, r, world)
            local = sharded.shard_channel_list(want, total, r, world)
            assert local.dtype == np.int32 and ((local >= 0) & (local < count)).all()
            assert list(local + first) == [c for c in want if first <= c < first + count]      # the list's order, duplicates kept
            back += list(local + first)
        assert sorted(back) == sorted(want)
    assert sharded.shard_channel_list([], total, 0, 2).size == 0 and sharded.shard_channel_list(None, total, 1, 2).size == 0
    with pytest.raises(ValueError):
        sharded.shard_channel_list([total], total, 0, 2)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_host_code_sanitized_with_every_hip_call_failed_once(tmp_path):
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    exe = str(tmp_path / "track_reset_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", FAKE, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           *[os.path.join(CSRC, s) for s in build.HOST_SOURCES], os.path.join(FAKE, "fake_hip.cpp"),
           "-x", "c++", os.path.join(CSRC, "fx_tracks.hip"), "-x", "none",
           os.path.join(ROOT, "tests", "cpp", "track_reset_host.cpp"), "-o", exe, "-ldl", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "ok: 0 problems" in p.stdout and "each failed once" in p.stdout, p.stdout[-2000:]


def test_the_unit_is_built_for_gfx950_and_capi_names_no_symbol_of_it(fx):
    build = fx.build if hasattr(fx, "build") and hasattr(fx.build, "UNITS") else __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_tracks.hip" in build.SOURCES and any(u[0] == "fx_tracks.hip" for u in build.UNITS)
    fx.load_library()
    blob = open(fx.library_path(), "rb").read()
    assert b"fx_reset_channels_kernel" in blob and b"gfx950" in blob
    for source in build.HOST_SOURCES:
        text = open(os.path.join(CSRC, source)).read()
        for name in ENTRIES + ("launch_reset_channels_kernel", "ResetParams"):
            assert name not in text, (source, name)


def test_no_scalar_store_instruction_in_the_source_tree():
    words = re.compile("|".join(["s_" + w for w in ("store_dword", "buffer_store", "scratch_store", "atomic_", "buffer_atomic", "dcache_wb", "dcache_discard")]), re.I)
    hits = []
    for top in (PKG, os.path.join(ROOT, "include"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "examples")):
        for base, dirs, files in os.walk(top):
            dirs[:] = [d for d in dirs if d not in ("lib", "__pycache__", "_ref")]
            for f in files:
                if f.endswith((".hip", ".h", ".hpp", ".cpp", ".c", ".py", ".s", ".S", ".cmake", ".sh")):
                    path = os.path.join(base, f)
                    if words.search(open(path, errors="replace").read()):
                        hits.append(os.path.relpath(path, ROOT))
    assert not hits, hits
