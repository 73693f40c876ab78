"""The pinned and device list pair of the list-taking units (csrc/fx_context.h: fx_staged_list, fx_reserve_list, fx_release_list)
without a GPU: tests/cpp/staged_list_host.cpp, built with the shim's host units of build.HOST_SOURCES against tests/cpp/fake_hip/
under ASan + UBSan, grows a list from nothing and by half again, and fails every HIP call of a growing reserve once; and the two
units that stage a list keep no copy of that code."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
FAKE = os.path.join(ROOT, "tests", "cpp", "fake_hip")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_staged_list_sanitized_with_every_hip_call_failed_once(tmp_path):
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    exe = str(tmp_path / "staged_list_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", FAKE, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           *[os.path.join(CSRC, s) for s in build.HOST_SOURCES], os.path.join(FAKE, "fake_hip.cpp"),
           os.path.join(ROOT, "tests", "cpp", "staged_list_host.cpp"), "-o", exe, "-ldl", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "ok: 0 problems" in p.stdout and "each failed once" in p.stdout, p.stdout[-2000:]


def test_the_list_taking_units_stage_their_lists_through_it():
    for unit in ("fx_tracks.hip", "fx_track_state.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "fx_reserve_list(" in text and "fx_release_list(" in text, unit
        assert "hipHostMalloc" not in text and "hipHostFree" not in text, unit
