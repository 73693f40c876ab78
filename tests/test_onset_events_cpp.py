"""The onset event list through the C++ host layer (include/fx_realtime.hpp): tests/cpp/onset_events_mirror.cpp compiled with g++
against libfx_hip.so.  On the GPU: a fx::LiveAnalyser with only an onset callback, fed 481-sample blocks against a 1024-point
window, must call back the (track, frame) sequence of a synchronous fx_push_samples run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(fx, tmp_path):
    fx.load_library()
    exe = str(tmp_path / "onset_events_mirror")
    lib_dir = os.path.dirname(fx.library_path())
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "onset_events_mirror.cpp"), "-o", exe,
                           "-L", lib_dir, "-lfx_hip", "-Wl,-rpath," + lib_dir, "-pthread"])
    return exe


def test_onset_events_mirror_cpu(fx, tmp_path):
    exe = _build(fx, tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "onset_events_mirror: ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_live_analyser_with_only_an_onset_callback(gpu_fx, tmp_path):
    exe = _build(gpu_fx, tmp_path)
    out = subprocess.run([exe, "--gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "onset_events_mirror --gpu: ok" in out.stdout, out.stdout + out.stderr
