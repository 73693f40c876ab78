"""OSC bundles on the host under sanitizers: tests/cpp/osc_bundles_host.cpp, a stand-alone program built from the shim's host units and
tests/cpp/fake_hip -- once under ASan + UBSan and once under TSan.  It runs osc_bundle_word (csrc/fx_osc_words.h, the function the
device kernel runs per output word) through the host encoders against bundles put together from fx_osc_encode messages (ref
OSCFeatureAnalysisOutput.h:107), fx::OSCBatchSender::setBundling publishing while the 60 Hz timer sends, and the receiver's bundle
parser on hostile datagrams.  No GPU, no Python in the process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
FAKE = os.path.join(ROOT, "tests", "cpp", "fake_hip")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_bundles_on_the_host_sanitized(tmp_path, sanitizer):
    build = __import__("importlib").import_module("feature-extractor_amd.build")
    assert "fx_osc_bundle.hip" not in build.HOST_SOURCES
    exe = str(tmp_path / "osc_bundles_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-fsanitize=" + sanitizer, "-fno-omit-frame-pointer",
           "-I", FAKE, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           *[os.path.join(CSRC, s) for s in build.HOST_SOURCES], os.path.join(FAKE, "fake_hip.cpp"),
           os.path.join(ROOT, "tests", "cpp", "osc_bundles_host.cpp"), "-o", exe, "-ldl", "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "ok: 0 problems" in p.stdout, p.stdout[-2000:]
    assert "WARNING: ThreadSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
