"""The 1024-point batch frame kernel's flux state by runs (csrc/fx_flux_runs.h, FluxRuns in csrc/fx_frame_kernel.hip.h), without a GPU: the
run split over every unit length and wavefront count, the compile-time check that the wavefront's flux image overlaps no live image and
stays inside the wavefront's buffer, the costing switch that bounds the change (-DFX_EXP_FLUX_NO_WAIT=1, read as a constant expression
like FX_EXP_LDS_EXCHANGE: tests/test_build_variants_cpu.py keeps the list of preprocessor conditionals closed), and the headline
kernel's registers as built."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _syntax_only(flags, csrc=CSRC):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fsyntax-only", "-Wno-unused-command-line-argument", "-DFX_PART=1"] + flags + [
        "-x", "hip", os.path.join(csrc, "fx_kernels.hip")]
    return subprocess.run(cmd, capture_output=True, text=True, cwd="/tmp")


def test_run_split_covers_every_unit_in_order_with_lengths_one_apart(tmp_path):
    """every (n, k) with n <= 600 frames and k <= 8 wavefronts: the runs cover the unit exactly, in frame order, lengths differ by at most 1"""
    exe = str(tmp_path / "flux_runs_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "flux_runs_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "4800 splits, 0 wrong"


def test_a_wrong_split_is_caught(tmp_path):
    """the host check is not vacuous: a split that gives the LAST wavefronts the longer runs breaks the static asserts on the examples"""
    src = open(os.path.join(ROOT, "tests", "cpp", "flux_runs_host.cpp")).read()
    header = open(os.path.join(CSRC, "fx_flux_runs.h")).read()
    old = "return slot * (n / k) + (slot < n % k ? slot : n % k);"
    assert header.count(old) == 1
    (tmp_path / "fx_flux_runs.h").write_text(header.replace(old, "return slot * (n / k) + (slot > k - n % k ? slot - (k - n % k) : 0);"))
    bad = tmp_path / "bad.cpp"
    bad.write_text(src.replace("../../feature-extractor_amd/csrc/", str(tmp_path) + "/"))
    p = subprocess.run(["g++", "-std=c++17", "-O1", str(bad), "-o", str(tmp_path / "bad")], capture_output=True, text=True)
    assert p.returncode != 0 and "13 frames on 8 wavefronts" in p.stderr, p.stderr[-1500:]


@needs_hipcc
@pytest.mark.parametrize("what,offset", [("inside the first exchange's rows", 5616), ("past the end of the wavefront's buffer", 5664), ("not a multiple of 16 bytes", 5640)])
def test_a_wrong_image_offset_does_not_compile(tmp_path, what, offset):
    """the image's place is a constant checked against the layouts (Geo, RealExchange) by a static_assert: a wrong one is caught by the
    compiler, before any GPU run"""
    csrc = tmp_path / "pkg" / "csrc"                               # (fx_kernels.h reaches the public header as ../../include/fx.h)
    shutil.copytree(CSRC, csrc)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    header = csrc / "fx_flux_runs.h"
    text = header.read_text()
    old = "constexpr FluxImagePlace FLUX_IMAGE_1024 = {5632};"
    assert text.count(old) == 1
    header.write_text(text.replace(old, "constexpr FluxImagePlace FLUX_IMAGE_1024 = {%d};" % offset))
    p = _syntax_only([], csrc=str(csrc))
    assert p.returncode != 0 and "flux runs: the wavefront's flux image overlaps a live image or leaves the wavefront's buffer" in p.stderr, (what, p.stderr[-1500:])


@needs_hipcc
def test_the_shipped_offset_compiles_and_the_costing_switch_is_read():
    assert _syntax_only([]).returncode == 0
    p = _syntax_only(["-DFX_EXP_FLUX_NO_WAIT=1"])
    assert p.returncode == 0 and "error:" not in p.stderr, p.stderr[-2000:]
    p = _syntax_only(["-DFX_EXP_FLUX_NO_WAIT=2"])
    assert p.returncode != 0 and "FX_EXP_FLUX_NO_WAIT: 0 or 1" in p.stderr


@needs_hipcc
def test_a_build_that_keeps_a_complex_image_keeps_the_turns(tmp_path):
    """with -DFX_EXP_LDS_EXCHANGE the second exchange writes the whole complex image (8720 B), which reaches over the flux image's place:
    such a costing build compiles because it keeps the channel image and the turn counter (FluxRuns::AVAILABLE), and the same build with
    that condition taken out is refused by the place's static assert -- the complex image is among the live images then"""
    p = _syntax_only(["-DFX_EXP_LDS_EXCHANGE=15"])
    assert p.returncode == 0 and "error:" not in p.stderr, p.stderr[-2000:]
    csrc = tmp_path / "pkg" / "csrc"
    shutil.copytree(CSRC, csrc)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    header = csrc / "fx_frame_kernel.hip.h"
    text = header.read_text()
    old = "AVAILABLE = N == 1024 && LDS_EXCHANGE_KINDS == 0u && FLUX_NO_WAIT == 0u;"
    assert text.count(old) == 1
    header.write_text(text.replace(old, "AVAILABLE = N == 1024 && FLUX_NO_WAIT == 0u;"))
    assert _syntax_only([], csrc=str(csrc)).returncode == 0                      # (the shipped exchange: still placed)
    p = _syntax_only(["-DFX_EXP_LDS_EXCHANGE=8"], csrc=str(csrc))
    assert p.returncode != 0 and "flux runs: the wavefront's flux image overlaps a live image or leaves the wavefront's buffer" in p.stderr, p.stderr[-1500:]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="ROCm's llvm tools not installed")
def test_headline_kernel_resources_hold(fx):
    """four wavefronts per SIMD: at most 128 VGPRs and not a byte of scratch, as before the change"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    fx.load_library(build_if_missing=True)
    k = [k for k in kr.kernels_of() if k["pretty"] == "fxk::fx_frame_kernel<1024, true, true, false, false>"]
    assert len(k) == 1
    assert k[0]["vgpr"] <= 128 and k[0].get("scratch", 0) == 0, k[0]
