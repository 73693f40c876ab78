"""The wire formats live in one header (csrc/fx_samples.hip.h) that stands without the FFT and the frame kernel, and the attached units
that read samples include it instead of the kernels' stack.  No GPU: one device-only compilation for gfx950 with the library's own
options, and a look at the units' #include lines."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNITS = ("fx_taps.hip", "fx_display.hip", "fx_clips.hip", "fx_monitor.hip")

# widen_one, widen_four and fetch_four at the four formats in one kernel, through the header's own dispatch; nothing else of the library
PROBE = """
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "fx_kernels.h"
#pragma clang fp contract(off)
namespace fxk {
#include "fx_wave.hip.h"
#include "fx_samples.hip.h"
template <int FMT> __device__ float probe_format(const void* src, int i)
{
    const f4 v = widen_four<FMT>(fetch_four<FMT>(src, 4 * i));
    return v[0] + v[1] + v[2] + v[3] + widen_one<FMT>(static_cast<const unsigned char*>(src) + i * sample_bytes(FMT));
}
__global__ void probe_kernel(const void* src, int fmt, float* out)
{
    FX_FORMAT(fmt, out[threadIdx.x] = probe_format<FMT>(src, (int) threadIdx.x));
}
static_assert(sample_bytes(FX_SAMPLE_F32) == 4 && sample_bytes(FX_SAMPLE_F16) == 2 && sample_bytes(FX_SAMPLE_S16) == 2 && sample_bytes(FX_SAMPLE_S24) == 3, "");
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_header_compiles_without_the_fft_and_the_frame_kernel(tmp_path):
    build = importlib.import_module("feature-extractor_amd.build")
    src = tmp_path / "probe.hip"
    src.write_text(PROBE)
    cmd = [HIPCC] + build.HIPCC_FLAGS + ["--cuda-device-only", "-I", CSRC, "-x", "hip", "-c", str(src), "-o", str(tmp_path / "probe.o")]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode == 0 and "error:" not in p.stderr, p.stderr[-2000:]
    assert os.path.getsize(tmp_path / "probe.o") > 0
    # the probe is the whole dependency: the header itself pulls nothing in
    assert "#include" not in open(os.path.join(CSRC, "fx_samples.hip.h")).read()


@pytest.mark.parametrize("unit", UNITS)
def test_attached_units_include_the_formats_not_the_kernels(unit):
    text = open(os.path.join(CSRC, unit)).read()
    included = re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, flags=re.M)
    assert "fx_samples.hip.h" in included, included
    assert "fx_fft.hip.h" not in included and "fx_frame_kernel.hip.h" not in included, included
