"""The planar tile through LDS is stated once (csrc/fx_planar_tile.hip.h), without a GPU: both byte movers include the header and
carry no copy of it, the header alone compiles for gfx950, and its index arithmetic -- tile_at, the chunk count and row bytes, the
bytes a chunk contributes -- places and drains every segment byte exactly once on the host under AddressSanitizer and UBSan
(tests/cpp/planar_tile_host.cpp), with the bank spread its comment claims."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADER = "fx_planar_tile.hip.h"
UNITS = ("fx_interleave.hip", "fx_rtp.hip")


def test_the_header_is_a_dependency_of_the_build():
    build = importlib.import_module("feature-extractor_amd.build")
    assert HEADER in build.HEADERS


@pytest.mark.parametrize("unit", UNITS)
def test_units_include_the_tile_and_restate_none_of_it(unit):
    text = open(os.path.join(CSRC, unit)).read()
    assert HEADER in re.findall(r'^\s*#\s*include\s*"([^"]+)"', text, flags=re.M)
    # (the load stages call store_sample<B>(..) and tile_to_rows<B>(..): neither name below followed by "(" is a call they make)
    for name in ("tile_at(", "store_sample(", "pick("):
        assert name not in text, name
    assert "TWIN" not in text


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_header_alone_compiles_for_gfx950(tmp_path):
    build = importlib.import_module("feature-extractor_amd.build")
    cmd = [HIPCC] + build.HIPCC_FLAGS + ["--cuda-device-only", "-fsyntax-only", "-x", "hip", os.path.join(CSRC, HEADER)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert p.returncode == 0 and "error:" not in p.stderr, p.stderr[-2000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_tile_arithmetic_on_the_host_sanitized(tmp_path):
    exe = str(tmp_path / "planar_tile_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "cpp", "planar_tile_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stdout[-500:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    # per width: (offsets modulo 16 its alignment allows) x (nf = 1 .. 64) x (rows 0, 7, 8, 63)
    assert lines[:3] == ["2 %d" % (8 * 64 * 4), "3 %d" % (16 * 64 * 4), "4 %d" % (4 * 64 * 4)]
    columns = 33 * (8 * 128 + 16 * 192 + 4 * 256)       # every start of 32 consecutive rows, every byte column of a full row
    assert lines[3] == "%d cases, %d columns on distinct banks" % (28 * 64 * 4, columns) and len(lines) == 4
