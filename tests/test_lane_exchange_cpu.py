"""The 1024-point transform's second exchange as lane swaps (csrc/fx_lane_exchange.h, second_exchange_regs in csrc/fx_fft.hip.h), without
a GPU: the swap schedule the kernel issues, simulated on labelled registers by a host program that includes the kernel's own header, and
the costing switch that keeps chosen transform kinds on the LDS exchange (tools/build_variants.py small name=-DFX_EXP_LDS_EXCHANGE=mask).

tests/test_build_variants_cpu.py keeps the list of preprocessor conditionals in csrc/ short and closed; the costing switch is therefore
read as a constant expression (lds_exchange_kinds) and its builds are held to compile here instead."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_swaps_deliver_every_last_pass_operand(tmp_path):
    """64 x 16 registers that hold their own (lane, element): after permlane32_swap (lanes 32-63 of the first operand <-> lanes 0-31 of
    the second) and permlane16_swap (rows 1, 3 of the first <-> rows 0, 2 of the second) in the kernel's order, operand ip of butterfly
    lane + 64*g is (16*ip + lane%16, lane/16 + 4*g) -- the position cpad(lane + 64*g) + item_off(256, ip) of the LDS path"""
    exe = str(tmp_path / "lane_exchange_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "lane_exchange_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "16 swaps of register pairs (32 instructions), 0 operands wrong"


def test_a_wrong_schedule_is_caught(tmp_path):
    """the simulation is not vacuous: with the two stages' instructions exchanged the operands are wrong"""
    src = open(os.path.join(ROOT, "tests", "cpp", "lane_exchange_host.cpp")).read()
    assert "(stage == 0 ? permlane32_swap : permlane16_swap)" in src
    bad = tmp_path / "bad.cpp"
    bad.write_text(src.replace("(stage == 0 ? permlane32_swap : permlane16_swap)", "(stage == 1 ? permlane32_swap : permlane16_swap)")
                      .replace("../../feature-extractor_amd/csrc/", CSRC + "/"))
    exe = str(tmp_path / "bad")
    subprocess.check_call(["g++", "-std=c++17", "-O1", str(bad), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 1 and "operands wrong" in out.stdout and " 0 operands wrong" not in out.stdout


def test_the_kernels_use_the_shared_mapping():
    fft = open(os.path.join(CSRC, "fx_fft.hip.h")).read()
    assert '#include "fx_lane_exchange.h"' in fft
    assert "__builtin_amdgcn_permlane32_swap" in fft and "__builtin_amdgcn_permlane16_swap" in fft
    assert "LX::swap(0, j)" in fft and "LX::swap(1, j)" in fft and "register_of(g, i)" in fft
    for line in fft.splitlines():                                # builtins, so that the compiler places the swaps' wait states
        assert not ("asm" in line and "permlane" in line), line


def _syntax_only(flags):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fsyntax-only", "-Wno-unused-command-line-argument", "-DFX_PART=1"] + flags + [
        "-x", "hip", os.path.join(CSRC, "fx_kernels.hip")]
    return subprocess.run(cmd, capture_output=True, text=True, cwd="/tmp")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("mask", [8, 15])
def test_costing_switch_compiles(mask):
    """the inverse transform alone on LDS (the LazyLag question), and the kernel without lane swaps"""
    p = _syntax_only(["-DFX_EXP_LDS_EXCHANGE=%d" % mask])
    assert p.returncode == 0 and "error:" not in p.stderr, p.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_costing_switch_is_read():
    """a mask beyond the four kinds is refused, so the value given on the command line is the one the trait sees"""
    p = _syntax_only(["-DFX_EXP_LDS_EXCHANGE=16"])
    assert p.returncode != 0 and "a mask of the four transform kinds" in p.stderr
