"""The 1024-point batch frame kernel's record of lane-derived constants (csrc/fx_lane_consts.hip.h), without a GPU: every costing build
(tools/build_variants.py small name=-DFX_EXP_LANE_CONSTS=mask) compiles for gfx950, the switch is really read, and the compile-time check
that holds every member -- plus the constant its section adds -- to the index the section would form from the lane number is not vacuous.

tests/test_build_variants_cpu.py keeps the list of preprocessor conditionals in csrc/ short and closed; like FX_EXP_LDS_EXCHANGE the switch
is therefore read as a constant expression and its builds are held to compile here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _syntax_only(flags, csrc=CSRC):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fsyntax-only", "-Wno-unused-command-line-argument", "-DFX_PART=1"] + flags + [
        "-x", "hip", os.path.join(csrc, "fx_kernels.hip")]
    return subprocess.run(cmd, capture_output=True, text=True, cwd="/tmp")


@pytest.mark.parametrize("mask", [0, 1, 2, 4, 8, 15])
def test_costing_switch_compiles(mask):
    """no record at all, each group on its own, and all of them"""
    p = _syntax_only(["-DFX_EXP_LANE_CONSTS=%d" % mask])
    assert p.returncode == 0 and "error:" not in p.stderr, p.stderr[-2000:]


def test_costing_switch_is_read():
    """a mask beyond the four groups is refused, so the value given on the command line is the one the kernel sees"""
    p = _syntax_only(["-DFX_EXP_LANE_CONSTS=16"])
    assert p.returncode != 0 and "a mask of the four groups of members" in p.stderr


@pytest.mark.parametrize("what,old,new", [
    ("the second pass's source slot", "RX::row((lane / 16) * 16) + (int) ((RX::SLOT_OF >> (4 * (lane % 16))) & 15ull)",
     "RX::row((lane / 16) * 16) + (int) ((RX::SLOT_OF >> (4 * (lane % 8))) & 15ull)"),
    ("the conjugation mask", "((RX::TWIN >> (lane % 16)) & 1u) << 31", "((RX::TWIN >> (lane % 16 + 1)) & 1u) << 31"),
    ("the first-pass read address", "return rimg<N>(rev(lane));", "return rimg<N>(lane);"),
    ("the warm-up distance", "return 16 + 4 * (16 / G::RQ);", "return 16;"),
    ("the left neighbours' distance", "return n + (G::BQ ? 4 : 0);", "return n;"),
])
def test_a_wrong_constant_does_not_compile(tmp_path, what, old, new):
    """the members are constexpr functions of the lane number, evaluated for all 64 lanes by a static_assert: a wrong one is caught by the
    compiler, before any GPU run"""
    csrc = tmp_path / "pkg" / "csrc"                               # (fx_kernels.h reaches the public header as ../../include/fx.h)
    shutil.copytree(CSRC, csrc)
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    header = csrc / "fx_lane_consts.hip.h"
    text = header.read_text()
    assert text.count(old) == 1, what
    header.write_text(text.replace(old, new))
    p = _syntax_only([], csrc=str(csrc))
    assert p.returncode != 0 and "LaneConsts: a member plus its section's constant" in p.stderr, (what, p.stderr[-1500:])


def test_the_record_is_formed_in_front_of_the_frame_loop_from_the_lane_alone():
    body = open(os.path.join(CSRC, "fx_frame_kernel.hip.h")).read()
    form = body.index("lcs.form(lane0, cbuf, tw)")
    assert form < body.index("for (int t = live ?")
    # nothing that changes under a wavefront in calls cut into time units goes in: not the channel, the chunk, the ticket or a frame
    record = open(os.path.join(CSRC, "fx_lane_consts.hip.h")).read()
    sig = record[record.index("void form("):]
    sig = sig[:sig.index(")") + 1]
    assert sig == "void form(int lane, f2* cbuf, const f2* tw)", sig
    assert '"fx_lane_consts.hip.h"' in open(os.path.join(ROOT, "feature-extractor_amd", "build.py")).read()
