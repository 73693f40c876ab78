"""The dispatch table (tests/dispatch_paths.py) against the sources, without a GPU: every launch form the kernel sources build is a form the
table knows, and the rows' expected launches reach each of them at every window size where it exists -- so a launch form added without a
row fails here.  The rows' work-unit counts are fx_plan_units' own answers, and the table holds to the rules it is built from."""
import os
import re

import pytest

import dispatch_paths as dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "feature-extractor_amd", "csrc")
SOURCES = ("fx_kernels.hip", "fx_hop_kernel.hip.h", "fx_reblock.hip")


def launch_forms():
    """{kernel form as written at a hipLaunchKernelGGL, whitespace removed}"""
    forms = set()
    for name in SOURCES:
        text = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r"hipLaunchKernelGGL\s*\(\s*(\(\s*)?([A-Za-z_]\w*\s*(<[^>]*>)?)", text):
            forms.add(re.sub(r"\s+", "", m.group(2)))
    return forms


def test_every_launch_form_in_the_sources_is_in_the_table():
    found = launch_forms()
    assert len(found) >= 20, found
    assert found == set(dp.FORMS), "forms without a table entry: %s; table entries the sources no longer launch: %s" % (
        sorted(found - set(dp.FORMS)), sorted(set(dp.FORMS) - found))


def test_the_rows_cover_every_form_at_every_window_size():
    got = dp.covered()
    want = {(f, n) for f, ns in list(dp.FORMS.items()) + list(dp.SUBFORMS.items()) for n in ns}
    assert not want - got, "launch forms no row reaches: %s" % sorted(want - got)
    assert not {g for g in got if g[0] not in dp.FORMS and g[0] not in dp.SUBFORMS}, got


def test_rows_are_well_formed():
    ids = [r.id for r in dp.ROWS]
    assert len(ids) == len(set(ids)), [i for i in ids if ids.count(i) > 1]
    for r in dp.ROWS:
        assert r.entry in ("hops", "frames", "samples", "ring"), r.id
        assert r.rule, r.id
        assert r.calls >= 3, r.id
        H = r.N // 2
        if r.entry == "samples":
            total = r.per[0] + r.per[1] * (r.calls - 1)
            assert total // H > 48, (r.id, total // H)
            assert r.fmt in ("f32", "s16"), r.id
        else:
            assert r.per * r.calls > 48, r.id
            assert set(r.expect) == {r.per}, r.id
        for t, seq in r.expect.items():
            assert seq and all(set(l) == set(dp.FIELDS) and l["window"] == r.N for l in seq), r.id
            # the stride contract: only a one-frame tail writes frame out_t0 of out_stride
            assert not any(l["out_stride"] and l["ep_T"] != 1 for l in seq), r.id
            # a call analyses its frames exactly once
            frames = sum(l["T"] for l in seq if l["kind"] in ("frame", "frame_tail", "hop", "hop_pair", "pair"))
            assert frames == t, (r.id, t, seq)


def test_block_rows_cover_fp32_and_a_pcm_format():
    """(every kind of block row is run with 32-bit floats and with 16-bit PCM)"""
    kinds = {}
    for r in dp.ROWS:
        if r.entry == "samples":
            kinds.setdefault(tuple(sorted({l["kind"] for seq in r.expect.values() for l in seq})), set()).add(r.fmt)
    for k, fmts in kinds.items():
        assert fmts == {"f32", "s16"}, (k, fmts)


def test_work_unit_counts_are_the_planners(fx):
    """num_chunks of each expected frame / pair launch is what fx_plan_units (host arithmetic) makes of the row's tuning"""
    capi = fx.capi
    try:
        capi.load_library()
    except Exception as e:          # (a checkout that has not been built)
        pytest.skip("libfx_hip.so not loadable: %s" % e)
    import ctypes
    flags = {"both": 0, "spectral": capi.SPECTRAL_ONLY, "harmonic": capi.HARMONIC_ONLY}
    for r in dp.ROWS:
        t = capi.Tuning()
        capi.load_library().fx_tuning_defaults(ctypes.byref(t))
        for k, v in r.tuning.items():
            if k == "unit_plan":
                t.set_plan(v)
            else:
                setattr(t, k, int(v))
        for seq in r.expect.values():
            for l in seq:
                if l["kind"] not in ("frame", "pair"):
                    continue
                # a captured ring step is never cut (its arguments are frozen at capture)
                captured = r.entry == "ring" and r.tuning.get("stream_graph", -1) != 0
                want = 1 if captured else len(capi.plan_units(r.N, flags[r.analysers], l["waves_per_ch"], l["T"], t))
                assert l["num_chunks"] == want, (r.id, l, want)


def test_one_round_of_workgroups_is_crossed_where_the_rows_say():
    """the rows that take fx_frame_tail_kernel hold at most one round of workgroups on 256 CUs (two per CU; one at 4096 points with more
    than four channels per workgroup); the one-frame rows that split the tail off do it by hook 4, not by count"""
    for r in dp.ROWS:
        for seq in r.expect.values():
            for l in seq:
                if l["kind"] == "frame_tail":
                    groups = -(-r.C // l["ch_per_wg"])
                    one_round = dp.CUS * (1 if (r.N == 4096 and l["ch_per_wg"] > 4) else 2)
                    assert groups <= one_round or r.hooks & 8, r.id
                if l["kind"] == "frame" and l["direct_state"] and r.N >= 1024 and r.entry != "ring":
                    assert r.hooks & 4, r.id
