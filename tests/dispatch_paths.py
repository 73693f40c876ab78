"""The table of analysis dispatch paths: each row is an entry point, a configuration and the launch sequence the library must make
for it (fx_last_launches_internal, BatchAnalyser.last_launches()).  The rows are derived from csrc/fx_plan.cpp -- plan_call (workgroup
shape, work units, hop kernel, one launch or two, two-hop calls as one-frame launches, the ring's fixed routes), csrc/fx_capi.cpp -- fx_push_samples (block
feed or re-blocking) -- and csrc/fx_stream.cpp -- fx_stream_submit (hop kernel, captured step or the three-queue path) -- and from the launchers of csrc/fx_kernels.hip, fx_hop_kernel.hip.h
and fx_reblock.hip.  The union of the rows covers every launch form those files build, at every window size where it exists
(tests/test_dispatch_cpu.py holds it to that); tests/test_gpu_dispatch.py runs every row on the device.

The sequences depend on the device's CU count (one round of workgroups); they are written for the MI355X's 256.

A row's `expect` maps the number of frames a call analyses to the launches of that call: a block of samples may complete a different
number of hops from call to call."""
from collections import namedtuple

import numpy as np

CUS = 256
ALL_N = (256, 512, 1024, 2048, 4096)
BIG_N = (1024, 2048, 4096)                      # windows with fx_hop_kernel, fx_frame_tail_kernel and the block-fed one-frame forms
FIELDS = ("kind", "window", "analysers", "T", "direct_state", "block_mode", "num_chunks", "ch_per_wg", "waves_per_ch", "hop_pairs",
          "ep_T", "out_stride", "ep_form", "reblock")
FUSED_TAIL_MAX_FRAMES = 8                       # csrc/fx_kernels.h


def _rec(kind, N, analysers=3, **kw):
    r = dict.fromkeys(FIELDS, 0)
    r.update(kind=kind, window=N, analysers=analysers, **kw)
    return r


def frame(N, T, ch, k, direct=0, block=0, chunks=1, an=3):
    return _rec("frame", N, an, T=T, direct_state=direct, block_mode=block, num_chunks=chunks, ch_per_wg=ch, waves_per_ch=k)


def pair(N, T, ch, k, chunks=1):
    return _rec("pair", N, 3, T=T, num_chunks=chunks, ch_per_wg=ch, waves_per_ch=k)


def frame_tail(N, ch, block=0, stride=0):
    return _rec("frame_tail", N, 3, T=1, direct_state=1, block_mode=block, num_chunks=1, ch_per_wg=ch, waves_per_ch=1, ep_T=1, out_stride=stride)


def hop(N, block=0, stride=0, pairs=False):
    return _rec("hop_pair" if pairs else "hop", N, 3, T=1, direct_state=0 if pairs else 1, block_mode=block, hop_pairs=int(pairs), ep_T=1,
                out_stride=stride)


def epi(N, T, stride=0, an=3):
    return _rec("epilogue", N, an, ep_T=T, out_stride=stride, ep_form=1 if T <= FUSED_TAIL_MAX_FRAMES else 2)


def reblock(N, form):
    return _rec("reblock", N, 0, reblock=form)


# entry: hops (fx_push_hops, `per` hops per call), frames (fx_process_frames, `per` windows per call), samples (fx_push_samples, block
# lengths `per`: the first, then the second repeated), ring (HopStream, `per` hops per batch)
Row = namedtuple("Row", "id N C entry per calls expect analysers low_latency tuning hooks fmt rule")


def row(id, N, entry, per, calls, expect, C=5, analysers="both", low_latency=False, tuning=None, hooks=0, fmt="f32", rule=""):
    return Row(id, N, C, entry, per, calls, expect, analysers, low_latency, tuning or {}, hooks, fmt, rule)


def _ch1(N, C=5):
    """channels per workgroup of a one-frame call through the direct batch form (plan_call): a workgroup's worth up to 1024 points,
    four at 2048, at 4096 eight from 2048 channels on"""
    return min(C, 8 if N <= 1024 else (4 if N == 2048 else (8 if C >= 2048 else 4)))


def _k(N):
    return 4 if N == 2048 else 8                # frame_kernel_preferred_shape


NO_HOP = {"one_hop_kernel": 0}
ROWS = []
for N in ALL_N:
    ROWS += [
        # batch calls (T > FUSED_TAIL_MAX_FRAMES): fx_frame_kernel<N,1,1>, finalise + epilogue + history; T < 2 k: never cut
        row("batch-%d" % N, N, "hops", 12, 5, {12: [frame(N, 12, 1, _k(N)), epi(N, 12)]}, fmt="s16" if N == 512 else "f32",
            rule="T > 8: the three-kernel tail"),
        # one analyser only: fx_frame_kernel<N,1,0> / <N,0,1>
        row("spectral-%d" % N, N, "hops", 12, 5, {12: [frame(N, 12, 1, _k(N), an=1), epi(N, 12, an=1)]}, analysers="spectral",
            rule="FX_SPECTRAL_ONLY: <N,1,0>"),
        row("harmonic-%d" % N, N, "hops", 12, 5, {12: [frame(N, 12, 1, _k(N), an=2), epi(N, 12, an=2)]}, analysers="harmonic",
            rule="FX_HARMONIC_ONLY: <N,0,1>"),
    ]
for N in (256, 512):
    ROWS += [
        # no hop kernel and no frame_tail kernel below 1024 points: every one-frame call is the direct form + the T == 1 fused tail
        row("direct-%d" % N, N, "hops", 1, 50, {1: [frame(N, 1, 5, 1, direct=1), epi(N, 1)]}, rule="one frame, N < 1024"),
        # a call of two hops below 1024 points is the batch form (two one-frame launches need N >= 1024), two channels per workgroup
        row("two-hop-%d" % N, N, "hops", 2, 26, {2: [frame(N, 2, 2, 2), epi(N, 2)]}, rule="T == 2, N < 1024: batch form"),
    ]
for N in BIG_N:
    ROWS += [
        # C * N <= 2^20 (2^22 at 4096 points): one launch of fx_hop_kernel<N,false>
        row("hop-%d" % N, N, "hops", 1, 50, {1: [hop(N)]}, rule="one frame, C x N under the hop kernel's limit"),
        # the hop kernel switched off: groups <= one round of workgroups, frames and tails in one launch
        row("frame-tail-%d" % N, N, "hops", 1, 50, {1: [frame_tail(N, _ch1(N))]}, tuning=NO_HOP, rule="groups <= 2 x CUs: fx_frame_tail_kernel"),
        # hook 4 (never fused): the direct form + the T == 1 form of fx_tail_fused_kernel
        row("direct-%d" % N, N, "hops", 1, 50, {1: [frame(N, 1, _ch1(N), 1, direct=1), epi(N, 1)]}, tuning=NO_HOP, hooks=4,
            rule="FX_HOOK_TAIL_NEVER_FUSED: frame kernel, then the one-frame tail"),
        # two hops: two one-frame launches, the second reading hop 1 / writing frame 1 (out_stride 2)
        row("two-hop-%d" % N, N, "hops", 2, 26, {2: [hop(N, stride=2)] * 2}, rule="T == 2, N >= 1024: two one-frame launches"),
        row("two-hop-frame-tail-%d" % N, N, "hops", 2, 26, {2: [frame_tail(N, _ch1(N), stride=2)] * 2}, tuning=NO_HOP,
            rule="T == 2 as two launches of fx_frame_tail_kernel"),
        row("two-hop-direct-%d" % N, N, "hops", 2, 26, {2: [frame(N, 1, _ch1(N), 1, direct=1), epi(N, 1, stride=2)] * 2}, tuning=NO_HOP, hooks=4,
            rule="T == 2 as two direct launches, each with its one-frame tail"),
        # hook 32: the batch kernels' two-frame form (two channels per workgroup up to 2048 points)
        row("two-hop-batch-%d" % N, N, "hops", 2, 26, {2: [frame(N, 2, 2 if N <= 2048 else 1, 2), epi(N, 2)]}, hooks=32,
            rule="FX_HOOK_NO_TWO_LAUNCHES: the two-frame batch form"),
    ]
    H = N // 2
    for fmt in ("f32", "s16"):
        first = reblock(N, 0)               # the stream's first block, 100 samples: no hop, re-blocked into the pending samples (rows kernel)
        ROWS += [
            # a block that completes one hop out of pending samples: the one-frame kernels read [pending | block] themselves
            row("block-hop-%d-%s" % (N, fmt), N, "samples", (100, H), 51, {0: [first], 1: [hop(N, block=1)]}, fmt=fmt,
                rule="block feed: fx_hop_kernel<N,true>"),
            row("block-frame-tail-%d-%s" % (N, fmt), N, "samples", (100, H), 51, {0: [first], 1: [frame_tail(N, _ch1(N), block=1)]},
                tuning=NO_HOP, fmt=fmt, rule="block feed: fx_frame_tail_kernel<N,true>"),
            row("block-direct-%d-%s" % (N, fmt), N, "samples", (100, H), 51, {0: [first], 1: [frame(N, 1, _ch1(N), 1, direct=1, block=1), epi(N, 1)]},
                tuning=NO_HOP, hooks=4, fmt=fmt, rule="block feed: the direct block-fed frame kernel"),
            # a block that completes two hops: two block-fed one-frame launches, the second leaving the rest
            row("block-two-hop-%d-%s" % (N, fmt), N, "samples", (100, 2 * H), 26, {0: [first], 2: [hop(N, block=1, stride=2)] * 2}, fmt=fmt,
                rule="block feed of two hops: two one-frame launches"),
        ]
for N in (2048, 4096):
    ROWS += [
        # the low-latency family: a frame across a pair of wavefronts (as many pairs as the launch bound allows: 8 / 6)
        row("pair-%d" % N, N, "hops", 12, 5, {12: [pair(N, 12, 1, 8 if N == 2048 else 6), epi(N, 12)]}, low_latency=True,
            rule="FX_LOW_LATENCY, T > 1: fx_pair_kernel"),
        row("hop-pair-%d" % N, N, "hops", 1, 50, {1: [hop(N, pairs=True)]}, low_latency=True, rule="FX_LOW_LATENCY, one frame: fx_hop_pair_kernel"),
        row("pair-one-frame-%d" % N, N, "hops", 1, 50, {1: [pair(N, 1, 1, 1), epi(N, 1)]}, low_latency=True, tuning=NO_HOP,
            rule="FX_LOW_LATENCY without the hop kernel: fx_pair_kernel + the one-frame tail"),
        # pairs never take the two-launch form
        row("pair-two-hop-%d" % N, N, "hops", 2, 26, {2: [pair(N, 2, 1, 2), epi(N, 2)]}, low_latency=True, rule="FX_LOW_LATENCY, T == 2"),
    ]
ROWS += [
    # T in 2 .. 8: fx_tail_fused_kernel's frame-per-lane form
    row("fused-tail-256", 256, "hops", 4, 13, {4: [frame(256, 4, 1, 4), epi(256, 4)]}, rule="2 <= T <= 8: fused tail"),
    # one analyser, one frame: no direct form (it needs both), four channels per workgroup, the one-frame tail
    row("spectral-one-frame-1024", 1024, "hops", 1, 50, {1: [frame(1024, 1, 4, 1, an=1), epi(1024, 1, an=1)]}, analysers="spectral",
        rule="FX_SPECTRAL_ONLY, T == 1"),
    row("spectral-one-frame-256", 256, "hops", 1, 50, {1: [frame(256, 1, 4, 1, an=1), epi(256, 1, an=1)]}, analysers="spectral",
        rule="FX_SPECTRAL_ONLY, T == 1"),
    row("harmonic-one-frame-1024", 1024, "hops", 1, 50, {1: [frame(1024, 1, 4, 1, an=2), epi(1024, 1, an=2)]}, analysers="harmonic",
        rule="FX_HARMONIC_ONLY, T == 1"),
    row("harmonic-one-frame-4096", 4096, "hops", 1, 50, {1: [frame(4096, 1, 4, 1, an=2), epi(4096, 1, an=2)]}, analysers="harmonic",
        rule="FX_HARMONIC_ONLY, T == 1"),
    # the hop kernel's limit crossed by channel count: 1025 x 1024 > 2^20 -> the batch kernels, 129 workgroups of 8 <= 512: one launch
    row("frame-tail-by-count-1024", 1024, "hops", 1, 50, {1: [frame_tail(1024, 8)]}, C=1025, rule="C x N > 2^20: batch kernels"),
    # cut in time: the default unit (8 waves x 8 frames at 1024 points): 96 frames = two units of 48
    row("cut-default-1024", 1024, "hops", 96, 3, {96: [frame(1024, 96, 1, 8, chunks=2), epi(1024, 96)]}, C=3, rule="T ~ 1.5 units: two equal units"),
    # frames_per_unit = 16 at 2048 points (never cut by default): three units of 16
    row("cut-frames-per-unit-2048", 2048, "hops", 48, 3, {48: [frame(2048, 48, 1, 4, chunks=3), epi(2048, 48)]}, C=3,
        tuning={"frames_per_unit": 16}, rule="fx_tuning::frames_per_unit"),
    # frames_per_unit = 8, T = 8 units: the plan of thirds, 24 16 8 8 8
    row("cut-thirds-1024", 1024, "hops", 64, 3, {64: [frame(1024, 64, 1, 8, chunks=5), epi(1024, 64)]}, C=3, tuning={"frames_per_unit": 8},
        rule="T >= 8 units: units of decreasing length"),
    # unit_plan gives the lengths outright
    row("cut-plan-512", 512, "hops", 40, 3, {40: [frame(512, 40, 1, 8, chunks=3), epi(512, 40)]}, C=3, tuning={"unit_plan": [8, 16, 16]},
        rule="fx_tuning::unit_plan"),
    # a cut call short enough for the fused tail, which then clears the ticket queue itself (two waves per channel, so that T >= 2 k)
    row("cut-plan-fused-256", 256, "hops", 8, 7, {8: [frame(256, 8, 1, 2, chunks=2), epi(256, 8)]}, C=3,
        tuning={"unit_plan": [4, 4], "waves_per_channel": 2}, rule="unit_plan with T <= 8: the fused tail clears the queue"),
    row("cut-pair-2048", 2048, "hops", 48, 3, {48: [pair(2048, 48, 1, 8, chunks=3), epi(2048, 48)]}, C=3, low_latency=True,
        tuning={"frames_per_unit": 16}, rule="fx_pair_kernel cut in time"),
    # pre-assembled windows (hop_mode 0)
    row("frames-1024", 1024, "frames", 12, 5, {12: [frame(1024, 12, 1, 8), epi(1024, 12)]}, rule="fx_process_frames, T > 8"),
    row("frames-one-frame-1024", 1024, "frames", 1, 50, {1: [hop(1024)]}, rule="fx_process_frames, one frame: the hop kernel"),
    # blocks of more than two hops at 1024 points: one launch of the batch kernel's block-fed form (<1024,1,1,0,1>)
    row("block-batch-1024-f32", 1024, "samples", (100, 1600), 17, {0: [reblock(1024, 0)], 3: [frame(1024, 3, 1, 3, block=1), epi(1024, 3)],
                                                                 4: [frame(1024, 4, 1, 4, block=1), epi(1024, 4)]}, C=3, rule="block feed, 2 < hops"),
    row("block-batch-1024-s16", 1024, "samples", (100, 1600), 17, {0: [reblock(1024, 0)], 3: [frame(1024, 3, 1, 3, block=1), epi(1024, 3)],
                                                                 4: [frame(1024, 4, 1, 4, block=1), epi(1024, 4)]}, C=3, fmt="s16",
        rule="block feed, 2 < hops"),
    # ... cut in time as well (97 / 98 hops: two units)
    row("block-batch-cut-1024-f32", 1024, "samples", (100, 50000), 3, {0: [reblock(1024, 0)], 97: [frame(1024, 97, 1, 8, block=1, chunks=2), epi(1024, 97)],
                                                                      98: [frame(1024, 98, 1, 8, block=1, chunks=2), epi(1024, 98)]}, C=3,
        rule="block feed, cut in time"),
    # ... up to 4096 hops per call; one more and the call is re-blocked (fx_reblock_kernel<4>), then the batch kernel over the hops
    row("block-4096-hops-1024-s16", 1024, "samples", (100, 4096 * 512), 4, {0: [reblock(1024, 0)],
                                                                           4096: [frame(1024, 4096, 1, 8, block=1, chunks=14), epi(1024, 4096)]}, C=2,
        fmt="s16", rule="the block feed's limit: 4096 hops"),
    row("block-4097-hops-1024-f32", 1024, "samples", (100, 4097 * 512), 4, {0: [reblock(1024, 0)],
                                                                           4097: [reblock(1024, 4), frame(1024, 4097, 1, 8, chunks=14), epi(1024, 4097)]},
        C=2, rule="beyond the block feed's limit: re-blocked"),
    # hook 16 (no block feed): every block re-blocked; the kernel by row length (pieces of 16 bytes per row: < 256 rows kernel, then
    # <1> / <2> / <4> pieces per thread)
    row("reblock-1-1024-f32", 1024, "samples", (1500, 1500), 18, {2: [reblock(1024, 1), hop(1024, stride=2), hop(1024, stride=2)],
                                                                  3: [reblock(1024, 1), frame(1024, 3, 1, 3), epi(1024, 3)]}, hooks=16,
        rule="FX_HOOK_NO_BLOCK_FEED: fx_reblock_kernel<1>"),
    row("reblock-rows-1024-s16", 1024, "samples", (1500, 1500), 18, {2: [reblock(1024, 0), hop(1024, stride=2), hop(1024, stride=2)],
                                                                     3: [reblock(1024, 0), frame(1024, 3, 1, 3), epi(1024, 3)]}, hooks=16, fmt="s16",
        rule="FX_HOOK_NO_BLOCK_FEED: fx_reblock_rows_kernel"),
    row("reblock-2-1024-f32", 1024, "samples", (2500, 2500), 11, {4: [reblock(1024, 2), frame(1024, 4, 1, 4), epi(1024, 4)],
                                                                  5: [reblock(1024, 2), frame(1024, 5, 1, 5), epi(1024, 5)]}, hooks=16,
        rule="FX_HOOK_NO_BLOCK_FEED: fx_reblock_kernel<2>"),
    row("reblock-1-1024-s16", 1024, "samples", (2500, 2500), 11, {4: [reblock(1024, 1), frame(1024, 4, 1, 4), epi(1024, 4)],
                                                                  5: [reblock(1024, 1), frame(1024, 5, 1, 5), epi(1024, 5)]}, hooks=16, fmt="s16",
        rule="FX_HOOK_NO_BLOCK_FEED: fx_reblock_kernel<1>"),
    row("reblock-4-1024-f32", 1024, "samples", (5000, 5000), 6, {9: [reblock(1024, 4), frame(1024, 9, 1, 8), epi(1024, 9)],
                                                                 10: [reblock(1024, 4), frame(1024, 10, 1, 8), epi(1024, 10)]}, hooks=16,
        rule="FX_HOOK_NO_BLOCK_FEED: fx_reblock_kernel<4>"),
    row("reblock-2-1024-s16", 1024, "samples", (5000, 5000), 6, {9: [reblock(1024, 2), frame(1024, 9, 1, 8), epi(1024, 9)],
                                                                 10: [reblock(1024, 2), frame(1024, 10, 1, 8), epi(1024, 10)]}, hooks=16, fmt="s16",
        rule="FX_HOOK_NO_BLOCK_FEED: fx_reblock_kernel<2>"),
    # 2048 points: more than two hops per block are re-blocked (no batch block-fed form beyond 1024 points)
    row("reblock-three-hops-2048-f32", 2048, "samples", (100, 3072), 18, {0: [reblock(2048, 0)], 3: [reblock(2048, 2), frame(2048, 3, 1, 3), epi(2048, 3)]},
        C=3, rule="N > 1024, hops > 2: re-blocked"),
    row("reblock-three-hops-2048-s16", 2048, "samples", (100, 3072), 18, {0: [reblock(2048, 0)], 3: [reblock(2048, 1), frame(2048, 3, 1, 3), epi(2048, 3)]},
        C=3, fmt="s16", rule="N > 1024, hops > 2: re-blocked"),
    # the ring: one hop per batch is one launch of fx_hop_kernel (results and flag written by the kernel)
    row("ring-hop-1024", 1024, "ring", 1, 50, {1: [hop(1024)]}, rule="ring, one hop: fx_hop_kernel"),
    row("ring-hop-4096", 4096, "ring", 1, 50, {1: [hop(4096)]}, rule="ring, one hop: fx_hop_kernel"),
    row("ring-hop-pair-2048", 2048, "ring", 1, 50, {1: [hop(2048, pairs=True)]}, low_latency=True, rule="ring, one hop, pairs"),
    # captured steps (replayed from the second call of a slot and parity on): never the frame_tail form, never cut
    row("ring-graph-1024", 1024, "ring", 1, 50, {1: [frame(1024, 1, 5, 1, direct=1), epi(1024, 1)]}, tuning={"stream_hop_kernel": 0},
        rule="ring, captured step without the hop kernel"),
    row("ring-graph-256", 256, "ring", 1, 50, {1: [frame(256, 1, 5, 1, direct=1), epi(256, 1)]}, rule="ring, captured step (no hop kernel at 256)"),
    row("ring-graph-4-512", 512, "ring", 4, 13, {4: [frame(512, 4, 1, 4), epi(512, 4)]}, rule="ring, captured step of four hops"),
    # the three-queue path (no capture): the step fx_run() makes
    row("ring-queues-hop-2048", 2048, "ring", 1, 50, {1: [hop(2048)]}, tuning={"stream_graph": 0}, rule="ring, no capture: fx_run()'s hop kernel"),
    row("ring-queues-1024", 1024, "ring", 1, 50, {1: [frame_tail(1024, 5)]}, tuning={"stream_graph": 0, "one_hop_kernel": 0},
        rule="ring, no capture, no hop kernel"),
    row("ring-queues-12-2048", 2048, "ring", 12, 5, {12: [frame(2048, 12, 1, 4), epi(2048, 12)]}, tuning={"stream_graph": 0},
        rule="ring, no capture, twelve hops"),
]

# ---- the launch forms the kernel sources build (tests/test_dispatch_cpu.py parses them) and the window sizes each exists at ----
FORMS = {
    "fx_frame_kernel<N,true,true>": ALL_N,
    "fx_frame_kernel<N,true,false>": ALL_N,
    "fx_frame_kernel<N,false,true>": ALL_N,
    "fx_frame_kernel<N,true,true,true>": ALL_N,
    "fx_frame_kernel<N,true,true,true,true>": BIG_N,
    "fx_frame_kernel<N,true,true,false,true>": (1024,),
    "fx_frame_tail_kernel<N,false>": BIG_N,
    "fx_frame_tail_kernel<N,true>": BIG_N,
    "fx_pair_kernel<N>": (2048, 4096),
    "fx_tail_fused_kernel": ALL_N,
    "fx_finalise_kernel": ALL_N,
    "fx_epilogue_kernel": ALL_N,
    "fx_history_kernel": ALL_N,
    "fx_hop_kernel<N,false>": BIG_N,
    "fx_hop_kernel<N,true>": BIG_N,
    "fx_hop_pair_kernel<N>": (2048, 4096),
    "fx_reblock_rows_kernel": (1024,),
    "fx_reblock_kernel<1>": (1024,),
    "fx_reblock_kernel<2>": (1024,),
    "fx_reblock_kernel<4>": (1024,),
}
# forms of one kernel the table must cover apart: fx_tail_fused_kernel's one-frame branch (tail_one_hop) at every size
SUBFORMS = {"fx_tail_fused_kernel[T=1]": ALL_N, "fx_tail_fused_kernel[T>1]": ALL_N}


def kernels_of(launch):
    """the kernel forms (FORMS / SUBFORMS keys) one recorded launch runs"""
    k, N = launch["kind"], launch["window"]
    if k == "frame":
        if launch["direct_state"]:
            name = "fx_frame_kernel<N,true,true,true,true>" if launch["block_mode"] else "fx_frame_kernel<N,true,true,true>"
        elif launch["block_mode"]:
            name = "fx_frame_kernel<N,true,true,false,true>"
        else:
            name = {3: "fx_frame_kernel<N,true,true>", 1: "fx_frame_kernel<N,true,false>", 2: "fx_frame_kernel<N,false,true>"}[launch["analysers"]]
        return [name]
    if k == "frame_tail":
        return ["fx_frame_tail_kernel<N,%s>" % ("true" if launch["block_mode"] else "false")]
    if k == "hop":
        return ["fx_hop_kernel<N,%s>" % ("true" if launch["block_mode"] else "false")]
    if k == "hop_pair":
        return ["fx_hop_pair_kernel<N>"]
    if k == "pair":
        return ["fx_pair_kernel<N>"]
    if k == "epilogue":
        if launch["ep_form"] == 1:
            return ["fx_tail_fused_kernel", "fx_tail_fused_kernel[T=1]" if launch["ep_T"] == 1 else "fx_tail_fused_kernel[T>1]"]
        return ["fx_finalise_kernel", "fx_epilogue_kernel", "fx_history_kernel"]
    if k == "reblock":
        return ["fx_reblock_rows_kernel" if launch["reblock"] == 0 else "fx_reblock_kernel<%d>" % launch["reblock"]]
    return []


def covered():
    """{(form, N)} the expected sequences of all rows launch"""
    out = set()
    for r in ROWS:
        for seq in r.expect.values():
            for launch in seq:
                for name in kernels_of(launch):
                    out.add((name, launch["window"]))
    return out


def timed_by_default(launches):
    """include/fx.h, fx_tuning::call_timing = -1: a call is timed when its launches analyse more than one frame per channel each"""
    return any(l["kind"] in ("frame", "pair") and l["T"] > 1 for l in launches)


def stream(C, hops, N, seed=0):
    """[C][hops][N/2]: the four signals of tests/signals.py one after another -- bursts, low tones, a tone with vibrato and noise, impulses
    on the window boundary -- so that onsets, silent stretches and a full flux state all cross call boundaries"""
    import signals
    q = hops // 4
    parts = [signals.bursts(C, q, N, seed=seed + 4), signals.low_tones(C, q, N, seed=seed + 7),
             signals.tone_vibrato_noise(C, q, N, seed=seed + 1), signals.impulse_on_boundary(C, hops - 3 * q, N)]
    return np.ascontiguousarray(np.concatenate(parts, axis=1).astype(np.float32))
