"""fx_push_interleaved on one MI355X (include/fx.h): what the de-interleave costs.

  (a) kernels  fx_deinterleave_kernel's rate (bytes read + written per second, identity map) at C = K = 1024 and 8192, n = 4800,
               f32 and s16, against fx_reblock_kernel in the same run (the planar twin at 2048 points re-blocks its 4800 samples).
               Run it under the kernel trace, in a run of its own, then summarise the trace:
                 rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/interleave_rate.py kernels
                 python tools/interleave_rate.py summary DIR
  (b) live     fx_push_interleaved against fx_push_samples of the same samples already planar: 480-sample f32 device blocks at 1024
               and 8192 channels (1024-point windows), timed as the README's planar figures are (64 calls back to back on the library's
               stream through the C ABI, outputs preallocated, one synchronisation), passes of the two alternated, median pass.
  (c) host     an interleaved host block through fx_push_interleaved against a numpy transpose + fx_push_samples of the host block.

Prints plain lines; profiles/interleave.txt holds a run's output.
"""
import argparse
import csv
import glob
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fx = importlib.import_module("feature-extractor_amd")

KERNEL_SHAPES = [(1024, "f32"), (1024, "s16"), (8192, "f32"), (8192, "s16")]
N_KERNEL = 4800


def _block(torch, n, C, fmt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.rand((n, C), generator=g, device="cuda") - 0.5) * 0.5
    return x if fmt == "f32" else (x * 32767).round().to(torch.int16)


def kernels(reps):
    import torch
    for C, fmt in KERNEL_SHAPES:
        x = _block(torch, N_KERNEL, C, fmt, C)
        planar = x.t().contiguous()
        an, twin = fx.BatchAnalyser(C, 2048), fx.BatchAnalyser(C, 2048)
        for _ in range(reps):
            an.push_interleaved(x)              # de-interleave, then the re-blocker (4800 samples = 4 hops + 512 at 2048 points)
            twin.push_samples(planar)
        torch.cuda.synchronize()
        print("kernels: C = K = %d, n = %d, %s: %d calls each" % (C, N_KERNEL, fmt, reps), flush=True)
        an.close(); twin.close()


def summary(trace_dir):
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows = []
    for p in paths:
        with open(p) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # `kernels` runs the shapes one after the other, the same number of calls each: the launches of each kernel, in time order, fall into
    # len(KERNEL_SHAPES) equal runs (the re-blocker runs in both contexts' calls: twice as many launches)
    times = {"deinterleave": [], "reblock": []}
    for r in rows:
        name = r.get("Kernel_Name", "")
        kind = "deinterleave" if "fx_deinterleave_kernel" in name else "reblock" if "fx_reblock" in name else None
        if kind:
            times[kind].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    S = len(KERNEL_SHAPES)
    if any(len(v) % S or not v for v in times.values()):
        raise SystemExit("launch counts %s are not %d equal runs" % ({k: len(v) for k, v in times.items()}, S))
    for i, (C, fmt) in enumerate(KERNEL_SHAPES):
        nbytes = 2 * C * N_KERNEL * (4 if fmt == "f32" else 2)       # read + written (the re-blocker's carry bytes left out)
        di = times["deinterleave"][i * len(times["deinterleave"]) // S:(i + 1) * len(times["deinterleave"]) // S]
        rb = times["reblock"][i * len(times["reblock"]) // S:(i + 1) * len(times["reblock"]) // S]
        td, tr = statistics.median(di) * 1e-9, statistics.median(rb) * 1e-9
        print("(a) C = K = %5d  n = %d  %s: fx_deinterleave_kernel %.2f TB/s (median %.1f us of %d), fx_reblock_kernel %.2f TB/s "
              "(median %.1f us of %d): ratio %.2f" % (C, N_KERNEL, fmt, nbytes / td / 1e12, td * 1e6, len(di), nbytes / tr / 1e12, tr * 1e6,
                                                     len(rb), tr / td))


def kernel_times(trace_dir):
    """every kernel of a trace: median duration by name and grid (for a trace of `live`: what the de-interleave adds on the GPU)"""
    by = {}
    for p in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as f:
            for r in csv.DictReader(f):
                key = (r.get("Kernel_Name", "")[:90], r.get("Grid_Size_X", ""), r.get("Grid_Size_Y", ""))
                by.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (name, gx, gy), v in sorted(by.items()):
        print("    %8.1f us median of %4d  grid %s x %s  %s" % (statistics.median(v) * 1e-3, len(v), gx, gy, name))


def _median_pair(f, g, reps):
    import torch
    a, b = [], []
    for i in range(reps):
        for fn, out in ((f, a), (g, b)) if i % 2 == 0 else ((g, b), (f, a)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(i)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
    return statistics.median(a) * 1e6, statistics.median(b) * 1e6


def live(reps, calls=64):
    """as the README's planar figures were taken (tools/device_blocks.py): `calls` calls back to back on the library's own stream
    through the C ABI -- outputs preallocated on the device, no allocation, no stream wait, no other call in between -- then one
    synchronisation; time per call = the pass over `calls`.  Passes of the two entry points alternate; the median pass counts."""
    import ctypes
    import torch
    n = 480
    for C in (1024, 8192):
        blocks = [_block(torch, n, C, "f32", 100 + i) for i in range(8)]
        planar = [x.t().contiguous() for x in blocks]
        sm = [torch.empty((C, 1, 12), dtype=torch.float32, device="cuda") for _ in range(2)]   # a 480-sample block completes <= 1 hop
        torch.cuda.synchronize()
        an, twin = fx.BatchAnalyser(C, 1024), fx.BatchAnalyser(C, 1024)
        lib = an._lib
        F32, DEV = fx.capi.SAMPLE_F32, fx.capi.MEM_DEVICE

        def inter(b):
            return lib.fx_push_interleaved(an._h, ctypes.c_void_p(blocks[b % 8].data_ptr()), n, C, F32, DEV, None,
                                           ctypes.c_void_p(sm[0].data_ptr()), None)

        def plan(b):
            return lib.fx_push_samples(twin._h, ctypes.c_void_p(planar[b % 8].data_ptr()), n, F32, DEV, None,
                                       ctypes.c_void_p(sm[1].data_ptr()), None)

        def one_pass(fn, a):
            a.sync()
            t0 = time.perf_counter()
            for b in range(calls):
                fx.capi.check(fn(b))
            a.sync()
            return (time.perf_counter() - t0) / calls * 1e6

        one_pass(inter, an); one_pass(plan, twin)                 # warm: buffers sized, kernels loaded
        ti, tp = [], []
        for r in range(reps):
            if r % 2 == 0:
                ti.append(one_pass(inter, an)); tp.append(one_pass(plan, twin))
            else:
                tp.append(one_pass(plan, twin)); ti.append(one_pass(inter, an))
        a, b = statistics.median(ti), statistics.median(tp)
        print("(b) %5d ch, %d-sample f32 device blocks, 1024-pt, %d calls back to back per pass, median of %d passes: fx_push_interleaved "
              "%.1f us, fx_push_samples (planar) %.1f us per call, ratio %.3f" % (C, n, calls, reps, a, b, a / b), flush=True)
        an.close(); twin.close()


def host(reps):
    n = 480
    rng = np.random.default_rng(1)
    for C in (1024, 8192):
        blocks = [(rng.random((n, C), dtype=np.float32) - 0.5) * 0.5 for _ in range(8)]
        an, twin = fx.BatchAnalyser(C, 1024), fx.BatchAnalyser(C, 1024)
        for i in range(20):
            an.push_interleaved(blocks[i % 8]); twin.push_samples(np.ascontiguousarray(blocks[i % 8].T))
        ti, tp = _median_pair(lambda i: an.push_interleaved(blocks[i % 8]),
                              lambda i: twin.push_samples(np.ascontiguousarray(blocks[i % 8].T)), reps)
        print("(c) %5d ch, %d-sample f32 host blocks, 1024-pt: push_interleaved %.1f us, numpy transpose + push_samples %.1f us, ratio %.3f"
              % (C, n, ti, tp, ti / tp), flush=True)
        an.close(); twin.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["kernels", "summary", "live", "host", "kernel_times"])
    ap.add_argument("trace_dir", nargs="?")
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    if a.part == "kernels":
        kernels(min(a.reps, 30))
    elif a.part == "summary":
        summary(a.trace_dir)
    elif a.part == "kernel_times":
        kernel_times(a.trace_dir)
    elif a.part == "live":
        live(min(a.reps, 15))
    else:
        host(a.reps)


if __name__ == "__main__":
    main()
