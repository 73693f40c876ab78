"""File sources on one MI355X (include/fx.h, fx_push_sources): what the gather costs.

  (a) kernels  fx_clip_gather_kernel's rate (bytes read + written per second) from cold HBM: every track plays its own long clip
               (65 536 samples; the banks are 0.5-2 GB at 8192 tracks, so each tick reads bytes no cache holds), n = 4800 samples
               per tick, C = 1024 and 8192, all four formats -- against fx_reblock_kernel in the same run: at 2048 points the
               planar block of a tick is re-blocked (in the sources context and in a twin given other planar blocks, eight in
               rotation), which moves the same bytes.  Run it under the kernel trace, in a run of its own, then summarise:
                 rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/clip_rate.py kernels
                 python tools/clip_rate.py summary DIR
  (b) live     a 480-sample fx_push_sources tick with every track playing a long clip against fx_push_samples of a planar device
               block of the same size: f32, 1024 and 8192 tracks, 1024-point windows, timed as profiles/interleave.txt (b) is
               (64 calls back to back on the library's stream through the C ABI, outputs preallocated, one synchronisation per
               pass), passes of the two alternated, median pass.
  (c) tiny     the same with every track looping a 1-sample and a 5-sample clip: the gather's byte-by-byte path.
  (d) rated    clips at their own sample rate (fx_set_clip_rates): a 480-sample fx_push_sources tick at 1024 and 8192 tracks,
               2048-point windows, with every track looping a 48 000-sample clip that is (1) unrated fp32, (2) 44.1 kHz in s16 and
               (3) 96 kHz in fp32, in a 48 kHz context -- timed as (b), passes of the three alternated, median pass.  The resample
               kernel's own time comes from a kernel trace of the same part in a run of its own (kernel_times DIR);
               profiles/clip_resample.txt holds a run's output.

Prints plain lines; profiles/clip_sources.txt holds a run's output.
"""
import argparse
import csv
import ctypes
import glob
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fx = importlib.import_module("feature-extractor_amd")

KERNEL_SHAPES = [(C, fmt) for C in (1024, 8192) for fmt in ("f32", "f16", "s16", "s24")]
N_KERNEL, L_KERNEL = 4800, 65536
BYTES = {"f32": 4, "f16": 2, "s16": 2, "s24": 3}


def _samples(torch, count, fmt, seed):
    """`count` samples of `fmt` on the device (s24: uint8, three bytes per sample)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if fmt == "s24":
        return torch.randint(0, 256, (3 * count,), generator=g, device="cuda", dtype=torch.uint8)
    if fmt == "s16":
        return torch.randint(-8000, 8000, (count,), generator=g, device="cuda", dtype=torch.int16)
    x = (torch.rand((count,), generator=g, device="cuda") - 0.5) * 0.5
    return x if fmt == "f32" else x.to(torch.float16)


def _playing(torch, C, N, fmt, L, seed, rate=None):
    """a context whose C tracks each play (looping) their own clip of L samples, files of `rate` Hz, from one borrowed bank"""
    an = fx.BatchAnalyser(C, N)
    bank = _samples(torch, C * L, fmt, seed)
    first = an.create_clips(bank, lengths=[L] * C, sample_format=fmt, borrow=True, sample_rates=rate)
    tracks = list(range(C))
    an.load_clips(tracks, [first + k for k in tracks])
    an.set_sources(tracks, "file")
    an.transport(tracks, "play")
    return an


def kernels(reps):
    import torch
    for C, fmt in KERNEL_SHAPES:
        an, twin = _playing(torch, C, 2048, fmt, L_KERNEL, C), fx.BatchAnalyser(C, 2048)
        planar = [_samples(torch, C * N_KERNEL, fmt, 50 + i).reshape(C, -1) for i in range(8)]
        for i in range(reps):
            an.push_sources(None, N_KERNEL, sample_format=fmt, device=True)     # the gather, then the re-blocker (4 hops + 704 samples)
            twin.push_samples(planar[i % 8], sample_format=fmt)
        torch.cuda.synchronize()
        print("kernels: C = %d, n = %d, %s: %d calls each" % (C, N_KERNEL, fmt, reps), flush=True)
        an.close(); twin.close()
        del planar


def summary(trace_dir):
    paths = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows = []
    for p in paths:
        with open(p) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # `kernels` runs the shapes one after the other, the same number of calls each: the launches of each kernel, in time order, fall
    # into len(KERNEL_SHAPES) equal runs (the re-blocker runs in both contexts' calls: twice as many launches)
    times = {"gather": [], "reblock": []}
    for r in rows:
        name = r.get("Kernel_Name", "")
        kind = "gather" if "fx_clip_gather_kernel" in name else "reblock" if "fx_reblock" in name else None
        if kind:
            times[kind].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    S = len(KERNEL_SHAPES)
    if any(len(v) % S or not v for v in times.values()):
        raise SystemExit("launch counts %s are not %d equal runs" % ({k: len(v) for k, v in times.items()}, S))
    for i, (C, fmt) in enumerate(KERNEL_SHAPES):
        nbytes = 2 * C * N_KERNEL * BYTES[fmt]                       # read + written (table rows and the re-blocker's carry bytes left out)
        ga = times["gather"][i * len(times["gather"]) // S:(i + 1) * len(times["gather"]) // S]
        rb = times["reblock"][i * len(times["reblock"]) // S:(i + 1) * len(times["reblock"]) // S]
        tg, tr = statistics.median(ga) * 1e-9, statistics.median(rb) * 1e-9
        print("(a) C = %5d  n = %d  %s: fx_clip_gather_kernel %.2f TB/s (median %.1f us of %d), fx_reblock_kernel %.2f TB/s "
              "(median %.1f us of %d): ratio %.2f" % (C, N_KERNEL, fmt, nbytes / tg / 1e12, tg * 1e6, len(ga), nbytes / tr / 1e12, tr * 1e6,
                                                     len(rb), tr / tg))


def kernel_times(trace_dir):
    """every kernel of a trace: median duration by name and grid (for a trace of `live`: what the gather adds on the GPU)"""
    by = {}
    for p in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(p) as f:
            for r in csv.DictReader(f):
                key = (r.get("Kernel_Name", "")[:90], r.get("Grid_Size_X", ""), r.get("Grid_Size_Y", ""))
                by.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for (name, gx, gy), v in sorted(by.items()):
        print("    %8.1f us median of %4d  grid %s x %s  %s" % (statistics.median(v) * 1e-3, len(v), gx, gy, name))


def live(reps, lengths, label, calls=64):
    """`calls` calls back to back on the library's own stream through the C ABI -- outputs preallocated on the device, no allocation,
    no stream wait, no other call in between -- then one synchronisation; time per call = the pass over `calls`.  Passes of the two
    entry points alternate; the median pass counts."""
    import torch
    n = 480
    for L in lengths:
        for C in (1024, 8192):
            an, twin = _playing(torch, C, 1024, "f32", L, 7 + L), fx.BatchAnalyser(C, 1024)
            planar = [_samples(torch, C * n, "f32", 100 + i).reshape(C, n) for i in range(8)]
            sm = [torch.empty((C, 1, 12), dtype=torch.float32, device="cuda") for _ in range(2)]   # a 480-sample block completes <= 1 hop
            torch.cuda.synchronize()
            lib = an._lib
            F32, DEV = fx.capi.SAMPLE_F32, fx.capi.MEM_DEVICE

            def sources(b):
                return lib.fx_push_sources(an._h, None, n, F32, DEV, None, ctypes.c_void_p(sm[0].data_ptr()), None)

            def plain(b):
                return lib.fx_push_samples(twin._h, ctypes.c_void_p(planar[b % 8].data_ptr()), n, F32, DEV, None,
                                           ctypes.c_void_p(sm[1].data_ptr()), None)

            def one_pass(fn, a):
                a.sync()
                t0 = time.perf_counter()
                for b in range(calls):
                    fx.capi.check(fn(b))
                a.sync()
                return (time.perf_counter() - t0) / calls * 1e6

            one_pass(sources, an); one_pass(plain, twin)              # warm: buffers sized, kernels loaded
            ts, tp = [], []
            for r in range(reps):
                if r % 2 == 0:
                    ts.append(one_pass(sources, an)); tp.append(one_pass(plain, twin))
                else:
                    tp.append(one_pass(plain, twin)); ts.append(one_pass(sources, an))
            a, b = statistics.median(ts), statistics.median(tp)
            print("(%s) %5d tracks each looping a %d-sample clip, %d-sample f32 ticks, 1024-pt, %d calls back to back per pass, median of %d "
                  "passes: fx_push_sources %.1f us, fx_push_samples (planar device block) %.1f us per call: +%.1f us, ratio %.3f"
                  % (label, C, L, n, calls, reps, a, b, a - b, a / b), flush=True)
            an.close(); twin.close()


RATED_SETUPS = [("unrated fp32 loops", "f32", None), ("44.1k -> 48k, s16 clips", "s16", 44100.0), ("96k -> 48k, fp32 clips", "f32", 96000.0)]


def rated(reps, calls=64):
    """(d): the three set-ups' ticks, timed as live() times its two entry points"""
    import torch
    n, N, L = 480, 2048, 48000
    F32, DEV = fx.capi.SAMPLE_F32, fx.capi.MEM_DEVICE
    for C in (1024, 8192):
        ans = [_playing(torch, C, N, fmt, L, 31 + i, rate) for i, (_, fmt, rate) in enumerate(RATED_SETUPS)]
        sm = torch.empty((C, 1, 12), dtype=torch.float32, device="cuda")       # a 480-sample block completes <= 1 hop
        torch.cuda.synchronize()

        def one_pass(an):
            an.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fx.capi.check(an._lib.fx_push_sources(an._h, None, n, F32, DEV, None, ctypes.c_void_p(sm.data_ptr()), None))
            an.sync()
            return (time.perf_counter() - t0) / calls * 1e6

        for an in ans:
            one_pass(an)                                                        # warm: buffers sized, kernels loaded
        times = [[] for _ in ans]
        for r in range(reps):
            for i in ([0, 1, 2], [2, 0, 1], [1, 2, 0])[r % 3]:
                times[i].append(one_pass(ans[i]))
        med = [statistics.median(t) for t in times]
        for (label, _, _), m in zip(RATED_SETUPS, med):
            print("(d) %5d tracks each looping a %d-sample clip, %d-sample f32 ticks, %d-pt, %d calls back to back per pass, median of %d passes: "
                  "%-24s %.1f us per fx_push_sources call, %.3f x the unrated tick" % (C, L, n, N, calls, reps, label + ":", m, m / med[0]), flush=True)
        for an in ans:
            an.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["kernels", "summary", "live", "tiny", "rated", "kernel_times"])
    ap.add_argument("trace_dir", nargs="?")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if a.part == "kernels":
        kernels(min(a.reps, 12))            # (12 ticks of 4800 samples stay inside the 65 536-sample clips: no wrap, no byte read twice)
    elif a.part == "summary":
        summary(a.trace_dir)
    elif a.part == "kernel_times":
        kernel_times(a.trace_dir)
    elif a.part == "rated":
        rated(a.reps)
    elif a.part == "live":
        live(a.reps, [48000], "b")
    else:
        live(a.reps, [1, 5], "c")


if __name__ == "__main__":
    main()
