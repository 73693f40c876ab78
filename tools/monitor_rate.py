"""The monitor mix on one MI355X (include/fx.h, fx_enable_monitor): what it adds to a tick.

  live     a 480-sample fp32 fx_push_sources tick, 1024-point windows, 1024 and 8192 tracks each looping its own 48 000-sample clip:
           this library with the monitor enabled and every track on, and with the monitor never enabled, against the PARENT
           commit's library on the same tick (--parent-lib: the libfx_hip.so of the parent's tree, built beside this one).  Timed
           as profiles/clip_sources.txt (b): 64 calls back to back on the library's stream through the C ABI, outputs preallocated,
           one synchronisation per pass, passes of the three alternated, median pass.
  kernels  the same ticks (monitor on) for a kernel trace, in a run of its own; then the summary: the mix kernel's rate beside the
           gather's from the same trace.
             rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/monitor_rate.py kernels
             python tools/monitor_rate.py summary DIR

Prints plain lines; profiles/monitor_mix.txt holds a run's output.
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
capi = fx.capi

SHAPES = (1024, 8192)
N_TICK, WINDOW, CLIP = 480, 1024, 48000


def _library(path):
    """another build of the library (the parent commit's) beside the shipped one: the entries it has get the binding's prototypes"""
    lib = ctypes.CDLL(path)
    for name, argtypes, restype in capi.PROTOTYPES:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
    return lib


class Playing:
    """a context of `lib` whose C tracks each loop their own clip of CLIP fp32 samples from one borrowed bank, through the C ABI alone"""

    def __init__(self, torch, lib, C, seed, monitor=False, window=WINDOW, clip=CLIP):
        self.lib, self.C, self.h = lib, C, ctypes.c_void_p()
        self.check(lib.fx_create(ctypes.byref(self.h), 0, C, window, 48000.0, 0))
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.bank = (torch.rand((C * clip,), generator=g, device="cuda") - 0.5) * 0.5
        ints = lambda v: (ctypes.c_int * len(v))(*v)                                           # noqa: E731
        first = ctypes.c_int(-1)
        lengths = (ctypes.c_longlong * C)(*([clip] * C))
        self.check(lib.fx_create_clips(self.h, ctypes.c_void_p(self.bank.data_ptr()), lengths, C, capi.SAMPLE_F32, capi.MEM_DEVICE, capi.CLIP_BORROW, ctypes.byref(first)))
        tracks = ints(list(range(C)))
        self.check(lib.fx_set_channel_clips(self.h, tracks, C, ints([first.value + k for k in range(C)]), None))
        self.check(lib.fx_set_channel_sources(self.h, tracks, C, ints([capi.SOURCE_FILE] * C)))
        self.check(lib.fx_transport(self.h, tracks, C, capi.PLAY))
        if monitor:
            self.check(lib.fx_enable_monitor(self.h, 1))
            self.check(lib.fx_set_channel_monitor(self.h, tracks, C, None, None, None))       # every track on, gains 1 / 1
        self.sm = torch.empty((C, 1, 12), dtype=torch.float32, device="cuda")                  # a 480-sample block completes <= 1 hop

    def check(self, status):
        if status != capi.FX_OK:
            raise RuntimeError(self.lib.fx_last_error().decode(errors="replace"))

    def tick(self):
        self.check(self.lib.fx_push_sources(self.h, None, N_TICK, capi.SAMPLE_F32, capi.MEM_DEVICE, None, ctypes.c_void_p(self.sm.data_ptr()), None))

    def one_pass(self, calls):
        self.check(self.lib.fx_sync(self.h))
        t0 = time.perf_counter()
        for _ in range(calls):
            self.tick()
        self.check(self.lib.fx_sync(self.h))
        return (time.perf_counter() - t0) / calls * 1e6

    def close(self):
        self.lib.fx_destroy(self.h)


def live(reps, parent_lib, calls=64):
    import torch
    ours = capi.load_library(build_if_missing=False)
    parent = _library(parent_lib)
    assert not hasattr(parent, "fx_enable_monitor"), "--parent-lib is not the parent commit's library: it has the monitor"
    for C in SHAPES:
        runs = [("parent commit", Playing(torch, parent, C, 7)), ("this commit, no monitor", Playing(torch, ours, C, 7)),
                ("this commit, monitor on", Playing(torch, ours, C, 7, monitor=True))]
        torch.cuda.synchronize()
        for _, p in runs:
            p.one_pass(calls)                                   # warm: buffers sized, kernels loaded
        times = [[] for _ in runs]
        for r in range(reps):
            for i in ([0, 1, 2], [2, 0, 1], [1, 2, 0])[r % 3]:
                times[i].append(runs[i][1].one_pass(calls))
        med = [statistics.median(t) for t in times]
        for (label, _), m, t in zip(runs, med, times):
            print("live: %5d tracks each looping a %d-sample clip, %d-sample f32 ticks, %d-pt, %d calls back to back per pass, median of %d passes "
                  "(min %.1f, max %.1f): %-24s %.1f us per fx_push_sources call: %+.1f us against the parent"
                  % (C, CLIP, N_TICK, WINDOW, calls, reps, min(t), max(t), label + ":", m, m - med[0]), flush=True)
        for _, p in runs:
            p.close()


def kernels(reps):
    import torch
    ours = capi.load_library(build_if_missing=False)
    for C in SHAPES:
        p = Playing(torch, ours, C, 7, monitor=True)
        for _ in range(reps):
            p.tick()
        torch.cuda.synchronize()
        print("kernels: C = %d, n = %d: %d ticks" % (C, N_TICK, reps), flush=True)
        p.close()


def summary(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    if not rows:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # `kernels` runs the shapes one after the other with the same number of ticks: each kernel's launches, in time order, fall into
    # len(SHAPES) equal runs
    names = {"mix": "fx_monitor_mix_kernel", "sum": "fx_monitor_sum_kernel", "gather": "fx_clip_gather_kernel"}
    times = {k: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if v in r.get("Kernel_Name", "")] for k, v in names.items()}
    S = len(SHAPES)
    if any(len(v) % S or not v for v in times.values()):
        raise SystemExit("launch counts %s are not %d equal runs" % ({k: len(v) for k, v in times.items()}, S))
    stride = (N_TICK + 7) // 8 * 8
    for i, C in enumerate(SHAPES):
        groups = (C + capi.MONITOR_GROUP - 1) // capi.MONITOR_GROUP
        part = {k: v[i * len(v) // S:(i + 1) * len(v) // S] for k, v in times.items()}
        med = {k: statistics.median(v) * 1e-9 for k, v in part.items()}
        nbytes = {"mix": C * N_TICK * 4 + groups * 2 * stride * 4 + 16 * C, "sum": (groups + 1) * 2 * stride * 4, "gather": 2 * C * N_TICK * 4}
        print("kernels: C = %5d  n = %d  f32: " % (C, N_TICK) + ";  ".join(
            "%s %.1f us (median of %d), %.2f TB/s of %d bytes read + written" % (names[k], med[k] * 1e6, len(part[k]), nbytes[k] / med[k] / 1e12, nbytes[k])
            for k in ("gather", "mix", "sum")))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["live", "kernels", "summary"])
    ap.add_argument("trace_dir", nargs="?")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--parent-lib", help="live: the parent commit's libfx_hip.so")
    a = ap.parse_args()
    if a.part == "live":
        if not a.parent_lib:
            raise SystemExit("live needs --parent-lib")
        live(a.reps, a.parent_lib)
    elif a.part == "kernels":
        kernels(max(a.reps, 32))
    else:
        summary(a.trace_dir)


if __name__ == "__main__":
    main()
