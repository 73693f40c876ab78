"""Listening tracks on one MI355X (include/fx.h, fx_set_channel_listen): what hearing the monitor output adds to a tick.

  live     a 480-sample fp32 fx_push_sources tick, 1024-point windows, 1024 and 8192 tracks each looping its own 48 000-sample clip,
           the monitor enabled with 64 sends on (every C / 64-th track): the PARENT commit's library (--parent-lib: the libfx_hip.so
           of the parent's tree, built beside this one) against this library with (a) no listener, (b) two listeners (tracks 0 and 1,
           left and right: the reference's case) and (c) every track listening.  Timed as profiles/monitor_mix.txt: 64 calls back to
           back on the library's stream through the C ABI, outputs preallocated, one synchronisation per pass, passes of the four
           alternated, median pass.  Before the passes the launch record of a tick of (a) is compared with the parent's.
  kernels  ticks with every track listening, for a kernel trace in a run of its own: the two live shapes, and 8192 tracks x 4800
           samples at 2048 points, where a tick's block is 157 MB and is re-blocked afterwards (fx_reblock_kernel moves the same
           bytes from cold HBM: the yardstick of profiles/clip_sources.txt).  Then the summary:
             rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/listen_rate.py kernels
             python tools/listen_rate.py summary DIR

Prints plain lines; profiles/monitor_listen.txt holds a run's output.
"""
import argparse
import csv
import ctypes
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import monitor_rate as mr                                                                      # noqa: E402

capi = mr.capi
SHAPES = [(1024, 480, 1024, 48000), (8192, 480, 1024, 48000), (8192, 4800, 2048, 65536)]       # tracks, tick, window, clip length
SENDS = 64


class Listening(mr.Playing):
    """mr.Playing with the monitor on, SENDS sends on and `listeners` tracks hearing the outputs (left and right in turn)"""

    def __init__(self, torch, lib, C, seed, listeners, n=mr.N_TICK, window=mr.WINDOW, clip=mr.CLIP):
        super().__init__(torch, lib, C, seed, monitor=True, window=window, clip=clip)
        self.n = n
        self.sm = torch.empty((C, max(1, (n + window // 2 - 1) // (window // 2)), 12), dtype=torch.float32, device="cuda")
        ints = lambda v: (ctypes.c_int * len(v))(*v)                                           # noqa: E731
        tracks = list(range(C))
        self.check(lib.fx_set_channel_monitor(self.h, ints(tracks), C, ints([1 if t % (C // SENDS) == 0 else 0 for t in tracks]), None, None))
        if listeners:
            self.check(lib.fx_set_channel_listen(self.h, ints(tracks[:listeners]), listeners, ints([1 + t % 2 for t in range(listeners)])))

    def tick(self):
        self.check(self.lib.fx_push_sources(self.h, None, self.n, capi.SAMPLE_F32, capi.MEM_DEVICE, None, ctypes.c_void_p(self.sm.data_ptr()), None))

    def record(self):
        cap, fields = capi.LAUNCH_RECORD_CAP, len(capi.LAUNCH_FIELDS)
        buf = (ctypes.c_int * (cap * fields))()
        fn = self.lib.fx_last_launches_internal
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int], ctypes.c_int
        count = fn(self.h, buf, cap)
        return [tuple(buf[i * fields:(i + 1) * fields]) for i in range(min(count, cap))]


def live(reps, parent_lib, calls=64):
    import torch
    ours = capi.load_library(build_if_missing=False)
    parent = mr._library(parent_lib)
    assert hasattr(parent, "fx_enable_monitor") and not hasattr(parent, "fx_set_channel_listen"), "--parent-lib is not the parent commit's library"
    for C, n, window, clip in SHAPES[:2]:
        runs = [("parent commit", Listening(torch, parent, C, 7, 0)), ("this commit, no listener", Listening(torch, ours, C, 7, 0)),
                ("this commit, two listeners", Listening(torch, ours, C, 7, 2)), ("this commit, all listening", Listening(torch, ours, C, 7, C))]
        torch.cuda.synchronize()
        for _, p in runs:
            p.one_pass(calls)                                   # warm: buffers sized, kernels loaded
        records = [p.record() for _, p in runs]
        kinds = lambda rec: [capi.LAUNCH_KINDS.get(r[0], r[0]) for r in rec]                   # noqa: E731
        print("record: %5d tracks: parent %s; no listener %s: identical %s; two listeners %s"
              % (C, kinds(records[0]), kinds(records[1]), records[0] == records[1], kinds(records[2])), flush=True)
        times = [[] for _ in runs]
        order = [[0, 1, 2, 3], [3, 0, 1, 2], [2, 3, 0, 1], [1, 2, 3, 0]]
        for r in range(reps):
            for i in order[r % 4]:
                times[i].append(runs[i][1].one_pass(calls))
        med = [statistics.median(t) for t in times]
        for (label, _), m, t in zip(runs, med, times):
            print("live: %5d tracks, %d sends on, %d-sample f32 ticks, %d-pt, %d calls back to back per pass, median of %d passes "
                  "(min %.1f, max %.1f): %-27s %.1f us per fx_push_sources call: %+.1f us against the parent"
                  % (C, SENDS, n, window, calls, reps, min(t), max(t), label + ":", m, m - med[0]), flush=True)
        for _, p in runs:
            p.close()


def kernels(reps):
    import torch
    ours = capi.load_library(build_if_missing=False)
    for C, n, window, clip in SHAPES:
        p = Listening(torch, ours, C, 7, C, n, window, clip)
        for _ in range(reps):
            p.tick()
        torch.cuda.synchronize()
        print("kernels: C = %d, n = %d, %d-pt: %d ticks" % (C, n, window, reps), flush=True)
        p.close()
        del p


def summary(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    if not rows:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    span = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))                      # noqa: E731
    listen = [span(r) for r in rows if "fx_monitor_listen_kernel" in r.get("Kernel_Name", "")]
    S = len(SHAPES)
    if not listen or len(listen) % S:
        raise SystemExit("%d launches of fx_monitor_listen_kernel are not %d equal runs" % (len(listen), S))
    per = len(listen) // S
    for i, (C, n, window, clip) in enumerate(SHAPES):
        mine = listen[i * per:(i + 1) * per]
        lo, hi = mine[0][0], mine[-1][1] + 10 ** 6              # (the analysis launches of the last tick follow its copy)
        med = statistics.median(e - s for s, e in mine) * 1e-9
        written = C * n * 4
        line = ("kernels: C = %5d  n = %4d  %d-pt, every track listening: fx_monitor_listen_kernel %.1f us (median of %d), %d bytes written: %.2f TB/s"
                % (C, n, window, med * 1e6, per, written, written / med / 1e12))
        for name in ("fx_clip_gather_kernel", "fx_monitor_mix_kernel", "fx_reblock_kernel"):
            t = [e - s for r in rows if name in r.get("Kernel_Name", "") for s, e in [span(r)] if lo <= s <= hi]
            if t:
                m = statistics.median(t) * 1e-9
                line += ";  %s %.1f us (median of %d)" % (name, m * 1e6, len(t))
                if name != "fx_monitor_mix_kernel":
                    line += ", %.2f TB/s of %d bytes read + written" % (2 * written / m / 1e12, 2 * written)
        print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["live", "kernels", "summary"])
    ap.add_argument("trace_dir", nargs="?")
    ap.add_argument("--reps", type=int, default=16)
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
