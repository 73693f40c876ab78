"""What deriving ranges and distributions from a feature buffer costs on one MI355X (include/fx.h, fx_offline_feature_ranges /
fx_offline_feature_distribution), beside the same work done the only way there was before them: copy the buffer to the host, then numpy.

  rate       a device-resident feature buffer [10][1024][4096] (rows of one LDS sort each) and [10][64][65536] (rows through the scratch:
             chunk sorts, global strides, chunk merges), num_brackets = 10, through the C ABI.  A call is timed between two synchronisations
             of the object's stream; warmed first, median of --reps calls.  The distribution is also timed with num_brackets = D (step 1: the
             walk is one add per lane, so this is the sort) and num_brackets = 1 (one lane walks the whole row: the serial sum at its worst).
             The host route: the copy to the host, then ranges by numpy's min / max and distributions by np.sort on the integer key plus
             np.add.accumulate (the serial fp32 sum), the rows dealt to --threads threads (numpy releases the interpreter lock in both).
  resources  registers, LDS and scratch of the kernels as built (tools/kernel_resources.py; needs no GPU).

Prints plain lines and writes them to --out (profiles/offline_stats.txt holds a run's output).
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
fx = importlib.import_module("feature-extractor_amd")
capi = fx.capi

SHAPES = ((10, 1024, 4096), (10, 64, 65536))
BRACKETS = 10
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(lib, h, call, reps):
    def once():
        capi.check(lib.fx_offline_sync(h))
        t0 = time.perf_counter()
        capi.check(call())
        capi.check(lib.fx_offline_sync(h))
        return time.perf_counter() - t0
    once()                                      # warm: scratch made, kernels loaded
    return statistics.median(once() for _ in range(reps))


def host_keys(v):
    b = v.view(np.uint32)
    keys = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    keys[np.isnan(v)] = np.uint32(0xFFFFFFFF)
    return keys


def host_distribution(rows, nb):
    """rows [n][D] -> [n][nb]: sort on the key, serial fp32 sums from +0.0f"""
    keys = np.sort(host_keys(rows), axis=-1)
    s = np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).view(np.float32)
    step = rows.shape[1] // nb
    s = s[:, :nb * step].reshape(rows.shape[0], nb, step)
    lead = np.zeros((rows.shape[0], nb, 1), np.float32)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([lead, s], axis=-1), axis=-1, dtype=np.float32)[..., -1] / np.float32(step)


def rate(reps, threads):
    import torch
    lib = capi.load_library(build_if_missing=False)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    for R, C, D in SHAPES:
        an = fx.offline.AudioAnalyser(C)
        g = torch.Generator(device="cuda").manual_seed(11)
        rows = torch.randn((R, C, D), generator=g, device="cuda")
        n = R * C
        ranges = torch.empty((R, C, 2), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t = timed(lib, an._h, lambda: lib.fx_offline_feature_ranges(an._h, ptr(rows), R, D, ptr(ranges), capi.MEM_DEVICE), reps)
        say("ranges:       [%d][%d][%d] (%d rows, %.0f MB): fx_offline_feature_ranges %.3f ms (median of %d) = %.2f TB/s read"
            % (R, C, D, n, 4e-6 * n * D, t * 1e3, reps, 4.0 * n * D / t / 1e12))
        times = {}
        for nb in (BRACKETS, D, 1):
            dist = torch.empty((R, C, nb), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            times[nb] = timed(lib, an._h, lambda: lib.fx_offline_feature_distribution(an._h, ptr(rows), R, D, nb, ptr(dist), capi.MEM_DEVICE), reps)
            if nb == BRACKETS:
                check = dist.cpu().numpy().reshape(n, nb)[:64]
            del dist
        say("distribution: [%d][%d][%d], %d brackets: fx_offline_feature_distribution %.3f ms = %.3g rows/s, %.3g keys/s; with D brackets (the sort, a "
            "one-add walk) %.3f ms; with 1 bracket (one lane walks the row) %.3f ms"
            % (R, C, D, BRACKETS, times[BRACKETS] * 1e3, n / times[BRACKETS], n * D / times[BRACKETS], times[D] * 1e3, times[1] * 1e3))
        # the host route: what the buffer costs to bring over, and numpy on `threads` threads
        t0 = time.perf_counter()
        host = rows.cpu().numpy().reshape(n, D)
        t_copy = time.perf_counter() - t0
        slices = [host[k * n // threads:(k + 1) * n // threads] for k in range(threads)]
        with ThreadPoolExecutor(threads) as pool:
            t0 = time.perf_counter()
            list(pool.map(lambda s: (s.min(axis=1), s.max(axis=1)), slices))
            t_ranges = time.perf_counter() - t0
            t0 = time.perf_counter()
            parts = list(pool.map(lambda s: host_distribution(s, BRACKETS), slices))
            t_dist = time.perf_counter() - t0
        same = np.array_equal(np.concatenate(parts)[:64].view(np.uint32), check.view(np.uint32))
        say("host route:   copy to the host %.1f ms; on %d threads: min / max %.1f ms, np.sort + serial sums %.1f ms (first 64 rows equal the "
            "library's bits: %s); the library is %.0f x (ranges) and %.0f x (distribution) the host route with its copy"
            % (t_copy * 1e3, threads, t_ranges * 1e3, t_dist * 1e3, same, (t_copy + t_ranges) / t, (t_copy + t_dist) / times[BRACKETS]))
        an.close()
        del rows, ranges
    say("bounds: a row of up to FX_OFFLINE_SORT_CHUNK keys is one workgroup's LDS compare-exchange passes (for 4096 keys 21 passes of one pair "
        "per thread through LDS with a barrier each, and 7 passes of six lane-swap strides on registers), then the bracket walk: a lane per "
        "bracket adds its step values one after the other, which is the difference between the D-bracket and the 10- and 1-bracket times above (the block first turns the keys back into floats, and for long rows stages a tile of every bracket's keys in LDS, so the walking lane does a load and an add per value).  "
        "Longer rows add, per doubling beyond the chunk, one more global-memory stride pass and one more chunk merge over the whole group in "
        "the scratch: their time is the keys' round trips through global memory.")


def resources():
    import kernel_resources as kr
    fx.load_library(build_if_missing=True)
    say("the kernels as built (VGPRs / SGPRs / scratch bytes per lane / static LDS bytes per workgroup; the sorts' keys are dynamic LDS):")
    wanted = ("distribution_lds_kernel", "chunk_sort_kernel", "global_stride_kernel", "chunk_merge_kernel", "walk_kernel", "feature_ranges_kernel", "smooth_rows_kernel")
    mine = [k for k in kr.kernels_of() if k["pretty"].startswith("fxo::")]
    names = kr.demangle([k["name"] for k in mine])
    for k in mine:
        name = names[k["name"]].replace("void ", "").split("(")[0]
        if name.split("::")[-1] in wanted:
            say("  %-40s %3d / %3d / %d / %d" % (name, k["vgpr"], k.get("sgpr", 0), k.get("scratch", 0), k.get("lds", 0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["rate", "resources"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the numpy route (the CPUs a job may use)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offline_stats.txt"))
    a = ap.parse_args()
    rate(a.reps, a.threads) if a.part == "rate" else resources()
    with open(a.out, "a" if a.part == "resources" else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
