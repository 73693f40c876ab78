"""The offline driver on one MI355X (include/fx.h, fx_offline_frames / fx_offline_analyse): what a file's analysis costs.

  rate       C = 64 mono files of S = 1 440 000 samples (30 s at 48 kHz), one frame every 512 samples (D = 2812), 1024- and 2048-point
             windows, every buffer device-resident, through the C ABI.  fx_offline_frames alone: frames a second, and the bytes it has to
             move -- the audio read once, the magnitudes written once -- against the 8 TB/s of the HBM.  Then the whole fx_offline_analyse,
             and the same call without the per-frame analyses (no DO_SPECTRAL, no DO_HARMONIC): the difference is the share of the D x 3
             per-frame launches.  A call is timed between two synchronisations of the object's stream (the stream is the object's own, so no
             event of the caller's can be recorded on it; a call runs for milliseconds to seconds, the two host calls for microseconds);
             warmed first, median of --reps calls.
  files      fx_offline_analyse_files on a library: 64 device-resident files of 10 to 50 s at 48 kHz (mean 30 s) in one bank, one D for all
             (2812: a step of 512 at the mean length), 1024- and 2048-point windows, S16 and F32: the frame stage alone (what = 0), then the
             whole analysis.  Then, on an equal-length F32 bank, the frame stage through the files entry and fx_offline_frames on the same
             audio, alternating in one run, both warmed first, the median and the range of the same --reps each: the difference is read
             against the run's own spread.
  resources  registers, LDS and scratch of the driver's kernels as built (tools/kernel_resources.py; needs no GPU).

Prints plain lines; profiles/offline_analyse.txt and profiles/offline_files.txt hold a run's output.
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
fx = importlib.import_module("feature-extractor_amd")
capi = fx.capi

C, S, STEP, RATE = 64, 1440000, 512, 48000
D = S // STEP                                   # 2812: S div D is 512 again
WINDOWS = (1024, 2048)
HBM_BYTES_PER_SECOND = 8e12


def timed(lib, h, call, reps):
    def once():
        capi.check(lib.fx_offline_sync(h))
        t0 = time.perf_counter()
        capi.check(call())
        capi.check(lib.fx_offline_sync(h))
        return time.perf_counter() - t0
    once()                                      # warm: tables and scratch made, kernels loaded
    return statistics.median(once() for _ in range(reps))


def rate(reps):
    import torch
    lib = capi.load_library(build_if_missing=False)
    assert S // D == STEP
    g = torch.Generator(device="cuda").manual_seed(9)
    audio = (torch.rand((C, S), generator=g, device="cuda") - 0.5) * 0.6
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    for N in WINDOWS:
        B = N // 2 + 1
        an = fx.offline.AudioAnalyser(C, RATE / 2.0)
        mags = torch.empty((D, C, B), dtype=torch.float32, device="cuda")
        energy = torch.empty((C, D), dtype=torch.float32, device="cuda")
        features = torch.empty((capi.OFFLINE_FEATURE_ROWS, C, D), dtype=torch.float32, device="cuda")
        lat = torch.empty((C,), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t = timed(lib, an._h, lambda: lib.fx_offline_frames(an._h, ptr(audio), S, D, N, ptr(mags), ptr(energy), capi.MEM_DEVICE), reps)
        moved = 4 * C * S + 4 * D * C * B
        print("frames:  C = %d, S = %d, D = %d (step %d), %d-pt: fx_offline_frames %.3f ms (median of %d): %.3g frames/s; %.1f MB of audio read + "
              "magnitudes written = %.2f TB/s, %.1f %% of 8 TB/s" % (C, S, D, STEP, N, t * 1e3, reps, D * C / t, moved / 1e6, moved / t / 1e12,
                                                                   100.0 * moved / t / HBM_BYTES_PER_SECOND), flush=True)
        everything = 63
        no_loop = everything & ~(capi.OFFLINE_DO_SPECTRAL | capi.OFFLINE_DO_HARMONIC)

        def analyse(what):
            def call():
                st = lib.fx_offline_analyse(an._h, ptr(audio), S, D, N, RATE, what, ptr(features), ptr(energy), ptr(lat), None, capi.MEM_DEVICE)
                return st
            return call
        whole = timed(lib, an._h, analyse(everything), max(3, reps // 3))
        rest = timed(lib, an._h, analyse(no_loop), max(3, reps // 3))
        print("analyse: C = %d, S = %d, D = %d, %d-pt, magnitudes through the scratch: fx_offline_analyse %.1f ms, of which %.1f ms without the "
              "per-frame analyses: the %d per-frame launches are %.1f %% of the call (%.1f us each)"
              % (C, S, D, N, whole * 1e3, rest * 1e3, 3 * D, 100.0 * (whole - rest) / whole, (whole - rest) / (3 * D) * 1e6), flush=True)
        an.close()
    print("the D x 3 per-frame launches are the known next limit of an analysis: they are serial in the frame through previousBinMagnitudes and "
          "previousF0.  The frame kernel is not.")


def files(reps):
    import numpy as np
    import torch
    lib = capi.load_library(build_if_missing=False)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731
    lengths = np.linspace(10 * RATE, 50 * RATE, C).astype(np.int64)                     # mean 30 s
    total = int(lengths.sum())
    lp = lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    rates = np.full(C, RATE, np.int32)
    rp = rates.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    g = torch.Generator(device="cuda").manual_seed(9)
    noise = (torch.rand((max(total, C * S),), generator=g, device="cuda") - 0.5) * 0.6
    f32 = noise[:total]
    banks = {"S16": (capi.SAMPLE_S16, (f32 * 32768.0).round().to(torch.int16)), "F32": (capi.SAMPLE_F32, f32)}
    for N in WINDOWS:
        B = N // 2 + 1
        an = fx.offline.AudioAnalyser(C, RATE / 2.0)
        mags = torch.empty((D, C, B), dtype=torch.float32, device="cuda")
        energy = torch.empty((C, D), dtype=torch.float32, device="cuda")
        features = torch.empty((capi.OFFLINE_FEATURE_ROWS, C, D), dtype=torch.float32, device="cuda")
        lat = torch.empty((C,), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for name, (fmt, bank) in banks.items():
            t = timed(lib, an._h, lambda: lib.fx_offline_analyse_files(an._h, ptr(bank), lp, fmt, D, N, None, 0, ptr(features), ptr(energy), None, ptr(mags),
                                                                       capi.MEM_DEVICE), reps)
            moved = bank.element_size() * total + 4 * D * C * B
            print("files frames:  C = %d files of %d .. %d samples (%s), D = %d, %d-pt: frame stage %.3f ms (median of %d): %.3g frames/s; %.1f MB of "
                  "samples read + magnitudes written = %.2f TB/s" % (C, lengths[0], lengths[-1], name, D, N, t * 1e3, reps, D * C / t, moved / 1e6,
                                                                     moved / t / 1e12), flush=True)
            whole = timed(lib, an._h, lambda: lib.fx_offline_analyse_files(an._h, ptr(bank), lp, fmt, D, N, rp, 63, ptr(features), ptr(energy), ptr(lat), None,
                                                                           capi.MEM_DEVICE), max(3, reps // 3))
            rest = timed(lib, an._h, lambda: lib.fx_offline_analyse_files(an._h, ptr(bank), lp, fmt, D, N, rp, 63 & ~3, ptr(features), ptr(energy), ptr(lat), None,
                                                                          capi.MEM_DEVICE), max(3, reps // 3))
            print("files analyse: the same library (%s), %d-pt, magnitudes through the scratch: fx_offline_analyse_files %.1f ms, of which %.1f ms without "
                  "the per-frame analyses: the %d per-frame launches are %.1f %% of the call" % (name, N, whole * 1e3, rest * 1e3, 3 * D,
                                                                                                 100.0 * (whole - rest) / whole), flush=True)
        # equal lengths: the files entry's frame stage against fx_offline_frames on the same audio, alternating
        audio = noise[:C * S]
        equal = np.full(C, S, np.int64)
        ep = equal.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
        calls = {"files": lambda: lib.fx_offline_analyse_files(an._h, ptr(audio), ep, capi.SAMPLE_F32, D, N, None, 0, ptr(features), ptr(energy), None, ptr(mags),
                                                               capi.MEM_DEVICE),
                 "frames": lambda: lib.fx_offline_frames(an._h, ptr(audio), S, D, N, ptr(mags), ptr(energy), capi.MEM_DEVICE)}
        times = {k: [] for k in calls}
        for k in calls:
            timed(lib, an._h, calls[k], 1)                                              # warm both first
        for _ in range(reps):
            for k in calls:
                capi.check(lib.fx_offline_sync(an._h))
                t0 = time.perf_counter()
                capi.check(calls[k]())
                capi.check(lib.fx_offline_sync(an._h))
                times[k].append(time.perf_counter() - t0)
        med = {k: statistics.median(v) for k, v in times.items()}
        print("equal lengths (C = %d, S = %d, D = %d, F32, %d-pt), alternating, %d each: files entry %.3f ms (%.3f .. %.3f), fx_offline_frames %.3f ms "
              "(%.3f .. %.3f): ratio of medians %.3f" % (C, S, D, N, reps, med["files"] * 1e3, min(times["files"]) * 1e3, max(times["files"]) * 1e3,
                                                         med["frames"] * 1e3, min(times["frames"]) * 1e3, max(times["frames"]) * 1e3,
                                                         med["files"] / med["frames"]), flush=True)
        an.close()
    print("a whole analysis is still its D x 3 serial per-frame launches, whatever the lengths: the files entry changes what the frame, crossing, "
          "RMS and attack kernels read, not that loop.")


def resources():
    import kernel_resources as kr
    fx.load_library(build_if_missing=True)
    print("the driver's kernels as built (VGPRs / SGPRs / scratch bytes per lane / static LDS bytes per workgroup):")
    mine = [k for k in kr.kernels_of() if k["pretty"].startswith("fxo::")]
    names = kr.demangle([k["name"] for k in mine])
    for k in mine:                                  # (kernels_of's short names end at the first bracket: these live in an unnamed namespace)
        name = names[k["name"]].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
        print("  %-40s %3d / %3d / %d / %d" % (name, k["vgpr"], k.get("sgpr", 0), k.get("scratch", 0), k.get("lds", 0)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["rate", "files", "resources"])
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    {"rate": lambda: rate(a.reps), "files": lambda: files(a.reps), "resources": resources}[a.part]()


if __name__ == "__main__":
    main()
