"""What the audio display costs (include/fx.h, fx_enable_display), three measurements of one session:

(a) per call: one 480-sample fx_push_samples call (device blocks, N = 1024, 480 samples per display block, 1024 levels) at 1024 and
    8192 channels, a context with the display against a twin without, alternated in one process; a host clock around `calls`
    back-to-back calls that ends in a synchronisation; medians of `rounds` rounds.
(b) long call: 1024 channels x 512 hops through fx_push_hops, device events around the call (queued behind a fill, so the events
    bracket device work), display on minus display off = the display launch; its algorithmic bytes (the samples + 8 B per
    publication + 32 B of state per track) over that time, against fx_reblock_kernel's rate measured the same way in the same
    process (tools/reblock_rate.py's shape: 65 536 channels x 511 samples that complete no hop; bytes read + written).
(c) --parent DIR: the headline `python bench.py --gpus 1 --steps 50 --warmup 10` of this tree and of the parent commit's tree at
    DIR (built beforehand), alternated, display never enabled.

    python tools/display_bench.py [--rounds 7] [--parent DIR] > profiles/display_bench.txt"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, SPB, LENGTH = 1024, 480, 1024


def per_call(fx, torch, rounds):
    print("(a) one 480-sample fx_push_samples call, display off / on alternated, us per call (host clock, synchronised)")
    for C, calls in ((1024, 800), (8192, 400)):
        block = (torch.rand((C, 480), device="cuda") - 0.5).contiguous()
        ans = {}
        for mode in ("off", "on"):
            an = fx.BatchAnalyser(C, N)
            if mode == "on":
                an.enable_display(SPB, LENGTH)
            ans[mode] = an
        times = {"off": [], "on": []}
        for r in range(rounds + 1):
            for mode in ("off", "on"):
                an = ans[mode]
                with torch.cuda.stream(an.torch_stream()):
                    an.reset_state()
                    an.sync()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        an.push_samples(block, want_raw=False)
                    an.sync()
                    dt = (time.perf_counter() - t0) / calls
                if r:                                   # round 0 warms up
                    times[mode].append(dt * 1e6)
        off, on = np.array(times["off"]), np.array(times["on"])
        print("  %5d channels, %d calls x %d rounds: off median %.1f us (%.1f .. %.1f); on median %.1f us (%.1f .. %.1f); "
              "the display costs %.1f us per call at the median = %.1f %% of the call"
              % (C, calls, rounds, np.median(off), off.min(), off.max(), np.median(on), on.min(), on.max(),
                 np.median(on) - np.median(off), 100.0 * (np.median(on) - np.median(off)) / np.median(off)), flush=True)
        for an in ans.values():
            an.close()


def device_ms(torch, an, busy, call):
    lib = an.torch_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    busy.zero_()
    e0.record(lib)
    call()
    e1.record(lib)
    an.sync()
    return e0.elapsed_time(e1)


def long_call(fx, torch, rounds):
    print("(b) 1024 channels x 512 hops in one fx_push_hops call, device events; fx_reblock_kernel as the yardstick")
    C, T, H = 1024, 512, N // 2
    hops = (torch.rand((C, T, H), device="cuda") - 0.5).contiguous()
    raw = torch.empty((C, T, 12), dtype=torch.float32, device="cuda")
    sm = torch.empty_like(raw)
    busy = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    ans = {}
    for mode in ("off", "on"):
        an = fx.BatchAnalyser(C, N)
        if mode == "on":
            an.enable_display(SPB, LENGTH)
        ans[mode] = an
    times = {"off": [], "on": []}
    for r in range(rounds + 1):
        for mode in ("off", "on"):
            an = ans[mode]
            with torch.cuda.stream(an.torch_stream()):
                ms = device_ms(torch, an, busy, lambda: an.push_hops(hops, out_raw=raw, out_smoothed=sm))
            if r:
                times[mode].append(ms)
    for an in ans.values():
        an.close()
    off, on = np.median(times["off"]), np.median(times["on"])
    samples = C * T * H
    moved = samples * 4 + 8 * C * (samples // C // SPB + 1) + 32 * C
    display_rate = moved / ((on - off) / 1e3)
    print("  call with the display off median %.3f ms (%.3f .. %.3f), on %.3f ms (%.3f .. %.3f): the display launch %.1f us"
          % (off, min(times["off"]), max(times["off"]), on, min(times["on"]), max(times["on"]), (on - off) * 1e3))
    print("  fx_display_kernel: %.1f MB (samples + publications + state) in %.1f us = %.2f TB/s" % (moved / 1e6, (on - off) * 1e3, display_rate / 1e12))
    # the yardstick: fx_reblock_kernel moving blocks that complete no hop
    Cr, n = 65536, 511
    an = fx.BatchAnalyser(Cr, N)
    x = torch.rand((Cr, n), device="cuda")
    best = []
    with torch.cuda.stream(an.torch_stream()):
        for r in range(rounds + 1):
            an.reset_state()
            ms = device_ms(torch, an, busy, lambda: an.push_samples(x, want_raw=False, want_smoothed=False))
            assert [l["kind"] for l in an.last_launches()] == ["reblock"]
            if r:
                best.append(ms)
    an.close()
    reblock_moved = 2 * x.numel() * 4
    reblock_rate = reblock_moved / (np.median(best) / 1e3)
    print("  fx_reblock_kernel: %.1f MB (read + written) in %.1f us median (%.1f .. %.1f) = %.2f TB/s"
          % (reblock_moved / 1e6, np.median(best) * 1e3, min(best) * 1e3, max(best) * 1e3, reblock_rate / 1e12))
    print("  ratio fx_display_kernel / fx_reblock_kernel: %.2f" % (display_rate / reblock_rate), flush=True)


def headline(parent, repeats):
    print("(c) display never enabled: `python bench.py --gpus 1 --steps 50 --warmup 10`, parent commit and this tree alternated, frames/s")
    values = {"parent": [], "this": []}
    for r in range(repeats):
        for name, cwd in (("parent", parent), ("this", ROOT)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=cwd,
                                 capture_output=True, text=True, check=True).stdout
            value = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"]
            values[name].append(value)
            print("    %-6s run %d  %.4e" % (name, r + 1, value), flush=True)
    p, t = np.array(values["parent"]), np.array(values["this"])
    spread = 100.0 * (p.max() - p.min()) / p.mean()
    diff = 100.0 * (t.mean() - p.mean()) / p.mean()
    print("  parent %.4e .. %.4e (spread %.2f %%), this tree %.4e .. %.4e; means differ by %+.2f %%: %s the parent's own spread"
          % (p.min(), p.max(), spread, t.min(), t.max(), diff, "inside" if abs(diff) <= spread else "OUTSIDE"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: run (c)")
    ap.add_argument("--repeats", type=int, default=4)
    args = ap.parse_args()
    import torch
    fx = importlib.import_module("feature-extractor_amd")
    print("audio display levels: what they cost (tools/display_bench.py), %s" % torch.cuda.get_device_name(0))
    per_call(fx, torch, args.rounds)
    long_call(fx, torch, args.rounds)
    if args.parent:
        headline(os.path.abspath(args.parent), args.repeats)


if __name__ == "__main__":
    main()
