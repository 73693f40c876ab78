"""What the onset event list costs per analysis call (include/fx.h, fx_enable_onset_events): the same device-resident call with the
list off and on, alternated in one process, for the live shapes (one hop x 8192 / 65 536 tracks) and a long call (512 frames x 1024
tracks).  Time: a host clock around `calls` back-to-back calls that ends in a synchronisation, best and median of `rounds` rounds.
The list is drained between rounds (outside the timed region), so it never overflows.

    python tools/onset_events_bench.py [--rounds 7] > profiles/onset_events_bench.txt"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import signals
    fx = importlib.import_module("feature-extractor_amd")
    N = 1024
    print("onset event list: cost per analysis call, list off / on alternated (tools/onset_events_bench.py), %s" % torch.cuda.get_device_name(0))
    for C, T, calls in [(8192, 1, 400), (65536, 1, 200), (1024, 512, 20)]:
        base = signals.bursts(256, max(T, 16), N)[:, :T]
        hops = torch.from_numpy(np.ascontiguousarray(np.tile(base, (C // 256, 1, 1)))).cuda()
        raw = torch.empty((C, T, 12), dtype=torch.float32, device="cuda")
        sm = torch.empty_like(raw)
        ans = {}
        for mode in ("off", "on"):
            an = fx.BatchAnalyser(C, N)
            an.set_onset_window_length(3)
            if mode == "on":
                an.enable_onset_events(1 << 24)
            ans[mode] = an
        times = {"off": [], "on": []}
        events = 0
        with torch.cuda.stream(ans["off"].torch_stream()):
            pass
        for r in range(args.rounds + 1):
            for mode in ("off", "on"):
                an = ans[mode]
                with torch.cuda.stream(an.torch_stream()):
                    an.sync()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        an.push_hops(hops, out_raw=raw, out_smoothed=sm)
                    an.sync()
                    dt = (time.perf_counter() - t0) / calls
                if r:                                   # round 0 warms up
                    times[mode].append(dt * 1e6)
                if mode == "on":
                    ev, lost = an.onset_events()
                    assert lost == 0
                    events = len(ev) / calls
        off, on = np.array(times["off"]), np.array(times["on"])
        print("  %6d tracks x %3d frames per call, %d calls x %d rounds: off best %.1f median %.1f us (spread %.1f .. %.1f); "
              "on best %.1f median %.1f us; list costs %.1f us per call at the median = %.1f %% of the call; %.0f events per call"
              % (C, T, calls, args.rounds, off.min(), np.median(off), off.min(), off.max(), on.min(), np.median(on),
                 np.median(on) - np.median(off), 100.0 * (np.median(on) - np.median(off)) / np.median(off), events))
        for an in ans.values():
            an.close()


if __name__ == "__main__":
    main()
