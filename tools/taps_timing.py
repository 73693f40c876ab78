"""On the GPU box: what arming analysis taps costs one call (include/fx.h, fx_request_taps).  One hop per call from device memory,
the same stream armed and unarmed, calls interleaved in rounds; an armed call re-arms K channels before it (the taps launch and its
capture), an unarmed one does not.  Prints the median wall time per call of each, and of the taps kernel alone (fx_get_taps not
included: it synchronises).
Usage: python3 tools/taps_timing.py [N C K] ...   (default: 2048 1024 8, 4096 1024 8)"""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

fx = importlib.import_module("feature-extractor_amd")


def per_call_us(an, hops, arm, calls=200):
    r = torch.empty((an.num_channels, 1, 12), dtype=torch.float32, device="cuda")
    s = torch.empty_like(r)
    an.sync()
    t0 = time.perf_counter()
    for i in range(calls):
        if arm is not None:
            an.request_taps(arm)
        an.push_hops(hops[i % len(hops)], out_raw=r, out_smoothed=s)
    an.sync()
    return (time.perf_counter() - t0) / calls * 1e6


def main(configs):
    for N, C, K in configs:
        an = fx.BatchAnalyser(C, N)
        hops = [torch.from_numpy(np.ascontiguousarray(fx.synth.hops(C, 1, N, first_hop=k))).cuda() for k in range(4)]
        arm = list(np.linspace(0, C - 1, K).astype(int))
        for _ in range(2):                                   # warm-up: allocations, code objects
            per_call_us(an, hops, arm, 20), per_call_us(an, hops, None, 20)
        plain, armed = [], []
        for _ in range(7):
            plain.append(per_call_us(an, hops, None))
            armed.append(per_call_us(an, hops, arm))
        assert an.last_launches()[0]["kind"] == "taps"
        an.close()
        p, a = float(np.median(plain)), float(np.median(armed))
        print("N=%d C=%d armed=%d: unarmed %.1f us/call, armed %.1f us/call, difference %.1f us (rounds: %s | %s)"
              % (N, C, K, p, a, a - p, " ".join("%.1f" % v for v in plain), " ".join("%.1f" % v for v in armed)))


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    main([tuple(args[i:i + 3]) for i in range(0, len(args), 3)] if args else [(2048, 1024, 8), (4096, 1024, 8)])
