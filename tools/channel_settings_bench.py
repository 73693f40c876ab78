"""What per-track settings cost: the bench shapes (1024 channels x 512 frames x 1024 points as fx_process_frames and as fx_push_hops, and one
hop per call at 8192 tracks) on a context where no per-track setter was called and on one where every track has its own gain, onset
sensitivity, window (1 .. 32) and type, alternating in one process; device-resident input, each figure the median / min / max of REPS
timed regions.  One JSON line per shape.  Results: profiles/channel_settings_bench.txt.

    python tools/channel_settings_bench.py"""
import importlib, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
fx = importlib.import_module("feature-extractor_amd")
fx.load_library(build_if_missing=False)
REPS = 7


def settings(an, C):
    rng = np.random.default_rng(3)
    an.set_channel_gains(rng.uniform(0.25, 2.0, C).astype(np.float32))
    an.set_channel_onset(rng.uniform(0.0, 1.0, C).astype(np.float32), rng.integers(1, 33, C).astype(np.int32), rng.integers(0, 3, C).astype(np.int32))


def timed(call, an, steps, warmup):
    for _ in range(warmup):
        call()
    an.sync()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(steps):
            call()
        an.sync()
        out.append((time.perf_counter() - t0) / steps)
    return out


def shape(name, C, N, T, entry, steps, warmup):
    x = torch.from_numpy(fx.synth.frames(C, T, N) if entry == "frames" else fx.synth.hops(C, T, N)).cuda()
    raw = torch.empty((C, T, 12), dtype=torch.float32, device=x.device)
    sm = torch.empty_like(raw)
    res = {}
    for mode in ("plain", "per_track", "plain_again", "per_track_again"):
        an = fx.BatchAnalyser(C, N, device=0)
        if mode.startswith("per_track"):
            settings(an, C)
        fn = an.process_frames if entry == "frames" else an.push_hops
        t = timed(lambda: fn(x, out_raw=raw, out_smoothed=sm), an, steps, warmup)
        an.close()
        res[mode] = {"median_us": round(1e6 * float(np.median(t)), 2), "min_us": round(1e6 * min(t), 2), "max_us": round(1e6 * max(t), 2),
                     "frames_per_s_median": round(C * T / float(np.median(t)), 0)}
    print(json.dumps({"shape": name, "C": C, "N": N, "T": T, "entry": entry, "steps": steps, **res}), flush=True)


shape("headline (fx_process_frames)", 1024, 1024, 512, "frames", 20, 3)
shape("headline as hops (fx_push_hops: the gain is applied)", 1024, 1024, 512, "hops", 20, 3)
shape("one hop per call, 8192 tracks", 8192, 1024, 1, "hops", 300, 30)
