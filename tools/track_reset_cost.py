"""What the per-track reset costs (profiles/NOTEBOOK.md, "Per-track reset and clear").

  --mode hop     one-hop cadence on a context WITH a per-track table: 8192 tracks x 2048-point window fed 480-sample device blocks
                 through fx_push_samples; a timed region is 32 calls (15 hops), each figure the median / min / max of REPS regions, in us
                 per call.  --package-root names the tree whose package and library run (this tree by default), so that a driver can
                 alternate this change and its parent commit, one fresh process each.
  --mode ab      the driver of that comparison: --parent-root names a checkout of the parent commit with its library built
                 (`git worktree add DIR HEAD~1`, then `python -c "import importlib; importlib.import_module('feature-extractor_amd.build').build()"`
                 in DIR); runs --mode hop ROUNDS times for the parent and for this tree, alternated, one fresh child process each, and
                 prints the children's lines and one summary line (medians of the medians, the parent's spread).
  --mode reset   wall time of fx_reset_channels (the call synchronises) for 1 and for 1024 of 8192 tracks on an idle context; the
                 kernel's own time comes from running this mode under a kernel trace.

One JSON line per figure."""
import argparse, importlib, json, os, sys, time
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["hop", "reset", "ab"], required=True)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
args = ap.parse_args()
if args.mode == "ab":
    import subprocess
    if not args.parent_root:
        ap.error("--mode ab needs --parent-root")
    got = {"parent": [], "this": []}
    for _ in range(args.rounds):
        for label, root in (("parent", os.path.abspath(args.parent_root)), ("this", args.package_root)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", "hop", "--package-root", root, "--label", label],
                                 capture_output=True, text=True, timeout=300)
            if out.returncode != 0:                 # nothing more is started after a child that failed
                sys.exit("child (%s) failed with %d:\n%s" % (label, out.returncode, out.stderr[-2000:]))
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            got[label].append(json.loads(line)["median_us"])
    p, t = got["parent"], got["this"]
    print(json.dumps({"mode": "ab", "rounds": args.rounds, "parent_median_us": float(np.median(p)), "parent_min_us": min(p), "parent_max_us": max(p),
                      "this_median_us": float(np.median(t)), "this_min_us": min(t), "this_max_us": max(t),
                      "difference_us": round(float(np.median(t) - np.median(p)), 2), "parent_spread_us": round(max(p) - min(p), 2)}), flush=True)
    sys.exit(0)
sys.path.insert(0, args.package_root)
import torch
fx = importlib.import_module("feature-extractor_amd")
fx.load_library(build_if_missing=False)
C, N, REPS = 8192, 2048, 9


def table(an):
    rng = np.random.default_rng(3)
    an.set_channel_gains(rng.uniform(0.25, 2.0, C).astype(np.float32))
    an.set_channel_onset(rng.uniform(0.0, 1.0, C).astype(np.float32), rng.integers(1, 33, C).astype(np.int32), rng.integers(0, 3, C).astype(np.int32))


if args.mode == "hop":
    an = fx.BatchAnalyser(C, N, device=0)
    table(an)
    x = torch.from_numpy(np.random.default_rng(1).normal(0, 0.3, (C, 480)).astype(np.float32)).cuda()
    region = 32

    def calls(n):
        for _ in range(n):
            an.push_samples(x, want_raw=True, want_smoothed=True)

    calls(4 * region)
    an.sync()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        calls(region)
        an.sync()
        t.append(1e6 * (time.perf_counter() - t0) / region)
    an.close()
    print(json.dumps({"mode": "hop", "label": args.label, "C": C, "N": N, "block": 480, "calls_per_region": region,
                      "median_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}), flush=True)
else:
    an = fx.BatchAnalyser(C, N, device=0)
    table(an)
    hops = torch.zeros((C, 4, N // 2), dtype=torch.float32, device="cuda")
    an.push_hops(hops)
    an.sync()
    for n in (1, 1024):
        tracks = np.random.default_rng(n).choice(C, n, replace=False).astype(np.int32)
        for _ in range(5):
            an.reset_channels(tracks)
        t = []
        for _ in range(51):
            an.sync()
            t0 = time.perf_counter()
            an.reset_channels(tracks)
            an.sync()
            t.append(1e6 * (time.perf_counter() - t0))
        print(json.dumps({"mode": "reset", "tracks": n, "of": C, "N": N, "calls": len(t), "median_us": round(float(np.median(t)), 1),
                          "min_us": round(min(t), 1), "max_us": round(max(t), 1)}), flush=True)
    an.close()
