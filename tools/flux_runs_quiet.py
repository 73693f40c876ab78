"""On the GPU box: what frames that are NOT accepted (silence: magnitude sum <= 0.05) cost the 1024-point batch kernel at the bench shape.
The kernel that keeps the flux state by runs (csrc/fx_flux_runs.h) leaves such frames' flux open while nothing has been accepted in a run
and forms their spectra once more after it; this prints the frame-kernel time per step for the bench input with
    none      nothing silenced (the headline),
    one       one channel silent throughout,
    tenth     every tenth channel silent throughout,
    passage   every channel silent in frames 100 .. 299 (a passage that spans run starts, unit boundaries and whole runs),
    all       every channel silent throughout.
Usage: python3 tools/flux_runs_quiet.py [case ...]        (a library variant: FX_LIBRARY_OVERRIDE, as tools/ab_variants.sh)
One line per case: case, frames/s, frame-kernel ms per step (20 steps after 5 warm-up steps)."""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
fx = importlib.import_module("feature-extractor_amd")
N, C, T = 1024, 1024, 512
base = torch.from_numpy(fx.synth.frames(C, T, N)).cuda()
for case in (sys.argv[1:] or ["none", "one", "tenth", "passage", "all"]):
    frames = base.clone()
    if case == "one":
        frames[517] = 0.0
    elif case == "tenth":
        frames[::10] = 0.0
    elif case == "passage":
        frames[:, 100:300] = 0.0
    elif case == "all":
        frames[:] = 0.0
    elif case != "none":
        raise SystemExit("unknown case " + case)
    an = fx.BatchAnalyser(C, N)
    fps, ms = bench.time_steps(an, frames, None, None, 20, warmup=5)[:2]
    an.close()
    print("%-8s %.6g frames/s  frame kernel %.4f ms" % (case, fps, ms), flush=True)
