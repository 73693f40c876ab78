"""What moving tracks costs ("fx_pack_tracks_kernel"): 8192 of 65 536 tracks at 1024 points exported to and
imported from a DEVICE buffer (fx_export_channels / fx_import_channels: the calls synchronise, so a host clock around them is the
call's whole time -- the header work on the host, the entry list's upload, the one launch), and in the same run a device-to-device
copy of the same number of bytes timed the same way, which is the yardstick fx_reblock_kernel is held to.  Calls alternate, so the three
see the same machine.  Sets no threshold.  Writes the figures to --out (profiles/track_state_bench.txt) and prints one JSON line.

The kernels' own times come from running this tool under a kernel trace (rocprofv3 --kernel-trace --stats -- python
tools/track_state_rate.py --reps 20 --out <file>): fx_pack_tracks_kernel, fx_unpack_tracks_kernel and the runtime's copy kernel."""
import argparse, importlib, json, os, sys, time
import numpy as np

# what a call is besides its kernel: written into the file whenever a call takes more than twice the copy (the kernels' own times,
# from a kernel trace of this tool, are kept apart in profiles/track_state_kernels.txt: this tool rewrites only its own file)
WHY = """
why a call is more than twice the copy: the kernel is a small part of it (profiles/track_state_kernels.txt: within 1.4 x of the
runtime's copy kernel).  The rest is the host's and the waits.  Both calls synchronise the context's stream before and after, as the
per-track setters do (the contract: the buffer is valid on return, a ring's batches in flight come first); the export writes one
header per track into the pinned entry list (96 B each) and uploads it; the import first fetches the headers back in one strided
copy on the context's stream (80 B out of every record) and waits for it, checks each, then puts ALL rows of the per-track table
in force through the setters' staged upload (32 B x every track of the context: the host mirror and the device table stay equal),
then the list.  Draining a shard is not on the audio path; nothing here was tuned beyond reading the rows in place.
"""

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--channels", type=int, default=65536)
ap.add_argument("--tracks", type=int, default=8192)
ap.add_argument("--window", type=int, default=1024)
ap.add_argument("--reps", type=int, default=101)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_state_bench.txt"))
args = ap.parse_args()
sys.path.insert(0, ROOT)
import torch
fx = importlib.import_module("feature-extractor_amd")
fx.load_library(build_if_missing=False)
C, K, N = args.channels, args.tracks, args.window

an = fx.BatchAnalyser(C, N, device=0)
rng = np.random.default_rng(7)
an.set_channel_gains(rng.uniform(0.25, 2.0, C).astype(np.float32))
gen = torch.Generator(device="cuda").manual_seed(7)
for _ in range(2):                                  # two calls of two hops: tails, flux rows and three ring rows hold values
    an.push_hops(torch.randn((C, 2, N // 2), dtype=torch.float32, device="cuda", generator=gen) * 0.3)
an.sync()
tracks = np.sort(rng.choice(C, K, replace=False)).astype(np.int32)
size = an.track_state_bytes()
nbytes = K * size
state = an.export_tracks(tracks, device=True)
other = torch.empty_like(state)
assert state.numel() == nbytes
lib, h = an._lib, an._h
import ctypes
lst = tracks.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
ptr = ctypes.c_void_p(state.data_ptr())


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0)


def export():
    fx.capi.check(lib.fx_export_channels(h, lst, K, ptr, nbytes, fx.capi.MEM_DEVICE))


def imports():
    fx.capi.check(lib.fx_import_channels(h, lst, K, ptr, nbytes, fx.capi.MEM_DEVICE))


def copy():
    other.copy_(state)


calls = {"export": export, "import": imports, "d2d_copy": copy}
for _ in range(5):
    for f in calls.values():
        timed(f)
t = {k: [] for k in calls}
for _ in range(args.reps):
    for k, f in calls.items():
        t[k].append(timed(f))
assert torch.equal(an.export_tracks(tracks, device=True), state)      # the imports put back what the exports took
an.close()

res = {"channels": C, "tracks": K, "window": N, "record_bytes": size, "bytes": nbytes, "reps": args.reps}
for k, v in t.items():
    med = float(np.median(v))
    res[k] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
              "GBps_read_plus_write": round(2 * nbytes / (med * 1e-6) / 1e9, 1)}
res["export_over_copy"] = round(res["export"]["median_us"] / res["d2d_copy"]["median_us"], 2)
res["import_over_copy"] = round(res["import"]["median_us"] / res["d2d_copy"]["median_us"], 2)
lines = ["track_state_rate.py: %d of %d tracks at %d points, records of %d B = %.1f MB through a device buffer; %d alternated calls each,"
         % (K, C, N, size, nbytes / 1e6, args.reps),
         "host clock around a call that ends in a synchronise (the WHOLE call: host header work, list upload, launch, wait)", ""]
for k in calls:
    r = res[k]
    lines.append("%-9s median %8.1f us  (min %8.1f, max %8.1f)   %7.1f GB/s read + written" % (k, r["median_us"], r["min_us"], r["max_us"], r["GBps_read_plus_write"]))
lines += ["", "export / copy = %.2f, import / copy = %.2f" % (res["export_over_copy"], res["import_over_copy"])]
if res["export_over_copy"] > 2.0 or res["import_over_copy"] > 2.0:
    lines += ["", WHY.strip()]
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
print(json.dumps(res), flush=True)
