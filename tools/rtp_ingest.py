"""What fx_push_rtp costs on one MI355X (writes profiles/rtp_ingest_bench.txt; with --window or --parent, profiles/rtp_window_bench.txt).

Shape: 8192 tracks = 1024 streams x 8 channels, L24, 48-sample packets, ticks of n = 480: 10 240 datagrams of 1164 bytes a tick,
11.8 MB of payload in and 11.8 MB of planar samples out.  Three calls are timed the same way -- 16 ticks back to back on the
library's stream through the C ABI, every buffer preallocated on the device, one synchronisation per pass, the passes of the three
alternated, medians and spreads over the passes:
  rtp          fx_push_rtp of the tick's datagrams (device-resident slots)
  planar       fx_push_samples of the same planar block [8192][480] s24
  interleaved  fx_push_interleaved of [480][8192] s24: the nearest existing byte mover, the same bytes each way
What the unpack adds to a tick is rtp - planar and what the de-interleave adds is interleaved - planar (both run on the stream ahead
of the same analysis): differences of whole calls, host side included, not kernel times.

    python tools/rtp_ingest.py [--passes 15] [--out profiles/rtp_ingest_bench.txt]

The reorder window (fx_rtp_set_window).  --window W[,W..] adds, per W, the call
  rtp_wW       fx_push_rtp with a window of W sample times: the same datagrams, each delivered 0 .. W - 48 sample times ahead of its
               own sample time by a seeded draw (feature-extractor_amd/rtp.py, arrival_ticks / cut_into_ticks), so a tick's slots hold
               what arrived during it, part of it for later ticks; the pass's last block must be the planar block, nothing missing
(`interleaved` is then left out unless --parent is given), and --parent FILE adds, for `rtp`, `interleaved` and every `rtp_wW`,
  NAME_parent  the same call on the library FILE, a build of the parent commit, loaded beside this one: this build's median must lie
               inside that call's own spread over its passes, which is what the measurement resolves (one gate line per pair)
to the alternated passes.

    python tools/rtp_ingest.py --window 480,4800 --parent PARENT/libfx_hip.so [--out profiles/rtp_window_bench.txt]

The difference of two whole calls is not the time of the unpack's launches themselves.  Those come from a kernel trace, in a run of
its own (the trace slows the host side), read back by --kernels; --only NAME runs that one call alone:

    rocprofv3 --kernel-trace -d DIR -o rtp -- python tools/rtp_ingest.py --passes 3 --out /dev/null [--window 480 --only rtp_w480]
    python tools/rtp_ingest.py --kernels DIR/rtp_results.db [--label TEXT]       (appends to --out)
"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAMS, PER, N_TICK, PACKET, WINDOW, TICKS = 1024, 8, 480, 48, 1024, 16


def kernels(db_path, out, label):
    """per-kernel medians of a traced run (rocprofv3's results database), and the span of a tick's unpack on the device"""
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, start, end from kernels order by start").fetchall()
    short = lambda name: name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("fxk::", "")
    by_name, spans = {}, []
    for i, (name, a, b) in enumerate(rows):
        by_name.setdefault(short(name), []).append((b - a) / 1000.0)
        if "fx_rtp_parse" in name:                        # a tick's unpack: from the owner table's fill to the end of its last launch
            last = "fx_rtp_deposit_kernel" if "span" in name else "fx_rtp_count_kernel"
            k = next(j for j in range(i, len(rows)) if last in rows[j][0])
            fills = [(rows[i - 1][2] - rows[i - 1][1]) / 1000.0]
            by_name.setdefault("owner table fill (the fill before each parse)", []).extend(fills)
            spans.append((rows[k][2] - rows[i - 1][1]) / 1000.0)
    lines = ["", "kernel trace of %s (python tools/rtp_ingest.py --kernels): us, median (min - max) of n dispatches" % (label or "the same shape")]
    for name in sorted(by_name):
        if "rtp" in name or "deinterleave" in name or "owner table" in name:
            v = by_name[name]
            lines.append("  %-50s %7.1f (%.1f - %.1f) of %d" % (name, statistics.median(v), min(v), max(v), len(v)))
    if spans:                                             # (none in a trace of the interleaved call)
        lines.append("  %-50s %7.1f (%.1f - %.1f) of %d" % ("a tick's unpack, fill start to last launch's end", statistics.median(spans), min(spans), max(spans), len(spans)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(out, "a") as f:
        f.write(text)


def other_library(capi, path):
    """a second build of the library beside the package's own, with the prototypes of the entries it has"""
    lib = ctypes.CDLL(path)
    for name, argtypes, restype in capi.PROTOTYPES + capi.INTERNAL_PROTOTYPES:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argtypes, restype
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None, help="a traced run's rocprofv3 results database: append its kernel times to --out")
    ap.add_argument("--label", default=None, help="with --kernels: what the traced run was")
    ap.add_argument("--window", default="", help="reorder windows to time, sample times, comma-separated")
    ap.add_argument("--parent", default=None, help="a build of the parent commit's library: its rtp call joins the alternated passes")
    ap.add_argument("--only", default=None, help="run this one call alone (a traced run)")
    ap.add_argument("--seed", type=int, default=0, help="of the arrival schedule's draw")
    args = ap.parse_args()
    windows = [int(w) for w in args.window.split(",") if w]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "rtp_window_bench.txt" if windows or args.parent else "rtp_ingest_bench.txt")
    if args.kernels:
        kernels(args.kernels, args.out, args.label)
        return
    import torch
    fx = importlib.import_module("feature-extractor_amd")
    capi, lib = fx.capi, fx.load_library()
    C = STREAMS * PER
    rng = np.random.default_rng(0)
    x = rng.integers(-(1 << 21), 1 << 21, (C, N_TICK), dtype=np.int64)
    slots, lengths, stream_of = fx.rtp.packetise(x, [PER] * STREAMS, PACKET, 0)
    P, stride = slots.shape
    # the same datagrams for every tick of a pass, their timestamps moved on by n per tick
    stamps = fx.rtp.timestamps_of(slots)
    restamped = lambda k: np.frombuffer((stamps + k * N_TICK).astype(">u4").tobytes(), np.uint8).reshape(P, 4)
    ip = ctypes.POINTER(ctypes.c_int)
    paired = ["rtp"] + ([] if windows and not args.parent else ["interleaved"]) + ["rtp_w%d" % w for w in windows]
    base = lambda name: name[:-len("_parent")] if name.endswith("_parent") else name
    names = []
    for n in ["rtp", "planar"] + paired[1:]:
        names += [n, n + "_parent"] if args.parent and n in paired else [n]
    if args.only:
        if args.only not in names:
            raise SystemExit("--only: one of %s" % ", ".join(names))
        names = [args.only]
    called = {base(n) for n in names}
    ticks = {}                                            # per call: [(slots on the device, lengths, stream_of, P)] * TICKS
    if "rtp" in called:
        on_time = []
        for k in range(TICKS):
            s = slots.copy()
            s[:, 4:8] = restamped(k)
            on_time.append((torch.from_numpy(s).cuda(), lengths, stream_of, P))
        ticks["rtp"] = on_time
    for w in windows:
        if "rtp_w%d" % w not in called:
            continue
        # a pass's datagrams as one list, in time order, each submitted in the tick during which it arrives
        everything = np.concatenate([slots] * TICKS)
        everything[:, 4:8] = np.concatenate([restamped(k) for k in range(TICKS)])
        position = np.concatenate([stamps + k * N_TICK for k in range(TICKS)])
        ahead = np.random.default_rng(args.seed).integers(0, max(w - PACKET, 0) + 1, position.size)
        arrival = fx.rtp.arrival_ticks(position, ahead, N_TICK)
        cut = fx.rtp.cut_into_ticks(everything, np.tile(lengths, TICKS), np.tile(stream_of, TICKS), arrival, TICKS)
        ticks["rtp_w%d" % w] = [(torch.from_numpy(np.ascontiguousarray(s)).cuda(), np.ascontiguousarray(l), np.ascontiguousarray(o), len(l)) for s, l, o in cut]
        del everything
    planar = torch.from_numpy(np.ascontiguousarray(fx.rtp.big_endian_bytes(x, 3)[:, :, ::-1]).reshape(C, 3 * N_TICK)).cuda()
    inter = torch.from_numpy(np.ascontiguousarray(fx.rtp.big_endian_bytes(x, 3)[:, :, ::-1].transpose(1, 0, 2)).reshape(N_TICK, 3 * C)).cuda()
    raw = torch.empty((C, 2, 12), dtype=torch.float32, device="cuda")
    sm = torch.empty((C, 2, 12), dtype=torch.float32, device="cuda")
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    frames = ctypes.c_int(0)

    def analyser(name):
        """(the analyser, the library its calls go to)"""
        its = parent_lib if name.endswith("_parent") else lib
        kept, capi._lib = capi._lib, its                  # (a BatchAnalyser keeps the library it was made with)
        try:
            an = fx.BatchAnalyser(C, WINDOW)
        finally:
            capi._lib = kept
        if name.startswith("rtp"):
            an.rtp_configure("l24", [PER] * STREAMS)
            an.set_rtp_sources(np.arange(C), np.arange(C) // PER, np.arange(C) % PER)
            if name.startswith("rtp_w"):
                an.rtp_set_window(int(base(name)[5:]))
        return an, its

    parent_lib = other_library(capi, args.parent) if args.parent else None
    ans = {name: analyser(name) for name in names}

    def one_pass(name):
        an, its = ans[name]
        an.reset_state()
        if name.startswith("rtp"):
            an.set_rtp_timestamps(np.arange(STREAMS), 0)
        an.sync()
        t0 = time.perf_counter()
        for k in range(TICKS):
            if name.startswith("rtp"):
                d, ln, so, count = ticks[base(name)][k]
                st = its.fx_push_rtp(an._h, vp(d) if count else None, ln.ctypes.data_as(ip), so.ctypes.data_as(ip), count, stride, N_TICK, capi.MEM_DEVICE, vp(raw), vp(sm), ctypes.byref(frames), None)
            elif name == "planar":
                st = its.fx_push_samples(an._h, vp(planar), N_TICK, capi.SAMPLE_S24, capi.MEM_DEVICE, vp(raw), vp(sm), ctypes.byref(frames))
            else:
                st = its.fx_push_interleaved(an._h, vp(inter), N_TICK, C, capi.SAMPLE_S24, capi.MEM_DEVICE, vp(raw), vp(sm), ctypes.byref(frames))
            if st != capi.FX_OK:
                raise capi.FxError(st, its.fx_last_error().decode(errors="replace"))
        an.sync()
        return (time.perf_counter() - t0) / TICKS * 1e6

    torch.cuda.synchronize()
    # the unpack is right before it is timed: the block of the last tick of a pass is the planar block, and nothing is missing
    notes = []
    for name in names:
        if not name.startswith("rtp"):
            continue
        one_pass(name)
        an = ans[name][0]
        assert an.rtp_block().tobytes() == planar.cpu().numpy().tobytes(), "%s: the unpacked block is not the planar block" % name
        stats = an.rtp_stats()
        assert int(stats["samples_missing"].sum()) == 0 and int(stats["packets"].sum()) == P * TICKS, name
        if name.startswith("rtp_w"):
            w = an.rtp_window()
            counts = [t[3] for t in ticks[base(name)]]
            assert int(w["held"].sum()) == 0 and int(w["recovered"].sum()) > 0
            if name == base(name):
                notes.append("  %s: datagrams per tick %d .. %d (first %d, last %d); %.1f %% of a pass's positions came out of the held state"
                         % (name, min(counts), max(counts), counts[0], counts[-1], 100.0 * int(w["recovered"].sum()) / (STREAMS * N_TICK * TICKS)))
    for name in names:                                    # warm-up
        one_pass(name)
    times = {name: [] for name in names}
    for _ in range(args.passes):
        for name in names:                                # alternated
            times[name].append(one_pass(name))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["fx_push_rtp on one MI355X (tools/rtp_ingest.py): %d tracks = %d streams x %d channels, L24, %d-sample packets, n = %d:" % (C, STREAMS, PER, PACKET, N_TICK),
             "%d datagrams of %d bytes (slot stride %d) a tick; %d-point context; %d ticks back to back per pass on the library's stream, device" % (P, int(lengths[0]), stride, WINDOW, TICKS),
             "buffers, one synchronisation per pass, the calls' passes alternated, %d passes each; us per tick, median (min - max):" % args.passes]
    for name in names:
        lines.append("  %-16s %8.1f (%.1f - %.1f)" % (name, med[name], min(times[name]), max(times[name])))
    pairs = [("what the unpack adds (rtp - planar, pass by pass):", "rtp", "planar"),
             ("what the de-interleave adds (interleaved - planar, pass by pass):", "interleaved", "planar")]
    pairs += [("what a window of %d adds (rtp_w%d - rtp, pass by pass):" % (w, w), "rtp_w%d" % w, "rtp") for w in windows]
    pairs += [("this build less the parent's (%s - %s_parent, pass by pass):" % (n, n), n, n + "_parent") for n in paired]
    diff = {}
    for what, a, b in pairs:
        if a in times and b in times:
            d = [u - v for u, v in zip(times[a], times[b])]
            diff[(a, b)] = statistics.median(d)
            lines.append("  %-66s %8.1f (%.1f - %.1f)" % (what, diff[(a, b)], min(d), max(d)))
    if ("interleaved", "planar") in diff and diff[("interleaved", "planar")] > 0:
        lines.append("  ratio of the two: %.2f   whole tick rtp / planar: %.3f" % (diff[("rtp", "planar")] / diff[("interleaved", "planar")], med["rtp"] / med["planar"]))
    for n in paired:                                      # the gate: the parent's own spread over its passes is what this measurement resolves
        if n in times and n + "_parent" in times:
            lo, hi = min(times[n + "_parent"]), max(times[n + "_parent"])
            lines.append("  %s gate: this build's %s median %.1f %s the parent's own spread %.1f - %.1f" % ("W = 0" if n == "rtp" else n, n, med[n], "lies inside" if lo <= med[n] <= hi else "lies OUTSIDE (%s)" % ("below" if med[n] < lo else "above"), lo, hi))
    lines += notes
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)
    for an, _ in ans.values():
        an.close()


if __name__ == "__main__":
    main()
