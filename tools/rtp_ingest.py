"""What fx_push_rtp costs on one MI355X (writes profiles/rtp_ingest_bench.txt).

Shape: 8192 tracks = 1024 streams x 8 channels, L24, 48-sample packets, ticks of n = 480: 10 240 datagrams of 1164 bytes a tick,
11.8 MB of payload in and 11.8 MB of planar samples out.  Three calls are timed the same way -- 16 ticks back to back on the
library's stream through the C ABI, every buffer preallocated on the device, one synchronisation per pass, the passes of the three
alternated, medians and spreads over the passes:
  rtp          fx_push_rtp of the tick's datagrams (device-resident slots)
  planar       fx_push_samples of the same planar block [8192][480] s24
  interleaved  fx_push_interleaved of [480][8192] s24: the nearest existing byte mover, the same bytes each way
What the unpack adds to a tick is rtp - planar and what the de-interleave adds is interleaved - planar (both run on the stream ahead
of the same analysis): differences of whole calls, host side included, not kernel times.  The de-interleave's device code is byte for byte the parent commit's (tools/kernel_resources.py --digests).

    python tools/rtp_ingest.py [--passes 15] [--out profiles/rtp_ingest_bench.txt]

The difference of two whole calls is not the time of the unpack's launches themselves.  Those come from a kernel trace, in a run of
its own (the trace slows the host side), read back by --kernels:

    rocprofv3 --kernel-trace -d DIR -o rtp -- python tools/rtp_ingest.py --passes 3 --out /dev/null
    python tools/rtp_ingest.py --kernels DIR/rtp_results.db        (appends to --out)
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


def kernels(db_path, out):
    """per-kernel medians of a traced run (rocprofv3's results database), and the span of a tick's unpack on the device"""
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, start, end from kernels order by start").fetchall()
    short = lambda name: name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("fxk::", "")
    by_name, spans = {}, []
    for i, (name, a, b) in enumerate(rows):
        by_name.setdefault(short(name), []).append((b - a) / 1000.0)
        if "fx_rtp_parse_kernel" in name:                 # a tick's unpack: from the owner table's fill to the end of the count
            k = next(j for j in range(i, len(rows)) if "fx_rtp_count_kernel" in rows[j][0])
            fills = [(rows[i - 1][2] - rows[i - 1][1]) / 1000.0]
            by_name.setdefault("owner table fill (the fill before each parse)", []).extend(fills)
            spans.append((rows[k][2] - rows[i - 1][1]) / 1000.0)
    lines = ["", "kernel trace of the same shape (python tools/rtp_ingest.py --kernels): us, median (min - max) of n dispatches"]
    for name in sorted(by_name):
        if "rtp" in name or "deinterleave" in name or "owner table" in name:
            v = by_name[name]
            lines.append("  %-50s %7.1f (%.1f - %.1f) of %d" % (name, statistics.median(v), min(v), max(v), len(v)))
    lines.append("  %-50s %7.1f (%.1f - %.1f) of %d" % ("a tick's unpack, fill start to count end", statistics.median(spans), min(spans), max(spans), len(spans)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(out, "a") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtp_ingest_bench.txt"))
    ap.add_argument("--kernels", default=None, help="a traced run's rocprofv3 results database: append its kernel times to --out")
    args = ap.parse_args()
    if args.kernels:
        kernels(args.kernels, args.out)
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
    stamps = np.array([int.from_bytes(bytes(slots[i, 4:8]), "big") for i in range(P)], np.int64)
    ticks = []
    for k in range(TICKS):
        s = slots.copy()
        s[:, 4:8] = np.frombuffer((stamps + k * N_TICK).astype(">u4").tobytes(), np.uint8).reshape(P, 4)
        ticks.append(torch.from_numpy(s).cuda())
    planar = torch.from_numpy(np.ascontiguousarray(fx.rtp.big_endian_bytes(x, 3)[:, :, ::-1]).reshape(C, 3 * N_TICK)).cuda()
    inter = torch.from_numpy(np.ascontiguousarray(fx.rtp.big_endian_bytes(x, 3)[:, :, ::-1].transpose(1, 0, 2)).reshape(N_TICK, 3 * C)).cuda()
    raw = torch.empty((C, 2, 12), dtype=torch.float32, device="cuda")
    sm = torch.empty((C, 2, 12), dtype=torch.float32, device="cuda")
    ip = ctypes.POINTER(ctypes.c_int)
    ln, so = lengths.ctypes.data_as(ip), stream_of.ctypes.data_as(ip)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    frames = ctypes.c_int(0)

    def analyser(rtp):
        an = fx.BatchAnalyser(C, WINDOW)
        if rtp:
            an.rtp_configure("l24", [PER] * STREAMS)
            an.set_rtp_sources(np.arange(C), np.arange(C) // PER, np.arange(C) % PER)
        return an

    ans = {"rtp": analyser(True), "planar": analyser(False), "interleaved": analyser(False)}

    def one_pass(name):
        an = ans[name]
        an.reset_state()
        if name == "rtp":
            an.set_rtp_timestamps(np.arange(STREAMS), 0)
        an.sync()
        t0 = time.perf_counter()
        for k in range(TICKS):
            if name == "rtp":
                st = lib.fx_push_rtp(an._h, vp(ticks[k]), ln, so, P, stride, N_TICK, capi.MEM_DEVICE, vp(raw), vp(sm), ctypes.byref(frames), None)
            elif name == "planar":
                st = lib.fx_push_samples(an._h, vp(planar), N_TICK, capi.SAMPLE_S24, capi.MEM_DEVICE, vp(raw), vp(sm), ctypes.byref(frames))
            else:
                st = lib.fx_push_interleaved(an._h, vp(inter), N_TICK, C, capi.SAMPLE_S24, capi.MEM_DEVICE, vp(raw), vp(sm), ctypes.byref(frames))
            capi.check(st)
        an.sync()
        return (time.perf_counter() - t0) / TICKS * 1e6

    torch.cuda.synchronize()
    # the unpack is right before it is timed: the block of the last tick of a pass is the planar block
    one_pass("rtp")
    assert ans["rtp"].rtp_block().tobytes() == planar.cpu().numpy().tobytes(), "the unpacked block is not the planar block"
    stats = ans["rtp"].rtp_stats()
    assert int(stats["samples_missing"].sum()) == 0 and int(stats["packets"].sum()) == P * TICKS
    for name in ans:                                    # warm-up
        one_pass(name)
    times = {name: [] for name in ans}
    for _ in range(args.passes):
        for name in ans:                                # alternated
            times[name].append(one_pass(name))
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["fx_push_rtp on one MI355X (tools/rtp_ingest.py): %d tracks = %d streams x %d channels, L24, %d-sample packets, n = %d:" % (C, STREAMS, PER, PACKET, N_TICK),
             "%d datagrams of %d bytes (slot stride %d) a tick; %d-point context; %d ticks back to back per pass on the library's stream, device" % (P, int(lengths[0]), stride, WINDOW, TICKS),
             "buffers, one synchronisation per pass, the three calls' passes alternated, %d passes each; us per tick, median (min - max):" % args.passes]
    for name in ("rtp", "planar", "interleaved"):
        lines.append("  %-12s %8.1f (%.1f - %.1f)" % (name, med[name], min(times[name]), max(times[name])))
    unpack = [a - b for a, b in zip(times["rtp"], times["planar"])]
    deint = [a - b for a, b in zip(times["interleaved"], times["planar"])]
    mu, md = statistics.median(unpack), statistics.median(deint)
    lines += ["  what the unpack adds (rtp - planar, pass by pass):              %8.1f (%.1f - %.1f)" % (mu, min(unpack), max(unpack)),
              "  what the de-interleave adds (interleaved - planar, pass by pass): %8.1f (%.1f - %.1f)" % (md, min(deint), max(deint)),
              "  ratio of the two: %.2f   whole tick rtp / planar: %.3f" % (mu / md if md > 0 else float("nan"), med["rtp"] / med["planar"])]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)
    for an in ans.values():
        an.close()


if __name__ == "__main__":
    main()
