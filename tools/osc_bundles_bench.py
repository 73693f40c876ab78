"""What OSC bundles cost and buy (include/fx.h, fx_get_osc_bundles / fx_osc_encode_bundles / FX_OSC_RECEIVER_BUNDLES).

(a) fx_get_osc_bundles at 1472 bytes to page-locked host memory against fx_get_osc_datagrams (fx_osc.hip, which this change does not
    touch: the parent commit's call) on the SAME context, the two alternated call by call in one process; 1024 / 8192 / 65 536 tracks;
    a host clock around one call, which ends in a synchronisation (FX_MEM_HOST); the median of `calls` calls each after a warm-up.  The
    bundles are at most (4 + 80) / 80 + 16 / 1444 = 1.06 x the bytes and both calls are launch-and-copy bound; a ratio above 1.2 at
    65 536 tracks is flagged and wants an explanation in profiles/NOTEBOOK.md.  Needs a GPU.
(b) the batch sender over loopback, 65 536 tracks, 60 Hz timer, WITHOUT segmented sends, one target and two: plain messages against
    bundles of 1472 bytes.  Datagrams and system calls per tick, late ticks, longest tick.  The one condition: a tick of bundles is
    exactly num_bundles x targets datagrams.  Needs no GPU.

    python tools/osc_bundles_bench.py [--sender-only] [--seconds 5] --write profiles/osc_bundles_bench.txt"""
import argparse
import ctypes
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

TRACKS = 65536
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def device_calls(fx, calls):
    import torch
    import signals
    lib = fx.load_library()
    capi = fx.capi
    N = 1024
    ip = ctypes.POINTER(ctypes.c_int)
    say("(a) fx_get_osc_bundles (1472 bytes) against fx_get_osc_datagrams on one context, alternated; to page-locked host memory; median of %d calls each; %s"
        % (calls, torch.cuda.get_device_name(0)))
    for C in (1024, 8192, 65536):
        an = fx.BatchAnalyser(C, N)
        base = signals.tone_vibrato_noise(256, 2, N, seed=5)
        an.push_hops(torch.from_numpy(np.ascontiguousarray(np.tile(base, (C // 256, 1, 1)))).cuda())
        an.sync()
        latest = an.get_features()
        plain_stride = capi.osc_stride("/Audio/A", 0, C)
        K, bundles, stride = capi.osc_bundle_plan(plain_stride, C, 1472)
        nbytes = max(C * plain_stride, bundles * stride)
        buf = ctypes.c_void_p()
        capi.check(lib.fx_host_alloc(ctypes.byref(buf), nbytes))
        host = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(nbytes,))
        plain_n, bundle_n = np.empty(C, np.int32), np.empty(bundles, np.int32)

        def plain_call():
            return lib.fx_get_osc_datagrams(an._h, b"/Audio/A", 0, buf, plain_stride, plain_n.ctypes.data_as(ip), capi.MEM_HOST)

        def bundle_call():
            return lib.fx_get_osc_bundles(an._h, b"/Audio/A", 0, 1, 1472, buf, stride, bundle_n.ctypes.data_as(ip), capi.MEM_HOST)

        capi.check(bundle_call())                           # the bytes first: the host encoder's, bitwise
        want, _ = capi.osc_encode_bundles("/Audio/A", 0, latest, 1, 1472)
        assert np.array_equal(host[:bundles * stride].reshape(bundles, stride), want), "the device's bundles are not the host encoder's"
        t = {"plain": [], "bundles": []}
        for k in range(calls + 10):
            for name, fn in (("plain", plain_call), ("bundles", bundle_call)):
                t0 = time.perf_counter()
                st = fn()
                dt = (time.perf_counter() - t0) * 1e6
                assert st == 0
                if k >= 10:                                 # ten warm-up calls of each
                    t[name].append(dt)
        p, b = float(np.median(t["plain"])), float(np.median(t["bundles"]))
        flag = "  ABOVE 1.2 x: see profiles/NOTEBOOK.md" if C == 65536 and b > 1.2 * p else ""
        say("  %6d tracks: datagrams %8d bytes, median %7.1f us (best %.1f); bundles K %d, %d x %d = %8d bytes (%.3f x), median %7.1f us (best %.1f); ratio %.2f%s"
            % (C, C * plain_stride, p, min(t["plain"]), K, bundles, stride, bundles * stride, bundles * stride / (C * plain_stride), b, min(t["bundles"]), b / p, flag))
        capi.check(lib.fx_host_free(buf))
        an.close()


def sender(fx, seconds, threads):
    capi = fx.capi
    C = TRACKS
    v = np.random.default_rng(1).standard_normal((C, 12)).astype(np.float32)
    forms = {"plain": capi.osc_encode_batch("/Audio/A", 0, v), "bundles": capi.osc_encode_bundles("/Audio/A", 0, v, 1, 1472)}
    say("(b) batch sender over loopback, %d tracks, 60 Hz timer for %.0f s, %d sender threads, NO segmented sends, receivers without UDP_GRO (host only, %d CPUs)"
        % (C, seconds, threads, os.cpu_count() or 0))
    ok = True
    for targets in (1, 2):
        for form in ("plain", "bundles"):
            d, n = forms[form]
            rx = [capi.OscReceiver("127.0.0.1:0", threads=2, gro=False, bundles=True) for _ in range(targets)]
            ports = ["127.0.0.1:%d" % r.port for r in rx]
            tx = capi.OscSender(ports[0], ports[1] if targets == 2 else None, threads=threads, gso=False)
            tx.update(d, n)
            one = tx.send()                                 # one tick by hand: its datagrams exactly
            base = tx.stats()
            tx.start(60.0)
            time.sleep(seconds)
            tx.stop()
            st = tx.stats()
            time.sleep(0.3)
            got = sum(r.stats()["datagrams"] for r in rx)
            elements = sum(r.bundle_stats()["elements"] for r in rx)
            ticks = st["ticks"] - base["ticks"]
            per_tick = (st["datagrams"] + st["dropped"] - base["datagrams"] - base["dropped"]) / max(ticks, 1)
            calls = (st["syscalls"] - base["syscalls"]) / max(ticks, 1)
            exact = one + base["dropped"] == d.shape[0] * targets and per_tick == d.shape[0] * targets
            ok = ok and (form == "plain" or exact)
            say("  %d target%s, %-8s %6d datagrams per tick (%s%d x %d), %7.1f system calls per tick; ticks %d, late %d, longest tick %.2f ms, mean %.2f ms; "
                "dropped by the sender %d; received %d of %d datagrams%s"
                % (targets, " " if targets == 1 else "s", form + ":", per_tick, "" if exact else "NOT ", d.shape[0], targets, calls, ticks, st["late_ticks"], st["max_tick_ms"],
                   (st["total_tick_ms"] - base["total_tick_ms"]) / max(ticks, 1), st["dropped"], got, st["datagrams"],
                   ", %d messages in bundles" % elements if form == "bundles" else ""))
            tx.close()
            for r in rx:
                r.close()
    say("  condition (a tick of bundles is exactly num_bundles x targets datagrams): %s" % ("met" if ok else "NOT MET"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--sender-only", action="store_true", help="part (b) alone: needs no GPU")
    ap.add_argument("--device-only", action="store_true", help="part (a) alone")
    ap.add_argument("--write", default=None, help="also write the report to this file")
    args = ap.parse_args()
    fx = importlib.import_module("feature-extractor_amd")
    say("OSC bundles: what they cost on the device and buy in the sender (tools/osc_bundles_bench.py)")
    ok = True
    if not args.sender_only:
        device_calls(fx, args.calls)
    if not args.device_only:
        ok = sender(fx, args.seconds, args.threads)
    if args.write:
        with open(args.write, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
