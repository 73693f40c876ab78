"""What per-track OSC addresses cost (include/fx.h, fx_set_osc_addresses / fx_get_osc_datagrams_addressed / fx_osc_sender_set_routes).

(a) fx_get_osc_datagrams_addressed to page-locked host memory against fx_get_osc_datagrams (fx_osc.hip, which this change does not
    touch: the parent commit's call) on the SAME context, the two alternated call by call in one process; 1024 / 8192 / 65 536 tracks;
    addresses "/Audio/A<n>" (the same bytes and stride as the prefix form) and 64-byte addresses (stride 132).  Time: a host clock
    around one call, which ends in a synchronisation (FX_MEM_HOST); best / median over `calls` calls per round, `rounds` rounds after a
    warm-up round.  Yardstick: the prefix call's median scaled by the ratio of strides (the copy to the host dominates), with a margin
    equal to the prefix call's own round-to-round spread (largest - smallest round median) in this session.  The verdict is printed,
    never tuned.
(b) the batch sender over loopback with routes: 8192 tracks over 4 targets (primary and secondary), 60 Hz timer: ticks late, longest
    tick, datagrams received -- against the same sender without routes.  Recorded, not gated.

    python tools/osc_addresses_bench.py [--rounds 7] > profiles/osc_addresses_bench.txt"""
import argparse
import ctypes
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def pinned(fx, nbytes):
    p = ctypes.c_void_p()
    fx.capi.check(fx.load_library().fx_host_alloc(ctypes.byref(p), nbytes))
    return p


def datagram_calls(fx, rounds, calls):
    import torch
    import signals
    lib = fx.load_library()
    N = 1024
    ip = ctypes.POINTER(ctypes.c_int)
    print("(a) fx_get_osc_datagrams_addressed against fx_get_osc_datagrams on one context, alternated; to page-locked host memory; %s" % torch.cuda.get_device_name(0))
    for C in (1024, 8192, 65536):
        an = fx.BatchAnalyser(C, N)
        base = signals.tone_vibrato_noise(256, 2, N, seed=5)
        hops = torch.from_numpy(np.ascontiguousarray(np.tile(base, (C // 256, 1, 1)))).cuda()
        an.push_hops(hops)
        an.sync()
        latest = an.get_features()
        lengths = np.empty(C, np.int32)
        prefix_stride = fx.capi.osc_stride("/Audio/A", 0, C)
        for form in ("/Audio/A<n>", "64-byte addresses"):
            addr = ["/Audio/A%d" % c for c in range(C)] if form == "/Audio/A<n>" else ["/" + ("Mixer/Drums/Kick/%07d/" % c).ljust(63, "x") for c in range(C)]
            an.set_osc_addresses(addr)
            stride = an.osc_address_stride()
            buf = pinned(fx, C * max(stride, prefix_stride))
            host = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ctypes.c_ubyte)), shape=(C * max(stride, prefix_stride),))

            def prefix_call():
                return lib.fx_get_osc_datagrams(an._h, b"/Audio/A", 0, buf, prefix_stride, lengths.ctypes.data_as(ip), fx.capi.MEM_HOST)

            def addressed_call():
                return lib.fx_get_osc_datagrams_addressed(an._h, buf, stride, lengths.ctypes.data_as(ip), fx.capi.MEM_HOST)

            # the bytes first: the host twin's, bitwise
            fx.capi.check(addressed_call())
            want, _ = fx.capi.osc_encode_addressed(addr, latest, stride=stride)
            assert np.array_equal(host[:C * stride].reshape(C, stride), want), "the device's datagrams are not the host twin's"
            med = {"prefix": [], "addressed": []}
            best = {"prefix": [], "addressed": []}
            for r in range(rounds + 1):
                t = {"prefix": [], "addressed": []}
                for _ in range(calls):
                    for name, fn in (("prefix", prefix_call), ("addressed", addressed_call)):
                        t0 = time.perf_counter()
                        st = fn()
                        t[name].append((time.perf_counter() - t0) * 1e6)
                        assert st == 0
                if r:                                       # round 0 warms up
                    for name in t:
                        med[name].append(float(np.median(t[name])))
                        best[name].append(float(np.min(t[name])))
            p, a = np.array(med["prefix"]), np.array(med["addressed"])
            spread = p.max() - p.min()
            expected = float(np.median(p)) * stride / prefix_stride
            got = float(np.median(a))
            verdict = "inside" if got <= expected + spread else "OUTSIDE"
            print("  %6d tracks, %-17s stride %3d (prefix form %2d): prefix median %.1f us (round medians %.1f .. %.1f, best %.1f); addressed median %.1f us "
                  "(round medians %.1f .. %.1f, best %.1f); yardstick %.1f x %d/%d = %.1f us + spread %.1f us -> %s the band (%+.1f us against the yardstick)"
                  % (C, form + ":", stride, prefix_stride, np.median(p), p.min(), p.max(), min(best["prefix"]), got, a.min(), a.max(), min(best["addressed"]),
                     np.median(p), stride, prefix_stride, expected, spread, verdict, got - expected))
            fx.capi.check(lib.fx_host_free(buf))
        an.close()


def routed_sender(fx, seconds):
    capi = fx.capi
    C, targets = 8192, 4
    v = np.random.default_rng(1).standard_normal((C, 12)).astype(np.float32)
    d, n = capi.osc_encode_batch("/Audio/A", 0, v)
    print("(b) batch sender over loopback, %d tracks, 60 Hz timer for %.0f s, 4 sender threads, segmented sends on (host only)" % (C, seconds))
    for routes in (False, True):
        rx = [capi.OscReceiver("127.0.0.1:0", threads=2) for _ in range(targets if routes else 2)]
        ports = ["127.0.0.1:%d" % r.port for r in rx]
        tx = capi.OscSender(ports[0], ports[1], threads=4, gso=True)
        if routes:
            primary = np.arange(C) % targets
            secondary = (primary + 1 + (np.arange(C) // targets) % (targets - 1)) % targets
            tx.set_routes(ports, primary, secondary)
        tx.update(d, n)
        tx.start(60.0)
        time.sleep(seconds)
        tx.stop()
        st = tx.stats()
        time.sleep(0.3)
        got = sum(r.stats()["datagrams"] for r in rx)
        print("  %-34s ticks %d, late %d, longest tick %.3f ms, mean %.3f ms; datagrams %d in %d system calls, dropped by the sender %d, received %d (%.4f)"
              % ("routes over 4 targets (2 per track):" if routes else "no routes (primary + secondary):", st["ticks"], st["late_ticks"], st["max_tick_ms"],
                 st["total_tick_ms"] / max(st["ticks"], 1), st["datagrams"], st["syscalls"], st["dropped"], got, got / max(st["datagrams"], 1)))
        tx.close()
        for r in rx:
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--sender-only", action="store_true", help="part (b) alone: needs no GPU")
    args = ap.parse_args()
    fx = importlib.import_module("feature-extractor_amd")
    print("per-track OSC addresses and routes: what they cost (tools/osc_addresses_bench.py)")
    if not args.sender_only:
        datagram_calls(fx, args.rounds, args.calls)
    routed_sender(fx, args.seconds)


if __name__ == "__main__":
    main()
