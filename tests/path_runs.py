"""The analysis dispatch paths as tests/test_gpu_rates.py and tests/test_gpu_levels.py run them: one hop stream through one path, the
launches of every call asserted (no test here: the two modules hold the results to the oracle and to the batch path)."""
import numpy as np

HOOK_TAIL_NEVER_FUSED = 4                       # csrc/fx_kernels.h, FX_HOOK_TAIL_NEVER_FUSED


def _calls(an, hops, per, kinds=None):
    """push_hops `per` hops at a time; every call's launches are `kinds`"""
    outs = []
    for t in range(0, hops.shape[1], per):
        outs.append(an.push_hops(hops[:, t:t + per]))
        if kinds is not None:
            assert [l["kind"] for l in an.last_launches()] == list(kinds), (t, an.last_launches())
    return tuple(np.concatenate([o[k] for o in outs], axis=1) for k in (0, 1))


def _ring(gpu_fx, an, hops, per, kinds=None, depth=2):
    st = gpu_fx.HopStream(an, per, slots=3)
    got = []
    try:                                            # (the ring is closed before its analyser, also when an assertion fails)
        for t in range(0, hops.shape[1], per):
            if st.in_flight() == depth:
                got.append(st.collect())
            st.push(hops[:, t:t + per])
            if kinds is not None:
                assert [l["kind"] for l in an.last_launches()] == list(kinds), (t, an.last_launches())
        while st.in_flight():
            got.append(st.collect())
    finally:
        st.close()
    return tuple(np.concatenate([g[k] for g in got], axis=1) for k in (0, 1))


def run_path(gpu_fx, path, N, rate, hops, fused_calls):
    """(raw, smoothed) of hops [C][T][N/2] through one dispatch path, its launches asserted; fused_calls: the (from, to) frames of the
    calls of the fused tail's path, each of 2 to 8 frames"""
    C, T = hops.shape[0], hops.shape[1]
    low = path in ("pair", "hop_pair", "ring_hop_pair")
    an = gpu_fx.BatchAnalyser(C, N, rate, low_latency=low)
    try:
        if path == "batch":                                       # fx_frame_kernel, finalise + epilogue + history
            out = an.push_hops(hops)
            assert [(l["kind"], l["ep_form"]) for l in an.last_launches()] == [("frame", 0), ("epilogue", 2)]
        elif path == "fused_tail":                                # fx_tail_fused_kernel's frame-per-lane form
            assert [lo for lo, _ in fused_calls] + [T] == [0] + [hi for _, hi in fused_calls]
            parts = []
            for lo, hi in fused_calls:
                parts.append(an.push_hops(hops[:, lo:hi]))
                assert [(l["kind"], l["ep_form"]) for l in an.last_launches()] == [("frame", 0), ("epilogue", 1)], (lo, hi)
            out = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
        elif path == "direct":                                    # one-frame direct form + the one-frame tail
            an.set_tuning(one_hop_kernel=0)
            if N >= 1024:
                an.set_test_hooks(HOOK_TAIL_NEVER_FUSED)
            out = _calls(an, hops, 1, ("frame", "epilogue"))
        elif path == "frame_tail":                                # fx_frame_tail_kernel
            an.set_tuning(one_hop_kernel=0)
            out = _calls(an, hops, 1, ("frame_tail",))
        elif path == "hop":                                       # fx_hop_kernel through fx_push_hops
            out = _calls(an, hops, 1, ("hop",))
        elif path == "ring_hop":                                  # fx_hop_kernel through the ring
            out = _ring(gpu_fx, an, hops, 1, ("hop",))
        elif path == "pair":                                      # fx_pair_kernel
            out = an.push_hops(hops)
            assert [l["kind"] for l in an.last_launches()] == ["pair", "epilogue"]
        elif path == "hop_pair":                                  # fx_hop_pair_kernel
            out = _calls(an, hops, 1, ("hop_pair",))
        elif path == "ring_hop_pair":
            out = _ring(gpu_fx, an, hops, 1, ("hop_pair",))
        elif path == "blocks":                                    # the block-fed forms: 480-sample device blocks
            flat = hops.reshape(C, -1)
            parts = [an.push_samples(np.ascontiguousarray(flat[:, at:at + 480])) for at in range(0, flat.shape[1], 480)]
            out = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
            assert out[0].shape[1] == T and an.pending_samples() == 0
        else:
            raise KeyError(path)
    finally:
        an.close()
    return out
