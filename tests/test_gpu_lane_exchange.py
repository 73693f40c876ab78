"""The 1024-point kernels with their second FFT exchange done by lane swaps (csrc/fx_lane_exchange.h), against the CPU oracle at the
suite's budgets (oracle/ulp.py: onset and f0 exact, spread 2 ulp, the rest 0).  The inputs are seeded white noise plus the synthetic
mix: every bin of every transform is non-zero, so one mis-routed element changes every bin.  All tests here need a real MI355X.

Shapes: 3 channels x 9 frames (a partial last workgroup, more than one frame per wave), 2 x 130 (cut into time units: the hand-over),
5 x 1 through fx_hop_kernel and through fx_frame_tail_kernel, a spectral-only and a harmonic-only context, and a stream with frames whose
lag search runs past sample 255, where LazyLag::rest() consumes the exchanged operands.

(The global-minimum fallback itself -- no cnd below 0.01 anywhere in [2, N) -- cannot be reached by a 1024-point window: the search
is symmetric about N/2 and cnd is about 2 / s for a smooth autocorrelation, tests/test_levels_cpu.py.  What the lag frames have to do
is take the search past sample 255; that is asserted on the oracle's own cnd, and a fallback frame would count as well.)"""
import numpy as np
import pytest

import level_cases as lc
import signals

pytestmark = pytest.mark.gpu

N = 1024


def mix(C, T, seed):
    """white noise under the tone / vibrato / noise mix, [C][T][N/2]"""
    return (signals.tone_vibrato_noise(C, T, N, seed=seed) + 0.3 * signals.loud_noise(C, T, N, seed=seed + 100)).astype(np.float32)


_ORACLE = {}


def want(oracle, name, hops, **settings):
    """the oracle's (raw, smoothed) of a hop stream, computed once and shared (read-only)"""
    if name not in _ORACLE:
        out = oracle.push_hops(hops, N, **settings)
        for a in out:
            a.setflags(write=False)
        _ORACLE[name] = out
    return _ORACLE[name]


def close(got, ref, what):
    from oracle import fx_oracle as fo
    for k, name in ((0, "raw"), (1, "smoothed")):
        signals.assert_features_within(got[k], ref[k], signals.ulp_budget("default"), fo.FEATURE_NAMES, "%s %s" % (what, name))


def kinds(an):
    return [l["kind"] for l in an.last_launches()]


def test_batch_3_channels_9_frames(gpu_fx, oracle):
    hops = mix(3, 9, seed=11)
    an = gpu_fx.BatchAnalyser(3, N)
    got = an.push_hops(hops)
    assert kinds(an)[0] == "frame"
    an.close()
    close(got, want(oracle, "3x9", hops), "3 x 9")


def test_batch_2_channels_130_frames_cut_into_time_units(gpu_fx, oracle):
    hops = mix(2, 130, seed=12)
    an = gpu_fx.BatchAnalyser(2, N)
    got = an.push_hops(hops)
    assert kinds(an)[0] == "frame"
    an.close()
    close(got, want(oracle, "2x130", hops), "2 x 130")


@pytest.mark.parametrize("one_hop_kernel,kind", [(1, "hop"), (0, "frame_tail")])
def test_one_frame_calls_of_5_channels(gpu_fx, oracle, one_hop_kernel, kind):
    """5 channels x 1 frame per call, three calls: fx_hop_kernel, and with it forced off the direct frame-tail form"""
    hops = mix(5, 3, seed=13)
    an = gpu_fx.BatchAnalyser(5, N)
    an.set_tuning(one_hop_kernel=one_hop_kernel)
    outs = []
    for t in range(hops.shape[1]):
        outs.append(an.push_hops(hops[:, t:t + 1]))
        assert kinds(an) == [kind], (t, an.last_launches())
    an.close()
    got = tuple(np.concatenate([o[k] for o in outs], axis=1) for k in (0, 1))
    close(got, want(oracle, "5x1x3", hops), "5 x 1, %s" % kind)


@pytest.mark.parametrize("which,mask", [("spectral", 1), ("harmonic", 2)])
def test_single_analyser_contexts(gpu_fx, oracle, which, mask):
    hops = mix(3, 9, seed=11)
    an = gpu_fx.BatchAnalyser(3, N, analysers=which)
    got = an.push_hops(hops)
    an.close()
    close(got, want(oracle, "3x9 " + which, hops, analysers=mask), "3 x 9 %s only" % which)


def test_lag_search_past_sample_255(gpu_fx, oracle):
    """low tones: frames whose lag search is not decided within the first 256 lags -- checked on the oracle's own cnd first -- so that
    the rest of the inverse transform's last pass runs on the exchanged operands; through the batch kernel and the hop kernel"""
    hops = signals.low_tones(6, 6, N, seed=N + 2)
    regimes = {(c, t): lc.lag_regime(oracle, w) for c in range(hops.shape[0]) for t, w in enumerate(lc.windows(hops[c]))}
    past = sorted(k for k, v in regimes.items() if v in ("past 255", "fallback"))
    print("frames past sample 255:", past)
    assert past, regimes
    ref = want(oracle, "low tones", hops)
    an = gpu_fx.BatchAnalyser(6, N)
    close(an.push_hops(hops), ref, "low tones, batch")
    an.close()
    an = gpu_fx.BatchAnalyser(6, N)
    outs = [an.push_hops(hops[:, t:t + 1]) for t in range(hops.shape[1])]
    assert kinds(an) == ["hop"]
    an.close()
    close(tuple(np.concatenate([o[k] for o in outs], axis=1) for k in (0, 1)), ref, "low tones, hop kernel")
