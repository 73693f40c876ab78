"""The 1024-point batch frame kernel with its per-wavefront record of lane-derived constants (csrc/fx_lane_consts.hip.h: addresses, masks and
window bases formed once in front of the frame loop instead of once per frame), against the CPU oracle at the suite's budgets
(oracle/ulp.py: onset and f0 exact, spread 2 ulp, the rest 0).  Inputs as in tests/test_gpu_lane_exchange.py: seeded white noise plus the
synthetic mix, every bin of every transform non-zero, so one wrong address or one wrong conjugation mask changes every bin.  All tests here
need a real MI355X.

What the shapes are for: 3 x 9 -- a partial last workgroup, wavefronts that loop over more than one frame on one record; 5 x 3 -- a short
call, one frame and one record per wavefront; 2 x 130 -- a call cut into time units, where the workgroup's channel and chunk
come from a ticket after the record could have been formed; 3 x 9 then 3 x 7 on one context -- state carried between launches while the
records are rebuilt; 2000-sample blocks -- the block-fed batch form; int16 hops -- the load stage's other format branch on the same
addresses; one analyser alone; low tones -- LazyLag::rest() on the record's twiddle address."""
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


def launches(an):
    return [(l["kind"], l["T"], l["block_mode"], l["num_chunks"]) for l in an.last_launches()]


def test_batch_3_channels_9_frames(gpu_fx, oracle):
    hops = mix(3, 9, seed=21)
    an = gpu_fx.BatchAnalyser(3, N)
    got = an.push_hops(hops)
    assert launches(an)[0][:2] == ("frame", 9), an.last_launches()
    an.close()
    close(got, want(oracle, "3x9", hops), "3 x 9")


def test_batch_5_channels_3_frames_in_one_call(gpu_fx, oracle):
    """three frames a channel in one call: the planner gives a channel no more wavefronts than the call has frames, so every wavefront
    forms a record for one frame and its loop ends after it (a wavefront without a frame would form one and never read it)"""
    hops = mix(5, 3, seed=22)
    an = gpu_fx.BatchAnalyser(5, N)
    got = an.push_hops(hops)
    first = an.last_launches()[0]
    assert first["kind"] == "frame" and first["T"] == 3 and first["waves_per_ch"] == 3, first
    an.close()
    close(got, want(oracle, "5x3", hops), "5 x 3")


def test_batch_2_channels_130_frames_cut_into_time_units(gpu_fx, oracle):
    hops = mix(2, 130, seed=23)
    an = gpu_fx.BatchAnalyser(2, N)
    got = an.push_hops(hops)
    first = an.last_launches()[0]
    assert first["kind"] == "frame" and first["num_chunks"] > 1, first
    an.close()
    close(got, want(oracle, "2x130", hops), "2 x 130")


def test_two_launches_on_one_context(gpu_fx, oracle):
    """3 x 9 and then 3 x 7: the flux state, the tail of the window and the histories go from launch to launch; the records do not"""
    hops = mix(3, 16, seed=24)
    an = gpu_fx.BatchAnalyser(3, N)
    a = an.push_hops(np.ascontiguousarray(hops[:, :9]))
    assert launches(an)[0][:2] == ("frame", 9), an.last_launches()
    b = an.push_hops(np.ascontiguousarray(hops[:, 9:]))
    assert launches(an)[0][:2] == ("frame", 7), an.last_launches()
    an.close()
    got = tuple(np.concatenate([a[k], b[k]], axis=1) for k in (0, 1))
    close(got, want(oracle, "3x16", hops), "3 x 9 then 3 x 7")


def test_push_samples_2000_sample_blocks(gpu_fx, oracle):
    """2000-sample blocks are three or four hops a call: the batch kernel's block-fed form reads them where they lie"""
    hops = mix(3, 16, seed=24)
    flat = hops.reshape(3, -1)
    an = gpu_fx.BatchAnalyser(3, N)
    parts, seen = [], []
    for at in range(0, flat.shape[1], 2000):
        parts.append(an.push_samples(np.ascontiguousarray(flat[:, at:at + 2000])))
        seen += launches(an)
    # 16 hops are 8192 samples: four blocks of 2000 and one of 192, which completes the last hop together with what is pending
    assert an.pending_samples() == 0
    an.close()
    assert any(kind == "frame" and T >= 3 and blk for kind, T, blk, _ in seen), seen
    got = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
    assert got[0].shape[1] == 16
    close(got, want(oracle, "3x16", hops), "2000-sample blocks")


def test_int16_hops(gpu_fx, oracle):
    """the same stream as 16-bit PCM: the load stage widens the samples (another branch of the format switch) and stores them through the
    same lane addresses"""
    hops = mix(3, 9, seed=21)
    pcm = np.clip(np.round(hops / np.float32(8.0) * 32768.0), -32768, 32767).astype(np.int16)         # (the mix peaks above 1: scaled into range)
    floats = pcm.astype(np.float32) / np.float32(32768.0)
    an = gpu_fx.BatchAnalyser(3, N)
    got = an.push_hops(pcm, sample_format="s16")
    assert launches(an)[0][:2] == ("frame", 9), an.last_launches()
    an.close()
    assert np.abs(pcm).max() < 32767 and np.count_nonzero(pcm) > 0.99 * pcm.size
    close(got, want(oracle, "3x9 s16", floats), "3 x 9 from int16")


@pytest.mark.parametrize("which,mask", [("spectral", 1), ("harmonic", 2)])
def test_single_analyser_contexts(gpu_fx, oracle, which, mask):
    hops = mix(3, 9, seed=21)
    an = gpu_fx.BatchAnalyser(3, N, analysers=which)
    got = an.push_hops(hops)
    assert launches(an)[0][:2] == ("frame", 9), an.last_launches()
    an.close()
    close(got, want(oracle, "3x9 " + which, hops, analysers=mask), "3 x 9 %s only" % which)


def test_lag_search_past_sample_255(gpu_fx, oracle):
    """low tones: frames whose lag search is not decided within the first 256 lags -- checked on the oracle's own cnd first -- so that the
    rest of the inverse transform's last pass reads its twiddles through the record"""
    hops = signals.low_tones(6, 6, N, seed=N + 3)
    regimes = {(c, t): lc.lag_regime(oracle, w) for c in range(hops.shape[0]) for t, w in enumerate(lc.windows(hops[c]))}
    past = sorted(k for k, v in regimes.items() if v in ("past 255", "fallback"))
    print("frames past sample 255:", past)
    assert past, regimes
    an = gpu_fx.BatchAnalyser(6, N)
    got = an.push_hops(hops)
    assert launches(an)[0][:2] == ("frame", 6), an.last_launches()
    an.close()
    close(got, want(oracle, "low tones", hops), "low tones, batch")
