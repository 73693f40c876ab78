"""The 1024-point batch frame kernel's flux state by runs (csrc/fx_flux_runs.h; FluxRuns in csrc/fx_frame_kernel.hip.h): a channel's
wavefronts analyse contiguous runs of a work unit's frames, each against a flux image of its own, and the state crosses from wavefront to
wavefront once per run, behind it: a run's first accepted frame and every frame before it that is not accepted (silence, NaN, a level below
the acceptance threshold) leave their flux open, and it is closed against the predecessor's final image when both runs are over.  Every case is held to
the CPU oracle at the suite's budgets (oracle/ulp.py) and, bit for bit, to the same frames given in calls cut elsewhere (other units, other
runs, other first frames).  Whole frames ([C][T][N], fx_process_frames), so that a frame is silent or not by itself; run shapes are forced
through fx_tuning (waves_per_channel, unit_plan, frames_per_unit) as the dispatch-path tests do.  All tests here need a real MI355X.

Runs of a unit of n frames on k wavefronts: the first n % k wavefronts take n / k + 1 frames, the others n / k (flux_run_begin)."""
import numpy as np
import pytest

import overflow_cases as oc
import signals

pytestmark = pytest.mark.gpu

N = 1024
BUDGET = signals.ulp_budget("default")


def mix(C, T, seed):
    """white noise under the tone / vibrato / noise mix, as whole frames [C][T][N]: every bin of every frame non-zero"""
    hops = signals.tone_vibrato_noise(C, 2 * T, N, seed=seed) + 0.3 * signals.loud_noise(C, 2 * T, N, seed=seed + 100)
    return np.ascontiguousarray(hops.astype(np.float32).reshape(C, T, N))


def run_begin(n, k, slot):
    return slot * (n // k) + min(slot, n % k)


def first_frames(units, k):
    """the first frame of every wavefront's run but the unit's first, over a call cut into `units`"""
    out, at = [], 0
    for n in units:
        out += [at + run_begin(n, k, s) for s in range(1, min(n, k))]
        at += n
    return out


_ORACLE = {}


def want(oracle, name, frames):
    if name not in _ORACLE:
        out = oracle.process_frames(frames, N)
        for a in out:
            a.setflags(write=False)
        _ORACLE[name] = out
    return _ORACLE[name]


def same_bits(a, b, what):
    for k, name in ((0, "raw"), (1, "smoothed")):
        assert a[k].shape == b[k].shape
        x, y = np.ascontiguousarray(a[k], np.float32), np.ascontiguousarray(b[k], np.float32)
        differ = (x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))      # the same bits; a NaN is a NaN
        assert not differ.any(), "%s %s differs at (channel, frame, slot) %s" % (what, name, np.argwhere(differ)[:6].tolist())


def check(gpu_fx, oracle, name, frames, tuning, cuts, expect_chunks=None, expect_waves=None, masked=False):
    """one call under `tuning` against the oracle, and against the same frames in calls cut at `cuts` on a context with default tuning"""
    C, T = frames.shape[:2]
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_tuning(**tuning)
    got = an.process_frames(frames)
    first = an.last_launches()[0]
    assert first["kind"] == "frame" and first["T"] == T, first
    if expect_chunks is not None:
        assert first["num_chunks"] == expect_chunks, first
    if expect_waves is not None:
        assert first["waves_per_ch"] == expect_waves, first
    an.close()
    ref = want(oracle, name, frames)
    mask = oc.defined(ref[0]) if masked else (None, None)
    for k, label in ((0, "raw"), (1, "smoothed")):
        print(name, label, signals.assert_features_within(got[k], ref[k], BUDGET, what="%s %s" % (name, label), defined=mask[k]))
    other = gpu_fx.BatchAnalyser(C, N)
    parts, at = [], 0
    for n in cuts:
        parts.append(other.process_frames(np.ascontiguousarray(frames[:, at:at + n])))
        at += n
    assert at == T
    other.close()
    same_bits(got, tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1)), name + " against split calls")
    return got


def test_runs_of_one_and_two_frames(gpu_fx, oracle):
    """40 frames as units of 16, 8, 8, 8 on eight wavefronts: runs of two frames, then three units of one frame a wavefront"""
    frames = mix(3, 40, seed=31)
    check(gpu_fx, oracle, "3x40", frames, {"waves_per_channel": 8, "unit_plan": [16, 8, 8, 8]}, cuts=[7, 28, 5], expect_chunks=4, expect_waves=8)


def test_frames_no_multiple_of_the_wavefronts(gpu_fx, oracle):
    """43 frames in one unit: runs of 6, 6, 6 and five of 5"""
    frames = mix(4, 43, seed=32)
    check(gpu_fx, oracle, "4x43", frames, {"frames_per_unit": 0}, cuts=[9, 21, 13], expect_chunks=1, expect_waves=8)


@pytest.mark.parametrize("T,waves", [(11, 8), (5, 5)])
def test_fewer_frames_than_two_rounds(gpu_fx, oracle, T, waves):
    """11 frames on eight wavefronts: runs of 2, 2, 2 and five of 1; 5 frames: the planner gives the channel five wavefronts, one frame each"""
    frames = mix(5, T, seed=33 + T)
    check(gpu_fx, oracle, "5x%d" % T, frames, {}, cuts=[2, T - 2], expect_chunks=1, expect_waves=waves)


def test_a_run_that_starts_in_silence(gpu_fx, oracle):
    """the first frame of a run is silent and the next is not: both frames' flux is closed after the run, against the predecessor's state.  Units 16, 8, 8, 8:
    frame 6 is the first of the fourth run of the first unit, frames 18 and 19 are runs of their own in the second; each channel has
    its own silent frames, and channel 2 none"""
    frames = mix(3, 40, seed=34)
    units = [16, 8, 8, 8]
    starts = first_frames(units, 8)
    assert 6 in starts and 18 in starts and 19 in starts and 7 not in starts
    frames[0, 6] = 0.0
    frames[1, 18] = 0.0; frames[1, 19] = 0.0
    frames[0, 33] = 0.0
    check(gpu_fx, oracle, "silent first", frames, {"waves_per_channel": 8, "unit_plan": units}, cuts=[6, 13, 21], expect_chunks=4)


def test_whole_runs_of_silence_between_tones(gpu_fx, oracle):
    """40 frames in one unit are runs of 5: frames 10 .. 24 are three whole runs that accept nothing, so the fourth wavefront's open flux is
    closed against a state that came through them unchanged from the second; in channel 1 the silence starts and ends inside runs"""
    frames = mix(3, 40, seed=35)
    frames[0, 10:25] = 0.0
    frames[1, 12:28] = 0.0
    check(gpu_fx, oracle, "silent runs", frames, {"frames_per_unit": 0}, cuts=[11, 9, 20], expect_chunks=1, expect_waves=8)


def test_a_silent_call_between_tonal_calls(gpu_fx, oracle):
    """a call that accepts nothing hands the flux state on as it found it: the third call's first frame is against the first call's last"""
    frames = mix(3, 48, seed=36)
    frames[:, 16:32] = 0.0
    ref = want(oracle, "silent call", frames)
    an = gpu_fx.BatchAnalyser(3, N)
    parts = [an.process_frames(np.ascontiguousarray(frames[:, at:at + 16])) for at in (0, 16, 32)]
    an.close()
    got = tuple(np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
    for k, label in ((0, "raw"), (1, "smoothed")):
        print("silent call", label, signals.assert_features_within(got[k], ref[k], BUDGET, what="silent call " + label))
    whole = gpu_fx.BatchAnalyser(3, N)
    one = whole.process_frames(frames)
    whole.close()
    same_bits(got, one, "three calls of 16 against one of 48")


def test_nan_frames_at_the_ends_of_a_run(gpu_fx, oracle):
    """a frame with a NaN sample is not accepted (every magnitude is NaN): at a run's first place it leaves the state the predecessor's, at its last the
    state handed on is the frame before's.  One unit of 40 frames, runs of 5: frame 10 is a first, frame 14 a last"""
    frames = mix(3, 40, seed=37)
    assert 10 in first_frames([40], 8) and 15 in first_frames([40], 8)
    frames[0, 10, 300] = np.nan
    frames[1, 14, 17] = np.nan
    frames[2, 10, 0] = np.nan; frames[2, 14, 1023] = np.nan
    check(gpu_fx, oracle, "nan ends", frames, {"frames_per_unit": 0}, cuts=[10, 5, 25], expect_chunks=1, masked=True)


def test_a_silent_channel_beside_a_tonal_one(gpu_fx, oracle):
    """no wavefront of channel 1 accepts anything -- each takes its predecessor's image when both are done -- while its neighbours park and close"""
    frames = mix(3, 40, seed=38)
    frames[1] = 0.0
    check(gpu_fx, oracle, "silent channel", frames, {"waves_per_channel": 8, "unit_plan": [16, 8, 8, 8]}, cuts=[7, 28, 5], expect_chunks=4)


def test_quiet_frames_at_the_heads_of_runs(gpu_fx, oracle):
    """noise at sigma 3e-4 is far below the acceptance threshold and not silence: such frames replace nothing and have no flux of their
    own, and the accepted frame behind them is against the state from before them.  One unit of 40 frames, runs of 5: in channel 0 (a
    pure tone, so that the state has small bins) the third run starts with three quiet frames, in channel 1 the fourth run is quiet
    throughout and so are the first two frames of the fifth, channel 2 is quiet from the second run's second frame to the call's end"""
    frames = mix(3, 40, seed=39)
    frames[0] = signals.sine(1, 80, N).reshape(40, N)
    quiet = (3e-4 * signals.loud_noise(3, 80, N, seed=139)).astype(np.float32).reshape(3, 40, N)
    frames[0, 10:13] = quiet[0, 10:13]
    frames[1, 15:22] = quiet[1, 15:22]
    frames[2, 6:] = quiet[2, 6:]
    check(gpu_fx, oracle, "quiet heads", frames, {"frames_per_unit": 0}, cuts=[10, 6, 24], expect_chunks=1, expect_waves=8)
    ref = want(oracle, "quiet heads", frames)[0]
    assert (ref[0, 10:13, 1] > 0).all() and (ref[0, 10:13, 3] == 0).all() and ref[0, 13, 7] > 0, "the quiet frames are not silent, not accepted, and the next frame has a flux"
