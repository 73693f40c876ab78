"""Analysis taps on the device (include/fx.h, fx_request_taps / fx_get_taps): the reference's display buffers for armed channels.
(1) every committed fixture -- the reference's own getters, tests/golden/taps -- is reproduced bit for bit by arming before the same hop;
(2) on every analysis dispatch path of tests/dispatch_paths.py, arming channels 0 and C-1 before the third call adds exactly one taps
launch, first, to the call that serves it, the taps are the oracle's for the first frame that call analysed, and no result bit of any
call changes; (3) the lag position reproduces the raw F0 slot; (4) the calls that must not capture do not, and the request waits."""
import glob
import os

import numpy as np
import pytest

import dispatch_paths as dp
import taps_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "taps", "*.npz")))
ONSET_WINDOW = 21


def _taps_record(N, channels, blocks=0):
    r = dict.fromkeys(dp.FIELDS, 0)
    r.update(kind="taps", window=N, T=channels, block_mode=blocks)
    return r


def _f0_of_lag(x, N, nyquist=24000.0):
    """the raw F0 slot for a lag position x >= 0 (PitchAnalyser.h:57, RealTimeAnalyser.h:165-166)"""
    lag = np.float32(x) * np.float32(2 * N)
    return np.float32((nyquist * 2.0) / float(lag) / 5000.0)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fixture_reproduced(gpu_fx, path):
    d = np.load(path)
    N, hops, gain = int(d["window_size"]), d["hops"], float(d["gain"])
    C = 3
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_gain(gain)
    captures = list(d["captures"])
    for t in range(hops.shape[0]):
        if t in captures:
            an.request_taps([1])
        raw, _ = an.push_hops(np.ascontiguousarray(np.broadcast_to(hops[t], (C, 1, N // 2))))
        if t in captures:
            assert an.last_launches()[0]["kind"] == "taps"
            got = an.taps(1)
            i = captures.index(t)
            taps_model.assert_taps_equal(got, {f: d[f][i] for f in taps_model.FIELDS}, "%s hop %d" % (os.path.basename(path), t))
            assert got["frame_index"] == t
            x = got["lag_position"][0]
            if x >= 0:
                assert _f0_of_lag(x, N) == raw[1, 0, 2], (t, x, raw[1, 0, 2])
            with pytest.raises(gpu_fx.FxError):
                an.taps(0)
        else:
            assert all(l["kind"] != "taps" for l in an.last_launches())
    an.close()


# ---- every dispatch path ----
MASKS = {"both": 3, "spectral": 1, "harmonic": 2}


def _as_format(x, fmt):
    if fmt == "s16":
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return x


def _floats(x, fmt):
    return x.astype(np.float32) / np.float32(32768.0) if fmt == "s16" else x


def _windows(hops):
    C, T, H = hops.shape
    x = np.concatenate([np.zeros((C, 1, H), hops.dtype), hops], axis=1)
    return np.ascontiguousarray(np.concatenate([x[:, :-1], x[:, 1:]], axis=2))


def _plan(r):
    """the row's stream [C][hops][N/2] and its calls' pieces (as tests/test_gpu_dispatch.py plans them)"""
    H = r.N // 2
    if r.entry == "samples":
        first, then = r.per
        lengths = [first] + [then] * (r.calls - 1)
        total = sum(lengths)
        hops = total // H
        x = _as_format(dp.stream(r.C, hops + 1, r.N, seed=r.N).reshape(r.C, -1)[:, :total], r.fmt)
        pieces, at = [], 0
        for n in lengths:
            pieces.append(np.ascontiguousarray(x[:, at:at + n]))
            at += n
        return np.ascontiguousarray(x[:, :hops * H].reshape(r.C, hops, H)), pieces
    hops = _as_format(dp.stream(r.C, r.per * r.calls, r.N, seed=r.N), r.fmt)
    feed = _windows(hops) if r.entry == "frames" else hops
    return hops, [np.ascontiguousarray(feed[:, t:t + r.per]) for t in range(0, hops.shape[1], r.per)]


def _run(gpu_fx, r, pieces, arm_before=None, channels=()):
    an = gpu_fx.BatchAnalyser(r.C, r.N, analysers=r.analysers, low_latency=r.low_latency)
    an.set_onset_window_length(ONSET_WINDOW)
    if r.tuning:
        an.set_tuning(**r.tuning)
    if r.hooks:
        an.set_test_hooks(r.hooks)
    outs, records, taps = [], [], None
    for i, piece in enumerate(pieces):
        if i == arm_before:
            an.request_taps(list(channels))
        if r.entry == "hops":
            out = an.push_hops(piece)
        elif r.entry == "frames":
            out = an.process_frames(piece)
        else:
            out = an.push_samples(piece)
        outs.append(out)
        records.append(an.last_launches())
        if taps is None and arm_before is not None and i >= arm_before and out[0].shape[1] > 0:
            taps = {c: an.taps(c) for c in channels}
    an.close()
    return outs, records, taps


CALL_ROWS = [r for r in dp.ROWS if r.entry != "ring"]


@pytest.mark.parametrize("r", CALL_ROWS, ids=[r.id for r in CALL_ROWS])
def test_dispatch_path_with_taps(gpu_fx, oracle, r):
    import torch
    if torch.cuda.get_device_properties(0).multi_processor_count != dp.CUS:
        pytest.skip("the table's launch sequences are written for %d CUs" % dp.CUS)
    hops, pieces = _plan(r)
    channels = sorted({0, r.C - 1})
    base, base_rec, _ = _run(gpu_fx, r, pieces)
    outs, records, taps = _run(gpu_fx, r, pieces, arm_before=2, channels=channels)
    frames = [o[0].shape[1] for o in outs]
    served = next(i for i in range(2, len(pieces)) if frames[i] > 0)
    first_frame = sum(frames[:served])
    for i, (rec, want) in enumerate(zip(records, base_rec)):
        if i == served:
            blocks = int(r.entry == "samples" and (rec[1:] and (rec[1]["kind"] == "reblock" or rec[1]["block_mode"] == 1)))
            assert rec == [_taps_record(r.N, len(channels), blocks)] + want, (r.id, i, rec)
            assert rec[1:] == r.expect[frames[i]], (r.id, i)
        else:
            assert rec == want, (r.id, i, rec)
        assert np.array_equal(outs[i][0], base[i][0], equal_nan=True) and np.array_equal(outs[i][1], base[i][1], equal_nan=True), (r.id, i)
    x = _floats(hops, r.fmt)
    for c in channels:
        got = taps[c]
        if r.entry == "frames":
            window = _windows(x)[c, first_frame]
        else:
            tail = x[c, first_frame - 1] if first_frame > 0 else np.zeros(r.N // 2, np.float32)
            window = np.concatenate([tail, x[c, first_frame]]).astype(np.float32)
        assert got["frame_index"] == first_frame, (r.id, got["frame_index"], first_frame)
        taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, window), "%s channel %d" % (r.id, c))
        if MASKS[r.analysers] & 2 and got["lag_position"][0] >= 0:
            assert _f0_of_lag(got["lag_position"][0], r.N) == outs[served][0][c, 0, 2], (r.id, c)


# ---- sample formats and memory kinds the table does not reach ----
@pytest.mark.parametrize("fmt", ["f32", "f16", "s16", "s24"])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_formats_and_memory(gpu_fx, oracle, fmt, mem):
    import torch
    import signals
    N, C, T = 2048, 4, 6
    x = signals.tone_vibrato_noise(C, T, N)
    if fmt == "f32":
        data, floats = x, x
    elif fmt == "f16":
        data = x.astype(np.float16)
        floats = data.astype(np.float32)
    elif fmt == "s16":
        data = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        floats = data.astype(np.float32) / np.float32(32768.0)
    else:
        v = np.clip(np.round(x * 8388608.0), -8388608, 8388607).astype(np.int32)
        data = gpu_fx.pack_s24(v)
        floats = v.astype(np.float32) / np.float32(8388608.0)
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_gain(0.75)
    kw = {"sample_format": "s24"} if fmt == "s24" else {}
    for t in range(T):
        piece = np.ascontiguousarray(data[:, t:t + 1]) if fmt != "s24" else np.ascontiguousarray(data[:, t:t + 1]).view(type(data))
        if mem == "device":
            piece = torch.from_numpy(np.ascontiguousarray(piece).view(np.uint8) if fmt == "s24" else piece).cuda()
        if t == 3:
            an.request_taps([2])
        an.push_hops(piece, **kw)
        if t == 3:
            got = an.taps(2)
    an.close()
    g = np.float32(0.75)
    window = np.concatenate([floats[2, 2] * g, floats[2, 3] * g]).astype(np.float32)
    assert got["frame_index"] == 3
    taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, window), "%s %s" % (fmt, mem))


@pytest.mark.parametrize("N,block", [(1024, 300), (2048, 700), (4096, 5000), (512, 1000)])
@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_blocks_capture_the_first_hop_of_pending_and_block(gpu_fx, oracle, N, block, fmt):
    import torch
    import signals
    C = 3
    x = signals.tone_vibrato_noise(C, 8, N).reshape(C, -1)
    data = x.astype(np.float16) if fmt == "f16" else x
    floats = data.astype(np.float32)
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_gain(1.5)
    H, at, seen = N // 2, 0, 0
    captured = False
    while at + block <= x.shape[1]:
        piece = torch.from_numpy(np.ascontiguousarray(data[:, at:at + block])).cuda()
        pending = an.pending_samples()
        an.request_taps([0, C - 1])
        raw, _ = an.push_samples(piece)
        at += block
        if raw.shape[1] == 0:
            assert all(l["kind"] != "taps" for l in an.last_launches())
            continue
        assert an.last_launches()[0]["kind"] == "taps"
        for c in (0, C - 1):
            got = an.taps(c)
            tail = floats[c, (seen - 1) * H:seen * H] * np.float32(1.5) if seen else np.zeros(H, np.float32)
            window = np.concatenate([tail, floats[c, seen * H:(seen + 1) * H] * np.float32(1.5)]).astype(np.float32)
            assert got["frame_index"] == seen and seen * H == at - block - pending
            taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, window), "block %d channel %d frame %d" % (block, c, seen))
        seen += raw.shape[1]
        captured = True
    an.close()
    assert captured


@pytest.mark.parametrize("flags", [dict(analysers="spectral"), dict(analysers="harmonic"), dict(low_latency=True)])
def test_every_buffer_whatever_the_analysers(gpu_fx, oracle, flags):
    import signals
    N, C = 4096, 2
    x = signals.low_tones(C, 5, N)
    an = gpu_fx.BatchAnalyser(C, N, **flags)
    an.push_hops(x[:, :2])
    an.request_taps([1])
    an.push_hops(x[:, 2:5])
    got = an.taps(1)
    an.close()
    taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, np.concatenate([x[1, 1], x[1, 2]])), str(flags))
    assert got["frame_index"] == 2


# ---- the calls that do not capture ----
def test_request_waits_for_a_call_that_analyses(gpu_fx, oracle):
    import signals
    N, C, H = 1024, 4, 512
    x = signals.tone_vibrato_noise(C, 10, N)
    flat = x.reshape(C, -1)
    an = gpu_fx.BatchAnalyser(C, N)
    with pytest.raises(gpu_fx.FxError):
        an.taps(0)                                  # nothing captured yet
    an.request_taps([0])
    an.request_taps([0, 3])                         # accumulates; re-arming 0 changes nothing
    raw, _ = an.push_samples(np.ascontiguousarray(flat[:, :200]))   # completes no hop
    assert raw.shape[1] == 0 and all(l["kind"] != "taps" for l in an.last_launches())
    with pytest.raises(gpu_fx.FxError):
        an.taps(0)
    raw, _ = an.push_samples(np.ascontiguousarray(flat[:, 200:H + 400]))   # completes hop 0
    assert raw.shape[1] == 1
    rec = an.last_launches()
    assert rec[0] == _taps_record(N, 2, 1)
    for c in (0, 3):
        got = an.taps(c)
        assert got["frame_index"] == 0
        taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, np.concatenate([np.zeros(H, np.float32), x[c, 0]])), "first frame")
    with pytest.raises(gpu_fx.FxError):
        an.taps(1)                                  # not armed
    an.push_samples(np.ascontiguousarray(flat[:, H + 400:2 * H + 400]))
    assert all(l["kind"] != "taps" for l in an.last_launches())     # the request was served
    assert an.taps(3)["frame_index"] == 0          # the capture stays until the next one
    an.close()


def test_ring_submissions_leave_the_request_armed(gpu_fx, oracle):
    import signals
    N, C, H = 2048, 3, 1024
    x = signals.tone_vibrato_noise(C, 8, N)
    an = gpu_fx.BatchAnalyser(C, N)
    an.request_taps([1])
    for hops_per_batch, t0 in ((1, 0), (2, 1)):
        st = gpu_fx.HopStream(an, hops_per_batch, slots=2)
        st.push(np.ascontiguousarray(x[:, t0:t0 + hops_per_batch]))
        assert all(l["kind"] != "taps" for l in an.last_launches())
        st.collect()
        st.close()
    with pytest.raises(gpu_fx.FxError):
        an.taps(1)
    an.push_hops(np.ascontiguousarray(x[:, 3:5]))
    assert an.last_launches()[0]["kind"] == "taps"
    got = an.taps(1)
    assert got["frame_index"] == 3                  # frames count across calls, the ring's included
    taps_model.assert_taps_equal(got, taps_model.oracle_taps(oracle, np.concatenate([x[1, 2], x[1, 3]])), "after the ring")
    an.close()


def test_reset_drops_request_and_capture(gpu_fx):
    import signals
    N, C = 512, 2
    x = signals.tone_vibrato_noise(C, 6, N)
    an = gpu_fx.BatchAnalyser(C, N)
    an.request_taps([0])
    an.push_hops(np.ascontiguousarray(x[:, :2]))
    assert an.taps(0)["frame_index"] == 0
    an.push_hops(np.ascontiguousarray(x[:, 2:3]))
    an.request_taps([1])
    an.reset_state()
    with pytest.raises(gpu_fx.FxError):
        an.taps(0)
    an.push_hops(np.ascontiguousarray(x[:, 3:4]))
    assert all(l["kind"] != "taps" for l in an.last_launches())
    with pytest.raises(gpu_fx.FxError):
        an.taps(1)
    an.request_taps([1])
    an.push_hops(np.ascontiguousarray(x[:, 4:6]))
    assert an.taps(1)["frame_index"] == 1
    an.close()


def test_argument_validation(gpu_fx):
    an = gpu_fx.BatchAnalyser(70, 256)
    for bad in ([-1], [70], list(range(65))):
        with pytest.raises(gpu_fx.FxError) as e:
            an.request_taps(bad)
        assert e.value.code == gpu_fx.capi.FX_ERR_INVALID_ARGUMENT
    an.request_taps(list(range(40)))
    with pytest.raises(gpu_fx.FxError):
        an.request_taps(list(range(30, 70)))        # 70 distinct armed channels
    an.request_taps(list(range(30, 64)))            # 64: the limit
    x = np.zeros((70, 1, 128), np.float32)
    an.push_hops(x)
    assert an.last_launches()[0] == _taps_record(256, 64)
    assert an.taps(63)["frame_index"] == 0
    with pytest.raises(gpu_fx.FxError):
        an.taps(64)
    an.close()
