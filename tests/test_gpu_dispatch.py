"""Every analysis dispatch path of tests/dispatch_paths.py on the device: a stream of calls through the row's entry point and configuration,
long enough (more than HLEN = 48 hops, at least three calls) that the smoothing ring, an onset window of 21 and the flux state are carried
across calls.  For each call: (a) the launches it made (fx_last_launches_internal) are the row's; (b) its raw and smoothed vectors are the
oracle's -- onsets exactly, the other slots within the default family's ulp budget (oracle/ulp.py; FX_LOW_LATENCY rows: that family's);
(c) they are, bit for bit, what one fx_push_hops call over all of the stream's frames gives with default tuning (fx_process_frames for rows
of pre-assembled windows); (d) the smoothed vectors and the onset column are, bit for bit, what the reference's tail makes of the raw
stream (tests/tail_model.py), every channel.  Across the table: no epilogue is asked to write
strided rows for more than one frame, and fx_last_kernel_ms answers as include/fx.h says (every call with call_timing = 1; by default
exactly the calls whose launches analyse more than one frame each).  Ring steps are outside fx_last_kernel_ms' contract."""
import numpy as np
import pytest

import dispatch_paths as dp
import signals
import tail_model

pytestmark = pytest.mark.gpu

ONSET_WINDOW = 21
MASKS = {"both": 3, "spectral": 1, "harmonic": 2}
SCALE = {"f32": None, "s16": 32768.0}
ORACLE_CHANNELS = 8                 # rows of many channels: the oracle checks a spread of this many (bit-exact to the baseline: all of them)


@pytest.fixture(scope="module")
def cus(gpu_fx):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _as_format(x, fmt):
    if fmt == "s16":
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return x


def _floats(x, fmt):
    return x.astype(np.float32) / np.float32(SCALE[fmt]) if SCALE[fmt] else x


def _analyser(gpu_fx, r, call_timing=None):
    an = gpu_fx.BatchAnalyser(r.C, r.N, analysers=r.analysers, low_latency=r.low_latency)
    an.set_onset_window_length(ONSET_WINDOW)
    knobs = dict(r.tuning)
    if call_timing is not None:
        knobs["call_timing"] = call_timing
    if knobs:
        an.set_tuning(**knobs)
    if r.hooks:
        an.set_test_hooks(r.hooks)
    return an


def _plan(r):
    """the row's stream ([C][hops][N/2], in the row's sample format) and the pieces its calls take, in order"""
    H = r.N // 2
    if r.entry == "samples":
        first, then = r.per
        lengths = [first] + [then] * (r.calls - 1)
        total = sum(lengths)
        hops = total // H
        x = dp.stream(r.C, hops + 1, r.N, seed=r.N).reshape(r.C, -1)[:, :total]
        x = _as_format(x, r.fmt)
        pieces, at = [], 0
        for n in lengths:
            pieces.append(np.ascontiguousarray(x[:, at:at + n]))
            at += n
        return np.ascontiguousarray(x[:, :hops * H].reshape(r.C, hops, H)), pieces
    hops = _as_format(dp.stream(r.C, r.per * r.calls, r.N, seed=r.N), r.fmt)
    feed = _windows(hops) if r.entry == "frames" else hops
    return hops, [np.ascontiguousarray(feed[:, t:t + r.per]) for t in range(0, hops.shape[1], r.per)]


def _windows(hops):
    """[C][T][N] 50 %-overlap windows of a hop stream that is silent before its first hop"""
    C, T, H = hops.shape
    x = np.concatenate([np.zeros((C, 1, H), hops.dtype), hops], axis=1)
    return np.ascontiguousarray(np.concatenate([x[:, :-1], x[:, 1:]], axis=2))


def _call(an, r, piece):
    if r.entry == "hops":
        return an.push_hops(piece)
    if r.entry == "frames":
        return an.process_frames(piece)
    return an.push_samples(piece)


def _run_calls(gpu_fx, an, r, pieces):
    """every call of the row on `an`: the vectors, the launch record of each call, whether fx_last_kernel_ms answered after it"""
    outs, records, timed = [], [], []
    for piece in pieces:
        out = _call(an, r, piece)
        records.append(an.last_launches())
        outs.append(out)
        try:
            an.last_kernel_ms()
            timed.append(True)
        except gpu_fx.FxError:
            timed.append(False)
    return outs, records, timed


def _run_ring(gpu_fx, an, r, pieces):
    st = gpu_fx.HopStream(an, r.per, slots=3, dtype=pieces[0].dtype)
    outs, records = [], []
    for piece in pieces:
        if st.in_flight() == 2:
            outs.append(st.collect())
        st.push(piece)
        records.append(an.last_launches())
    while st.in_flight():
        outs.append(st.collect())
    st.close()
    return outs, records


def _check_launches(r, records, frames):
    seen = set()
    for i, (rec, t) in enumerate(zip(records, frames)):
        assert t in r.expect, "%s call %d analysed %d frames per channel; the row declares %s" % (r.id, i, t, sorted(r.expect))
        assert rec == r.expect[t], "%s call %d (%d frames):\n  launched %s\n  expected %s" % (r.id, i, t, rec, r.expect[t])
        for launch in rec:
            assert not (launch["out_stride"] != 0 and launch["ep_T"] != 1), (r.id, i, launch)
        seen.add(t)
    assert seen == set(r.expect), "%s: the stream never made calls of %s frames" % (r.id, sorted(set(r.expect) - seen))


@pytest.mark.parametrize("r", dp.ROWS, ids=[r.id for r in dp.ROWS])
def test_dispatch_path(gpu_fx, oracle, cus, r):
    if cus != dp.CUS:
        pytest.skip("the table's launch sequences are written for %d CUs; this device reports %d" % (dp.CUS, cus))
    hops, pieces = _plan(r)
    assert len(pieces) >= 3 and hops.shape[1] > 48, (len(pieces), hops.shape)
    an = _analyser(gpu_fx, r)
    if r.entry == "ring":
        outs, records = _run_ring(gpu_fx, an, r, pieces)
        timed = None
    else:
        outs, records, timed = _run_calls(gpu_fx, an, r, pieces)
    an.close()
    frames = [o[0].shape[1] for o in outs]
    assert sum(frames) == hops.shape[1], (r.id, frames)
    # (a) the launches
    _check_launches(r, records, frames)
    raw = np.concatenate([o[0] for o in outs], axis=1)
    sm = np.concatenate([o[1] for o in outs], axis=1)
    # (c) bit for bit one call over the whole stream, default tuning
    base = gpu_fx.BatchAnalyser(r.C, r.N, analysers=r.analysers, low_latency=r.low_latency)
    base.set_onset_window_length(ONSET_WINDOW)
    want = base.process_frames(_windows(hops)) if r.entry == "frames" else base.push_hops(hops)
    base.close()
    assert np.array_equal(raw, want[0], equal_nan=True), "%s: raw vectors differ from one fx_push_hops call" % r.id
    assert np.array_equal(sm, want[1], equal_nan=True), "%s: smoothed vectors differ from one fx_push_hops call" % r.id
    # (b) the oracle
    sel = np.unique(np.linspace(0, r.C - 1, min(r.C, ORACLE_CHANNELS)).astype(int))
    x = _floats(hops[sel], r.fmt)
    settings = dict(onset_window=ONSET_WINDOW, analysers=MASKS[r.analysers])
    oraw, osm = oracle.process_frames(_windows(x), r.N, **settings) if r.entry == "frames" else oracle.push_hops(x, r.N, **settings)
    budget = signals.ulp_budget("low_latency" if r.low_latency else "default")
    signals.assert_features_within(raw[sel], oraw, budget, oracle.FEATURE_NAMES, r.id + " raw")
    signals.assert_features_within(sm[sel], osm, budget, oracle.FEATURE_NAMES, r.id + " smoothed")
    # (d) the tail, exactly
    tail_model.assert_tail_exact(raw, sm, [(0, "onset_window", ONSET_WINDOW)], analysers=MASKS[r.analysers], what=r.id)
    if timed is None:
        return
    # fx_last_kernel_ms: by default exactly the calls include/fx.h names; with call_timing = 1 every call that analysed frames
    for i, (rec, t, ok) in enumerate(zip(records, frames, timed)):
        if t:
            assert ok == dp.timed_by_default(rec), (r.id, i, rec, ok)
    an = _analyser(gpu_fx, r, call_timing=1)
    _, records1, timed1 = _run_calls(gpu_fx, an, r, pieces[:4])
    an.close()
    assert records1 == records[:4], r.id
    for i, (t, ok) in enumerate(zip(frames[:4], timed1)):
        if t:
            assert ok, (r.id, i, "call_timing = 1 and no timing")
