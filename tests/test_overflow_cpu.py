"""The overflow cases (tests/overflow_cases.py) on the CPU, by the oracle alone: the regimes the module describes exist at every size, the
mask of undefined slot-frames is as small as the reference's out-of-bounds read makes it, the bad hops really move onsets, a gain reaches
the same place as samples scaled beforehand, and the oracle equals the reference's own headers wherever those define an answer (recorded
in tests/golden/overflow/cases.npz by tests/golden/make_overflow_cases.py).  These are the conditions that keep
tests/test_gpu_overflow.py honest: it holds the kernels to the oracle on the same cases."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import overflow_cases as oc  # noqa: E402
from rate_cases import same_bits  # noqa: E402
from refdiff_record import Replay  # noqa: E402

refdiff = Replay(os.path.join(ROOT, "tests", "golden", "overflow", "cases.npz"))

ONSET, RMS, F0, CENTROID, SPREAD, FLATNESS, LER, FLUX, SLOPE = range(9)
GAIN_LEVELS = (8.0, 9.5, 19.0, 36.0)
HALF = oc.T // 2

# Frames whose raw f0 is not the full-scale twin's although the level lies below the band.  10^e is no power of two, so the scaled samples
# are rounded once more and a frame whose lag search rests on a near-tie of two cnd values answers a neighbouring lag (one lag up or down
# at e <= 5: only the low tones, whose valleys are that flat, and only from 2048 points on); at 1e7 the low tones from 1024 points on
# are inside the overflow band already (the longer the window, the larger the autocorrelation's squares).  Everywhere else f0 is the
# twin's bit for bit; the count per (size, base, e) is held exactly.
LOUD_F0_MOVES = {(1024, "low_tones", 7.0): 3, (2048, "low_tones", 2.0): 1, (2048, "low_tones", 7.0): 14,
                 (4096, "low_tones", 2.0): 2, (4096, "low_tones", 3.0): 2, (4096, "low_tones", 5.0): 2, (4096, "low_tones", 7.0): 23}


def _channel(N, b, e):
    (i,) = oc.channels(N, b, e)
    return i


@pytest.mark.parametrize("N", oc.SIZES)
def test_inputs_are_the_recorded_ones_and_only_overflowing_channels_are_dropped(N):
    hops, labels = oc.hops(N), oc.labels(N)
    assert hops.shape == (len(labels), oc.T, N // 2) and oc.crc(N) == oc.CRC[N]
    for b in oc.BASES:
        for e in oc.LEVELS:
            finite = bool(np.isfinite(oc.scaled(oc.full_scale(N, b), e)).all())
            assert ((b, e) in labels) == finite, (N, b, e)
            if finite:
                assert same_bits(hops[_channel(N, b, e)], oc.scaled(oc.full_scale(N, b), e)).all()
    assert all(e == 38.0 for _, e in oc.overflowing(N))
    for i, (kind, e) in enumerate(labels):                          # non-finite samples: the transients' bad values and nothing else
        if kind in ("tone_bad", "bursts_bad"):
            value, position = e.split("@")
            twin = oc.clean(N)[0 if kind == "tone_bad" else 1]
            differ = np.argwhere(~same_bits(hops[i], twin))
            hop_set = {0} if position == "first" else set(oc.BAD_HOPS)
            assert {int(t) for t, _ in differ} == hop_set and len(differ) == len(hop_set) * (N // 2 if position == "hop" else 1)
            assert all(same_bits(hops[i][t, s], oc.bad_value(value)) for t, s in differ)
        else:
            assert np.isfinite(hops[i]).all(), (N, kind, e)
    for k, (kind, idx) in enumerate(oc.clean_channels(N).items()):
        assert len(idx) >= 2 and all(np.array_equal(hops[i], oc.clean(N)[k]) for i in idx), kind


@pytest.mark.parametrize("N", oc.SIZES)
def test_the_regimes_exist(oracle, N):
    raw, _ = oc.oracle_run(oracle, N)
    nyq_f0 = np.float32(-2.0 * 24000.0 / 5000.0)
    twin = {b: oracle.push_hops(oc.full_scale(N, b)[None], N)[0][0] for b in oc.BASES}
    # LOUD: the serial flatness product overflows -- in every frame from 1e5 on, and for the tone and the noise at every loud level (from
    # the second frame on: the first window is half silence); the low tones' product is tiny and crosses the edge between 1e2 and 1e3, so
    # some of their channels hold finite and inf frames side by side.  Everything else is finite, and f0 is the full-scale twin's bits.
    for b in oc.BASES:
        for e in oc.LOUD:
            r = raw[_channel(N, b, e)]
            overflowed = np.isposinf(r[:, FLATNESS])
            assert overflowed.any() and (r[:, FLATNESS] > 0).all() and (r[:, F0] > 0).all(), (N, b, e)
            assert overflowed[1 if e < 5.0 else 0:].all() or (b == "low_tones" and e < 5.0), (N, b, e)
            assert np.isfinite(np.delete(r, FLATNESS, axis=1)).all(), (N, b, e)
            moved = int((~same_bits(r[:, F0], twin[b][:, F0])).sum())
            assert moved == LOUD_F0_MOVES.get((N, b, e), 0), (N, b, e, moved)
    # BAND: per base a level whose f0 stays > 0 and differs from full scale's in at least half of the frames, and one with lag -1 in
    # at least half
    for b in oc.BASES:
        moving, gone = [], []
        for e in oc.BAND:
            f0 = raw[_channel(N, b, e)][:, F0]
            if (f0 > 0).all() and int((f0 != twin[b][:, F0]).sum()) >= HALF:
                moving.append(e)
            if int((f0 <= 0).sum()) >= HALF:
                gone.append(e)
                assert (f0[f0 <= 0] == nyq_f0).all()
        print("N=%d %s: f0 > 0 and moved in at least %d frames at 1e%s; lag -1 in at least %d frames at 1e%s" % (N, b, HALF, moving, HALF, gone))
        assert moving and gone, (N, b, moving, gone)
        assert int((raw[_channel(N, b, 11.0)][:, F0] == nyq_f0).sum()) >= oc.T - 1 and (raw[_channel(N, b, 18.5)][:, F0] == nyq_f0).all()
    # RMS edge: a channel whose non-finite raw slots are the RMS and at most the flatness besides
    edge = []
    for b in oc.BASES:
        for e in oc.RMS_EDGE:
            r = raw[_channel(N, b, e)]
            if np.isposinf(r[:, RMS]).all() and np.isfinite(np.delete(r, [RMS, FLATNESS], axis=1)).all():
                edge.append((b, e))
    assert edge, N
    assert all(np.isfinite(raw[_channel(N, b, 18.5)][:, RMS]).all() for b in oc.BASES)
    # HIGH: flux inf
    for b in oc.BASES:
        for e in oc.HIGH:
            assert np.isposinf(raw[_channel(N, b, e)][:, FLUX]).all(), (N, b, e)
    # transform overflow: centroid, spread or slope NaN somewhere
    assert any(np.isnan(raw[i][:, [CENTROID, SPREAD, SLOPE]]).any() for e in oc.TRANSFORM for i in oc.channels(N, None, e)), N
    # the walks pass through the band and out of it, in both directions
    (fi,), (fo_,) = oc.channels(N, "fade_in"), oc.channels(N, "fade_out")
    for i, first, last in ((fi, 0, oc.T - 1), (fo_, oc.T - 1, 0)):
        assert raw[i, first, F0] > 0 and raw[i, last, F0] == nyq_f0 and np.isfinite(np.delete(raw[i, first], FLATNESS)).all()


@pytest.mark.parametrize("N", oc.SIZES)
def test_the_mask_is_bounded(oracle, N):
    raw, sm = oc.oracle_run(oracle, N)
    labels = oc.labels(N)
    for mask in oc.defined(raw):
        assert mask.shape == raw.shape and mask[:, :, :9].all()
        for b in oc.BASES:
            for e in oc.LOUD:
                assert mask[_channel(N, b, e)].all()
        for idx in oc.clean_channels(N).values():
            assert mask[idx].all()
        for i in oc.transients(N):
            assert ((~mask[i]).sum(axis=0) <= 2 * 2 + 2 * 9 + 2).all(), oc.label_id(labels[i])
    mraw, msm = oc.defined(raw)
    for i in oc.transients(N):                                      # recovery is really observed, raw and smoothed
        after = oc.last_bad_frame(labels[i]) + 1
        for mask, out in ((mraw, raw), (msm, sm)):
            ok = mask[i, after:][:, list(oc.HARMONIC_SLOTS)].all(axis=1)
            assert int(ok.sum()) >= 4, (N, oc.label_id(labels[i]), int(ok.sum()))
            assert np.isfinite(out[i, after:][ok][:, list(oc.HARMONIC_SLOTS)]).all(), (N, oc.label_id(labels[i]))
    # the mask is what it says: undefined raw iff f0 is not > 0, smoothed iff any of the last ten frames is
    bad = ~(raw[:, :, F0] > 0)
    for s in oc.HARMONIC_SLOTS:
        assert np.array_equal(~mraw[:, :, s], bad)
        for t in range(oc.T):
            assert np.array_equal(~msm[:, t, s], bad[:, max(0, t - 9):t + 1].any(axis=1))


@pytest.mark.parametrize("N", oc.SIZES)
@pytest.mark.parametrize("onset_type", [0, 1, 2])
def test_onsets_are_really_exercised(oracle, onset_type, N):
    """the bad hops both create an onset the clean bursts channel lacks and delete one it has, for every onset type"""
    on = oc.oracle_run(oracle, N, onset_type=onset_type, onset_sensitivity=0.2, onset_window=5)[0][:, :, ONSET] > 0
    clean = on[oc.channels(N, "clean_bursts")[0]]
    bad = on[oc.channels(N, "bursts_bad")]
    gained, lost = (bad & ~clean).any(axis=1), (clean & ~bad).any(axis=1)
    print("N=%d type %d: clean onsets at %s; %d twins gain an onset, %d lose one" % (N, onset_type, np.nonzero(clean)[0], gained.sum(), lost.sum()))
    assert gained.any() and lost.any()


@pytest.mark.parametrize("N", oc.SIZES)
def test_gain_reaches_the_same_place(oracle, N):
    """full-scale samples under gain 10^e (a float) equal the samples scaled beforehand under gain 1, bit for bit"""
    want = oc.oracle_run(oracle, N)
    for b in oc.BASES:
        for e in GAIN_LEVELS:
            got = oracle.push_hops(oc.full_scale(N, b)[None], N, gain=float(np.float32(10.0 ** e)))
            for k in (0, 1):
                assert same_bits(got[k][0], want[k][_channel(N, b, e)]).all(), (N, b, e, ("raw", "smoothed")[k])


@pytest.mark.parametrize("N", oc.SIZES)
def test_one_bad_sample_stays_in_the_smoothed_rms_for_6_or_11_frames(oracle, N):
    """a NaN in the stream's first sample: raw RMS non-finite in frames 0 and 1; smoothed RMS non-finite in frames 0..5 where the two
    analysers share their features (both write the RMS slot, so its 10-entry history holds five frames) and in frames 0..10 where each
    has its own -- then finite again"""
    (i,) = oc.channels(N, "tone_bad", "nan@first")
    hops = oc.hops(N)[i:i + 1]
    for order, frames in ((0, 6), (1, 6), (2, 11)):
        raw, sm = oracle.push_hops(hops, N, order=order)
        assert np.array_equal(np.flatnonzero(~np.isfinite(raw[0, :, RMS])), [0, 1])
        assert np.array_equal(np.flatnonzero(~np.isfinite(sm[0, :, RMS])), np.arange(frames)), (N, order)


@pytest.mark.parametrize("N", [1024, 4096])
def test_taps_model_reproduces_the_oracles_buffers(oracle, N):
    """tests/taps_model.py restates the display buffers from the oracle's building blocks; for the windows whose taps
    tests/test_gpu_overflow.py takes -- overflowing squares, 0 * inf under the Bartlett window, bins that overflow inside the transforms
    -- its autocorrelation gives the oracle's own cnd, and its lag walk the lag behind the oracle's raw f0"""
    import taps_model
    raw = oc.oracle_run(oracle, N)[0]
    seen_nan = False
    for c in oc.tap_channels(N):
        window = oc.tap_window(N, c)
        taps = taps_model.oracle_taps(oracle, window)
        pitch = oracle.forward_real(oracle.bartlett(oracle.lowpass(window)))
        f0, lag, cnd = oracle.estimate_pitch(pitch)
        assert same_bits(taps_model.cnd_from(taps_model.autocorrelation(oracle, pitch)), cnd).all()
        assert same_bits(taps["cnd"], cnd[:N]).all() and same_bits(np.float32(f0 / 5000.0), raw[c, oc.TAP_FRAME, F0])
        x = taps["lag_position"][0] * np.float32(2 * N)
        assert x == lag if x >= 0 else not (cnd[2:N] < np.float32(0.01)).any()
        seen_nan |= bool(np.isnan(taps["cnd"]).any())
        if c == oc.channels(N, "tone_bad", "+inf@0")[0]:
            assert np.isposinf(window[0]) and np.isnan(oracle.bartlett(window)[0])             # 0 * inf
    assert seen_nan


# ---- the reference's own headers (tools/refdiff, log10(float) correctly rounded), from the record ----
def defined_everywhere(raw):
    """the channels whose raw f0 is > 0 in every frame: the reference never reads out of bounds there"""
    return [i for i in range(raw.shape[0]) if (raw[i, :, F0] > 0).all()]


@pytest.mark.parametrize("N", oc.SIZES)
def test_oracle_is_bit_identical_to_the_reference_headers_where_f0_is_positive(oracle, N):
    """both analysers, every channel whose f0 > 0 in every frame (the loud ladder, the band levels that keep a lag, the 1e12 transients,
    the clean channels): every raw and smoothed value"""
    oraw, osm = oc.oracle_run(oracle, N)
    keep = defined_everywhere(oraw)
    assert len(keep) >= 30 and all(oc.channels(N, b, e)[0] in keep for b in ("tone", "loud_noise") for e in oc.LOUD)
    raw, sm = refdiff.run(np.ascontiguousarray(oc.hops(N)[keep]), N, mode="cr")
    assert same_bits(raw, oraw[keep]).all(), "raw differs at %s" % (np.argwhere(~same_bits(raw, oraw[keep]))[:5],)
    assert same_bits(sm, osm[keep]).all(), "smoothed differs at %s" % (np.argwhere(~same_bits(sm, osm[keep]))[:5],)


@pytest.mark.parametrize("N", oc.SIZES)
def test_oracle_is_bit_identical_to_the_reference_spectral_analyser_on_every_channel(oracle, N):
    """the spectral analyser alone reads nothing out of bounds: every channel, the transients and the transform-overflow levels included"""
    raw, sm = refdiff.run(np.ascontiguousarray(oc.hops(N)), N, mode="cr", analysers=1)
    oraw, osm = oc.oracle_run(oracle, N, analysers=1)
    assert same_bits(raw, oraw).all(), "raw differs at %s" % (np.argwhere(~same_bits(raw, oraw))[:5],)
    assert same_bits(sm, osm).all(), "smoothed differs at %s" % (np.argwhere(~same_bits(sm, osm))[:5],)
