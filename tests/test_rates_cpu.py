"""The sample rate's rounding edges on the CPU: the rate cases (tests/rate_cases.py) really sit on them, the oracle equals the reference's
own headers there bit for bit at all ten rates (recorded in tests/golden/rates/cases.npz by tests/golden/make_rate_cases.py), and the
oracle is invariant under a power-of-two change of rate.  tests/test_gpu_rates.py holds the kernels to the oracle on the same cases."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import rate_cases as rc  # noqa: E402
from refdiff_record import Replay  # noqa: E402

refdiff = Replay(os.path.join(ROOT, "tests", "golden", "rates", "cases.npz"))

F0, INHARM = 2, 11
# (size, rate) pairs at which no input was found within bounded search: none
EXEMPT = ()


def edge_frames(raw, raw48, rate):
    """frames whose raw inharmonicity differs from the 48 kHz run by more than 1e-4 relative while the lag is equal"""
    a, b = raw[:, :, INHARM].astype(np.float64), raw48[:, :, INHARM].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(a - b) / np.abs(b)
    return (rc.lags(raw, rate) == rc.lags(raw48, 48000.0)) & (rel > 1e-4)


@pytest.mark.parametrize("N", rc.EDGE_SIZES)
def test_rate_cases_sit_on_the_edges(oracle, N):
    """The selection condition, on the inputs and by the oracle alone: for every rate that is not a power of two times 48 kHz at least
    one frame's raw inharmonicity differs from the 48 kHz run by more than 1e-4 relative while its lag is the same.  The count per
    (size, rate) is printed.  192 kHz = 4 x 48 kHz can never meet it (scaling by four is exact): there the opposite is held, every
    bit equal but F0's (test_oracle_power_of_two_invariance)."""
    assert len(EXEMPT) <= 4 and all(n != 1024 for n, _ in EXEMPT)
    raw48 = rc.oracle_run(oracle, N, 48000.0)[0]
    for rate in rc.EDGE_RATES:
        count = int(edge_frames(rc.oracle_run(oracle, N, rate)[0], raw48, rate).sum())
        print("N=%d rate=%s: %d of %d frames on an edge" % (N, rc.rate_id(rate), count, rc.C * rc.T))
        if (N, rate) not in EXEMPT:
            assert count >= 1, (N, rate)
    raw192 = rc.oracle_run(oracle, N, 192000.0)[0]
    assert int(edge_frames(raw192, raw48, 192000.0).sum()) == 0 and np.array_equal(rc.lags(raw192, 192000.0), rc.lags(raw48, 48000.0))


@pytest.mark.parametrize("N", rc.SIZES)
def test_oracle_power_of_two_invariance(oracle, N):
    """24, 48, 96 and 192 kHz: every expression the rate enters scales exactly (1 / nyquist included), so raw and smoothed vectors
    are bit-identical but for F0, which is exactly halved / doubled / quadrupled (a power of two times a float: exact, the smoothed
    value too, since its filter is linear in exact scalings)"""
    rc.assert_power_of_two_invariant(lambda rate: rc.oracle_run(oracle, N, rate), "oracle N=%d" % N)


REFERENCE_FRAMES = 12            # the record holds the first hops of each case: a frame's value does not depend on those after it


@pytest.mark.parametrize("N", rc.SIZES)
@pytest.mark.parametrize("rate", rc.RATES, ids=[rc.rate_id(r) for r in rc.RATES])
def test_oracle_is_bit_identical_to_the_reference_headers_at_every_rate(oracle, N, rate):
    """the reference's own headers (tools/refdiff, log10(float) correctly rounded) on the rate cases: every raw and smoothed value"""
    hops = np.ascontiguousarray(rc.hops(N, frames=REFERENCE_FRAMES))
    raw, sm = refdiff.run(hops, N, sample_rate=rate, mode="cr")
    oraw, osm = rc.oracle_run(oracle, N, rate)
    oraw, osm = oraw[:, :REFERENCE_FRAMES], osm[:, :REFERENCE_FRAMES]
    assert rc.same_bits(raw, oraw).all(), "raw differs at %s" % (np.argwhere(~rc.same_bits(raw, oraw))[:5],)
    assert rc.same_bits(sm, osm).all(), "smoothed differs at %s" % (np.argwhere(~rc.same_bits(sm, osm))[:5],)


def test_reference_collector_with_the_rate_changed_mid_stream(oracle):
    """the reference's own collector and analysers with sampleRateChanged between blocks (to a non-dyadic rate and back) against the
    oracle with the same setter calls: the event list the GPU's mid-stream test uses"""
    N, Cn = 1024, 3
    hops = np.ascontiguousarray(rc.hops(N, channels=Cn))
    H = N // 2
    events = [(8 * H, "sample_rate", rc.MID_STREAM_RATE), (16 * H, "sample_rate", 48000.0)]
    raw, sm = refdiff.run_blocks(hops.reshape(Cn, -1), N, H, order=0, events=events)
    oraw, osm = rc.oracle_with_rate_events(oracle, hops, N, [(8, rc.MID_STREAM_RATE), (16, 48000.0)])
    assert rc.same_bits(raw, oraw).all() and rc.same_bits(sm, osm).all()
