"""What the library derives from a feature buffer on the GPU (include/fx.h: fx_offline_feature_ranges, fx_offline_feature_distribution,
fx_offline_smoothing / fx_offline_smooth_rows / fx_offline_get_smoothing) against the tests' model (tests/offline_stats_model.py, itself
held to the reference's unmodified header by tests/test_offline_stats_cpu.py) and, where it has the case, against the header's own results
(tests/golden/offline/feature_stats.npz): bit for bit, a NaN equal to any NaN.  C = 3 channels and two or three rows of different data, so
that a mixed-up row or channel shows."""
import ctypes
import os
import sys

import numpy as np
import pytest

import offline_stats_model as model
from offline_stats_model import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_feature_stats_cases import feature_stats_inputs, wide_magnitudes  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "offline", "feature_stats.npz")
C = 3
F32 = np.float32
CHUNK = model.SORT_CHUNK


@pytest.fixture(scope="module")
def an(gpu_fx):
    assert gpu_fx.capi.OFFLINE_SORT_CHUNK == CHUNK and gpu_fx.capi.OFFLINE_SCRATCH_BYTES == model.SCRATCH_BYTES
    a = gpu_fx.offline.AudioAnalyser(C)
    yield a
    a.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN), feature_stats_inputs()


# ---- ranges ----
def range_rows(D, seed):
    """[3][C][D]: noise, with the corner cases of the comparison chain in the rows that are long enough to hold them"""
    rng = np.random.default_rng(seed)
    rows = rng.normal(0, 1, (3, C, D)).astype(F32)
    a, b = D // 3, D - 1                                                 # two places a wave or more apart in the long rows
    rows[0, 1, 0] = np.nan                                               # a NaN at row[0]: both ends for ever
    if D >= 2:
        rows[0, 2, [D // 2, b]] = np.nan                                 # NaNs elsewhere: stepped over
        rows[2, 0, D // 2] = np.inf; rows[2, 0, b] = -np.inf
        rows[2, 1, b] = -50.0                                            # the minimum at the last index
        rows[2, 2, b] = 50.0
    if D >= 3 and a != b:
        rows[1, 0] = np.abs(rows[1, 0]) + 1; rows[1, 0, a] = -0.0; rows[1, 0, b] = 0.0      # zero minimum: -0 first
        rows[1, 1] = np.abs(rows[1, 1]) + 1; rows[1, 1, a] = 0.0; rows[1, 1, b] = -0.0      # ... +0 first
        rows[1, 2] = -np.abs(rows[1, 2]) - 1; rows[1, 2, 0] = 0.0; rows[1, 2, b] = -0.0     # zero maximum, at row[0] and behind
    return rows


@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 257, 1000])
def test_ranges_equal_the_model(an, D):
    rows = range_rows(D, 100 + D)
    got = an.feature_ranges(rows)
    assert got.shape == (3, C, 2) and same(got, model.feature_ranges(rows)), (got, model.feature_ranges(rows))
    if D >= 3:
        assert got[1, 0, 0].view(np.uint32) == 0x80000000 and got[1, 1, 0].view(np.uint32) == 0 and got[1, 2, 1].view(np.uint32) == 0
    assert np.isnan(got[0, 1]).all()
    flipped = np.ascontiguousarray(rows[::-1, ::-1])                     # other rows and channels in the same places
    assert same(an.feature_ranges(flipped), np.ascontiguousarray(got[::-1, ::-1]))


def test_ranges_equal_the_reference_header(an, golden):
    g, cases = golden
    for k, row in enumerate(cases["ranges"]):
        rows = np.stack([np.ones_like(row), row, -np.ones_like(row)])[None]          # the case between two other channels
        got = an.feature_ranges(rows)
        assert same(got[0, 1], g["range_%d" % k]), (k, got, g["range_%d" % k])
        assert same(got[0, 0], np.array([1, 1], F32)) and same(got[0, 2], np.array([-1, -1], F32))


# ---- distributions ----
def distribution_rows(D, seed):
    """[3][C][D], nine kinds of data"""
    rng = np.random.default_rng(seed)
    noise = rng.normal(0, 1, (9, D)).astype(F32)
    rows = noise.copy()
    rows[1] = (np.floor(rng.uniform(0, 8, D)) / 8 - 0.5).astype(F32)                 # 8 levels: long runs of ties
    rows[2] = np.sort(noise[2])                                                      # already sorted
    rows[3] = np.sort(noise[3])[::-1]                                                # reversed
    rows[4] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], F32), D)                   # a mix of +-0
    rows[5, rng.integers(0, D, 3)] = np.inf; rows[5, rng.integers(0, D, 2)] = -np.inf
    rows[6, ::3] = (rng.integers(-200, 200, len(rows[6, ::3])) * F32(1e-45)).astype(F32)     # subnormals beside normals
    rows[7] = wide_magnitudes(rng, D)                                                # 1e-8 .. 1e8: the summation order shows
    rows[8, rng.integers(0, D, 1 + D // 50)] = np.nan                                # NaNs (ours: behind +inf) ...
    rows[8, rng.integers(0, D)] = np.frombuffer(np.uint32(0xFFC00001).tobytes(), F32)[0]     # ... whatever their sign
    return rows.reshape(3, C, D)


@pytest.mark.parametrize("D", [1, 2, 7, 64, 65, 1000, 1024, 1025, CHUNK - 1, CHUNK, CHUNK + 3, 2 * CHUNK + 5])
def test_distributions_equal_the_model(an, D):
    rows = distribution_rows(D, 200 + D)
    for nb in (1, 3, 10, D, D + 1):
        got, want = an.discrete_feature_distribution(rows, nb), model.distributions(rows, nb)
        assert got.shape == (3, C, nb) and same(got, want), (D, nb, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])
    assert np.isnan(an.discrete_feature_distribution(rows, D + 1)).all()             # step 0: 0.0f / 0.0f in every bracket
    if D >= 1000:                                                                    # the cases discriminate: a tree sum is another result
        assert not same(model.distributions(rows[2, 1], 3, model.pairwise_sums), model.distributions(rows[2, 1], 3))


def test_distributions_equal_the_reference_header(an, golden):
    g, cases = golden
    for k, (row, nb) in enumerate(cases["distributions"]):
        rows = np.stack([row[::-1], row, np.roll(row, 1)])[None]                     # the same values in three orders: one distribution
        got = an.discrete_feature_distribution(rows, nb)
        for c in range(C):
            assert same(got[0, c], g["dist_%d" % k]), (k, c)


def test_distribution_groups_of_long_rows_meet_at_a_seam(an):
    """D = CHUNK + 3 = 8195 values are padded to P = 16384 keys = 64 KiB a row: the 16 MiB scratch holds 16 MiB / 64 KiB = 256 rows, so
    R x C = 86 x 3 = 258 rows (8.5 MB of input) are sorted as a group of 256 and a group of 2."""
    D, R = CHUNK + 3, 86
    P = 1 << (D - 1).bit_length()
    assert P == 16384 and model.SCRATCH_BYTES // (4 * P) == 256 < R * C
    rows = np.random.default_rng(77).normal(0, 1, (R, C, D)).astype(F32)
    rows[85, 1] = wide_magnitudes(np.random.default_rng(78), D)                      # row 256: the first of the second group
    rows[85, 0, 5] = np.nan                                                          # row 255: the last of the first
    got, want = an.discrete_feature_distribution(rows, 10), model.distributions(rows, 10)
    assert same(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    assert same(an.discrete_feature_distribution(rows[80:], 10), got[80:])           # the same rows inside one group: the same bits


# ---- smoothing ----
def smoothing_rows(D=40, seed=5):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (10, C, D)) * 10.0 ** rng.integers(-3, 4, (10, C, 1))).astype(F32)


@pytest.mark.parametrize("depth", [1, 2, 10, 64])
def test_smoothing_equals_the_model_however_it_is_called(an, depth):
    rows = smoothing_rows()
    D = rows.shape[2]
    m = model.Smoothers(C, depth)
    want = m.smooth_rows(rows)
    an.smoothing(depth)
    whole = an.smooth_rows(rows)                                                     # count = D: one launch
    assert whole.shape == (9, C, D) and same(whole, want)
    current, history = an.smoothed_state()
    assert same(current, m.current) and same(history, m.history) and same(current, whole[:, :, -1])
    an.reset()                                                                       # fx_offline_reset is the analyser's: the smoothers stay
    assert all(same(a, b) for a, b in zip(an.smoothed_state(), (current, history)))
    again = an.smooth_rows(rows, first=3, count=5)                                   # the state carries on from call to call
    assert same(again, m.smooth_rows(rows, 3, 5)) and not same(again, whole[:, :, 3:8])
    an.smoothing(depth)                                                              # constructed anew: all zero
    current, history = an.smoothed_state()
    assert not current.any() and not history.any() and history.shape == (9, C, depth)
    singles = np.concatenate([an.smooth_rows(rows, first=i, count=1) for i in range(D)], axis=2)     # the reference's call, D times
    assert same(singles, whole)
    an.smoothing(depth)
    two = np.concatenate([an.smooth_rows(rows, 0, 17), an.smooth_rows(rows, 17)], axis=2)            # the state carries over two calls
    assert same(two, whole)
    an.smoothing(0)


def test_smoothing_equals_the_reference_header(an, golden):
    g, cases = golden
    for k, (depth, values) in enumerate(cases["smoothing"]):
        rows = np.zeros((9, C, len(values)), F32)
        rows[:, 1, :] = values.T                                                     # the case between two silent channels
        an.smoothing(depth)
        got = an.smooth_rows(rows)
        assert same(np.ascontiguousarray(got[:, 1, :].T), g["smooth_%d_current" % k]), k
        assert same(an.smoothed_state()[1][:, 1, :], g["smooth_%d_history" % k]) and not got[:, 0, :].any() and not got[:, 2, :].any()
    an.smoothing(0)


# ---- host and device buffers; the chain on the device ----
def test_device_buffers_give_the_same_bits(an):
    import torch
    for D in (1000, CHUNK + 3):
        rows = distribution_rows(D, 300 + D)
        dev = torch.from_numpy(rows).cuda()
        assert same(an.feature_ranges(dev), an.feature_ranges(rows))
        assert same(an.discrete_feature_distribution(dev, 10), an.discrete_feature_distribution(rows, 10))
    rows = smoothing_rows()
    an.smoothing(4)
    host = an.smooth_rows(rows)
    an.smoothing(4)
    assert same(an.smooth_rows(torch.from_numpy(rows).cuda()), host)
    an.smoothing(0)


def test_analysis_ranges_and_distributions_chain_on_the_device(gpu_fx):
    """fx_offline_analyse leaves its features in device memory; the ranges and distributions are taken from that buffer where it lies and
    equal the route through the host, and FeatureSpace.from_buffer is fed by them."""
    import torch
    fx, capi = gpu_fx, gpu_fx.capi
    lib = fx.load_library()
    S, D, N, nb = 6000, 24, 256, 5
    t = np.arange(S) / 48000.0
    audio = np.stack([np.sin(2 * np.pi * f * t) * np.exp(-3 * t * k) for k, f in enumerate((440.0, 1230.0, 3100.0))])
    audio = (audio + np.random.default_rng(4).normal(0, 0.05, (C, S))).astype(F32)
    host = fx.offline.AudioAnalyser(C)
    buf = host.perform_spectral_analysis(audio, D, N, 48000)
    ranges, dist = buf.feature_ranges(), np.stack([buf.get_discrete_feature_distribution(r, nb) for r in range(10)])
    assert same(ranges, model.feature_ranges(buf.feature_buffer)) and same(dist, model.distributions(buf.feature_buffer, nb))
    assert buf.feature_buffer[capi.OFFLINE_CENTROID].any() and buf.feature_buffer[capi.OFFLINE_ZERO_CROSSES].any()
    dev = fx.offline.AudioAnalyser(C)
    d_audio = torch.from_numpy(audio).cuda()
    what = 63
    features, lat = torch.empty((10, C, D), dtype=torch.float32, device="cuda"), torch.empty(C, dtype=torch.float32, device="cuda")
    d_ranges, d_dist = torch.empty((10, C, 2), dtype=torch.float32, device="cuda"), torch.empty((10, C, nb), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    capi.check(lib.fx_offline_analyse(dev._h, d_audio.data_ptr(), S, D, N, 48000, what, features.data_ptr(), None, lat.data_ptr(), None, capi.MEM_DEVICE))
    capi.check(lib.fx_offline_feature_ranges(dev._h, features.data_ptr(), 10, D, d_ranges.data_ptr(), capi.MEM_DEVICE))
    capi.check(lib.fx_offline_feature_distribution(dev._h, features.data_ptr(), 10, D, nb, d_dist.data_ptr(), capi.MEM_DEVICE))
    capi.check(lib.fx_offline_sync(dev._h))
    assert same(features.cpu().numpy(), buf.feature_buffer) and same(d_ranges.cpu().numpy(), ranges) and same(d_dist.cpu().numpy(), dist)
    for c in range(C):
        space = fx.offline.FeatureSpace.from_buffer(buf, c)
        want = model.FeatureSpace(buf.estimated_log_attack_time[c], *[model.Range(*ranges[r, c]) for r in (capi.OFFLINE_CENTROID, capi.OFFLINE_SLOPE, capi.OFFLINE_ZERO_CROSSES)])
        got = np.array([v for r in (space.attack_range, space.spectral_centroid_range, space.spectral_slope_range, space.zero_crosses_range) for v in r], F32)
        assert same(got, want.flat())
    host.close(); dev.close()


# ---- refusals ----
def test_every_refusal_names_its_value_and_launches_nothing(gpu_fx):
    import torch
    fx, capi = gpu_fx, gpu_fx.capi
    lib = fx.load_library()
    a = fx.offline.AudioAnalyser(C)
    R, D, nb = 2, 5, 2
    rows = torch.from_numpy(np.random.default_rng(9).normal(0, 1, (9, C, D)).astype(F32)).cuda()
    out_r = torch.full((R, C, 2), -7.0, dtype=torch.float32, device="cuda")
    out_d = torch.full((R, C, nb), -7.0, dtype=torch.float32, device="cuda")
    out_s = torch.full((9, C, D), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h, p, dev = a._h, rows.data_ptr(), capi.MEM_DEVICE
    a.smoothing(3)
    capi.check(lib.fx_offline_feature_ranges(h, p, R, D, out_r.data_ptr(), dev))
    capi.check(lib.fx_offline_feature_distribution(h, p, R, D, nb, out_d.data_ptr(), dev))
    capi.check(lib.fx_offline_smooth_rows(h, p, D, 0, D, out_s.data_ptr(), dev))
    capi.check(lib.fx_offline_sync(h))
    good = [t.cpu().numpy().copy() for t in (out_r, out_d, out_s)]
    state = a.smoothed_state()
    assert same(good[0], model.feature_ranges(rows.cpu().numpy()[:R])) and not (good[2] == -7).any()
    refused = [
        (lambda: lib.fx_offline_feature_ranges(h, None, R, D, out_r.data_ptr(), dev), b"null argument"),
        (lambda: lib.fx_offline_feature_ranges(h, p, R, D, None, dev), b"null argument"),
        (lambda: lib.fx_offline_feature_ranges(h, p, 0, D, out_r.data_ptr(), dev), b"num_rows 0"),
        (lambda: lib.fx_offline_feature_ranges(h, p, R, 0, out_r.data_ptr(), dev), b"num_downsamples 0"),
        (lambda: lib.fx_offline_feature_ranges(h, p, R, D, out_r.data_ptr(), 7), b"memory kind 7"),
        (lambda: lib.fx_offline_feature_distribution(h, None, R, D, nb, out_d.data_ptr(), dev), b"null argument"),
        (lambda: lib.fx_offline_feature_distribution(h, p, R, D, nb, None, dev), b"null argument"),
        (lambda: lib.fx_offline_feature_distribution(h, p, -1, D, nb, out_d.data_ptr(), dev), b"num_rows -1"),
        (lambda: lib.fx_offline_feature_distribution(h, p, R, 0, nb, out_d.data_ptr(), dev), b"num_downsamples 0"),
        (lambda: lib.fx_offline_feature_distribution(h, p, R, D, 0, out_d.data_ptr(), dev), b"num_brackets 0"),
        (lambda: lib.fx_offline_feature_distribution(h, p, R, D, nb, out_d.data_ptr(), 2), b"memory kind 2"),
        (lambda: lib.fx_offline_feature_distribution(h, p, R, (16 << 20) // 4 + 1, nb, out_d.data_ptr(), dev), b"num_downsamples 4194305"),
        (lambda: lib.fx_offline_smoothing(h, -1), b"depth -1"),
        (lambda: lib.fx_offline_smoothing(h, 65), b"depth 65"),
        (lambda: lib.fx_offline_smooth_rows(h, None, D, 0, 1, out_s.data_ptr(), dev), b"null argument"),
        (lambda: lib.fx_offline_smooth_rows(h, p, 0, 0, 1, out_s.data_ptr(), dev), b"num_downsamples 0"),
        (lambda: lib.fx_offline_smooth_rows(h, p, D, -1, 1, out_s.data_ptr(), dev), b"first -1"),
        (lambda: lib.fx_offline_smooth_rows(h, p, D, 0, 0, out_s.data_ptr(), dev), b"count 0"),
        (lambda: lib.fx_offline_smooth_rows(h, p, D, 3, 3, out_s.data_ptr(), dev), b"first 3 + count 3 > num_downsamples 5"),
        (lambda: lib.fx_offline_smooth_rows(h, p, D, 0, 1, out_s.data_ptr(), 9), b"memory kind 9"),
    ]
    for k, (call, words) in enumerate(refused):
        assert call() == capi.FX_ERR_INVALID_ARGUMENT and words in lib.fx_last_error(), (k, lib.fx_last_error())
    capi.check(lib.fx_offline_sync(h))
    assert all(same(t.cpu().numpy(), g) for t, g in zip((out_r, out_d, out_s), good))                # nothing was launched into them
    assert all(same(x, y) for x, y in zip(a.smoothed_state(), state))                                # ... nor on the state
    a.smoothing(0)                                                                                   # no smoother: both entries say so
    fp = ctypes.POINTER(ctypes.c_float)
    cur = np.zeros((9, C), F32)
    assert lib.fx_offline_smooth_rows(h, p, D, 0, 1, out_s.data_ptr(), dev) == capi.FX_ERR_INVALID_ARGUMENT and b"no smoother" in lib.fx_last_error()
    assert lib.fx_offline_get_smoothing(h, cur.ctypes.data_as(fp), None) == capi.FX_ERR_INVALID_ARGUMENT and b"no smoother" in lib.fx_last_error()
    capi.check(lib.fx_offline_sync(h))
    assert same(out_s.cpu().numpy(), good[2])
    with pytest.raises(fx.FxError):
        a.discrete_feature_distribution(rows.cpu().numpy(), 0)
    with pytest.raises(ValueError):
        a.feature_ranges(np.zeros((2, C + 1, 4), F32))
    a.close()
