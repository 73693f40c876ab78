"""GPU tests of the ingest side of the path (AudioDataCollector.h:36-94, AudioFilePlayer.h:41-61) and of the
per-channel history ring behind the smoothing / onset stage (RealTimeAudioAnalysis.h:59-71, RealTimeAnalyser.h:201-234):
16-bit PCM converted in the kernels' load stage, the pinned ring at every batch size, calls of every length across the
ring's wrap-around.  Through the C ABI, against the f32 path bit for bit and against the CPU oracle.  Need a real MI355X."""
import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu

BUDGET = signals.ulp_budget("default")          # per-slot ulp budget of the family (oracle/ulp.py)


def close(got, want, what):
    from oracle import fx_oracle as fo
    return signals.assert_features_within(got, want, BUDGET, fo.FEATURE_NAMES, what)


def pcm16(C, T, N, seed):
    """16-bit PCM hops [C][T][N/2] with everything a file holds: tones, noise, bursts, silence, full-scale samples."""
    f = signals.bursts(C, T, N, seed=seed) * 0.8
    f[0] += signals.tone_vibrato_noise(1, T, N, seed=seed + 1)[0] * 0.2
    v = np.clip(np.round(f * 32768.0), -32768, 32767).astype(np.int16)
    v[-1, 0, :4] = [-32768, 32767, 0, -1]
    return v


def decoded(v):
    """what include/fx_wav.hpp (JUCE's WAV reader) makes of 16-bit samples: v / 2^15, exact"""
    return v.astype(np.float32) / np.float32(32768.0)


def same(a, b, what=""):
    for k in (0, 1):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
def test_pcm16_hops_equal_the_decoded_floats_bitwise_and_match_the_oracle(gpu_fx, oracle, N):
    C, T = 5, 23
    v = pcm16(C, T, N, seed=N)
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_gain(0.75)
    ref = gpu_fx.BatchAnalyser(C, N)
    ref.set_gain(0.75)
    # ragged calls: the window's first half comes from the fp32 tail (first hop of a call) or from the 16-bit input
    got = [an.push_hops(v[:, a:b]) for a, b in ((0, 1), (1, 9), (9, 10), (10, 23))]
    want = ref.push_hops(decoded(v))
    got = (np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1))
    same(got, want, "s16 vs f32, N=%d" % N)
    oraw, osm = oracle.push_hops(decoded(v), N, gain=0.75)
    close(got[0], oraw, "s16 raw N=%d" % N)
    close(got[1], osm, "s16 smoothed N=%d" % N)


@pytest.mark.parametrize("N", [1024, 2048])
def test_pcm16_preassembled_frames_and_device_buffers(gpu_fx, N):
    import torch
    C, T = 4, 11
    v = pcm16(C, T + 1, N, seed=7)
    flat = v.reshape(C, -1)
    frames = np.stack([flat[:, t * (N // 2): t * (N // 2) + N] for t in range(T)], axis=1)          # [C][T][N]
    want = gpu_fx.BatchAnalyser(C, N).process_frames(decoded(frames))
    same(gpu_fx.BatchAnalyser(C, N).process_frames(np.ascontiguousarray(frames)), want, "host s16 frames")
    an = gpu_fx.BatchAnalyser(C, N)
    raw, sm = an.process_frames(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    an.sync()
    same((raw.cpu().numpy(), sm.cpu().numpy()), want, "device s16 frames")


@pytest.mark.parametrize("N", [2048, 4096])
def test_pcm16_on_wavefront_pairs(gpu_fx, N):
    C, T = 3, 12
    v = pcm16(C, T, N, seed=3 * N)
    an = gpu_fx.BatchAnalyser(C, N, low_latency=True)
    ref = gpu_fx.BatchAnalyser(C, N, low_latency=True)
    got = [an.push_hops(v[:, a:b]) for a, b in ((0, 5), (5, 6), (6, 12))]              # batch pairs, one-hop pairs, batch pairs
    want = [ref.push_hops(decoded(v)[:, a:b]) for a, b in ((0, 5), (5, 6), (6, 12))]
    for g, w in zip(got, want):
        same(g, w, "pairs s16 N=%d" % N)


@pytest.mark.parametrize("N,C,B,graph", [(1024, 6, 1, None), (4096, 2, 1, None), (2048, 5, 3, "1"), (2048, 5, 3, "0"), (1024, 300, 16, None)])
def test_pcm16_through_the_ring_equals_push_hops_of_the_decoded_floats(gpu_fx, monkeypatch, N, C, B, graph):
    """one hop per call (fx_hop_kernel reads the 16-bit hop out of the pinned slot), small batches (captured step, plain
    launches) and a batch large enough for the three-queue path"""
    if graph is not None:
        monkeypatch.setenv("FX_STREAM_GRAPH", graph)
    nb = 9
    v = pcm16(C, B * nb, N, seed=11 + B)
    want = gpu_fx.BatchAnalyser(C, N).push_hops(decoded(v))
    an = gpu_fx.BatchAnalyser(C, N)
    st = gpu_fx.HopStream(an, B, slots=3, dtype=np.int16)
    got = []
    for b in range(nb):
        if st.in_flight() == 3:
            got.append(st.collect())
        st.push(v[:, b * B:(b + 1) * B], fill_threads=3 if B == 16 else 1)      # (a 4.9 MB batch: the library's fill pool copies it)
    while st.in_flight():
        got.append(st.collect())
    st.close()
    same((np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1)), want, "ring s16")


@pytest.mark.parametrize("N,order,onset", [(1024, 0, (5, 1)), (1024, 1, (32, 2)), (2048, 2, (21, 0)), (4096, 0, (32, 1))])
def test_calls_of_every_length_across_the_history_ring_equal_one_call_bitwise(gpu_fx, oracle, N, order, onset):
    """The raw values behind smoothing and onset live in a ring of 48 rows per channel (row = frame index mod 48).  Calls of
    1, 2..8 (the fused tail), 9..47, 48, and more than 48 frames, placed so that they start at every phase of the ring and
    wrap it several times, with the longest onset window (32: the detector then reaches 40 frames back)."""
    C = 3
    sizes = [1, 1, 5, 1, 8, 30, 1, 47, 1, 1, 48, 3, 1, 70, 1, 2, 1, 13, 1, 1, 1]
    T = sum(sizes)
    hops = signals.bursts(C, T, N, seed=N + order)
    kw = dict(order=order)
    one = gpu_fx.BatchAnalyser(C, N, **kw)
    one.set_onset_window_length(onset[0]); one.set_onset_detection_type(onset[1]); one.set_onset_detection_sensitivity(0.2)
    want = one.push_hops(hops)
    an = gpu_fx.BatchAnalyser(C, N, **kw)
    an.set_onset_window_length(onset[0]); an.set_onset_detection_type(onset[1]); an.set_onset_detection_sensitivity(0.2)
    parts, at = [], 0
    for n in sizes:
        parts.append(an.push_hops(hops[:, at:at + n]))
        at += n
    got = (np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1))
    same(got, want, "ring N=%d" % N)
    assert np.array_equal(an.get_features(), one.get_features(), equal_nan=True)
    oraw, osm = oracle.push_hops(hops, N, order=order, onset_window=onset[0], onset_type=onset[1], onset_sensitivity=0.2)
    assert oraw[:, :, 0].sum() > 0 or onset[0] == 32         # (the case really contains onsets; none survive a 32-frame window)
    close(got[0], oraw, "ring raw")
    close(got[1], osm, "ring smoothed")


def test_one_hop_calls_on_every_path_across_the_history_ring(gpu_fx):
    """120 one-hop calls (the ring wraps twice) on the one-launch hop kernel, on the batch kernels + fused tail, through the pinned
    ring, and on wavefront pairs: each equals the single long call of its kernel family bit for bit, onset window changed mid-way."""
    N, C, T = 2048, 4, 120
    hops = signals.bursts(C, T, N, seed=99)

    def run(make, step):
        an = make()
        out = []
        for t in range(T):
            if t == 70:
                an.set_onset_window_length(17)
            out.append(step(an, t))
        return np.concatenate([o[0] for o in out], 1), np.concatenate([o[1] for o in out], 1)

    def long_call(**kw):
        an = gpu_fx.BatchAnalyser(C, N, **kw)
        a = an.push_hops(hops[:, :70])
        an.set_onset_window_length(17)
        b = an.push_hops(hops[:, 70:])
        return np.concatenate([a[0], b[0]], 1), np.concatenate([a[1], b[1]], 1)

    want = long_call()
    for knob in (1, 0):
        def make(knob=knob):
            an = gpu_fx.BatchAnalyser(C, N)
            an.set_tuning(one_hop_kernel=knob)
            return an
        same(run(make, lambda an, t: an.push_hops(hops[:, t:t + 1])), want, "one_hop_kernel=%d" % knob)
    want_pairs = long_call(low_latency=True)
    same(run(lambda: gpu_fx.BatchAnalyser(C, N, low_latency=True), lambda an, t: an.push_hops(hops[:, t:t + 1])), want_pairs, "pairs")
    # through the pinned ring, three calls in flight
    an = gpu_fx.BatchAnalyser(C, N)
    st = gpu_fx.HopStream(an, 1, slots=3)
    got = []
    for t in range(T):
        if t == 70:
            an.set_onset_window_length(17)
        if st.in_flight() == 3:
            got.append(st.collect())
        st.push(hops[:, t:t + 1])
    while st.in_flight():
        got.append(st.collect())
    st.close()
    same((np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1)), want, "hop kernel through the ring")


# ---- the small gaps the round-3 review listed (Weak 12) ----
@pytest.mark.parametrize("N", [512, 1024, 2048, 4096])
def test_fp16_preassembled_frames_on_the_default_kernel(gpu_fx, oracle, N):
    C, T = 4, 9
    f16 = gpu_fx.synth.frames(C, T, N, first_channel=5).astype(np.float16)
    got = gpu_fx.BatchAnalyser(C, N).process_frames(f16)
    same(got, gpu_fx.BatchAnalyser(C, N).process_frames(f16.astype(np.float32)), "fp16 frames N=%d" % N)
    oraw, osm = oracle.process_frames(f16.astype(np.float32), N)
    close(got[0], oraw, "fp16 frames raw")
    close(got[1], osm, "fp16 frames smoothed")


@pytest.mark.parametrize("N,B,graph", [(1024, 4, "1"), (2048, 3, "0"), (4096, 2, "1")])
def test_hop_stream_batches_of_several_hops_in_fp16(gpu_fx, oracle, monkeypatch, N, B, graph):
    monkeypatch.setenv("FX_STREAM_GRAPH", graph)
    C, nb = 3, 8
    h16 = signals.tone_vibrato_noise(C, B * nb, N, seed=B).astype(np.float16)
    an = gpu_fx.BatchAnalyser(C, N)
    st = gpu_fx.HopStream(an, B, slots=2, dtype=np.float16)
    got = []
    for b in range(nb):
        if st.in_flight() == 2:
            got.append(st.collect())
        st.push(h16[:, b * B:(b + 1) * B])
    while st.in_flight():
        got.append(st.collect())
    st.close()
    got = (np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1))
    same(got, gpu_fx.BatchAnalyser(C, N).push_hops(h16.astype(np.float32)), "fp16 ring B=%d" % B)
    oraw, osm = oracle.push_hops(h16.astype(np.float32), N)
    close(got[0], oraw, "fp16 ring raw")
    close(got[1], osm, "fp16 ring smoothed")


@pytest.mark.parametrize("N", [2048, 4096])
@pytest.mark.parametrize("order", [1, 2])
def test_order_modes_at_the_split_sizes(gpu_fx, oracle, N, order):
    hops = signals.bursts(3, 30, N, seed=40 + order)
    raw, sm = gpu_fx.BatchAnalyser(3, N, order=order).push_hops(hops)
    oraw, osm = oracle.push_hops(hops, N, order=order)
    close(raw, oraw, "order %d N=%d raw" % (order, N))
    close(sm, osm, "order %d N=%d smoothed" % (order, N))


def test_config2_bench_shape_two_calls_state_carried(gpu_fx, oracle):
    """BASELINE configs[2] at the shape bench.py times it: 4096 channels x 2048-pt x 64 frames per call, two calls (flux state,
    overlap tail and histories carried in HBM between them), 24 random channels against the oracle."""
    import torch
    N, C, T = 2048, 4096, 64
    an = gpu_fx.BatchAnalyser(C, N)
    outs, picks = [], np.sort(np.random.default_rng(2).choice(C, 24, replace=False))
    held = []
    for k in range(2):
        h = gpu_fx.synth.hops(C, T, N, first_hop=k * T)
        held.append(h[picks].copy())
        raw, sm = an.push_hops(torch.from_numpy(h).cuda())
        an.sync()
        outs.append((raw[torch.from_numpy(picks).cuda()].cpu().numpy(), sm[torch.from_numpy(picks).cuda()].cpu().numpy()))
        del h, raw, sm
    oraw, osm = oracle.push_hops(np.concatenate(held, axis=1), N)
    close(np.concatenate([o[0] for o in outs], 1), oraw, "configs[2] raw")
    close(np.concatenate([o[1] for o in outs], 1), osm, "configs[2] smoothed")


@pytest.mark.parametrize("N,C", [(512, 700), (1024, 1100), (2048, 600), (4096, 520)])
def test_short_calls_over_many_channels_equal_one_long_call_bitwise(gpu_fx, oracle, N, C):
    """Calls of 1..8 frames per channel over >= 512 channels: one-frame calls run the frame kernel with the flux state left in
    global memory (FrameParams::direct_state), and the scalar tails, smoothing and onset run with a THREAD per channel
    (fx_tail_block_kernel) instead of a wavefront per channel.  Same bits as one long call (uncut frame kernel + the
    three-kernel tail), and as the oracle on a sample of channels, across a wrap of the history ring."""
    sizes = [1, 1, 3, 1, 8, 2, 1, 1, 7, 1, 5, 1, 1, 8, 8, 1, 4, 1, 1, 6]
    T = sum(sizes)
    hops = np.tile(signals.bursts(20, T, N, seed=N), (C // 20, 1, 1))
    hops[::7] *= 0.5
    one = gpu_fx.BatchAnalyser(C, N)
    one.set_onset_window_length(9)
    want = one.push_hops(hops)
    an = gpu_fx.BatchAnalyser(C, N)
    an.set_onset_window_length(9)
    an.set_tuning(one_hop_kernel=0)
    parts, at = [], 0
    for n in sizes:
        parts.append(an.push_hops(hops[:, at:at + n]))
        at += n
    got = (np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1))
    same(got, want, "many channels N=%d" % N)
    assert np.array_equal(an.get_features(), one.get_features(), equal_nan=True)
    pick = [0, 7, C - 1]
    oraw, osm = oracle.push_hops(hops[pick], N, onset_window=9)
    close(got[0][pick], oraw, "many channels raw")
    close(got[1][pick], osm, "many channels smoothed")


# ---- packed 24-bit PCM (FX_SAMPLE_S24) ----
def pcm24(C, T, N, seed):
    """(packed bytes [C][T][3 N/2] uint8, the floats a WAV reader decodes them to [C][T][N/2])"""
    f = signals.bursts(C, T, N, seed=seed) * 0.8
    f[0] += signals.tone_vibrato_noise(1, T, N, seed=seed + 1)[0] * 0.2
    v = np.clip(np.round(f * 8388608.0), -8388608, 8388607).astype(np.int32)
    v[-1, 0, :4] = [-8388608, 8388607, 0, -1]
    return None, v


@pytest.mark.parametrize("N", [256, 512, 1024, 2048, 4096])
def test_pcm24_hops_equal_the_decoded_floats_bitwise_and_match_the_oracle(gpu_fx, oracle, N):
    C, T = 4, 19
    _, v = pcm24(C, T, N, seed=2 * N)
    packed = gpu_fx.pack_s24(v)                               # [C][T][3 N/2] bytes, little endian
    assert packed.shape == (C, T, 3 * (N // 2)) and packed.dtype == np.uint8
    floats = v.astype(np.float32) / np.float32(8388608.0)      # include/fx_wav.hpp: the sample left-justified in an int32, times 2^-31
    an, ref = gpu_fx.BatchAnalyser(C, N), gpu_fx.BatchAnalyser(C, N)
    an.set_gain(1.5); ref.set_gain(1.5)
    got = [an.push_hops(packed[:, a:b]) for a, b in ((0, 1), (1, 8), (8, 9), (9, 19))]
    got = (np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1))
    same(got, ref.push_hops(floats), "s24 vs f32, N=%d" % N)
    oraw, osm = oracle.push_hops(floats, N, gain=1.5)
    close(got[0], oraw, "s24 raw N=%d" % N)
    close(got[1], osm, "s24 smoothed N=%d" % N)


@pytest.mark.parametrize("N,C,B,low", [(1024, 3, 1, False), (4096, 2, 1, True), (2048, 5, 3, False), (1024, 200, 16, False)])
def test_pcm24_through_the_ring_frames_and_pairs(gpu_fx, N, C, B, low):
    """one hop per call (the one-launch hop kernels read the packed hop out of the pinned slot), small and large batches through the
    ring, the low-latency family, and pre-assembled frames from device memory"""
    import torch
    nb = 6
    _, v = pcm24(C, B * nb, N, seed=31 + B)
    packed, floats = gpu_fx.pack_s24(v), v.astype(np.float32) / np.float32(8388608.0)
    want = gpu_fx.BatchAnalyser(C, N, low_latency=low).push_hops(floats)
    an = gpu_fx.BatchAnalyser(C, N, low_latency=low)
    st = gpu_fx.HopStream(an, B, slots=3, dtype=np.uint8)
    got = []
    for b in range(nb):
        if st.in_flight() == 3:
            got.append(st.collect())
        st.push(packed[:, b * B:(b + 1) * B], fill_threads=2 if B == 16 else 1)
    while st.in_flight():
        got.append(st.collect())
    st.close()
    same((np.concatenate([g[0] for g in got], 1), np.concatenate([g[1] for g in got], 1)), want, "ring s24")
    # frames [C][T][N] assembled from the same samples, packed, in device memory
    T = B * nb - 1
    flat = v.reshape(C, -1)
    frames = np.stack([flat[:, t * (N // 2): t * (N // 2) + N] for t in range(T)], axis=1)
    an2 = gpu_fx.BatchAnalyser(C, N, low_latency=low)
    raw, sm = an2.process_frames(torch.from_numpy(np.asarray(gpu_fx.pack_s24(frames))).cuda(), sample_format="s24")
    with pytest.raises(ValueError):                       # bytes are never taken for 24-bit PCM on their dtype alone
        an2.process_frames(torch.from_numpy(np.asarray(gpu_fx.pack_s24(frames))).cuda())
    an2.sync()
    same((raw.cpu().numpy(), sm.cpu().numpy()), gpu_fx.BatchAnalyser(C, N, low_latency=low).process_frames(frames.astype(np.float32) / np.float32(8388608.0)), "s24 frames")
