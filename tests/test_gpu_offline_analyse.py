"""The offline driver on the GPU (include/fx.h, fx_offline_frames / fx_offline_analyse): audio in, the reference's feature buffer out.
The frame / window / magnitude kernel against the tests' model (tests/offline_analyse_model.py: numpy indexing, the oracle's Bartlett gain
and forward transform, float32 magnitudes, a serial float32 energy sum) bit for bit; the driver against the per-frame entries it is made
of, bit for bit, and against the model; the Audio row; the seam between two chunks of the object's scratch; the refusals."""
import ctypes
import itertools

import numpy as np
import pytest

import offline_analyse_model as model

pytestmark = pytest.mark.gpu


def same(a, b):
    """bit for bit; a NaN equals a NaN whatever its sign and payload (tests/test_offline.py)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.tobytes() == b.tobytes():
        return True
    if a.dtype.kind != "f":
        return False
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


# ---- 1. frames ----
FRAME_CASES = [("a%d" % n, n, 3 * n + 7, 5) for n in model.WINDOWS] + [("b", 1024, 1024, 1), ("c", 1024, 1025, 1), ("d", 1024, 700, 20),
                                                                       ("e", 256, 5000, 4), ("f", 256, 300, 200)]


def frame_audio(N, S, D, seed):
    """[3][S]: noise of sigma 0.3; silence; noise with an inf where sample 0 of a frame reads it (under the gain 0) and a NaN behind it"""
    rng = np.random.default_rng(seed)
    audio = np.stack([rng.normal(0, 0.3, S), np.zeros(S), rng.normal(0, 0.3, S)]).astype(np.float32)
    step = S // D
    first = 0 if D == 1 else next(f for f in range(D) if f * step - N // 2 >= 0)        # the first frame that starts inside the audio
    at = 0 if D == 1 else first * step - N // 2
    audio[2, at] = np.inf
    audio[2, at + 5] = np.nan
    return audio, first


_frames_expected = {}


def frames_expected(oracle, name, N, S, D):
    if name not in _frames_expected:                                # (the model runs once per case; nothing changes what it returned)
        audio, first = frame_audio(N, S, D, 100 + len(name) + N)
        mags, energy = model.magnitude_frames(oracle, audio, D, N)
        for a in (audio, mags, energy):
            a.setflags(write=False)
        _frames_expected[name] = (audio, first, mags, energy)
    return _frames_expected[name]


@pytest.mark.parametrize("name,N,S,D", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_frames_equal_the_model_from_host_and_device_memory(gpu_fx, oracle, name, N, S, D):
    import torch
    audio, first, want_mags, want_energy = frames_expected(oracle, name, N, S, D)
    C, B = 3, N // 2 + 1
    # what the case is for: the inf under the gain 0 made the whole frame NaN, the silent channel's energy row is all +0
    assert np.isnan(want_mags[first, 2]).all() and np.isfinite(want_mags[:, 0]).all() and not want_energy[1].view(np.uint32).any()
    an = gpu_fx.offline.AudioAnalyser(C)
    mags, energy = an.magnitude_frames(audio, D, N)                                       # host memory
    assert mags.shape == (D, C, B) and energy.shape == (C, D)
    assert same(mags, want_mags), (name, np.argwhere(mags.view(np.uint32) != want_mags.view(np.uint32))[:5])
    assert same(energy, want_energy), name
    d_audio = torch.from_numpy(audio.copy()).cuda()                                       # device memory, through the C ABI
    d_mags = torch.full((D, C, B), -7.0, dtype=torch.float32, device="cuda")
    d_energy = torch.full((C, D), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu_fx.capi.check(an._lib.fx_offline_frames(an._h, vp(d_audio), S, D, N, vp(d_mags), vp(d_energy), gpu_fx.capi.MEM_DEVICE))
    gpu_fx.capi.check(an._lib.fx_offline_sync(an._h))
    assert same(d_mags.cpu().numpy(), want_mags) and same(d_energy.cpu().numpy(), want_energy), name
    d_mags.fill_(-7.0)                                                                     # energy == NULL: the magnitudes alone
    torch.cuda.synchronize()
    gpu_fx.capi.check(an._lib.fx_offline_frames(an._h, vp(d_audio), S, D, N, vp(d_mags), None, gpu_fx.capi.MEM_DEVICE))
    gpu_fx.capi.check(an._lib.fx_offline_sync(an._h))
    assert same(d_mags.cpu().numpy(), want_mags), name
    host_mags = np.full((D, C, B), -7.0, np.float32)
    gpu_fx.capi.check(an._lib.fx_offline_frames(an._h, vp(audio), S, D, N, vp(host_mags), None, gpu_fx.capi.MEM_HOST))
    assert same(host_mags, want_mags), name
    if name == "a1024":                                                                    # a CUDA tensor through the Python method
        t_mags, t_energy = an.magnitude_frames(d_audio, D, N)
        assert same(t_mags, want_mags) and same(t_energy, want_energy)


# ---- 2. the driver is the pieces ----
def harmonic_audio(S, seed, fundamental=220.0, sample_rate=48000):
    """[4][S]: harmonics of the fundamental plus noise, twice at different levels; silence (for the gates); the harmonics with more noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(S) / float(sample_rate)
    tone = sum(np.sin(2 * np.pi * fundamental * h * t) / h for h in range(1, 7))
    return np.stack([0.2 * tone + rng.normal(0, 0.01, S), 0.05 * tone + rng.normal(0, 0.002, S), np.zeros(S),
                     0.1 * tone + rng.normal(0, 0.05, S)]).astype(np.float32)


def pieces(an, audio, D, N, sample_rate):
    """fx_offline_analyse's results from the entries it is made of: the frames, then every frame through the per-frame entries"""
    C, S = audio.shape
    mags, energy = an.magnitude_frames(audio, D, N)
    features = np.zeros((model.FEATURE_ROWS, C, D), np.float32)
    for f in range(D):
        features[[model.CENTROID, model.SPREAD, model.FLATNESS, model.FLUX], :, f] = an.calculate_spectral_characteristics(mags[f]).T
        features[model.SLOPE, :, f] = an.calculate_normalised_spectral_slope(mags[f])
        features[[model.F0, model.HER, model.INHARMONICITY], :, f] = an.calculate_harmonic_characteristics(mags[f]).T
    features[model.ZERO_CROSSES] = an.analyse_normalised_zero_crosses(audio, D)
    lat = np.array([an.set_log_attack_time(energy[c], S, D, sample_rate) for c in range(C)], np.float32)
    return features, energy, lat, mags


PIECE_ROWS = [r for r in range(model.FEATURE_ROWS) if r != model.AUDIO]
EXACT_ROWS = [model.CENTROID, model.FLUX, model.SLOPE, model.ZERO_CROSSES, model.F0, model.HER, model.INHARMONICITY, model.AUDIO]


def test_analyse_is_its_pieces_and_the_model_and_carries_the_state(gpu_fx, oracle):
    N, C, S, D, rate, nyq = 1024, 4, 12000, 20, 48000, 24000.0
    driver, by_hand, state = gpu_fx.offline.AudioAnalyser(C, nyq), gpu_fx.offline.AudioAnalyser(C, nyq), model.State(C)
    for call, audio in enumerate((harmonic_audio(S, 21), harmonic_audio(S, 22, 330.0))):      # the second call starts from the first one's state
        got = driver.perform_spectral_analysis(audio, D, N, rate, keep_fft=True)
        features, energy, lat, mags = pieces(by_hand, audio, D, N, rate)
        assert same(got.magnitudes, mags) and same(got.energy_envelope, energy) and same(got.estimated_log_attack_time, lat), call
        for r in PIECE_ROWS:
            assert same(got.feature_buffer[r], features[r]), (call, r)
        assert same(driver.previous_f0, by_hand.previous_f0) and same(driver.previous_bin_magnitudes, by_hand.previous_bin_magnitudes), call
        want, want_energy, want_lat, want_mags = model.analyse(oracle, state, audio, D, N, rate, nyq)
        assert same(got.magnitudes, want_mags) and same(got.energy_envelope, want_energy) and same(got.estimated_log_attack_time, want_lat), call
        for r in EXACT_ROWS:
            assert same(got.feature_buffer[r], want[r]), (call, r, got.feature_buffer[r], want[r])
        for r in (model.SPREAD, model.FLATNESS):                    # pow() is rounded independently on the device: tests/test_offline.py's budget
            np.testing.assert_allclose(got.feature_buffer[r], want[r], rtol=2e-7, atol=0)
        assert same(driver.previous_f0, state.previous_f0) and same(driver.previous_bin_magnitudes, state.previous_bins), call
        # the case is what it is meant to be: a pitch is found, the silent channel passes no gate and its attack time is log10 (0)
        assert (got.feature_buffer[model.F0][[0, 1, 3]] > 0).any() and not got.feature_buffer[PIECE_ROWS][:, 2].any()
        assert np.isneginf(got.estimated_log_attack_time[2]) and np.isfinite(got.estimated_log_attack_time[[0, 1, 3]]).all()
        assert got.get_feature_sample(model.FLUX, 3, 7) == want[model.FLUX, 3, 7] and got.fft_bins(1).shape == (N // 2 + 1, D)
    assert driver.previous_f0[[0, 1, 3]].all() and driver.previous_bin_magnitudes[0].any()


def test_every_subset_of_what_fills_its_rows_and_leaves_the_others_zero(gpu_fx):
    N, C, S, D, rate = 1024, 4, 12000, 20, 48000
    audio = harmonic_audio(S, 21)
    an = gpu_fx.offline.AudioAnalyser(C, 24000.0)
    full = an.perform_spectral_analysis(audio, D, N, rate)
    raw = an.perform_spectral_analysis(audio, D, N, rate, spectral=False, harmonic=False, zero_crosses=False, normalise=False, log_attack=False)
    rows_of = {"spectral": [model.CENTROID, model.SLOPE, model.SPREAD, model.FLATNESS, model.FLUX], "harmonic": [model.F0, model.HER, model.INHARMONICITY],
               "zero_crosses": [model.ZERO_CROSSES], "audio_rms": [model.AUDIO]}
    flags = ("spectral", "harmonic", "zero_crosses", "audio_rms", "normalise", "log_attack")
    seen = 0
    for bits in itertools.product((False, True), repeat=len(flags)):
        on = dict(zip(flags, bits))
        if on["normalise"] and not on["audio_rms"]:
            continue                                                # refused: tests below
        an.reset()                                                  # every call from a new analyser's state, as `full` was made
        got = an.perform_spectral_analysis(audio, D, N, rate, **on)
        for flag, rows in rows_of.items():
            for r in rows:
                if not on[flag]:
                    assert not got.feature_buffer[r].view(np.uint32).any(), (on, r)         # +0, every bit
                elif r == model.AUDIO and not on["normalise"]:
                    assert same(got.feature_buffer[r], raw.feature_buffer[r]), on
                else:
                    assert same(got.feature_buffer[r], full.feature_buffer[r]), (on, r)
        assert same(got.energy_envelope, full.energy_envelope)
        assert same(got.estimated_log_attack_time, full.estimated_log_attack_time) if on["log_attack"] else got.estimated_log_attack_time is None
        seen += 1
    assert seen == 48


# ---- 3. the Audio row ----
@pytest.mark.parametrize("S,D", [(300, 200), (7 * 30 + 3, 30), (640, 10), (655, 10)], ids=["spb1", "spb7", "spb64", "spb65"])
def test_audio_row_equals_the_model(gpu_fx, S, D):
    rng = np.random.default_rng(S)
    audio = np.stack([rng.normal(0, 0.3, S), rng.normal(0, 0.3, S), np.zeros(S), rng.normal(0, 0.3, S), rng.normal(0, 0.3, S)]).astype(np.float32)
    audio[1, 5] = -3.0                                              # with one sample per step: the normalising maximum comes from |lo|
    audio[3, 0] = np.nan                                            # a NaN at row[0] ...
    audio[4, (S // D) * 3] = np.nan                                 # ... and one elsewhere
    an = gpu_fx.offline.AudioAnalyser(5)
    only = dict(spectral=False, harmonic=False, zero_crosses=False, log_attack=False)
    raw = an.perform_spectral_analysis(audio, D, 256, 48000, normalise=False, **only).feature_buffer
    norm = an.perform_spectral_analysis(audio, D, 256, 48000, normalise=True, **only).feature_buffer
    want_raw = model.rms_row(audio, D)
    want_norm = model.normalise_row(want_raw)
    assert same(raw[model.AUDIO], want_raw), (raw[model.AUDIO], want_raw)
    assert same(norm[model.AUDIO], want_norm), (norm[model.AUDIO], want_norm)
    assert not raw[:model.AUDIO].any() and not norm[:model.AUDIO].any()
    # the cases are what they are meant to be
    assert np.isnan(want_norm[2]).all() and np.isnan(want_norm[3]).all()                 # silence: 0 * (1 / 0); a NaN at row[0] is both ends of the range
    rest = np.delete(want_norm[4], 3)                               # a NaN elsewhere is stepped over: the others are scaled by their own maximum
    assert np.isnan(want_norm[4, 3]) and np.isfinite(rest).all() and 1.0 - 2.0 ** -23 <= np.abs(rest).max() <= 1.0      # (m * fl (1 / m) is 1 or an ulp less)
    assert 1.0 - 2.0 ** -23 <= np.abs(want_norm[1]).max() <= 1.0
    if S // D == 1:
        assert same(want_raw, audio[:, :D]) and want_norm[1, 5] == -1.0


# ---- 4. the seam between two chunks of the scratch ----
@pytest.mark.parametrize("S,D", [(4480, 70), (8960, 140)], ids=["one-seam", "two-seams"])
def test_chunks_of_the_scratch_leave_the_same_bits(gpu_fx, S, D):
    """C = 32, N = 4096: F = (16 << 20) div (4 * 32 * 2049) = 63 frames fit the scratch, so the 70 frames of the first case are cut after
    frame 62 and the 140 of the second after frames 62 and 125.  GPU against GPU: with the magnitudes kept nothing is cut."""
    import torch
    C, N, rate = 32, 4096, 48000
    assert max(1, model.SCRATCH_BYTES // (4 * C * (N // 2 + 1))) == 63
    rng = np.random.default_rng(D)
    audio = torch.from_numpy((rng.normal(0, 0.3, (C, S)) * np.linspace(0.2, 1.0, S)).astype(np.float32)).cuda()
    only = dict(harmonic=False, zero_crosses=False, audio_rms=False, normalise=False, log_attack=False)
    kept_an, cut_an = gpu_fx.offline.AudioAnalyser(C), gpu_fx.offline.AudioAnalyser(C)
    kept = kept_an.perform_spectral_analysis(audio, D, N, rate, keep_fft=True, **only)
    cut = cut_an.perform_spectral_analysis(audio, D, N, rate, keep_fft=False, **only)
    assert same(cut.feature_buffer, kept.feature_buffer) and same(cut.energy_envelope, kept.energy_envelope)
    assert same(cut_an.previous_bin_magnitudes, kept_an.previous_bin_magnitudes)
    assert kept.feature_buffer[model.FLUX][:, [62, 63, D - 1]].all() and kept.feature_buffer[model.CENTROID].all() and cut.magnitudes is None


# ---- 5. refusals ----
def test_refusals_come_before_any_launch_or_state_change(gpu_fx):
    capi = gpu_fx.capi
    C, N, S, D, rate = 2, 256, 2000, 8, 48000
    audio = harmonic_audio(S, 5, 1500.0)[:C]
    an = gpu_fx.offline.AudioAnalyser(C, 24000.0)
    an.perform_spectral_analysis(audio, D, N, rate)
    f0, bins = an.previous_f0, an.previous_bin_magnitudes
    assert f0.any() and bins.shape == (C, N // 2 + 1) and bins.any()
    lib, h = an._lib, an._h
    CANARY = np.float32(-1234.5)
    features = np.full((model.FEATURE_ROWS, C, D), CANARY)
    energy, lat, mags = np.full((C, D), CANARY), np.full(C, CANARY), np.full((D, C, 4096 // 2 + 1), CANARY)

    def refused(status, *words):
        assert status == capi.FX_ERR_INVALID_ARGUMENT, status
        message = lib.fx_last_error().decode()
        for w in words:
            assert str(w) in message, (w, message)
        assert same(an.previous_f0, f0) and same(an.previous_bin_magnitudes, bins), message
        for out in (features, energy, lat, mags):
            assert (out == CANARY).all(), message

    def analyse(audio=audio, S=S, D=D, N=N, rate=rate, what=model.DO_ALL, features=features, lat=lat, kind=capi.MEM_HOST):
        return lib.fx_offline_analyse(h, vp(audio), S, D, N, rate, what, vp(features), vp(energy), vp(lat), vp(mags), kind)

    def frames(audio=audio, S=S, D=D, N=N, mags=mags, kind=capi.MEM_HOST):
        return lib.fx_offline_frames(h, vp(audio), S, D, N, vp(mags), vp(energy), kind)

    for entry in (analyse, frames):
        refused(entry(audio=None), "null argument")
        refused(entry(S=0), "num_samples 0")
        refused(entry(S=-3), "num_samples -3")
        refused(entry(D=0), "num_downsamples 0")
        refused(entry(D=S + 1), "num_downsamples %d" % (S + 1), "num_samples %d" % S)
        for n in (0, 128, 1000, 8192, -256):
            refused(entry(N=n), "window_size %d" % n)
        refused(entry(S=255, D=1), "window_size 256", "255")
        refused(entry(kind=7), "memory kind 7")
    refused(analyse(features=None), "null argument")
    refused(frames(mags=None), "null argument")
    refused(analyse(what=model.DO_NORMALISE_AUDIO | model.DO_SPECTRAL), "FX_OFFLINE_DO_NORMALISE_AUDIO", model.DO_NORMALISE_AUDIO | model.DO_SPECTRAL)
    refused(analyse(lat=None), "log_attack_time")
    refused(analyse(rate=999), "sample_rate 999")
    refused(analyse(N=512), "129 bins", "257")                     # previousBinMagnitudes has this analyser's window size
    assert analyse(N=512, what=model.DO_ALL & ~model.DO_SPECTRAL) == capi.FX_OK          # ... which the harmonic analysis does not read
    assert analyse(rate=999, what=model.DO_ALL & ~model.DO_LOG_ATTACK) == capi.FX_OK    # the sample rate is the log attack time's alone
    assert not (features == CANARY).any() and same(an.previous_bin_magnitudes, bins)
