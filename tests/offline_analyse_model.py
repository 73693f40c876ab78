"""The offline driver (include/fx.h, fx_offline_frames / fx_offline_analyse) restated for the tests: frames by numpy indexing, the Bartlett
gain and the forward transform of the oracle, magnitudes and energy in numpy float32, the per-frame rows through the oracle's offline_*
functions, the RMS row and its normalisation from the specification's formulas.  "ref:" citations are relative to the reference's Source/."""
import numpy as np

f32, f64 = np.float32, np.float64
(CENTROID, SLOPE, SPREAD, FLATNESS, FLUX, ZERO_CROSSES, F0, HER, INHARMONICITY, AUDIO, FEATURE_ROWS) = range(11)
DO_SPECTRAL, DO_HARMONIC, DO_ZERO_CROSSES, DO_AUDIO, DO_NORMALISE_AUDIO, DO_LOG_ATTACK = 1, 2, 4, 8, 16, 32
DO_ALL = 63
WINDOWS = (256, 512, 1024, 2048, 4096)
SCRATCH_BYTES = 16 << 20


def windows(channel, num_downsamples, window_size):
    """one channel's samples [S] -> [D][N]: the window of every frame before the gain (ref AudioAnalysis.h:146-181)"""
    a = np.asarray(channel, f32)
    S, D, N = a.shape[0], int(num_downsamples), int(window_size)
    if D == 1:
        return a[None, :N].copy()
    step = S // D
    i = np.arange(D)[:, None] * step + np.arange(N)[None, :] - N // 2
    inside = (i >= 0) & (i < S)
    return np.where(inside, a[np.clip(i, 0, S - 1)], f32(0.0)).astype(f32)


def windowed(oracle, channel, num_downsamples, window_size):
    """-> [D][N]: every frame as the transform reads it (the reference's fftIn after scaleBufferWithBartlettWindowing, ref :667-676)"""
    with np.errstate(invalid="ignore"):
        return np.stack([oracle.bartlett(w) for w in windows(channel, num_downsamples, window_size)])


def magnitude_frames(oracle, audio, num_downsamples, window_size):
    """audio [C][S] -> (magnitudes [D][C][N / 2 + 1], energy [C][D])"""
    audio = np.asarray(audio, f32)
    C, D, B = audio.shape[0], int(num_downsamples), int(window_size) // 2 + 1
    mags, energy = np.empty((D, C, B), f32), np.empty((C, D), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            for f, x in enumerate(windowed(oracle, audio[c], D, window_size)):
                spec = oracle.forward_real(x)
                re, im = spec[0::2][:B], spec[1::2][:B]
                m = np.sqrt(re * re + im * im)                      # float32 throughout: two products, one sum, one correctly rounded root
                assert m.dtype == f32
                mags[f, c] = m
                energy[c, f] = np.cumsum(m, dtype=f32)[-1]          # serial, in bin order (np.sum is pairwise)
    return mags, energy


def rms_row(audio, num_downsamples):
    """ref AudioFeatures.h:158-184 fillDownsampledRMSAudioChannels: audio [C][S] -> [C][D]"""
    audio = np.asarray(audio, f32)
    C, S = audio.shape
    D = int(num_downsamples)
    spb = S // D
    if spb == 1:
        return audio[:, :D].copy()
    row = np.empty((C, D), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(C):
            for i in range(D):
                a = audio[c, i * spb:(i + 1) * spb]
                total = np.cumsum((a * a).astype(f64))[-1]              # float squares, a serial double sum from +0.0
                row[c, i] = f32(np.sqrt(total / f64(spb)))
    return row


def normalise_row(row):
    """ref AudioFeatures.h:186-195 with the stand-in's findMinMax, one channel at a time: row [C][D] -> [C][D]"""
    row = np.asarray(row, f32)
    out = np.empty_like(row)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(row.shape[0]):
            lo = hi = row[c, 0]
            for v in row[c, 1:]:
                if v < lo:
                    lo = v
                if v > hi:
                    hi = v
            a, b = np.abs(lo), np.abs(hi)
            m = b if a < b else a                                       # jmax (a, b) = a < b ? b : a
            out[c] = row[c] * (f32(1.0) / m)
    return out


class State:
    """what an fx_offline carries from call to call: previousF0 [C] and previousBinMagnitudes [C][bins] (zero-filled when first used)"""

    def __init__(self, num_channels):
        self.previous_f0 = np.zeros(num_channels, f64)
        self.previous_bins = None


def analyse(oracle, state, audio, num_downsamples, window_size, sample_rate, nyquist, what=DO_ALL):
    """-> (features [10][C][D], energy [C][D], log attack time [C] or None, magnitudes [D][C][B]); `state` is updated in place"""
    audio = np.asarray(audio, f32)
    C, S = audio.shape
    D, B = int(num_downsamples), int(window_size) // 2 + 1
    features = np.zeros((FEATURE_ROWS, C, D), f32)
    mags, energy = magnitude_frames(oracle, audio, D, window_size)
    if what & DO_SPECTRAL and state.previous_bins is None:
        state.previous_bins = np.zeros((C, B), f64)
    for f in range(D):                                                  # the order of ref AudioAnalysis.h:229-246
        if what & DO_SPECTRAL:
            out4 = oracle.offline_spectral_characteristics(mags[f], nyquist, state.previous_bins)
            features[[CENTROID, SPREAD, FLATNESS, FLUX], :, f] = out4.T
            features[SLOPE, :, f] = oracle.offline_spectral_slope(mags[f])
        if what & DO_HARMONIC:
            features[[F0, HER, INHARMONICITY], :, f] = oracle.offline_harmonic_characteristics(mags[f], nyquist, state.previous_f0).T
    if what & DO_ZERO_CROSSES:
        features[ZERO_CROSSES] = oracle.offline_zero_crosses(audio, D)
    if what & DO_AUDIO:
        features[AUDIO] = rms_row(audio, D)
        if what & DO_NORMALISE_AUDIO:
            features[AUDIO] = normalise_row(features[AUDIO])
    lat = None
    if what & DO_LOG_ATTACK:
        lat = np.array([oracle.offline_log_attack_time(energy[c], S, D, sample_rate) for c in range(C)], f32)
    return features, energy, lat, mags
