"""The analysis taps of include/fx.h (fx_get_taps) restated from the oracle's building blocks: what the reference's display buffers hold
for one overlapped window.  Used by tests/test_taps_cpu.py (the committed fixtures) and tests/test_gpu_taps.py (the device)."""
import numpy as np

FIELDS = ("window", "spectrum", "pitch_spectrum", "autocorrelation", "cnd", "lag_position")


def lag_position(cnd, N):
    """getLagEstimateFromCumulativeDifference's normalisedLagPosition (PitchAnalyser.h:161-190,192-217): cnd holds at least N + 1 values"""
    x, y = np.float32(-1.0), np.float32(100.0)
    s = 2
    while s < N:
        if cnd[s] < np.float32(0.01):
            while s + 1 < N and cnd[s + 1] < cnd[s]:
                s += 1
            right = s + 1
            x, y = (np.float32(s), cnd[s]) if cnd[s] <= cnd[right] else (np.float32(right), cnd[right])
            break
        s += 1
    return np.array([x / np.float32(2 * N), y], np.float32)


def oracle_taps(oracle, window):
    """{field: array} for one window [N] (float32); the CND is the oracle's (fxo_estimate_pitch), the autocorrelation its restatement"""
    window = np.ascontiguousarray(window, np.float32)
    N = window.shape[0]
    spectrum = oracle.forward_real(oracle.bartlett(window))
    pitch = oracle.forward_real(oracle.bartlett(oracle.lowpass(window)))
    _, _, cnd2n = oracle.estimate_pitch(pitch)
    return {"window": window, "spectrum": spectrum, "pitch_spectrum": pitch, "autocorrelation": autocorrelation(oracle, pitch)[:N],
            "cnd": cnd2n[:N], "lag_position": lag_position(cnd2n, N)}


def autocorrelation(oracle, pitch_spectrum):
    """v[s] = d[s] * d[s] * s over all 2N samples, d the planar inverse transform of (re^2, 0) times 1.0f / N (PitchAnalyser.h:83-127)"""
    re = pitch_spectrum[0::2]
    N = re.shape[0]
    z = oracle.fft_complex((re * re).astype(np.float32).astype(np.complex64), inverse=True)
    d = np.concatenate([z.real, z.imag]).astype(np.float32) * np.float32(1.0 / N)
    with np.errstate(over="ignore", invalid="ignore"):
        return (d * d) * np.arange(2 * N, dtype=np.float32)


def cnd_from(v):
    """the running fp32 sum and the ratios of getCumulativeNormalisedDifferenceFromAutoCorrelationBuffer (PitchAnalyser.h:129-159)"""
    sums = np.add.accumulate(np.concatenate([[np.float32(0)], v[1:]]).astype(np.float32), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = np.where(sums != 0, v / np.where(sums != 0, sums, np.float32(1)), np.float32(0)).astype(np.float32)
    out[0] = 1.0
    return out


def assert_taps_equal(got, want, what=""):
    for k in FIELDS:
        g, w = np.asarray(got[k], np.float32), np.asarray(want[k], np.float32)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        ok = (g == w) | (np.isnan(g) & np.isnan(w))
        assert ok.all(), "%s %s: %d values differ, first at %d: %r against %r" % (
            what, k, int((~ok).sum()), int(np.argmin(ok)), g[np.argmin(ok)], w[np.argmin(ok)])
