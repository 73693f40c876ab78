"""fx_offline_analyse_files (include/fx.h) restated for the tests: split the bank, widen each file by the wire formats' rules (v / 2^15,
v / 2^23 from three little-endian bytes, fp16 exactly), and run tests/offline_analyse_model.py's analyse on that file alone -- one channel,
its own State, its own sample rate and nyquist."""
import numpy as np

import offline_analyse_model as model

F32, F16, S16, S24 = 0, 1, 2, 3                                     # FX_SAMPLE_*
BYTES = {F32: 4, F16: 2, S16: 2, S24: 3}
DTYPE = {F32: np.float32, F16: np.float16, S16: np.int16, S24: np.uint8}


def widen(raw, fmt):
    """one file's samples as they lie in the bank (float32 / float16 / int16 values, or uint8 bytes, three a sample) -> float32"""
    raw = np.asarray(raw)
    if fmt == F32:
        return raw.astype(np.float32)
    if fmt == F16:
        return raw.astype(np.float16).astype(np.float32)            # every fp16 value is an fp32 value
    if fmt == S16:
        return raw.astype(np.int16).astype(np.float32) / np.float32(32768.0)
    t = raw.astype(np.uint8).reshape(-1, 3).astype(np.int32)
    v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    return v.astype(np.float32) / np.float32(8388608.0)            # 24 significant bits: the conversion and the scaling are exact


def quantise(x, fmt):
    """float samples -> the bank's values of a format (round to nearest, saturating): test input only"""
    x = np.asarray(x, np.float64)
    if fmt == F32:
        return x.astype(np.float32)
    if fmt == F16:
        return x.astype(np.float16)
    if fmt == S16:
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    q = np.clip(np.rint(x * 8388608.0), -8388608, 8388607).astype(np.int64) & 0xFFFFFF
    return np.stack([q & 0xFF, (q >> 8) & 0xFF, (q >> 16) & 0xFF], axis=-1).astype(np.uint8).reshape(-1)


def split(bank, lengths, fmt):
    """the bank (a flat array of the format's values; bytes for S24) -> its files: file c starts at sample sum (lengths[:c])"""
    per = 3 if fmt == S24 else 1
    starts = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])
    assert starts[-1] * per == np.asarray(bank).shape[0]
    return [np.asarray(bank)[starts[c] * per:starts[c + 1] * per] for c in range(len(lengths))]


class States:
    """one offline_analyse_model.State per file: each file's analyser is its own"""

    def __init__(self, num_files):
        self.each = [model.State(1) for _ in range(num_files)]

    @property
    def previous_f0(self):
        return np.concatenate([s.previous_f0 for s in self.each])

    @property
    def previous_bins(self):
        return np.concatenate([s.previous_bins for s in self.each])


def analyse(oracle, states, bank, lengths, fmt, num_downsamples, window_size, sample_rates, nyquists, what=model.DO_ALL):
    """-> (features [10][C][D], energy [C][D], log attack time [C] or None, magnitudes [D][C][B]); `states` is updated in place"""
    files = split(bank, lengths, fmt)
    C = len(files)
    rates, nyq = np.broadcast_to(sample_rates, (C,)), np.broadcast_to(np.asarray(nyquists, np.float64), (C,))
    parts = [model.analyse(oracle, states.each[c], widen(files[c], fmt)[None, :], num_downsamples, window_size, int(rates[c]), float(nyq[c]), what)
             for c in range(C)]
    features = np.concatenate([p[0] for p in parts], axis=1)
    energy = np.concatenate([p[1] for p in parts], axis=0)
    lat = None if parts[0][2] is None else np.concatenate([p[2] for p in parts])
    mags = np.concatenate([p[3] for p in parts], axis=1)
    return features, energy, lat, mags
