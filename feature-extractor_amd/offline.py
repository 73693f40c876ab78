"""Host-side mirror of the reference's LEGACY offline analyser (struct AudioAnalyser, ref AudioAnalysis.h) on top of the
C ABI (fx_offline_*): one object stands for `num_channels` analysers.  Method names follow the reference."""
import ctypes

import numpy as np

from . import capi


class AudioAnalyser:
    def __init__(self, num_channels, nyquist_frequency=24000.0, device=0):                # ref AudioAnalysis.h:107
        self._lib = capi.load_library()
        self.num_channels = int(num_channels)
        h = ctypes.c_void_p()
        capi.check(self._lib.fx_offline_create(ctypes.byref(h), int(device), self.num_channels, float(nyquist_frequency)))
        self._h = h
        self._bins = 0          # length of previousBinMagnitudes: fixed by the first calculate_spectral_characteristics after construction / reset

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fx_offline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        capi.check(self._lib.fx_offline_reset(self._h))
        self._bins = 0

    @property
    def previous_f0(self):                                                                  # ref AudioAnalysis.h:697
        out = np.empty(self.num_channels, np.float64)
        capi.check(self._lib.fx_offline_get_previous_f0(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def _rows(self, a):
        a = np.ascontiguousarray(a, np.float32)
        if a.ndim != 2 or a.shape[0] != self.num_channels:
            raise ValueError("expected [%d][...] float32" % self.num_channels)
        return a

    def analyse_normalised_zero_crosses(self, audio, num_downsamples):                      # ref :517-541
        audio = self._rows(audio)
        out = np.empty((self.num_channels, int(num_downsamples)), np.float32)
        capi.check(self._lib.fx_offline_zero_crosses(self._h, audio.ctypes.data_as(ctypes.c_void_p), audio.shape[1], int(num_downsamples),
                                                     out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return out

    def set_log_attack_time(self, energy_envelope, num_input_samples, num_downsamples, sample_rate):   # ref :611-622
        env = np.ascontiguousarray(energy_envelope, np.float32).reshape(-1)
        out = np.empty(1, np.float32)
        capi.check(self._lib.fx_offline_log_attack_time(self._h, env.ctypes.data_as(ctypes.c_void_p), env.shape[0], int(num_input_samples),
                                                        int(num_downsamples), int(sample_rate), out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return out[0]

    def calculate_fft_lbp(self, fft_results, previous_fft_frame):                           # ref :543-564
        cur, prev = self._rows(fft_results), self._rows(previous_fft_frame)
        if cur.shape != prev.shape:
            raise ValueError("frames differ in shape")
        bits = np.empty(cur.shape, np.uint8)
        hi, act = np.empty(self.num_channels, np.float32), np.empty(self.num_channels, np.float32)
        capi.check(self._lib.fx_offline_fft_lbp(self._h, cur.ctypes.data_as(ctypes.c_void_p), prev.ctypes.data_as(ctypes.c_void_p), cur.shape[1],
                                                bits.ctypes.data_as(ctypes.c_void_p), hi.ctypes.data_as(ctypes.c_void_p),
                                                act.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return bits, hi, act

    def calculate_harmonic_characteristics(self, fft_results):                              # ref :253-303
        mags = self._rows(fft_results)
        out = np.empty((self.num_channels, 3), np.float32)
        capi.check(self._lib.fx_offline_harmonic_characteristics(self._h, mags.ctypes.data_as(ctypes.c_void_p), mags.shape[1],
                                                                 out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return out

    def calculate_spectral_characteristics(self, fft_results):                              # ref :463-515
        """magnitudes [C][num_bins] of one frame -> [C][4] = centroid / nyquist, spread, flatness, flux; previousBinMagnitudes is kept."""
        mags = self._rows(fft_results)
        out = np.empty((self.num_channels, 4), np.float32)
        capi.check(self._lib.fx_offline_spectral_characteristics(self._h, mags.ctypes.data_as(ctypes.c_void_p), mags.shape[1],
                                                                 out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        self._bins = mags.shape[1]
        return out

    @property
    def previous_bin_magnitudes(self):                                                      # ref :700
        if self._bins == 0:         # nothing analysed since construction / reset: the reference's vector exists, zero-filled, at its window size -- which this object learns from the first frame
            return np.zeros((self.num_channels, 0), np.float64)
        out = np.empty((self.num_channels, self._bins), np.float64)
        capi.check(self._lib.fx_offline_get_previous_bins(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self._bins))
        return out

    def calculate_normalised_spectral_slope(self, fft_results):                             # ref :566-609
        mags = self._rows(fft_results)
        out = np.empty(self.num_channels, np.float32)
        capi.check(self._lib.fx_offline_spectral_slope(self._h, mags.ctypes.data_as(ctypes.c_void_p), mags.shape[1],
                                                       out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return out

    def analyse_auto_correlation(self, data):                                               # ref :623-665
        """data [C][num_items][2] (r, i) -> (products [C][num_items][2] of getConjugateComplexMultiplicationInPlace, peak bin [C],
        frequency [C] float64 as analyseAutoCorrelation prints it)."""
        data = np.array(data, np.float32, order="C")
        if data.ndim != 3 or data.shape[0] != self.num_channels or data.shape[2] != 2:
            raise ValueError("expected [%d][num_items][2] float32" % self.num_channels)
        peaks, freqs = np.empty(self.num_channels, np.int32), np.empty(self.num_channels, np.float64)
        capi.check(self._lib.fx_offline_auto_correlation(self._h, data.ctypes.data_as(ctypes.c_void_p), data.shape[1],
                                                         peaks.ctypes.data_as(ctypes.c_void_p), freqs.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return data, peaks, freqs

    # ---- the offline driver: audio in, the reference's feature buffer out (fx_offline_frames / fx_offline_analyse) ----
    def _audio(self, audio):
        """-> (the array or tensor to keep alive, its address, num_samples, memory kind, an allocator of float32 results beside it)"""
        if _is_device_tensor(audio):
            import torch
            if audio.dtype != torch.float32 or audio.dim() != 2 or audio.shape[0] != self.num_channels:
                raise ValueError("expected [%d][num_samples] float32" % self.num_channels)
            audio = audio.contiguous()
            torch.cuda.current_stream(audio.device).synchronize()       # the library reads it on a stream of its own
            return audio, audio.data_ptr(), int(audio.shape[1]), capi.MEM_DEVICE, lambda *shape: torch.empty(shape, dtype=torch.float32, device=audio.device)
        audio = self._rows(audio)
        return audio, audio.ctypes.data, int(audio.shape[1]), capi.MEM_HOST, lambda *shape: np.empty(shape, np.float32)

    def _finish(self, kind, *results):
        """device results are read after the object's stream has run dry; each comes back as a numpy array"""
        if kind == capi.MEM_DEVICE:
            capi.check(self._lib.fx_offline_sync(self._h))
        return [None if r is None else (r if isinstance(r, np.ndarray) else r.cpu().numpy()) for r in results]

    def magnitude_frames(self, audio, num_downsamples, window_size):                         # ref :146-181, :667-676, :208
        """audio [C][S] (numpy: through host memory; a CUDA torch tensor: used where it lies) -> (magnitudes [D][C][window_size / 2 + 1],
        energy envelope [C][D]) of the windows performSpectralAnalysis cuts: one per downsample, centred on it, Bartlett-windowed."""
        keep, address, S, kind, new = self._audio(audio)
        D, N = int(num_downsamples), int(window_size)
        if D < 1 or N not in capi.OFFLINE_WINDOWS:           # (the library refuses these too: the shapes below need them first)
            raise capi.FxError(capi.FX_ERR_INVALID_ARGUMENT, "num_downsamples %d, window_size %d" % (D, N))
        mags, energy = new(D, self.num_channels, N // 2 + 1), new(self.num_channels, D)
        capi.check(self._lib.fx_offline_frames(self._h, address, S, D, N, _address(mags), _address(energy), kind))
        return tuple(self._finish(kind, mags, energy))

    def perform_spectral_analysis(self, audio, num_downsamples, window_size, sample_rate, spectral=True, harmonic=True, zero_crosses=True,
                                  audio_rms=True, normalise=True, log_attack=True, keep_fft=False):          # ref :129-251
        """The reference's offline analysis of audio [C][S], each channel a mono file of its own -> ConcatenatedFeatureBuffer.  The analysers'
        state (previous_f0, previous_bin_magnitudes) carries on from the calls before."""
        keep, address, S, kind, new = self._audio(audio)
        D, N, C = int(num_downsamples), int(window_size), self.num_channels
        if D < 1 or N not in capi.OFFLINE_WINDOWS:
            raise capi.FxError(capi.FX_ERR_INVALID_ARGUMENT, "num_downsamples %d, window_size %d" % (D, N))
        what = ((capi.OFFLINE_DO_SPECTRAL if spectral else 0) | (capi.OFFLINE_DO_HARMONIC if harmonic else 0)
                | (capi.OFFLINE_DO_ZERO_CROSSES if zero_crosses else 0) | (capi.OFFLINE_DO_AUDIO if audio_rms else 0)
                | (capi.OFFLINE_DO_NORMALISE_AUDIO if normalise else 0) | (capi.OFFLINE_DO_LOG_ATTACK if log_attack else 0))
        features, energy = new(capi.OFFLINE_FEATURE_ROWS, C, D), new(C, D)
        lat = new(C) if log_attack else None
        mags = new(D, C, N // 2 + 1) if keep_fft else None
        capi.check(self._lib.fx_offline_analyse(self._h, address, S, D, N, int(sample_rate), what, _address(features), _address(energy),
                                                _address(lat), _address(mags), kind))
        if spectral:
            self._bins = N // 2 + 1
        features, energy, lat, mags = self._finish(kind, features, energy, lat, mags)
        return ConcatenatedFeatureBuffer(features, energy, lat, mags, D, int(sample_rate), analyser=self)

    # ---- a library of files of different lengths in one call (fx_offline_analyse_files) ----
    _FORMAT_OF = {"float32": capi.SAMPLE_F32, "float16": capi.SAMPLE_F16, "int16": capi.SAMPLE_S16, "uint8": capi.SAMPLE_S24}

    def _format(self, dtype_name, sample_format):
        """the FX_SAMPLE_* of a dtype, or None: sample_format, when given, must name it, and bytes are samples only when it says so"""
        fmt = self._FORMAT_OF.get(dtype_name)
        if (sample_format is None and fmt == capi.SAMPLE_S24) or (sample_format is not None and int(sample_format) != fmt):
            return None
        return fmt

    def _bank(self, files, sample_format):
        """files: a list of 1-D numpy arrays of one dtype (float32, float16, int16, or uint8 bytes with sample_format=SAMPLE_S24), or a pair
        (flat CUDA tensor, lengths) -> (what to keep alive, address, lengths [C] int64, sample format, memory kind, an allocator)"""
        if isinstance(files, tuple) and len(files) == 2 and _is_device_tensor(files[0]):
            import torch
            bank, lengths = files
            fmt = self._format(str(bank.dtype).split(".")[-1], sample_format)
            if fmt is None or bank.dim() != 1:
                raise ValueError("expected a flat float32 / float16 / int16 tensor, or uint8 bytes with sample_format=SAMPLE_S24")
            bank = bank.contiguous()
            lengths = np.ascontiguousarray(lengths, np.int64)
            if lengths.shape != (self.num_channels,) or int(lengths.sum()) * (3 if fmt == capi.SAMPLE_S24 else 1) != bank.numel():
                raise ValueError("expected %d lengths that add up to the bank" % self.num_channels)
            torch.cuda.current_stream(bank.device).synchronize()         # the library reads it on a stream of its own
            return bank, bank.data_ptr(), lengths, fmt, capi.MEM_DEVICE, lambda *shape: torch.empty(shape, dtype=torch.float32, device=bank.device)
        files = [np.ascontiguousarray(f) for f in files]
        if len(files) != self.num_channels or any(f.ndim != 1 or f.dtype != files[0].dtype for f in files):
            raise ValueError("expected %d one-dimensional arrays of one dtype" % self.num_channels)
        fmt = self._format(files[0].dtype.name, sample_format)
        if fmt is None or (fmt == capi.SAMPLE_S24 and any(f.size % 3 for f in files)):
            raise ValueError("expected float32 / float16 / int16 arrays, or uint8 bytes (three a sample) with sample_format=SAMPLE_S24")
        lengths = np.array([f.size // (3 if fmt == capi.SAMPLE_S24 else 1) for f in files], np.int64)
        bank = np.concatenate(files) if files else np.empty(0, np.float32)
        return bank, bank.ctypes.data, lengths, fmt, capi.MEM_HOST, lambda *shape: np.empty(shape, np.float32)

    def perform_spectral_analysis_files(self, files, num_downsamples, window_size, sample_rates, spectral=True, harmonic=True, zero_crosses=True,
                                        audio_rms=True, normalise=True, log_attack=True, keep_fft=False, sample_format=None):
        """perform_spectral_analysis of C files of different lengths (and rates) in one call: every channel's results are what that file alone
        gives.  sample_rates: one int or C ints; each analyser's nyquist is set_nyquists' business -- nothing is resampled.
        -> ConcatenatedFeatureBuffer with num_samples [C] and sample_rate [C]."""
        keep, address, lengths, fmt, kind, new = self._bank(files, sample_format)
        D, N, C = int(num_downsamples), int(window_size), self.num_channels
        if D < 1 or N not in capi.OFFLINE_WINDOWS:
            raise capi.FxError(capi.FX_ERR_INVALID_ARGUMENT, "num_downsamples %d, window_size %d" % (D, N))
        rates = np.ascontiguousarray(np.broadcast_to(np.asarray(sample_rates, np.int32), (C,)))
        what = ((capi.OFFLINE_DO_SPECTRAL if spectral else 0) | (capi.OFFLINE_DO_HARMONIC if harmonic else 0)
                | (capi.OFFLINE_DO_ZERO_CROSSES if zero_crosses else 0) | (capi.OFFLINE_DO_AUDIO if audio_rms else 0)
                | (capi.OFFLINE_DO_NORMALISE_AUDIO if normalise else 0) | (capi.OFFLINE_DO_LOG_ATTACK if log_attack else 0))
        features, energy = new(capi.OFFLINE_FEATURE_ROWS, C, D), new(C, D)
        lat = new(C) if log_attack else None
        mags = new(D, C, N // 2 + 1) if keep_fft else None
        capi.check(self._lib.fx_offline_analyse_files(self._h, address, lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), fmt, D, N,
                                                      rates.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), what, _address(features), _address(energy),
                                                      _address(lat), _address(mags), kind))
        if spectral:
            self._bins = N // 2 + 1
        features, energy, lat, mags = self._finish(kind, features, energy, lat, mags)
        return ConcatenatedFeatureBuffer(features, energy, lat, mags, D, rates.copy(), analyser=self, num_samples=lengths)

    def set_nyquists(self, values):                                                          # ref AudioAnalysis.h:107, one per channel's analyser
        values = np.ascontiguousarray(values, np.float64)
        if values.shape != (self.num_channels,):
            raise ValueError("expected %d values" % self.num_channels)
        capi.check(self._lib.fx_offline_set_nyquists(self._h, values.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    @property
    def nyquists(self):
        out = np.empty(self.num_channels, np.float64)
        capi.check(self._lib.fx_offline_get_nyquists(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    # ---- what the reference derives from a feature buffer (fx_offline_feature_ranges / _distribution / _smooth_rows) ----
    def _feature_rows(self, rows, least=1):
        """rows [R][C][D] (numpy: through host memory; a CUDA torch tensor: used where it lies) -> (the array or tensor to keep alive, its
        address, R, D, memory kind, an allocator of float32 results beside it)"""
        if _is_device_tensor(rows):
            import torch
            if rows.dtype != torch.float32 or rows.dim() != 3 or rows.shape[1] != self.num_channels or rows.shape[0] < least:
                raise ValueError("expected [>= %d][%d][num_downsamples] float32" % (least, self.num_channels))
            rows = rows.contiguous()
            torch.cuda.current_stream(rows.device).synchronize()         # the library reads it on a stream of its own
            return rows, rows.data_ptr(), int(rows.shape[0]), int(rows.shape[2]), capi.MEM_DEVICE, lambda *shape: torch.empty(shape, dtype=torch.float32, device=rows.device)
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 3 or rows.shape[1] != self.num_channels or rows.shape[0] < least:
            raise ValueError("expected [>= %d][%d][num_downsamples] float32" % (least, self.num_channels))
        return rows, rows.ctypes.data, int(rows.shape[0]), int(rows.shape[2]), capi.MEM_HOST, lambda *shape: np.empty(shape, np.float32)

    def feature_ranges(self, rows):                                                          # ref AudioFeatures.h:208-213, per row and channel
        """rows [R][C][D] -> [R][C][2]: getFeatureRange's (start, end) of every row and channel"""
        keep, address, R, D, kind, new = self._feature_rows(rows)
        out = new(R, self.num_channels, 2)
        capi.check(self._lib.fx_offline_feature_ranges(self._h, address, R, D, _address(out), kind))
        return self._finish(kind, out)[0]

    def discrete_feature_distribution(self, rows, num_brackets):                             # ref AudioFeatures.h:215-240
        """rows [R][C][D] -> [R][C][num_brackets]: getDiscreteFeatureDistribution of every row and channel"""
        keep, address, R, D, kind, new = self._feature_rows(rows)
        nb = int(num_brackets)
        if nb < 1:                                           # (the library refuses it too: the shape below needs it first)
            raise capi.FxError(capi.FX_ERR_INVALID_ARGUMENT, "num_brackets %d" % nb)
        out = new(R, self.num_channels, nb)
        capi.check(self._lib.fx_offline_feature_distribution(self._h, address, R, D, nb, _address(out), kind))
        return self._finish(kind, out)[0]

    def smoothing(self, depth):                                                              # ref AudioFeatures.h:358-369
        """construct every channel's SmoothedFeatures (depth 1 .. 64) anew; 0 frees them"""
        capi.check(self._lib.fx_offline_smoothing(self._h, int(depth)))
        self._smoothing_depth = int(depth)

    def smooth_rows(self, rows, first=0, count=None):                                        # ref AudioFeatures.h:371-379
        """rows [R >= 9][C][D]: updateValues on columns first .. first + count - 1 (count None: to the end) -> current values [9][C][count]"""
        keep, address, R, D, kind, new = self._feature_rows(rows, capi.OFFLINE_SMOOTHED_FEATURES)
        count = D - int(first) if count is None else int(count)
        out = new(capi.OFFLINE_SMOOTHED_FEATURES, self.num_channels, max(count, 1))
        capi.check(self._lib.fx_offline_smooth_rows(self._h, address, D, int(first), count, _address(out), kind))
        return self._finish(kind, out)[0]

    def smoothed_state(self):                                                                # ref AudioFeatures.h:382-383
        """-> (currentFeatureValues [9][C], featureHistory [9][C][depth]) of the channels' smoothers"""
        depth = getattr(self, "_smoothing_depth", 0)
        current = np.empty((capi.OFFLINE_SMOOTHED_FEATURES, self.num_channels), np.float32)
        history = np.empty((capi.OFFLINE_SMOOTHED_FEATURES, self.num_channels, depth), np.float32)
        fp = ctypes.POINTER(ctypes.c_float)
        capi.check(self._lib.fx_offline_get_smoothing(self._h, current.ctypes.data_as(fp), history.ctypes.data_as(fp)))
        return current, history


def _is_device_tensor(a):
    return type(a).__module__.split(".")[0] == "torch" and a.is_cuda


def _address(a):
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


class ConcatenatedFeatureBuffer:
    """The results of AudioAnalyser.perform_spectral_analysis under the reference's names (ref AudioFeatures.h:14-314), on the host.
    `feature` arguments are the FX_OFFLINE_* row numbers (capi.OFFLINE_CENTROID .. capi.OFFLINE_AUDIO)."""

    def __init__(self, feature_buffer, energy_envelope, estimated_log_attack_time, magnitudes, num_downsamples, sample_rate, analyser=None, num_samples=None):
        self._analyser = analyser                                       # the AudioAnalyser whose GPU derives ranges and distributions
        self.feature_buffer = feature_buffer                            # [10][C][D]: featureBuffer, less its FFT part
        self.energy_envelope = energy_envelope                          # [C][D]
        self.estimated_log_attack_time = estimated_log_attack_time      # [C], or None if not analysed
        self.magnitudes = magnitudes                                    # [D][C][bins], or None unless keep_fft
        self.num_downsamples = int(num_downsamples)
        # (an int: ref :301) -- or, from perform_spectral_analysis_files, one int per file [C], beside each file's own number of samples [C]
        self.sample_rate = int(sample_rate) if np.ndim(sample_rate) == 0 else np.asarray(sample_rate, np.int32)
        self.num_samples = None if num_samples is None else np.asarray(num_samples, np.int64)
        self.num_feature_channels = feature_buffer.shape[1]

    def get_feature_buffer(self, feature):                                                  # ref :242-254
        return self.feature_buffer[int(feature)].copy()

    def get_feature_sample(self, feature, channel, index):                                  # ref :256-264
        return self.feature_buffer[int(feature), int(channel), int(index)]

    def get_feature_range(self, feature):                                                   # ref :208-213, findMinMax over every channel's row
        row = self.feature_buffer[int(feature)].reshape(-1)
        lo = hi = row[0]
        for v in row[1:]:
            if v < lo:
                lo = v
            if v > hi:
                hi = v
        return lo, hi

    def _gpu(self):
        if self._analyser is None:
            raise ValueError("this buffer was made without an analyser (ConcatenatedFeatureBuffer(..., analyser=...))")
        return self._analyser

    def feature_ranges(self):                                                               # ref :208-213, per row and channel, on the GPU
        """-> [10][C][2]: every row's (start, end), each channel a file of its own"""
        return self._gpu().feature_ranges(self.feature_buffer)

    def get_discrete_feature_distribution(self, feature, num_brackets):                     # ref :215-240, on the GPU
        """-> [C][num_brackets]"""
        return self._gpu().discrete_feature_distribution(self.feature_buffer[int(feature)][None], num_brackets)[0]

    def get_average_feature_sample(self, feature, index):                                   # ref :266-275: a serial float sum
        av = np.float32(0.0)
        for c in range(self.num_feature_channels):
            av = np.float32(av + self.feature_buffer[int(feature), c, int(index)])
        return np.float32(av / np.float32(self.num_feature_channels))

    def fft_bins(self, channel):                                                            # ref :142-156 setFFTBinsForSample: [bin][downsample]
        if self.magnitudes is None:
            raise ValueError("the analysis kept no magnitudes (keep_fft=False)")
        return self.magnitudes[:, int(channel), :].T


class Range:
    """JUCE's Range<float> as far as FeatureSpace uses it: the constructor keeps end >= start, and each setter moves the other end along
    (tools/refdiff/juce_standin.h:55-66)."""

    def __init__(self, start=0.0, end=0.0):
        start, end = np.float32(start), np.float32(end)
        self.start, self.end = start, (start if end < start else end)

    def set_start(self, start):
        self.start = np.float32(start)
        if self.end < self.start:
            self.end = self.start

    def set_end(self, end):
        self.end = np.float32(end)
        if self.end < self.start:
            self.start = self.end

    def __iter__(self):
        return iter((self.start, self.end))


class FeatureSpace:
    """ref AudioFeatures.h:319-349: four ranges that describe a file, folded over a corpus by compare_and_update_ranges.  A handful of
    floats per file: host arithmetic, fed by the GPU's ranges (from_buffer)."""

    def __init__(self, attack=None, centroid_range=None, slope_range=None, crosses_range=None):
        self.attack_range = Range() if attack is None else Range(attack, 0.0)               # :331
        self.spectral_centroid_range = centroid_range if centroid_range is not None else Range()
        self.spectral_slope_range = slope_range if slope_range is not None else Range()
        self.zero_crosses_range = crosses_range if crosses_range is not None else Range()

    @staticmethod
    def compare_and_update_ranges(existing_range, new_range):                               # :337-343, as written: both tests are `<`
        if new_range.start < existing_range.start:
            existing_range.set_start(new_range.start)
        if new_range.end < existing_range.end:
            existing_range.set_end(new_range.end)

    @classmethod
    def from_buffer(cls, buffer, channel, ranges=None):
        """the space of one channel (a mono file) of an analysed buffer: its estimated log attack time and the GPU's centroid, slope and
        zero-crossing ranges (ranges: buffer.feature_ranges(), when the caller already has them)"""
        if buffer.estimated_log_attack_time is None:
            raise ValueError("the analysis estimated no log attack time (log_attack=False)")
        ranges = buffer.feature_ranges() if ranges is None else ranges
        c = int(channel)
        return cls(buffer.estimated_log_attack_time[c], Range(*ranges[capi.OFFLINE_CENTROID, c]), Range(*ranges[capi.OFFLINE_SLOPE, c]),
                   Range(*ranges[capi.OFFLINE_ZERO_CROSSES, c]))
