"""Host-side mirror of the reference's analyser interface on top of the C ABI.

One BatchAnalyser stands for `num_channels` AnalyserTrackControllers' analysis halves
(ref AnalyserTrackController.h:199-206): per channel a RealTimeSpectralAnalyser, a
RealTimeHarmonicAnalyser and the AudioFeatures they write.  Method names follow the reference
(RealTimeAnalyser.h:111-114, :244-258; AudioDataCollector.h:124).
"""
import ctypes

import numpy as np

from . import capi


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class PackedS24(np.ndarray):
    """uint8 bytes that ARE packed 24-bit PCM (what pack_s24 returns): the tag by which push_hops / process_frames take a byte array
    as FX_SAMPLE_S24.  A plain uint8 array is never taken for it -- 8-bit data would be read as samples three bytes wide."""


def pack_s24(values):
    """int32 samples in [-2^23, 2^23) -> packed 24-bit PCM, little endian, three bytes per sample along a new last axis folded into the
    last one: [...][n] -> PackedS24 (uint8) [...][3 n] (the layout of a 24-bit WAV file's data chunk, FX_SAMPLE_S24)."""
    v = np.ascontiguousarray(values, "<i4")
    return np.ascontiguousarray(v.view(np.uint8).reshape(v.shape + (4,))[..., :3]).reshape(v.shape[:-1] + (3 * v.shape[-1],)).view(PackedS24)


_FORMAT_NAMES = {"f32": capi.SAMPLE_F32, "f16": capi.SAMPLE_F16, "s16": capi.SAMPLE_S16, "s24": capi.SAMPLE_S24}
# THE dtype-to-format table (torch's dtypes go by the same names): uint8 is packed 24-bit PCM, three bytes per sample, and only where
# the caller says so; int16 is 16-bit PCM, v / 32768 in the kernels' load stage (include/fx_wav.hpp's scaling)
_DTYPE_FORMATS = {np.dtype(np.float32): capi.SAMPLE_F32, np.dtype(np.float16): capi.SAMPLE_F16, np.dtype(np.int16): capi.SAMPLE_S16,
                  np.dtype(np.uint8): capi.SAMPLE_S24}
_torch_formats = {}                              # the same by torch's dtypes, filled when the first tensor arrives


def _describe_input(x, sample_format, device, align=16):
    """What an analysis call needs of its input x -- a numpy array (host memory) or a torch CUDA tensor on cuda:`device` whose data starts
    on an `align`-byte boundary (fx.h: 16 for whole hops and frames, 4 for blocks) -- as the tuple (ptr c_void_p, fmt capi.SAMPLE_*,
    mem capi.MEM_*, count of SAMPLES: a third of the bytes of s24, keep: what holds the memory, alive over the call, and the torch device
    of a device block, else None).  ValueError for what the library would misread, before any use of it."""
    if sample_format is not None and sample_format not in _FORMAT_NAMES:
        raise ValueError("sample_format must be one of %s" % ", ".join(sorted(_FORMAT_NAMES)))
    want = None if sample_format is None else _FORMAT_NAMES[sample_format]
    torch_input = _is_torch(x)
    if torch_input:
        if not x.is_cuda:
            raise ValueError("torch input must live on the GPU (use numpy for host buffers)")
        if not x.is_contiguous():
            raise ValueError("device input must be contiguous")
        if not _torch_formats:
            import torch
            _torch_formats.update((getattr(torch, dt.name), f) for dt, f in _DTYPE_FORMATS.items())
        fmt = _torch_formats.get(x.dtype)
        if fmt is None:                          # (a tensor is refused, not converted: the conversion would be a hidden kernel and copy)
            raise ValueError("samples must be float32, float16, int16 (16-bit PCM) or uint8 (packed 24-bit PCM)")
        tagged, size = False, x.numel()
    else:
        tagged = isinstance(x, PackedS24)
        x = np.ascontiguousarray(x)
        fmt = _DTYPE_FORMATS.get(x.dtype)
        if fmt is None:                          # float64, int32 ...: their values as float32
            x, fmt = np.ascontiguousarray(x, np.float32), capi.SAMPLE_F32
        size = x.size
    if fmt == capi.SAMPLE_S24:
        if not (tagged or want == capi.SAMPLE_S24):
            raise ValueError('uint8 samples are taken as packed 24-bit PCM only with sample_format="s24" (or as a PackedS24 array from pack_s24)')
        if size % 3:
            raise ValueError("input size is not a multiple of 3 bytes, the size of a packed 24-bit sample")
        size //= 3
    if want is not None and want != fmt:
        raise ValueError("sample_format=%r does not describe a %s %s" % (sample_format, x.dtype, "tensor" if torch_input else "array"))
    if not torch_input:
        return x.ctypes.data_as(ctypes.c_void_p), fmt, capi.MEM_HOST, size, x, None
    ptr, where = x.data_ptr(), x.device
    if ptr % align:
        raise ValueError("device input must start on a %d-byte boundary (an offset view of a tensor may not)" % align)
    if where.index != device:
        raise ValueError("input lives on %s, the analyser on cuda:%d" % (where, device))
    return ctypes.c_void_p(ptr), fmt, capi.MEM_DEVICE, size, x, where


def interleaved_dims(shape, size, fmt, num_source_channels=None):
    """(frames n, source channels K) of an interleaved block: K is num_source_channels, or the last axis of a 2-D block (in samples:
    a third of it for packed s24).  ValueError unless the block holds whole frames of K samples."""
    per = 3 if fmt == capi.SAMPLE_S24 else 1
    if num_source_channels is None:
        if len(shape) != 2:
            raise ValueError("an interleaved block is [n][K] (uint8 [n][3K] for s24), or give num_source_channels")
        if shape[1] % per:
            raise ValueError("a frame of packed 24-bit samples is a multiple of 3 bytes, not %d" % shape[1])
        num_source_channels = shape[1] // per
    K = int(num_source_channels)
    if K < 1:
        raise ValueError("an interleaved block has at least one source channel")
    if size % (K * per):
        raise ValueError("input size is not a multiple of the source channel count (%d)" % K)
    return size // (K * per), K


class BatchAnalyser:
    def __init__(self, num_channels, window_size=2048, sample_rate=48000.0, device=0,
                 order=capi.ORDER_SPECTRAL_THEN_HARMONIC, analysers="both", low_latency=False):
        """low_latency: FX_LOW_LATENCY of include/fx.h -- the kernel family for hosts that analyse one hop per call as it
        arrives and care about that hop's round trip (windows of 2048 / 4096 points: every frame on a pair of wavefronts;
        decisions identical to the default family, continuous slots may differ in the last bit)."""
        self._lib = capi.load_library()
        self.num_channels = int(num_channels)
        self.window_size = int(window_size)
        self.device = int(device)
        h = ctypes.c_void_p()
        flags = int(order) | {"both": 0, "spectral": capi.SPECTRAL_ONLY, "harmonic": capi.HARMONIC_ONLY}[analysers]
        if low_latency:
            flags |= capi.LOW_LATENCY
        capi.check(self._lib.fx_create(ctypes.byref(h), self.device, self.num_channels, self.window_size,
                                       float(sample_rate), flags))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference setters ----
    def sample_rate_changed(self, sr):                       # RealTimeAnalyser::sampleRateChanged
        capi.check(self._lib.fx_set_sample_rate(self._h, float(sr)))

    def set_onset_detection_sensitivity(self, s):            # RealTimeAnalyser.h:244
        capi.check(self._lib.fx_set_onset_sensitivity(self._h, float(s)))

    def set_onset_window_length(self, n):                    # RealTimeAnalyser.h:250
        capi.check(self._lib.fx_set_onset_window(self._h, int(n)))

    def set_onset_detection_type(self, t):                   # RealTimeAnalyser.h:258
        capi.check(self._lib.fx_set_onset_type(self._h, int(t)))

    def set_gain(self, g):                                   # AudioDataCollector::setGain
        capi.check(self._lib.fx_set_gain(self._h, float(g)))

    def reset_state(self):
        capi.check(self._lib.fx_reset_state(self._h))

    # ---- the same settings per track (include/fx.h, fx_set_channel_gains / fx_set_channel_onset; AnalyserTrackController.h:126-134) ----
    def _per_track(self, values, dtype, what):
        if values is None:
            return None, None
        a = np.ascontiguousarray(np.asarray(values, dtype=dtype).ravel())
        if a.size != self.num_channels:
            raise ValueError("per-track %s have one entry per track (%d), not %d" % (what, self.num_channels, a.size))
        return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float if dtype == np.float32 else ctypes.c_int))

    def set_channel_gains(self, gains):
        """AudioDataCollector::setGain per track: track c's hops are scaled by gains[c] from the next call on."""
        a, ptr = self._per_track(gains, np.float32, "gains")
        capi.check(self._lib.fx_set_channel_gains(self._h, ptr))

    def set_channel_onset(self, sensitivity=None, window=None, type=None):
        """Onset sensitivity / window length / detection type per track; None leaves a setting alone.  A window entry < 0 leaves that
        track's window and onset histories alone, one in [1, 32] sets it and empties that track's histories."""
        s, sp = self._per_track(sensitivity, np.float32, "sensitivities")
        w, wp = self._per_track(window, np.int32, "onset windows")
        t, tp = self._per_track(type, np.int32, "onset types")
        capi.check(self._lib.fx_set_channel_onset(self._h, sp, wp, tp))

    def channel_settings(self):
        """What each track runs with now: dict of gain, sensitivity (float32 [C]), window, type (int32 [C])."""
        C = self.num_channels
        out = {"gain": np.empty(C, np.float32), "sensitivity": np.empty(C, np.float32), "window": np.empty(C, np.int32), "type": np.empty(C, np.int32)}
        capi.check(self._lib.fx_get_channel_settings(self._h, out["gain"].ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                     out["sensitivity"].ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                     out["window"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                                     out["type"].ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    # ---- per-track reset and clear (include/fx.h, fx_reset_channels / fx_clear_pending_channels; MainComponent.cpp:137-186) ----
    def _track_list(self, channels):
        """a list of tracks as int32, checked here before any context use: integers in [0, num_channels); duplicates allowed"""
        a = np.asarray(channels if channels is not None else [])
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("a track list holds integers, not %s" % a.dtype)
        a = np.ascontiguousarray(a.ravel().astype(np.int64))
        bad = np.flatnonzero((a < 0) | (a >= self.num_channels))
        if bad.size:
            raise ValueError("entry %d: track %d out of range [0,%d)" % (int(bad[0]), int(a[bad[0]]), self.num_channels))
        a = a.astype(np.int32)
        return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def reset_channels(self, channels):
        """A new AnalyserTrackController in these slots: the listed tracks' window tail, flux state, histories, latest vector and pending
        samples become those of a new context (the pending count and every setting stay); their frame index starts at 0 again.  The
        other tracks are untouched.  Synchronises the context's stream."""
        a, ptr = self._track_list(channels)
        capi.check(self._lib.fx_reset_channels(self._h, ptr, int(a.size)))

    def clear_pending_channels(self, channels):
        """AudioDataCollector::clearBuffer on the listed tracks only: their pending samples become zeros."""
        a, ptr = self._track_list(channels)
        capi.check(self._lib.fx_clear_pending_channels(self._h, ptr, int(a.size)))

    def channel_frames(self):
        """Frames each track has analysed since it was created or last reset (int64 [C])."""
        out = np.empty(self.num_channels, np.int64)
        capi.check(self._lib.fx_get_channel_frames(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))))
        return out

    # ---- moving tracks between contexts (include/fx.h, fx_export_channels / fx_import_channels) ----
    def track_state_bytes(self):
        """Bytes of one track's record (a multiple of 16)."""
        return int(self._lib.fx_track_state_bytes(self._h))

    def export_tracks(self, channels, device=False):
        """The listed tracks' whole state, one record each: uint8 [n][track_state_bytes()], numpy or (device=True) a CUDA torch tensor.
        Duplicates allowed; nothing in the context changes.  Synchronises the context's stream: the records are valid on return."""
        a, ptr = self._track_list(channels)
        size = self.track_state_bytes()
        if device:
            import torch
            out = torch.empty((int(a.size), size), dtype=torch.uint8, device=torch.device("cuda", self.device))
            if a.size:
                self._ordered(out.device, self._lib.fx_export_channels, self._h, ptr, int(a.size), ctypes.c_void_p(out.data_ptr()), out.numel(), capi.MEM_DEVICE)
        else:
            out = np.empty((int(a.size), size), np.uint8)
            capi.check(self._lib.fx_export_channels(self._h, ptr, int(a.size), out.ctypes.data_as(ctypes.c_void_p), out.size, capi.MEM_HOST))
        return out

    def import_tracks(self, channels, state):
        """Records of export_tracks (of this or any compatible context: same window size, order, analysers, kernel family and pending
        samples) into the listed slots, record i into channels[i]; no slot twice.  `state`: uint8, numpy (any shape with the records back
        to back) or a CUDA torch tensor.  The tracks go on exactly as they would have where they were."""
        a, ptr = self._track_list(channels)
        if hasattr(state, "data_ptr"):
            if str(state.dtype) != "torch.uint8" or not state.is_cuda or not state.is_contiguous():
                raise ValueError("track records on the device are a contiguous CUDA uint8 tensor")
            self._ordered(state.device, self._lib.fx_import_channels, self._h, ptr, int(a.size), ctypes.c_void_p(state.data_ptr()), state.numel(), capi.MEM_DEVICE)
            return
        s = np.asarray(state)
        if s.dtype != np.uint8:
            raise ValueError("track records are uint8, not %s" % s.dtype)
        s = np.ascontiguousarray(s)
        capi.check(self._lib.fx_import_channels(self._h, ptr, int(a.size), s.ctypes.data_as(ctypes.c_void_p), s.size, capi.MEM_HOST))

    # ---- launch-shape knobs (within a kernel family they never change a result bit; waves_per_frame selects the family) ----
    def get_tuning(self):
        t = capi.Tuning()
        capi.check(self._lib.fx_get_tuning(self._h, ctypes.byref(t)))
        return t

    def set_tuning(self, tuning=None, **knobs):
        """Replace the context's knobs (struct fx_tuning); keyword arguments change single fields of the current ones."""
        t = tuning if tuning is not None else self.get_tuning()
        names = {f[0] for f in capi.Tuning._fields_}
        for k, v in knobs.items():
            if k not in names:                      # (setattr on a ctypes.Structure would take a mistyped name silently)
                raise ValueError("fx_tuning has no knob %r (it has: %s)" % (k, ", ".join(sorted(names))))
            if k == "unit_plan":
                t.set_plan(v)
            else:
                setattr(t, k, int(v))
        capi.check(self._lib.fx_set_tuning(self._h, ctypes.byref(t)))
        return t

    def set_test_hooks(self, bits):
        """fx_set_tuning_internal (csrc/fx_kernels.h, FX_HOOK_*): tests only, not part of include/fx.h."""
        capi.check(self._lib.fx_set_tuning_internal(self._h, int(bits)))

    def last_launches(self):
        """fx_last_launches_internal (csrc/fx_kernels.h, tests only): the launches the last analysis call made, in order, one dict each
        (capi.LAUNCH_FIELDS; 'kind' as a name: frame, frame_tail, hop, hop_pair, pair, epilogue, reblock, osc, taps, deinterleave, onset_events, osc_table,
        osc_bundle, display, sources, resample, monitor, listen, rtp)."""
        cap = capi.LAUNCH_RECORD_CAP
        buf = (ctypes.c_int * (cap * len(capi.LAUNCH_FIELDS)))()
        n = self._lib.fx_last_launches_internal(self._h, buf, cap)
        if n > cap:
            raise RuntimeError("the last call made %d launches; the record keeps %d" % (n, cap))
        out = []
        for i in range(n):
            rec = dict(zip(capi.LAUNCH_FIELDS, buf[i * len(capi.LAUNCH_FIELDS):(i + 1) * len(capi.LAUNCH_FIELDS)]))
            rec["kind"] = capi.LAUNCH_KINDS[rec["kind"]]
            out.append(rec)
        return out

    def sync(self):
        capi.check(self._lib.fx_sync(self._h))

    # ---- analysis taps: the reference's display buffers (include/fx.h, fx_request_taps) ----
    def request_taps(self, channels):
        """Arm the display buffers of these channels: the next analysis call that analyses a frame captures its first frame's."""
        ch = np.ascontiguousarray(np.atleast_1d(np.asarray(channels, dtype=np.int32)))
        capi.check(self._lib.fx_request_taps(self._h, ch.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(ch.size)))

    def taps(self, channel):
        """The latest capture of `channel`: window [N], spectrum [2N], pitch_spectrum [2N], autocorrelation [N], cnd [N],
        lag_position [2] (float32 arrays) and frame_index (int)."""
        N = self.window_size
        out = {"window": np.empty(N, np.float32), "spectrum": np.empty(2 * N, np.float32), "pitch_spectrum": np.empty(2 * N, np.float32),
               "autocorrelation": np.empty(N, np.float32), "cnd": np.empty(N, np.float32), "lag_position": np.empty(2, np.float32)}
        frame = ctypes.c_longlong()
        ptr = {k: v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for k, v in out.items()}
        capi.check(self._lib.fx_get_taps(self._h, int(channel), ptr["window"], ptr["spectrum"], ptr["pitch_spectrum"],
                                         ptr["autocorrelation"], ptr["cnd"], ptr["lag_position"], ctypes.byref(frame)))
        out["frame_index"] = frame.value
        return out

    # ---- onset events: every track's onset callback as one list made on the GPU (include/fx.h, fx_enable_onset_events) ----
    def enable_onset_events(self, capacity):
        """Enable the onset event list with room for `capacity` events (or resize it: the stored events are dropped); 0 disables it."""
        capi.check(self._lib.fx_enable_onset_events(self._h, int(capacity)))

    def onset_events(self, max_events=None):
        """Drain the list: (events, dropped).  `events` is a structured array (capi.ONSET_EVENT_DTYPE: frame i8, channel i4,
        call_frame i4) of the oldest stored events -- all of them, or at most max_events, the rest staying for the next call -- in
        the list's order (earlier calls first, then call_frame, then channel: (frame, channel) order while no track was reset on
        its own); `dropped` the events lost to overflow since the previous drain."""
        n, dropped = ctypes.c_int(0), ctypes.c_longlong(0)
        if max_events is None:
            capi.check(self._lib.fx_get_onset_events(self._h, None, 0, ctypes.byref(n), None))
            max_events = n.value
        if int(max_events) < 0:
            raise ValueError("max_events must be >= 0")
        out = np.empty(max(int(max_events), 1), capi.ONSET_EVENT_DTYPE)      # (never a null pointer: max_events == 0 is still a drain)
        capi.check(self._lib.fx_get_onset_events(self._h, out.ctypes.data_as(ctypes.c_void_p), int(max_events), ctypes.byref(n), ctypes.byref(dropped)))
        return out[:n.value].copy(), dropped.value

    # ---- audio display levels: every track's scrolling waveform, made on the GPU (include/fx.h, fx_enable_display) ----
    def enable_display(self, samples_per_block=256, length=1024):
        """Enable the audio display (AnalyserTrack.h:27-29: setSamplesPerBlock (256), setBufferSize (1024)) or resize it: every track
        becomes a new component with a ring of `length` (lo, hi) levels, one published per samples_per_block samples; length 0
        disables it."""
        capi.check(self._lib.fx_enable_display(self._h, int(samples_per_block), int(length)))
        self._display_length = int(length)

    def set_display_samples_per_block(self, n):
        """setSamplesPerBlock: in force from the next sample on; the running block keeps its count."""
        capi.check(self._lib.fx_set_display_samples_per_block(self._h, int(n)))

    def clear_display(self, channels):
        """clear() on the listed tracks: levels, running value and count become zero, the ring position stays."""
        a, ptr = self._track_list(channels)
        capi.check(self._lib.fx_clear_display_channels(self._h, ptr, int(a.size)))

    def display(self, channels=None, device=False):
        """The listed tracks' levels (None: all tracks) in drawing order, oldest first: float32 [n][length][2] of (lo, hi), numpy or
        (device=True) a CUDA torch tensor, after the analysis calls made so far."""
        if channels is None:
            n, ptr = self.num_channels, None
        else:
            a, ptr = self._track_list(channels)
            n = int(a.size)
        length = getattr(self, "_display_length", 0)
        if device:
            import torch
            out = torch.empty((n, length, 2), dtype=torch.float32, device=torch.device("cuda", self.device))
            self._ordered(out.device, self._lib.fx_get_display, self._h, ptr, n, ctypes.c_void_p(out.data_ptr() if out.numel() else 0), capi.MEM_DEVICE)
        else:
            out = np.empty((n, length, 2), np.float32)
            capi.check(self._lib.fx_get_display(self._h, ptr, n, out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return out

    def last_kernel_ms(self):
        a, b = ctypes.c_float(), ctypes.c_float()
        capi.check(self._lib.fx_last_kernel_ms(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def profile_begin(self):
        capi.check(self._lib.fx_profile_begin(self._h))

    def profile_end(self):
        """(frame kernel ms, smoothing/onset kernels ms, calls) summed since profile_begin()."""
        a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        capi.check(self._lib.fx_profile_end(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return a.value, b.value, n.value

    def stream(self):
        s = ctypes.c_void_p()
        capi.check(self._lib.fx_get_stream(self._h, ctypes.byref(s)))
        return s.value

    # ---- analysis ----
    def _ordered(self, device, fn, *args):
        """capi.check(fn(*args)) for a call whose buffers are torch's device memory, ordered against torch's current stream."""
        # The library enqueues on its own HIP stream.  Order it after the producer of the input on torch's current
        # stream, and torch's current stream after the call, both on the device (no host sync).  Because
        # the current stream waits for the analysis, anything torch later does with these blocks on that
        # stream -- reading the results, freeing and recycling the input -- is ordered after the kernels that use
        # them.  (Tensor.record_stream is deliberately not used: the allocator would record events on the
        # library's stream when the tensors die, possibly after fx_destroy has destroyed that stream.)
        # A caller that works ON the library's stream (`with torch.cuda.stream(analyser.torch_stream()):`) needs no ordering
        # at all -- and the two waits are half of a one-hop call's cost from Python (25 of 56 us: tools/py_call_overhead.py).
        import torch
        cur = torch.cuda.current_stream(device)
        lib = self._torch_stream(device)
        foreign = cur.cuda_stream != lib.cuda_stream
        if foreign:
            lib.wait_stream(cur)
        capi.check(fn(*args))
        if foreign:
            cur.wait_stream(lib)

    def _analyse(self, entry, d, counts, frames, want_raw, want_smoothed, out_raw=None, out_smoothed=None, block=False):
        """Results, ordering, call -- for every analysis entry point: library entry `entry` on the input d (_describe_input) with the
        counts fx.h puts between the pointer and the format; raw / smoothed [C][frames][12] are numpy for host input and torch for a
        device block (where out_raw / out_smoothed are used instead when given).  block: the entry takes any number of samples
        (fx_push_samples, fx_push_interleaved) -- it reports its frames, which must be `frames`, and gets no result pointer for none."""
        ptr, fmt, mem, _, _, device = d
        shape = (self.num_channels, frames, 12)
        if mem == capi.MEM_DEVICE:
            raw, sm = out_raw, out_smoothed
            for name, o in (("out_raw", raw), ("out_smoothed", sm)):
                if o is not None:
                    self._check_out(o, shape[0] * frames * 12, name)
            if (raw is None and want_raw) or (sm is None and want_smoothed):
                import torch
                raw = torch.empty(shape, dtype=torch.float32, device=device) if raw is None and want_raw else raw
                sm = torch.empty(shape, dtype=torch.float32, device=device) if sm is None and want_smoothed else sm
            results = [ctypes.c_void_p(r.data_ptr()) if r is not None else None for r in (raw, sm)]
        else:
            raw = np.empty(shape, np.float32) if want_raw else None
            sm = np.empty(shape, np.float32) if want_smoothed else None
            results = [r.ctypes.data_as(ctypes.c_void_p) if r is not None else None for r in (raw, sm)]
        if block and not frames:
            results = [None, None]
        args = (self._h, ptr) + counts + (fmt, mem, results[0], results[1])
        if block:
            frames_out = ctypes.c_int(0)
            args += (ctypes.byref(frames_out),)
        fn = getattr(self._lib, entry)
        if mem == capi.MEM_DEVICE:
            self._ordered(device, fn, *args)
        else:
            capi.check(fn(*args))
        if block:
            assert frames_out.value == frames
        return raw, sm

    def torch_stream(self):
        """The library's stream as a torch stream.  Inside `with torch.cuda.stream(analyser.torch_stream()):` the producer of
        the samples, the analysis and the consumer of the results are ordered by the stream itself, and device-buffer calls
        skip the cross-stream waits they otherwise make against torch's current stream."""
        import torch
        return self._torch_stream(torch.device("cuda", self.device))

    def _torch_stream(self, device):
        """The library's hipStream_t as a torch stream (for device-side ordering against torch's streams)."""
        s = getattr(self, "_ext_stream", None)
        if s is None:
            import torch
            s = self._ext_stream = torch.cuda.ExternalStream(self.stream(), device=device)
        return s

    def _check_out(self, o, numel, name):
        if not (_is_torch(o) and o.is_cuda and o.device.index == self.device and o.is_contiguous()
                and str(o.dtype) == "torch.float32" and o.numel() == numel):
            raise ValueError("%s must be a contiguous float32 CUDA tensor on cuda:%d with %d elements" % (name, self.device, numel))

    def _frames(self, entry, x, per_frame, want_raw, want_smoothed, out_raw, out_smoothed, sample_format):
        """Sample formats by dtype: float32, float16, int16 (16-bit PCM); packed 24-bit PCM (three bytes per sample) is a PackedS24
        array (pack_s24) or any uint8 buffer passed with sample_format="s24" -- never inferred from dtype uint8 alone.  The integer
        formats are widened in the kernels' load stage to exactly the floats a WAV reader would produce.  Device buffers must start
        on a 16-byte boundary (fx.h)."""
        d = _describe_input(x, sample_format, self.device, 16)
        T, rest = divmod(d[3], self.num_channels * per_frame)
        if rest:
            raise ValueError("input size is not a multiple of channels x samples per frame")
        return self._analyse(entry, d, (T,), T, want_raw, want_smoothed, out_raw, out_smoothed)

    def push_hops(self, hops, want_raw=True, want_smoothed=True, out_raw=None, out_smoothed=None, sample_format=None):
        """hops [C][T][N/2] -> (raw [C][T][12], smoothed [C][T][12])."""
        return self._frames("fx_push_hops", hops, self.window_size // 2, want_raw, want_smoothed, out_raw, out_smoothed, sample_format)

    def process_frames(self, frames, want_raw=True, want_smoothed=True, out_raw=None, out_smoothed=None, sample_format=None):
        """frames [C][T][N] -> (raw [C][T][12], smoothed [C][T][12])."""
        return self._frames("fx_process_frames", frames, self.window_size, want_raw, want_smoothed, out_raw, out_smoothed, sample_format)

    # ---- the collector's interface: device blocks of any length (ref AudioDataCollector.h:36-94) ----
    def pending_samples(self):
        """samples per channel that fx_push_samples is holding back (< window_size / 2)"""
        return int(self._lib.fx_pending_samples(self._h))

    def clear_buffer(self):                                  # AudioDataCollector::clearBuffer, AudioDataCollector.h:122
        capi.check(self._lib.fx_clear_pending(self._h))

    def push_samples(self, samples, want_raw=True, want_smoothed=True, sample_format=None):
        """samples [C][n] for ANY n >= 0 (a device block: 441, 480, 512 ... samples per channel) -> (raw [C][frames][12], smoothed
        [C][frames][12]) with frames = (pending + n) // (window_size / 2); what is left over stays pending in device memory.  Same bits
        as push_hops on the same stream cut into hops.  numpy (host) or torch CUDA tensors (from a 4-byte boundary), formats as push_hops."""
        d = _describe_input(samples, sample_format, self.device, 4)
        n, rest = divmod(d[3], self.num_channels)
        if rest:
            raise ValueError("input size is not a multiple of the channel count")
        frames = (self.pending_samples() + n) // (self.window_size // 2)
        return self._analyse("fx_push_samples", d, (n,), frames, want_raw, want_smoothed, block=True)

    # ---- interleaved input through a per-track channel map (include/fx.h, fx_set_channel_map / fx_push_interleaved) ----
    def set_channel_map(self, channel_map):
        """AudioDataCollector::setChannelToCollect for every track at once: track c collects source channel channel_map[c] of the
        blocks given to push_interleaved; None restores the identity.  Pending samples and histories are kept."""
        if channel_map is None:
            capi.check(self._lib.fx_set_channel_map(self._h, None))
            return
        m = np.ascontiguousarray(np.asarray(channel_map, dtype=np.int32).ravel())
        if m.size != self.num_channels:
            raise ValueError("a channel map has one entry per track (%d), not %d" % (self.num_channels, m.size))
        capi.check(self._lib.fx_set_channel_map(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))

    def push_interleaved(self, block, want_raw=True, want_smoothed=True, sample_format=None, num_source_channels=None):
        """block [n][K] of K source channels per frame (uint8 [n][3K] for s24; a flat block needs num_source_channels) -> (raw, smoothed)
        as push_samples returns them for the planar block [c][i] = block[i][map[c]].  numpy (host) or torch CUDA tensors."""
        d = _describe_input(block, sample_format, self.device, 4)
        _, fmt, _, count, keep, _ = d
        n, K = interleaved_dims(tuple(keep.shape), count * (3 if fmt == capi.SAMPLE_S24 else 1), fmt, num_source_channels)
        frames = (self.pending_samples() + n) // (self.window_size // 2)
        return self._analyse("fx_push_interleaved", d, (n, K), frames, want_raw, want_smoothed, block=True)

    # ---- RTP audio in: a tick's L16 / L24 datagrams unpacked on the GPU (include/fx.h, fx_rtp_configure .. fx_push_rtp) ----
    def rtp_configure(self, payload_format, channels_per_stream):
        """S streams of channels_per_stream[s] channels each, all "l16" or "l24" (capi.RTP_L16 / RTP_L24); every stream not running,
        every track's source none, the statistics zero.  No streams frees the unit."""
        fmt = capi.RTP_FORMATS.get(payload_format, payload_format) if isinstance(payload_format, str) else payload_format
        if isinstance(fmt, str):
            raise ValueError("a payload format is one of %s" % ", ".join(sorted(capi.RTP_FORMATS)))
        ch = np.ascontiguousarray(np.asarray(channels_per_stream, dtype=np.int32).ravel())
        capi.check(self._lib.fx_rtp_configure(self._h, int(fmt), int(ch.size), ch.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if ch.size else None))
        self._rtp = (int(ch.size), 2 if int(fmt) == capi.RTP_L16 else 3) if ch.size else None

    def set_rtp_sources(self, tracks, stream, channel=0):
        """Track tracks[i] hears channel channel[i] of stream stream[i] (one value for all is fine; stream -1 or None: none, the track
        hears zeros).  Of a track listed twice the last entry wins; the listed tracks' pending samples become zeros."""
        a, ptr = self._track_list(tracks)
        streams = list(stream) if isinstance(stream, (list, tuple, np.ndarray)) else [stream]
        s, sp = self._per_entry([-1 if x is None else x for x in streams], int(a.size))
        c, cp = self._per_entry(channel, int(a.size))
        capi.check(self._lib.fx_rtp_set_track_sources(self._h, ptr, int(a.size), sp, cp))

    def rtp_sources(self):
        """The track table: dict of stream (int32 [C], -1: none) and channel (int32 [C])."""
        out = {"stream": np.empty(self.num_channels, np.int32), "channel": np.empty(self.num_channels, np.int32)}
        ip = ctypes.POINTER(ctypes.c_int)
        capi.check(self._lib.fx_rtp_get_track_sources(self._h, out["stream"].ctypes.data_as(ip), out["channel"].ctypes.data_as(ip)))
        return out

    def set_rtp_timestamps(self, streams, timestamps):
        """Stream streams[i] runs from the next tick on, whose first sample time has the RTP timestamp timestamps[i] (mod 2^32)."""
        s = np.ascontiguousarray(np.asarray(streams, dtype=np.int32).ravel())
        t = np.ascontiguousarray((np.asarray(timestamps, dtype=np.int64).ravel() & 0xFFFFFFFF).astype(np.uint32))
        if t.size == 1 and s.size != 1:
            t = np.full(s.size, t[0], np.uint32)
        if t.size != s.size:
            raise ValueError("one timestamp per listed stream (%d), not %d" % (s.size, t.size))
        capi.check(self._lib.fx_rtp_set_cursors(self._h, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(s.size), t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))))

    def _rtp_streams(self):
        if getattr(self, "_rtp", None) is None:
            raise ValueError("RTP input is not configured (rtp_configure)")
        return self._rtp

    def rtp_timestamps(self):
        """The cursors: (timestamp uint32 [S], running int32 [S]); the host's copy, no device use."""
        S, _ = self._rtp_streams()
        t, r = np.empty(S, np.uint32), np.empty(S, np.int32)
        capi.check(self._lib.fx_rtp_get_cursors(self._h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), r.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return t, r

    def push_rtp(self, slots, lengths, stream_of, num_samples, want_raw=True, want_smoothed=True, want_disposition=True):
        """One tick of num_samples samples per track from the datagrams in `slots` (uint8 [P][stride]: numpy, or a torch CUDA tensor
        from a 4-byte boundary), datagram i the first lengths[i] bytes of slot i, from stream stream_of[i] (host arrays)
        -> (raw, smoothed, disposition): the results as push_samples returns them for the unpacked block, and one byte of
        capi.RTP_* bits per packet (None if not wanted).  P == 0 is a tick of pure loss."""
        n = int(num_samples)
        ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).ravel())
        so = np.ascontiguousarray(np.asarray(stream_of, dtype=np.int32).ravel())
        torch_input = _is_torch(slots)
        if torch_input:
            if not slots.is_cuda or not slots.is_contiguous() or str(slots.dtype) != "torch.uint8" or slots.dim() != 2:
                raise ValueError("device slots are a contiguous uint8 CUDA tensor [P][stride]")
            if slots.device.index != self.device:
                raise ValueError("the slots live on %s, the analyser on cuda:%d" % (slots.device, self.device))
            if slots.data_ptr() % 4:
                raise ValueError("device slots must start on a 4-byte boundary")
            P, stride, ptr, where = int(slots.shape[0]), int(slots.shape[1]), ctypes.c_void_p(slots.data_ptr()), slots.device
        else:
            slots = np.ascontiguousarray(slots, np.uint8)
            if slots.ndim != 2:
                raise ValueError("slots are uint8 [P][stride]")
            P, stride, ptr, where = int(slots.shape[0]), int(slots.shape[1]), slots.ctypes.data_as(ctypes.c_void_p), None
        if ln.size != P or so.size != P:
            raise ValueError("one length and one stream per slot (%d), not %d and %d" % (P, ln.size, so.size))
        frames = (self.pending_samples() + n) // (self.window_size // 2) if n > 0 else 0
        shape = (self.num_channels, frames, 12)
        if torch_input:
            import torch
            raw = torch.empty(shape, dtype=torch.float32, device=where) if want_raw else None
            sm = torch.empty(shape, dtype=torch.float32, device=where) if want_smoothed else None
            disp = torch.zeros(P, dtype=torch.uint8, device=where) if want_disposition else None
            pointers = [ctypes.c_void_p(r.data_ptr()) if r is not None and r.numel() else None for r in (raw, sm, disp)]
        else:
            raw = np.empty(shape, np.float32) if want_raw else None
            sm = np.empty(shape, np.float32) if want_smoothed else None
            disp = np.zeros(P, np.uint8) if want_disposition else None
            pointers = [r.ctypes.data_as(ctypes.c_void_p) if r is not None and r.size else None for r in (raw, sm, disp)]
        frames_out = ctypes.c_int(0)
        ip = ctypes.POINTER(ctypes.c_int)
        args = (self._h, ptr if P else None, ln.ctypes.data_as(ip) if P else None, so.ctypes.data_as(ip) if P else None, P, stride if P else 12, n,
                capi.MEM_DEVICE if torch_input else capi.MEM_HOST, pointers[0], pointers[1], ctypes.byref(frames_out), pointers[2])
        if torch_input:
            self._ordered(where, self._lib.fx_push_rtp, *args)
        else:
            capi.check(self._lib.fx_push_rtp(*args))
        assert frames_out.value == frames
        return raw, sm, disp

    def rtp_block(self, device=False):
        """The last tick's planar block as push_samples would take it: int16 [C][n] for L16, uint8 [C][3n] for L24 (numpy, or a CUDA
        torch tensor written asynchronously on the library's stream); n == 0 before the first tick."""
        _, B = self._rtp_streams()
        n, fmt, probe = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        # (no room at all: refused while a block is held, and the refusal still reports its length)
        status = self._lib.fx_rtp_get_block(self._h, ctypes.byref(probe), 0, ctypes.byref(n), ctypes.byref(fmt), capi.MEM_HOST)
        if status != capi.FX_OK and n.value == 0:
            capi.check(status)
        shape = (self.num_channels, n.value) if B == 2 else (self.num_channels, 3 * n.value)
        nbytes = self.num_channels * n.value * B
        if device:
            import torch
            out = torch.empty(shape, dtype=torch.int16 if B == 2 else torch.uint8, device=torch.device("cuda", self.device))
            if nbytes:
                self._ordered(out.device, self._lib.fx_rtp_get_block, self._h, ctypes.c_void_p(out.data_ptr()), nbytes, ctypes.byref(n), ctypes.byref(fmt), capi.MEM_DEVICE)
        else:
            out = np.empty(shape, np.int16 if B == 2 else np.uint8)
            if nbytes:
                capi.check(self._lib.fx_rtp_get_block(self._h, out.ctypes.data_as(ctypes.c_void_p), nbytes, ctypes.byref(n), ctypes.byref(fmt), capi.MEM_HOST))
        return out

    def rtp_stats(self):
        """Per stream, summed since rtp_configure: dict of int64 [S] arrays, capi.RTP_STATS_FIELDS."""
        S, _ = self._rtp_streams()
        out = np.empty((S, len(capi.RTP_STATS_FIELDS)), np.int64)
        capi.check(self._lib.fx_rtp_get_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return {name: out[:, k].copy() for k, name in enumerate(capi.RTP_STATS_FIELDS)}

    def rtp_set_window(self, window):
        """The reorder window, 0 .. capi.RTP_MAX_WINDOW sample times: what a tick's packets own up to `window` sample times beyond
        the tick is held on the device for the tick that covers it.  Discards everything held; 0 (where rtp_configure starts): none."""
        capi.check(self._lib.fx_rtp_set_window(self._h, int(window)))

    def rtp_window(self):
        """{"window": W, "held": int64 [S], the owned positions each stream holds now, "recovered": int64 [S], the block positions
        since rtp_configure / rtp_set_window that were owned only through the held state}"""
        S, _ = self._rtp_streams()
        w = ctypes.c_int(0)
        out = np.zeros((S, len(capi.RTP_WINDOW_STATS_FIELDS)), np.int64)
        capi.check(self._lib.fx_rtp_get_window(self._h, ctypes.byref(w), out.ctypes.data_as(ctypes.c_void_p)))
        return dict({"window": w.value}, **{name: out[:, k].copy() for k, name in enumerate(capi.RTP_WINDOW_STATS_FIELDS)})

    # ---- file sources: tracks play device-resident clips (include/fx.h, fx_create_clips .. fx_push_sources; AudioFilePlayer.h:41-67) ----
    def create_clips(self, samples, lengths=None, sample_format=None, borrow=False, sample_rates=None):
        """A bank of clips in device memory -> the first clip's id (the clips get consecutive ids).  `samples`: the clips back to back
        as ONE numpy array (host) or torch CUDA tensor (from a 4-byte boundary) with `lengths` in samples, or a list of numpy arrays,
        one clip each.  Formats as push_samples.  borrow=True (device tensors only): the bank refers to the tensor's memory, which
        the analyser keeps alive until destroy_clips and the caller must not change.  sample_rates: the clips' own rate in Hz, one
        for all or one per clip (set_clip_rates); None or 0: the context's."""
        if isinstance(samples, (list, tuple)):
            if lengths is not None:
                raise ValueError("a list of clips carries its own lengths")
            if not samples:
                raise ValueError("a bank holds at least one clip")
            tagged = all(isinstance(p, PackedS24) for p in samples)
            per = 3 if tagged or sample_format == "s24" else 1
            parts = [np.ascontiguousarray(p).ravel() for p in samples]
            lengths = [p.size // per for p in parts]
            samples = np.concatenate(parts)
            if tagged:
                samples = samples.view(PackedS24)
        if lengths is None:
            raise ValueError("give the clips' lengths (in samples)")
        ptr, fmt, mem, count, keep, device = _describe_input(samples, sample_format, self.device, 4)
        ls = np.ascontiguousarray(np.asarray(lengths).ravel().astype(np.int64))
        if int(ls.sum()) != count:
            raise ValueError("the clips' lengths add up to %d samples, the bank holds %d" % (int(ls.sum()), count))
        if borrow and mem != capi.MEM_DEVICE:
            raise ValueError("only a device tensor can be borrowed")
        rates = None if sample_rates is None else self._clip_rates(sample_rates, int(ls.size))
        first = ctypes.c_int(-1)
        args = (self._h, ptr, ls.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), int(ls.size), fmt, mem, capi.CLIP_BORROW if borrow else 0, ctypes.byref(first))
        if mem == capi.MEM_DEVICE:
            self._ordered(device, self._lib.fx_create_clips, *args)
            if not borrow:
                self.sync()                      # the copy has read the tensor: the caller may drop it
        else:
            capi.check(self._lib.fx_create_clips(*args))
        if borrow:
            if not hasattr(self, "_borrowed"):
                self._borrowed = {}
            self._borrowed[first.value] = keep
        if rates is not None:
            self.set_clip_rates(range(first.value, first.value + int(ls.size)), rates)
        return first.value

    @staticmethod
    def _clip_rates(rates, size):
        """one float64 per clip from a scalar or a sequence"""
        v = np.asarray(rates, dtype=np.float64).ravel()
        if v.size == 1 and size != 1:
            v = np.full(size, v[0], np.float64)
        if v.size != size:
            raise ValueError("one sample rate per clip (%d), not %d" % (size, v.size))
        return np.ascontiguousarray(v)

    def set_clip_rates(self, clip_ids, rates):
        """fx_set_clip_rates: clip clip_ids[i] is a file of rates[i] Hz (one rate for all is fine; 0: the context's rate).  A track that
        loads a clip whose rate is not the context's plays it through the resampler of include/fx.h, at the right pitch.  Refused
        while a listed clip is loaded on a track."""
        ids = np.ascontiguousarray(np.asarray(list(clip_ids), dtype=np.int32).ravel())
        v = self._clip_rates(rates, int(ids.size))
        capi.check(self._lib.fx_set_clip_rates(self._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(ids.size),
                                               v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def destroy_clips(self, first_id):
        """Frees the bank whose first clip is `first_id`; refused while a track has one of its clips loaded."""
        capi.check(self._lib.fx_destroy_clips(self._h, int(first_id)))
        getattr(self, "_borrowed", {}).pop(int(first_id), None)

    def _per_entry(self, values, size, names=None):
        """one int32 per list entry from a scalar or a sequence (names: strings that stand for values)"""
        vals = list(values) if isinstance(values, (list, tuple, np.ndarray)) else [values]
        vals = [names[x] if names and isinstance(x, str) and x in names else x for x in vals]
        if not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in vals):
            raise ValueError("expected integers%s, not %r" % (" or one of %s" % ", ".join(sorted(names)) if names else "", values))
        v = np.asarray(vals, dtype=np.int32).ravel()
        if v.size == 1 and size != 1:
            v = np.full(size, v[0], np.int32)
        if v.size != size:
            raise ValueError("one value per listed track (%d), not %d" % (size, v.size))
        v = np.ascontiguousarray(v)
        return v, v.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def load_clips(self, channels, clip_ids, loop=None):
        """loadFileIntoTransport for the listed tracks: track channels[i] gets clip clip_ids[i] (-1 or None: no file; one id for all is
        fine), looping unless loop (one flag or one per entry) says otherwise.  The tracks stop at position 0 and their pending samples
        become zeros."""
        a, ptr = self._track_list(channels)
        ids = list(clip_ids) if isinstance(clip_ids, (list, tuple, np.ndarray)) else [clip_ids]
        v, vp = self._per_entry([-1 if x is None else x for x in ids], int(a.size))
        l, lp = None, None
        if loop is not None:
            flags = list(loop) if isinstance(loop, (list, tuple, np.ndarray)) else [loop]
            l, lp = self._per_entry([int(bool(x)) for x in flags], int(a.size))
        capi.check(self._lib.fx_set_channel_clips(self._h, ptr, int(a.size), vp, lp))

    def set_sources(self, channels, sources):
        """The listed tracks listen to the live block ("input", capi.SOURCE_INPUT) or to their clip ("file", capi.SOURCE_FILE); their
        pending samples become zeros either way, and a track that goes to the input stops its player."""
        a, ptr = self._track_list(channels)
        v, vp = self._per_entry(sources, int(a.size), {"input": capi.SOURCE_INPUT, "file": capi.SOURCE_FILE})
        capi.check(self._lib.fx_set_channel_sources(self._h, ptr, int(a.size), vp))

    def transport(self, channels, command):
        """"play", "pause", "stop" or "restart" (capi.PLAY ...) for the listed tracks, as the reference's buttons: play, pause and stop
        zero the tracks' pending samples, restart keeps them and keeps the state."""
        a, ptr = self._track_list(channels)
        if isinstance(command, str):
            if command not in capi.TRANSPORT_COMMANDS:
                raise ValueError("a transport command is one of %s" % ", ".join(sorted(capi.TRANSPORT_COMMANDS)))
            command = capi.TRANSPORT_COMMANDS[command]
        capi.check(self._lib.fx_transport(self._h, ptr, int(a.size), int(command)))

    def transport_state(self):
        """The table: dict of source, state (int32 [C]; capi.SOURCE_*, capi.TRANSPORT_*), position, laps (int64 [C])."""
        C = self.num_channels
        out = {"source": np.empty(C, np.int32), "state": np.empty(C, np.int32), "position": np.empty(C, np.int64), "laps": np.empty(C, np.int64)}
        ip, llp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)
        capi.check(self._lib.fx_get_transport(self._h, out["source"].ctypes.data_as(ip), out["state"].ctypes.data_as(ip),
                                              out["position"].ctypes.data_as(llp), out["laps"].ctypes.data_as(llp)))
        return out

    def push_sources(self, live=None, num_samples=None, want_raw=True, want_smoothed=True, sample_format=None, device=False):
        """One tick: every track gets n samples -- row c of `live` ([C][n] as push_samples takes it) where the track's source is the
        input, its clip's next n samples where it plays a file, silence otherwise -- and they are analysed as push_samples analyses
        them -> (raw, smoothed).  live=None (allowed while no track listens to the input) needs num_samples and sample_format (the
        clips' format, "f32" by default -- which is also what a tick must be in while a clip with a rate of its own is loaded: the
        resampler renders fp32); device=True then returns torch tensors."""
        if live is not None:
            d = _describe_input(live, sample_format, self.device, 4)
            n, rest = divmod(d[3], self.num_channels)
            if rest:
                raise ValueError("input size is not a multiple of the channel count")
            if num_samples is not None and int(num_samples) != n:
                raise ValueError("the live block holds %d samples per track, not %d" % (n, int(num_samples)))
        else:
            if num_samples is None:
                raise ValueError("a tick without a live block needs num_samples")
            name = "f32" if sample_format is None else sample_format
            if name not in _FORMAT_NAMES:
                raise ValueError("sample_format must be one of %s" % ", ".join(sorted(_FORMAT_NAMES)))
            n, where = int(num_samples), None
            if device:
                import torch
                where = torch.device("cuda", self.device)
            d = (None, _FORMAT_NAMES[name], capi.MEM_DEVICE if device else capi.MEM_HOST, 0, None, where)
        frames = (self.pending_samples() + n) // (self.window_size // 2) if n > 0 else 0
        return self._analyse("fx_push_sources", d, (n,), frames, want_raw, want_smoothed, block=True)

    # ---- monitor mix: every tick's tracks summed to a stereo output (include/fx.h, fx_enable_monitor .. fx_get_monitor) ----
    def enable_monitor(self, enable=True):
        """Make the monitor (every send off, gains 1 / 1, no tick yet) or free it; enabling an enabled monitor keeps its sends.  While
        it is enabled every push_sources tick also mixes what the tracks play down to two output channels on the device."""
        capi.check(self._lib.fx_enable_monitor(self._h, 1 if enable else 0))

    def _gains(self, values, size, what):
        """one finite float32 per list entry from a scalar or a sequence; None stays None (that gain is kept)"""
        if values is None:
            return None, None
        v = np.asarray(values, dtype=np.float32).ravel()
        if v.size == 1 and size != 1:
            v = np.full(size, v[0], np.float32)
        if v.size != size:
            raise ValueError("one %s gain per listed track (%d), not %d" % (what, size, v.size))
        bad = np.flatnonzero(~np.isfinite(v))
        if bad.size:
            raise ValueError("entry %d: the %s gain %r is not a finite number" % (int(bad[0]), what, float(v[bad[0]])))
        v = np.ascontiguousarray(v)
        return v, v.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def set_monitor(self, channels, on=True, left=None, right=None):
        """The listed tracks' sends: on (one flag or one per entry), left / right gain (one value or one per entry; None keeps it).
        Of a track listed twice the last entry wins.  In force from the next tick on."""
        a, ptr = self._track_list(channels)
        flags = list(on) if isinstance(on, (list, tuple, np.ndarray)) else [on]
        o, op = self._per_entry([int(bool(x)) for x in flags], int(a.size))
        l, lp = self._gains(left, int(a.size), "left")
        r, rp = self._gains(right, int(a.size), "right")
        capi.check(self._lib.fx_set_channel_monitor(self._h, ptr, int(a.size), op, lp, rp))

    def monitor_sends(self):
        """The send table: dict of on (int32 [C]), left, right (float32 [C])."""
        C = self.num_channels
        out = {"on": np.empty(C, np.int32), "left": np.empty(C, np.float32), "right": np.empty(C, np.float32)}
        fp = ctypes.POINTER(ctypes.c_float)
        capi.check(self._lib.fx_get_channel_monitor(self._h, out["on"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), out["left"].ctypes.data_as(fp),
                                                    out["right"].ctypes.data_as(fp)))
        return out

    def get_monitor(self, device=False):
        """The last tick's mix, float32 [2][n] (left, right; n == 0 before the first tick): numpy, or (device=True) a CUDA torch tensor
        written asynchronously on the library's stream."""
        n, probe = ctypes.c_int(0), ctypes.c_float(0.0)
        # (no room at all: refused while a mix is held, and the refusal still reports the mix's length)
        status = self._lib.fx_get_monitor(self._h, ctypes.byref(probe), 0, ctypes.byref(n), capi.MEM_HOST)
        if status != capi.FX_OK and n.value == 0:
            capi.check(status)
        if device:
            import torch
            out = torch.empty((2, n.value), dtype=torch.float32, device=torch.device("cuda", self.device))
            if n.value:
                self._ordered(out.device, self._lib.fx_get_monitor, self._h, ctypes.c_void_p(out.data_ptr()), n.value, ctypes.byref(n), capi.MEM_DEVICE)
        else:
            out = np.empty((2, n.value), np.float32)
            if n.value:
                capi.check(self._lib.fx_get_monitor(self._h, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n), capi.MEM_HOST))
        return out

    # ---- listening tracks: analysers hear the monitor output (include/fx.h, "Listening tracks") ----
    def set_listen(self, channels, listen):
        """What the listed tracks' analysers hear from the next tick on: "self" (capi.LISTEN_SELF, the track's own row), "left" or
        "right" (capi.LISTEN_LEFT / LISTEN_RIGHT: that output of the monitor mix); one value or one per entry.  Of a track listed twice
        the last entry wins.  The listed tracks' pending samples become zeros, also where nothing changes.  Needs the monitor."""
        a, ptr = self._track_list(channels)
        v, vp = self._per_entry(listen, int(a.size), capi.LISTENS)
        bad = np.flatnonzero((v < capi.LISTEN_SELF) | (v > capi.LISTEN_RIGHT))
        if bad.size:
            raise ValueError("entry %d: unknown listen %d (one of %s)" % (int(bad[0]), int(v[bad[0]]), ", ".join(sorted(capi.LISTENS))))
        capi.check(self._lib.fx_set_channel_listen(self._h, ptr, int(a.size), vp))

    def listens(self):
        """What every track hears: int32 [C] of capi.LISTEN_*."""
        out = np.empty(self.num_channels, np.int32)
        capi.check(self._lib.fx_get_channel_listen(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return out

    def get_features(self, out=None):
        """Latest AudioFeatures::getValue of every slot, [C][12]: a host array, or -- with `out`, a contiguous
        float32 CUDA tensor of that shape -- an asynchronous device copy on the library's stream (what the OSC
        sink of a sharded run gathers)."""
        if out is not None:
            self._check_out(out, self.num_channels * 12, "out")
            self._ordered(out.device, self._lib.fx_get_smoothed, self._h, ctypes.c_void_p(out.data_ptr()), capi.MEM_DEVICE)
            return out
        out = np.empty((self.num_channels, 12), np.float32)
        capi.check(self._lib.fx_get_smoothed(self._h, out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return out

    def set_osc_addresses(self, addresses):
        """fx_set_osc_addresses: every track's own OSC address (the reference's per-track bundleAddress, AnalyserTrackController.h:17,146),
        one str / bytes per track, or None to drop the table.  A setting: resets keep it.  Synchronises the context's stream."""
        if addresses is None:
            capi.check(self._lib.fx_set_osc_addresses(self._h, None))
            return
        addresses = list(addresses)
        if len(addresses) != self.num_channels:
            raise ValueError("one OSC address per track (%d), not %d" % (self.num_channels, len(addresses)))
        capi.check(self._lib.fx_set_osc_addresses(self._h, capi.c_strings(addresses)))

    def osc_address_stride(self):
        """fx_osc_address_stride: the longest message of the address table, or -1 without one"""
        return self._lib.fx_osc_address_stride(self._h)

    def osc_datagrams(self, prefix="/Audio/A", first_channel=0, stride=None, addressed=False):
        """fx_get_osc_datagrams: every channel's wire-ready OSC feature message, written on the device from the latest smoothed vectors
        (ref OSCFeatureAnalysisOutput.h:89-113, MainComponent.cpp:170).  Returns (datagrams uint8 [C][stride], lengths int32 [C]).
        addressed=True: fx_get_osc_datagrams_addressed, the addresses of set_osc_addresses instead of prefix and first_channel."""
        if addressed:
            stride = self.osc_address_stride() if stride is None else int(stride)
            out = np.empty((self.num_channels, max(stride, 0)), np.uint8)
            lengths = np.empty(self.num_channels, np.int32)
            capi.check(self._lib.fx_get_osc_datagrams_addressed(self._h, out.ctypes.data_as(ctypes.c_void_p), stride,
                                                                lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), capi.MEM_HOST))
            return out, lengths
        stride = capi.osc_stride(prefix, first_channel, self.num_channels) if stride is None else int(stride)
        out = np.empty((self.num_channels, stride), np.uint8)
        lengths = np.empty(self.num_channels, np.int32)
        capi.check(self._lib.fx_get_osc_datagrams(self._h, prefix.encode(), int(first_channel), out.ctypes.data_as(ctypes.c_void_p), stride,
                                                  lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), capi.MEM_HOST))
        return out, lengths

    def osc_bundles(self, prefix="/Audio/A", first_channel=0, addressed=False, timetag=capi.OSC_TIMETAG_IMMEDIATE, max_datagram_bytes=1472, device=False):
        """fx_get_osc_bundles: the same messages as OSC 1.0 bundles, K tracks per datagram (capi.osc_bundle_plan), formed on the device in
        one launch.  Returns (bundles uint8 [B][stride], lengths int32 [B]); datagram b = bundles[b, :lengths[b]].  addressed=True:
        fx_get_osc_bundles_addressed, the addresses of set_osc_addresses.  device=True: the bundles stay on the GPU, a torch uint8
        tensor written asynchronously on the library's stream."""
        longest = self.osc_address_stride() if addressed else capi.osc_stride(prefix, first_channel, self.num_channels)
        if longest < 0:
            raise capi.FxError(capi.FX_ERR_INVALID_ARGUMENT, "the context has no OSC address table (set_osc_addresses)")
        _, bundles, stride = capi.osc_bundle_plan(longest, self.num_channels, max_datagram_bytes)
        lengths = np.empty(bundles, np.int32)
        lp = lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        if device:
            import torch
            out = torch.empty((bundles, stride), dtype=torch.uint8, device=torch.device("cuda", self.device))
            ptr, kind = ctypes.c_void_p(out.data_ptr()), capi.MEM_DEVICE
        else:
            out = np.empty((bundles, stride), np.uint8)
            ptr, kind = out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST
        if addressed:
            args = (self._lib.fx_get_osc_bundles_addressed, self._h, int(timetag), int(max_datagram_bytes), ptr, stride, lp, kind)
        else:
            args = (self._lib.fx_get_osc_bundles, self._h, prefix.encode(), int(first_channel), int(timetag), int(max_datagram_bytes), ptr, stride, lp, kind)
        if device:
            self._ordered(out.device, *args)
        else:
            capi.check(args[0](*args[1:]))
        return out, lengths

    # ---- multi-GPU: gather of the latest smoothed vectors to the OSC sink rank (RCCL, through the C ABI) ----
    @staticmethod
    def comm_unique_id():
        """bytes to hand to every rank's comm_create (rank 0 creates them)."""
        buf = ctypes.create_string_buffer(capi.COMM_ID_BYTES)
        capi.check(capi.load_library().fx_comm_unique_id(buf, capi.COMM_ID_BYTES))
        return buf.raw

    def comm_create(self, rank, world_size, unique_id):
        capi.check(self._lib.fx_comm_create(self._h, int(rank), int(world_size), ctypes.c_char_p(unique_id), len(unique_id)))
        self._world = int(world_size)

    def comm_destroy(self):
        capi.check(self._lib.fx_comm_destroy(self._h))

    def comm_layout(self):
        """(total channels over all ranks, [first channel of rank r])."""
        total = ctypes.c_int()
        first = (ctypes.c_int * self._world)()
        capi.check(self._lib.fx_comm_layout(self._h, ctypes.byref(total), first))
        return total.value, list(first)

    def gather_features(self, dst=0, out=None):
        """Asynchronous gather of every rank's latest smoothed vectors to rank `dst`.  `out`: on dst a host
        array or contiguous float32 CUDA tensor of [total_channels][12]; valid after comm_sync()."""
        if out is None:
            capi.check(self._lib.fx_gather_smoothed(self._h, int(dst), None, capi.MEM_DEVICE))
        elif _is_torch(out):
            total, _ = self.comm_layout()
            self._check_out(out, total * 12, "out")
            capi.check(self._lib.fx_gather_smoothed(self._h, int(dst), ctypes.c_void_p(out.data_ptr()), capi.MEM_DEVICE))
        else:
            if not (out.dtype == np.float32 and out.flags.c_contiguous):
                raise ValueError("out must be a C-contiguous float32 array")
            capi.check(self._lib.fx_gather_smoothed(self._h, int(dst), out.ctypes.data_as(ctypes.c_void_p), capi.MEM_HOST))
        return out

    def comm_sync(self):
        capi.check(self._lib.fx_comm_sync(self._h))

    def comm_stats(self):
        """fx_comm_stats: RCCL's rank count, gathers issued / timed, their summed and longest device time (ms) on the side stream."""
        n, g, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        tot, mx = ctypes.c_double(), ctypes.c_double()
        capi.check(self._lib.fx_comm_stats(self._h, ctypes.byref(n), ctypes.byref(g), ctypes.byref(t), ctypes.byref(tot), ctypes.byref(mx)))
        return {"rccl_ranks": n.value, "gathers": g.value, "gathers_timed": t.value, "gather_ms_total": tot.value, "gather_ms_max": mx.value,
                "gather_ms_mean": tot.value / t.value if t.value else None}


class HopStream:
    """Streaming ingest on top of a BatchAnalyser: the stand-in for AudioDataCollector's ring
    (ref AudioDataCollector.h:36-94).  Batches of `hops_per_batch` hops per channel are written into
    pinned host slots; the copy to the GPU runs on a side stream and overlaps the previous batch's
    analysis; results come back in order."""

    def __init__(self, analyser, hops_per_batch, slots=3, dtype=np.float32):
        self._an = analyser
        self._lib = analyser._lib
        self.hops = int(hops_per_batch)
        self.slots = int(slots)
        self.dtype = np.dtype(dtype)
        fmt = _DTYPE_FORMATS.get(self.dtype)
        if fmt is None:
            raise ValueError("HopStream samples are float32, float16, int16 (16-bit PCM) or uint8 (packed 24-bit PCM, three bytes per sample)")
        h = ctypes.c_void_p()
        capi.check(self._lib.fx_stream_create(analyser._h, self.hops, self.slots, fmt, ctypes.byref(h)))
        self._h = h
        self._shape = (analyser.num_channels, self.hops, (analyser.window_size // 2) * (3 if self.dtype == np.uint8 else 1))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fx_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def in_flight(self):
        return int(self._lib.fx_stream_in_flight(self._h))

    def slot(self):
        """numpy view [C][hops][N/2] of the next pinned slot to fill."""
        p = ctypes.c_void_p()
        capi.check(self._lib.fx_stream_acquire(self._h, ctypes.byref(p)))
        n = int(np.prod(self._shape))
        buf = (ctypes.c_char * (n * self.dtype.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=self.dtype).reshape(self._shape)

    def submit(self):
        capi.check(self._lib.fx_stream_submit(self._h))

    def push(self, hops, fill_threads=1):
        """Copy one batch into the next slot and submit it.  fill_threads > 1: the copy is made by that many host threads inside
        the library (fx_stream_push) -- for batches of many megabytes, where one thread's memcpy is several times slower than PCIe."""
        hops = np.asarray(hops, self.dtype)
        if hops.size != int(np.prod(self._shape)):
            raise ValueError("a batch is %r samples" % (self._shape,))
        if fill_threads > 1:
            hops = np.ascontiguousarray(hops)
            capi.check(self._lib.fx_stream_push(self._h, hops.ctypes.data_as(ctypes.c_void_p), int(fill_threads)))
            return
        self.slot()[...] = hops.reshape(self._shape)
        self.submit()

    def push_samples(self, samples, fill_threads=1):
        """A block of n samples per channel, [C][n] with 0 <= n <= hops_per_batch * window_size / 2 (a device callback's block), into the
        next slot: fx_stream_push_samples.  collect_samples() returns what the context's pending samples and the block yielded.
        (No sample_format argument, unlike BatchAnalyser.push_samples: a ring's format is fixed when it is created -- `dtype` of HopStream,
        uint8 = packed 24-bit -- and the block is converted to it.)"""
        x = np.ascontiguousarray(samples, self.dtype)
        per = 3 if self.dtype == np.uint8 else 1
        C = self._shape[0]
        if x.size % (C * per):
            raise ValueError("input size is not a multiple of the channel count")
        capi.check(self._lib.fx_stream_push_samples(self._h, x.ctypes.data_as(ctypes.c_void_p), x.size // (C * per), int(fill_threads)))

    def collect_samples(self, want_raw=True, want_smoothed=True):
        """(raw [C][frames][12], smoothed [C][frames][12]) of the oldest batch; frames may be 0 for a block that completed no hop."""
        C = self._shape[0]
        raw = np.empty((C, self.hops, 12), np.float32)
        sm = np.empty((C, self.hops, 12), np.float32)
        n = ctypes.c_int(0)
        capi.check(self._lib.fx_stream_collect_samples(self._h, raw.ctypes.data_as(ctypes.c_void_p), sm.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
        f = n.value
        flat_r, flat_s = raw.reshape(-1)[:C * f * 12].reshape(C, f, 12), sm.reshape(-1)[:C * f * 12].reshape(C, f, 12)
        return (flat_r.copy() if want_raw else None), (flat_s.copy() if want_smoothed else None)

    def collect(self, want_raw=True, want_smoothed=True):
        C = self._shape[0]
        raw = np.empty((C, self.hops, 12), np.float32) if want_raw else None
        sm = np.empty((C, self.hops, 12), np.float32) if want_smoothed else None
        capi.check(self._lib.fx_stream_collect(self._h,
                                               raw.ctypes.data_as(ctypes.c_void_p) if raw is not None else None,
                                               sm.ctypes.data_as(ctypes.c_void_p) if sm is not None else None))
        return raw, sm
