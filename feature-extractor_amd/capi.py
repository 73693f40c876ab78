"""ctypes binding of include/fx.h (libfx_hip.so)."""
import ctypes
import os

import numpy as np

from . import build as _build

NUM_FEATURES = 12
(ONSET, RMS, F0, CENTROID, SPREAD, FLATNESS, LER, FLUX, SLOPE, HER, OER, INHARM) = range(12)
FEATURE_NAMES = ["onset", "rms", "f0", "centroid", "spread", "flatness", "ler", "flux",
                 "slope", "her", "oer", "inharm"]
ONSET_SPECTRAL, ONSET_AMPLITUDE, ONSET_COMBINATION = 0, 1, 2
ORDER_SPECTRAL_THEN_HARMONIC, ORDER_HARMONIC_THEN_SPECTRAL, ORDER_ISOLATED = 0, 1, 2
SPECTRAL_ONLY, HARMONIC_ONLY, LOW_LATENCY = 4, 8, 16
MEM_HOST, MEM_DEVICE = 0, 1
SAMPLE_F32, SAMPLE_F16, SAMPLE_S16, SAMPLE_S24 = 0, 1, 2, 3
FX_OK, FX_ERR_INVALID_ARGUMENT, FX_ERR_NO_DEVICE, FX_ERR_HIP, FX_ERR_OUT_OF_MEMORY, FX_ERR_UNSUPPORTED = range(6)

COMM_ID_BYTES = 128
ABI_VERSION = 6
MAX_UNITS = 24
# fx_last_launches_internal (csrc/fx_kernels.h, tests only): struct fx_launch_record, field by field, and FX_LAUNCH_* by number
LAUNCH_FIELDS = ["kind", "window", "analysers", "T", "direct_state", "block_mode", "num_chunks", "ch_per_wg", "waves_per_ch", "hop_pairs",
                 "ep_T", "out_stride", "ep_form", "reblock"]
LAUNCH_KINDS = {1: "frame", 2: "frame_tail", 3: "hop", 4: "hop_pair", 5: "pair", 6: "epilogue", 7: "reblock", 8: "osc", 9: "taps",
                10: "deinterleave", 11: "onset_events", 12: "osc_table", 13: "osc_bundle", 14: "display", 15: "sources", 16: "resample", 17: "monitor",
                18: "listen", 19: "rtp"}
# file sources (include/fx.h): FX_SOURCE_*, FX_TRANSPORT_*, the fx_transport commands FX_PLAY .. FX_RESTART, FX_CLIP_BORROW
SOURCE_INPUT, SOURCE_FILE = 0, 1
TRANSPORT_NO_FILE, TRANSPORT_PLAYING, TRANSPORT_PAUSED, TRANSPORT_STOPPED, TRANSPORT_FINISHED = range(5)
PLAY, PAUSE, STOP, RESTART = range(4)
TRANSPORT_COMMANDS = {"play": PLAY, "pause": PAUSE, "stop": STOP, "restart": RESTART}
CLIP_BORROW = 1
# RTP input (include/fx.h): FX_RTP_L16 / FX_RTP_L24, the disposition bits FX_RTP_*, struct fx_rtp_stats' fields in order
RTP_L16, RTP_L24 = 0, 1
RTP_FORMATS = {"l16": RTP_L16, "l24": RTP_L24}
RTP_PLACED, RTP_LATE, RTP_EARLY, RTP_MALFORMED, RTP_IGNORED = 1, 2, 4, 8, 16
RTP_STATS_FIELDS = ["packets", "malformed", "late_packets", "early_packets", "samples_placed", "samples_missing"]
# the reorder window: FX_RTP_HELD, FX_RTP_MAX_WINDOW, struct fx_rtp_window_stats' fields in order
RTP_HELD = 32
RTP_MAX_WINDOW = 65536
RTP_WINDOW_STATS_FIELDS = ["held", "recovered"]
MONITOR_GROUP = 64                  # FX_MONITOR_GROUP: the tracks whose sends are summed in a row before the groups are
LISTEN_SELF, LISTEN_LEFT, LISTEN_RIGHT = 0, 1, 2       # FX_LISTEN_*: what a track's analysers hear (fx_set_channel_listen)
LISTENS = {"self": LISTEN_SELF, "left": LISTEN_LEFT, "right": LISTEN_RIGHT}
MAX_DISPLAY_LENGTH, MAX_DISPLAY_SAMPLES_PER_BLOCK = 4096, 65536
MAX_TAP_CHANNELS = 64
OSC_ADDRESS_MAX = 124               # FX_OSC_ADDRESS_MAX
OSC_SENDER_MAX_TARGETS = 64         # FX_OSC_SENDER_MAX_TARGETS
OSC_BUNDLE_MAX_ELEMENTS = 1024      # FX_OSC_BUNDLE_MAX_ELEMENTS
OSC_TIMETAG_IMMEDIATE = 1           # FX_OSC_TIMETAG_IMMEDIATE
LAUNCH_RECORD_CAP = 8
# the offline driver (include/fx.h): FX_OFFLINE_* feature rows (ref AudioFeatures.h:20-31, less FFT), FX_OFFLINE_DO_*, FX_OFFLINE_SCRATCH_BYTES
(OFFLINE_CENTROID, OFFLINE_SLOPE, OFFLINE_SPREAD, OFFLINE_FLATNESS, OFFLINE_FLUX, OFFLINE_ZERO_CROSSES, OFFLINE_F0, OFFLINE_HER,
 OFFLINE_INHARMONICITY, OFFLINE_AUDIO, OFFLINE_FEATURE_ROWS) = range(11)
OFFLINE_DO_SPECTRAL, OFFLINE_DO_HARMONIC, OFFLINE_DO_ZERO_CROSSES, OFFLINE_DO_AUDIO, OFFLINE_DO_NORMALISE_AUDIO, OFFLINE_DO_LOG_ATTACK = 1, 2, 4, 8, 16, 32
OFFLINE_SCRATCH_BYTES = 16 << 20
OFFLINE_WINDOWS = (256, 512, 1024, 2048, 4096)
OFFLINE_SORT_CHUNK = 8192           # FX_OFFLINE_SORT_CHUNK: the longest row fx_offline_feature_distribution sorts wholly in LDS
OFFLINE_SMOOTHED_FEATURES, OFFLINE_MAX_SMOOTHING_DEPTH = 9, 64      # SmoothedFeatures' rows (ref AudioFeatures.h:360), fx_offline_smoothing's depths


class OscSenderStats(ctypes.Structure):
    """struct fx_osc_sender_stats of include/fx.h"""
    _fields_ = [("ticks", ctypes.c_longlong), ("late_ticks", ctypes.c_longlong), ("datagrams", ctypes.c_longlong), ("dropped", ctypes.c_longlong),
                ("syscalls", ctypes.c_longlong), ("last_tick_ms", ctypes.c_double), ("max_tick_ms", ctypes.c_double), ("total_tick_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OnsetEvent(ctypes.Structure):
    """struct fx_onset_event of include/fx.h: one (track, frame) whose raw onset slot is 1"""
    _fields_ = [("frame", ctypes.c_longlong), ("channel", ctypes.c_int), ("call_frame", ctypes.c_int)]


# the same record as a numpy structured type (BatchAnalyser.onset_events)
ONSET_EVENT_DTYPE = np.dtype([("frame", np.int64), ("channel", np.int32), ("call_frame", np.int32)])
MAX_ONSET_EVENTS = 1 << 26


class Tuning(ctypes.Structure):
    """struct fx_tuning of include/fx.h: launch-shape knobs.  Within a kernel family none changes a result bit;
    waves_per_frame selects the family (include/fx.h, FX_LOW_LATENCY) and cannot change once frames have been analysed."""
    _fields_ = [("waves_per_channel", ctypes.c_int), ("channels_per_workgroup", ctypes.c_int), ("waves_per_frame", ctypes.c_int),
                ("frames_per_unit", ctypes.c_int), ("unit_plan_len", ctypes.c_int), ("unit_plan", ctypes.c_int * MAX_UNITS),
                ("stream_graph", ctypes.c_int), ("stream_hop_kernel", ctypes.c_int), ("stream_zero_copy", ctypes.c_int),
                ("one_hop_kernel", ctypes.c_int), ("call_timing", ctypes.c_int), ("handover_spin_limit", ctypes.c_int), ("stream_fill_streaming", ctypes.c_int)]

    @classmethod
    def defaults(cls):
        t = cls()
        load_library().fx_tuning_defaults(ctypes.byref(t))
        return t

    @classmethod
    def from_env(cls):
        t = cls()
        load_library().fx_tuning_from_env(ctypes.byref(t))
        return t

    def set_plan(self, sizes):
        self.unit_plan_len = len(sizes)
        for k, v in enumerate(sizes):
            self.unit_plan[k] = int(v)
        return self


def _prototypes():
    vp, i, u, f, d, ll, cp = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_char_p
    P = ctypes.POINTER
    vpp, ip, fp, dp, llp, tp, strings = P(vp), P(i), P(f), P(d), P(ll), P(Tuning), P(cp)
    ull = ctypes.c_ulonglong
    st = i                  # fx_status and int: ctypes' default restype (fx_track_state_bytes' size_t is at most 2432 + 6 * 4096: read as int)
    return [
        ("fx_create", [vpp, i, i, i, d, u], st), ("fx_destroy", [vp], st), ("fx_reset_state", [vp], st),
        ("fx_set_sample_rate", [vp, d], st), ("fx_set_onset_sensitivity", [vp, f], st), ("fx_set_onset_window", [vp, i], st),
        ("fx_set_onset_type", [vp, i], st), ("fx_set_gain", [vp, f], st),
        ("fx_set_channel_gains", [vp, fp], st), ("fx_set_channel_onset", [vp, fp, ip, ip], st), ("fx_get_channel_settings", [vp, fp, fp, ip, ip], st),
        ("fx_reset_channels", [vp, ip, i], st), ("fx_clear_pending_channels", [vp, ip, i], st), ("fx_get_channel_frames", [vp, llp], st),
        ("fx_track_state_bytes", [vp], st), ("fx_export_channels", [vp, ip, i, vp, ctypes.c_size_t, i], st),
        ("fx_import_channels", [vp, ip, i, vp, ctypes.c_size_t, i], st),
        ("fx_push_hops", [vp, vp, i, i, i, vp, vp], st), ("fx_push_samples", [vp, vp, i, i, i, vp, vp, ip], st),
        ("fx_set_channel_map", [vp, ip], st), ("fx_push_interleaved", [vp, vp, i, i, i, i, vp, vp, ip], st),
        ("fx_pending_samples", [vp], st), ("fx_clear_pending", [vp], st),
        ("fx_rtp_configure", [vp, i, i, ip], st), ("fx_rtp_set_track_sources", [vp, ip, i, ip, ip], st), ("fx_rtp_get_track_sources", [vp, ip, ip], st),
        ("fx_rtp_set_cursors", [vp, ip, i, P(u)], st), ("fx_rtp_get_cursors", [vp, P(u), ip], st),
        ("fx_push_rtp", [vp, vp, ip, ip, i, i, i, i, vp, vp, ip, vp], st), ("fx_rtp_get_block", [vp, vp, ctypes.c_size_t, ip, ip, i], st),
        ("fx_rtp_get_stats", [vp, vp], st), ("fx_rtp_set_window", [vp, i], st), ("fx_rtp_get_window", [vp, ip, vp], st),
        ("fx_create_clips", [vp, vp, llp, i, i, i, u, ip], st), ("fx_destroy_clips", [vp, i], st), ("fx_set_channel_clips", [vp, ip, i, ip, ip], st),
        ("fx_set_clip_rates", [vp, ip, i, dp], st), ("fx_get_resampler_table", [fp, i, ip, ip], st),
        ("fx_set_channel_sources", [vp, ip, i, ip], st), ("fx_transport", [vp, ip, i, i], st), ("fx_get_transport", [vp, ip, ip, llp, llp], st),
        ("fx_push_sources", [vp, vp, i, i, i, vp, vp, ip], st),
        ("fx_enable_monitor", [vp, i], st), ("fx_set_channel_monitor", [vp, ip, i, ip, fp, fp], st), ("fx_get_channel_monitor", [vp, ip, fp, fp], st),
        ("fx_get_monitor", [vp, vp, i, ip, i], st), ("fx_set_channel_listen", [vp, ip, i, ip], st), ("fx_get_channel_listen", [vp, ip], st),
        ("fx_process_frames", [vp, vp, i, i, i, vp, vp], st),
        ("fx_get_smoothed", [vp, vp, i], st), ("fx_host_alloc", [vpp, ctypes.c_size_t], st), ("fx_host_free", [vp], st),
        ("fx_sync", [vp], st), ("fx_get_stream", [vp, vpp], st), ("fx_last_kernel_ms", [vp, fp, fp], st),
        ("fx_request_taps", [vp, ip, i], st), ("fx_get_taps", [vp, i, fp, fp, fp, fp, fp, fp, llp], st),
        ("fx_enable_onset_events", [vp, i], st), ("fx_get_onset_events", [vp, vp, i, ip, llp], st),
        ("fx_enable_display", [vp, i, i], st), ("fx_set_display_samples_per_block", [vp, i], st),
        ("fx_clear_display_channels", [vp, ip, i], st), ("fx_get_display", [vp, ip, i, vp, i], st),
        ("fx_stream_create", [vp, i, i, i, vpp], st), ("fx_stream_destroy", [vp], st), ("fx_stream_acquire", [vp, vpp], st),
        ("fx_stream_submit", [vp], st), ("fx_stream_push", [vp, vp, i], st), ("fx_stream_collect", [vp, vp, vp], st),
        ("fx_stream_submit_samples", [vp, i], st), ("fx_stream_push_samples", [vp, vp, i, i], st),
        ("fx_stream_collect_samples", [vp, vp, vp, ip], st), ("fx_stream_in_flight", [vp], st),
        ("fx_tuning_defaults", [tp], None), ("fx_tuning_from_env", [tp], None), ("fx_get_tuning", [vp, tp], st), ("fx_set_tuning", [vp, tp], st),
        ("fx_plan_units", [i, u, i, i, tp, ip, i], st), ("fx_twiddle_symmetry", [i], st),
        ("fx_profile_begin", [vp], st), ("fx_profile_end", [vp, dp, dp, ip], st),
        ("fx_comm_unique_id", [vp, i], st), ("fx_comm_create", [vp, i, i, vp, i], st), ("fx_comm_destroy", [vp], st),
        ("fx_comm_layout", [vp, ip, ip], st), ("fx_gather_smoothed", [vp, i, vp, i], st), ("fx_comm_sync", [vp], st),
        ("fx_comm_stats", [vp, ip, ip, ip, dp, dp], st),
        ("fx_offline_create", [vpp, i, i, d], st), ("fx_offline_destroy", [vp], st), ("fx_offline_reset", [vp], st), ("fx_offline_sync", [vp], st),
        ("fx_offline_get_previous_f0", [vp, dp], st), ("fx_offline_zero_crosses", [vp, vp, i, i, vp, i], st),
        ("fx_offline_log_attack_time", [vp, vp, i, i, i, i, vp, i], st), ("fx_offline_fft_lbp", [vp, vp, vp, i, vp, vp, vp, i], st),
        ("fx_offline_harmonic_characteristics", [vp, vp, i, vp, i], st), ("fx_offline_spectral_characteristics", [vp, vp, i, vp, i], st),
        ("fx_offline_get_previous_bins", [vp, dp, i], st), ("fx_offline_spectral_slope", [vp, vp, i, vp, i], st),
        ("fx_offline_auto_correlation", [vp, vp, i, vp, vp, i], st),
        ("fx_offline_frames", [vp, vp, i, i, i, vp, vp, i], st), ("fx_offline_analyse", [vp, vp, i, i, i, i, u, vp, vp, vp, vp, i], st),
        ("fx_offline_analyse_files", [vp, vp, llp, i, i, i, ip, u, vp, vp, vp, vp, i], st),
        ("fx_offline_set_nyquists", [vp, dp], st), ("fx_offline_get_nyquists", [vp, dp], st),
        ("fx_offline_feature_ranges", [vp, vp, i, i, vp, i], st), ("fx_offline_feature_distribution", [vp, vp, i, i, i, vp, i], st),
        ("fx_offline_smoothing", [vp, i], st), ("fx_offline_smooth_rows", [vp, vp, i, i, i, vp, i], st), ("fx_offline_get_smoothing", [vp, fp, fp], st),
        ("fx_pack_osc12", [fp, fp], None), ("fx_pack_osc10", [fp, fp], None), ("fx_osc_encode", [cp, fp, P(ctypes.c_ubyte), i], st),
        ("fx_osc_message_bytes", [cp, i], st), ("fx_osc_encode_batch", [cp, i, i, fp, vp, i, ip], st),
        ("fx_get_osc_datagrams", [vp, cp, i, vp, i, ip, i], st),
        ("fx_set_osc_addresses", [vp, strings], st), ("fx_osc_address_stride", [vp], st), ("fx_get_osc_datagrams_addressed", [vp, vp, i, ip, i], st),
        ("fx_osc_encode_addressed", [strings, i, fp, vp, i, ip], st),
        ("fx_osc_bundle_plan", [i, i, i, ip, ip, ip], st), ("fx_osc_timetag", [d], st),
        ("fx_osc_encode_bundles", [cp, i, i, fp, ull, i, vp, i, ip], st), ("fx_osc_encode_bundles_addressed", [strings, i, fp, ull, i, vp, i, ip], st),
        ("fx_get_osc_bundles", [vp, cp, i, ull, i, vp, i, ip, i], st), ("fx_get_osc_bundles_addressed", [vp, ull, i, vp, i, ip, i], st),
        ("fx_osc_sender_create", [vpp, cp, cp, i, u], st), ("fx_osc_sender_destroy", [vp], st), ("fx_osc_sender_update", [vp, vp, i, ip, i], st),
        ("fx_osc_sender_send", [vp, llp], st), ("fx_osc_sender_start", [vp, d], st), ("fx_osc_sender_stop", [vp], st),
        ("fx_osc_sender_get_stats", [vp, P(OscSenderStats)], st), ("fx_osc_sender_set_routes", [vp, strings, i, ip, ip, i], st),
        ("fx_osc_receiver_create", [vpp, cp, i, cp, i, u], st), ("fx_osc_receiver_destroy", [vp], st), ("fx_osc_receiver_port", [vp], st),
        ("fx_osc_receiver_get_stats", [vp, llp, llp, llp], st), ("fx_osc_receiver_get_bundle_stats", [vp, llp, llp, P(ull)], st),
        ("fx_osc_receiver_last", [vp, i, vp, i, ip], st),
        ("fx_last_error", [], cp), ("fx_abi_version", [], st),
    ], [("fx_set_tuning_internal", [vp, u], st), ("fx_last_launches_internal", [vp, vp, i], st)]


# (name, argument types, restype) of every symbol include/fx.h declares, in its order -- and, apart, of the two test entries of
# csrc/fx_kernels.h; load_library() gives each function of the library its prototype from here
PROTOTYPES, INTERNAL_PROTOTYPES = _prototypes()
EXPORTS = [name for name, _, _ in PROTOTYPES]


class FxError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("fx error %d: %s" % (code, message))
        self.code = code


_lib = None


def library_path():
    """The shipped library -- or, for experiments only, the file FX_LIBRARY_OVERRIDE names (a variant built by tools/build_variants.py:
    selected by path, never copied over the shipped one)."""
    return os.environ.get("FX_LIBRARY_OVERRIDE") or _build.LIB_PATH


def load_library(build_if_missing=True):
    """Load libfx_hip.so; raises if it is missing and cannot be built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    override = os.environ.get("FX_LIBRARY_OVERRIDE")
    if build_if_missing and not override:
        _build.build()
    if not os.path.exists(library_path()):
        raise FxError(FX_ERR_UNSUPPORTED, "libfx_hip.so has not been built (run feature-extractor_amd/build.py)" if not override else "FX_LIBRARY_OVERRIDE names no file: %s" % override)
    # One HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64 / librccl (same SONAMEs as
    # /opt/rocm's): if libfx_hip.so is loaded first it binds /opt/rocm's copies, a later `import torch` then brings a
    # second runtime into the process and that one finds no GPU ("No HIP GPUs are available").  Loading torch's first
    # makes both sides share one runtime, whichever order the caller imports things in.  (C++ hosts link /opt/rocm.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(library_path())
    for name, argtypes, restype in PROTOTYPES + INTERNAL_PROTOTYPES:
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L


def check(status):
    if status != FX_OK:
        raise FxError(status, load_library().fx_last_error().decode(errors="replace"))


def plan_units(window_size, flags, waves_per_channel, num_frames, tuning=None):
    """fx_plan_units: the work-unit lengths a call of `num_frames` frames per channel is cut into (host arithmetic)."""
    buf = (ctypes.c_int * MAX_UNITS)()
    n = load_library().fx_plan_units(int(window_size), int(flags), int(waves_per_channel), int(num_frames),
                                     ctypes.byref(tuning) if tuning is not None else None, buf, MAX_UNITS)
    return list(buf[:n])


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


RESAMPLER_ZERO_CROSSINGS, RESAMPLER_PHASES = 16, 512


def resampler_table():
    """fx_get_resampler_table: (the table float32 [Z * P + 2], Z, P) of the resampler rated clips play through (host arithmetic)"""
    out = np.empty(RESAMPLER_ZERO_CROSSINGS * RESAMPLER_PHASES + 2, np.float32)
    z, p = ctypes.c_int(0), ctypes.c_int(0)
    check(load_library().fx_get_resampler_table(_fp(out), out.size, ctypes.byref(z), ctypes.byref(p)))
    return out, z.value, p.value


def pack_osc12(features12):
    v = np.ascontiguousarray(features12, np.float32)
    out = np.empty(12, np.float32)
    load_library().fx_pack_osc12(_fp(v), _fp(out))
    return out


def pack_osc10(features12):
    v = np.ascontiguousarray(features12, np.float32)
    out = np.empty(10, np.float32)
    load_library().fx_pack_osc10(_fp(v), _fp(out))
    return out


def osc_encode(address, features12):
    v = np.ascontiguousarray(features12, np.float32)
    buf = (ctypes.c_ubyte * 512)()
    n = load_library().fx_osc_encode(address.encode(), _fp(v), buf, 512)
    if n < 0:
        raise FxError(FX_ERR_INVALID_ARGUMENT, "OSC address too long")
    return bytes(buf[:n])


OSC_SENDER_GSO = 1
OSC_RECEIVER_NO_GRO = 1
OSC_RECEIVER_BUNDLES = 2


def osc_message_bytes(prefix, channel):
    return load_library().fx_osc_message_bytes(prefix.encode(), int(channel))


def osc_stride(prefix, first_channel, num_channels):
    """the smallest legal stride for these channels' messages: the longest message (already a multiple of 4)"""
    n = osc_message_bytes(prefix, first_channel + max(num_channels, 1) - 1)
    if n < 0:
        raise FxError(FX_ERR_INVALID_ARGUMENT, "OSC prefix too long or a negative channel number")
    return n


def osc_encode_batch(prefix, first_channel, smoothed, stride=None):
    """fx_osc_encode_batch: (datagrams uint8 [C][stride], lengths int32 [C]) for smoothed [C][12]; message c = datagrams[c, :lengths[c]]"""
    v = np.ascontiguousarray(smoothed, np.float32).reshape(-1, 12)
    stride = osc_stride(prefix, first_channel, v.shape[0]) if stride is None else int(stride)
    out = np.empty((v.shape[0], stride), np.uint8)
    lengths = np.empty(v.shape[0], np.int32)
    n = load_library().fx_osc_encode_batch(prefix.encode(), int(first_channel), v.shape[0], _fp(v), out.ctypes.data_as(ctypes.c_void_p), stride,
                                           lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if n != v.shape[0]:
        raise FxError(FX_ERR_INVALID_ARGUMENT, "fx_osc_encode_batch refused its arguments (prefix, channel range or stride)")
    return out, lengths


def c_strings(strings):
    """a list of str / bytes as the `const char* const*` the address and target entries take (keep the result alive over the call)"""
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in strings]
    return (ctypes.c_char_p * len(raw))(*raw)


def osc_address_bytes(address):
    """bytes of the message of this address: address + NUL padded to 4, 16 bytes of type tags, 48 of floats"""
    return ((len(address.encode() if isinstance(address, str) else address) + 4) & ~3) + 64


def osc_encode_addressed(addresses, smoothed, stride=None):
    """fx_osc_encode_addressed: (datagrams uint8 [n][stride], lengths int32 [n]) for smoothed [n][12] and one address per track;
    stride None = the smallest legal one, the longest message."""
    v = np.ascontiguousarray(smoothed, np.float32).reshape(-1, 12)
    addresses = list(addresses)
    if len(addresses) != v.shape[0]:
        raise ValueError("one address per track (%d), not %d" % (v.shape[0], len(addresses)))
    stride = max([osc_address_bytes(a) for a in addresses] + [4]) if stride is None else int(stride)
    out = np.empty((v.shape[0], max(stride, 0)), np.uint8)
    lengths = np.empty(v.shape[0], np.int32)
    n = load_library().fx_osc_encode_addressed(c_strings(addresses), v.shape[0], _fp(v), out.ctypes.data_as(ctypes.c_void_p), stride,
                                               lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if n != v.shape[0]:
        raise FxError(FX_ERR_INVALID_ARGUMENT, load_library().fx_last_error().decode(errors="replace"))
    return out, lengths


def osc_bundle_plan(longest_message_bytes, num_tracks, max_datagram_bytes=1472):
    """fx_osc_bundle_plan: (tracks per bundle K, number of bundles, stride) of a call's bundles"""
    k, b, stride = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    check(load_library().fx_osc_bundle_plan(int(longest_message_bytes), int(num_tracks), int(max_datagram_bytes), ctypes.byref(k), ctypes.byref(b), ctypes.byref(stride)))
    return k.value, b.value, stride.value


_timetag_fn = None


def osc_timetag(unix_seconds):
    """fx_osc_timetag: the OSC 1.0 time tag (NTP seconds since 1900 << 32 | fraction) of a Unix time.  The one entry of fx.h that
    returns 64 bits: the prototype table's restype column is int for every status-returning entry (tests/test_binding_inputs_cpu.py
    holds it to that), so this call goes through a foreign-function object of its own with the true return type."""
    global _timetag_fn
    if _timetag_fn is None:
        _timetag_fn = ctypes.CFUNCTYPE(ctypes.c_ulonglong, ctypes.c_double)(("fx_osc_timetag", load_library()))
    return int(_timetag_fn(float(unix_seconds)))


def _bundle_buffers(longest, num_tracks, max_datagram_bytes, stride):
    _, bundles, need = osc_bundle_plan(longest, num_tracks, max_datagram_bytes)
    stride = need if stride is None else int(stride)
    return np.empty((bundles, max(stride, 0)), np.uint8), np.empty(bundles, np.int32), stride


def osc_encode_bundles(prefix, first_channel, smoothed, timetag=OSC_TIMETAG_IMMEDIATE, max_datagram_bytes=1472, stride=None):
    """fx_osc_encode_bundles: (bundles uint8 [B][stride], lengths int32 [B]) for smoothed [n][12]; datagram b = bundles[b, :lengths[b]]"""
    v = np.ascontiguousarray(smoothed, np.float32).reshape(-1, 12)
    out, lengths, stride = _bundle_buffers(osc_stride(prefix, first_channel, v.shape[0]), v.shape[0], max_datagram_bytes, stride)
    n = load_library().fx_osc_encode_bundles(prefix.encode(), int(first_channel), v.shape[0], _fp(v), int(timetag), int(max_datagram_bytes),
                                             out.ctypes.data_as(ctypes.c_void_p), stride, lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if n != out.shape[0]:
        raise FxError(FX_ERR_INVALID_ARGUMENT, load_library().fx_last_error().decode(errors="replace"))
    return out, lengths


def osc_encode_bundles_addressed(addresses, smoothed, timetag=OSC_TIMETAG_IMMEDIATE, max_datagram_bytes=1472, stride=None):
    """fx_osc_encode_bundles_addressed: the same with one address per track"""
    v = np.ascontiguousarray(smoothed, np.float32).reshape(-1, 12)
    addresses = list(addresses)
    if len(addresses) != v.shape[0]:
        raise ValueError("one address per track (%d), not %d" % (v.shape[0], len(addresses)))
    out, lengths, stride = _bundle_buffers(max(osc_address_bytes(a) for a in addresses), v.shape[0], max_datagram_bytes, stride)
    n = load_library().fx_osc_encode_bundles_addressed(c_strings(addresses), v.shape[0], _fp(v), int(timetag), int(max_datagram_bytes),
                                                       out.ctypes.data_as(ctypes.c_void_p), stride, lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    if n != out.shape[0]:
        raise FxError(FX_ERR_INVALID_ARGUMENT, load_library().fx_last_error().decode(errors="replace"))
    return out, lengths


class OscSender:
    """fx_osc_sender: sendmmsg batches from `threads` threads to a primary and an optional secondary target, paced by start(rate_hz)."""

    def __init__(self, primary="127.0.0.1:9000", secondary=None, threads=1, gso=False):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        check(self._lib.fx_osc_sender_create(ctypes.byref(self._h), primary.encode(), secondary.encode() if secondary else None, int(threads), OSC_SENDER_GSO if gso else 0))

    def update(self, datagrams, lengths):
        d = np.ascontiguousarray(datagrams, np.uint8)
        n = np.ascontiguousarray(lengths, np.int32)
        if d.ndim != 2 or n.shape != (d.shape[0],):
            raise ValueError("datagrams [count][stride] and lengths [count]")
        check(self._lib.fx_osc_sender_update(self._h, d.ctypes.data_as(ctypes.c_void_p), d.shape[1], n.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), d.shape[0]))

    def set_routes(self, targets, primary=None, secondary=None):
        """fx_osc_sender_set_routes: message i goes to targets[primary[i]] and, where secondary[i] >= 0, to targets[secondary[i]];
        targets None restores the create-time pair."""
        if targets is None:
            check(self._lib.fx_osc_sender_set_routes(self._h, None, 0, None, None, 0))
            return
        ip = ctypes.POINTER(ctypes.c_int)
        p = np.ascontiguousarray(primary, np.int32).ravel()
        q = None if secondary is None else np.ascontiguousarray(secondary, np.int32).ravel()
        if q is not None and q.shape != p.shape:
            raise ValueError("primary and secondary have one entry per message")
        check(self._lib.fx_osc_sender_set_routes(self._h, c_strings(targets), len(targets), p.ctypes.data_as(ip),
                                                 q.ctypes.data_as(ip) if q is not None else None, p.size))

    def send(self):
        sent = ctypes.c_longlong(0)
        check(self._lib.fx_osc_sender_send(self._h, ctypes.byref(sent)))
        return sent.value

    def start(self, rate_hz=60.0):
        check(self._lib.fx_osc_sender_start(self._h, float(rate_hz)))

    def stop(self):
        check(self._lib.fx_osc_sender_stop(self._h))

    def stats(self):
        st = OscSenderStats()
        check(self._lib.fx_osc_sender_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            self._lib.fx_osc_sender_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OscReceiver:
    """fx_osc_receiver: counts OSC feature messages arriving on a local UDP port (tests, benchmarks, soak runs)."""

    def __init__(self, bind="127.0.0.1:0", threads=1, prefix=None, keep_channels=0, gro=True, bundles=False):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        check(self._lib.fx_osc_receiver_create(ctypes.byref(self._h), bind.encode(), int(threads), prefix.encode() if prefix else None, int(keep_channels),
                                               (0 if gro else OSC_RECEIVER_NO_GRO) | (OSC_RECEIVER_BUNDLES if bundles else 0)))
        self.port = self._lib.fx_osc_receiver_port(self._h)

    def stats(self):
        a, b, c = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
        check(self._lib.fx_osc_receiver_get_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"datagrams": a.value, "bytes": b.value, "malformed": c.value}

    def bundle_stats(self):
        """fx_osc_receiver_get_bundle_stats (a receiver made with bundles=True)"""
        a, b, t = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_ulonglong(0)
        check(self._lib.fx_osc_receiver_get_bundle_stats(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(t)))
        return {"bundles": a.value, "elements": b.value, "last_timetag": t.value}

    def last(self, channel):
        buf = (ctypes.c_ubyte * 160)()
        n = ctypes.c_int(0)
        check(self._lib.fx_osc_receiver_last(self._h, int(channel), buf, 160, ctypes.byref(n)))
        return bytes(buf[:n.value])

    def close(self):
        if self._h:
            self._lib.fx_osc_receiver_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
