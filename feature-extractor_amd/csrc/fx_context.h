// fx_context.h -- the context behind the C ABI (include/fx.h), shared by the shim's host units (fx_capi.cpp, fx_plan.cpp, fx_stream.cpp,
// fx_comm.cpp) and the units that attach through its hooks (fx_taps.hip, fx_interleave.hip, fx_events.hip, fx_tracks.hip,
// fx_osc_table.hip, fx_osc_bundle.hip, fx_track_state.hip, fx_display.hip, fx_clips.hip, fx_monitor.hip, fx_rtp.hip).  Internal.
//
// What a new attached unit uses instead of copying its neighbour: a list of tracks is judged by fx_check_channel_list and
// fx_check_channel_entries (the call's own values between the two), a memory kind by fx_check_memory_kind (or fx_check_call, with a
// sample format); a list that travels through pinned memory to the device lives in a fx_staged_list (fx_reserve_list /
// fx_release_list), other scratch on fx_grow; a unit that allocates before any analysis call asks fx_require_device first; a HIP
// error becomes a status by HIP_TRY or fx_hip_status; the release hook frees its device buffers with fx_free_device.  All of it is
// defined in fx_capi.cpp, so the fake-HIP host builds (build.py, HOST_SOURCES) bring it along.
#ifndef FX_CONTEXT_H
#define FX_CONTEXT_H

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "fx_kernels.h"

fx_status fx_fail(fx_status code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

inline fx_status fx_hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? FX_ERR_OUT_OF_MEMORY : FX_ERR_HIP; }
#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fx_fail(fx_hip_status(e_), "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

inline bool known_format(int f) { return f == FX_SAMPLE_F32 || f == FX_SAMPLE_F16 || f == FX_SAMPLE_S16 || f == FX_SAMPLE_S24; }
inline size_t sample_size(int f) { return (size_t) fxk::sample_bytes(f); }
// A call's sample format and the memory kinds of its input and results (an entry point passes what it has): FX_ERR_INVALID_ARGUMENT
// for an unknown one, the format's refusal first.  fx_check_memory_kind: one kind alone, "unknown memory kind %d".
fx_status fx_check_call(int sample_format, int in_kind = FX_MEM_HOST, int out_kind = FX_MEM_HOST);
fx_status fx_check_memory_kind(int kind);

// The contract of every entry that takes a list of tracks, in two steps because a setter judges the values it brings between them
// ("the call's own values, then the range of its entries"); no device use.  fx_check_channel_list: "null context", "negative channel
// count %d", "null channel list with %d entries".  fx_check_channel_entries (of a list that passed the first): the first entry outside
// [0, C), "entry %d: channel %d out of range [0,%d)".
fx_status fx_check_channel_list(const fx_context* ctx, const int* channels, int num_channels);
fx_status fx_check_channel_entries(const fx_context* ctx, const int* channels, int num_channels);

// FX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)", unless the runtime reports a device
fx_status fx_require_device();
// hipFree of every pointer that is not null, in order; failures are ignored (a release hook has nobody to tell)
void fx_free_device(std::initializer_list<void*> bufs);

// Scratch that follows the largest call seen (fx_capi.cpp): *ptr holds at least `need` bytes afterwards, or is null (capacity 0) with
// FX_ERR_OUT_OF_MEMORY / FX_ERR_HIP.  What the buffer held is not kept.
fx_status fx_grow(void** ptr, size_t* cap, size_t need);
template <typename T> fx_status fx_grow(T** ptr, size_t* cap, size_t need)
{
    void* p = *ptr;
    const fx_status st = fx_grow(&p, cap, need);
    *ptr = static_cast<T*>(p);
    return st;
}

// A list a call fills on the host and a kernel reads: pinned memory (what an upload in flight reads) and its device copy, `cap`
// entries each.  fx_reserve_list: room for `entries` of entry_bytes (the same size at every call); no HIP call when they fit.  It
// grows by at least half again, as fx_grow: a host whose lists get longer does not pay a free (it waits for the device) and a pinned
// allocation per call.  Growing waits for the context's stream first (a copy in flight may read the old pair), allocates the new
// pair before the old one goes -- a failed allocation ("allocating the track list failed: %s") leaves the old lists in place -- and
// attempts both frees before it reports the first that failed: the new lists are in place either way.  What the lists held is not kept.
// fx_release_list: frees both (nothing to do for an empty list) and leaves the list empty.
struct fx_staged_list {
    void*  pinned = nullptr;
    void*  device = nullptr;
    size_t cap = 0;
};
fx_status fx_reserve_list(fx_context* ctx, fx_staged_list* list, size_t entries, size_t entry_bytes);
void fx_release_list(fx_staged_list* list);

struct fx_comm;     // fx_comm.cpp
void fx_comm_release(fx_context* ctx);   // called by fx_destroy
fx_status fx_check_device_error(fx_context* ctx);   // after a synchronisation: FX_ERR_HIP if a kernel reported a failed hand-over
// appends an entry of `kind` to the context's launch record (fx_last_launches_internal) and returns it for the launcher's own fields;
// null beyond FX_LAUNCH_RECORD_CAP.  The only writer of fx_context::launches.
fx_launch_record* note_launch(fx_context* ctx, int kind, int analysers);

// fx_push_samples after its launch record is started: a block of num_samples samples per channel, [C][num_samples], from in_kind memory
// (a device block 4-byte aligned), results to out_kind memory.  Re-blocking, the block feed, taps and the carry all happen here, so that
// fx_push_interleaved (fx_interleave.hip) hands over the planar block it assembled and shares every step after it.
fx_status fx_push_block(fx_context* ctx, const void* samples, int num_samples, int sample_format, int in_kind, int out_kind,
                        float* out_raw, float* out_smoothed, int* frames_out, bool taps);
// fx_push_block's refusals that depend on the pending samples alone (a format change while samples are pending, a block of more than
// 2^24 hops): FX_ERR_INVALID_ARGUMENT or FX_OK, no device use.  fx_push_interleaved makes them before it launches anything.
fx_status fx_block_refusal(const fx_context* ctx, int num_samples, int sample_format);

// Analysis taps (fx_request_taps / fx_get_taps, include/fx.h) live in fx_taps.hip; this file only carries their state and the two hooks
// fx_request_taps installs, so that the rest of the library refers to no symbol of that unit.
struct fx_taps;
struct fx_interleave;   // fx_interleave.hip
struct fx_events;       // fx_events.hip
struct fx_tracks;       // fx_tracks.hip
struct fx_track_state;  // fx_track_state.hip
struct fx_display;      // fx_display.hip
struct fx_clips;        // fx_clips.hip
struct fx_monitor;      // fx_monitor.hip
struct fx_rtp;          // fx_rtp.hip
// The OSC address table in force (fx_osc_table.hip makes and frees it; fx_osc_bundle.hip reads it): one device allocation, [C][128]
// bytes of rows, then int len[C]; the messages' lengths on the host.
struct fx_osc_table {
    unsigned char*   d_table = nullptr;
    std::vector<int> message_bytes;     // [C]
    int              longest = 0;       // the smallest legal stride
};
// Where an analysis call reads its frames (the taps take the FIRST, the audio display every hop), as the kernels read them: `in` (device) holds rows of in_row_bytes per channel; hop_mode 1:
// hops of N/2 samples, the window is [the channel's tail | hop 0 x gain]; 0: whole frames, frame 0 as given.  carry != null: the hop is
// the first N/2 samples of [pending | block] (fx_blocks.hip.h, BlockStream), the pending row of the channel at carry + c * carry_row_bytes.
struct fx_tap_source {
    const void*          in;
    int                  sample_format;
    int                  hop_mode;
    long long            in_row_bytes;
    const unsigned char* carry;
    int                  carry_bytes, carry_row_bytes;
};

struct fx_context {
    int      device = 0;
    int      C = 0, N = 0;
    double   sample_rate = 48000.0;
    unsigned flags = 0;
    // settings (ref RealTimeAnalyser.h:244-258, SpectralCharacteristics.h:237-241,311, AudioDataCollector.h:129)
    float    gain = 1.0f;
    int      onset_window = 5;
    int      onset_type = FX_ONSET_AMPLITUDE;
    float    onset_multiplier = 1.7f;
    float    onset_sensitivity = 0.7f;      // what fx_get_channel_settings reports (onset_multiplier is the float sum 1 + sensitivity)
    long long frames_seen = 0;
    long long onset_reset_frame = 0;
    // Per-track settings (fx_set_channel_gains / fx_set_channel_onset): empty / null until the first per-track call, and until then the
    // kernels read the four values above.  `chan` is what every track runs with, d_chan its device copy (FrameParams::chan: allocated
    // once, never moved), h_chan_stage the pinned rows an upload in flight reads.  Once they exist the context-wide setters write every
    // row too, so the values above and the table never disagree about a track nobody set on its own.
    std::vector<fxk::ChannelSettings> chan;
    std::vector<float>                chan_sensitivity;
    fxk::ChannelSettings* d_chan = nullptr;
    fxk::ChannelSettings* h_chan_stage = nullptr;

    hipStream_t stream = nullptr;
    hipEvent_t  ev[3] = {nullptr, nullptr, nullptr};
    bool        ev_valid = false;
    bool        profiling = false;
    std::vector<hipEvent_t> prof_events;     // 3 per recorded call
    size_t      prof_used = 0;

    float* d_tw = nullptr;        // [N][2]
    float* d_prev = nullptr;      // [C][N/2]
    float* d_tail[2] = {nullptr, nullptr};   // [C][N/2], ping-pong
    float* d_hist = nullptr;      // [C][HLEN][12]: per channel a ring of the newest HLEN frames' raw values (row = frame index mod HLEN)
    float* d_latest = nullptr;    // [C][12]
    int    cur = 0;
    unsigned test_hooks = 0;      // fx_set_tuning_internal (fx_kernels.h): tests only
    fx_launch_record launches[FX_LAUNCH_RECORD_CAP];    // fx_last_launches_internal (fx_kernels.h): what the last call launched
    int      num_launches = 0;                          // (may exceed the cap: those beyond it are counted, not kept)
    fx_tuning tuning;             // launch-shape knobs: taken from the environment ONCE, in fx_create (fx_set_tuning replaces them)
    unsigned* h_err = nullptr;    // pinned, coherent: a kernel stores 1 here when a work unit gave up waiting for its predecessor (sticky)
    unsigned* d_err = nullptr;    // device view of h_err
    unsigned* d_queue = nullptr;  // [1 + C]: ticket counter and per-channel chunk counts of a frame-kernel launch cut in time (FrameParams::queue)

    // fx_push_samples: what a channel's device blocks have left over, < N/2 samples in `carry_format` (AudioDataCollector's ring holds
    // them un-gained, AudioDataCollector.h:42-64,88); two buffers, the re-blocking kernel reads one and writes the other
    unsigned char* d_carry[2] = {nullptr, nullptr};   // [C][N/2 * 4 bytes]
    int    carry_cur = 0;
    int    carry_count = 0;       // samples per channel pending (the same for every channel: blocks arrive for all channels at once)
    int    carry_format = FX_SAMPLE_F32;
    unsigned char* d_hops = nullptr;    // [C][hops][N/2] samples assembled for one fx_push_samples call
    size_t hops_cap = 0;

    float* d_raw = nullptr;       // [C][T_cap][12]
    fxk::FramePart* d_part = nullptr;   // [C][T_cap]
    size_t part_cap = 0;
    void*  d_in = nullptr;        // staging for host input
    float* d_out_raw = nullptr;   // staging for host output
    float* d_out_sm = nullptr;
    size_t raw_cap = 0, in_cap = 0, out_cap = 0;
    float* d_flux_park = nullptr; // FrameParams::flux_park: [C][wavefronts per channel][N/2], 1024-point batch calls with both analysers (flux_park_need)
    size_t flux_park_cap = 0;

    unsigned char* d_osc = nullptr;   // [C][stride]: fx_get_osc_datagrams' messages before they go to a host buffer
    size_t osc_cap = 0;

    double bin_var = 0.0;
    float  lpf_a = 0.0f, lpf_b = 0.0f;
    float  first_tw[18] = {0};
    bool   tw_quarter_turn = false;     // FrameParams::tw_quarter_turn
    float  tw_at_quarter[2] = {0.0f, -1.0f};
    int    compute_units = 256;         // of this context's device (MI355X: 256)

    fx_comm* comm = nullptr;      // fx_comm_create (fx_comm.cpp); null for a single-GPU context

    // taps (fx_taps.hip): null until the first fx_request_taps, which installs the hooks.  taps_armed: channels waiting for a capture.
    fx_taps* taps = nullptr;
    int      taps_armed = 0;
    fx_status (*taps_launch)(fx_context*, const fx_tap_source&) = nullptr;   // capture the call's first frame; clears the request
    void      (*taps_release)(fx_context*) = nullptr;                         // drop request, capture and memory (reset, destroy)

    // interleaved input (fx_interleave.hip): the channel map, its device copy and the staging buffers; null until the first
    // fx_set_channel_map / fx_push_interleaved, which installs the hook.  The map is a setting: fx_destroy calls the hook, fx_reset_state does not.
    fx_interleave* interleave = nullptr;
    void (*interleave_release)(fx_context*) = nullptr;

    // the onset event list (fx_events.hip): null until fx_enable_onset_events, which installs the hooks (and removes them again when
    // it disables the list).  events_launch: after the last analysis launch of a call of T frames per channel whose raw vectors are
    // in d_raw [C][T][12], frame0 the stream index of the call's first frame.  events_reset: fx_reset_state, the list emptied and kept.
    fx_events* events = nullptr;
    fx_status (*events_launch)(fx_context*, const float* d_raw, int T, long long frame0) = nullptr;
    fx_status (*events_reset)(fx_context*) = nullptr;
    void      (*events_release)(fx_context*) = nullptr;

    // per-track reset and clear (fx_tracks.hip): the channel list's staging and device copy; null until the first fx_reset_channels /
    // fx_clear_pending_channels, which installs the hook fx_destroy calls.  The tracks' first frames live in `chan` (first_frame).
    fx_tracks* tracks = nullptr;
    void (*tracks_release)(fx_context*) = nullptr;

    // per-track OSC addresses (fx_osc_table.hip): the address table on the device and the messages' lengths; null while no table is
    // set.  fx_set_osc_addresses installs the hook fx_destroy calls.  A setting: no reset touches it.
    fx_osc_table* osc_table = nullptr;
    void (*osc_table_release)(fx_context*) = nullptr;

    // moving tracks between contexts (fx_track_state.hip): the entry list's staging, its device copy and the records' scratch; null
    // until the first fx_export_channels / fx_import_channels, which installs the hook fx_destroy calls.
    fx_track_state* track_state = nullptr;
    void (*track_state_release)(fx_context*) = nullptr;

    // audio display levels (fx_display.hip): null until fx_enable_display, which installs the hooks (and removes them again when it
    // disables the display).  display_launch: once the analysis launches of a call of T frames per channel are enqueued, `src` where
    // they read its samples.  display_reset: the listed tracks (null: all C) become new components (fx_reset_state, fx_reset_channels),
    // or are cleared with their ring position kept (keep_next).
    fx_display* display = nullptr;
    fx_status (*display_launch)(fx_context*, const fx_tap_source& src, int T) = nullptr;
    fx_status (*display_reset)(fx_context*, const int* channels, int n, bool keep_next) = nullptr;
    void      (*display_release)(fx_context*) = nullptr;

    // file sources (fx_clips.hip): the clip banks, the per-track transport tables and the staging of fx_push_sources; null until the
    // first call of that unit, which installs the hook fx_destroy calls.  The player's state, not the analysers': no reset touches it.
    fx_clips* clips = nullptr;
    void (*clips_release)(fx_context*) = nullptr;

    // the monitor mix (fx_monitor.hip): the send table, the partial sums and the last tick's mix; null until fx_enable_monitor, which
    // installs the hooks (and removes them again when it disables the monitor).  fx_push_sources calls monitor_prepare before it
    // launches anything (room for a tick of num_samples: a failure changes nothing) and monitor_launch once the tick's planar block
    // is complete on the stream: `planar` [C][num_samples] starts a device buffer on a 16-byte boundary that holds 32 bytes
    // more than the block (the kernel's 16-byte loads end past a row's end).  The slot's state, not the analysers': no reset touches it.
    // monitor_prepare also refuses a tick that is not fp32 while a track listens to an output, and monitor_launch WRITES `planar`:
    // the rows of the tracks that listen (fx_set_channel_listen) become the mix before the analysers read them.
    fx_monitor* monitor = nullptr;
    fx_status (*monitor_prepare)(fx_context*, int num_samples, int sample_format) = nullptr;
    fx_status (*monitor_launch)(fx_context*, void* planar, int num_samples, int sample_format) = nullptr;
    void      (*monitor_release)(fx_context*) = nullptr;

    // RTP input (fx_rtp.hip): the stream and track tables, the statistics and the scratch of fx_push_rtp; null until fx_rtp_configure,
    // which installs the hook fx_destroy calls (and frees the unit again when it is given no streams).  The slot's state, not the
    // analysers': no reset touches it.
    fx_rtp* rtp = nullptr;
    void (*rtp_release)(fx_context*) = nullptr;
};

// The per-track rows (fx_capi.cpp), for the units that change them.  fx_channel_rows: what every track runs with now -- the table's rows,
// or the context-wide values (first_frame 0) while no table exists.  fx_upload_channel_rows: puts `rows` in force for the calls that
// follow, in stream order; synchronises the stream; the first upload allocates the table; a failure leaves the old rows in force, on
// the device and in fx_context::chan (and no table where there was none).
void fx_channel_rows(const fx_context* ctx, std::vector<fxk::ChannelSettings>* rows, std::vector<float>* sensitivity);
fx_status fx_upload_channel_rows(fx_context* ctx, const std::vector<fxk::ChannelSettings>& rows, const std::vector<float>& sensitivity);

#endif
