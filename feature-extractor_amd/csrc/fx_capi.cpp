// fx_capi.cpp -- extern "C" shim declared in include/fx.h.  Host-side plumbing only: device
// buffers, per-channel state residency in HBM, stream ordering, launch of the gfx950 kernels.
// There is no CPU path: without a usable gfx950 device every entry point fails.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "fx_plan.h"
#include "fx_osc_words.h"

thread_local std::string g_fx_err;

fx_status fx_fail(fx_status code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_fx_err = buf;
    return code;
}

fx_status fx_check_call(int sample_format, int in_kind, int out_kind)
{
    if (!known_format(sample_format)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown sample format %d", sample_format);
    const fx_status st = fx_check_memory_kind(in_kind);
    return st != FX_OK ? st : fx_check_memory_kind(out_kind);
}

fx_status fx_check_memory_kind(int kind)
{
    if (kind != FX_MEM_HOST && kind != FX_MEM_DEVICE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown memory kind %d", kind);
    return FX_OK;
}

// ---- what the attached units share (fx_context.h states each contract) ----
fx_status fx_check_channel_list(const fx_context* c, const int* channels, int num_channels)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (num_channels < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative channel count %d", num_channels);
    if (num_channels > 0 && !channels) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null channel list with %d entries", num_channels);
    return FX_OK;
}

fx_status fx_check_channel_entries(const fx_context* c, const int* channels, int num_channels)
{
    for (int i = 0; i < num_channels; i++)
        if (channels[i] < 0 || channels[i] >= c->C)
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: channel %d out of range [0,%d)", i, channels[i], c->C);
    return FX_OK;
}

fx_status fx_require_device()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { (void) hipGetLastError(); return fx_fail(FX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)"); }
    return FX_OK;
}

void fx_free_device(std::initializer_list<void*> bufs)
{
    for (void* b : bufs) if (b) (void) hipFree(b);
}

fx_status fx_reserve_list(fx_context* c, fx_staged_list* list, size_t entries, size_t entry_bytes)
{
    if (entries <= list->cap) return FX_OK;
    size_t want = entries;
    if (want < list->cap + list->cap / 2) want = list->cap + list->cap / 2;
    HIP_TRY(hipStreamSynchronize(c->stream));
    void* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, want * entry_bytes, hipHostMallocDefault));
    void* d = nullptr;
    {
        const hipError_t e = hipMalloc(&d, want * entry_bytes);
        if (e != hipSuccess) {
            (void) hipHostFree(h);
            return fx_fail(fx_hip_status(e), "allocating the track list failed: %s", hipGetErrorString(e));
        }
    }
    void* old_d = list->device; void* old_h = list->pinned;
    list->device = d; list->pinned = h; list->cap = want;
    const hipError_t freed_d = old_d ? hipFree(old_d) : hipSuccess;
    const hipError_t freed_h = old_h ? hipHostFree(old_h) : hipSuccess;
    HIP_TRY(freed_d);
    HIP_TRY(freed_h);
    return FX_OK;
}

void fx_release_list(fx_staged_list* list)
{
    if (list->device) (void) hipFree(list->device);
    if (list->pinned) (void) hipHostFree(list->pinned);
    *list = fx_staged_list();
}

// Scratch that follows the largest call seen.  Growing frees and reallocates (hipFree waits for the device), so a
// buffer that has grown once grows by at least half again: a caller ramping its batch size up does not pay per call.
fx_status fx_grow(void** ptr, size_t* cap, size_t need)
{
    if (need <= *cap) return FX_OK;
    size_t want = need;
    if (*ptr) {
        if (want < *cap + *cap / 2) want = *cap + *cap / 2;
        // the pointer is forgotten BEFORE the free is attempted: a free that reports a failure must not be repeated by the next call
        // (found by tests/cpp/host_sanitize.cpp: the old order freed the block twice)
        void* old = *ptr;
        *ptr = nullptr;
        *cap = 0;
        HIP_TRY(hipFree(old));
    }
    *ptr = nullptr;
    *cap = 0;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess && want != need) { (void) hipGetLastError(); want = need; e = hipMalloc(&p, want); }
    if (e != hipSuccess) return fx_fail(fx_hip_status(e), "hipMalloc of %zu bytes failed: %s", want, hipGetErrorString(e));
    *ptr = p;
    *cap = want;
    return FX_OK;
}

static bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// ---- per-track settings (fx_set_channel_gains / fx_set_channel_onset; fx_context::chan) ----
// what every track runs with now: the table's rows, or the context-wide values while no table exists (fx_context.h)
void fx_channel_rows(const fx_context* c, std::vector<fxk::ChannelSettings>* rows, std::vector<float>* sensitivity)
{
    if (!c->chan.empty()) { *rows = c->chan; *sensitivity = c->chan_sensitivity; return; }
    rows->assign((size_t) c->C, fxk::ChannelSettings{c->gain, c->onset_multiplier, c->onset_window, c->onset_type, c->onset_reset_frame, 0});
    sensitivity->assign((size_t) c->C, c->onset_sensitivity);
}

// Puts `rows` in force for the calls that follow, in stream order: a copy on the context's stream from pinned rows that stay until the
// next upload has waited for it.  The first upload allocates the table.  A failure leaves the old settings in force (and no table
// where there was none).
fx_status fx_upload_channel_rows(fx_context* c, const std::vector<fxk::ChannelSettings>& rows, const std::vector<float>& sensitivity)
{
    const size_t bytes = rows.size() * sizeof(fxk::ChannelSettings);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));               // (the upload before this one has read the staging rows)
    if (!c->h_chan_stage) {
        void* q = nullptr;
        HIP_TRY(hipHostMalloc(&q, bytes, hipHostMallocDefault));
        c->h_chan_stage = static_cast<fxk::ChannelSettings*>(q);
    }
    fxk::ChannelSettings* table = c->d_chan;
    if (!table) {
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, bytes));
        table = static_cast<fxk::ChannelSettings*>(q);
    }
    memcpy(c->h_chan_stage, rows.data(), bytes);
    const hipError_t e = hipMemcpyAsync(table, c->h_chan_stage, bytes, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        if (!c->d_chan) (void) hipFree(table);
        return fx_fail(FX_ERR_HIP, "uploading the per-track settings failed: %s", hipGetErrorString(e));
    }
    c->d_chan = table;
    c->chan = rows;
    c->chan_sensitivity = sensitivity;
    return FX_OK;
}

namespace {

// A context-wide setter on a context that has a table: `set` changes one row, every row gets it.  No table: nothing to do.
template <typename F> fx_status set_every_channel(fx_context* c, F set)
{
    if (c->chan.empty()) return FX_OK;
    std::vector<fxk::ChannelSettings> rows = c->chan;
    std::vector<float> sensitivity = c->chan_sensitivity;
    for (size_t i = 0; i < rows.size(); i++) set(rows[i], sensitivity[i]);
    return fx_upload_channel_rows(c, rows, sensitivity);
}

fx_status zero_state(fx_context* c)
{
    // (first: the one step that can leave the per-track rows as they were.  Every track's stream and onset histories start at frame 0 again.)
    { const fx_status st = set_every_channel(c, [](fxk::ChannelSettings& r, float&) { r.onset_reset_frame = 0; r.first_frame = 0; }); if (st != FX_OK) return st; }
    const size_t half = (size_t) c->C * (c->N / 2);
    HIP_TRY(hipMemsetAsync(c->d_prev, 0, half * sizeof(float), c->stream));
    for (int i = 0; i < 2; i++) HIP_TRY(hipMemsetAsync(c->d_tail[i], 0, half * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_hist, 0, (size_t) c->C * fxk::HLEN * FX_NUM_FEATURES * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_latest, 0, (size_t) c->C * FX_NUM_FEATURES * sizeof(float), c->stream));
    // the work units' ticket counter and hand-over counts: zero between calls (a cut call's last kernel leaves them so; a call that
    // failed half way is followed by this reset)
    HIP_TRY(hipMemsetAsync(c->d_queue, 0, sizeof(unsigned) * (1 + (size_t) c->C), c->stream));
    c->frames_seen = 0;
    c->onset_reset_frame = 0;
    c->carry_count = 0;                     // (a freshly constructed AudioDataCollector: nothing written, nothing pending)
    return FX_OK;
}

} // namespace

// the reference's table for a window size: phase in double, entries rounded to float (JUCE 4.2 FFT::FFTConfig)
static std::vector<float> reference_twiddles(int window_size)
{
    std::vector<float> tw(2 * (size_t) window_size);
    for (int i = 0; i < window_size; i++) {
        const double phase = -2.0 * 3.14159265358979323846 * i / window_size;
        tw[2 * i] = (float) std::cos(phase);
        tw[2 * i + 1] = (float) std::sin(phase);
    }
    return tw;
}

extern "C" int fx_twiddle_symmetry(int window_size)
{
    if (!is_pow2(window_size) || window_size < 256 || window_size > 4096) return 0;
    const std::vector<float> tw = reference_twiddles(window_size);
    std::vector<float> ordered(tw.size());
    float first[18];
    fxk::build_pass_twiddles(window_size, tw.data(), ordered.data());
    fxk::fill_first_pass_twiddles(window_size, ordered.data(), first);
    return (fxk::first_pass_twiddles_hermitian(window_size, first) ? 1 : 0) | (fxk::twiddles_have_quarter_turn(window_size, tw.data()) ? 2 : 0);
}

extern "C" void fx_tuning_defaults(fx_tuning* t)
{
    if (!t) return;
    memset(t, 0, sizeof *t);
    t->frames_per_unit = -1;
    t->stream_graph = t->stream_hop_kernel = t->stream_zero_copy = t->one_hop_kernel = t->call_timing = t->stream_fill_streaming = -1;
}

// The ONLY place the library reads the environment: called once per context, by fx_create.
extern "C" void fx_tuning_from_env(fx_tuning* t)
{
    if (!t) return;
    fx_tuning_defaults(t);
    auto geti = [](const char* name, int* out, int lo) { if (const char* e = getenv(name)) { const int v = atoi(e); if (v >= lo) *out = v; } };
    geti("FX_WAVES", &t->waves_per_channel, 1);
    geti("FX_CHANNELS_PER_WG", &t->channels_per_workgroup, 1);
    geti("FX_WAVES_PER_FRAME", &t->waves_per_frame, 1);
    geti("FX_FRAMES_PER_CHUNK", &t->frames_per_unit, 0);
    if (const char* plan = getenv("FX_CHUNK_PLAN")) {
        int n = 0;
        for (const char* q = plan; *q && n < FX_MAX_UNITS; ) { const int v = atoi(q); if (v > 0) t->unit_plan[n++] = v; while (*q && *q != ',') q++; if (*q == ',') q++; }
        t->unit_plan_len = n;
    }
    geti("FX_STREAM_GRAPH", &t->stream_graph, 0);
    geti("FX_STREAM_HOP_KERNEL", &t->stream_hop_kernel, 0);
    geti("FX_STREAM_ZEROCOPY", &t->stream_zero_copy, 0);
    geti("FX_ONE_HOP_KERNEL", &t->one_hop_kernel, 0);
    geti("FX_CALL_TIMING", &t->call_timing, 0);
    geti("FX_HANDOVER_SPINS", &t->handover_spin_limit, 1);
    geti("FX_STREAM_FILL_STREAMING", &t->stream_fill_streaming, 0);
}

extern "C" fx_status fx_get_tuning(fx_context* c, fx_tuning* out)
{
    if (!c || !out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    *out = c->tuning;
    return FX_OK;
}

extern "C" fx_status fx_set_tuning(fx_context* c, const fx_tuning* t)
{
    if (!c || !t) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (t->waves_per_channel < 0 || t->channels_per_workgroup < 0 || t->waves_per_frame < 0 || t->waves_per_frame > 2 ||
        t->unit_plan_len < 0 || t->unit_plan_len > FX_MAX_UNITS || t->handover_spin_limit < 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "tuning value out of range");
    // the kernel family is fixed while a history exists: the two families' continuous slots may differ in the last bit, and a
    // channel's smoothing window must not hold values of both
    if (c->frames_seen > 0 && uses_pairs(c, t->waves_per_frame) != uses_pairs(c, c->tuning.waves_per_frame))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "waves_per_frame selects the kernel family and %lld frames have been analysed with the other one; "
                                                "fx_reset_state first", c->frames_seen);
    c->tuning = *t;              // (nothing below can fail: a refused call leaves the old knobs in place)
    return FX_OK;
}

// tests only (csrc/fx_kernels.h; not in include/fx.h)
extern "C" fx_status fx_set_tuning_internal(fx_context* c, unsigned test_hooks)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    c->test_hooks = test_hooks;
    return FX_OK;
}

// tests only (csrc/fx_kernels.h; not in include/fx.h)
extern "C" int fx_last_launches_internal(fx_context* c, fx_launch_record* out, int cap)
{
    if (!c) return 0;
    const int kept = c->num_launches < FX_LAUNCH_RECORD_CAP ? c->num_launches : FX_LAUNCH_RECORD_CAP;
    for (int i = 0; i < kept && i < cap && out; i++) out[i] = c->launches[i];
    return c->num_launches;
}

// A frame-kernel work unit that gave up waiting for its predecessor's flux state stores 1 to c->h_err (pinned host
// memory).  Sticky: every synchronising entry point reports it until fx_reset_state.
fx_status fx_check_device_error(fx_context* c)
{
    if (c && c->h_err && *(volatile unsigned*) c->h_err != 0)
        return fx_fail(FX_ERR_HIP, "a frame-kernel work unit timed out waiting for the flux state of the unit before it; "
                                   "the results of that call and of every call since are not valid (fx_reset_state clears this)");
    return FX_OK;
}

// The launch record (fx_last_launches_internal): a handful of host stores per launch; each entry point that launches starts it anew.
fx_launch_record* note_launch(fx_context* c, int kind, int analysers)
{
    const int i = c->num_launches++;
    if (i >= FX_LAUNCH_RECORD_CAP) return nullptr;
    fx_launch_record& r = c->launches[i];
    r = fx_launch_record{};
    r.kind = kind;
    r.window = c->N;
    r.analysers = analysers;
    return &r;
}

extern "C" {

int fx_abi_version(void) { return FX_ABI_VERSION; }
const char* fx_last_error(void) { return g_fx_err.c_str(); }

fx_status fx_create(fx_context** out, int device_id, int num_channels, int window_size, double sample_rate, unsigned flags)
{
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null output pointer");
    *out = nullptr;
    if (num_channels <= 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "num_channels must be positive");
    if (!is_pow2(window_size) || window_size < 256 || window_size > 4096)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "window_size must be a power of two in [256, 4096], got %d", window_size);
    if (!(sample_rate > 0.0)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
    if ((flags & FX_ORDER_MASK) == 3u || (flags & ~(FX_ORDER_MASK | FX_SPECTRAL_ONLY | FX_HARMONIC_ONLY | FX_LOW_LATENCY)) ||
        ((flags & FX_SPECTRAL_ONLY) && (flags & FX_HARMONIC_ONLY)))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown or contradictory flags 0x%x", flags);

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void) hipGetLastError();
        return fx_fail(FX_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    }
    if (device_id < 0 || device_id >= count) return fx_fail(FX_ERR_INVALID_ARGUMENT, "device_id %d out of range [0,%d)", device_id, count);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fx_fail(FX_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", device_id, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device_id));

    fx_context* c = new (std::nothrow) fx_context();
    if (!c) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    std::unique_ptr<fx_context, fx_status (*)(fx_context*)> half_built(c, fx_destroy);    // destroyed on every return but the last
    if (prop.multiProcessorCount > 0) c->compute_units = prop.multiProcessorCount;
    c->device = device_id;
    c->C = num_channels;
    c->N = window_size;
    c->sample_rate = sample_rate;
    c->flags = flags;
    fx_tuning_from_env(&c->tuning);          // once; nothing on the analysis path reads the environment

    fx_status st = FX_OK;
    {
        hipError_t e = fxk::prepare_kernels(window_size);
        if (e == hipSuccess) e = fxk::prepare_hop_kernel(window_size);
        if (e == hipSuccess) e = fxk::prepare_pair_kernel(window_size);
        if (e != hipSuccess) return fx_fail(FX_ERR_HIP, "kernel preparation failed: %s", hipGetErrorString(e));
    }
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (int i = 0; i < 3; i++) HIP_TRY(hipEventCreate(&c->ev[i]));
    const size_t half = (size_t) num_channels * (window_size / 2);
    HIP_TRY(hipMalloc((void**) &c->d_tw, sizeof(float) * 4 * window_size));      // the pass-ordered table, then the frame kernel's LDS image of it
    HIP_TRY(hipMalloc((void**) &c->d_prev, sizeof(float) * half));
    for (int i = 0; i < 2; i++) HIP_TRY(hipMalloc((void**) &c->d_tail[i], sizeof(float) * half));
    HIP_TRY(hipMalloc((void**) &c->d_hist, sizeof(float) * (size_t) num_channels * fxk::HLEN * FX_NUM_FEATURES));
    HIP_TRY(hipMalloc((void**) &c->d_latest, sizeof(float) * (size_t) num_channels * FX_NUM_FEATURES));
    HIP_TRY(hipMalloc((void**) &c->d_queue, sizeof(unsigned) * (1 + (size_t) num_channels)));
    for (int i = 0; i < 2; i++) HIP_TRY(hipMalloc((void**) &c->d_carry[i], half * 4));
    HIP_TRY(hipHostMalloc((void**) &c->h_err, 64, hipHostMallocCoherent));
    *c->h_err = 0;
    { void* q = nullptr; HIP_TRY(hipHostGetDevicePointer(&q, c->h_err, 0)); c->d_err = static_cast<unsigned*>(q); }

    // Twiddle table exactly as the reference's FFT builds it (JUCE 4.2 FFT::FFTConfig, SURVEY.md
    // App. A.1): phase in double, entries rounded to float.  The inverse table is its conjugate.
    {
        const std::vector<float> tw = reference_twiddles(window_size);
        std::vector<float> ordered(tw.size());
        fxk::build_pass_twiddles(window_size, tw.data(), ordered.data());    // same values, pass access order
        fxk::fill_first_pass_twiddles(window_size, ordered.data(), c->first_tw);
        if (!fxk::first_pass_twiddles_hermitian(window_size, c->first_tw))
            return fx_fail(FX_ERR_UNSUPPORTED, "this host's cos/sin produce a twiddle table without the mirror symmetry the kernels rely on");
        c->tw_quarter_turn = fxk::twiddles_have_quarter_turn(window_size, tw.data());
        c->tw_at_quarter[0] = tw[2 * (size_t) (window_size / 4)]; c->tw_at_quarter[1] = tw[2 * (size_t) (window_size / 4) + 1];     // (false only costs the 4096-point kernel two global reads per item)
        HIP_TRY(hipMemcpy(c->d_tw, ordered.data(), ordered.size() * sizeof(float), hipMemcpyHostToDevice));
        std::vector<float> image(ordered.size(), 0.0f);
        fxk::build_twiddle_image(window_size, ordered.data(), image.data());
        HIP_TRY(hipMemcpy(c->d_tw + ordered.size(), image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // ref SpectralCharacteristics.h:180-189: binVar does not depend on the signal
    {
        const int M = window_size / 2;
        double bv = 0.0;
        for (double i = 0.0; i < M; i++) {
            const double ni = i / (double) M;
            bv += (ni - 0.5) * (ni - 0.5);
        }
        c->bin_var = bv / (double) M;
    }
    // ref RealTimeAudioAnalysis.h:122,127: float_Pi / m and exp(-float_Pi / m), m = 2.0f, in fp32
    {
        const float float_pi = 3.14159265358979323846f;
        c->lpf_a = float_pi / 2.0f;
        c->lpf_b = std::exp(-float_pi / 2.0f);
    }
    if ((st = zero_state(c)) != FX_OK) return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out = half_built.release();
    return FX_OK;
}

fx_status fx_destroy(fx_context* c)
{
    if (!c) return FX_OK;
    (void) hipSetDevice(c->device);
    fx_comm_release(c);
    if (c->stream) (void) hipStreamSynchronize(c->stream);
    if (c->taps_release) c->taps_release(c);
    if (c->interleave_release) c->interleave_release(c);
    if (c->events_release) c->events_release(c);
    if (c->tracks_release) c->tracks_release(c);
    if (c->osc_table_release) c->osc_table_release(c);
    if (c->track_state_release) c->track_state_release(c);
    if (c->display_release) c->display_release(c);
    if (c->clips_release) c->clips_release(c);
    if (c->monitor_release) c->monitor_release(c);
    if (c->rtp_release) c->rtp_release(c);
    fx_free_device({c->d_tw, c->d_prev, c->d_tail[0], c->d_tail[1], c->d_hist, c->d_latest,
                    c->d_raw, c->d_part, c->d_in, c->d_out_raw, c->d_queue, c->d_carry[0], c->d_carry[1], c->d_hops, c->d_osc, c->d_chan, c->d_flux_park});
    if (c->h_err) (void) hipHostFree(c->h_err);
    if (c->h_chan_stage) (void) hipHostFree(c->h_chan_stage);
    for (int i = 0; i < 3; i++) if (c->ev[i]) (void) hipEventDestroy(c->ev[i]);
    for (hipEvent_t e : c->prof_events) (void) hipEventDestroy(e);
    if (c->stream) (void) hipStreamDestroy(c->stream);
    delete c;
    return FX_OK;
}

fx_status fx_reset_state(fx_context* c)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->h_err) *c->h_err = 0;
    if (c->taps_release) c->taps_release(c);
    if (c->events_reset) { const fx_status st = c->events_reset(c); if (st != FX_OK) return st; }     // the list emptied, still enabled
    if (c->display_reset) { const fx_status st = c->display_reset(c, nullptr, c->C, false); if (st != FX_OK) return st; }   // every track a new component
    return zero_state(c);
}

fx_status fx_set_sample_rate(fx_context* c, double sr)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!(sr > 0.0)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "sample_rate must be positive");
    c->sample_rate = sr;
    return FX_OK;
}

fx_status fx_set_onset_sensitivity(fx_context* c, float s)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!(s >= 0.0f)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "sensitivity must be >= 0");   // jassert, RealTimeAnalyser.h:246
    const fx_status st = set_every_channel(c, [s](fxk::ChannelSettings& r, float& sens) { r.onset_multiplier = 1.0f + s; sens = s; });
    if (st != FX_OK) return st;
    c->onset_multiplier = 1.0f + s;
    c->onset_sensitivity = s;
    return FX_OK;
}

fx_status fx_set_onset_window(fx_context* c, int length)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (length < 1 || length > fxk::MAX_ONSET_WINDOW)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "onset window must be in [1,%d]", fxk::MAX_ONSET_WINDOW);
    const long long now = c->frames_seen;
    const fx_status st = set_every_channel(c, [length, now](fxk::ChannelSettings& r, float&) { r.onset_window = length; r.onset_reset_frame = now; });
    if (st != FX_OK) return st;
    c->onset_window = length;
    c->onset_reset_frame = c->frames_seen;      // both histories emptied, RealTimeAudioAnalysis.h:73-81
    return FX_OK;
}

fx_status fx_set_onset_type(fx_context* c, int type)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (type < FX_ONSET_SPECTRAL || type > FX_ONSET_COMBINATION) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown onset type %d", type);
    const fx_status st = set_every_channel(c, [type](fxk::ChannelSettings& r, float&) { r.onset_type = type; });
    if (st != FX_OK) return st;
    c->onset_type = type;
    return FX_OK;
}

fx_status fx_set_gain(fx_context* c, float gain)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    const fx_status st = set_every_channel(c, [gain](fxk::ChannelSettings& r, float&) { r.gain = gain; });
    if (st != FX_OK) return st;
    c->gain = gain;
    return FX_OK;
}

fx_status fx_set_channel_gains(fx_context* c, const float* gain)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!gain) return FX_OK;
    std::vector<fxk::ChannelSettings> rows;
    std::vector<float> sensitivity;
    fx_channel_rows(c, &rows, &sensitivity);
    for (int i = 0; i < c->C; i++) rows[(size_t) i].gain = gain[i];
    return fx_upload_channel_rows(c, rows, sensitivity);
}

fx_status fx_set_channel_onset(fx_context* c, const float* sensitivity, const int* window, const int* type)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!sensitivity && !window && !type) return FX_OK;
    // every entry is checked before any is taken (the context-wide setters' own conditions)
    for (int i = 0; i < c->C; i++) {
        if (sensitivity && !(sensitivity[i] >= 0.0f)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: sensitivity must be >= 0", i);
        if (window && (window[i] == 0 || window[i] > fxk::MAX_ONSET_WINDOW))
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: onset window must be in [1,%d] (or < 0: unchanged)", i, fxk::MAX_ONSET_WINDOW);
        if (type && (type[i] < FX_ONSET_SPECTRAL || type[i] > FX_ONSET_COMBINATION))
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: unknown onset type %d", i, type[i]);
    }
    std::vector<fxk::ChannelSettings> rows;
    std::vector<float> sens;
    fx_channel_rows(c, &rows, &sens);
    for (int i = 0; i < c->C; i++) {
        fxk::ChannelSettings& r = rows[(size_t) i];
        if (sensitivity) { r.onset_multiplier = 1.0f + sensitivity[i]; sens[(size_t) i] = sensitivity[i]; }
        if (window && window[i] > 0) { r.onset_window = window[i]; r.onset_reset_frame = c->frames_seen; }   // setHistoryLength: both histories emptied
        if (type) r.onset_type = type[i];
    }
    return fx_upload_channel_rows(c, rows, sens);
}

fx_status fx_get_channel_settings(fx_context* c, float* gain, float* sensitivity, int* window, int* type)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    std::vector<fxk::ChannelSettings> rows;
    std::vector<float> sens;
    fx_channel_rows(c, &rows, &sens);
    for (int i = 0; i < c->C; i++) {
        if (gain) gain[i] = rows[(size_t) i].gain;
        if (sensitivity) sensitivity[i] = sens[(size_t) i];
        if (window) window[i] = rows[(size_t) i].onset_window;
        if (type) type[i] = rows[(size_t) i].onset_type;
    }
    return FX_OK;
}

fx_status fx_push_hops(fx_context* c, const void* hops, int num_hops, int sample_format, int mem_kind,
                       float* out_raw, float* out_smoothed)
{
    begin_launches(c);
    if (c && c->carry_count > 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d samples per channel are pending from fx_push_samples; whole hops would overtake them "
                                                "(finish the stream with fx_push_samples, or fx_reset_state)", c->carry_count);
    return fx_run(c, hops, num_hops, sample_format, mem_kind, mem_kind, 1, out_raw, out_smoothed, nullptr, true, true);
}

// ---- the collector's real interface: device blocks of any length (ref AudioDataCollector.h:36-94) ----
int fx_pending_samples(fx_context* c) { return c ? c->carry_count : 0; }

fx_status fx_clear_pending(fx_context* c)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(fxk::clear_carry(c->d_carry[c->carry_cur], (size_t) c->C * (c->N / 2) * 4, c->stream));
    return FX_OK;
}

// the refusals of a block that depend on the context's pending samples alone (fx_context.h): fx_push_block makes them, and
// fx_push_interleaved makes them before its de-interleave launch
extern "C++" fx_status fx_block_refusal(const fx_context* c, int num_samples, int sample_format)
{
    if (c->carry_count > 0 && sample_format != c->carry_format)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d pending samples per channel are in sample format %d, this block in %d: a stream keeps one format "
                                                "between hop boundaries", c->carry_count, c->carry_format, sample_format);
    if (((long long) c->carry_count + num_samples) / (c->N / 2) > (1ll << 24))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "block of %d samples per channel is too long for one call", num_samples);
    return FX_OK;
}

// the launches that wrote the other carry buffer are enqueued: it holds the stream's pending samples, `rest` per channel
static void hand_carry_over(fx_context* c, int rest, int sample_format)
{
    c->carry_cur ^= 1;
    c->carry_count = rest;
    c->carry_format = sample_format;
}

// the block path of fx_push_samples (fx_context.h): the launch record is the caller's
extern "C++" fx_status fx_push_block(fx_context* c, const void* samples, int num_samples, int sample_format, int in_kind, int out_kind,
                        float* out_raw, float* out_smoothed, int* frames_out, bool taps)
{
    if (frames_out) *frames_out = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (num_samples < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative sample count");
    { const fx_status cs = fx_check_call(sample_format, in_kind, out_kind); if (cs != FX_OK) return cs; }
    if (num_samples == 0) return FX_OK;
    if (!samples) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null input buffer");
    { const fx_status rs = fx_block_refusal(c, num_samples, sample_format); if (rs != FX_OK) return rs; }
    const int H = c->N / 2;
    const size_t esz = sample_size(sample_format);
    const long long have = (long long) c->carry_count + num_samples;
    const long long hops64 = have / H;
    const int hops = (int) hops64, rest = (int) (have - hops64 * H);
    HIP_TRY(hipSetDevice(c->device));
    { const fx_status es = fx_check_device_error(c); if (es != FX_OK) return es; }

    // whole hops and nothing pending: the block IS the hop buffer -- from an aligned device buffer, or a host block (512-sample callbacks
    // against a 1024-point window: one copy in, no re-blocking)
    if (c->carry_count == 0 && rest == 0 && (in_kind == FX_MEM_HOST || reinterpret_cast<uintptr_t>(samples) % 16 == 0)) {
        const fx_status st = fx_run(c, samples, hops, sample_format, in_kind, out_kind, 1, out_raw, out_smoothed, nullptr, taps, taps);
        if (st == FX_OK && frames_out) *frames_out = hops;
        return st;
    }
    fx_status st;
    const unsigned char* d_block = static_cast<const unsigned char*>(samples);
    const size_t block_bytes = (size_t) c->C * (size_t) num_samples * esz;
    if (in_kind == FX_MEM_HOST) {
        if ((st = fx_grow(&c->d_in, &c->in_cap, block_bytes)) != FX_OK) return st;
        HIP_TRY(hipMemcpyAsync(c->d_in, samples, block_bytes, hipMemcpyHostToDevice, c->stream));
        d_block = static_cast<const unsigned char*>(c->d_in);
    } else if (reinterpret_cast<uintptr_t>(samples) % 4 != 0) {
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "device input must be 4-byte aligned (16-byte aligned to be analysed in place)");
    }
    if (hops >= 1 && hops <= (c->N == 1024 ? 4096 : 2) && blocks_feed_kernels(c)) {
        // A block that completes hops is read by the analysis kernels directly from [pending | block]: the live case -- 441 / 480 / 512 ...
        // samples, one hop; 960 / 1000 / 1024, two -- as one-frame launches, longer blocks (1024-point windows) as one launch of the batch
        // kernel's block-fed form; the call's last frame leaves the rest in the other carry buffer.  No pass over the samples beside the
        // analysis.  (Windows of 2048 / 4096 points re-block calls of more than two hops: measured faster there, fx_kernels.hip launch_t.)
        const BlockFeed feed = {c->d_carry[c->carry_cur], c->d_carry[c->carry_cur ^ 1], (int) ((size_t) c->carry_count * esz), H * 4,
                                (long long) num_samples * (long long) esz};
        st = fx_run(c, d_block, hops, sample_format, FX_MEM_DEVICE, out_kind, 1, out_raw, out_smoothed, &feed, taps, taps);
        if (st != FX_OK) return st;             // (the stream is no longer the caller's: fx_reset_state, as the contract says)
        hand_carry_over(c, rest, sample_format);
        if (frames_out) *frames_out = hops;
        return FX_OK;
    }
    const size_t hop_bytes = (size_t) c->C * (size_t) hops * H * esz;
    if ((st = fx_grow(&c->d_hops, &c->hops_cap, hop_bytes)) != FX_OK) return st;
    fxk::ReblockParams rp;
    rp.in = d_block;
    rp.carry_in = c->d_carry[c->carry_cur];
    rp.hops_out = c->d_hops;
    rp.carry_out = c->d_carry[c->carry_cur ^ 1];
    rp.in_row_bytes = (long long) num_samples * (long long) esz;
    rp.out_row_bytes = (long long) hops * H * (long long) esz;
    rp.carry_bytes = (int) ((size_t) c->carry_count * esz);
    rp.carry_row_bytes = H * 4;
    rp.C = c->C;
    // armed taps read the first hop from [pending | block] before the re-blocking kernel moves the pending samples on
    if (taps && hops > 0 && c->taps_armed && c->taps_launch) {
        const fx_tap_source src = {d_block, sample_format, 1, rp.in_row_bytes, rp.carry_in, rp.carry_bytes, rp.carry_row_bytes};
        if ((st = c->taps_launch(c, src)) != FX_OK) return st;
    }
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_REBLOCK, 0)) r->reblock = fxk::reblock_form(rp);
    HIP_TRY(fxk::launch_reblock_kernel(rp, c->stream));
    // the stream holds the new carry whatever happens to the analysis below
    hand_carry_over(c, rest, sample_format);
    if (hops > 0) {
        st = fx_run(c, c->d_hops, hops, sample_format, FX_MEM_DEVICE, out_kind, 1, out_raw, out_smoothed, nullptr, false, taps);   // (taps: served above)
        if (st != FX_OK) return st;
    } else if (in_kind == FX_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(c->stream));            // the caller's block may be reused on return
    }
    if (frames_out) *frames_out = hops;
    return FX_OK;
}

// fx_push_samples; `taps`: whether the call serves armed taps (the ring's submissions do not, include/fx.h)
extern "C++" fx_status push_samples(fx_context* c, const void* samples, int num_samples, int sample_format, int mem_kind,
                                    float* out_raw, float* out_smoothed, int* frames_out, bool taps)
{
    if (frames_out) *frames_out = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    begin_launches(c);
    return fx_push_block(c, samples, num_samples, sample_format, mem_kind, mem_kind, out_raw, out_smoothed, frames_out, taps);
}

fx_status fx_push_samples(fx_context* c, const void* samples, int num_samples, int sample_format, int mem_kind,
                          float* out_raw, float* out_smoothed, int* frames_out)
{
    return push_samples(c, samples, num_samples, sample_format, mem_kind, out_raw, out_smoothed, frames_out, true);
}

fx_status fx_process_frames(fx_context* c, const void* frames, int num_frames, int sample_format, int mem_kind,
                            float* out_raw, float* out_smoothed)
{
    begin_launches(c);
    if (c && c->carry_count > 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d samples per channel are pending from fx_push_samples (finish the stream with fx_push_samples, or fx_reset_state)", c->carry_count);
    return fx_run(c, frames, num_frames, sample_format, mem_kind, mem_kind, 0, out_raw, out_smoothed, nullptr, true, true);
}

fx_status fx_get_smoothed(fx_context* c, float* out, int mem_kind)
{
    if (!c || !out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t) c->C * FX_NUM_FEATURES * sizeof(float);
    HIP_TRY(hipMemcpyAsync(out, c->d_latest, bytes,
                           mem_kind == FX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (mem_kind != FX_MEM_DEVICE) { HIP_TRY(hipStreamSynchronize(c->stream)); return fx_check_device_error(c); }
    return FX_OK;
}


// ref OSCFeatureAnalysisOutput.h:89-113 for every track at once: the messages are formed by fx_osc_kernel from `latest`
fx_status fx_get_osc_datagrams(fx_context* c, const char* prefix, int first_channel, unsigned char* out, int stride, int* lengths, int mem_kind)
{
    if (!c || !prefix || !out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (mem_kind != FX_MEM_HOST && mem_kind != FX_MEM_DEVICE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown memory kind %d", mem_kind);
    const int longest = first_channel < 0 || first_channel > 0x7fffffff - c->C ? -1 : fx_osc_message_bytes(prefix, first_channel + c->C - 1);
    if (longest < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "OSC prefix longer than %d bytes, or a channel number out of range", fxk::FX_OSC_PREFIX_MAX);
    if (stride < longest || (stride & 3)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "stride %d: must be a multiple of 4 and hold the longest message (%d bytes)", stride, longest);
    if (mem_kind == FX_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 3)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "a device buffer of messages must start on a 4-byte boundary");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t) c->C * (size_t) stride;
    if (mem_kind == FX_MEM_HOST) { const fx_status st = fx_grow(&c->d_osc, &c->osc_cap, bytes); if (st != FX_OK) return st; }
    fxk::OscParams p = {};
    p.latest = c->d_latest;
    p.out = mem_kind == FX_MEM_HOST ? c->d_osc : out;
    p.C = c->C;
    p.stride = stride;
    p.first_channel = first_channel;
    p.prefix_len = (int) strlen(prefix);
    memcpy(p.prefix, prefix, (size_t) p.prefix_len);
    begin_launches(c);
    note_launch(c, FX_LAUNCH_OSC, 0);
    HIP_TRY(fxk::launch_osc_kernel(p, c->stream));
    if (lengths) for (int i = 0; i < c->C; i++) lengths[i] = fx_osc_message_bytes(prefix, first_channel + i);
    if (mem_kind == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, c->d_osc, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fx_check_device_error(c);
    }
    return FX_OK;
}

fx_status fx_host_alloc(void** out, size_t bytes)
{
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { (void) hipGetLastError(); return fx_fail(FX_ERR_NO_DEVICE, "no HIP device available (page-locked memory is the runtime's)"); }
    void* p = nullptr;
    HIP_TRY(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault));
    *out = p;
    return FX_OK;
}

fx_status fx_host_free(void* p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return FX_OK;
}

fx_status fx_sync(fx_context* c)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return fx_check_device_error(c);
}

fx_status fx_get_stream(fx_context* c, void** stream)
{
    if (!c || !stream) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    *stream = (void*) c->stream;
    return FX_OK;
}

fx_status fx_last_kernel_ms(fx_context* c, float* frame_ms, float* epi_ms)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!c->ev_valid) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the last analysis call recorded no timing (none made yet, a profiled one, or a one-frame call without fx_tuning::call_timing = 1)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev[2]));
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
    if (frame_ms) *frame_ms = a;
    if (epi_ms) *epi_ms = b;
    return fx_check_device_error(c);
}

fx_status fx_profile_begin(fx_context* c)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    c->profiling = true;
    c->prof_used = 0;
    return FX_OK;
}

fx_status fx_profile_end(fx_context* c, double* frame_ms, double* epi_ms, int* calls)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double a = 0.0, b = 0.0;
    for (size_t i = 0; i + 3 <= c->prof_used; i += 3) {
        float x = 0.f, y = 0.f;
        HIP_TRY(hipEventElapsedTime(&x, c->prof_events[i], c->prof_events[i + 1]));
        HIP_TRY(hipEventElapsedTime(&y, c->prof_events[i + 1], c->prof_events[i + 2]));
        a += x; b += y;
    }
    if (frame_ms) *frame_ms = a;
    if (epi_ms) *epi_ms = b;
    if (calls) *calls = (int) (c->prof_used / 3);
    c->profiling = false;
    c->prof_used = 0;
    return fx_check_device_error(c);
}

// ---- OSC sink helpers (ref OSCFeatureAnalysisOutput.h:107, README.md:57) ----
static const int k_osc12[12] = {FX_ONSET, FX_RMS, FX_F0, FX_CENTROID, FX_SLOPE, FX_SPREAD,
                                FX_FLATNESS, FX_LER, FX_FLUX, FX_HER, FX_OER, FX_INHARM};
static const int k_osc10[10] = {FX_ONSET, FX_RMS, FX_F0, FX_CENTROID, FX_SLOPE, FX_SPREAD,
                                FX_FLATNESS, FX_FLUX, FX_HER, FX_INHARM};

void fx_pack_osc12(const float* f, float* out) { for (int i = 0; i < 12; i++) out[i] = f[k_osc12[i]]; }
void fx_pack_osc10(const float* f, float* out) { for (int i = 0; i < 10; i++) out[i] = f[k_osc10[i]]; }

int fx_osc_encode(const char* address, const float* f, unsigned char* out, int cap)
{
    if (!address || !f || !out) return -1;
    const int alen = (int) strlen(address);
    const int apad = (alen + 4) & ~3;           // NUL-terminated, padded to a multiple of 4
    const int tpad = 16;                        // ",ffffffffffff" + NUL -> 16
    const int total = apad + tpad + 48;
    if (total > cap) return -1;
    memset(out, 0, (size_t) total);
    memcpy(out, address, (size_t) alen);
    memcpy(out + apad, ",ffffffffffff", 13);
    unsigned char* p = out + apad + tpad;
    for (int i = 0; i < 12; i++) {
        unsigned int bits;
        memcpy(&bits, &f[k_osc12[i]], 4);
        p[0] = (unsigned char) (bits >> 24); p[1] = (unsigned char) (bits >> 16);
        p[2] = (unsigned char) (bits >> 8);  p[3] = (unsigned char) bits;
        p += 4;
    }
    return total;
}

int fx_osc_message_bytes(const char* prefix, int channel)
{
    if (!prefix || channel < 0) return -1;
    const size_t plen = strlen(prefix);
    if (plen > (size_t) fxk::FX_OSC_PREFIX_MAX) return -1;
    int digits = 1;
    for (int t = channel; t >= 10; t /= 10) digits++;
    return (((int) plen + digits + 4) & ~3) + 16 + 48;
}

int fx_osc_encode_batch(const char* prefix, int first_channel, int num_channels, const float* smoothed, unsigned char* out, int stride, int* lengths)
{
    if (!prefix || !smoothed || !out || num_channels < 0 || first_channel < 0 || (stride & 3)) return -1;
    if (num_channels == 0) return 0;
    if (first_channel > 0x7fffffff - num_channels) return -1;
    const int longest = fx_osc_message_bytes(prefix, first_channel + num_channels - 1);
    if (longest < 0 || stride < longest) return -1;
    const size_t plen = strlen(prefix);
    char address[fxk::FX_OSC_PREFIX_MAX + 16];
    memcpy(address, prefix, plen);
    for (int c = 0; c < num_channels; c++) {
        snprintf(address + plen, sizeof address - plen, "%d", first_channel + c);
        unsigned char* slot = out + (size_t) c * (size_t) stride;
        const int n = fx_osc_encode(address, smoothed + (size_t) c * FX_NUM_FEATURES, slot, stride);
        if (n < 0) return -1;
        memset(slot + n, 0, (size_t) (stride - n));
        if (lengths) lengths[c] = n;
    }
    return num_channels;
}

// fx_osc_encode for n tracks with addresses of their own: the host twin of the device call of fx_osc_table.hip, which holds the same
// address rules (fx_osc_words.h)
int fx_osc_encode_addressed(const char* const* addresses, int n, const float* smoothed, unsigned char* out, int stride, int* lengths)
{
    if (n < 0 || (stride & 3) || (n > 0 && (!addresses || !smoothed || !out))) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument, a negative count or a stride that is no multiple of 4"); return -1; }
    int longest = 0;
    for (int c = 0; c < n; c++) {
        int alen = 0;
        if (const char* fault = fxk::osc_address_fault(addresses[c], &alen)) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: the OSC address %s", c, fault); return -1; }
        if (fxk::osc_addressed_bytes(alen) > longest) longest = fxk::osc_addressed_bytes(alen);
    }
    if (stride < longest) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "stride %d does not hold the longest message (%d bytes)", stride, longest); return -1; }
    for (int c = 0; c < n; c++) {
        unsigned char* slot = out + (size_t) c * (size_t) stride;
        const int len = fx_osc_encode(addresses[c], smoothed + (size_t) c * FX_NUM_FEATURES, slot, stride);
        if (len < 0) return -1;
        memset(slot + len, 0, (size_t) (stride - len));
        if (lengths) lengths[c] = len;
    }
    return n;
}

// ---- bundles (ref OSCFeatureAnalysisOutput.h:107 messages as the elements of OSC 1.0 bundles; fx_osc_words.h holds the layout) ----
fx_status fx_osc_bundle_plan(int longest_message_bytes, int num_tracks, int max_datagram_bytes, int* tracks_per_bundle, int* num_bundles, int* stride)
{
    if (num_tracks < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "a bundle plan for %d tracks", num_tracks);
    if (max_datagram_bytes > 65507) return fx_fail(FX_ERR_INVALID_ARGUMENT, "max_datagram_bytes %d: a UDP datagram carries at most 65507 bytes", max_datagram_bytes);
    const int K = fxk::osc_bundle_tracks(longest_message_bytes, num_tracks, max_datagram_bytes);
    if (K < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "max_datagram_bytes %d does not hold a bundle of one message of %d bytes (16 + 4 + the message)", max_datagram_bytes, longest_message_bytes);
    if (tracks_per_bundle) *tracks_per_bundle = K;
    if (num_bundles) *num_bundles = (num_tracks + K - 1) / K;
    if (stride) *stride = 16 + K * (4 + longest_message_bytes);
    return FX_OK;
}

unsigned long long fx_osc_timetag(double unix_seconds)
{
    const double ntp = unix_seconds + 2208988800.0;            // 1900-01-01 to 1970-01-01 in seconds
    if (!(ntp >= 0.0) || ntp >= 4294967296.0) return FX_OSC_TIMETAG_IMMEDIATE;
    const double whole = std::floor(ntp);
    unsigned long long fraction = (unsigned long long) ((ntp - whole) * 4294967296.0);
    if (fraction > 0xFFFFFFFFull) fraction = 0xFFFFFFFFull;
    return ((unsigned long long) whole << 32) | fraction;
}

// The bundles of `p` (host pointers; C, latest and the address source filled in), one word at a time through osc_bundle_word: the host
// twin of fx_osc_bundle_kernel.  Returns the number of bundles, or -1.
static int encode_bundles(fxk::OscBundleParams& p, int longest, unsigned long long timetag, int max_datagram_bytes, int stride, int* lengths)
{
    int K = 0, bundles = 0, need = 0;
    if (fx_osc_bundle_plan(longest, p.C, max_datagram_bytes, &K, &bundles, &need) != FX_OK) return -1;
    if (stride < need || (stride & 3)) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "stride %d: must be a multiple of 4 and hold the fullest bundle (%d bytes)", stride, need); return -1; }
    p.K = K;
    p.stride = stride;
    p.timetag_hi = (unsigned) (timetag >> 32);
    p.timetag_lo = (unsigned) timetag;
    std::vector<int> off;
    try { off.resize((size_t) K + 1); } catch (const std::bad_alloc&) { (void) fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed"); return -1; }
    for (int b = 0; b < bundles; b++) {
        const int count = p.C - b * K < K ? p.C - b * K : K;
        off[0] = fxk::FX_OSC_BUNDLE_HEADER_WORDS;
        for (int e = 0; e < count; e++) off[(size_t) e + 1] = off[(size_t) e] + 1 + fxk::osc_bundle_element_words(p, b * K + e);
        unsigned char* slot = p.out + (size_t) b * (size_t) stride;
        for (int w = 0; w < stride >> 2; w++) {
            const unsigned v = fxk::osc_bundle_word(p, b, off.data(), count, w);
            memcpy(slot + 4 * (size_t) w, &v, 4);
        }
        if (lengths) lengths[b] = 4 * off[(size_t) count];
    }
    return bundles;
}

int fx_osc_encode_bundles(const char* prefix, int first_channel, int n, const float* smoothed, unsigned long long timetag, int max_datagram_bytes,
                          unsigned char* out, int stride, int* lengths)
{
    if (!prefix || !smoothed || !out || n < 0 || first_channel < 0) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument, a negative count or a negative channel number"); return -1; }
    if (n == 0) return 0;
    const int longest = first_channel > 0x7fffffff - n ? -1 : fx_osc_message_bytes(prefix, first_channel + n - 1);
    if (longest < 0) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "OSC prefix longer than %d bytes, or a channel number out of range", fxk::FX_OSC_PREFIX_MAX); return -1; }
    fxk::OscBundleParams p = {};
    p.latest = smoothed;
    p.out = out;
    p.C = n;
    p.first_channel = first_channel;
    p.prefix_len = (int) strlen(prefix);
    memcpy(p.prefix, prefix, (size_t) p.prefix_len);
    return encode_bundles(p, longest, timetag, max_datagram_bytes, stride, lengths);
}

int fx_osc_encode_bundles_addressed(const char* const* addresses, int n, const float* smoothed, unsigned long long timetag, int max_datagram_bytes,
                                    unsigned char* out, int stride, int* lengths)
{
    if (n < 0 || (n > 0 && (!addresses || !smoothed || !out))) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument or a negative count"); return -1; }
    if (n == 0) return 0;
    // an address table's image as osc_table_word reads it: zero-padded rows and the lengths
    std::vector<unsigned> rows;
    std::vector<int> len;
    try { rows.assign((size_t) n * fxk::FX_OSC_ROW_WORDS, 0u); len.resize((size_t) n); } catch (const std::bad_alloc&) { (void) fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed"); return -1; }
    int longest = 0;
    for (int c = 0; c < n; c++) {
        int alen = 0;
        if (const char* fault = fxk::osc_address_fault(addresses[c], &alen)) { (void) fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: the OSC address %s", c, fault); return -1; }
        memcpy(rows.data() + (size_t) c * fxk::FX_OSC_ROW_WORDS, addresses[c], (size_t) alen);
        len[(size_t) c] = alen;
        if (fxk::osc_addressed_bytes(alen) > longest) longest = fxk::osc_addressed_bytes(alen);
    }
    fxk::OscBundleParams p = {};
    p.latest = smoothed;
    p.rows = rows.data();
    p.len = len.data();
    p.out = out;
    p.C = n;
    return encode_bundles(p, longest, timetag, max_datagram_bytes, stride, lengths);
}

} // extern "C"
