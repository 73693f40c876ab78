// fx_track_state.hip -- moving tracks between contexts (include/fx.h: fx_track_state_bytes, fx_export_channels, fx_import_channels).
//
// The reference's tracks are heap objects (AnalyserTrackController.h): a host moves one by moving a pointer.  Here a track is a row of
// each of the context's [C][...] tables, so the way back out is a RECORD: header, latest vector, the 48-row ring in track order, flux
// row, tail row, pending row (TrackHeader and track_piece, fx_kernels.h).  The tails only ever use differences such as frames_before -
// first_frame and g - onset_reset_frame, and ring rows relative to hist_base, so a record carries the two differences (frames,
// onset_frames) and the ring rotated to start at the track's frame frames - 48; an import turns them back into the destination's
// global indices: first_frame = frames_seen - frames, onset_reset_frame = frames_seen - onset_frames (either may be negative: every
// consumer subtracts them in long long), record row k to ring row (frames_seen - 48 + k) mod 48.
//
// Export: the host writes every listed track's header into the pinned entry list (it knows all of it: fx_context::chan and the
// context-wide values), ONE copy takes the list to the device and ONE launch of fx_pack_tracks_kernel gathers the rows behind the
// headers.  Import: the headers are checked first (a device buffer gives them up in one strided copy on the context's stream), then the slots' rows of the
// per-track table travel by fx_upload_channel_rows, as every per-track setter's do, and ONE launch of fx_unpack_tracks_kernel scatters
// the rest.  Both calls wait for the context's stream, so a fx_stream_* ring's submitted batches come before them and later ones after.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: the first call installs the context's release hook
// (fx_context.h).  The kernels are compiled by hipcc only; a host-only build of this file (tests/cpp/track_state_host.cpp) brings its
// own launch_pack_tracks_kernel / launch_unpack_tracks_kernel, written from the same track_piece().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"
#include "fx_plan.h"

#if !defined(__HIPCC__)
// (the host-only build's HIP header has no strided copy: the test program defines this one)
extern "C" hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t stream);
#endif

#if defined(__HIPCC__)
namespace fxk {

constexpr int TRACK_THREADS = 256, TRACK_WAVES = TRACK_THREADS / 64;

// A wavefront per (list entry, 64 pieces of 16 bytes): wavefront w of the launch moves pieces (w mod wave_pieces) * 64 .. + 63 of the
// record of entry w / wave_pieces, one 16-byte load and one 16-byte store per lane.  The entry's slot and frame count are read at
// wave-uniform addresses (scalar loads, like channel_gain).  No LDS, no atomics: every byte is read once and written once.
struct TrackWork { long long entry; int q, c; long long frames; bool live; };
__device__ __forceinline__ TrackWork track_work(const TrackStateParams& p, int rec_pieces)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int wave_pieces = (rec_pieces + 63) / 64;
    const long long w = (long long) blockIdx.x * TRACK_WAVES + wave;
    TrackWork k = {w / wave_pieces, 0, 0, 0, false};
    if (k.entry >= p.n) return k;
    k.q = (int) (w - k.entry * wave_pieces) * 64 + lane;
    typedef const int __attribute__((address_space(4)))* UniformIntPtr;
    typedef const long long __attribute__((address_space(4)))* UniformLongPtr;
    k.c = *(UniformIntPtr) &p.entries[k.entry].channel;
    k.frames = *(UniformLongPtr) &p.entries[k.entry].header.frames;
    k.live = (unsigned) k.c < (unsigned) p.C && k.q < rec_pieces;         // (the host has checked every entry)
    return k;
}

// tables -> records.  Writes every piece of a record: the header from the entry, zeros for ring rows of frames before the track's
// first and for the pending row's bytes beyond the pending samples.
__global__ void __launch_bounds__(TRACK_THREADS) fx_pack_tracks_kernel(const TrackStateParams p)
{
    const int rec_pieces = TRACK_FIXED_PIECES + 3 * p.row_pieces;
    const TrackWork k = track_work(p, rec_pieces);
    if (!k.live) return;
    const TrackPiece t = track_piece(k.q, p.row_pieces, p.hist_base);
    const size_t row_at = (size_t) k.c * (size_t) p.row_pieces + (size_t) t.at;
    uint4 v = {0u, 0u, 0u, 0u};
    switch (t.where) {
    case TRACK_IN_HEADER: v = reinterpret_cast<const uint4*>(&p.entries[k.entry].header)[t.at]; break;
    case TRACK_IN_LATEST: v = reinterpret_cast<const uint4*>(p.latest)[(size_t) k.c * TRACK_LATEST_PIECES + t.at]; break;
    case TRACK_IN_RING:
        if (k.frames - HLEN + t.ring_row >= 0) v = reinterpret_cast<const uint4*>(p.hist)[(size_t) k.c * TRACK_RING_PIECES + t.at];
        break;
    case TRACK_IN_PREV: v = reinterpret_cast<const uint4*>(p.prev)[row_at]; break;
    case TRACK_IN_TAIL: v = reinterpret_cast<const uint4*>(p.tail)[row_at]; break;
    default:
        if (t.at * 16 < p.carry_bytes) {
            v = reinterpret_cast<const uint4*>(p.carry)[row_at];
            v.x &= track_carry_mask(t.at, 0, p.carry_bytes);
            v.y &= track_carry_mask(t.at, 1, p.carry_bytes);
            v.z &= track_carry_mask(t.at, 2, p.carry_bytes);
            v.w &= track_carry_mask(t.at, 3, p.carry_bytes);
        }
        break;
    }
    reinterpret_cast<uint4*>(p.records)[(size_t) k.entry * (size_t) rec_pieces + (size_t) k.q] = v;
}

// records -> tables.  All 48 ring rows and the whole pending row are written (a record holds zeros where it holds nothing); the
// header's pieces are the host's to read.
__global__ void __launch_bounds__(TRACK_THREADS) fx_unpack_tracks_kernel(const TrackStateParams p)
{
    const int rec_pieces = TRACK_FIXED_PIECES + 3 * p.row_pieces;
    const TrackWork k = track_work(p, rec_pieces);
    if (!k.live) return;
    const TrackPiece t = track_piece(k.q, p.row_pieces, p.hist_base);
    if (t.where == TRACK_IN_HEADER) return;
    const uint4 v = reinterpret_cast<const uint4*>(p.records)[(size_t) k.entry * (size_t) rec_pieces + (size_t) k.q];
    const size_t row_at = (size_t) k.c * (size_t) p.row_pieces + (size_t) t.at;
    switch (t.where) {
    case TRACK_IN_LATEST: reinterpret_cast<uint4*>(p.latest)[(size_t) k.c * TRACK_LATEST_PIECES + t.at] = v; break;
    case TRACK_IN_RING: reinterpret_cast<uint4*>(p.hist)[(size_t) k.c * TRACK_RING_PIECES + t.at] = v; break;
    case TRACK_IN_PREV: reinterpret_cast<uint4*>(p.prev)[row_at] = v; break;
    case TRACK_IN_TAIL: reinterpret_cast<uint4*>(p.tail)[row_at] = v; break;
    default: reinterpret_cast<uint4*>(p.carry)[row_at] = v; break;
    }
}

template <typename K> static hipError_t launch_tracks(K kernel, const TrackStateParams& p, hipStream_t stream)
{
    if (p.n <= 0) return hipSuccess;
    const long long waves = (long long) p.n * (long long) ((track_record_pieces(p.row_pieces * 8) + 63) / 64);
    const long long wgs = (waves + TRACK_WAVES - 1) / TRACK_WAVES;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned) wgs), dim3(TRACK_THREADS), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_pack_tracks_kernel(const TrackStateParams& p, hipStream_t stream) { return launch_tracks(fx_pack_tracks_kernel, p, stream); }
hipError_t launch_unpack_tracks_kernel(const TrackStateParams& p, hipStream_t stream) { return launch_tracks(fx_unpack_tracks_kernel, p, stream); }

} // namespace fxk
#endif

struct fx_track_state {
    fx_staged_list entries;                 // of fxk::TrackEntry
    fxk::TrackEntry* h_entries() const { return static_cast<fxk::TrackEntry*>(entries.pinned); }
    fxk::TrackEntry* d_entries() const { return static_cast<fxk::TrackEntry*>(entries.device); }
    unsigned char* d_records = nullptr;     // a call whose buffer is host memory: the records of one chunk (at most SCRATCH_BYTES)
    size_t records_cap = 0;
};

namespace {

constexpr unsigned STATE_FLAGS = FX_ORDER_MASK | FX_SPECTRAL_ONLY | FX_HARMONIC_ONLY;

void track_state_release(fx_context* c)
{
    fx_track_state* t = c->track_state;
    if (!t) return;
    if (t->d_records) (void) hipFree(t->d_records);
    fx_release_list(&t->entries);
    delete t;
    c->track_state = nullptr;
}

size_t record_bytes(const fx_context* c) { return fxk::track_record_pieces(c->N) * 16; }

// the list and the buffer, fx_reset_channels' rules for the first: every entry is checked before anything is touched, no device use
fx_status check_call(const fx_context* c, const int* channels, int num_channels, const void* buffer, size_t bytes, int mem_kind, bool import)
{
    fx_status st = fx_check_channel_list(c, channels, num_channels);
    if (st == FX_OK) st = fx_check_channel_entries(c, channels, num_channels);
    if (st == FX_OK) st = fx_check_memory_kind(mem_kind);
    if (st != FX_OK) return st;
    if (num_channels == 0) return FX_OK;
    if (import) {
        // (the order of two writes to one slot would decide the result)
        std::vector<int> seen((size_t) c->C, -1);
        for (int i = 0; i < num_channels; i++) {
            int& first = seen[(size_t) channels[i]];
            if (first >= 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: channel %d is listed twice (entry %d)", i, channels[i], first);
            first = i;
        }
    }
    if (!buffer) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null record buffer");
    const size_t need = (size_t) num_channels * record_bytes(c);
    if (bytes < need) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the record buffer holds %zu bytes; %d records of %zu need %zu", bytes, num_channels, record_bytes(c), need);
    if (mem_kind == FX_MEM_DEVICE && reinterpret_cast<uintptr_t>(buffer) % 16 != 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "a device record buffer must be 16-byte aligned");
    return FX_OK;
}

// A call whose buffer is host memory moves its records through device scratch a chunk at a time, so that moving every track of a
// large context (a restart) does not leave the context holding as much scratch as state: at most 32 MB, one record at least.
// FX_HOOK_SMALL_TRACK_CHUNKS (tests): two records a chunk.
constexpr size_t SCRATCH_BYTES = (size_t) 32 << 20;
size_t chunk_records(const fx_context* c)
{
    if (c->test_hooks & FX_HOOK_SMALL_TRACK_CHUNKS) return 2;
    const size_t n = SCRATCH_BYTES / record_bytes(c);
    return n ? n : 1;
}

// room for n entries in the pinned and the device list (fx_reserve_list, fx_context.h) and for `records` records in the device scratch
fx_status reserve(fx_context* c, size_t n, size_t records)
{
    if (!c->track_state) {
        c->track_state = new (std::nothrow) fx_track_state();
        if (!c->track_state) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
        c->track_state_release = track_state_release;
    }
    fx_track_state* t = c->track_state;
    { const fx_status st = fx_reserve_list(c, &t->entries, n, sizeof(fxk::TrackEntry)); if (st != FX_OK) return st; }
    if (records) return fx_grow(&t->d_records, &t->records_cap, records * record_bytes(c));
    return FX_OK;
}

int family_of(const fx_context* c) { return uses_pairs(c, c->tuning.waves_per_frame) ? 2 : 1; }

// what the track in slot `channel` would say of itself now
fxk::TrackHeader header_of(const fx_context* c, const fxk::ChannelSettings& r, float sensitivity)
{
    fxk::TrackHeader h;
    memset(&h, 0, sizeof h);
    h.magic = fxk::TRACK_MAGIC;
    h.version = fxk::TRACK_LAYOUT_VERSION;
    h.N = c->N;
    h.flags = c->flags & STATE_FLAGS;
    h.family = family_of(c);
    h.pending = c->carry_count;
    h.carry_format = c->carry_count > 0 ? c->carry_format : FX_SAMPLE_F32;
    h.onset_window = r.onset_window;
    h.frames = c->frames_seen - r.first_frame;
    h.onset_frames = c->frames_seen - r.onset_reset_frame;
    h.gain = r.gain;
    h.sensitivity = sensitivity;
    h.onset_multiplier = r.onset_multiplier;
    h.onset_type = r.onset_type;
    h.record_bytes = (unsigned) record_bytes(c);
    return h;
}

// entries [first, first + n) of the uploaded list, their records at `records`
fxk::TrackStateParams params_of(fx_context* c, size_t first, size_t n, unsigned char* records)
{
    fxk::TrackStateParams p;
    p.entries = c->track_state->d_entries() + first;
    p.n = (int) n;
    p.C = c->C;
    p.row_pieces = c->N / 8;                    // N/2 * 4 bytes in 16-byte pieces
    p.hist_base = (int) (c->frames_seen % fxk::HLEN);
    p.carry_bytes = (int) ((size_t) c->carry_count * sample_size(c->carry_format));
    p.prev = c->d_prev;
    p.tail = c->d_tail[c->cur];
    p.carry = c->d_carry[c->carry_cur];
    p.hist = c->d_hist;
    p.latest = c->d_latest;
    p.records = records;
    return p;
}

// whether record i may go into this context: FX_OK, or FX_ERR_INVALID_ARGUMENT naming the record and the field
fx_status check_header(const fx_context* c, int i, const fxk::TrackHeader& h)
{
    if (h.magic != fxk::TRACK_MAGIC) return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: not a track record (magic %08x)", i, h.magic);
    if (h.version != fxk::TRACK_LAYOUT_VERSION)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: layout version %u, this library reads %u", i, h.version, fxk::TRACK_LAYOUT_VERSION);
    if (h.N != c->N) return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: window size %d, the context's is %d", i, h.N, c->N);
    if (h.record_bytes != record_bytes(c)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: record size %u, the context's is %zu", i, h.record_bytes, record_bytes(c));
    if (h.flags != (c->flags & STATE_FLAGS))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: create flags %#x (order and analysers), the context's are %#x", i, h.flags, c->flags & STATE_FLAGS);
    if (h.family != family_of(c))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: kernel family of %d wavefronts per frame, the context's is %d", i, h.family, family_of(c));
    if (h.pending != c->carry_count)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: pending count %d, the context's is %d", i, h.pending, c->carry_count);
    if (h.pending > 0 && h.carry_format != c->carry_format)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: carry format %d, the context's pending samples are of format %d", i, h.carry_format, c->carry_format);
    // what the setters refuse, a record does not bring in either
    if (h.frames < 0 || h.onset_frames < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: negative frame count", i);
    if (h.onset_window < 1 || h.onset_window > fxk::MAX_ONSET_WINDOW) return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: onset window %d", i, h.onset_window);
    if (h.onset_type < FX_ONSET_SPECTRAL || h.onset_type > FX_ONSET_COMBINATION) return fx_fail(FX_ERR_INVALID_ARGUMENT, "record %d: onset type %d", i, h.onset_type);
    return FX_OK;
}

} // namespace

extern "C" {

size_t fx_track_state_bytes(fx_context* c) { return c ? record_bytes(c) : 0; }

fx_status fx_export_channels(fx_context* c, const int* channels, int num_channels, void* out, size_t out_bytes, int mem_kind)
{
    fx_status st = check_call(c, channels, num_channels, out, out_bytes, mem_kind, false);
    if (st != FX_OK || num_channels == 0) return st;
    const bool host = mem_kind == FX_MEM_HOST;
    const size_t rec = record_bytes(c), total = (size_t) num_channels;
    const size_t chunk = host ? (chunk_records(c) < total ? chunk_records(c) : total) : total;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // (the batches submitted so far are in the tables; the pinned list is free)
    if ((st = reserve(c, total, host ? chunk : 0)) != FX_OK) return st;
    fx_track_state* t = c->track_state;
    // what each listed track runs with: its row of the table, or the context-wide values (first_frame 0) while there is none (fx_channel_rows)
    const fxk::ChannelSettings wide = {c->gain, c->onset_multiplier, c->onset_window, c->onset_type, c->onset_reset_frame, 0};
    for (int i = 0; i < num_channels; i++) {
        const size_t ch = (size_t) channels[i];
        fxk::TrackEntry& e = t->h_entries()[i];
        memset(&e, 0, sizeof e);
        e.header = c->chan.empty() ? header_of(c, wide, c->onset_sensitivity) : header_of(c, c->chan[ch], c->chan_sensitivity[ch]);
        e.channel = channels[i];
    }
    HIP_TRY(hipMemcpyAsync(t->d_entries(), t->h_entries(), (size_t) num_channels * sizeof(fxk::TrackEntry), hipMemcpyHostToDevice, c->stream));
    // (the stream orders a chunk's copy out of the scratch before the next chunk's launch into it)
    for (size_t first = 0; first < total; first += chunk) {
        const size_t n = total - first < chunk ? total - first : chunk;
        const fxk::TrackStateParams p = params_of(c, first, n, host ? t->d_records : static_cast<unsigned char*>(out));
        const hipError_t e = fxk::launch_pack_tracks_kernel(p, c->stream);
        if (e != hipSuccess) return fx_fail(FX_ERR_HIP, "launching the track export failed: %s", hipGetErrorString(e));
        if (host) HIP_TRY(hipMemcpyAsync(static_cast<unsigned char*>(out) + first * rec, t->d_records, n * rec, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return fx_check_device_error(c);
}

fx_status fx_import_channels(fx_context* c, const int* channels, int num_channels, const void* in, size_t in_bytes, int mem_kind)
{
    fx_status st = check_call(c, channels, num_channels, in, in_bytes, mem_kind, true);
    if (st != FX_OK || num_channels == 0) return st;
    const bool host = mem_kind == FX_MEM_HOST;
    const size_t rec = record_bytes(c), total = (size_t) num_channels;
    const size_t chunk = host ? (chunk_records(c) < total ? chunk_records(c) : total) : total;
    // every header is judged before anything changes: a host buffer's before any device use, a device buffer's after one strided copy.
    // That copy runs on the context's stream, like every other use of a device buffer: whatever the caller queued there to fill the
    // buffer (fx_get_stream), or made that stream wait for, comes first.
    std::vector<fxk::TrackHeader> headers((size_t) num_channels);
    if (host) {
        for (int i = 0; i < num_channels; i++) memcpy(&headers[(size_t) i], static_cast<const unsigned char*>(in) + (size_t) i * rec, sizeof(fxk::TrackHeader));
    } else {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpy2DAsync(headers.data(), sizeof(fxk::TrackHeader), in, rec, sizeof(fxk::TrackHeader), total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < num_channels; i++)
        if ((st = check_header(c, i, headers[(size_t) i])) != FX_OK) return st;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((st = reserve(c, total, host ? chunk : 0)) != FX_OK) return st;
    fx_track_state* t = c->track_state;
    // the rows first (their upload waits for the stream): whole or not at all, the host mirror and the device table equal either way
    std::vector<fxk::ChannelSettings> rows;
    std::vector<float> sensitivity;
    fx_channel_rows(c, &rows, &sensitivity);
    for (int i = 0; i < num_channels; i++) {
        const fxk::TrackHeader& h = headers[(size_t) i];
        fxk::ChannelSettings& r = rows[(size_t) channels[i]];
        r.gain = h.gain;
        r.onset_multiplier = h.onset_multiplier;
        r.onset_window = h.onset_window;
        r.onset_type = h.onset_type;
        r.first_frame = c->frames_seen - h.frames;
        r.onset_reset_frame = c->frames_seen - h.onset_frames;
        sensitivity[(size_t) channels[i]] = h.sensitivity;
    }
    if ((st = fx_upload_channel_rows(c, rows, sensitivity)) != FX_OK) return st;
    for (int i = 0; i < num_channels; i++) {
        fxk::TrackEntry& e = t->h_entries()[i];
        memset(&e, 0, sizeof e);
        e.header = headers[(size_t) i];
        e.channel = channels[i];
    }
    HIP_TRY(hipMemcpyAsync(t->d_entries(), t->h_entries(), (size_t) num_channels * sizeof(fxk::TrackEntry), hipMemcpyHostToDevice, c->stream));
    for (size_t first = 0; first < total; first += chunk) {
        const size_t n = total - first < chunk ? total - first : chunk;
        if (host) HIP_TRY(hipMemcpyAsync(t->d_records, static_cast<const unsigned char*>(in) + first * rec, n * rec, hipMemcpyHostToDevice, c->stream));
        const fxk::TrackStateParams p = params_of(c, first, n, host ? t->d_records : static_cast<unsigned char*>(const_cast<void*>(in)));
        const hipError_t e = fxk::launch_unpack_tracks_kernel(p, c->stream);
        if (e != hipSuccess) return fx_fail(FX_ERR_HIP, "launching the track import failed: %s", hipGetErrorString(e));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return fx_check_device_error(c);
}

} // extern "C"
