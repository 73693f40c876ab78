// fx_tracks.hip -- per-track reset and clear (include/fx.h: fx_reset_channels, fx_clear_pending_channels, fx_get_channel_frames).
//
// ref AnalyserTrackController.h:199-210, MainComponent.cpp:137-186: every track is an object of its own, destroyed and built again one
// at a time; a fresh one has an empty overlap buffer, zero flux state, empty ValueHistorys and a zeroed collector ring.  The transport
// buttons call AudioDataCollector::clearBuffer on that track's collectors only (AnalyserTrackController.h:109-112,135-137,167-171).
//
// A reset is two things.  (1) The track's rows of the per-track table (ChannelSettings, fx_kernels.h) get first_frame = onset_reset_frame
// = the global index of the next frame: the tails count what the track's histories hold from there (track_frames_before), and its rows
// of the [C][HLEN][12] ring that are older are never valid, so the ring is not touched.  The rows travel by the staged upload every
// per-track setter uses (fx_upload_channel_rows), which keeps fx_context::chan and the device table equal.  (2) ONE launch of
// fx_reset_channels_kernel zeroes the listed tracks' rows of the flux state, of the window tail and of the pending samples the next
// call reads, and of the latest vector; fx_clear_pending_channels is the same launch with the pending rows alone.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: the first call installs the context's release hook (fx_context.h).  The kernel is
// compiled by hipcc only; a host-only build of this file (tests/cpp/track_reset_host.cpp) brings its own launch_reset_channels_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"

#if defined(__HIPCC__)
namespace fxk {

constexpr int RESET_THREADS = 256, RESET_WAVES = RESET_THREADS / 64;

// A wavefront per row piece of 64 x 16 bytes: wavefront w of the launch zeroes piece (w mod pieces) of the rows of list entry
// (w / pieces), one 16-byte store per lane and buffer; the first wavefront of an entry also takes the three 16-byte pieces of the
// latest vector.  The entry is read at a wave-uniform address (a scalar load, like channel_gain).  Duplicates in the list store the
// same zeros twice.
__global__ void __launch_bounds__(RESET_THREADS) fx_reset_channels_kernel(const ResetParams p)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int wave_pieces = (p.row_pieces + 63) / 64;
    const long long w = (long long) blockIdx.x * RESET_WAVES + wave;
    const long long entry = w / wave_pieces;
    if (entry >= p.n) return;
    const int piece0 = (int) (w - entry * wave_pieces) * 64;
    typedef const int __attribute__((address_space(4)))* UniformIntPtr;
    const int c = *(UniformIntPtr) (p.list + entry);
    if ((unsigned) c >= (unsigned) p.C) return;                       // (the host has checked every entry)
    const uint4 zero = {0u, 0u, 0u, 0u};
    const int piece = piece0 + lane;
    if (piece < p.row_pieces) {
        const size_t at = (size_t) c * (size_t) p.row_pieces + (size_t) piece;
        if (p.clear & FX_CLEAR_PREV) reinterpret_cast<uint4*>(p.prev)[at] = zero;
        if (p.clear & FX_CLEAR_TAIL) reinterpret_cast<uint4*>(p.tail)[at] = zero;
        if (p.clear & FX_CLEAR_CARRY) reinterpret_cast<uint4*>(p.carry)[at] = zero;
    }
    if ((p.clear & FX_CLEAR_LATEST) && piece0 == 0 && lane < FX_NUM_FEATURES / 4)
        reinterpret_cast<uint4*>(p.latest)[(size_t) c * (FX_NUM_FEATURES / 4) + lane] = zero;
}
static_assert(FX_NUM_FEATURES % 4 == 0, "a latest row is whole 16-byte pieces");

hipError_t launch_reset_channels_kernel(const ResetParams& p, hipStream_t stream)
{
    if (p.n <= 0 || !p.clear) return hipSuccess;
    const long long waves = (long long) p.n * ((p.row_pieces + 63) / 64);
    const long long wgs = (waves + RESET_WAVES - 1) / RESET_WAVES;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fx_reset_channels_kernel, dim3((unsigned) wgs), dim3(RESET_THREADS), 0, stream, p);
    return hipGetLastError();
}

} // namespace fxk
#endif

struct fx_tracks {
    fx_staged_list list;            // of int
};

namespace {

void tracks_release(fx_context* c)
{
    fx_tracks* t = c->tracks;
    if (!t) return;
    fx_release_list(&t->list);
    delete t;
    c->tracks = nullptr;
}

// every entry is checked before anything is touched: no device use
fx_status check_list(const fx_context* c, const int* channels, int num_channels)
{
    const fx_status st = fx_check_channel_list(c, channels, num_channels);
    return st != FX_OK ? st : fx_check_channel_entries(c, channels, num_channels);
}

// room for n entries in the pinned and the device list (fx_reserve_list, fx_context.h)
fx_status reserve_list(fx_context* c, size_t n)
{
    if (!c->tracks) {
        c->tracks = new (std::nothrow) fx_tracks();
        if (!c->tracks) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
        c->tracks_release = tracks_release;
    }
    return fx_reserve_list(c, &c->tracks->list, n, sizeof(int));
}

// the list to the device and the one launch, on the context's stream (idle when this is called: the pinned list is free)
fx_status clear_rows(fx_context* c, const int* channels, int num_channels, unsigned clear)
{
    fx_tracks* t = c->tracks;
    int* d_list = static_cast<int*>(t->list.device);
    memcpy(t->list.pinned, channels, (size_t) num_channels * sizeof(int));
    HIP_TRY(hipMemcpyAsync(d_list, t->list.pinned, (size_t) num_channels * sizeof(int), hipMemcpyHostToDevice, c->stream));
    fxk::ResetParams p;
    p.list = d_list;
    p.n = num_channels;
    p.C = c->C;
    p.row_pieces = c->N / 8;                    // N/2 * 4 bytes in 16-byte pieces
    p.clear = clear;
    p.prev = c->d_prev;
    p.tail = c->d_tail[c->cur];
    p.carry = c->d_carry[c->carry_cur];
    p.latest = c->d_latest;
    const hipError_t e = fxk::launch_reset_channels_kernel(p, c->stream);
    if (e != hipSuccess) return fx_fail(FX_ERR_HIP, "launching the per-track clear failed: %s", hipGetErrorString(e));
    return FX_OK;
}

} // namespace

extern "C" {

fx_status fx_reset_channels(fx_context* c, const int* channels, int num_channels)
{
    fx_status st = check_list(c, channels, num_channels);
    if (st != FX_OK || num_channels == 0) return st;
    HIP_TRY(hipSetDevice(c->device));
    if ((st = reserve_list(c, (size_t) num_channels)) != FX_OK) return st;
    // the rows first (their upload waits for the stream: after it the pinned list is free too): whole or not at all, the host mirror and the device table equal either way
    std::vector<fxk::ChannelSettings> rows;
    std::vector<float> sensitivity;
    fx_channel_rows(c, &rows, &sensitivity);
    for (int i = 0; i < num_channels; i++) {
        fxk::ChannelSettings& r = rows[(size_t) channels[i]];
        r.first_frame = c->frames_seen;
        r.onset_reset_frame = c->frames_seen;
    }
    if ((st = fx_upload_channel_rows(c, rows, sensitivity)) != FX_OK) return st;
    if ((st = clear_rows(c, channels, num_channels, fxk::FX_CLEAR_PREV | fxk::FX_CLEAR_TAIL | fxk::FX_CLEAR_CARRY | fxk::FX_CLEAR_LATEST)) != FX_OK) return st;
    // the audio display's own launch (fx_display.hip): the listed tracks' components are new ones too
    return c->display_reset ? c->display_reset(c, channels, num_channels, false) : FX_OK;
}

fx_status fx_clear_pending_channels(fx_context* c, const int* channels, int num_channels)
{
    fx_status st = check_list(c, channels, num_channels);
    if (st != FX_OK || num_channels == 0) return st;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((st = reserve_list(c, (size_t) num_channels)) != FX_OK) return st;
    return clear_rows(c, channels, num_channels, fxk::FX_CLEAR_CARRY);
}

fx_status fx_get_channel_frames(fx_context* c, long long* frames)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!frames) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null output array");
    for (int i = 0; i < c->C; i++) frames[i] = c->frames_seen - (c->chan.empty() ? 0 : c->chan[(size_t) i].first_frame);
    return FX_OK;
}

} // extern "C"
