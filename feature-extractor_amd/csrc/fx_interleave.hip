// fx_interleave.hip -- interleaved input through a per-track channel map (include/fx.h, fx_set_channel_map / fx_push_interleaved).
//
// ref MainComponent.cpp:140-170 builds one track per active input of the audio device, and each track's AudioDataCollector collects
// one device channel, channelData[channelToCollect] (AudioDataCollector.h:21-23,36-70), which setChannelToCollect (:123) moves while
// the stream runs.  Here every track's source is one entry of the context's channel map, and a block arrives as the device and file
// formats carry it, interleaved: [n][K] frames of K source channels.  One launch of fx_deinterleave_kernel turns it into the planar
// block [C][n] that fx_push_samples takes (track c's row = source map[c]) in a staging buffer, and fx_push_block (fx_capi.cpp) does
// the rest: the same launches, the same bits as fx_push_samples of that planar block.  Bytes only: no conversion, no gain (the
// analysis kernels' load stage does both).
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: the first fx_set_channel_map / fx_push_interleaved installs the context's release hook.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"
#include "fx_planar_tile.hip.h"

namespace fxk {
namespace {

struct DeinterleaveParams {
    const unsigned char* in;    // [n][K] samples of B bytes
    const int*           map;   // [C], 0 <= map[c] < K
    unsigned char*       out;   // [C][n] samples of B bytes, 16-byte aligned
    long long            n;
    int                  K, C;
};

template <int B> __device__ __forceinline__ unsigned load_sample(const unsigned char* p)
{
    if constexpr (B == 4) return *reinterpret_cast<const unsigned*>(p);
    else if constexpr (B == 2) return *reinterpret_cast<const unsigned short*>(p);
    else return (unsigned) p[0] | ((unsigned) p[1] << 8) | ((unsigned) p[2] << 16);
}

// A workgroup takes PT_FRAMES frames of PT_TRACKS consecutive tracks.  Load: lane = track, wavefront = frame, so a wavefront reads
// samples[f][map[c0 .. c0 + 63]] -- one contiguous run of 64 samples for the identity map or any map of consecutive sources.  The
// samples go to the tile of fx_planar_tile.hip.h, each row at the byte its planar destination has modulo 16, and from there to the
// planar rows.
template <int B>
__global__ void __launch_bounds__(PT_THREADS)
fx_deinterleave_kernel(const DeinterleaveParams p)
{
    constexpr int ROW = pt_row_bytes(B);
    __shared__ __attribute__((aligned(16))) unsigned char tile[PT_TRACKS * ROW];
    const long long f0 = (long long) blockIdx.x * PT_FRAMES;
    const int c0 = (int) blockIdx.y * PT_TRACKS;
    const int nf = p.n - f0 < PT_FRAMES ? (int) (p.n - f0) : PT_FRAMES;
    const long long row_bytes = p.n * B;

    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = c0 + lane;
        if (c < p.C) {
            const int m = (int) (((long long) c * row_bytes + f0 * B) & 15);
            const unsigned char* src = p.in + (f0 * p.K + p.map[c]) * B;
            const long long pitch = (long long) p.K * B;
            unsigned v[PT_FRAMES / 4];
#pragma unroll
            for (int j = 0; j < PT_FRAMES / 4; j++) {
                const int f = wave + 4 * j;
                if (f < nf) v[j] = load_sample<B>(src + f * pitch);
            }
#pragma unroll
            for (int j = 0; j < PT_FRAMES / 4; j++) {
                const int f = wave + 4 * j;
                if (f < nf) store_sample<B>(tile, lane, ROW, m + f * B, v[j]);
            }
        }
    }
    __syncthreads();

    tile_to_rows<B>(tile, p.out, c0, p.C, row_bytes, f0 * B, nf);
}

hipError_t launch_deinterleave_kernel(const DeinterleaveParams& p, int bytes_per_sample, hipStream_t stream)
{
    if (p.n <= 0 || p.C <= 0) return hipSuccess;
    const long long gx = (p.n + PT_FRAMES - 1) / PT_FRAMES, gy = ((long long) p.C + PT_TRACKS - 1) / PT_TRACKS;
    if (gx > 0x7fffffffll || gy > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned) gx, (unsigned) gy), block(PT_THREADS);
    switch (bytes_per_sample) {
        case 4: hipLaunchKernelGGL(fx_deinterleave_kernel<4>, grid, block, 0, stream, p); break;
        case 3: hipLaunchKernelGGL(fx_deinterleave_kernel<3>, grid, block, 0, stream, p); break;
        case 2: hipLaunchKernelGGL(fx_deinterleave_kernel<2>, grid, block, 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace
} // namespace fxk

struct fx_interleave {
    std::vector<int> map;               // [C]: track c collects source map[c]
    int              max_source = 0;    // the largest entry: blocks of fewer source channels are refused
    int*             d_map = nullptr;   // device copy of map
    unsigned char*   d_src = nullptr;   // a host block's interleaved samples
    unsigned char*   d_planar = nullptr;// the planar block handed to fx_push_block
    size_t           src_cap = 0, planar_cap = 0;
};

namespace {

void interleave_release(fx_context* c)
{
    fx_interleave* s = c->interleave;
    if (!s) return;
    fx_free_device({s->d_map, s->d_src, s->d_planar});
    delete s;
    c->interleave = nullptr;
}

// the context's state for interleaved input, with the identity map on first use
fx_status interleave_state(fx_context* c, fx_interleave** out)
{
    if (!c->interleave) {
        std::vector<int> identity((size_t) c->C);
        for (int i = 0; i < c->C; i++) identity[(size_t) i] = i;
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, sizeof(int) * (size_t) c->C));
        const hipError_t e = hipMemcpy(q, identity.data(), sizeof(int) * (size_t) c->C, hipMemcpyHostToDevice);
        fx_interleave* s = e == hipSuccess ? new (std::nothrow) fx_interleave() : nullptr;
        if (!s) {
            (void) hipFree(q);
            return e != hipSuccess ? fx_fail(FX_ERR_HIP, "hipMemcpy of the channel map failed: %s", hipGetErrorString(e))
                                   : fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
        }
        s->map.swap(identity);
        s->max_source = c->C - 1;
        s->d_map = static_cast<int*>(q);
        c->interleave = s;
        c->interleave_release = interleave_release;
    }
    *out = c->interleave;
    return FX_OK;
}

} // namespace

extern "C" {

fx_status fx_set_channel_map(fx_context* c, const int* map)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    int top = c->C - 1;
    if (map) {
        top = 0;
        for (int i = 0; i < c->C; i++) {
            if (map[i] < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "map[%d] = %d: a source channel is >= 0", i, map[i]);
            if (map[i] > top) top = map[i];
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    fx_interleave* s = nullptr;
    fx_status st;
    if ((st = interleave_state(c, &s)) != FX_OK) return st;
    std::vector<int> next((size_t) c->C);
    for (int i = 0; i < c->C; i++) next[(size_t) i] = map ? map[i] : i;
    // blocks already pushed read the old map on the device: they finish before it is replaced.  The host copy, and the bound that
    // fx_push_interleaved checks, change only once the device copy has.
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(s->d_map, next.data(), sizeof(int) * (size_t) c->C, hipMemcpyHostToDevice));
    s->map.swap(next);
    s->max_source = top;
    return FX_OK;
}

fx_status fx_push_interleaved(fx_context* c, const void* samples, int num_samples, int num_source_channels, int sample_format,
                              int mem_kind, float* out_raw, float* out_smoothed, int* frames_out)
{
    if (frames_out) *frames_out = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    c->num_launches = 0;
    if (num_samples < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative sample count");
    if (num_source_channels < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d source channels: a frame holds at least one", num_source_channels);
    { const fx_status cs = fx_check_call(sample_format, mem_kind, mem_kind); if (cs != FX_OK) return cs; }
    if (num_samples == 0) return FX_OK;
    if (!samples) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null input buffer");
    if (mem_kind == FX_MEM_DEVICE && reinterpret_cast<uintptr_t>(samples) % 4 != 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "device input must be 4-byte aligned");
    // fx_push_block's own refusals, before the de-interleave is launched: a refused call changes nothing
    { const fx_status rs = fx_block_refusal(c, num_samples, sample_format); if (rs != FX_OK) return rs; }
    const int top = c->interleave ? c->interleave->max_source : c->C - 1;
    if (top >= num_source_channels)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "the channel map reads source channel %d; the block has %d", top, num_source_channels);

    HIP_TRY(hipSetDevice(c->device));
    { const fx_status es = fx_check_device_error(c); if (es != FX_OK) return es; }
    fx_interleave* s = nullptr;
    fx_status st;
    if ((st = interleave_state(c, &s)) != FX_OK) return st;
    const int esz = (int) sample_size(sample_format);
    const size_t in_bytes = (size_t) num_samples * (size_t) num_source_channels * (size_t) esz;
    const size_t planar_bytes = (size_t) c->C * (size_t) num_samples * (size_t) esz;
    const unsigned char* d_in = static_cast<const unsigned char*>(samples);
    if (mem_kind == FX_MEM_HOST) {
        if ((st = fx_grow(&s->d_src, &s->src_cap, in_bytes)) != FX_OK) return st;
        HIP_TRY(hipMemcpyAsync(s->d_src, samples, in_bytes, hipMemcpyHostToDevice, c->stream));
        d_in = s->d_src;
    }
    if ((st = fx_grow(&s->d_planar, &s->planar_cap, planar_bytes)) != FX_OK) return st;
    fxk::DeinterleaveParams p;
    p.in = d_in;
    p.map = s->d_map;
    p.out = s->d_planar;
    p.n = num_samples;
    p.K = num_source_channels;
    p.C = c->C;
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_DEINTERLEAVE, 0)) r->T = num_samples;
    HIP_TRY(fxk::launch_deinterleave_kernel(p, esz, c->stream));
    int frames = 0;
    st = fx_push_block(c, s->d_planar, num_samples, sample_format, FX_MEM_DEVICE, mem_kind, out_raw, out_smoothed, &frames, true);
    if (st != FX_OK) return st;
    // the caller may reuse a host block on return (a call that analysed frames into host memory has synchronised already)
    if (mem_kind == FX_MEM_HOST && frames == 0) HIP_TRY(hipStreamSynchronize(c->stream));
    if (frames_out) *frames_out = frames;
    return FX_OK;
}

} // extern "C"
