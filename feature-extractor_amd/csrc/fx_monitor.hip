// fx_monitor.hip -- the monitor mix (include/fx.h: fx_enable_monitor .. fx_get_monitor): every tick's tracks summed to a stereo output.
//
// ref AudioFilePlayer.h:30-34: a player is an AudioSourcePlayer on the device manager, so what a track plays is also HEARD -- every
// player renders into the sound card's output buffers and the speakers carry the sum.  Here the tick's planar block [C][n]
// (fx_clips.hip: the live rows, the clips, the resampler's rows) is in device memory when fx_push_sources hands it to the analysers,
// and an enabled monitor mixes it down to [2][n] fp32 on the way, through a per-track send table (on, left gain, right gain).
//
// The sum's ORDER is the specification (include/fx.h, "The mix"): tracks ascending inside groups of FX_MONITOR_GROUP, then the groups
// ascending, every operation IEEE fp32 and none contracted -- one bit pattern whatever the launch geometry.  So there are two
// kernels and no atomics: fx_monitor_mix_kernel, a wavefront per (group, tile of samples) with lanes along the samples, writes the
// group's partial rows P[g][ch][i]; fx_monitor_sum_kernel, a thread per (ch, i), adds the groups' rows in order.  A context of one
// group writes its partial rows straight to the output and launches no second kernel.
//
// LISTENING TRACKS (include/fx.h, "Listening tracks"; ref AudioDataCollector.h:42,53: a file track's collectors copy one channel of the
// device's OUTPUT buffer).  Once the mix is complete fx_monitor_listen_kernel copies an output row over the row of every track that
// listens to it, a wavefront per (listener, tile of samples), so the analysers that follow read the mix.  The mix was formed from
// every track's own row before, so nothing feeds back.  A context in which no track listens never launches it.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: fx_enable_monitor installs the context's hooks.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <cmath>
#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"

#pragma clang fp contract(off)

namespace fxk {

// (the load stage's widen_four: what the monitor makes of a sample is what the analysis kernels do)
#include "fx_wave.hip.h"          // f4
#include "fx_samples.hip.h"
#include "fx_blocks.hip.h"        // the shifted 16-byte read, dwords4

namespace {

static_assert(FX_MONITOR_GROUP == 64, "a group's 64 sends are walked by one wavefront; include/fx.h states the number");

// A track's send.  One 16-byte row: a group's 64 are one 1-KB load, a row per lane.
struct __attribute__((aligned(16))) MonitorSend {
    int   on;
    float left, right;
    int   listen;       // FX_LISTEN_*: what the track's analysers hear.  The host's column is the truth; the kernels walk ListenEntry
};
static_assert(sizeof(MonitorSend) == 16, "a send is one 16-byte piece");

struct MixParams {
    const unsigned char* in;        // the planar block [C][n], rows back to back from a 16-byte boundary, MIX_SLACK readable bytes behind it
    const MonitorSend*   sends;     // [C]
    float*               out;       // [groups][2][stride]
    int                  n, C, stride, tiles;       // stride: n rounded up to a multiple of 8 (rows of `out` start on 32-byte boundaries)
};

constexpr int MIX_THREADS = 64;     // one wavefront: no barrier, and short blocks (441 / 480 / 512 samples) still spread over the chip
constexpr int MIX_UNROLL = 32;      // rows whose loads are in flight before the first of them is added: a group is two round trips

// samples a lane mixes: 16 bytes of fp32 or of a 16-bit format, 12 bytes of packed 24-bit samples (which one 16-byte load covers at
// any byte alignment)
__host__ __device__ constexpr int lane_samples(int fmt) { return fmt == FX_SAMPLE_F16 || fmt == FX_SAMPLE_S16 ? 8 : 4; }

// The PB (12 or 16) bytes of a row from byte `lane_off` (a multiple of 4) on.  Rows start at c * n * B bytes: any 2-byte boundary for
// the 16-bit formats and any byte for packed s24.  So the piece is read as the gather reads a clip: the aligned dwords around it with
// one global_load_dwordx4 (and a fifth dword where 16 bytes straddle five: RawPiece, fx_blocks.hip.h), shifted into place with v_alignbyte_b32
// once the row's turn in the sum has come (shifted_piece; shifting at the load would wait for it).  The shift is the row's, the same in
// every lane, and 0 for fp32.  A lane's piece may run past its row's end into the next row, and the last row's into the MIX_SLACK
// bytes that follow the block (fx_context.h, monitor_launch): those samples are not stored.
template <int B> __device__ __forceinline__ unsigned row_shift(long long row_off) { return B == 4 ? 0u : (unsigned) row_off & 3u; }
template <int B, int PB> __device__ __forceinline__ RawPiece load_piece(const unsigned char* in, long long row_off, long long lane_off)
{
    const unsigned sh = row_shift<B>(row_off);
    return load_raw_piece(in + (row_off - sh) + lane_off, PB == 16 ? sh : 0u);
}
// a lane reads at most the 20 bytes from the dword boundary below its piece, and its piece starts inside the block
constexpr int MIX_SLACK = 32;
static_assert(MIX_SLACK >= 20, "room behind the block for the last row's last piece");

// Workgroup (one wavefront) w mixes samples [tile * 64 * S, +64 * S) of group w / tiles: lane l holds the S samples from i0 on of both
// output channels and walks the group's tracks whose send is on, in ascending order.  The group's 64 sends arrive with ONE load, a row
// per lane; a ballot of `on` is the wave-uniform list of the tracks to add, walked lowest bit first, and a track's gains come out of
// its lane into scalar registers (v_readlane_b32).  (A scalar load per track was tried first: 64 dependent trips to the scalar cache
// a workgroup.)  So an off track is not even read, let alone added as 0 * x: what it carries never reaches the output.  The adds
// are one chain per output sample, the loads are not: the rows of the next MIX_UNROLL tracks are requested, unconditionally and
// back to back, before the first of them is added; a batch with fewer tracks left reads its first row again and a uniform branch
// skips the adds.  Lanes past the row's end read the row's start and store nothing.
template <int FMT>
__global__ void __launch_bounds__(MIX_THREADS)
fx_monitor_mix_kernel(const MixParams p)
{
    constexpr int B = sample_bytes(FMT), S = lane_samples(FMT), PB = S * B;
    const int lane = (int) threadIdx.x;
    const int g = (int) (blockIdx.x / (unsigned) p.tiles), tile = (int) (blockIdx.x % (unsigned) p.tiles);
    const long long i0 = ((long long) tile * MIX_THREADS + lane) * S;
    const bool stores = i0 < p.n;
    const int c0 = g * FX_MONITOR_GROUP;
    const int count = p.C - c0 < FX_MONITOR_GROUP ? p.C - c0 : FX_MONITOR_GROUP;
    const long long row_bytes = (long long) p.n * B, lane_off = stores ? i0 * B : 0;
    MonitorSend mine = MonitorSend{0, 0.0f, 0.0f, 0};
    if (lane < count) mine = p.sends[c0 + lane];
    unsigned long long todo = __ballot(mine.on != 0);
    float left[S], right[S];
#pragma unroll
    for (int j = 0; j < S; j++) { left[j] = 0.0f; right[j] = 0.0f; }
    while (todo) {
        RawPiece piece[MIX_UNROLL];
        int track[MIX_UNROLL];
        int have = 0;
#pragma unroll
        for (int u = 0; u < MIX_UNROLL; u++) {
            track[u] = todo ? __builtin_ctzll(todo) : track[0];
            have += todo ? 1 : 0;
            todo &= todo - 1;
            piece[u] = load_piece<B, PB>(p.in, (long long) (c0 + track[u]) * row_bytes, lane_off);
        }
#pragma unroll
        for (int u = 0; u < MIX_UNROLL; u++) {
            if (u < have) {
                const float gl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.left), track[u]));
                const float gr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.right), track[u]));
                const uint4 raw = shifted_piece(piece[u], row_shift<B>((long long) (c0 + track[u]) * row_bytes));
                float x[S];
                if constexpr (S == 8) {
                    const f4 a = widen_four<FMT>(uint4{raw.x, raw.y, 0u, 0u}), b = widen_four<FMT>(uint4{raw.z, raw.w, 0u, 0u});
                    x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
                    x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
                } else {
                    const f4 a = widen_four<FMT>(raw);
                    x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
                }
#pragma unroll
                for (int j = 0; j < S; j++) {
                    left[j] = left[j] + gl * x[j];
                    right[j] = right[j] + gr * x[j];
                }
            }
        }
    }
    if (!stores) return;
    // (stride is a multiple of 8 >= n: a lane's S floats lie inside its row, on a 16-byte boundary, also where the row ends inside them)
    float* l = p.out + (size_t) g * 2 * (size_t) p.stride + i0;
    float* r = l + p.stride;
#pragma unroll
    for (int j = 0; j < S; j += 4) {
        *reinterpret_cast<float4*>(l + j) = float4{left[j], left[j + 1], left[j + 2], left[j + 3]};
        *reinterpret_cast<float4*>(r + j) = float4{right[j], right[j + 1], right[j + 2], right[j + 3]};
    }
}

constexpr int SUM_THREADS = 64;
constexpr int SUM_UNROLL = 32, SUM_REST = 8;

// out[e] = +0 + P[0][e] + P[1][e] + ..., in that order, for every element e of a group's two rows: a thread per element, the groups'
// reads coalesced, SUM_UNROLL of them requested back to back before the first is added; what is left goes SUM_REST at a time (a
// batch with fewer groups left reads its first row again; a uniform branch skips the adds).  A second launch on the stream, not a
// "last workgroup" counter: it is ordered for free.
__global__ void __launch_bounds__(SUM_THREADS)
fx_monitor_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int groups, int n, int stride)
{
    const int elements = 2 * stride;
    const int e = (int) (blockIdx.x * SUM_THREADS + threadIdx.x);
    if (e >= elements || (e < stride ? e : e - stride) >= n) return;       // (the rows' padding holds nothing)
    const float* at = part + e;
    float acc = 0.0f;
    int g = 0;
    for (; g + SUM_UNROLL <= groups; g += SUM_UNROLL) {
        float v[SUM_UNROLL];
#pragma unroll
        for (int u = 0; u < SUM_UNROLL; u++) v[u] = at[(size_t) (g + u) * (size_t) elements];
#pragma unroll
        for (int u = 0; u < SUM_UNROLL; u++) acc = acc + v[u];
    }
    for (; g < groups; g += SUM_REST) {
        float v[SUM_REST];
#pragma unroll
        for (int u = 0; u < SUM_REST; u++) v[u] = at[(size_t) (g + u < groups ? g + u : g) * (size_t) elements];
#pragma unroll
        for (int u = 0; u < SUM_REST; u++)
            if (g + u < groups) acc = acc + v[u];
    }
    out[e] = acc;
}

} // namespace

// (outside the unnamed namespace: tools/kernel_resources.py names the kernel in DESIGN.md's table of registers)
// A track that listens, and the output row it hears (0 left, 1 right).  The device's list is COMPACT: a context of 65 536 tracks with two
// listeners -- the reference's own case -- reads 16 bytes of it, not the 1 MB of its send table.
struct ListenEntry { int track, output; };

struct ListenParams {
    const ListenEntry* list;    // [count]
    const float*       mix;     // [2][stride]: the tick's mix, complete on the stream
    float*             planar;  // the tick's planar fp32 block [C][n]
    int                n, stride, tiles, count;
};

constexpr int LISTEN_THREADS = 64;      // one wavefront, lanes along the samples
constexpr int LISTEN_QUADS = 2;         // 16-byte pieces a lane moves, both loads in flight before the first store
constexpr int LISTEN_TILE = LISTEN_THREADS * 4 * LISTEN_QUADS;     // 512 samples: a 441- / 480- / 512-sample tick is one wavefront a listener

// Workgroup (one wavefront) w copies samples [tile * 512, +512) of output row list[w / tiles].output over row list[w / tiles].track of
// the planar block, bit for bit (the words move as unsigned: a NaN keeps its payload).  Piece j of lane l is the four samples from
// tile * 512 + j * 256 + 4 l on: a wavefront's loads and stores are 1 KB of consecutive addresses.  The source row starts on a 32-byte
// boundary (stride is a multiple of 8), so a piece is one aligned 16-byte load, also where the row ends inside it: the padding up to
// `stride` is allocated, read and not stored.  The destination row starts at track * n floats -- a dword boundary and no more when
// n % 4 != 0 -- so a piece is stored as four dwords from a dword boundary (dwords4), and the n % 4 samples of the tail one dword at a
// time: nothing is stored past the row's end, where the next track's row begins.  Every offset is 64-bit (65 536 tracks x 8193 samples
// x 4 bytes pass 2^31).  The entry is the same in every lane: it arrives through the scalar cache.
__global__ void __launch_bounds__(LISTEN_THREADS)
fx_monitor_listen_kernel(const ListenParams p)
{
    const unsigned w = blockIdx.x / (unsigned) p.tiles, tile = blockIdx.x % (unsigned) p.tiles;
    const ListenEntry e = p.list[w];
    const unsigned* src = reinterpret_cast<const unsigned*>(p.mix) + (size_t) e.output * (size_t) p.stride;
    unsigned* dst = reinterpret_cast<unsigned*>(p.planar) + (size_t) e.track * (size_t) p.n;
    const long long i0 = (long long) tile * LISTEN_TILE + (long long) threadIdx.x * 4;
    uint4 v[LISTEN_QUADS];
#pragma unroll
    for (int j = 0; j < LISTEN_QUADS; j++) {
        const long long i = i0 + (long long) j * (LISTEN_THREADS * 4);
        v[j] = i < p.n ? *reinterpret_cast<const uint4*>(src + i) : uint4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < LISTEN_QUADS; j++) {
        const long long i = i0 + (long long) j * (LISTEN_THREADS * 4);
        if (i + 4 <= p.n) {
            *(GlobalDwords4Out) (dst + i) = dwords4{v[j].x, v[j].y, v[j].z, v[j].w};
        } else if (i < p.n) {
            const int left = (int) (p.n - i);       // 1 .. 3
            dst[i] = v[j].x;
            if (left > 1) dst[i + 1] = v[j].y;
            if (left > 2) dst[i + 2] = v[j].z;
        }
    }
}

namespace {

hipError_t launch_listen_kernel(ListenParams p, hipStream_t stream)
{
    if (p.n <= 0 || p.count <= 0) return hipSuccess;
    p.tiles = (p.n + LISTEN_TILE - 1) / LISTEN_TILE;
    const long long wgs = (long long) p.count * p.tiles;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fx_monitor_listen_kernel, dim3((unsigned) wgs), dim3(LISTEN_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_monitor_kernels(MixParams p, float* part, float* out, int sample_format, hipStream_t stream)
{
    if (p.n <= 0 || p.C <= 0) return hipSuccess;
    const int groups = (p.C + FX_MONITOR_GROUP - 1) / FX_MONITOR_GROUP;
    const int per_tile = MIX_THREADS * lane_samples(sample_format);
    p.tiles = (p.n + per_tile - 1) / per_tile;
    p.out = groups == 1 ? out : part;
    const long long wgs = (long long) groups * p.tiles;
    const long long elements = 2ll * p.stride;
    if (wgs > 0x7fffffffll || elements > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned) wgs), block(MIX_THREADS);
    // (not FX_FORMAT: an unknown format is refused here, and the code object keeps its kernels in this order)
    switch (sample_format) {
        case FX_SAMPLE_F32: hipLaunchKernelGGL(fx_monitor_mix_kernel<FX_SAMPLE_F32>, grid, block, 0, stream, p); break;
        case FX_SAMPLE_F16: hipLaunchKernelGGL(fx_monitor_mix_kernel<FX_SAMPLE_F16>, grid, block, 0, stream, p); break;
        case FX_SAMPLE_S16: hipLaunchKernelGGL(fx_monitor_mix_kernel<FX_SAMPLE_S16>, grid, block, 0, stream, p); break;
        case FX_SAMPLE_S24: hipLaunchKernelGGL(fx_monitor_mix_kernel<FX_SAMPLE_S24>, grid, block, 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || groups == 1) return e;
    hipLaunchKernelGGL(fx_monitor_sum_kernel, dim3((unsigned) ((elements + SUM_THREADS - 1) / SUM_THREADS)), dim3(SUM_THREADS), 0, stream,
                       part, out, groups, p.n, p.stride);
    return hipGetLastError();
}

} // namespace
} // namespace fxk

struct fx_monitor {
    fxk::MonitorSend*             d_sends = nullptr;    // [C]
    std::vector<fxk::MonitorSend> sends;                // the same on the host: only this unit's calls change it
    float*                        d_part = nullptr;     // [groups][2][stride], contexts of more than one group
    float*                        d_out = nullptr;      // [2][stride]: the last tick's mix
    size_t                        part_cap = 0, out_cap = 0;    // bytes
    int                           n = 0, stride = 0;    // the last tick's samples and its rows' stride; n == 0: no tick yet
    // the tracks whose listen (sends[t].listen) is not FX_LISTEN_SELF, ascending: on the host, and the same in device memory, [C]
    // entries allocated with the monitor (a setter never reallocates under ticks in flight) and copied in stream order by the
    // setter.  A tick's launch takes the host's count as an argument: list and count agree at every point of the stream.
    fxk::ListenEntry*             d_listen = nullptr;
    std::vector<fxk::ListenEntry> listeners;
};

namespace {

void monitor_release(fx_context* c)
{
    fx_monitor* m = c->monitor;
    if (!m) return;
    fx_free_device({m->d_sends, m->d_part, m->d_out, m->d_listen});
    delete m;
    c->monitor = nullptr;
}

int stride_of(int num_samples) { return (int) (((long long) num_samples + 7) & ~7ll); }

// room for a tick of num_samples, before fx_push_sources launches anything.  A tick that needs more room than the last one replaces
// the last mix anyway; if the larger buffer cannot be had, the old one is gone with it (fx_grow) and the monitor holds no tick.
fx_status monitor_prepare(fx_context* c, int num_samples, int sample_format)
{
    fx_monitor* m = c->monitor;
    if (!m || num_samples <= 0) return FX_OK;
    // the mix is fp32 and a listener's row becomes the mix (the rule of rated clips, fx_push_sources)
    if (!m->listeners.empty() && sample_format != FX_SAMPLE_F32)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d listens to the monitor's output, which is fp32: this call is in sample format %d", m->listeners[0].track, sample_format);
    const size_t row = (size_t) stride_of(num_samples) * sizeof(float);
    const int groups = (c->C + FX_MONITOR_GROUP - 1) / FX_MONITOR_GROUP;
    fx_status st = FX_OK;
    if (2 * row > m->out_cap) {
        m->n = 0;
        st = fx_grow(&m->d_out, &m->out_cap, 2 * row);
    }
    if (st == FX_OK && groups > 1) st = fx_grow(&m->d_part, &m->part_cap, (size_t) groups * 2 * row);
    return st;
}

// the tick's planar block is complete on the stream (fx_context.h states what `planar` must be)
fx_status monitor_launch(fx_context* c, void* planar, int num_samples, int sample_format)
{
    fx_monitor* m = c->monitor;
    if (!m || num_samples <= 0) return FX_OK;
    fxk::MixParams p;
    p.in = static_cast<const unsigned char*>(planar);
    p.sends = m->d_sends;
    p.out = nullptr;
    p.n = num_samples;
    p.C = c->C;
    p.stride = stride_of(num_samples);
    p.tiles = 0;
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_MONITOR, 0)) r->T = num_samples;
    HIP_TRY(fxk::launch_monitor_kernels(p, m->d_part, m->d_out, sample_format, c->stream));
    m->n = num_samples;
    m->stride = p.stride;
    if (m->listeners.empty()) return FX_OK;
    // the mix is complete on the stream: the listeners' rows become it before the analysers read them (fp32: monitor_prepare)
    const fxk::ListenParams lp{m->d_listen, m->d_out, static_cast<float*>(planar), num_samples, p.stride, 0, (int) m->listeners.size()};
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_LISTEN, 0)) r->T = num_samples;
    HIP_TRY(fxk::launch_listen_kernel(lp, c->stream));
    return FX_OK;
}

} // namespace

extern "C" {

fx_status fx_enable_monitor(fx_context* c, int enable)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!enable && !c->monitor) return FX_OK;
    // (fx_destroy_clips' rule for loaded clips: what a track still uses is not freed under it)
    if (!enable && !c->monitor->listeners.empty())
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d listens to the monitor's output (fx_set_channel_listen)", c->monitor->listeners[0].track);
    { const fx_status st = fx_require_device(); if (st != FX_OK) return st; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));        // ticks in flight write the monitor that is about to go; copies in flight read it
    if (!enable) {
        monitor_release(c);
        c->monitor_prepare = nullptr;
        c->monitor_launch = nullptr;
        c->monitor_release = nullptr;
        return FX_OK;
    }
    if (c->monitor) return FX_OK;                    // (the sends stay)
    fx_monitor* m = new (std::nothrow) fx_monitor();
    if (!m) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    try {
        m->sends.assign((size_t) c->C, fxk::MonitorSend{0, 1.0f, 1.0f, FX_LISTEN_SELF});
    } catch (const std::bad_alloc&) {
        delete m;
        return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    const size_t bytes = m->sends.size() * sizeof(fxk::MonitorSend);
    void *q = nullptr, *ql = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess) e = hipMemcpy(q, m->sends.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&ql, (size_t) c->C * sizeof(fxk::ListenEntry));
    if (e != hipSuccess) {
        if (q) (void) hipFree(q);
        if (ql) (void) hipFree(ql);
        delete m;
        return fx_fail(fx_hip_status(e), "allocating the send table failed: %s", hipGetErrorString(e));
    }
    m->d_sends = static_cast<fxk::MonitorSend*>(q);
    m->d_listen = static_cast<fxk::ListenEntry*>(ql);
    c->monitor = m;
    c->monitor_prepare = monitor_prepare;
    c->monitor_launch = monitor_launch;
    c->monitor_release = monitor_release;
    return FX_OK;
}

fx_status fx_set_channel_monitor(fx_context* c, const int* channels, int num_channels, const int* on, const float* left, const float* right)
{
    fx_status st = fx_check_channel_list(c, channels, num_channels);
    if (st != FX_OK) return st;
    // the call's own values, then the range of its entries (fx_set_channel_clips' order)
    for (int i = 0; i < num_channels; i++) {
        if (left && !std::isfinite(left[i])) return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: the left gain %g is not a finite number", i, left[i]);
        if (right && !std::isfinite(right[i])) return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: the right gain %g is not a finite number", i, right[i]);
    }
    if ((st = fx_check_channel_entries(c, channels, num_channels)) != FX_OK) return st;
    fx_monitor* m = c->monitor;
    if (!m) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the monitor is not enabled on this context (fx_enable_monitor)");
    if (num_channels == 0) return FX_OK;
    HIP_TRY(hipSetDevice(c->device));
    // in list order, so the last entry of a track wins; the touched stretch of the table follows the ticks enqueued so far.  (The
    // rows are pageable memory: the copy has left them when the call returns.)  A failed copy puts the old rows back.
    int lo = c->C, hi = -1;
    for (int i = 0; i < num_channels; i++) { lo = channels[i] < lo ? channels[i] : lo; hi = channels[i] > hi ? channels[i] : hi; }
    std::vector<fxk::MonitorSend> before;
    try {
        before.assign(m->sends.begin() + lo, m->sends.begin() + hi + 1);
    } catch (const std::bad_alloc&) {
        return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    for (int i = 0; i < num_channels; i++) {
        fxk::MonitorSend& s = m->sends[(size_t) channels[i]];
        s.on = !on || on[i] ? 1 : 0;
        if (left) s.left = left[i];
        if (right) s.right = right[i];
    }
    const hipError_t e = hipMemcpyAsync(m->d_sends + lo, m->sends.data() + lo, (size_t) (hi - lo + 1) * sizeof(fxk::MonitorSend), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        for (int t = lo; t <= hi; t++) m->sends[(size_t) t] = before[(size_t) (t - lo)];
        return fx_fail(FX_ERR_HIP, "copying the sends failed: %s", hipGetErrorString(e));
    }
    return FX_OK;
}

fx_status fx_get_channel_monitor(fx_context* c, int* on, float* left, float* right)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    const fx_monitor* m = c->monitor;
    if (!m) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the monitor is not enabled on this context (fx_enable_monitor)");
    for (int t = 0; t < c->C; t++) {
        const fxk::MonitorSend& s = m->sends[(size_t) t];
        if (on) on[t] = s.on;
        if (left) left[t] = s.left;
        if (right) right[t] = s.right;
    }
    return FX_OK;
}

fx_status fx_set_channel_listen(fx_context* c, const int* channels, int num_channels, const int* listen)
{
    fx_status st = fx_check_channel_list(c, channels, num_channels);
    if (st != FX_OK) return st;
    if (num_channels > 0 && !listen) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null listen list with %d entries", num_channels);
    // the call's own values, then the range of its entries (fx_set_channel_monitor's order)
    for (int i = 0; i < num_channels; i++)
        if (listen[i] != FX_LISTEN_SELF && listen[i] != FX_LISTEN_LEFT && listen[i] != FX_LISTEN_RIGHT)
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: unknown listen %d", i, listen[i]);
    if ((st = fx_check_channel_entries(c, channels, num_channels)) != FX_OK) return st;
    fx_monitor* m = c->monitor;
    if (!m) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the monitor is not enabled on this context (fx_enable_monitor)");
    if (num_channels == 0) return FX_OK;
    HIP_TRY(hipSetDevice(c->device));
    // the column as it will be (in list order: the last entry of a track wins) and its compact list, made beside the ones in force:
    // a failed call changes nothing.  The copy reads the monitor's own list, which lives as long as the monitor.
    std::vector<int> column;
    std::vector<fxk::ListenEntry> next;
    try {
        column.resize((size_t) c->C);
        for (int t = 0; t < c->C; t++) column[(size_t) t] = m->sends[(size_t) t].listen;
        for (int i = 0; i < num_channels; i++) column[(size_t) channels[i]] = listen[i];
        for (int t = 0; t < c->C; t++)
            if (column[(size_t) t] != FX_LISTEN_SELF) next.push_back(fxk::ListenEntry{t, column[(size_t) t] - FX_LISTEN_LEFT});
    } catch (const std::bad_alloc&) {
        return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    m->listeners.swap(next);
    if (!m->listeners.empty()) {
        const hipError_t e = hipMemcpyAsync(m->d_listen, m->listeners.data(), m->listeners.size() * sizeof(fxk::ListenEntry), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            m->listeners.swap(next);
            return fx_fail(FX_ERR_HIP, "copying the listeners failed: %s", hipGetErrorString(e));
        }
    }
    for (int t = 0; t < c->C; t++) m->sends[(size_t) t].listen = column[(size_t) t];
    // toggleCollectInput clears the collector whichever way it is switched (ref AudioDataCollector.h:119)
    return fx_clear_pending_channels(c, channels, num_channels);
}

fx_status fx_get_channel_listen(fx_context* c, int* listen)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!listen) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null output pointer");
    const fx_monitor* m = c->monitor;
    if (!m) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the monitor is not enabled on this context (fx_enable_monitor)");
    for (int t = 0; t < c->C; t++) listen[t] = m->sends[(size_t) t].listen;
    return FX_OK;
}

fx_status fx_get_monitor(fx_context* c, float* out, int capacity, int* num_samples, int mem_kind)
{
    if (num_samples) *num_samples = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null output pointer");
    { const fx_status st = fx_check_memory_kind(mem_kind); if (st != FX_OK) return st; }
    const fx_monitor* m = c->monitor;
    if (!m) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the monitor is not enabled on this context (fx_enable_monitor)");
    if (num_samples) *num_samples = m->n;            // (also where the room is refused: a host learns what to bring)
    if (capacity < m->n) return fx_fail(FX_ERR_INVALID_ARGUMENT, "capacity %d: the last tick's mix holds %d samples per output channel", capacity, m->n);
    if (mem_kind == FX_MEM_DEVICE && reinterpret_cast<uintptr_t>(out) % 4 != 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "device output must be 4-byte aligned");
    if (m->n == 0) return FX_OK;
    HIP_TRY(hipSetDevice(c->device));
    const hipMemcpyKind kind = mem_kind == FX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t bytes = (size_t) m->n * sizeof(float);
    HIP_TRY(hipMemcpyAsync(out, m->d_out, bytes, kind, c->stream));
    HIP_TRY(hipMemcpyAsync(out + capacity, m->d_out + m->stride, bytes, kind, c->stream));
    if (mem_kind == FX_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fx_check_device_error(c);
    }
    return FX_OK;
}

} // extern "C"
