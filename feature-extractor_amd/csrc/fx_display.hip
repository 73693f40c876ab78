// fx_display.hip -- audio display levels: every track's scrolling waveform, made on the GPU (include/fx.h, fx_enable_display /
// fx_set_display_samples_per_block / fx_clear_display_channels / fx_get_display).
//
// ref AnalyserTrackController.h:74-78 (setBufferToDrawUpdatedCallback on the harmonic collector), AudioDataCollector.h:88-91 (the
// callback gets every gained hop the collector hands out), AnalyserTrack.h:148-157 (updateBufferToPush pushes the hop into the
// AudioVisualiserComponent), AnalyserTrack.h:27-29 (setSamplesPerBlock (256), setBufferSize (1024)), AnalyserTrackController.h:154-158
// (setSamplesPerBlock with the device's block size), :105,114 (clearAudioDisplayData).  The component (JUCE 4.2.3
// AudioVisualiserComponent::ChannelInfo) keeps a ring levels[L] of (lo, hi) pairs, a running pair `value`, `sub` and `next`, and runs
// for every sample x
//     if (--sub <= 0) { next %= L; levels[next++] = value; sub = samplesPerBlock; value = (x, x); }
//     else { lo' = lo < x ? lo : x;  t = x < hi ? hi : x;  hi' = lo' < t ? t : lo';  value = (lo', hi'); }
// so a block is published when the first sample of the next one arrives, ties take the newer sample (the sign of a zero is the latest
// one's), and a NaN sample makes both ends NaN until the next sample replaces both.
//
// The parallel form.  A run of samples is summarised by (lo, hi, "holds a NaN"); combine(L, R) is R when R holds a NaN, otherwise
// (L.lo < R.lo ? L.lo : R.lo, R.hi < L.hi ? L.hi : R.hi): associative, and folding a run's single samples (x, x, isnan(x)) left to
// right behind the carried `value` gives the sequential result bit for bit (tests/display_model.py, tests/test_display_cpu.py).  From a
// track's `sub` and the call's S samples the call's publications are fixed before any sample is read: the first at sample
// f = max(sub - 1, 0), then one every samplesPerBlock; P of them.  Publication k stores the fold of the samples since publication k - 1
// (k = 0: the carried value and the samples before f) at ring slot (next mod L + k) mod L, and lands iff k >= P - L: decided from
// indices, no store races another.
//
// fx_display_kernel: ONE launch per analysis call.  The samples between two publications are a display block; a wavefront takes whole
// display blocks of one track -- DISPLAY_CHUNK samples' worth, always cut AT a publication, so no float crosses wavefronts -- and
// walks them in tiles of 64 lanes x 8 consecutive samples: a lane folds its eight samples (a publication inside them starts a new
// segment), a segmented Kogge-Stone scan over the lanes gives every lane the fold of what precedes it in its segment, and the lane walks
// its samples once more, storing (lo, hi) wherever a display block ends.  No atomics; the order is the samples' own.  Each sample is
// read once, where the analysis reads it (hops, whole frames' second halves, or [pending | block]), widened by the same widen_one and
// scaled by the track's gain as the load stage does.  The wavefront that holds the call's last sample writes the track's new state to
// the OTHER of two state tables (the track's other wavefronts are still reading the old one).
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: fx_enable_display installs the context's three hooks (fx_context.h).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <new>

#include "fx_kernels.h"
#include "fx_context.h"

#pragma clang fp contract(off)

namespace fxk {

#include "fx_wave.hip.h"          // lane_get
#include "fx_samples.hip.h"
#include "fx_blocks.hip.h"        // BlockStream

namespace {

constexpr int DISPLAY_THREADS = 256, DISPLAY_WAVES = DISPLAY_THREADS / 64;
constexpr int DISPLAY_PER_LANE = 8;                             // consecutive samples a lane folds per tile (16: 82 VGPRs, a live call of
                                                                // 8192 tracks no longer fits the chip in one round -- measured slower)
constexpr int DISPLAY_TILE = 64 * DISPLAY_PER_LANE;
constexpr int DISPLAY_CHUNK = 8 * DISPLAY_TILE;                 // samples a wavefront aims to take (whole display blocks)
constexpr int MAX_LENGTH = 4096, MAX_SAMPLES_PER_BLOCK = 65536;
constexpr long long MAX_CALL_SAMPLES = 0x7fffffffll - 2ll * MAX_SAMPLES_PER_BLOCK - DISPLAY_CHUNK;    // sample indices stay ints

// A track's component between calls (ChannelInfo's value, subSample, nextSample); levels live in their own table.
struct DisplayState {
    float lo, hi;
    int   sub, next;
};
static_assert(sizeof(DisplayState) == 16, "read and written as one 16-byte piece");

struct DisplayParams {
    fx_tap_source       src;            // where the call's samples are, as the analysis reads them
    const DisplayState* state_in;       // [C]
    DisplayState*       state_out;      // [C], the other table
    float2*             levels;         // [C][L]
    const ChannelSettings* chan;        // per-track settings or null: hops are shown with the track's own gain
    float               gain;
    int                 C, L, spb;
    int                 S;              // samples per track in this call: T * N/2
    int                 half_shift;     // log2(N/2): whole frames are read at their second halves
    int                 per_chunk;      // display blocks a wavefront takes
    int                 chunks;         // wavefronts per track
};

// num / den for 0 <= num < 2^22 and den >= 1, with inv = 1.0f / den: the float quotient is off by less than one, the remainder says
// which way.  (An integer division is ~40 instructions on this hardware; the indices below need one per lane and tile.)
__device__ __forceinline__ int small_div(int num, int den, float inv)
{
    int q = (int) ((float) num * inv);
    const int r = num - q * den;
    if (r < 0) q--;
    if (r >= den) q++;
    return q;
}
__device__ __forceinline__ int small_mod(int num, int den, float inv) { return num - small_div(num, den, inv) * den; }

enum { SEG_NAN = 1, SEG_HEAD = 2, SEG_FULL = 4 };
struct Seg { float lo, hi; int f; };

// the fold's step with segment heads and empty runs: what lies right of the last head, as combine() would fold it
__device__ __forceinline__ Seg seg_combine(const Seg& l, const Seg& r)
{
    Seg o;
    const bool keep_l = !(r.f & SEG_FULL);
    const bool take_r = !(l.f & SEG_FULL) || (r.f & (SEG_HEAD | SEG_NAN));
    const float lo = l.lo < r.lo ? l.lo : r.lo;
    const float hi = r.hi < l.hi ? l.hi : r.hi;
    o.lo = keep_l ? l.lo : (take_r ? r.lo : lo);
    o.hi = keep_l ? l.hi : (take_r ? r.hi : hi);
    // (the NaN mark is the trailing segment's)
    o.f = (r.f & SEG_HEAD) ? (r.f | (l.f & SEG_FULL)) : (l.f | r.f);
    return o;
}
__device__ __forceinline__ Seg seg_shfl_up(const Seg& s, int d)
{
    return Seg{__shfl_up(s.lo, d, 64), __shfl_up(s.hi, d, 64), __shfl_up(s.f, d, 64)};
}

// Where fp32 samples i .. i + DISPLAY_PER_LANE - 1 of the call lie in one piece of memory, or null: they straddle the pending samples
// and the block, or two frames.  Two 16-byte loads per lane instead of eight 4-byte ones (the texture path moves whole lines).
__device__ __forceinline__ const float* display_run(const DisplayParams& p, const unsigned char* row, const unsigned char* carry_row, int i)
{
    const long long d = (long long) i * 4;
    if (p.src.carry) {
        if (d >= p.src.carry_bytes) return reinterpret_cast<const float*>(row + (d - p.src.carry_bytes));
        if (d + DISPLAY_PER_LANE * 4 <= p.src.carry_bytes) return reinterpret_cast<const float*>(carry_row + d);
        return nullptr;
    }
    if (p.src.hop_mode) return reinterpret_cast<const float*>(row + d);
    const long long t = i >> p.half_shift, h = 1ll << p.half_shift, in_frame = i & (h - 1);
    if (in_frame + DISPLAY_PER_LANE > h) return nullptr;
    return reinterpret_cast<const float*>(row) + (t * 2 * h + h + in_frame);
}

// sample i of channel row `row` of the call, widened as the analysis kernels widen it (no gain yet)
template <int FMT> __device__ __forceinline__ float display_sample(const DisplayParams& p, const unsigned char* row, const unsigned char* carry_row, int i)
{
    constexpr int B = sample_bytes(FMT);
    if (p.src.carry) {
        const BlockStream bs = {carry_row, row, p.src.carry_bytes, p.src.in_row_bytes};
        return widen_one<FMT>(stream_sample<B>(bs, i));
    }
    long long at = i;
    if (!p.src.hop_mode) {
        // fx_process_frames: frame t's second half (the hop the overlapper would have been handed)
        const long long t = i >> p.half_shift, h = 1ll << p.half_shift;
        at = t * 2 * h + h + (i & (h - 1));
    }
    return widen_one<FMT>(row + at * B);
}

template <int FMT> __device__ __forceinline__ void display_wave(const DisplayParams& p, int c, int chunk, int lane)
{
    const DisplayState s0 = p.state_in[c];
    const int S = p.S, spb = p.spb, L = p.L;
    const int f = s0.sub > 1 ? s0.sub - 1 : 0;                 // the sample whose arrival publishes first
    const int P = f < S ? 1 + (S - 1 - f) / spb : 0;           // publications of this call
    const int n0 = s0.next % L;
    const int land_from = P - L;                               // publication k is kept iff k >= land_from
    float2* levels = p.levels + (long long) c * L;

    // display block k of the call starts at sample start(k): 0, then the publications f, f + spb, ...
    auto start = [&](long long k) -> int {
        const long long at = k <= 0 ? 0 : (long long) f + (k - 1) * spb;
        return at < S ? (int) at : S;
    };
    const int a = start((long long) chunk * p.per_chunk), b = start((long long) (chunk + 1) * p.per_chunk);
    // sub == 0 or 1: the call's first sample publishes the carried value as it stands
    if (chunk == 0 && lane == 0 && f == 0 && land_from <= 0) levels[n0] = float2{s0.lo, s0.hi};
    if (a >= b) return;

    const float gain = channel_gain(p.chan, p.gain, c);
    const bool scale = p.src.hop_mode && gain != 1.0f;         // ref AudioDataCollector.h:88, as the load stage applies it
    const unsigned char* row = static_cast<const unsigned char*>(p.src.in) + (long long) c * p.src.in_row_bytes;
    const unsigned char* carry_row = p.src.carry ? p.src.carry + (long long) c * p.src.carry_row_bytes : nullptr;

    // the run before sample a: the carried value for the track's first wavefront, nothing for the others (a is a publication)
    Seg carry = {0.0f, 0.0f, 0};
    if (chunk == 0) carry = Seg{s0.lo, s0.hi, SEG_FULL | ((s0.lo != s0.lo) ? SEG_NAN : 0)};

    // wave-uniform, kept from tile to tile: the first publication at or after the tile's first sample -- its distance d_t, its index
    // k_t, its ring slot.  Sample a is sample 0 (the first publication is f away) or publication chunk * per_chunk - 1 itself.
    const float inv_spb = 1.0f / (float) spb, inv_L = 1.0f / (float) L;
    int d_t = chunk == 0 ? f : 0, k_t = chunk == 0 ? 0 : chunk * p.per_chunk - 1;
    int slot_t = (int) (((unsigned) n0 + (unsigned) k_t) % (unsigned) L);
    for (int tile = a; tile < b; tile += DISPLAY_TILE) {
        // the lane's own: first publication at or after ITS first sample
        const int o = lane * DISPLAY_PER_LANE, i0 = tile + o;
        const int j = o > d_t ? small_div(o - d_t + spb - 1, spb, inv_spb) : 0;
        const int d0 = d_t + j * spb - o;                                      // >= 0
        const int k0 = k_t + j;

        float x[DISPLAY_PER_LANE];
        const bool whole = i0 + DISPLAY_PER_LANE <= b;                         // all of the lane's samples are the wavefront's
        const float* run = nullptr;
        if constexpr (FMT == FX_SAMPLE_F32) { if (whole) run = display_run(p, row, carry_row, i0); }
        if (run) {
#pragma unroll
            for (int q = 0; q < DISPLAY_PER_LANE / 4; q++) {
                const dwords4 v = reinterpret_cast<const dwords4*>(run)[q];        // (a run starts on a dword boundary and no more)
                x[4 * q] = __uint_as_float(v[0]); x[4 * q + 1] = __uint_as_float(v[1]); x[4 * q + 2] = __uint_as_float(v[2]); x[4 * q + 3] = __uint_as_float(v[3]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < DISPLAY_PER_LANE; e++) {
                x[e] = 0.0f;
                if (i0 + e < b) x[e] = display_sample<FMT>(p, row, carry_row, i0 + e);
            }
        }
        if (scale) {
#pragma unroll
            for (int e = 0; e < DISPLAY_PER_LANE; e++) x[e] *= gain;
        }
        // the lane's summary
        Seg mine = {0.0f, 0.0f, 0};
        if (whole && d0 >= DISPLAY_PER_LANE) {
            // no publication among them: the component's own fold (a NaN end loses every comparison, so the next sample replaces it)
            float lo = x[0], hi = x[0];
            bool nan = x[0] != x[0];
#pragma unroll
            for (int e = 1; e < DISPLAY_PER_LANE; e++) {
                lo = lo < x[e] ? lo : x[e];
                hi = x[e] < hi ? hi : x[e];
                nan |= x[e] != x[e];
            }
            mine = Seg{lo, hi, SEG_FULL | (nan ? SEG_NAN : 0)};
        } else {
            int d = d0;
#pragma unroll
            for (int e = 0; e < DISPLAY_PER_LANE; e++) {
                int fl = i0 + e < b ? (SEG_FULL | ((x[e] != x[e]) ? SEG_NAN : 0)) : 0;        // (past the wavefront's samples: an empty run)
                if (e == d) { fl |= fl ? SEG_HEAD : 0; d += spb; }
                mine = seg_combine(mine, Seg{x[e], x[e], fl});
            }
        }
        if (lane == 0) mine = seg_combine(carry, mine);
        // inclusive segmented scan over the lanes
        Seg incl = mine;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const Seg up = seg_shfl_up(incl, s);
            if (lane >= s) incl = seg_combine(up, incl);
        }
        Seg acc = seg_shfl_up(incl, 1);
        if (lane == 0) acc = carry;
        // once more over the samples of a lane in which a display block ends, with what precedes them: the block is published
        if (d0 <= DISPLAY_PER_LANE) {
            int d = d0, k = k0;
            int slot = small_mod(slot_t + j, L, inv_L);
#pragma unroll
            for (int e = 0; e < DISPLAY_PER_LANE; e++) {
                const int i = i0 + e;
                int fl = i < b ? (SEG_FULL | ((x[e] != x[e]) ? SEG_NAN : 0)) : 0;
                if (e == d) { fl |= fl ? SEG_HEAD : 0; d += spb; k++; slot = slot + 1 == L ? 0 : slot + 1; }
                acc = seg_combine(acc, Seg{x[e], x[e], fl});
                // (k, slot: the NEXT publication's, at sample i0 + d)
                if (i < b && e + 1 == d && i + 1 < S && k >= land_from) levels[slot] = float2{acc.lo, acc.hi};
            }
        }
        carry = Seg{lane_get(incl.lo, 63), lane_get(incl.hi, 63), lane_get(incl.f, 63)};
        d_t -= DISPLAY_TILE;
        if (d_t < 0) {
            const int steps = small_div(spb - 1 - d_t, spb, inv_spb);          // publications inside the tile behind the first
            d_t += steps * spb;
            k_t += steps;
            slot_t = small_mod(slot_t + steps, L, inv_L);
        }
    }
    // the wavefront with the call's last sample leaves the track's state
    if (b == S && lane == 0) {
        DisplayState s1;
        s1.lo = carry.lo;
        s1.hi = carry.hi;
        if (P == 0) { s1.sub = s0.sub - S; s1.next = s0.next; }
        else {
            const long long last = (long long) f + (long long) (P - 1) * spb;
            s1.sub = (int) (spb - ((long long) S - 1 - last));
            s1.next = (int) (((unsigned) n0 + (unsigned) (P - 1)) % (unsigned) L) + 1;
        }
        p.state_out[c] = s1;
    }
}

} // namespace

// (named in fxk itself, like the analysis kernels: tools/kernel_resources.py finds it by its prefix)
__global__ void __launch_bounds__(DISPLAY_THREADS) fx_display_kernel(const DisplayParams p)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const unsigned w = blockIdx.x * DISPLAY_WAVES + wave;        // (the host launches fewer than 2^31 wavefronts)
    const unsigned track = w / (unsigned) p.chunks;
    if (track >= (unsigned) p.C) return;
    const int c = (int) track, chunk = (int) (w - track * (unsigned) p.chunks);
    FX_FORMAT(p.src.sample_format, display_wave<FMT>(p, c, chunk, lane));
}

// New components (keep_next 0: levels, value, sub and next zero) or clear() (keep_next 1: next stays) for the listed tracks, or for
// all of them (list null, n = C).  A wavefront per 64 ring entries; the first of a track takes its state.
struct DisplayResetParams {
    const int*    list;
    DisplayState* state;        // [C], the table the next call reads
    float2*       levels;       // [C][L]
    int           n, C, L, keep_next;
};
__global__ void __launch_bounds__(DISPLAY_THREADS) fx_display_reset_kernel(const DisplayResetParams p)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int row_waves = (p.L + 63) / 64;
    const long long w = (long long) blockIdx.x * DISPLAY_WAVES + wave;
    const long long entry = w / row_waves;
    if (entry >= p.n) return;
    const int c = p.list ? p.list[entry] : (int) entry;
    if ((unsigned) c >= (unsigned) p.C) return;                       // (the host has checked every entry)
    const int first = (int) (w - entry * row_waves) * 64, at = first + lane;
    if (at < p.L) p.levels[(long long) c * p.L + at] = float2{0.0f, 0.0f};
    if (first == 0 && lane == 0) {
        DisplayState s = {0.0f, 0.0f, 0, p.keep_next ? p.state[c].next : 0};
        p.state[c] = s;
    }
}

// The listed tracks' rings in drawing order, oldest first: out[i][k] = levels[c_i][(next + k) mod L].  A lane moves two entries,
// one 16-byte store (out: 4-byte aligned at least).
struct DisplayGetParams {
    const int*          list;       // [n] or null: track i
    const DisplayState* state;
    const float2*       levels;
    float*              out;        // [n][L][2]
    int                 n, C, L;
};
__global__ void __launch_bounds__(DISPLAY_THREADS) fx_display_get_kernel(const DisplayGetParams p)
{
    const long long entries = (long long) p.n * p.L;
    const long long e0 = ((long long) blockIdx.x * DISPLAY_THREADS + threadIdx.x) * 2;
    if (e0 >= entries) return;
    float2 v[2] = {float2{0.0f, 0.0f}, float2{0.0f, 0.0f}};
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const long long e = e0 + q;
        if (e >= entries) break;
        const long long i = e / p.L;
        const int k = (int) (e - i * p.L);
        const int c = p.list ? p.list[i] : (int) i;
        if ((unsigned) c >= (unsigned) p.C) continue;                 // (the host has checked every entry)
        int from = p.state[c].next % p.L + k;
        if (from >= p.L) from -= p.L;
        v[q] = p.levels[(long long) c * p.L + from];
    }
    // (floats from a dword boundary, not dwords4 / dwords2 of fx_blocks.hip.h: stored as unsigned words, this kernel's code comes out different)
    struct __attribute__((packed, aligned(4))) floats4 { float x, y, z, w; };
    struct __attribute__((packed, aligned(4))) floats2 { float x, y; };
    if (e0 + 1 < entries) *reinterpret_cast<floats4*>(p.out + 2 * e0) = floats4{v[0].x, v[0].y, v[1].x, v[1].y};
    else *reinterpret_cast<floats2*>(p.out + 2 * e0) = floats2{v[0].x, v[0].y};
}

} // namespace fxk

struct fx_display {
    fxk::DisplayState* d_state[2] = {nullptr, nullptr};    // [C] each: a call reads one and writes the other
    int                cur = 0;                            // the table the next call reads
    float2*            d_levels = nullptr;                 // [C][L]
    int*               d_list = nullptr;                   // a channel list's device copy
    size_t             list_cap = 0;                       // bytes
    float*             d_out = nullptr;                    // fx_get_display's rows before they go to a host buffer
    size_t             out_cap = 0;                        // bytes
    int                L = 0, spb = 0;
};

namespace {

void display_release(fx_context* c)
{
    fx_display* d = c->display;
    if (!d) return;
    fx_free_device({d->d_state[0], d->d_state[1], d->d_levels, d->d_list, d->d_out});
    delete d;
    c->display = nullptr;
}

// the list's device copy, ordered on the stream (the caller's list is pageable memory: the copy has left it when the call returns)
fx_status upload_list(fx_context* c, const int* channels, int n)
{
    fx_display* d = c->display;
    { const fx_status st = fx_grow(&d->d_list, &d->list_cap, (size_t) n * sizeof(int)); if (st != FX_OK) return st; }
    HIP_TRY(hipMemcpyAsync(d->d_list, channels, (size_t) n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return FX_OK;
}

// fx_reset_state / fx_reset_channels (keep_next false: new components) and fx_clear_display_channels (keep_next true: clear());
// channels null: all tracks
fx_status display_reset(fx_context* c, const int* channels, int n, bool keep_next)
{
    fx_display* d = c->display;
    if (!d || n <= 0) return FX_OK;
    if (channels) { const fx_status st = upload_list(c, channels, n); if (st != FX_OK) return st; }
    fxk::DisplayResetParams p;
    p.list = channels ? d->d_list : nullptr;
    p.state = d->d_state[d->cur];
    p.levels = d->d_levels;
    p.n = n;
    p.C = c->C;
    p.L = d->L;
    p.keep_next = keep_next ? 1 : 0;
    const long long waves = (long long) n * ((d->L + 63) / 64);
    const long long wgs = (waves + fxk::DISPLAY_WAVES - 1) / fxk::DISPLAY_WAVES;
    if (wgs > 0x7fffffffll) return fx_fail(FX_ERR_INVALID_ARGUMENT, "list of %d tracks is too long for one display reset", n);
    hipLaunchKernelGGL(fxk::fx_display_reset_kernel, dim3((unsigned) wgs), dim3(fxk::DISPLAY_THREADS), 0, c->stream, p);
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

// after the analysis launches of a call of T frames per channel are enqueued: the call's samples, where the analysis reads them
fx_status display_launch(fx_context* c, const fx_tap_source& src, int T)
{
    fx_display* d = c->display;
    if (!d || T <= 0) return FX_OK;
    const int H = c->N / 2;
    const long long S = (long long) T * H;
    if (S > fxk::MAX_CALL_SAMPLES) return fx_fail(FX_ERR_INVALID_ARGUMENT, "call of %d frames is too long for the audio display", T);
    fxk::DisplayParams p;
    p.src = src;
    p.state_in = d->d_state[d->cur];
    p.state_out = d->d_state[d->cur ^ 1];
    p.levels = d->d_levels;
    p.chan = c->d_chan;
    p.gain = c->gain;
    p.C = c->C;
    p.L = d->L;
    p.spb = d->spb;
    p.S = (int) S;
    p.half_shift = 0;
    while ((1 << p.half_shift) < H) p.half_shift++;
    // whole display blocks per wavefront; a track has at most 2 + (S - 1) / spb of them (the carried one, then one per publication)
    p.per_chunk = d->spb >= fxk::DISPLAY_CHUNK ? 1 : fxk::DISPLAY_CHUNK / d->spb;
    const long long blocks = 2 + (S - 1) / d->spb;
    p.chunks = (int) ((blocks + p.per_chunk - 1) / p.per_chunk);
    const long long waves = (long long) c->C * p.chunks;
    const long long wgs = (waves + fxk::DISPLAY_WAVES - 1) / fxk::DISPLAY_WAVES;
    if (waves + fxk::DISPLAY_WAVES > 0x7fffffffll) return fx_fail(FX_ERR_INVALID_ARGUMENT, "call of %d frames x %d channels is too long for the audio display", T, c->C);
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_DISPLAY, 0)) r->T = T;
    hipLaunchKernelGGL(fxk::fx_display_kernel, dim3((unsigned) wgs), dim3(fxk::DISPLAY_THREADS), 0, c->stream, p);
    HIP_TRY(hipGetLastError());
    d->cur ^= 1;
    return FX_OK;
}

// the list contract of fx_context.h, with this unit's own rule: a null list of C entries means every track
fx_status check_list(const fx_context* c, const int* channels, int n, bool null_is_all)
{
    if (null_is_all && !channels && n >= 0 && n == c->C) return FX_OK;
    const fx_status st = fx_check_channel_list(c, channels, n);
    return st != FX_OK ? st : fx_check_channel_entries(c, channels, n);
}

} // namespace

extern "C" {

fx_status fx_enable_display(fx_context* c, int samples_per_block, int buffer_size)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (buffer_size < 0 || buffer_size > fxk::MAX_LENGTH)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "buffer_size %d: the audio display holds 1 .. %d levels per track (0 disables it)", buffer_size, fxk::MAX_LENGTH);
    if (buffer_size > 0 && (samples_per_block < 1 || samples_per_block > fxk::MAX_SAMPLES_PER_BLOCK))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "samples_per_block %d: 1 .. %d", samples_per_block, fxk::MAX_SAMPLES_PER_BLOCK);
    if (buffer_size == 0 && !c->display) return FX_OK;
    { const fx_status st = fx_require_device(); if (st != FX_OK) return st; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));        // launches in flight write the display that is about to go
    if (buffer_size == 0) {
        display_release(c);
        c->display_launch = nullptr;
        c->display_reset = nullptr;
        c->display_release = nullptr;
        return FX_OK;
    }
    // the new display whole before the old one goes: a failed allocation leaves the old one in force
    fx_display* d = new (std::nothrow) fx_display();
    if (!d) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    const size_t state_bytes = (size_t) c->C * sizeof(fxk::DisplayState), level_bytes = (size_t) c->C * (size_t) buffer_size * sizeof(float2);
    auto build = [&]() -> fx_status {
        for (int i = 0; i < 2; i++) {
            void* q = nullptr;
            HIP_TRY(hipMalloc(&q, state_bytes));
            d->d_state[i] = static_cast<fxk::DisplayState*>(q);
            HIP_TRY(hipMemsetAsync(q, 0, state_bytes, c->stream));
        }
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, level_bytes));
        d->d_levels = static_cast<float2*>(q);
        HIP_TRY(hipMemsetAsync(q, 0, level_bytes, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return FX_OK;
    };
    const fx_status st = build();
    if (st != FX_OK) {
        fx_free_device({d->d_state[0], d->d_state[1], d->d_levels});
        delete d;
        return st;
    }
    d->L = buffer_size;
    d->spb = samples_per_block;
    display_release(c);
    c->display = d;
    c->display_launch = display_launch;
    c->display_reset = display_reset;
    c->display_release = display_release;
    return FX_OK;
}

fx_status fx_set_display_samples_per_block(fx_context* c, int samples_per_block)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (samples_per_block < 1 || samples_per_block > fxk::MAX_SAMPLES_PER_BLOCK)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "samples_per_block %d: 1 .. %d", samples_per_block, fxk::MAX_SAMPLES_PER_BLOCK);
    if (!c->display) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the audio display is not enabled on this context (fx_enable_display)");
    c->display->spb = samples_per_block;             // (a launch argument: in force for the calls that follow, in stream order)
    return FX_OK;
}

fx_status fx_clear_display_channels(fx_context* c, const int* channels, int num_channels)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    const fx_status st = check_list(c, channels, num_channels, false);
    if (st != FX_OK) return st;
    if (!c->display) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the audio display is not enabled on this context (fx_enable_display)");
    if (num_channels == 0) return FX_OK;
    HIP_TRY(hipSetDevice(c->device));
    return display_reset(c, channels, num_channels, true);
}

fx_status fx_get_display(fx_context* c, const int* channels, int num_channels, float* levels, int mem_kind)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    { fx_status st = fx_check_memory_kind(mem_kind); if (st == FX_OK) st = check_list(c, channels, num_channels, true); if (st != FX_OK) return st; }
    fx_display* d = c->display;
    if (!d) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the audio display is not enabled on this context (fx_enable_display)");
    if (num_channels == 0) return FX_OK;
    if (!levels) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null levels buffer");
    if (mem_kind == FX_MEM_DEVICE && reinterpret_cast<uintptr_t>(levels) % 4 != 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "device levels buffer must be 4-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    fx_status st;
    if (channels && (st = upload_list(c, channels, num_channels)) != FX_OK) return st;
    const size_t bytes = (size_t) num_channels * (size_t) d->L * sizeof(float2);
    float* out = levels;
    if (mem_kind == FX_MEM_HOST) {
        if ((st = fx_grow(&d->d_out, &d->out_cap, bytes)) != FX_OK) return st;
        out = d->d_out;
    }
    fxk::DisplayGetParams p;
    p.list = channels ? d->d_list : nullptr;
    p.state = d->d_state[d->cur];
    p.levels = d->d_levels;
    p.out = out;
    p.n = num_channels;
    p.C = c->C;
    p.L = d->L;
    const long long lanes = ((long long) num_channels * d->L + 1) / 2;
    const long long wgs = (lanes + fxk::DISPLAY_THREADS - 1) / fxk::DISPLAY_THREADS;
    hipLaunchKernelGGL(fxk::fx_display_get_kernel, dim3((unsigned) wgs), dim3(fxk::DISPLAY_THREADS), 0, c->stream, p);
    HIP_TRY(hipGetLastError());
    if (mem_kind == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(levels, d->d_out, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fx_check_device_error(c);
    }
    return FX_OK;
}

} // extern "C"
