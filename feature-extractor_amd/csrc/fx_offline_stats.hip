// fx_offline_stats.hip -- what the reference derives from a ConcatenatedFeatureBuffer (ref AudioFeatures.h), for every row and channel at
// once on gfx950: getFeatureRange (:208-213), getDiscreteFeatureDistribution (:215-240) and SmoothedFeatures (:356-421), behind the
// fx_offline_feature_* / fx_offline_smooth* entries of include/fx.h, whose comments are the specification.  "ref:" citations are relative to
// the reference's Source/.
//
// The distribution's sort is a bitonic network on integer keys (the float's bits made monotonic; every NaN the largest key, which is also the
// padding to a power of two).  A compare-exchange of stride j < 64 stays inside a wave: the key sits in a register and its partner comes by
// a lane swap, so phases of up to 64 keys and the last six strides of every later phase touch LDS once.  Strides >= 64 go through LDS with
// one pair per thread and neighbouring threads on neighbouring keys (no two lanes of a group on one bank); strides >= the chunk, for rows
// longer than a chunk, are a kernel of their own on global memory.  The bracket sums are the reference's serial fp32 sums, a lane per bracket.
#include <hip/hip_runtime.h>

#include "fx_context.h"
#include "fx_offline_object.h"

#pragma clang fp contract(off)

namespace fxo {

constexpr int NT = 256;
constexpr int CHUNK = FX_OFFLINE_SORT_CHUNK;
constexpr unsigned PAD_KEY = 0xFFFFFFFFu;
constexpr int NONE = 0x7fffffff;
constexpr int SMOOTHED = 9;                 // AudioFeature::NumFeatures - 2: "only 1-D features" (ref AudioFeatures.h:360)
constexpr int MAX_DEPTH = 64;
static_assert(CHUNK >= NT && (CHUNK & (CHUNK - 1)) == 0 && NT == 256, "a chunk is a power of two, a whole number of passes of the block");

// ascending keys = ascending values; subnormals as the numbers they are; every NaN behind +inf
__device__ __forceinline__ unsigned key_of(float v)
{
    if (v != v) return PAD_KEY;
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned bits_of(unsigned k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }      // the float's bits again

// the strides j_top .. 1 (j_top <= 32) of the phase that merges blocks of k keys, on the key each lane holds: g is the key's index in its row
// (its low six bits are the lane), and a block is ascending where (g & k) == 0
__device__ __forceinline__ unsigned lane_strides(unsigned v, unsigned g, unsigned k, int j_top)
{
    const bool up = (g & k) == 0;
    for (int j = j_top; j > 0; j >>= 1) {
        const unsigned w = __shfl_xor(v, j, 64);
        const bool low = (g & (unsigned) j) == 0;
        const unsigned mn = v < w ? v : w, mx = v < w ? w : v;
        v = up == low ? mn : mx;
    }
    return v;
}
// phases 2 .. 64 on a register: runs of 64 sorted keys, ascending and descending in turn
__device__ __forceinline__ unsigned lane_phases(unsigned v, unsigned g)
{
    for (unsigned k = 2; k <= 64; k <<= 1) v = lane_strides(v, g, k, (int) (k >> 1));
    return v;
}
// the strides j_first .. 1 (64 <= j_first < n) of phase k on n keys in LDS, key i of which is key gbase + i of its row.  Ends on a barrier.
__device__ __forceinline__ void lds_strides(unsigned* s, int n, unsigned gbase, unsigned k, int j_first)
{
    for (int j = j_first; j >= 64; j >>= 1) {
        for (int t = threadIdx.x; t < n / 2; t += NT) {
            const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
            const unsigned a = s[lo], b = s[hi];
            const bool up = ((gbase + (unsigned) lo) & k) == 0;
            if ((a > b) == up) { s[lo] = b; s[hi] = a; }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += NT) s[i] = lane_strides(s[i], gbase + (unsigned) i, k, 32);       // (n is a multiple of 64: whole waves)
    __syncthreads();
}
// n keys (a power of two, 64 <= n <= CHUNK) of a row, from its key gbase on, into LDS and through the phases 2 .. n
__device__ __forceinline__ void lds_sort(unsigned* s, int n, const float* row, int D, unsigned gbase)
{
    for (int i = threadIdx.x; i < n; i += NT) {
        const unsigned g = gbase + (unsigned) i;
        s[i] = lane_phases(g < (unsigned) D ? key_of(row[g]) : PAD_KEY, g);
    }
    __syncthreads();
    for (unsigned k = 128; k <= (unsigned) n; k <<= 1) lds_strides(s, n, gbase, k, (int) (k >> 1));
}
// ref AudioFeatures.h:231-236: av + p[0] + p[1] + ... in index order, one addition after the other (eight loads ahead of their additions).
// p holds the floats' bits, not keys: the whole block turns a key back before one lane walks it, so that the walk is a load and an add.
__device__ __forceinline__ float serial_add(float av, const unsigned* p, int n)
{
    int s = 0;
    for (; s + 8 <= n; s += 8) {
        unsigned q[8];
#pragma unroll
        for (int u = 0; u < 8; u++) q[u] = p[s + u];
#pragma unroll
        for (int u = 0; u < 8; u++) av = av + __uint_as_float(q[u]);       // :235
    }
    for (; s < n; s++) av = av + __uint_as_float(p[s]);
    return av;
}
// ref AudioFeatures.h:227-238 on sorted keys in LDS: a lane per bracket
__device__ __forceinline__ void walk_brackets(unsigned* keys, int D, int num_brackets, float* out)
{
    const int step = D / num_brackets;                                     // :227
    const float fstep = (float) step;
    for (int i = threadIdx.x; i < D; i += NT) keys[i] = bits_of(keys[i]);
    __syncthreads();
    for (int b = threadIdx.x; b < num_brackets; b += NT)
        out[b] = serial_add(0.0f, keys + (size_t) b * step, step) / fstep; // :237 (step 0: 0.0f / 0.0f)
}

// ---- rows of up to CHUNK values: block = (row, channel); P keys of dynamic LDS ----
__global__ void __launch_bounds__(NT) distribution_lds_kernel(const float* __restrict__ rows, int D, int P, int num_brackets, float* __restrict__ out)
{
    extern __shared__ unsigned s_keys[];
    lds_sort(s_keys, P, rows + (size_t) blockIdx.x * D, D, 0u);
    walk_brackets(s_keys, D, num_brackets, out + (size_t) blockIdx.x * num_brackets);
}

// ---- longer rows, P keys each in global memory: block = (row of the group, chunk) ----
__global__ void __launch_bounds__(NT) chunk_sort_kernel(const float* __restrict__ rows, int D, int P, unsigned* __restrict__ keys)
{
    extern __shared__ unsigned s_keys[];
    const int chunks = P / CHUNK, row = blockIdx.x / chunks;
    const unsigned gbase = (unsigned) (blockIdx.x % chunks) * CHUNK;
    lds_sort(s_keys, CHUNK, rows + (size_t) row * D, D, gbase);
    unsigned* k = keys + (size_t) row * P + gbase;
    for (int i = threadIdx.x; i < CHUNK; i += NT) k[i] = s_keys[i];
}
// stride j >= CHUNK of phase k: thread = pair
__global__ void __launch_bounds__(NT) global_stride_kernel(unsigned* keys, int P, unsigned k, unsigned j, long long pairs)
{
    const long long t = (long long) blockIdx.x * NT + threadIdx.x;
    if (t >= pairs) return;
    const unsigned half = (unsigned) P / 2, q = (unsigned) (t % half);
    unsigned* r = keys + (size_t) (t / half) * P;
    const unsigned lo = ((q & ~(j - 1)) << 1) | (q & (j - 1)), hi = lo + j;
    const unsigned a = r[lo], b = r[hi];
    const bool up = (lo & k) == 0;
    if ((a > b) == up) { r[lo] = b; r[hi] = a; }
}
// the strides CHUNK / 2 .. 1 of phase k
__global__ void __launch_bounds__(NT) chunk_merge_kernel(unsigned* keys, int P, unsigned k)
{
    extern __shared__ unsigned s_keys[];
    const int chunks = P / CHUNK, row = blockIdx.x / chunks;
    const unsigned gbase = (unsigned) (blockIdx.x % chunks) * CHUNK;
    unsigned* g = keys + (size_t) row * P + gbase;
    for (int i = threadIdx.x; i < CHUNK; i += NT) s_keys[i] = g[i];
    __syncthreads();
    lds_strides(s_keys, CHUNK, gbase, k, CHUNK / 2);
    for (int i = threadIdx.x; i < CHUNK; i += NT) g[i] = s_keys[i];
}
// ref AudioFeatures.h:227-238 on sorted keys in global memory, block = row: up to NT brackets at a time, a lane each.  The block brings a tile of
// every bracket's keys into LDS side by side (coalesced; a row stride of T + 1 keeps the walking lanes on different banks), then each lane adds
// its T keys on: the sum stays serial in sorted order, only the loads are shared.
constexpr int WALK_TILE = 8192;
__global__ void __launch_bounds__(NT) walk_kernel(const unsigned* __restrict__ keys, int D, int P, int num_brackets, float* __restrict__ out)
{
    __shared__ unsigned s_tile[WALK_TILE + NT];
    const unsigned* k = keys + (size_t) blockIdx.x * P;
    float* o = out + (size_t) blockIdx.x * num_brackets;
    const int step = D / num_brackets;                                     // :227
    const float fstep = (float) step;
    if (step <= 32) {                                                      // a few keys a bracket: every lane fetches its own (a tile would hold NT brackets of them)
        for (int b = threadIdx.x; b < num_brackets; b += NT) {
            float av = 0.0f;
            for (int s = 0; s < step; s++) av = av + __uint_as_float(bits_of(k[(size_t) b * step + s]));
            o[b] = av / fstep;
        }
        return;
    }
    for (int b0 = 0; b0 < num_brackets; b0 += NT) {
        const int nb = min(NT, num_brackets - b0);
        int tshift = 13;                                                   // T = 2^tshift keys of each bracket per tile: nb * T <= WALK_TILE, T < 2 * step (step > 32)
        for (int p = 1; p < nb; p <<= 1) tshift--;
        while (tshift > 0 && (1 << (tshift - 1)) >= step) tshift--;
        const int T = 1 << tshift;
        float av = 0.0f;
        for (int t0 = 0; t0 < step; t0 += T) {
            const int len = min(T, step - t0);
            __syncthreads();                                               // (the tile before this one has been added)
            for (int e = threadIdx.x; e < (nb << tshift); e += NT) {
                const int bl = e >> tshift, u = e & (T - 1);
                if (u < len) s_tile[bl * (T + 1) + u] = bits_of(k[(size_t) (b0 + bl) * step + t0 + u]);
            }
            __syncthreads();
            if ((int) threadIdx.x < nb) av = serial_add(av, s_tile + threadIdx.x * (T + 1), len);
        }
        if ((int) threadIdx.x < nb) o[b0 + threadIdx.x] = av / fstep;      // :237 (step 0: 0.0f / 0.0f)
    }
}

// ---- ref AudioFeatures.h:208-213 getFeatureRange, block = (row, channel).  The serial chain's answer is, for each end, the FIRST of the values that
// compare equal to the extreme of the non-NaN values behind row[0] -- unless row[0] itself ties or beats it, or is a NaN, which nothing moves:
// (better value, then smaller index) is a total order on the candidates, so it reduces in any grouping; row[0] is compared last, strictly ----
__device__ __forceinline__ bool lower_first(float v, int i, float w, int k) { return k != NONE && (i == NONE || w < v || (w == v && k < i)); }
__device__ __forceinline__ bool higher_first(float v, int i, float w, int k) { return k != NONE && (i == NONE || w > v || (w == v && k < i)); }
__global__ void __launch_bounds__(NT) feature_ranges_kernel(const float* __restrict__ rows, int D, float* __restrict__ out)
{
    __shared__ float s_lo[NT / 64], s_hi[NT / 64];
    __shared__ int s_li[NT / 64], s_hj[NT / 64];
    const float* r = rows + (size_t) blockIdx.x * D;
    float lo = 0.0f, hi = 0.0f;
    int li = NONE, hj = NONE;                                              // no candidate yet
    for (int i = 1 + threadIdx.x; i < D; i += NT) {                        // ascending i: a thread's first among equals stays
        const float v = r[i];
        if (v == v) {                                                      // `row[i] < lo` and `row[i] > hi` are false for a NaN
            if (li == NONE || v < lo) { lo = v; li = i; }
            if (hj == NONE || v > hi) { hi = v; hj = i; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float wl = __shfl_xor(lo, o, 64), wh = __shfl_xor(hi, o, 64);
        const int kl = __shfl_xor(li, o, 64), kh = __shfl_xor(hj, o, 64);
        if (lower_first(lo, li, wl, kl)) { lo = wl; li = kl; }
        if (higher_first(hi, hj, wh, kh)) { hi = wh; hj = kh; }
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_li[threadIdx.x >> 6] = li; s_hi[threadIdx.x >> 6] = hi; s_hj[threadIdx.x >> 6] = hj; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; w++) {
            if (lower_first(lo, li, s_lo[w], s_li[w])) { lo = s_lo[w]; li = s_li[w]; }
            if (higher_first(hi, hj, s_hi[w], s_hj[w])) { hi = s_hi[w]; hj = s_hj[w]; }
        }
        float l = r[0], h = r[0];                                          // index 0 is before every candidate: only `<` / `>` moves it
        if (li != NONE && lo < l) l = lo;
        if (hj != NONE && hi > h) h = hi;
        out[2 * (size_t) blockIdx.x] = l;
        out[2 * (size_t) blockIdx.x + 1] = h;
    }
}

// ---- ref AudioFeatures.h:371-420 SmoothedFeatures::updateValues, `count` of them in a row: thread = (feature, channel), its history a column of LDS ----
__global__ void __launch_bounds__(64) smooth_rows_kernel(const float* __restrict__ rows, int D, int first, int count, int n, int depth,
                                                         float* __restrict__ current, float* __restrict__ history, float* __restrict__ out)
{
    __shared__ float h[MAX_DEPTH * 64];                                    // [k][lane]
    const int g = blockIdx.x * 64 + threadIdx.x;                           // f * C + c
    if (g >= n) return;                                                    // (no barrier below: a thread reads what it wrote itself)
    float* col = h + threadIdx.x;
    for (int k = 0; k < depth; k++) col[k * 64] = history[(size_t) g * depth + k];
    float cur = current[g];
    const float divisor = (float) depth + 1;                               // :418
    const float* in = rows + (size_t) g * D + first;
    for (int i0 = 0; i0 < count; i0 += 8) {
        float nv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) nv[u] = i0 + u < count ? in[i0 + u] : 0.0f;       // (the loads of eight updates ahead of their chains)
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (i0 + u < count) {
                float av = 0.0f;                                           // :399-409 and :413-417 in one walk: the shifted history, oldest first
                for (int k = 0; k + 1 < depth; k++) { const float v = col[(k + 1) * 64]; col[k * 64] = v; av = av + v; }
                col[(depth - 1) * 64] = cur;
                av = av + cur;
                av = av / divisor;
                cur = av + (nv[u] - av) * 0.5f;                            // :389-393
                if (out) out[(size_t) g * count + i0 + u] = cur;
            }
        }
    }
    for (int k = 0; k < depth; k++) history[(size_t) g * depth + k] = col[k * 64];
    current[g] = cur;
}

namespace {

int padded_keys(int D) { int p = 64; while (p < D) p <<= 1; return p; }

// what every entry on rows refuses, before anything is launched
fx_status check_rows(fx_offline* o, const float* rows, int R, int D, int mem_kind)
{
    if (!o || !rows) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (R < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "num_rows %d: need at least 1", R);
    if (D < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "num_downsamples %d: need at least 1", D);
    if ((long long) R * o->C > 0x7fffffffLL) return fx_fail(FX_ERR_INVALID_ARGUMENT, "num_rows %d x %d channels: more than 2^31 - 1 rows", R, o->C);
    if (mem_kind != FX_MEM_HOST && mem_kind != FX_MEM_DEVICE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown memory kind %d", mem_kind);
    return FX_OK;
}

// the input on the device (the caller's, or a staged copy) and, for host results, room for them
fx_status stage(fx_offline* o, int mem_kind, const float* in, size_t in_bytes, float* out, size_t out_bytes, const float** d_in, float** d_out)
{
    *d_in = in; *d_out = out;
    if (mem_kind == FX_MEM_DEVICE) return FX_OK;
    fx_status st = fx_grow(&o->d_in, &o->in_cap, in_bytes);
    if (st == FX_OK && out) st = fx_grow(&o->d_out, &o->out_cap, out_bytes);
    if (st != FX_OK) return st;
    HIP_TRY(hipMemcpyAsync(o->d_in, in, in_bytes, hipMemcpyHostToDevice, o->stream));
    *d_in = static_cast<const float*>(o->d_in);
    if (out) *d_out = static_cast<float*>(o->d_out);
    return FX_OK;
}

fx_status hand_back(fx_offline* o, int mem_kind, float* out, const float* d_out, size_t out_bytes)
{
    if (mem_kind != FX_MEM_HOST) return FX_OK;
    if (out) HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return FX_OK;
}

} // namespace
} // namespace fxo

extern "C" {

fx_status fx_offline_feature_ranges(fx_offline* o, const float* rows, int num_rows, int num_downsamples, float* out, int mem_kind)
{
    const int R = num_rows, D = num_downsamples;
    fx_status st = fxo::check_rows(o, rows, R, D, mem_kind);
    if (st != FX_OK) return st;
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(o->device));
    const size_t n = (size_t) R * o->C;
    const float* d_rows; float* d_out;
    if ((st = fxo::stage(o, mem_kind, rows, sizeof(float) * n * D, out, sizeof(float) * 2 * n, &d_rows, &d_out)) != FX_OK) return st;
    hipLaunchKernelGGL(fxo::feature_ranges_kernel, dim3((unsigned) n), dim3(fxo::NT), 0, o->stream, d_rows, D, d_out);
    HIP_TRY(hipGetLastError());
    return fxo::hand_back(o, mem_kind, out, d_out, sizeof(float) * 2 * n);
}

fx_status fx_offline_feature_distribution(fx_offline* o, const float* rows, int num_rows, int num_downsamples, int num_brackets, float* out, int mem_kind)
{
    const int R = num_rows, D = num_downsamples;
    fx_status st = fxo::check_rows(o, rows, R, D, mem_kind);
    if (st != FX_OK) return st;
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (num_brackets < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "num_brackets %d: need at least 1", num_brackets);
    if ((size_t) D > FX_OFFLINE_SCRATCH_BYTES / sizeof(unsigned))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "num_downsamples %d: one padded row exceeds the scratch of %u bytes", D, (unsigned) FX_OFFLINE_SCRATCH_BYTES);
    HIP_TRY(hipSetDevice(o->device));
    const size_t n = (size_t) R * o->C;
    const int P = fxo::padded_keys(D);
    const size_t group = D <= fxo::CHUNK ? n : FX_OFFLINE_SCRATCH_BYTES / (sizeof(unsigned) * (size_t) P);      // rows per pass through the scratch (>= 1)
    // every allocation first
    if (D > fxo::CHUNK && (st = fx_grow(&o->d_scratch, &o->scratch_cap, sizeof(unsigned) * (size_t) P * (group < n ? group : n))) != FX_OK) return st;
    const float* d_rows; float* d_out;
    if ((st = fxo::stage(o, mem_kind, rows, sizeof(float) * n * D, out, sizeof(float) * n * num_brackets, &d_rows, &d_out)) != FX_OK) return st;
    if (D <= fxo::CHUNK) {
        hipLaunchKernelGGL(fxo::distribution_lds_kernel, dim3((unsigned) n), dim3(fxo::NT), sizeof(unsigned) * (size_t) P, o->stream, d_rows, D, P, num_brackets, d_out);
        HIP_TRY(hipGetLastError());
        return fxo::hand_back(o, mem_kind, out, d_out, sizeof(float) * n * num_brackets);
    }
    unsigned* keys = static_cast<unsigned*>(o->d_scratch);
    const size_t chunk_lds = sizeof(unsigned) * (size_t) fxo::CHUNK;
    for (size_t r0 = 0; r0 < n; r0 += group) {
        const size_t rows_now = n - r0 < group ? n - r0 : group;
        const unsigned blocks = (unsigned) (rows_now * (size_t) (P / fxo::CHUNK));
        const long long pairs = (long long) rows_now * (P / 2);
        hipLaunchKernelGGL(fxo::chunk_sort_kernel, dim3(blocks), dim3(fxo::NT), chunk_lds, o->stream, d_rows + r0 * D, D, P, keys);
        for (unsigned k = 2u * fxo::CHUNK; k <= (unsigned) P; k <<= 1) {
            for (unsigned j = k >> 1; j >= (unsigned) fxo::CHUNK; j >>= 1)
                hipLaunchKernelGGL(fxo::global_stride_kernel, dim3((unsigned) ((pairs + fxo::NT - 1) / fxo::NT)), dim3(fxo::NT), 0, o->stream, keys, P, k, j, pairs);
            hipLaunchKernelGGL(fxo::chunk_merge_kernel, dim3(blocks), dim3(fxo::NT), chunk_lds, o->stream, keys, P, k);
        }
        hipLaunchKernelGGL(fxo::walk_kernel, dim3((unsigned) rows_now), dim3(fxo::NT), 0, o->stream, keys, D, P, num_brackets, d_out + r0 * num_brackets);
        HIP_TRY(hipGetLastError());
    }
    return fxo::hand_back(o, mem_kind, out, d_out, sizeof(float) * n * num_brackets);
}

fx_status fx_offline_smoothing(fx_offline* o, int depth)
{
    if (!o) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (depth < 0 || depth > fxo::MAX_DEPTH) return fx_fail(FX_ERR_INVALID_ARGUMENT, "depth %d: need 1 .. %d, or 0 for none", depth, fxo::MAX_DEPTH);
    HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipStreamSynchronize(o->stream));
    float* current = nullptr; float* history = nullptr;
    if (depth > 0) {                                                        // the new state first: a failed allocation leaves the old one in force
        const size_t n = (size_t) fxo::SMOOTHED * o->C;
        HIP_TRY(hipMalloc((void**) &current, sizeof(float) * n));
        hipError_t e = hipMalloc((void**) &history, sizeof(float) * n * depth);
        if (e == hipSuccess) e = hipMemsetAsync(current, 0, sizeof(float) * n, o->stream);
        if (e == hipSuccess) e = hipMemsetAsync(history, 0, sizeof(float) * n * depth, o->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
        if (e != hipSuccess) {
            (void) hipFree(current);
            if (history) (void) hipFree(history);
            return fx_fail(fx_hip_status(e), "constructing the smoothers failed: %s", hipGetErrorString(e));
        }
    }
    if (o->d_smooth_current) (void) hipFree(o->d_smooth_current);
    if (o->d_smooth_history) (void) hipFree(o->d_smooth_history);
    o->d_smooth_current = current; o->d_smooth_history = history; o->smooth_depth = depth;
    return FX_OK;
}

fx_status fx_offline_smooth_rows(fx_offline* o, const float* rows, int num_downsamples, int first, int count, float* out, int mem_kind)
{
    const int D = num_downsamples;
    fx_status st = fxo::check_rows(o, rows, fxo::SMOOTHED, D, mem_kind);
    if (st != FX_OK) return st;
    if (!o->d_smooth_current) return fx_fail(FX_ERR_INVALID_ARGUMENT, "no smoother constructed (fx_offline_smoothing)");
    if (first < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "first %d: need at least 0", first);
    if (count < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "count %d: need at least 1", count);
    if ((long long) first + count > D) return fx_fail(FX_ERR_INVALID_ARGUMENT, "first %d + count %d > num_downsamples %d", first, count, D);
    HIP_TRY(hipSetDevice(o->device));
    const int n = fxo::SMOOTHED * o->C;
    const float* d_rows; float* d_out;
    if ((st = fxo::stage(o, mem_kind, rows, sizeof(float) * (size_t) n * D, out, sizeof(float) * (size_t) n * count, &d_rows, &d_out)) != FX_OK) return st;
    hipLaunchKernelGGL(fxo::smooth_rows_kernel, dim3((unsigned) ((n + 63) / 64)), dim3(64), 0, o->stream, d_rows, D, first, count, n, o->smooth_depth,
                       o->d_smooth_current, o->d_smooth_history, d_out);
    HIP_TRY(hipGetLastError());
    return fxo::hand_back(o, mem_kind, out, d_out, sizeof(float) * (size_t) n * count);
}

fx_status fx_offline_get_smoothing(fx_offline* o, float* current, float* history)
{
    if (!o) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (!o->d_smooth_current) return fx_fail(FX_ERR_INVALID_ARGUMENT, "no smoother constructed (fx_offline_smoothing)");
    HIP_TRY(hipSetDevice(o->device));
    const size_t n = (size_t) fxo::SMOOTHED * o->C;
    if (current) HIP_TRY(hipMemcpyAsync(current, o->d_smooth_current, sizeof(float) * n, hipMemcpyDeviceToHost, o->stream));
    if (history) HIP_TRY(hipMemcpyAsync(history, o->d_smooth_history, sizeof(float) * n * o->smooth_depth, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return FX_OK;
}

} // extern "C"
