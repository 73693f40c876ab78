// fx_osc_bundle.hip -- OSC bundles formed on the device: many tracks' messages per datagram (include/fx.h: fx_get_osc_bundles,
// fx_get_osc_bundles_addressed).
//
// The reference sends one message per track per tick (ref OSCFeatureAnalysisOutput.h:107); at 65 536 tracks x 60 Hz that is 3.9e6
// datagrams a second.  An OSC 1.0 bundle -- "#bundle\0", a 64-bit time tag, then (int32 size, message) per element -- carries K tracks'
// messages in one datagram: about 17 at 1472 bytes.  The elements are the very bytes fx_get_osc_datagrams(_addressed) writes; bundle b
// holds tracks [b * K, min(C, (b + 1) * K)), K from fx_osc_bundle_plan (host arithmetic), so nothing about a layout is kept anywhere
// between calls.
//
// fx_osc_bundle_kernel: the messages of a bundle differ in length (decimal digits in the prefix form, 68 .. 192 bytes in the table form),
// so where an element starts is a prefix sum.  A wavefront (K <= 64, four bundles per workgroup) or the workgroup of 256 threads
// (K <= 1024) takes a bundle: lanes take elements and scan their word counts (__shfl_up within a wavefront, wavefront totals through
// LDS) into an offset table in LDS; then lanes take output words, consecutive lanes consecutive words, and each finds its element by
// binary search in that table and forms the word with osc_bundle_word (fx_osc_words.h: the function the host encoders run too).  Pure
// byte movement: plain vector loads and stores, no atomics, 4.1 KB of LDS.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "fx_kernels.h"
#include "fx_context.h"
#include "fx_osc_words.h"

namespace fxk {

constexpr int OSC_BUNDLE_THREADS = 256, OSC_BUNDLE_WAVES = OSC_BUNDLE_THREADS / 64;
static_assert(FX_OSC_PREFIX_BYTES == FX_OSC_PREFIX_MAX, "OscBundleParams holds the longest prefix");
static_assert(OSC_BUNDLE_WAVES * (64 + 1) <= FX_OSC_BUNDLE_MAX_ELEMENTS + 1, "the wavefronts' offset tables share the workgroup's");
static_assert(FX_OSC_BUNDLE_MAX_ELEMENTS % OSC_BUNDLE_THREADS == 0, "whole rounds of the workgroup scan");

// inclusive prefix sum over the wavefront's lanes
__device__ __forceinline__ int osc_wave_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

__global__ void __launch_bounds__(OSC_BUNDLE_THREADS) fx_osc_bundle_kernel(const OscBundleParams p)
{
    __shared__ int s_off[FX_OSC_BUNDLE_MAX_ELEMENTS + 1];
    __shared__ int s_total[OSC_BUNDLE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bundles = (p.C + p.K - 1) / p.K;
    const bool per_wave = p.K <= 64;                                        // (uniform over the launch)
    const int b = per_wave ? (int) blockIdx.x * OSC_BUNDLE_WAVES + wave : (int) blockIdx.x;
    const bool live = b < bundles;                                          // (a whole wavefront, or the whole workgroup)
    const int count = !live ? 0 : (p.C - b * p.K < p.K ? p.C - b * p.K : p.K);
    int* off = per_wave ? s_off + wave * (64 + 1) : s_off;

    if (per_wave) {
        const int incl = osc_wave_scan(lane < count ? 1 + osc_bundle_element_words(p, b * p.K + lane) : 0, lane);
        if (lane == 0) off[0] = FX_OSC_BUNDLE_HEADER_WORDS;
        if (lane < count) off[lane + 1] = FX_OSC_BUNDLE_HEADER_WORDS + incl;
        __syncthreads();
    } else {
        int carry = FX_OSC_BUNDLE_HEADER_WORDS;
        if (tid == 0) off[0] = carry;
        for (int base = 0; base < count; base += OSC_BUNDLE_THREADS) {      // (count is the workgroup's: every thread makes the same rounds)
            const int e = base + tid;
            const int incl = osc_wave_scan(e < count ? 1 + osc_bundle_element_words(p, b * p.K + e) : 0, lane);
            if (lane == 63) s_total[wave] = incl;
            __syncthreads();
            int before = carry;
#pragma unroll
            for (int w = 0; w < OSC_BUNDLE_WAVES; w++) {
                const int s = s_total[w];
                if (w < wave) before += s;
                carry += s;
            }
            if (e < count) off[e + 1] = before + incl;
            __syncthreads();                                                // (s_total is rewritten by the next round; after the last, `off` is whole)
        }
    }
    if (!live) return;

    const int words = p.stride >> 2;
    unsigned* out = reinterpret_cast<unsigned*>(p.out + (size_t) b * (size_t) p.stride);
    const int first = per_wave ? lane : tid, step = per_wave ? 64 : OSC_BUNDLE_THREADS;
    for (int w = first; w < words; w += step) out[w] = osc_bundle_word(p, b, off, count, w);
}

// p.K and p.stride are fx_osc_bundle_plan's (the caller has checked them): a slot holds the fullest bundle, and in the table form a thread
// reads words [0, (len + 4) / 4) <= FX_OSC_ROW_WORDS of a track's row only.  Writes [0, num_bundles * stride) of p.out and nothing else.
static hipError_t launch_osc_bundle_kernel(const OscBundleParams& p, hipStream_t stream)
{
    if (p.C <= 0) return hipSuccess;
    if (p.K < 1 || p.K > FX_OSC_BUNDLE_MAX_ELEMENTS || p.K > p.C || p.stride < 16 + p.K * (4 + 68) || (p.stride & 3) || !p.latest || !p.out ||
        (reinterpret_cast<uintptr_t>(p.out) & 3) || (p.rows ? !p.len : (p.prefix_len < 0 || p.prefix_len > FX_OSC_PREFIX_BYTES || p.first_channel < 0 || p.first_channel > 0x7fffffff - p.C)))
        return hipErrorInvalidValue;
    const int bundles = (p.C + p.K - 1) / p.K;
    const int wgs = p.K <= 64 ? (bundles + OSC_BUNDLE_WAVES - 1) / OSC_BUNDLE_WAVES : bundles;
    hipLaunchKernelGGL(fx_osc_bundle_kernel, dim3((unsigned) wgs), dim3(OSC_BUNDLE_THREADS), 0, stream, p);
    return hipGetLastError();
}

} // namespace fxk

namespace {

// What the two entry points share once `p` names the address source and `longest` is its longest message: the plan, the refusals that
// are left (all before any device use), the launch and the lengths.  message_bytes(c): the bytes of track c's message.
template <typename MessageBytes>
fx_status get_bundles(fx_context* c, fxk::OscBundleParams& p, int longest, unsigned long long timetag, int max_datagram_bytes, unsigned char* out, int stride,
                      int* lengths, int mem_kind, MessageBytes message_bytes)
{
    int K = 0, bundles = 0, need = 0;
    const fx_status planned = fx_osc_bundle_plan(longest, c->C, max_datagram_bytes, &K, &bundles, &need);
    if (planned != FX_OK) return planned;
    if (stride < need || (stride & 3)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "stride %d: must be a multiple of 4 and hold the fullest bundle (%d bytes)", stride, need);
    if (mem_kind == FX_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 3)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "a device buffer of bundles must start on a 4-byte boundary");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t) bundles * (size_t) stride;
    if (mem_kind == FX_MEM_HOST) { const fx_status st = fx_grow(&c->d_osc, &c->osc_cap, bytes); if (st != FX_OK) return st; }
    p.latest = c->d_latest;
    p.out = mem_kind == FX_MEM_HOST ? c->d_osc : out;
    p.C = c->C;
    p.K = K;
    p.stride = stride;
    p.timetag_hi = (unsigned) (timetag >> 32);
    p.timetag_lo = (unsigned) timetag;
    c->num_launches = 0;                            // an entry point that launches starts the launch record anew
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_OSC_BUNDLE, 0)) r->T = K;
    HIP_TRY(fxk::launch_osc_bundle_kernel(p, c->stream));
    if (lengths)
        for (int b = 0; b < bundles; b++) {
            int n = 16;
            for (int t = b * K; t < c->C && t < (b + 1) * K; t++) n += 4 + message_bytes(t);
            lengths[b] = n;
        }
    if (mem_kind == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, c->d_osc, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fx_check_device_error(c);
    }
    return FX_OK;
}

} // namespace

extern "C" {

// ref OSCFeatureAnalysisOutput.h:89-113 for every track at once, K tracks' messages per OSC 1.0 bundle
fx_status fx_get_osc_bundles(fx_context* c, const char* prefix, int first_channel, unsigned long long timetag, int max_datagram_bytes, unsigned char* out,
                             int stride, int* lengths, int mem_kind)
{
    if (!c || !prefix || !out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (mem_kind != FX_MEM_HOST && mem_kind != FX_MEM_DEVICE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown memory kind %d", mem_kind);
    const int longest = first_channel < 0 || first_channel > 0x7fffffff - c->C ? -1 : fx_osc_message_bytes(prefix, first_channel + c->C - 1);
    if (longest < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "OSC prefix longer than %d bytes, or a channel number out of range", fxk::FX_OSC_PREFIX_MAX);
    fxk::OscBundleParams p = {};
    p.first_channel = first_channel;
    p.prefix_len = (int) strlen(prefix);
    memcpy(p.prefix, prefix, (size_t) p.prefix_len);
    return get_bundles(c, p, longest, timetag, max_datagram_bytes, out, stride, lengths, mem_kind,
                       [&](int t) { return fx_osc_message_bytes(prefix, first_channel + t); });
}

// the same with every track's own bundleAddress (ref OSCFeatureAnalysisOutput.h:107; fx_set_osc_addresses)
fx_status fx_get_osc_bundles_addressed(fx_context* c, unsigned long long timetag, int max_datagram_bytes, unsigned char* out, int stride, int* lengths, int mem_kind)
{
    if (!c || !out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (mem_kind != FX_MEM_HOST && mem_kind != FX_MEM_DEVICE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown memory kind %d", mem_kind);
    const fx_osc_table* t = c->osc_table;
    if (!t) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the context has no OSC address table (fx_set_osc_addresses)");
    fxk::OscBundleParams p = {};
    p.rows = reinterpret_cast<const unsigned*>(t->d_table);
    p.len = reinterpret_cast<const int*>(t->d_table + (size_t) c->C * fxk::FX_OSC_ROW_BYTES);
    return get_bundles(c, p, t->longest, timetag, max_datagram_bytes, out, stride, lengths, mem_kind, [t](int track) { return t->message_bytes[(size_t) track]; });
}

} // extern "C"
