// fx_taps.hip -- analysis taps: the reference's display buffers (include/fx.h, fx_request_taps / fx_get_taps).
//
// ref RealTimeAudioAnalysis.h:221-232 (the overlapped window), :268-283 (the spectral and the harmonic analyser's transform),
// PitchAnalyser.h:30-53,66-72,187 (autocorrelation, cumulative normalised difference, normalised lag position).  Each of the reference's
// flags is a one-shot: the next frame analysed copies its buffer.  Here an armed channel's buffers are formed from the window the call's
// first frame analyses, by ONE launch of fx_taps_kernel (one workgroup per armed channel) on the context's stream, ahead of every launch
// of the call that changes the context's state.  The kernel reads the window where the analysis kernels read it -- the carried tail, the
// caller's hops / frame / [pending | block] stream, widened by the same widen_one -- and restates the reference's arithmetic plainly:
// the transforms run the reference FFT's butterfly DAG as fx_plain_fft.hip.h states it (one butterfly per thread and level through
// LDS), and the serial parts (the low-pass, the fp32 running sum, the lag walk) on one lane.  Off the hot path: clarity before speed.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: fx_request_taps installs the context's two hooks (fx_context.h), and the analysis entry
// points call them only when channels are armed.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"

#pragma clang fp contract(off)

namespace fxk {

#include "fx_wave.hip.h"          // f4
#include "fx_samples.hip.h"
#include "fx_blocks.hip.h"        // BlockStream

namespace {

constexpr int TAP_THREADS = 256;

// what one capture stores per channel, in this order: window [N], spectrum [2N], pitch spectrum [2N], autocorrelation [N], cnd [N],
// lag position [2]
__host__ __device__ constexpr long long tap_row_floats(int n) { return 7ll * n + 2; }

struct TapsParams {
    fx_tap_source src;
    const float*  tail;         // [C][N/2] fp32, already gained: FrameParams::tail_in of the call
    float         gain;
    const ChannelSettings* chan;    // per-track settings or null (FrameParams::chan): the window shows the channel's own gain
    const float*  tw;           // [N][2] the reference's forward table (phase in double, rounded to float); the inverse uses its conjugate
    const float*  ramp;         // [N] the Bartlett window's gains, as applyGainRamp accumulates them
    float         lpf_a, lpf_b; // FrameParams::lpf_a / lpf_b
    float*        out;          // [num][tap_row_floats(N)]
    int           num;
    int           channels[FX_MAX_TAP_CHANNELS];
};

// the plan, the complex helpers and plain_transform: the one statement of the reference FFT's DAG
#include "fx_plain_fft.hip.h"

// sample j of the channel's first new hop (hop_mode 1) or of its first frame (hop_mode 0), widened as the analysis kernels widen it
template <int FMT> __device__ __forceinline__ float first_sample(const fx_tap_source& src, int c, int j)
{
    constexpr int B = sample_bytes(FMT);
    const unsigned char* row = static_cast<const unsigned char*>(src.in) + (long long) c * src.in_row_bytes;
    if (src.carry) {
        const BlockStream bs = {src.carry + (long long) c * src.carry_row_bytes, row, src.carry_bytes, src.in_row_bytes};
        return widen_one<FMT>(stream_sample<B>(bs, j));
    }
    return widen_one<FMT>(row + (long long) j * B);
}

template <int N, int FMT> __device__ void load_window(const TapsParams& p, int c, float* win)
{
    constexpr int H = N / 2;
    // (c is the workgroup's channel: uniform, the gain a scalar as in the analysis kernels -- channel_gain, fx_kernels.h, written out:
    // through the helper this kernel's code comes out different)
    const float gain = p.chan ? *(UniformFloatPtr) &p.chan[__builtin_amdgcn_readfirstlane(c)].gain : p.gain;
    for (int i = threadIdx.x; i < N; i += TAP_THREADS) {
        float x;
        if (!p.src.hop_mode) x = first_sample<FMT>(p.src, c, i);                      // fx_process_frames: as given, no gain
        else if (i < H) x = p.tail[(long long) c * H + i];
        else {
            x = first_sample<FMT>(p.src, c, i - H);
            if (gain != 1.0f) x *= gain;                                           // ref AudioDataCollector.h:88, as the kernels apply it
        }
        win[i] = x;
    }
}

template <int N>
__global__ void __launch_bounds__(TAP_THREADS) fx_taps_kernel(const TapsParams p)
{
    __shared__ cpx buf[N];
    __shared__ float aux[N];
    __shared__ float tail_scalar[2];         // v[N] and cnd[N]: the lag walk may look one sample past the first N
    const int slot = blockIdx.x, c = p.channels[slot], tid = threadIdx.x;
    float* out = p.out + (long long) slot * tap_row_floats(N);
    float* o_win = out;
    float* o_spec = out + N;
    float* o_pitch = out + 3 * N;
    float* o_ac = out + 5 * N;
    float* o_cnd = out + 6 * N;
    float* o_lag = out + 7 * N;
    using P = PlainPlan<N>;

    // the overlapped window (RealTimeAudioDataOverlapper::getNextBuffer, RealTimeAudioAnalysis.h:205-228)
    FX_FORMAT(p.src.sample_format, (load_window<N, FMT>(p, c, aux)));
    __syncthreads();
    for (int i = tid; i < N; i += TAP_THREADS) o_win[i] = aux[i];

    // spectral analyser: Bartlett window (RealTimeAnalyser.h:212) -> forward transform (:215)
    for (int q = tid; q < N; q += TAP_THREADS) {
        const int k = P::source(q);
        buf[q] = cpx{aux[k] * p.ramp[k], 0.0f};
    }
    __syncthreads();
    plain_transform<N, false, TAP_THREADS>(buf, p.tw);
    for (int q = tid; q < N; q += TAP_THREADS) reinterpret_cast<float2*>(o_spec)[q] = float2{buf[q].r, buf[q].i};

    // harmonic analyser: one-pole low-pass (RealTimeAudioAnalysis.h:106-125; serial), Bartlett window, forward transform (RealTimeAnalyser.h:152-160)
    if (tid == 0) {
        float prev = aux[0];
        for (int s = 1; s < N; s++) {
            prev = (p.lpf_a * aux[s]) + (p.lpf_b * prev);
            aux[s] = prev;
        }
    }
    __syncthreads();
    for (int q = tid; q < N; q += TAP_THREADS) {
        const int k = P::source(q);
        buf[q] = cpx{aux[k] * p.ramp[k], 0.0f};
    }
    __syncthreads();
    plain_transform<N, false, TAP_THREADS>(buf, p.tw);
    for (int q = tid; q < N; q += TAP_THREADS) {
        reinterpret_cast<float2*>(o_pitch)[q] = float2{buf[q].r, buf[q].i};
        aux[q] = buf[q].r * buf[q].r;        // getComplexConjugateMultiplication (PitchAnalyser.h:83-108): re * re, imag 0
    }
    __syncthreads();

    // getAutoCorrelationFromConjugateMultiplication (:110-127): inverse transform, 1/N, v[s] = d[s] * d[s] * s
    for (int q = tid; q < N; q += TAP_THREADS) buf[q] = cpx{aux[P::source(q)], 0.0f};
    __syncthreads();
    plain_transform<N, true, TAP_THREADS>(buf, p.tw);
    const float scale = 1.0f / N;
    for (int s = tid; s < N; s += TAP_THREADS) {
        const float d = buf[s].r * scale;
        const float v = d * d * (float) s;
        aux[s] = v;
        o_ac[s] = v;
    }
    if (tid == 0) {
        const float d = buf[0].i * scale;    // sample N of the planar result: the imaginary part of element 0
        tail_scalar[0] = d * d * (float) N;
    }
    __syncthreads();

    // getCumulativeNormalisedDifferenceFromAutoCorrelationBuffer (:129-159): the running fp32 sum, serial, into buf[s].r; then the ratios
    if (tid == 0) {
        float sum = 0.0f;
        for (int s = 1; s < N; s++) {
            sum += aux[s];
            buf[s].r = sum;
        }
        sum += tail_scalar[0];
        tail_scalar[1] = (sum != 0.0f) ? tail_scalar[0] / sum : 0.0f;
    }
    __syncthreads();
    for (int s = tid; s < N; s += TAP_THREADS) {
        const float sum = buf[s].r, v = aux[s];
        const float cnd = s == 0 ? 1.0f : ((sum != 0.0f) ? v / sum : 0.0f);
        aux[s] = cnd;
        o_cnd[s] = cnd;
    }
    __syncthreads();

    // getLagEstimateFromCumulativeDifference (:161-190) + getInterpolatedValley... (:192-217): only its first branch is reachable
    if (tid == 0) {
        float x = -1.0f, y = 100.0f;
        for (int s = 2; s < N; s++) {
            if (aux[s] < 0.01f) {
                while (s + 1 < N && aux[s + 1] < aux[s]) s++;
                const int right = s + ((s < N + 1) ? 1 : 0);
                const float here = aux[s], there = right < N ? aux[right] : tail_scalar[1];
                if (here <= there) { x = (float) s; y = here; }
                else { x = (float) right; y = there; }
                break;
            }
        }
        o_lag[0] = x / (float) (2 * N);          // normalisedLagPosition (:187): x over the buffer's 2N samples
        o_lag[1] = y;
    }
}

// the reference's forward table (JUCE 4.2 FFT::FFTConfig: phase in double, entries rounded to float), then the Bartlett window's gains:
// applyGainRamp (0 -> 1) over the first half and (1 -> 0) over the second, each gain the float sum of the increments before it
std::vector<float> tap_constants(int n)
{
    std::vector<float> k(3 * (size_t) n);
    for (int i = 0; i < n; i++) {
        const double phase = -2.0 * 3.14159265358979323846 * i / n;
        k[2 * i] = (float) std::cos(phase);
        k[2 * i + 1] = (float) std::sin(phase);
    }
    float* ramp = k.data() + 2 * (size_t) n;
    const int h = n / 2;
    float g = 0.0f;
    const float up = (1.0f - 0.0f) / h, down = (0.0f - 1.0f) / h;
    for (int i = 0; i < h; i++) { ramp[i] = g; g += up; }
    g = 1.0f;
    for (int i = 0; i < h; i++) { ramp[h + i] = g; g += down; }
    return k;
}

} // namespace
} // namespace fxk

struct fx_taps {
    std::vector<int> armed;         // channels waiting for a capture, in the order they were armed
    std::vector<int> captured;      // channels of the latest capture, in slot order
    long long        frame = -1;    // frame index of the latest capture (the context's count)
    std::vector<long long> first;   // per captured channel: the first frame of its stream then (fx_reset_channels), so that
                                    // fx_get_taps reports the track's own index
    float*           d_consts = nullptr;    // fxk::tap_constants
    float*           d_store = nullptr;     // [slots][tap_row_floats(N)]
    int              slots = 0;
};

namespace {

void taps_release(fx_context* c)
{
    if (!c->taps) return;
    if (c->taps->d_consts) (void) hipFree(c->taps->d_consts);
    if (c->taps->d_store) (void) hipFree(c->taps->d_store);
    delete c->taps;
    c->taps = nullptr;
    c->taps_armed = 0;
}

fx_status taps_launch(fx_context* c, const fx_tap_source& src)
{
    fx_taps* t = c->taps;
    if (!t || t->armed.empty()) return FX_OK;
    const int n = c->N, k = (int) t->armed.size();
    if (!t->d_consts) {
        const std::vector<float> consts = fxk::tap_constants(n);
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, consts.size() * sizeof(float)));
        t->d_consts = static_cast<float*>(q);
        HIP_TRY(hipMemcpy(t->d_consts, consts.data(), consts.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (t->slots < k) {
        // (the store grows to the armed count: the old capture goes with it -- this call replaces it anyway)
        t->captured.clear();
        if (t->d_store) { float* old = t->d_store; t->d_store = nullptr; t->slots = 0; HIP_TRY(hipFree(old)); }
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, (size_t) k * (size_t) fxk::tap_row_floats(n) * sizeof(float)));
        t->d_store = static_cast<float*>(q);
        t->slots = k;
    }
    fxk::TapsParams p;
    p.src = src;
    p.tail = c->d_tail[c->cur];
    p.gain = c->gain;
    p.chan = c->d_chan;
    p.tw = t->d_consts;
    p.ramp = t->d_consts + 2 * (size_t) n;
    p.lpf_a = c->lpf_a;
    p.lpf_b = c->lpf_b;
    p.out = t->d_store;
    p.num = k;
    for (int i = 0; i < FX_MAX_TAP_CHANNELS; i++) p.channels[i] = i < k ? t->armed[i] : 0;
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_TAPS, 0)) { r->T = k; r->block_mode = src.carry ? 1 : 0; }
    const dim3 grid((unsigned) k), block(fxk::TAP_THREADS);
    switch (n) {
        case 256:  hipLaunchKernelGGL(fxk::fx_taps_kernel<256>, grid, block, 0, c->stream, p); break;
        case 512:  hipLaunchKernelGGL(fxk::fx_taps_kernel<512>, grid, block, 0, c->stream, p); break;
        case 1024: hipLaunchKernelGGL(fxk::fx_taps_kernel<1024>, grid, block, 0, c->stream, p); break;
        case 2048: hipLaunchKernelGGL(fxk::fx_taps_kernel<2048>, grid, block, 0, c->stream, p); break;
        case 4096: hipLaunchKernelGGL(fxk::fx_taps_kernel<4096>, grid, block, 0, c->stream, p); break;
        default:   return fx_fail(FX_ERR_UNSUPPORTED, "no taps kernel for window size %d", n);
    }
    HIP_TRY(hipGetLastError());
    t->captured.swap(t->armed);
    t->armed.clear();
    t->frame = c->frames_seen;
    t->first.assign(t->captured.size(), 0);
    if (!c->chan.empty())
        for (size_t i = 0; i < t->captured.size(); i++) t->first[i] = c->chan[(size_t) t->captured[i]].first_frame;
    c->taps_armed = 0;
    return FX_OK;
}

} // namespace

extern "C" {

fx_status fx_request_taps(fx_context* c, const int* channels, int num_channels)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (num_channels < 0 || (num_channels > 0 && !channels)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "bad channel list");
    std::vector<int> want = c->taps ? c->taps->armed : std::vector<int>();
    for (int i = 0; i < num_channels; i++) {
        const int ch = channels[i];
        if (ch < 0 || ch >= c->C) return fx_fail(FX_ERR_INVALID_ARGUMENT, "channel %d out of range [0,%d)", ch, c->C);
        if (std::find(want.begin(), want.end(), ch) == want.end()) want.push_back(ch);
    }
    if ((int) want.size() > FX_MAX_TAP_CHANNELS)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d channels armed for taps; at most %d", (int) want.size(), FX_MAX_TAP_CHANNELS);
    if (!c->taps) {
        c->taps = new (std::nothrow) fx_taps();
        if (!c->taps) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    c->taps->armed.swap(want);
    c->taps_armed = (int) c->taps->armed.size();
    c->taps_launch = taps_launch;
    c->taps_release = taps_release;
    return FX_OK;
}

fx_status fx_get_taps(fx_context* c, int channel, float* window, float* spectrum, float* pitch_spectrum, float* autocorrelation,
                      float* cnd, float* lag_position, long long* frame_index)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    const fx_taps* t = c->taps;
    const int slot = t ? (int) (std::find(t->captured.begin(), t->captured.end(), channel) - t->captured.begin()) : 0;
    if (!t || slot >= (int) t->captured.size()) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the latest capture holds no taps of channel %d", channel);
    const int n = c->N;
    std::vector<float> row((size_t) fxk::tap_row_floats(n));
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(row.data(), t->d_store + (size_t) slot * row.size(), row.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const float* r = row.data();
    if (window) std::copy(r, r + n, window);
    if (spectrum) std::copy(r + n, r + 3 * n, spectrum);
    if (pitch_spectrum) std::copy(r + 3 * n, r + 5 * n, pitch_spectrum);
    if (autocorrelation) std::copy(r + 5 * n, r + 6 * n, autocorrelation);
    if (cnd) std::copy(r + 6 * n, r + 7 * n, cnd);
    if (lag_position) std::copy(r + 7 * n, r + 7 * n + 2, lag_position);
    if (frame_index) *frame_index = t->frame - t->first[(size_t) slot];
    return FX_OK;
}

} // extern "C"
