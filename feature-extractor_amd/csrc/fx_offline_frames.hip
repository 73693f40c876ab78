// fx_offline_frames.hip -- the offline driver's own kernels (include/fx.h, fx_offline_frames / fx_offline_analyse): the frame / window /
// magnitude stage of the reference's AudioAnalyser::performSpectralAnalysis (ref AudioAnalysis.h:129-251; "ref:" citations are relative to
// the reference's Source/), and the parts of its ConcatenatedFeatureBuffer (ref AudioFeatures.h:14-314) that are arithmetic: the downsampled
// RMS row, its normalisation, the log attack time of every channel at once, and the placing of the per-frame results in the feature rows.
// The entries themselves, and the per-frame kernels they run between these, are in fx_offline.hip.
//
// The frame kernel is the hot path of an offline analysis -- N log N a frame against the O(N) of every per-frame kernel: one workgroup per
// (frame, channel); the window is read in sample order (coalesced; the padding rule decides per sample), multiplied by the Bartlett gain and
// written to LDS at its leaf position of the reference FFT's recursion; the transform is the plain per-level form of fx_plain_fft.hip.h, which
// fx_taps.hip runs too (one butterfly per thread and level, table twiddles, no fused multiply-add: the DAG of every transform in this
// library, so the same bits); the magnitudes leave in bin order (coalesced) and one lane adds them up in bin order for the energy envelope.
// LDS: N complex + N / 2 + 1 floats = 48 KB at 4096 points.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "fx_offline_frames.h"

#pragma clang fp contract(off)

namespace fxo {
namespace {

constexpr int NT = 256;

// the plan, the complex helpers and plain_transform: the one statement of the reference FFT's DAG
#include "fx_plain_fft.hip.h"

#include "fx_offline_frame_body.hip.h"
#include "fx_offline_steps.hip.h"

struct PlainSamples {                                                       // a channel of audio [C][S]
    const float* a;
    __device__ __forceinline__ float operator()(long long i) const { return a[i]; }
};

// block = (frame, channel): blockIdx.x = (f - first_frame) * C + c
template <int N>
__global__ void __launch_bounds__(NT) offline_frames_kernel(const float* __restrict__ audio, int C, int S, int D, int first_frame,
                                                            const float* __restrict__ tw, float* __restrict__ mags, float* __restrict__ energy)
{
    constexpr int H = N / 2, B = N / 2 + 1;
    const int fl = blockIdx.x / C, c = blockIdx.x - fl * C, f = first_frame + fl;
    const int step = S / D;                                                 // :135 (int division)
    // :150-161: the window is centred on the downsample -- unless there is one frame only, which starts at sample 0
    const long long start = D == 1 ? 0 : (long long) f * step - H;
    frame_body<N>(PlainSamples{audio + (size_t) c * S}, S, start, tw, mags + ((size_t) fl * C + c) * B, energy ? energy + (size_t) c * D + f : nullptr);
}

// ---- ref AudioFeatures.h:158-184 fillDownsampledRMSAudioChannels: lane = (channel, downsample), walking its step serially ----
__global__ void __launch_bounds__(NT) rms_row_kernel(const float* __restrict__ audio, int C, int S, int D, float* __restrict__ row)
{
    const long long t = (long long) blockIdx.x * NT + threadIdx.x;
    if (t >= (long long) C * D) return;
    const int c = (int) (t / D), i = (int) (t - (long long) c * D);
    const int spb = S / D;                                                  // :161
    row[t] = rms_of_step(PlainSamples{audio + (size_t) c * S + (size_t) i * spb}, spb);
}

// ---- ref AudioFeatures.h:186-195 normaliseAudioChannels, one channel's row per block.  findMinMax starts both ends from row[0] and moves on
// `<` / `>` only: a NaN elsewhere is skipped (so one early in a thread's stride hides nothing), a NaN at row[0] stays -- thread 0's business ----
__global__ void __launch_bounds__(NT) normalise_row_kernel(float* row, int D)
{
    __shared__ float s_lo[NT], s_hi[NT];
    __shared__ float s_scale;
    float* r = row + (size_t) blockIdx.x * D;
    float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();          // (+inf never moves the minimum, -inf never the maximum)
    for (int i = 1 + threadIdx.x; i < D; i += NT) { const float v = r[i]; if (v < lo) lo = v; if (v > hi) hi = v; }
    s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        float l = r[0], h = r[0];
        for (int k = 0; k < NT; k++) { if (s_lo[k] < l) l = s_lo[k]; if (s_hi[k] > h) h = s_hi[k]; }
        const float al = fabsf(l), ah = fabsf(h);
        const float m = al < ah ? ah : al;                                  // jmax (a, b) = a < b ? b : a
        s_scale = 1.0f / m;                                                 // :193
    }
    __syncthreads();
    const float scale = s_scale;
    for (int i = threadIdx.x; i < D; i += NT) r[i] = r[i] * scale;          // :194
}

// ---- ref AudioAnalysis.h:611-622 setLogAttackTime, block = channel, over the rows of energy [C][n] ----
__global__ void __launch_bounds__(NT) log_attack_times_kernel(const float* __restrict__ energy, int n, int num_input_samples, int num_downsamples,
                                                              int sample_rate, float* __restrict__ out)
{
    const int samples_per_step = num_input_samples / num_downsamples;       // :620
    log_attack_block(energy + (size_t) blockIdx.x * n, n, samples_per_step, sample_rate, out + blockIdx.x);
}

// ---- ref AudioFeatures.h:133-140 setFeatureSample, for the per-frame results of a whole call: thread = (frame, channel) ----
enum { ROW_CENTROID = 0, ROW_SLOPE, ROW_SPREAD, ROW_FLATNESS, ROW_FLUX, ROW_ZERO_CROSSES, ROW_F0, ROW_HER, ROW_INHARMONICITY };
__global__ void __launch_bounds__(NT) scatter_rows_kernel(const float* __restrict__ out4, const float* __restrict__ slope, const float* __restrict__ out3,
                                                          int C, int D, float* __restrict__ features)
{
    const long long t = (long long) blockIdx.x * NT + threadIdx.x;          // = f * C + c
    if (t >= (long long) C * D) return;
    const int f = (int) (t / C), c = (int) (t - (long long) f * C);
    const size_t rows = (size_t) C * D, at = (size_t) c * D + f;
    if (out4) {                                                             // centroid / nyquist, spread, flatness, flux
        features[ROW_CENTROID * rows + at] = out4[4 * t];
        features[ROW_SPREAD * rows + at] = out4[4 * t + 1];
        features[ROW_FLATNESS * rows + at] = out4[4 * t + 2];
        features[ROW_FLUX * rows + at] = out4[4 * t + 3];
    }
    if (slope) features[ROW_SLOPE * rows + at] = slope[t];
    if (out3) {                                                             // f0, harmonic energy ratio, inharmonicity
        features[ROW_F0 * rows + at] = out3[3 * t];
        features[ROW_HER * rows + at] = out3[3 * t + 1];
        features[ROW_INHARMONICITY * rows + at] = out3[3 * t + 2];
    }
}

unsigned blocks_for(long long items) { return (unsigned) ((items + NT - 1) / NT); }

} // namespace

std::vector<float> forward_table(int n)
{
    std::vector<float> k(2 * (size_t) n);
    for (int i = 0; i < n; i++) {
        const double phase = -2.0 * 3.14159265358979323846 * i / n;
        k[2 * i] = (float) std::cos(phase);
        k[2 * i + 1] = (float) std::sin(phase);
    }
    return k;
}

fx_status launch_frames(hipStream_t stream, const float* audio, int C, int S, int D, int n, int first_frame, int num_frames, const float* table,
                        float* mags, float* energy)
{
    const int bins = n / 2 + 1;
    const int per_launch = (1 << 30) / C;                                   // the grid's x extent stays below 2^31
    for (int done = 0; done < num_frames; done += per_launch) {
        const int frames = num_frames - done < per_launch ? num_frames - done : per_launch;
        const dim3 grid((unsigned) ((long long) frames * C)), block(NT);
        float* m = mags + (size_t) done * C * bins;
        const int first = first_frame + done;
        switch (n) {
            case 256:  hipLaunchKernelGGL(offline_frames_kernel<256>, grid, block, 0, stream, audio, C, S, D, first, table, m, energy); break;
            case 512:  hipLaunchKernelGGL(offline_frames_kernel<512>, grid, block, 0, stream, audio, C, S, D, first, table, m, energy); break;
            case 1024: hipLaunchKernelGGL(offline_frames_kernel<1024>, grid, block, 0, stream, audio, C, S, D, first, table, m, energy); break;
            case 2048: hipLaunchKernelGGL(offline_frames_kernel<2048>, grid, block, 0, stream, audio, C, S, D, first, table, m, energy); break;
            case 4096: hipLaunchKernelGGL(offline_frames_kernel<4096>, grid, block, 0, stream, audio, C, S, D, first, table, m, energy); break;
            default: return fx_fail(FX_ERR_INVALID_ARGUMENT, "window_size %d is not one of 256, 512, 1024, 2048, 4096", n);
        }
        HIP_TRY(hipGetLastError());
    }
    return FX_OK;
}

fx_status launch_rms_row(hipStream_t stream, const float* audio, int C, int S, int D, float* row)
{
    hipLaunchKernelGGL(rms_row_kernel, dim3(blocks_for((long long) C * D)), dim3(NT), 0, stream, audio, C, S, D, row);
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

fx_status launch_normalise_row(hipStream_t stream, float* row, int C, int D)
{
    hipLaunchKernelGGL(normalise_row_kernel, dim3((unsigned) C), dim3(NT), 0, stream, row, D);
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

fx_status launch_log_attack_times(hipStream_t stream, const float* energy, int C, int D, int S, int sample_rate, float* out)
{
    hipLaunchKernelGGL(log_attack_times_kernel, dim3((unsigned) C), dim3(NT), 0, stream, energy, D, S, D, sample_rate, out);
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

fx_status launch_scatter_rows(hipStream_t stream, const float* out4, const float* slope, const float* out3, int C, int D, float* features)
{
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks_for((long long) C * D)), dim3(NT), 0, stream, out4, slope, out3, C, D, features);
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

} // namespace fxo
