// fx_offline_files.hip -- the offline driver's kernels over a BANK of files (include/fx.h, fx_offline_analyse_files): C files of different
// lengths back to back, in any FX_SAMPLE_* wire format.  Nothing is computed here that fx_offline_frames.hip / fx_offline.hip do not
// compute: the frame (fx_offline_frame_body.hip.h), the zero-crossing count, the RMS of a step and the log attack time
// (fx_offline_steps.hip.h) are those units' own statements.  What differs is where a sample comes from -- widen_one of fx_samples.hip.h, the
// one statement of the formats, at byte (first_c + i) * sample_bytes of the bank -- and where a length does: S_c and step_c = S_c div D from
// the file's record (fxo::FileRecord, formed on the host), never an argument.
// Every sample is read by loads of its own width (one float, one 16-bit word, three bytes): no load touches a byte outside the bank, whatever
// the alignment of a file's start and wherever the last file ends.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>

#include "fx_kernels.h"
#include "fx_offline_frames.h"

#pragma clang fp contract(off)

namespace fxk {
#include "fx_wave.hip.h"          // f4
#include "fx_samples.hip.h"
} // namespace fxk

namespace fxo {
namespace {

constexpr int NT = 256;

#include "fx_plain_fft.hip.h"
#include "fx_offline_frame_body.hip.h"
#include "fx_offline_steps.hip.h"

// samples of one file from `at` on: a(i) = the widening of the sample i places behind it
template <int FMT> struct FileSamples {
    const unsigned char* at;
    __device__ __forceinline__ FileSamples(const void* bank, long long first) : at(static_cast<const unsigned char*>(bank) + first * fxk::sample_bytes(FMT)) {}
    __device__ __forceinline__ float operator()(long long i) const { return fxk::widen_one<FMT>(at + i * fxk::sample_bytes(FMT)); }
};

// block = (frame, file): blockIdx.x = (f - first_frame) * C + c
template <int N, int FMT>
__global__ void __launch_bounds__(NT) offline_frames_files_kernel(const void* __restrict__ bank, const FileRecord* __restrict__ files, int C, int D, int first_frame,
                                                                  const float* __restrict__ tw, float* __restrict__ mags, float* __restrict__ energy)
{
    constexpr int H = N / 2, B = N / 2 + 1;
    const int fl = blockIdx.x / C, c = blockIdx.x - fl * C, f = first_frame + fl;
    const FileRecord file = files[c];
    const long long start = D == 1 ? 0 : (long long) f * file.step - H;     // ref AudioAnalysis.h:150-161, with the file's own step
    frame_body<N>(FileSamples<FMT>(bank, file.first), file.S, start, tw, mags + ((size_t) fl * C + c) * B, energy ? energy + (size_t) c * D + f : nullptr);
}

// block = (file, downsample step)
template <int FMT>
__global__ void __launch_bounds__(NT) zero_crosses_files_kernel(const void* __restrict__ bank, const FileRecord* __restrict__ files, int D, float* __restrict__ row)
{
    const int c = blockIdx.x / D, i = blockIdx.x % D;
    const FileRecord file = files[c];
    zero_crosses_block(FileSamples<FMT>(bank, file.first + (long long) i * file.step), file.step, row + (size_t) c * D + i);
}

// lane = (file, downsample)
template <int FMT>
__global__ void __launch_bounds__(NT) rms_row_files_kernel(const void* __restrict__ bank, const FileRecord* __restrict__ files, int C, int D, float* __restrict__ row)
{
    const long long t = (long long) blockIdx.x * NT + threadIdx.x;
    if (t >= (long long) C * D) return;
    const int c = (int) (t / D), i = (int) (t - (long long) c * D);
    const FileRecord file = files[c];
    row[t] = rms_of_step(FileSamples<FMT>(bank, file.first + (long long) i * file.step), file.step);
}

// block = file, over the rows of energy [C][D]
__global__ void __launch_bounds__(NT) log_attack_times_files_kernel(const float* __restrict__ energy, const FileRecord* __restrict__ files, int D, float* __restrict__ out)
{
    const FileRecord file = files[blockIdx.x];
    log_attack_block(energy + (size_t) blockIdx.x * D, D, file.step, file.rate, out + blockIdx.x);
}

template <int FMT>
fx_status launch_frames_of(hipStream_t stream, const void* bank, const FileRecord* files, int C, int D, int n, int first, dim3 grid, const float* table,
                           float* m, float* energy)
{
    const dim3 block(NT);
    switch (n) {
        case 256:  hipLaunchKernelGGL((offline_frames_files_kernel<256, FMT>), grid, block, 0, stream, bank, files, C, D, first, table, m, energy); break;
        case 512:  hipLaunchKernelGGL((offline_frames_files_kernel<512, FMT>), grid, block, 0, stream, bank, files, C, D, first, table, m, energy); break;
        case 1024: hipLaunchKernelGGL((offline_frames_files_kernel<1024, FMT>), grid, block, 0, stream, bank, files, C, D, first, table, m, energy); break;
        case 2048: hipLaunchKernelGGL((offline_frames_files_kernel<2048, FMT>), grid, block, 0, stream, bank, files, C, D, first, table, m, energy); break;
        case 4096: hipLaunchKernelGGL((offline_frames_files_kernel<4096, FMT>), grid, block, 0, stream, bank, files, C, D, first, table, m, energy); break;
        default: return fx_fail(FX_ERR_INVALID_ARGUMENT, "window_size %d is not one of 256, 512, 1024, 2048, 4096", n);
    }
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

} // namespace

fx_status launch_frames_files(hipStream_t stream, const void* bank, const FileRecord* files, int format, int C, int D, int n, int first_frame,
                              int num_frames, const float* table, float* mags, float* energy)
{
    const int bins = n / 2 + 1;
    const int per_launch = (1 << 30) / C;                                   // the grid's x extent stays below 2^31
    for (int done = 0; done < num_frames; done += per_launch) {
        const int frames = num_frames - done < per_launch ? num_frames - done : per_launch;
        const dim3 grid((unsigned) ((long long) frames * C));
        float* m = mags + (size_t) done * C * bins;
        fx_status st = FX_OK;
        FX_FORMAT(format, st = launch_frames_of<FMT>(stream, bank, files, C, D, n, first_frame + done, grid, table, m, energy));
        if (st != FX_OK) return st;
    }
    return FX_OK;
}

fx_status launch_zero_crosses_files(hipStream_t stream, const void* bank, const FileRecord* files, int format, int C, int D, float* row)
{
    FX_FORMAT(format, hipLaunchKernelGGL(zero_crosses_files_kernel<FMT>, dim3((unsigned) (C * D)), dim3(NT), 0, stream, bank, files, D, row));
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

fx_status launch_rms_row_files(hipStream_t stream, const void* bank, const FileRecord* files, int format, int C, int D, float* row)
{
    const unsigned blocks = (unsigned) (((long long) C * D + NT - 1) / NT);
    FX_FORMAT(format, hipLaunchKernelGGL(rms_row_files_kernel<FMT>, dim3(blocks), dim3(NT), 0, stream, bank, files, C, D, row));
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

fx_status launch_log_attack_times_files(hipStream_t stream, const float* energy, const FileRecord* files, int C, int D, float* out)
{
    hipLaunchKernelGGL(log_attack_times_files_kernel, dim3((unsigned) C), dim3(NT), 0, stream, energy, files, D, out);
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

} // namespace fxo
