// fx_offline_frames.h -- what fx_offline.hip's driver entries (fx_offline_frames / fx_offline_analyse, include/fx.h) launch from
// fx_offline_frames.hip.  Every pointer is device memory; every launch goes onto `stream` and returns once it is enqueued.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "fx_context.h"

namespace fxo {

inline bool known_window(int n) { return n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096; }
inline int window_slot(int n) { return n == 256 ? 0 : n == 512 ? 1 : n == 1024 ? 2 : n == 2048 ? 3 : 4; }

// the reference FFT's forward table [n][2] (JUCE 4.2 FFT::FFTConfig: phase in double, entries rounded to float)
std::vector<float> forward_table(int n);

// frames [first_frame, first_frame + num_frames) of every channel: window (ref AudioAnalysis.h:146-181), Bartlett gain (:667-676), forward
// transform, magnitudes to mags[((f - first_frame) * C + c) * (n / 2 + 1) + b], energy (or null) to energy[c * D + f]
fx_status launch_frames(hipStream_t stream, const float* audio, int C, int S, int D, int n, int first_frame, int num_frames, const float* table,
                        float* mags, float* energy);
// ref AudioFeatures.h:158-184 fillDownsampledRMSAudioChannels: audio [C][S] -> row [C][D]
fx_status launch_rms_row(hipStream_t stream, const float* audio, int C, int S, int D, float* row);
// ref AudioFeatures.h:186-195 normaliseAudioChannels, per channel: row [C][D] in place
fx_status launch_normalise_row(hipStream_t stream, float* row, int C, int D);
// ref AudioAnalysis.h:611-622 setLogAttackTime of each channel's energy row [C][D] -> out [C]
fx_status launch_log_attack_times(hipStream_t stream, const float* energy, int C, int D, int S, int sample_rate, float* out);
// the per-frame entries' results of D frames -- out4 [D][C][4], slope [D][C], out3 [D][C][3]; a null pointer = not computed -- into the rows
// of features [10][C][D] (ref AudioFeatures.h:133-140 setFeatureSample)
fx_status launch_scatter_rows(hipStream_t stream, const float* out4, const float* slope, const float* out3, int C, int D, float* features);

// ---- a bank of files (fx_offline_analyse_files): C files back to back in one FX_SAMPLE_* format, each with a record the host forms -- the
// device never divides by D.  Defined in fx_offline_files.hip; the arithmetic is the kernels' above (fx_offline_frame_body.hip.h,
// fx_offline_steps.hip.h), read through fx_samples.hip.h's widening with S_c, step_c and the file's rate in place of S, S div D and sample_rate.
struct FileRecord {
    long long first;        // index of the file's first sample in the bank
    int S;                  // its number of samples
    int step;               // S div D: the frames' step, the Audio row's spb, the attack time's samples_per_step
    int rate;               // its sample rate (0 unless the log attack time is asked for)
    int pad;
};
fx_status launch_frames_files(hipStream_t stream, const void* bank, const FileRecord* files, int format, int C, int D, int n, int first_frame,
                              int num_frames, const float* table, float* mags, float* energy);
fx_status launch_zero_crosses_files(hipStream_t stream, const void* bank, const FileRecord* files, int format, int C, int D, float* row);
fx_status launch_rms_row_files(hipStream_t stream, const void* bank, const FileRecord* files, int format, int C, int D, float* row);
fx_status launch_log_attack_times_files(hipStream_t stream, const float* energy, const FileRecord* files, int C, int D, float* out);

// what the driver analyses: audio [C][S] fp32 of one length and rate (files == null), or a bank of files
struct Source {
    const void* samples;            // device memory
    int S, sample_rate;             // audio [C][S]
    const FileRecord* files;        // [C], device memory
    int format;
};

} // namespace fxo
