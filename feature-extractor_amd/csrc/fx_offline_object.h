// fx_offline_object.h -- the object behind include/fx.h's fx_offline_* entries, shared by the units that implement them
// (fx_offline.hip: the per-frame entries and the driver; fx_offline_stats.hip: what is derived from a feature buffer).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "fx_context.h"
#include "fx_offline_frames.h"

struct fx_offline {
    int device = 0;
    int C = 0;
    double nyquist = 24000.0;           // as created; each channel's own value is h_nyquist / d_nyquist
    hipStream_t stream = nullptr;
    double* d_prev_f0 = nullptr;        // [C] previousF0 of each channel's analyser (ref AudioAnalysis.h:109,293,697)
    double* d_prev_bins = nullptr;      // [C][prev_bins] previousBinMagnitudes of each channel's analyser (ref :120-121,510,700); null until first used
    int     prev_bins = 0;
    void*   d_in = nullptr;  size_t in_cap = 0;      // staging for host buffers
    void*   d_out = nullptr; size_t out_cap = 0;
    // the offline driver (fx_offline_frames / fx_offline_analyse)
    float*  d_table[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};    // the forward table of each window size, made on first use
    void*   d_scratch = nullptr; size_t scratch_cap = 0;                   // magnitudes of one chunk of frames, when the caller keeps none; the sort keys of one group of long rows
    void*   d_work = nullptr; size_t work_cap = 0;                         // the per-frame results of a call [D][C][4 | 1 | 3], an energy envelope nobody asked for
    // per-channel tables the host forms and the kernels read: each goes up from its host copy on the stream, and `staged` marks the last
    // such copy -- the host copies are rewritten only after it (fx_offline_wait_staged), never under a copy in flight
    std::vector<double> h_nyquist;      double* d_nyquist = nullptr;       // [C] nyquistFrequency of each channel's analyser (ref AudioAnalysis.h:107)
    std::vector<fxo::FileRecord> h_files; fxo::FileRecord* d_files = nullptr;  // [C] fx_offline_analyse_files' records, null until first used
    hipEvent_t staged = nullptr;
    // each channel's SmoothedFeatures (ref AudioFeatures.h:356-421; fx_offline_smoothing): null until constructed
    float*  d_smooth_current = nullptr;                                    // [9][C] currentFeatureValues
    float*  d_smooth_history = nullptr;                                    // [9][C][smooth_depth] featureHistory, oldest first
    int     smooth_depth = 0;
};
