// fx_offline_steps.hip.h -- the offline driver's arithmetic over samples and envelopes, stated once: the zero-crossing count of one downsample
// step, the RMS of one step, the log attack time of one energy row.  The kernels over audio [C][S] of one length (fx_offline.hip,
// fx_offline_frames.hip) and the kernels over a bank of files (fx_offline_files.hip) call these; they differ in where a sample comes from
// and where a length does -- an argument, or the file's record.  `A` is a callable: a(s) = sample s of the run at hand, as a float.
// Included inside a unit's namespace, after its NT (threads per workgroup), under `#pragma clang fp contract(off)`; not a stand-alone header.
// "ref:" citations are relative to the reference's Source/.

// ref AudioAnalysis.h:534-535: does the signal cross zero between two neighbouring samples?
__device__ __forceinline__ bool is_zero_cross(float first, float second)
{
    const float d = first - second;
    return (first > 0.0f && d > first) || (first < 0.0f && d < first);
}

// ref AudioAnalysis.h:528-538, one downsample step of `step` samples by a whole workgroup: the integer count, then count * 2 / step
template <typename A> __device__ __forceinline__ void zero_crosses_block(const A& a, int step, float* out)
{
    __shared__ int s_cnt[NT / 64];
    int n = 0;
    for (int s = threadIdx.x; s < step - 1; s += NT)                       // :529
        if (is_zero_cross(a(s), a(s + 1))) n++;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < NT / 64; w++) total += s_cnt[w];
        *out = (float) total * 2.0f / (float) step;                        // :538 (a float count is exact below 2^24)
    }
}

// ref AudioFeatures.h:161-184, one downsample step of `spb` samples by one lane (getRMSLevel: float squares, double sum in sample order,
// sqrt of the double mean); with one sample per step the sample as it is (:165-172)
template <typename A> __device__ __forceinline__ float rms_of_step(const A& a, int spb)
{
    if (spb == 1) return a(0);
    double sum = 0.0;
    for (int s = 0; s < spb; s++) { const float x = a(s); sum += (double) (x * x); }
    return (float) sqrt(sum / (double) spb);
}

// ref AudioAnalysis.h:619-621: the first index holding the envelope's maximum, in milliseconds, as a logarithm
__device__ __forceinline__ float log_attack_time_of(int i, int samples_per_step, int sample_rate)
{
    const double ms_per_sample = 1.0 / (double) (sample_rate / 1000);      // :619 (sampleRate is an int: AudioFeatures.h:303)
    return (float) log10((double) (float) (i * samples_per_step) * (float) ms_per_sample);         // :621
}

// ref AudioAnalysis.h:611-622 setLogAttackTime of one envelope env[n] by a whole workgroup
__device__ __forceinline__ void log_attack_block(const float* env, int n, int samples_per_step, int sample_rate, float* out)
{
    __shared__ float s_max[NT];
    __shared__ int s_idx[NT];
    float m = -__builtin_huge_valf();
    bool any = false;
    // findMinMax (...).getEnd(), :615: the maximum starts from env[0] and moves on `>` only, so a NaN anywhere but at 0 is skipped -- here too, or one
    // early in a thread's stride would hide the maxima behind it (as in auto_correlation_kernel); a NaN at env[0] is thread 0's business
    for (int k = threadIdx.x; k < n; k += NT) { const float v = env[k]; if (v == v && (!any || v > m)) { m = v; any = true; } }
    s_max[threadIdx.x] = any ? m : -__builtin_huge_valf();                 // (-inf never moves the maximum)
    __syncthreads();
    if (threadIdx.x == 0) { float mm = env[0]; for (int k = 0; k < NT; k++) if (s_max[k] > mm) mm = s_max[k]; s_max[0] = mm; }      // a NaN at 0 stays: it equals no entry, i = n
    __syncthreads();
    const float max_energy = s_max[0];
    int first = n;                                                         // first index holding the maximum, :616-618
    for (int k = threadIdx.x; k < n; k += NT) if (env[k] == max_energy) { first = k; break; }
    s_idx[threadIdx.x] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        int i = n;
        for (int k = 0; k < NT; k++) if (s_idx[k] < i) i = s_idx[k];
        *out = log_attack_time_of(i, samples_per_step, sample_rate);
    }
}
