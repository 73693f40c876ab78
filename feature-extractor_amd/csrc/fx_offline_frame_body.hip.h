// fx_offline_frame_body.hip.h -- one frame of the offline driver by one workgroup, stated once: the window (ref AudioAnalysis.h:146-181),
// the Bartlett gain (:667-676), the forward transform, the magnitudes in bin order, the serial energy sum.  offline_frames_kernel
// (fx_offline_frames.hip: audio [C][S] of one length) and offline_frames_files_kernel (fx_offline_files.hip: a bank of files in a wire
// format) run it; they differ in what a(i) reads and in where S comes from.
// Included inside a unit's namespace after fx_plain_fft.hip.h and the unit's NT; not a stand-alone header.

// a(i), 0 <= i < S: sample i of the channel as a float.  start: the sample under j = 0.  energy_at: where the frame's energy goes, or null.
template <int N, typename A>
__device__ __forceinline__ void frame_body(const A& a, int S, long long start, const float* __restrict__ tw, float* __restrict__ out, float* energy_at)
{
    constexpr int H = N / 2, B = N / 2 + 1;
    __shared__ cpx buf[N];
    __shared__ float mag[B];
    using P = PlainPlan<N>;
    const int tid = threadIdx.x;
    for (int j = tid; j < N; j += NT) {
        const long long i = start + j;                                      // :167
        const float v = (i >= 0 && i < S) ? a(i) : 0.0f;                    // :169-177: zero padding for the ends
        // scaleBufferWithBartlettWindowing (:667-676): two gain ramps, each gain the float sum of the increments 1 / H before it -- exact
        const float w = j < H ? (float) j * (2.0f / N) : 2.0f - (float) j * (2.0f / N);
        buf[P::position(j)] = cpx{v * w, 0.0f};                             // (always multiplied: inf * 0 = NaN, as applyGainRamp makes it)
    }
    __syncthreads();
    plain_transform<N, false, NT>(buf, tw);
    // performFrequencyOnlyForwardTransform, as tools/refdiff/juce_standin.h states it: sqrt (re * re + im * im) in float, bins 0 .. N / 2
    for (int b = tid; b < B; b += NT) {
        const cpx x = buf[b];
        const float m = sqrtf(x.r * x.r + x.i * x.i);
        mag[b] = m;
        out[b] = m;
    }
    if (!energy_at) return;
    __syncthreads();
    if (tid == 0) {                                                         // sumAccrossChannels (:705-716) of one channel: serial, in float
        float e = 0.0f;
#pragma unroll 8
        for (int b = 0; b < B; b++) e += mag[b];
        *energy_at = e;                                                     // :249
    }
}
