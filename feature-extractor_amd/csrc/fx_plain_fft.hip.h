// fx_plain_fft.hip.h -- the reference FFT's butterfly DAG as plain code: the single statement of the transform whose bits define this
// library (JUCE 4.2 kiss-style radix-4/2 decimation in time, table twiddles, no fused multiply-add), one butterfly per thread and level
// through LDS.  The analysis taps (fx_taps.hip, forward and inverse) and the offline frame kernel (fx_offline_frames.hip, forward) run
// it; the hot path's register FFT (fx_fft.hip.h) computes the same DAG in another schedule.
// Included inside a unit's namespace, under `#pragma clang fp contract(off)`; not a stand-alone header.

// The reference FFT's factorisation of N (oracle/fx_oracle.c fft_cfg_init): radix 4 while it divides, then one radix 2.  Level k (0 = the
// outermost call of the recursion) has twiddle stride 4^k, and each of its butterflies spans length(k) points.
template <int N> struct PlainPlan {
    static constexpr int LOG = N == 256 ? 8 : N == 512 ? 9 : N == 1024 ? 10 : N == 2048 ? 11 : 12;
    static constexpr int R4 = LOG / 2;
    static constexpr int LEVELS = R4 + (LOG & 1);
    static __device__ __forceinline__ int radix(int k) { return k < R4 ? 4 : 2; }
    static __device__ __forceinline__ int stride(int k) { return 1 << (2 * k); }
    static __device__ __forceinline__ int length(int k) { return N / (stride(k) * radix(k)); }
    // the input element that lands at position p of the output before the butterflies (the leaves of the recursion)
    static __device__ __forceinline__ int source(int p)
    {
        int idx = 0;
        for (int k = 0; k < LEVELS; k++) {
            const int L = length(k), j = p / L;
            p -= j * L;
            idx += j * stride(k);
        }
        return idx;
    }
    // source()'s inverse: where input sample j stands before the butterflies -- its digits, level by level, most significant first
    static __device__ __forceinline__ int position(int j)
    {
        int p = 0;
#pragma unroll
        for (int k = 0; k < LEVELS; k++) p += ((j >> (2 * k)) & (radix(k) - 1)) * length(k);
        return p;
    }
};

struct cpx { float r, i; };
__device__ __forceinline__ cpx c_mul(cpx a, cpx b) { return cpx{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
__device__ __forceinline__ cpx c_add(cpx a, cpx b) { return cpx{a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ cpx c_sub(cpx a, cpx b) { return cpx{a.r - b.r, a.i - b.i}; }
// entry j of the forward table [N][2]; the inverse uses its conjugate
template <bool INV> __device__ __forceinline__ cpx tw_at(const float* tw, int j)
{
    const float2 t = reinterpret_cast<const float2*>(tw)[j];
    return cpx{t.x, INV ? -t.y : t.y};
}

// The butterflies of every level, innermost first, over buf (already in leaf order), by a workgroup of THREADS: fft_butterfly4 /
// fft_butterfly2 of the oracle, operation for operation.  Ends behind a barrier.
template <int N, bool INV, int THREADS> __device__ void plain_transform(cpx* buf, const float* tw)
{
    using P = PlainPlan<N>;
    for (int k = P::LEVELS - 1; k >= 0; k--) {
        const int r = P::radix(k), s = P::stride(k), L = P::length(k);
        for (int q = threadIdx.x; q < N / r; q += THREADS) {
            const int b = q / L, i = q - b * L;
            cpx* d = buf + b * r * L + i;
            if (r == 4) {
                const cpx s0 = c_mul(d[L], tw_at<INV>(tw, i * s));
                const cpx s1 = c_mul(d[2 * L], tw_at<INV>(tw, 2 * i * s));
                const cpx s2 = c_mul(d[3 * L], tw_at<INV>(tw, 3 * i * s));
                const cpx s3 = c_add(s0, s2), s4 = c_sub(s0, s2), s5 = c_sub(d[0], s1);
                const cpx d0 = c_add(d[0], s1);
                d[2 * L] = c_sub(d0, s3);
                d[0] = c_add(d0, s3);
                if (INV) {
                    d[L] = cpx{s5.r - s4.i, s5.i + s4.r};
                    d[3 * L] = cpx{s5.r + s4.i, s5.i - s4.r};
                } else {
                    d[L] = cpx{s5.r + s4.i, s5.i - s4.r};
                    d[3 * L] = cpx{s5.r - s4.i, s5.i + s4.r};
                }
            } else {
                const cpx t = c_mul(d[L], tw_at<INV>(tw, i * s));
                d[L] = c_sub(d[0], t);
                d[0] = c_add(d[0], t);
            }
        }
        __syncthreads();
    }
}
