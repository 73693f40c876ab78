// fx_samples.hip.h -- the sample formats on the wire, stated once: what a sample of each format widens to (one at a time, four at a
// time), how four of them are fetched, and the step from a run-time format to a template argument.  The frame, pair and hop kernels'
// load stage and every attached unit that reads samples (fx_taps.hip, fx_display.hip, fx_clips.hip, fx_monitor.hip) make the same
// floats of the same bytes because they all call these.  Bytes per sample: sample_bytes, fx_kernels.h (the host asks too).
// Included inside namespace fxk, after fx_wave.hip.h (f4); not a stand-alone header.

// Sample formats on the wire (FX_SAMPLE_*, include/fx.h): fp32, fp16, or signed PCM of 16 bits (v / 2^15) or 24 bits packed in three
// bytes, little endian (v / 2^23) -- exactly what the WAV reader makes of such files (include/fx_wav.hpp, JUCE's int -> float scaling:
// the sample left-justified in an int32, times 2^-31), so integer audio crosses PCIe at two / three bytes a sample and loses
// nothing.  The carried-over window tail is always fp32.
// a 24-bit sample left-justified in 32 bits -> float: 24 significant bits, so the conversion and the power-of-two scaling are exact
__device__ __forceinline__ float from_left_justified(unsigned w) { return (float) (int) w * (1.0f / 2147483648.0f); }
// LAST_USE: the frame's last read of its window (the split sizes fetch it three times): a non-temporal load, so that the L2 lets go of
// a window nobody will ask for again before it lets go of one that is between its reads.  The windows in flight on an XCD are about
// the size of its L2 at 4096 points; measured there (1024 channels x 64 whole frames): counter traffic 2.24 -> 1.53 x the algorithmic
// bytes, kernel 1.557 -> 1.548 ms; on overlapping hops 1.32 -> 1.21 x; 2048 points unchanged (profiles/r04_4096.txt (8)).
template <int FMT, bool LAST_USE = false> __device__ __forceinline__ float widen_one(const void* at)
{
    if (LAST_USE && FMT == FX_SAMPLE_F32) return __builtin_nontemporal_load(static_cast<const float*>(at));
    if (LAST_USE && FMT == FX_SAMPLE_S16) return (float) (int) __builtin_nontemporal_load(static_cast<const short*>(at)) * (1.0f / 32768.0f);
    if (LAST_USE && FMT == FX_SAMPLE_F16) return __half2float(__ushort_as_half(__builtin_nontemporal_load(static_cast<const unsigned short*>(at))));
    if (FMT == FX_SAMPLE_F16) return __half2float(*static_cast<const __half*>(at));
    if (FMT == FX_SAMPLE_S16) return (float) (int) *static_cast<const short*>(at) * (1.0f / 32768.0f);
    if (FMT == FX_SAMPLE_S24) {
        // (three byte loads: a packed sample starts at any byte, and a wider load at the last sample of a buffer would read past its end)
        const unsigned char* b = static_cast<const unsigned char*>(at);
        return from_left_justified(((unsigned) b[0] << 8) | ((unsigned) b[1] << 16) | ((unsigned) b[2] << 24));
    }
    return *static_cast<const float*>(at);
}
// four consecutive samples: r = the 16 bytes of four floats, (r.x, r.y) = the 8 bytes of four 16-bit samples, or (r.x, r.y, r.z) = the
// 12 bytes of four packed 24-bit samples
template <int FMT> __device__ __forceinline__ f4 widen_four(uint4 r)
{
    if (FMT == FX_SAMPLE_S24)
        return f4{from_left_justified(r.x << 8), from_left_justified((r.y << 16) | ((r.x >> 16) & 0xff00u)),
                  from_left_justified((r.z << 24) | ((r.y >> 8) & 0xffff00u)), from_left_justified(r.z & 0xffffff00u)};
    if (FMT == FX_SAMPLE_F16) {
        const float2 a = __half22float2(*reinterpret_cast<const __half2*>(&r.x));
        const float2 b = __half22float2(*reinterpret_cast<const __half2*>(&r.y));
        return f4{a.x, a.y, b.x, b.y};
    }
    if (FMT == FX_SAMPLE_S16) {
        const f4 v = f4{(float) ((int) (r.x << 16) >> 16), (float) ((int) r.x >> 16), (float) ((int) (r.y << 16) >> 16), (float) ((int) r.y >> 16)};
        return v * (1.0f / 32768.0f);                                          // exact: a power of two
    }
    return f4{__uint_as_float(r.x), __uint_as_float(r.y), __uint_as_float(r.z), __uint_as_float(r.w)};
}
template <int FMT> __device__ __forceinline__ uint4 fetch_four(const void* src, int i)       // samples i .. i + 3 of src
{
    if (FMT == FX_SAMPLE_F32) return *reinterpret_cast<const uint4*>(static_cast<const float*>(src) + i);
    if (FMT == FX_SAMPLE_S24) {             // i is a multiple of 4: twelve bytes from a 4-byte boundary
        const uint3 v = *reinterpret_cast<const uint3*>(static_cast<const unsigned char*>(src) + 3 * i);
        return uint4{v.x, v.y, v.z, 0u};
    }
    const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(src) + i);
    return uint4{v.x, v.y, 0u, 0u};
}
// run `CALL` with the constants FA / FB set to the formats of a window's two halves: fb is the call's sample format, fa is
// either the same or fp32 (the tail)
#define FX_FORMATS(fa, fb, CALL) do {                                                                                              \
        if ((fb) == FX_SAMPLE_F16)      { if ((fa) == FX_SAMPLE_F16) { constexpr int FA = FX_SAMPLE_F16, FB = FX_SAMPLE_F16; CALL; }   \
                                          else                       { constexpr int FA = FX_SAMPLE_F32, FB = FX_SAMPLE_F16; CALL; } } \
        else if ((fb) == FX_SAMPLE_S16) { if ((fa) == FX_SAMPLE_S16) { constexpr int FA = FX_SAMPLE_S16, FB = FX_SAMPLE_S16; CALL; }   \
                                          else                       { constexpr int FA = FX_SAMPLE_F32, FB = FX_SAMPLE_S16; CALL; } } \
        else if ((fb) == FX_SAMPLE_S24) { if ((fa) == FX_SAMPLE_S24) { constexpr int FA = FX_SAMPLE_S24, FB = FX_SAMPLE_S24; CALL; }   \
                                          else                       { constexpr int FA = FX_SAMPLE_F32, FB = FX_SAMPLE_S24; CALL; } } \
        else                            { constexpr int FA = FX_SAMPLE_F32, FB = FX_SAMPLE_F32; CALL; }                                \
    } while (0)
// run `CALL` with the constant FMT set to a run-time sample format; anything that is not one of the other three runs as fp32
#define FX_FORMAT(fmt, CALL) do {                                                         \
        switch (fmt) {                                                                    \
            case FX_SAMPLE_F16: { constexpr int FMT = FX_SAMPLE_F16; CALL; } break;       \
            case FX_SAMPLE_S16: { constexpr int FMT = FX_SAMPLE_S16; CALL; } break;       \
            case FX_SAMPLE_S24: { constexpr int FMT = FX_SAMPLE_S24; CALL; } break;       \
            default:            { constexpr int FMT = FX_SAMPLE_F32; CALL; } break;       \
        }                                                                                 \
    } while (0)
