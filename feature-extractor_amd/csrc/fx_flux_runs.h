// fx_flux_runs.h -- how the 1024-point batch frame kernel (both analysers) shares a work unit's frames among a channel's wavefronts,
// and where in its own buffer each of them keeps the flux state.
// Plain constexpr functions, no HIP header needed: fx_frame_kernel.hip.h includes this file (inside namespace fxk) for the kernel and
// its static asserts, tests/cpp/flux_runs_host.cpp for a check of the split over every unit length and wavefront count.
#ifndef FX_FLUX_RUNS_H
#define FX_FLUX_RUNS_H
#if defined(__HIPCC__)
#define FX_FR_HD __host__ __device__
#else
#define FX_FR_HD
#endif

// A unit of n frames over k wavefronts: wavefront `slot` analyses the contiguous run [flux_run_begin(n, k, slot), flux_run_begin(n, k,
// slot + 1)) of the unit's frames.  The runs are in frame order, cover the unit exactly and differ in length by at most one (the first
// n % k are the longer ones); with n < k the last k - n wavefronts have nothing to do.  Inside a run the previous accepted spectrum of
// every frame but the first is the wavefront's own, so the flux state is handed over once per run instead of once per frame.
FX_FR_HD constexpr int flux_run_begin(int n, int k, int slot) { return slot * (n / k) + (slot < n % k ? slot : n % k); }
// the last wavefront that has a run: its flux image is the channel's state after the unit
FX_FR_HD constexpr int flux_last_slot(int n, int k) { return n < 1 ? 0 : (n < k ? n : k) - 1; }

// The wavefront's own flux image (bins image: re of the last accepted frame, BIMG floats) lies behind everything a section keeps in the
// wave's buffer, which since the second exchange is done by lane swaps no longer holds a complex image: the largest live images are the
// first exchange's rows and the real image.
//   buf_bytes: the wave's buffer; image_bytes: the bins image; live_bytes: the end of the largest image any section writes
struct FluxImagePlace {
    int offset_bytes;
    FX_FR_HD constexpr bool fits(int buf_bytes, int image_bytes, int live_bytes) const
    {
        return offset_bytes % 16 == 0 && offset_bytes >= live_bytes && offset_bytes + image_bytes <= buf_bytes;
    }
};
// 1024 points: 64 rows of 11 float2 (RealExchange) end at byte 5632, the real image at 5136, the harmonic scratch at 4112, the lag
// scan's plain image at 4096; the image's 3072 bytes end at 8704 of the buffer's 8720, and the int behind them is the wavefront's
// "run finished" flag.
constexpr FluxImagePlace FLUX_IMAGE_1024 = {5632};
#undef FX_FR_HD
#endif
