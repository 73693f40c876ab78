// fx_lane_consts.hip.h -- LaneConsts<N, GROUPS>: what a lane of the 1024-point batch frame kernel derives from its lane number alone, formed
// once per wavefront in front of the frame loop and held in VGPRs, instead of once per frame behind every re-materialisation point.
// Included by fx_fft.hip.h (inside namespace fxk) behind the layouts it indexes: Geo, rimg / bimg, RealExchange, Plan, rev4.
//
// The kernel is bound by VALU issue since the second exchange went into registers, so an instruction that is not
// arithmetic on the frame's data is time.  Hoisting everything (no opaque() at all) needs 85 registers more than four waves per SIMD
// leave; the record is the selection made by hand: the values that take the most instructions to form per register they occupy.
// Measured (profiles/lane_consts_ab.txt, lane_consts_counters.txt): 2669 -> 2540 VALU instructions per frame, 2.594 -> 2.543 ms per
// 524 288 frames at the medians of five; each of the three groups of members is slower left out (2.557 / 2.548 / 2.554 ms without group
// 1 / 2 / 4); with the transparent top as well (all four) the kernel spills 16 B, so that one stays opaque.
// Every member is a function of the lane number and of the wave's LDS buffer / the workgroup's twiddle table only -- never of the
// channel, the chunk, the ticket or the frame index, which change under a wavefront in calls that are cut into time units.
//
// Groups (FX_EXP_LANE_CONSTS=<mask> builds a costing variant with just those groups: tools/build_variants.py small name=-DFX_EXP_LANE_CONSTS=5):
//   1 LCG_TRANSFORM  the first exchange's store row, the second pass's source address and conjugation mask, the second and last
//                   pass's twiddle addresses                                                                       (5 VGPRs, 4 transforms a frame)
//   2 LCG_REV        what hangs on rev4(lane): the first-pass read address in the real image, the ds_bpermute index of the power
//                   spectrum, the Bartlett base of the spectral window                                              (3 VGPRs)
//   4 LCG_IMAGES     the lane's places in the real image (frame load, low-pass) and in the bins image (last-pass stores, the lane's own
//                   run of bins), and the low-pass window's gain ramp                                               (6 VGPRs)
//   8 LCG_TOP        no members: the top of the frame loop (re-materialisation point 15) is transparent, and the compiler hoists what
//                   it finds there itself
enum { LCG_TRANSFORM = 1, LCG_REV = 2, LCG_IMAGES = 4, LCG_TOP = 8, LCG_ALL = 15 };

// The lane-number parts of the record as plain integers (float2 / float element offsets inside the wave's buffer or the twiddle
// table), constexpr so that the host pass of the compiler holds them to the expressions they replace for all 64 lanes (consistent()).
template <int N> struct LaneOffsets {
    typedef Geo<N> G;
    typedef RealExchange<N> RX;
    typedef Plan<N> PL;
    // LCG_TRANSFORM
    __host__ __device__ static constexpr int row(int lane) { return RX::row(lane); }                                       // fft_first_pass: slot 0 of the lane's item
    __host__ __device__ static constexpr int src(int lane) { return RX::row((lane / 16) * 16) + (int) ((RX::SLOT_OF >> (4 * (lane % 16))) & 15ull); }
    __host__ __device__ static constexpr unsigned flip(int lane) { return ((RX::TWIN >> (lane % 16)) & 1u) << 31; }
    __host__ __device__ static constexpr int tw1(int lane) { return PL::OFF1 + lane % PL::L1; }
    __host__ __device__ static constexpr int tw2(int lane) { return PL::OFF2 + lane; }
    // LCG_REV
    __host__ __device__ static constexpr int rev(int lane) { return rev4<G::IDIG>(lane); }
    __host__ __device__ static constexpr int rbase(int lane) { return rimg<N>(rev(lane)); }
    // LCG_IMAGES
    __host__ __device__ static constexpr int load_at(int lane) { return rimg<N>(4 * lane); }       // load_window: samples 256*q + 4*lane .. + 3
    __host__ __device__ static constexpr int own(int lane) { return rimg<N>(G::P * lane); }         // lowpass_window: the lane's own run of P samples
    __host__ __device__ static constexpr int bins(int lane) { return bimg<N>(G::U * lane); }        // the lane's own run of U bins
    __host__ __device__ static constexpr int bin_lane(int lane) { return bimg<N>(lane); }           // last pass: bin lane + 64*m

    // base-4 digit reversal, digit by digit (what rev4's bit tricks have to equal)
    __host__ __device__ static constexpr int rev_by_digits(int x)
    {
        int r = 0;
        for (int d = 0; d < G::IDIG; d++) { r = 4 * r + (x & 3); x >>= 2; }
        return r;
    }
    // Every use of the record is "member + compile-time constant" where the code without it forms an index from the lane number: the
    // two agree for all 64 lanes.  (The uses: fft_first_pass, fft_second_pass_regs, fft_last_pass_consume, LazyLag, load_window,
    // FrameWave::sum_squares / pitch / spectral / lowpass_window / harmonic_spectrum.)
    __host__ __device__ static constexpr bool consistent()
    {
        for (int lane = 0; lane < 64; lane++) {
            const int k = lane % 16;
            // second pass: element k of the first-pass items (lane / 16) * 16 + i sits SLOTS float2 apart, in its slot or its twin's
            int slot = -1;
            for (int q = 0; q < RX::SLOTS; q++)
                if (RX::stored(q) == k || (((RX::TWIN >> k) & 1u) && RX::stored(q) == (k == 12 ? 4 : 16 - k))) slot = q;
            if (slot < 0 || src(lane) != ((lane / 16) * 16) * RX::SLOTS + slot) return false;
            if (row(lane) != lane * RX::SLOTS || row(lane) + RX::SLOTS > cpad(N) + 2) return false;
            const bool twin = k == 3 || k == 7 || k == 11 || k == 12 || k == 15;
            if (flip(lane) != (twin ? 0x80000000u : 0u)) return false;
            if (tw1(lane) != k || tw2(lane) != 15 * 16 + lane || tw2(lane) + 64 * 3 + 2 * PL::L2 >= N) return false;
            // first-pass order: input j of the lane's item is sample rev4(lane) + ITEMS_A * r(j)
            if (rev(lane) != rev_by_digits(lane) || rev(lane) >= G::ITEMS_A) return false;
            for (int j = 0; j < G::RA; j++) {
                const int r = (j >> 2) + 4 * (j & 3);
                if (rbase(lane) + first_pass_rstep<N>(j) != rimg<N>(rev(lane) + G::ITEMS_A * r)) return false;
            }
            // frame load: 4 samples at 256*q + 4*lane of either half
            for (int q = 0; q < N / 512; q++)
                if (load_at(lane) + rimg_step<N>(256 * q) != rimg<N>(256 * q + 4 * lane)
                    || load_at(lane) + rimg_step<N>(N / 2 + 256 * q) != rimg<N>(N / 2 + 256 * q + 4 * lane)) return false;
            // low-pass: the lane's own P samples are contiguous, and so are the 16 warm-up samples in front of them (lanes > 0)
            for (int i = 0; i < G::P; i++)
                if (own(lane) + i != rimg<N>(G::P * lane + i)) return false;
            if (lane > 0)
                for (int i = 0; i < 16; i++)
                    if (own(lane) - warmup_back() + i != rimg<N>(G::P * lane - 16 + i)) return false;
            // bins image: the lane's own U bins and their neighbours; the last pass's bins lane + 64*m
            for (int j = 0; j < G::U; j++)
                if (bins(lane) + j != bimg<N>(G::U * lane + j)) return false;
            if (lane > 0 && (bins(lane) - left_back(2) != bimg<N>(G::U * lane - 2) || bins(lane) - left_back(1) != bimg<N>(G::U * lane - 1))) return false;
            if (lane < 63 && bins(lane) + right_step() != bimg<N>(G::U * lane + G::U)) return false;
            for (int m = 0; m < G::U; m++)
                if (bin_lane(lane) + bimg_step<N>(64 * m) != bimg<N>(lane + 64 * m)) return false;
        }
        return true;
    }
    // distances inside the padded images that the sections add to a member (compile-time constants)
    __host__ __device__ static constexpr int warmup_back() { return 16 + 4 * (16 / G::RQ); }          // 16 samples and the padding between them and the lane's run
    __host__ __device__ static constexpr int left_back(int n) { return n + (G::BQ ? 4 : 0); }       // bin U*lane - n, n <= U: one padding gap away
    __host__ __device__ static constexpr int right_step() { return G::U + (G::BQ ? 4 : 0); }        // bin U*lane + U
};
static_assert(LaneOffsets<1024>::consistent(), "LaneConsts: a member plus its section's constant is the index the section forms from the lane number");

#define FX_LC_TEXT_(x) #x
#define FX_LC_TEXT(x) FX_LC_TEXT_(x)
// (read as a constant expression like FX_EXP_LDS_EXCHANGE: spelled out, the macro's own name stands here when nothing defines it)
constexpr unsigned LANE_CONSTS_SHIPPED = LCG_TRANSFORM | LCG_REV | LCG_IMAGES;
constexpr unsigned LANE_CONSTS_GROUPS = lds_exchange_kinds(FX_LC_TEXT(FX_EXP_LANE_CONSTS), LANE_CONSTS_SHIPPED);
static_assert(LANE_CONSTS_GROUPS <= (unsigned) LCG_ALL, "FX_EXP_LANE_CONSTS: a mask of the four groups of members");

// GROUPS == 0: the form without a record (every other size and kernel); nothing reads a member then and none is ever formed.
template <int N, unsigned GROUPS = 0u> struct LaneConsts {
    static constexpr bool TRANSFORM = (GROUPS & LCG_TRANSFORM) != 0, REV = (GROUPS & LCG_REV) != 0, IMAGES = (GROUPS & LCG_IMAGES) != 0, TOP = (GROUPS & LCG_TOP) != 0;
    static_assert(GROUPS == 0u || N == 1024, "the record belongs to the 1024-point frame kernel");
    typedef LaneOffsets<N> O;
    // LCG_TRANSFORM
    f2*        row;         // cbuf + RealExchange<N>::row(lane): where fft_first_pass stores the lane's item
    const f2*  src;         // the second pass's first operand: row of first-pass item (lane / 16) * 16, slot of element lane % 16 (or of its twin)
    unsigned   flip;        // sign bit where that slot holds the twin (the conjugate)
    const f2*  tw1;         // tw + OFF1 + lane % 16: the second pass's twiddles
    const f2*  tw2;         // tw + OFF2 + lane: the last pass's
    // LCG_REV
    const float* rbase;     // rbuf + first_pass_rbase<N>(lane, 0)
    int        bperm;       // rev4(lane) << 2: the lane whose power spectrum this lane's next first pass consumes (ds_bpermute)
    float      base;        // Bartlett gain of sample rev4(lane)
    // LCG_IMAGES.  (`warm` and `left2` are the lowest address their sections touch, so that every access is the member plus an
    // immediate offset: a member minus a constant is an address of its own, which the compiler would form once and keep.)
    float*     load_at;     // rbuf + rimg(4 * lane)
    float*     warm;        // rbuf + rimg(P * lane) - O::warmup_back(): the low-pass's 16 warm-up samples, the lane's own run behind them
    float*     left2;       // fbuf + bimg(U * lane) - O::left_back(2): bin U*lane - 2; the lane's own run of bins O::left_back(2) further on
    float*     bin_lane;    // fbuf + bimg(lane)
    float      w0, wstep;   // bartlett_gain<N>(P * lane), and its step per sample inside the lane's run
    // A gain taken from the record goes through here where it is used: sixteen gains computed from a loop-invariant base are
    // loop-invariant themselves, and hoisted they are sixteen registers (one move per use instead).
    static __device__ __forceinline__ float fresh(float v) { asm volatile("" : "+v"(v)); return v; }

    __device__ __forceinline__ void form(int lane, f2* cbuf, const f2* tw)
    {
        float* rbuf = reinterpret_cast<float*>(cbuf);
        if constexpr (TRANSFORM) {
            row = cbuf + O::row(lane);
            src = cbuf + O::src(lane);
            flip = O::flip(lane);
            tw1 = tw + O::tw1(lane);
            tw2 = tw + O::tw2(lane);
        }
        if constexpr (REV) {
            rbase = rbuf + O::rbase(lane);
            bperm = O::rev(lane) << 2;
            base = (float) O::rev(lane) * (2.0f / N);
        }
        if constexpr (IMAGES) {
            load_at = rbuf + O::load_at(lane);
            warm = rbuf + O::own(lane) - O::warmup_back();
            left2 = rbuf + O::bins(lane) - O::left_back(2);
            bin_lane = rbuf + O::bin_lane(lane);
            w0 = bartlett_gain<N>(Geo<N>::P * lane);
            wstep = lane < 32 ? (2.0f / N) : -(2.0f / N);
        }
    }
};
