// fx_lane_exchange.h -- positions inside the padded complex image, and the second exchange of the 1024-point transform
// as lane swaps: which element of which lane every last-pass operand is, and the swaps that bring it there.
// Plain constexpr functions, no HIP header needed: fx_fft.hip.h includes this file (inside namespace fxk) for the kernels and
// their static asserts, tests/cpp/lane_exchange_host.cpp for a simulation of the swaps on labelled registers.
#if defined(__HIPCC__)
#define FX_LX_HD __host__ __device__
#else
#define FX_LX_HD
#endif

// complex image: position p at p + (p >> 4) (one float2 of padding per 16)
FX_LX_HD constexpr int cpad(int p) { return p + (p >> 4); }

// offset of element i of an item inside the padded complex image, relative to cpad(base):
// cpad(base + L0*i) - cpad(base) is a compile-time constant because base = blk*(R*L0) + k, k < L0
FX_LX_HD constexpr int item_off(int L0, int i) { return L0 * i + (L0 >= 16 ? (L0 / 16) * i : ((L0 * i) >> 4)); }

// The second exchange of the un-split 1024-point transform (plan 16 x 16 x 4) without LDS.
//   produced: after the second pass lane `it` holds the 16 elements of item `it`, element i at position (it/16)*256 + it%16 + 16*i
//   consumed: the last pass wants, in lane `lane`, the operands ip = 0..3 of butterfly lane + 64*g: positions lane + 64*g + 256*ip
// so operand (lane, g, ip) is element lane/16 + 4*g of lane 16*ip + lane%16: inside every group of lanes {r, r+16, r+32, r+48} and
// every group of elements {4g .. 4g+3} a 4 x 4 transpose between "row of 16 lanes" and "element index mod 4".  Two stages of
// register-pair swaps do it in place -- v_permlane32_swap exchanges the high bit of the row with the high bit of the element index,
// v_permlane16_swap the low bits -- after which the operand sits in the consuming lane's register e[4*g + ip].
struct LaneSwap { int first, second; };             // indices into e[16] of one swap's two operands (each an f2: two dwords)
template <int N> struct LaneExchange {
    static constexpr bool AVAILABLE = N == 1024;
    static constexpr int STAGES = 2, SWAPS = 8;     // swaps of register pairs per stage
    // padded position of element i of second-pass item `it` / of operand ip of last-pass butterfly lane + 64*g (what the LDS path writes and reads)
    FX_LX_HD static constexpr int produced_at(int it, int i) { return cpad((it / 16) * 256 + it % 16) + item_off(16, i); }
    FX_LX_HD static constexpr int consumed_at(int lane, int g, int ip) { return cpad(lane + 64 * g) + item_off(256, ip); }
    // the same operand as (lane, element) of the second pass's registers
    FX_LX_HD static constexpr int source_lane(int lane, int ip) { return 16 * ip + lane % 16; }
    FX_LX_HD static constexpr int source_element(int lane, int g) { return lane / 16 + 4 * g; }
    // where the swaps leave it in the consuming lane
    FX_LX_HD static constexpr int register_of(int g, int ip) { return 4 * g + ip; }
    // swap j of a stage.  Stage 0 is v_permlane32_swap (lanes 32-63 of `first` <-> lanes 0-31 of `second`) on elements 2 apart,
    // stage 1 v_permlane16_swap (rows 1 and 3 of `first` <-> rows 0 and 2 of `second`) on neighbouring elements.
    FX_LX_HD static constexpr LaneSwap swap(int stage, int j)
    {
        return stage == 0 ? LaneSwap{4 * (j / 2) + j % 2, 4 * (j / 2) + j % 2 + 2} : LaneSwap{4 * (j / 2) + 2 * (j % 2), 4 * (j / 2) + 2 * (j % 2) + 1};
    }
    // every operand of every lane really is the position the last pass reads
    FX_LX_HD static constexpr bool consistent()
    {
        for (int lane = 0; lane < 64; lane++)
            for (int g = 0; g < 4; g++)
                for (int ip = 0; ip < 4; ip++)
                    if (produced_at(source_lane(lane, ip), source_element(lane, g)) != consumed_at(lane, g, ip)) return false;
        return true;
    }
};
static_assert(LaneExchange<1024>::consistent(), "operand (lane, g, ip) of the last pass is element lane/16 + 4g of lane 16*ip + lane%16");
