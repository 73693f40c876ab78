// The 1024-point transform's in-register second exchange (csrc/fx_lane_exchange.h), simulated on registers that hold their own
// label: 64 lanes x 16 elements, entry = (source lane, element).  The swaps are the ones the kernel issues (LaneExchange<1024>::swap)
// with the documented semantics of the two instructions; afterwards every last-pass operand must be the element the LDS exchange
// would have delivered.  Prints one line per failure; exit status 0 if there is none.
#include <cstdio>
#include <utility>

#include "../../feature-extractor_amd/csrc/fx_lane_exchange.h"

typedef LaneExchange<1024> LX;
struct Label { int lane, element; };

// v_permlane32_swap first, second: lanes 32-63 of `first` <-> lanes 0-31 of `second`
static void permlane32_swap(Label* first, Label* second)
{
    for (int l = 0; l < 32; l++) std::swap(first[32 + l], second[l]);
}
// v_permlane16_swap first, second: rows 1 and 3 of `first` <-> rows 0 and 2 of `second` (a row: 16 lanes)
static void permlane16_swap(Label* first, Label* second)
{
    for (int row = 1; row < 4; row += 2)
        for (int c = 0; c < 16; c++) std::swap(first[16 * row + c], second[16 * (row - 1) + c]);
}

int main()
{
    static Label reg[16][64];                          // reg[element][lane]
    for (int i = 0; i < 16; i++)
        for (int l = 0; l < 64; l++) reg[i][l] = Label{l, i};
    int swaps = 0;
    for (int stage = 0; stage < LX::STAGES; stage++)
        for (int j = 0; j < LX::SWAPS; j++, swaps++) {
            const LaneSwap s = LX::swap(stage, j);
            if (s.first < 0 || s.second > 15 || s.first >= s.second) { std::printf("stage %d swap %d: operands %d, %d\n", stage, j, s.first, s.second); return 1; }
            (stage == 0 ? permlane32_swap : permlane16_swap)(reg[s.first], reg[s.second]);
        }
    int bad = 0;
    for (int lane = 0; lane < 64; lane++)
        for (int g = 0; g < 4; g++)
            for (int ip = 0; ip < 4; ip++) {
                const Label got = reg[LX::register_of(g, ip)][lane];
                // the label the issue of record states, and the mapping functions the static asserts use
                const bool label = got.lane == 16 * ip + lane % 16 && got.element == lane / 16 + 4 * g
                                   && got.lane == LX::source_lane(lane, ip) && got.element == LX::source_element(lane, g);
                // the position the LDS path reads (fft_last_pass_fused, LazyLag::load) against the one fft_pass stores to
                const int it = got.lane, base = (it / 16) * 256 + it % 16;
                const bool position = cpad(lane + 64 * g) + item_off(256, ip) == cpad(base) + item_off(16, got.element)
                                      && LX::consumed_at(lane, g, ip) == LX::produced_at(got.lane, got.element);
                if (!label || !position) {
                    if (bad++ < 16) std::printf("lane %d butterfly %d operand %d: holds (lane %d, element %d)\n", lane, g, ip, got.lane, got.element);
                }
            }
    std::printf("%d swaps of register pairs (%d instructions), %d operands wrong\n", swaps, 2 * swaps, bad);
    return bad ? 1 : 0;
}
