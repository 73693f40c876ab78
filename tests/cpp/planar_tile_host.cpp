// planar_tile_host.cpp -- the index arithmetic of csrc/fx_planar_tile.hip.h on the host, under AddressSanitizer and UBSan
// (tests/test_planar_tile_cpu.py builds and runs it).  For every sample width B, every offset m modulo 16 that a row of B-byte samples
// can have, every count nf = 1 .. PT_FRAMES and rows on both sides of a rotation step: the samples' bytes go to a tile by tile_at, as
// store_sample puts them, and come back chunk by chunk as tile_to_rows takes them -- the chunk's dwords un-rotated by r >> 3, its
// bytes [lo, hi) of tile_chunk_bytes.  Every byte of [m, m + nf * B) must arrive exactly once with its value, and none outside.
// Then the header's bank claim: at one column, 32 consecutive rows of equal m fall on 32 distinct banks.
//   stdout:   <B> <cases>            per width
//             <cases> cases, <columns> columns on distinct banks
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../feature-extractor_amd/csrc/fx_planar_tile.hip.h"

using namespace fxk;

static unsigned char value_of(int f, int i) { return (unsigned char) (1 + (f * 7 + i * 83) % 255); }      // never 0

static int fail(const char* what, int B, int m, int nf, int r, int at)
{
    printf("FAILED: %s (B %d, m %d, nf %d, row %d, byte %d)\n", what, B, m, nf, r, at);
    return 1;
}

static int one_case(int B, int m, int nf, int r)
{
    const int CHUNKS = pt_chunks(B), ROW = pt_row_bytes(B);
    std::vector<unsigned char> tile((size_t) PT_TRACKS * ROW, 0), want((size_t) ROW, 0), got((size_t) ROW, 0);
    std::vector<int> placed((size_t) PT_TRACKS * ROW, 0), written((size_t) ROW, 0);
    // the load stage: sample f's byte i at byte m + f * B + i of row r
    for (int f = 0; f < nf; f++)
        for (int i = 0; i < B; i++) {
            const int col = m + f * B + i, at = tile_at(r, ROW, col);
            if (at < r * ROW || at >= (r + 1) * ROW) return fail("tile_at leaves the row", B, m, nf, r, col);
            if (placed[(size_t) at]++) return fail("two bytes at one place of the tile", B, m, nf, r, col);
            tile[(size_t) at] = want[(size_t) col] = value_of(f, i);
        }
    // the drain
    for (int k = 0; k < CHUNKS; k++) {
        const TileBytes at = tile_chunk_bytes(k, m, nf, B);
        if (at.lo >= at.hi) continue;
        if (at.lo < 16 * k || at.hi > 16 * k + 16) return fail("a chunk's bytes outside the chunk", B, m, nf, r, at.lo);
        unsigned s[4], q[4];
        memcpy(s, &tile[(size_t) r * ROW + 16 * k], 16);
        for (int j = 0; j < 4; j++) q[j] = s[(j + (r >> 3)) & 3];
        for (int b = at.lo - 16 * k; b < at.hi - 16 * k; b++) {            // (a whole chunk: the same sixteen bytes as one store)
            unsigned char bytes[4];
            memcpy(bytes, &q[b >> 2], 4);
            got[(size_t) 16 * k + b] = bytes[b & 3];
            written[(size_t) 16 * k + b]++;
        }
    }
    for (int b = 0; b < ROW; b++) {
        const bool inside = b >= m && b < m + nf * B;
        if (written[(size_t) b] != (inside ? 1 : 0)) return fail(inside ? "a byte of the segment not written once" : "a byte outside the segment written", B, m, nf, r, b);
        if (inside && got[(size_t) b] != want[(size_t) b]) return fail("a byte arrives with another's value", B, m, nf, r, b);
    }
    return 0;
}

int main()
{
    static_assert(pt_chunks(2) == 9 && pt_chunks(3) == 13 && pt_chunks(4) == 17, "the row pitches the header's bank comment speaks of");
    const int rows[] = {0, 7, 8, 63};
    long long cases = 0, columns = 0;
    for (int B = 2; B <= 4; B++) {
        const int step = B == 3 ? 1 : B;                // a row's offset modulo 16 is a multiple of B's alignment
        long long mine = 0;
        for (int m = 0; m < 16; m += step)
            for (int nf = 1; nf <= PT_FRAMES; nf++)
                for (int r : rows) {
                    if (one_case(B, m, nf, r)) return 1;
                    mine++;
                }
        printf("%d %lld\n", B, mine);
        cases += mine;
        // 32 consecutive rows (a store's lane group) at one column: 32 distinct banks of (byte address / 4) % 32
        const int ROW = pt_row_bytes(B);
        for (int m = 0; m < 16; m += step)
            for (int col = m; col < m + PT_FRAMES * B; col++)
                for (int r0 = 0; r0 + 32 <= PT_TRACKS; r0++) {
                    unsigned seen = 0;
                    for (int r = r0; r < r0 + 32; r++) seen |= 1u << ((tile_at(r, ROW, col) / 4) % 32);
                    if (seen != 0xffffffffu) return fail("32 rows at one column share a bank", B, m, PT_FRAMES, r0, col);
                    columns++;
                }
    }
    printf("%lld cases, %lld columns on distinct banks\n", cases, columns);
    return 0;
}
