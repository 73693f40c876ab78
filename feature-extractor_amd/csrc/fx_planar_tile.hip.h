// fx_planar_tile.hip.h -- the tile both byte movers share: PT_TRACKS planar rows of PT_FRAMES samples on their way to memory through
// LDS.  fx_deinterleave_kernel (fx_interleave.hip) and the RTP gather (fx_rtp.hip) each have a load stage of their own and call this
// header for everything after it.
//
// The load stage puts sample f of tile row r at byte m + f * B of the row (store_sample), m the byte the row's segment has in the
// planar block modulo 16.  The drain (tile_to_rows) reads whole 16-byte chunks back (ds_read_b128) and writes them to 16-byte
// aligned addresses (global_store_dwordx4), consecutive lanes along a row and on into the next one.  Only the first and last chunk
// of a row's segment are partial: they are written byte by byte, each byte once, whatever the row pitch n * B makes of the alignment.
//
// The index arithmetic is plain host/device functions, in the manner of fx_rtp_packet.h and fx_flux_runs.h, so that the stand-alone
// host program (tests/cpp/planar_tile_host.cpp) walks this one statement; the LDS reads and the global stores are device code.
#ifndef FX_PLANAR_TILE_HIP_H
#define FX_PLANAR_TILE_HIP_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FX_PT_FN __host__ __device__ constexpr
#else
#define FX_PT_FN constexpr
#endif

namespace fxk {

constexpr int PT_FRAMES = 64, PT_TRACKS = 64, PT_THREADS = 256;
static_assert(PT_THREADS == 4 * 64 && PT_TRACKS == 64, "lane = track, four wavefronts step through the positions");

// a row's segment of PT_FRAMES * B bytes, placed at its offset modulo 16
FX_PT_FN int pt_chunks(int B) { return PT_FRAMES * B / 16 + 1; }
FX_PT_FN int pt_row_bytes(int B) { return 16 * pt_chunks(B); }

// Byte `col` of tile row r: chunks of 16 bytes in order, the four dwords of a chunk rotated by (r / 8) % 4.  A row is 9 (2-byte
// samples), 13 (3) or 17 (4) chunks, 36, 52 or 68 dwords: on the 32 banks a store sees, row r starts at bank 4 r, 20 r or 4 r modulo
// 32, eight distinct multiples of 4 for r = 0 .. 7 and the same again for r + 8; the rotation moves those apart, so the load stage's
// stores (a group of 32 lanes = 32 rows at one sample) fall on 32 distinct banks where the rows' offsets modulo 16 agree, and on at
// most two lanes a bank where they do not.  The drain's reads of whole chunks are not affected.
FX_PT_FN int tile_at(int r, int row_bytes, int col)
{
    return r * row_bytes + (col & ~15) + ((((col >> 2) + (r >> 3)) & 3) << 2) + (col & 3);
}

// The bytes [lo, hi) of a row that its chunk k contributes, the row's nf samples of B bytes starting at byte m (0 .. 15): empty
// (lo >= hi) for a chunk outside the segment, 16 bytes for a whole one.
struct TileBytes {
    int lo, hi;
};
FX_PT_FN TileBytes tile_chunk_bytes(int k, int m, int nf, int B)
{
    return TileBytes{m > 16 * k ? m : 16 * k, m + nf * B < 16 * k + 16 ? m + nf * B : 16 * k + 16};
}

#if defined(__HIPCC__)

// (a row's offset modulo 16 is a multiple of B's alignment for 2- and 4-byte samples: those never straddle a dword of the tile)
template <int B> __device__ __forceinline__ void store_sample(unsigned char* tile, int r, int row_bytes, int col, unsigned v)
{
    if constexpr (B == 4) *reinterpret_cast<unsigned*>(tile + tile_at(r, row_bytes, col)) = v;
    else if constexpr (B == 2) *reinterpret_cast<unsigned short*>(tile + tile_at(r, row_bytes, col)) = (unsigned short) v;
    else {
#pragma unroll
        for (int i = 0; i < 3; i++) tile[tile_at(r, row_bytes, col + i)] = (unsigned char) (v >> (8 * i));
    }
}

__device__ __forceinline__ unsigned pick(const uint4& q, int j)
{
    j &= 3;
    return j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w;
}

// The tile's rows to out, [C] rows of row_bytes bytes (16-byte aligned): tracks c0 .. of the block's C, nf samples of B bytes from
// byte first_byte of each row.  All PT_THREADS threads of the workgroup, after the barrier that ends the load stage.
template <int B>
__device__ __forceinline__ void tile_to_rows(const unsigned char* tile, unsigned char* out, int c0, int C, long long row_bytes, long long first_byte, int nf)
{
    constexpr int CHUNKS = pt_chunks(B), ROW = pt_row_bytes(B);
    for (int i = threadIdx.x; i < PT_TRACKS * CHUNKS; i += PT_THREADS) {
        const int r = i / CHUNKS, k = i - r * CHUNKS, c = c0 + r;
        if (c >= C) break;                                  // (r only grows with i)
        const long long seg = (long long) c * row_bytes + first_byte;
        const int m = (int) (seg & 15);
        const TileBytes at = tile_chunk_bytes(k, m, nf, B);
        if (at.lo >= at.hi) continue;
        const uint4 s = *reinterpret_cast<const uint4*>(tile + r * ROW + 16 * k);
        const int rot = r >> 3;
        const uint4 q{pick(s, rot), pick(s, rot + 1), pick(s, rot + 2), pick(s, rot + 3)};
        unsigned char* dst = out + (seg - m) + 16 * k;
        if (at.hi - at.lo == 16) {
            *reinterpret_cast<uint4*>(dst) = q;
        } else {
            for (int b = at.lo - 16 * k; b < at.hi - 16 * k; b++) dst[b] = (unsigned char) (pick(q, b >> 2) >> (8 * (b & 3)));
        }
    }
}

#endif // __HIPCC__

} // namespace fxk

#undef FX_PT_FN
#endif
