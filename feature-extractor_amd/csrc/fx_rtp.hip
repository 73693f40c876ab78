// fx_rtp.hip -- RTP audio in: a tick's L16 / L24 datagrams unpacked to the planar block on the GPU (include/fx.h, fx_rtp_configure /
// fx_push_rtp).
//
// Audio in the numbers this library is built for arrives over the network (AES67, ST 2110-30, Ravenna): RTP datagrams whose payload
// is big-endian signed PCM, a few channels interleaved per stream, a few dozen sample times per packet.  A receiver collects a tick's
// datagrams in slots of one stride and says which stream each came from; this unit does the rest on the device, as a pure function
// of what it was given: fx_rtp_parse_kernel judges every header (fx_rtp_packet.h), places the packet against its stream's cursor and
// claims the tick positions it covers in an owner table [S][n] (integer atomicMax: the packet of the greatest index wins, whatever
// order the wavefronts run in); fx_rtp_gather_kernel forms the planar block [C][n] that fx_push_samples takes -- track c's row is
// channel j of stream s, byte-reversed to little endian, zeros where no packet owns the position -- and fx_rtp_count_kernel adds the
// tick's owned and missing positions to the per-stream statistics.  fx_push_block (fx_capi.cpp) does the rest: the same launches, the
// same bits as fx_push_samples of that planar block.  Integer atomics only: every result is the same at every run.
//
// The reorder window (fx_rtp_set_window, W > 0 sample times): a tick works on a span of n + W positions, and what its packets own
// beyond the tick stays on the device until the tick that covers it.  Per stream the held state is a ring of W sample times of WIRE
// bytes (stream-interleaved, big-endian, as they arrived: the gather reads a held sample with the load_reversed it uses on a slot) and
// a 64-bit stamp per ring position: 0 = empty, else (tick number << 32) | (packet index + 1), claimed with atomicMax, so the most
// recently submitted packet owns a position whatever order the wavefronts run in.  Span position q lives in ring slot
// (head + q) % W, head moving on by n per tick.  The far end of the span, positions [max(n, W), n + W), has the ring slots of the
// positions [.., n) this tick consumes: those claims go to a per-tick table behind the owner table (`far`, min(n, W) entries a
// stream, filled with it), and the order of the launches does the rest --
//   fill, fx_rtp_parse_span_kernel   claims: [0, n) in the owner table, [n, W) in the stamps, the far end in `far`
//   fx_rtp_gather_span_kernel        reads the slots and, where no packet of the tick owns a position, the ring
//   fx_rtp_count_span_kernel         counts, and one thread per consumed ring slot replaces its stamp by the far claim (or 0)
//   fx_rtp_deposit_kernel            writes the bytes of the held positions the tick's packets own into the ring
// -- so the gather has read a slot's bytes and the count its stamp before either is overwritten: the ring needs no spare capacity,
// for any n (n > W: everything held is consumed and the whole carry is new).  With W == 0 a tick takes the path above, unchanged.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: fx_rtp_configure installs the context's release hook.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"
#include "fx_rtp_packet.h"
#include "fx_planar_tile.hip.h"

namespace fxk {

struct RtpStream {          // a row of the stream table
    int      channels;      // 1 .. 64
    unsigned origin;        // running: the cursor of a tick is origin + RtpTick::advanced (mod 2^32)
    int      running;
};
struct RtpTrack {           // a row of the track table: what track c hears
    int stream;             // -1: none, the track hears zeros
    int channel;
};
struct RtpRecord {          // what the parse leaves of packet i for the gather; read only where the owner table names i
    int payload;            // the payload's offset in the slot
    int d0;                 // the tick position of its first sample time
};
static_assert(sizeof(fx_rtp_stats) == 6 * sizeof(long long), "the statistics are six counters per stream, accumulated as such");
enum { ST_PACKETS = 0, ST_MALFORMED, ST_LATE, ST_EARLY, ST_PLACED, ST_MISSING, ST_FIELDS };

struct RtpTick {
    const unsigned char* slots;     // [P][stride], 4-byte aligned
    const int*           lengths;   // [P], 0 .. stride
    const int*           stream_of; // [P], 0 .. S - 1
    const RtpStream*     streams;   // [S]
    const RtpTrack*      tracks;    // [C]
    RtpRecord*           records;   // [P]
    int*                 owner;     // [S][n]: -1, or the greatest index of a packet that covers the position
    unsigned char*       disposition;   // [P] or null
    unsigned long long*  stats;     // [S][ST_FIELDS]
    unsigned char*       out;       // [C][n] samples of B bytes, 16-byte aligned
    int                  P, stride, S, C, n;
    int                  B;         // bytes per sample: 2 (L16) or 3 (L24)
    unsigned             advanced;  // samples per stream of the ticks before this one (mod 2^32)
};

struct RtpHeldRange {       // packet i's span positions beyond the tick, [lo, hi); empty: none (not HELD, or no valid packet of a running stream)
    int lo, hi;
};
enum { WS_HELD = 0, WS_RECOVERED, WS_FIELDS };

struct RtpSpan {            // a tick with a reorder window
    RtpTick              t;         // t.owner: [S][n], the tick's own positions
    int*                 far;       // [S][E], E = min(n, W): as owner, for the span positions [max(n, W), n + W)
    RtpHeldRange*        held;      // [P]
    unsigned char*       ring;      // the streams' rings of wire bytes
    const long long*     ring_base; // [S]: the byte at which stream s's ring of W * F bytes starts, a multiple of 4
    unsigned long long*  stamps;    // [S][W]
    unsigned long long*  wstats;    // [WS_FIELDS][S]
    int                  W, E;
    int                  head;      // span position q has ring slot (head + q) % W
    unsigned             tick;      // this tick's number, from 1
};

__device__ __forceinline__ unsigned long long span_stamp(unsigned tick, int i) { return ((unsigned long long) tick << 32) | (unsigned) (i + 1); }
__device__ __forceinline__ int span_slot(const RtpSpan& p, int q) { return (int) (((unsigned) p.head + (unsigned) q) % (unsigned) p.W); }

struct SlotBytes {
    const unsigned char* at;
    __device__ unsigned operator()(int k) const { return at[k]; }
};

// One wavefront per packet.  Every lane forms the same few values from the same header bytes (uniform loads); the lanes then spread
// along the positions the packet covers.  Lane 0 leaves the record, the disposition and the packet's counts.
// (One body for both forms of the tick, as rtp_gather below: Span = nullptr_t without a reorder window, const RtpSpan* with one.  The
// packet is then placed in the span of n + W positions and claims each covered position where that part of the span keeps its owners
// (the unit's header comment).  A position of [n, W) whose stamp was 0 is newly held: counted here; the far end's and the consumed
// positions' share of `held` is the count's.)
template <typename Span>
__device__ __forceinline__ void rtp_parse(const RtpTick& p, Span w)
{
    constexpr bool WINDOW = !std::is_same<Span, std::nullptr_t>::value;
    const int lane = threadIdx.x & 63, i = (int) blockIdx.x * 4 + (int) (threadIdx.x >> 6);
    if (i >= p.P) return;
    const int s = p.stream_of[i], len = p.lengths[i];
    const RtpStream st = p.streams[s];
    unsigned long long* stats = p.stats + (size_t) s * ST_FIELDS;
    fx_rtp_parsed h;
    unsigned bits;
    [[maybe_unused]] RtpHeldRange keep{0, 0};
    if (!fx_rtp_parse(SlotBytes{p.slots + (size_t) i * (size_t) p.stride}, len, st.channels * p.B, &h)) {
        bits = FX_RTP_BIT_MALFORMED;
        if (lane == 0) atomicAdd(&stats[ST_MALFORMED], 1ull);
    } else if (!st.running) {
        bits = FX_RTP_BIT_IGNORED;
        if (lane == 0) atomicAdd(&stats[ST_PACKETS], 1ull);
    } else {
        int W = 0;
        if constexpr (WINDOW) W = w->W;
        const fx_rtp_span_placement at = fx_rtp_place_span(h.timestamp, st.origin + p.advanced, h.sample_times, p.n, W);
        bits = at.bits;
        const int lo = (int) at.lo, hi = (int) at.hi;       // (n + W fits an int: the host saw to it)
        int* owner = p.owner + (size_t) s * (size_t) p.n;
        if constexpr (!WINDOW) {
            for (int q = lo + lane; q < hi; q += 64) atomicMax(&owner[q], i);
        } else {
            const int far0 = p.n > W ? p.n : W;
            int* far = w->far + (size_t) s * (size_t) w->E;
            unsigned long long* stamps = w->stamps + (size_t) s * (size_t) W;
            const unsigned long long mine = span_stamp(w->tick, i);
            int fresh = 0;
            for (int q = lo + lane; q < hi; q += 64) {
                if (q < p.n) atomicMax(&owner[q], i);
                else if (q >= far0) atomicMax(&far[q - far0], i);
                else fresh += atomicMax(&stamps[span_slot(*w, q)], mine) == 0ull;
            }
            if (bits & FX_RTP_BIT_HELD) keep = RtpHeldRange{lo > p.n ? lo : p.n, hi};
            if (p.n < W) {                                      // (uniform: only then is there a part [n, W))
                for (int d = 32; d > 0; d >>= 1) fresh += __shfl_xor(fresh, d);
                if (lane == 0 && fresh) atomicAdd(&w->wstats[(size_t) WS_HELD * p.S + s], (unsigned long long) fresh);
            }
        }
        if (lane == 0) {
            p.records[i] = RtpRecord{h.payload, at.d0};
            atomicAdd(&stats[ST_PACKETS], 1ull);
            const bool in_span = bits & (FX_RTP_BIT_PLACED | FX_RTP_BIT_HELD);          // (HELD: only ever with a window)
            if (!in_span && (bits & FX_RTP_BIT_LATE)) atomicAdd(&stats[ST_LATE], 1ull);
            if (!in_span && (bits & FX_RTP_BIT_EARLY)) atomicAdd(&stats[ST_EARLY], 1ull);
        }
    }
    if (lane == 0) {
        if constexpr (WINDOW) w->held[i] = keep;
        if (p.disposition) p.disposition[i] = (unsigned char) bits;
    }
}

__global__ void __launch_bounds__(256)
fx_rtp_parse_kernel(const RtpTick p)
{
    rtp_parse(p, nullptr);
}

__global__ void __launch_bounds__(256)
fx_rtp_parse_span_kernel(const RtpSpan w)
{
    rtp_parse(w.t, &w);
}

// The B bytes (1 .. 4) at byte `at` of `base`, first byte lowest; what lies above them is whatever follows.  They lie inside one
// datagram, and a slot starts and ends on a dword boundary (as a stream's ring does, with a dword of slack behind it), so the one or
// two aligned dwords around them lie inside the slot: no wide load that could cross the end of the slots' memory.
template <int B> __device__ __forceinline__ unsigned load_bytes(const unsigned char* base, long long at)
{
    const unsigned sh = (unsigned) at & 3u;
    const unsigned* w = reinterpret_cast<const unsigned*>(base + (at - sh));
    const unsigned lo = w[0], hi = sh + B > 4 ? w[1] : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

// a big-endian sample of B bytes there, as the little-endian sample in the low bytes (one v_perm_b32 and a shift)
template <int B> __device__ __forceinline__ unsigned load_reversed(const unsigned char* base, long long at)
{
    return __builtin_bswap32(load_bytes<B>(base, at)) >> (32 - 8 * B);
}

// A workgroup takes PT_FRAMES positions of PT_TRACKS consecutive tracks.  Load: lane = track, wavefront = position, so a wavefront
// reads, of every stream its tracks hear, one sample time of one packet: F contiguous bytes where consecutive tracks hear consecutive
// channels, and the sample time after it four steps later.  The owner and the record are the same address for all lanes of a stream
// (one request).  The samples go to the tile of fx_planar_tile.hip.h and from there to the planar rows.
// (One body for both forms of the tick: Span = const RtpSpan* with a reorder window -- a position no packet of the tick owns is then
// read from the stream's ring where its stamp says it is held -- and nullptr_t without, which is the kernel as it was.)
constexpr int PT_GROUP = 8;
static_assert((PT_FRAMES / 4) % PT_GROUP == 0, "four wavefronts step through the positions, PT_GROUP at a time");
template <int B, typename Span>
__device__ __forceinline__ void rtp_gather(const RtpTick& p, Span w)
{
    constexpr int ROW = pt_row_bytes(B);
    constexpr bool WINDOW = !std::is_same<Span, std::nullptr_t>::value;
    __shared__ __attribute__((aligned(16))) unsigned char tile[PT_TRACKS * ROW];
    const int q0 = (int) blockIdx.x * PT_FRAMES;
    const int c0 = (int) blockIdx.y * PT_TRACKS;
    const int nq = p.n - q0 < PT_FRAMES ? p.n - q0 : PT_FRAMES;

    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = c0 + lane;
        if (c < p.C) {
            const int m = (int) (((long long) c * p.n * B + (long long) q0 * B) & 15);
            const RtpTrack t = p.tracks[c];
            const int F = t.stream >= 0 ? p.streams[t.stream].channels * B : 0;
            const int* owner = p.owner + (size_t) (t.stream >= 0 ? t.stream : 0) * (size_t) p.n + q0;
            const bool heard = t.stream >= 0;
            [[maybe_unused]] const unsigned long long* stamps = nullptr;     // the stream's stamps and its ring (a 4-byte aligned base)
            [[maybe_unused]] const unsigned char* ring = nullptr;
            if constexpr (WINDOW) {
                if (heard) {
                    stamps = w->stamps + (size_t) t.stream * (size_t) w->W;
                    ring = w->ring + w->ring_base[t.stream];
                }
            }
            // PT_GROUP positions at a time, each of the three dependent loads (owner, record, sample) for all of them before the next
#pragma unroll 1
            for (int j0 = 0; j0 < PT_FRAMES / 4; j0 += PT_GROUP) {
                int own[PT_GROUP];
                RtpRecord rec[PT_GROUP];
                unsigned v[PT_GROUP];
#pragma unroll
                for (int g = 0; g < PT_GROUP; g++) {
                    const int f = wave + 4 * (j0 + g);
                    own[g] = heard && f < nq ? owner[f] : -1;
                }
                // (the stamps beside the owners, not behind them: a position's stamp is asked for whether or not a packet owns it)
                [[maybe_unused]] int slot[PT_GROUP];
                if constexpr (WINDOW) {
                    unsigned long long stamp[PT_GROUP];
#pragma unroll
                    for (int g = 0; g < PT_GROUP; g++) {
                        const int f = wave + 4 * (j0 + g);
                        slot[g] = heard && f < nq && q0 + f < w->W ? span_slot(*w, q0 + f) : -1;
                        stamp[g] = slot[g] >= 0 ? stamps[slot[g]] : 0ull;
                    }
#pragma unroll
                    for (int g = 0; g < PT_GROUP; g++)
                        if (own[g] >= 0 || stamp[g] == 0ull) slot[g] = -1;
                }
#pragma unroll
                for (int g = 0; g < PT_GROUP; g++) rec[g] = own[g] >= 0 ? p.records[own[g]] : RtpRecord{0, 0};
#pragma unroll
                for (int g = 0; g < PT_GROUP; g++) {
                    const int f = wave + 4 * (j0 + g);
                    v[g] = own[g] >= 0 ? load_reversed<B>(p.slots, (long long) own[g] * p.stride + rec[g].payload + (long long) (q0 + f - rec[g].d0) * F + t.channel * B) : 0u;
                    if constexpr (WINDOW)
                        if (slot[g] >= 0) v[g] = load_reversed<B>(ring, (long long) slot[g] * F + t.channel * B);
                }
#pragma unroll
                for (int g = 0; g < PT_GROUP; g++) {
                    const int f = wave + 4 * (j0 + g);
                    if (f < nq) store_sample<B>(tile, lane, ROW, m + f * B, v[g]);
                }
            }
        }
    }
    __syncthreads();

    tile_to_rows<B>(tile, p.out, c0, p.C, (long long) p.n * B, (long long) q0 * B, nq);
}

template <int B>
__global__ void __launch_bounds__(PT_THREADS)
fx_rtp_gather_kernel(const RtpTick p)
{
    rtp_gather<B>(p, nullptr);
}

template <int B>
__global__ void __launch_bounds__(PT_THREADS)
fx_rtp_gather_span_kernel(const RtpSpan w)
{
    rtp_gather<B>(w.t, &w);
}

// Owned and missing positions of the tick, per running stream: workgroup (s, y) steps through the stream's row of the owner table,
// every wavefront counts by ballot and adds its sums once.
// (One body for both forms of the tick.  With a reorder window a position of the tick is owned through a packet of the tick or,
// failing that, through the held state (recovered).  The thread of a position q < E = min(n, W) is also the only one that touches
// ring slot (head + q) % W in this launch: it has read the stamp of the position the tick consumes, and leaves the stamp of the
// far-end position that takes the slot over -- Q = q + W for n < W, else the one Q of [n, n + W) with Q = q modulo W -- or 0.
// `held` moves by the difference.)
template <typename Span>
__device__ __forceinline__ void rtp_count(const RtpTick& p, Span w)
{
    constexpr bool WINDOW = !std::is_same<Span, std::nullptr_t>::value;
    const int s = (int) blockIdx.x;
    if (!p.streams[s].running) return;
    const int* owner = p.owner + (size_t) s * (size_t) p.n;
    int owned = 0, seen = 0;
    [[maybe_unused]] int recovered = 0, gained = 0, lost = 0;
    for (int q0 = (int) blockIdx.y * 256; q0 < p.n; q0 += 256 * (int) gridDim.y) {
        const int q = q0 + (int) threadIdx.x;
        const bool in = q < p.n;
        seen += __popcll(__ballot(in));
        const bool own = in && owner[q] >= 0;
        if constexpr (!WINDOW) {
            owned += __popcll(__ballot(own));
        } else {
            bool was = false, next = false;
            if (in && q < w->E) {
                unsigned long long* stamp = w->stamps + (size_t) s * (size_t) w->W + span_slot(*w, q);
                was = *stamp != 0ull;
                int k = q;
                if (p.n >= w->W) { k = (q - p.n) % w->W; if (k < 0) k += w->W; }
                const int i = w->far[(size_t) s * (size_t) w->E + k];
                next = i >= 0;
                *stamp = next ? span_stamp(w->tick, i) : 0ull;
            }
            owned += __popcll(__ballot(own || was));
            recovered += __popcll(__ballot(was && !own));
            gained += __popcll(__ballot(next));
            lost += __popcll(__ballot(was));
        }
    }
    if ((threadIdx.x & 63) == 0 && seen) {
        unsigned long long* stats = p.stats + (size_t) s * ST_FIELDS;
        atomicAdd(&stats[ST_PLACED], (unsigned long long) owned);
        atomicAdd(&stats[ST_MISSING], (unsigned long long) (seen - owned));
        if constexpr (WINDOW) {
            if (recovered) atomicAdd(&w->wstats[(size_t) WS_RECOVERED * p.S + s], (unsigned long long) recovered);
            if (gained != lost) atomicAdd(&w->wstats[(size_t) WS_HELD * p.S + s], (unsigned long long) (long long) (gained - lost));   // (wraps to the sum)
        }
    }
}

__global__ void __launch_bounds__(256)
fx_rtp_count_kernel(const RtpTick p)
{
    rtp_count(p, nullptr);
}

__global__ void __launch_bounds__(256)
fx_rtp_count_span_kernel(const RtpSpan w)
{
    rtp_count(w.t, &w);
}

// Bytes [r0, r1) of stream s's ring (ring slots [r0 / F, r1 / F), which hold the span positions from qa on) from byte `src` of the
// slots on, by one wavefront; position q's bytes only where packet i owns q.  Lane by lane one aligned dword of the ring: written
// whole, from the shifted read, where all four bytes lie in the run and packet i owns the (one or two: F >= 2) positions they belong
// to, else byte by byte -- a neighbouring position may be another packet's, whose wavefront writes its bytes of the same dword.
__device__ __forceinline__ void deposit_run(const RtpSpan& w, int s, int i, int F, int lane, int r0, int r1, int qa, long long src)
{
    const RtpTick& p = w.t;
    unsigned char* ring = w.ring + w.ring_base[s];
    const int far0 = p.n > w.W ? p.n : w.W;
    const unsigned long long mine = span_stamp(w.tick, i);
    const auto owns = [&](int q) {
        return q >= far0 ? w.far[(size_t) s * (size_t) w.E + (q - far0)] == i : w.stamps[(size_t) s * (size_t) w.W + span_slot(w, q)] == mine;
    };
    const int slot0 = r0 / F;
    for (int a = (r0 & ~3) + 4 * lane; a < r1; a += 4 * 64) {
        const int b0 = a > r0 ? a : r0, b1 = a + 4 < r1 ? a + 4 : r1;
        const int first = b0 / F, last = (b1 - 1) / F;
        const bool own_first = owns(qa + (first - slot0)), own_last = last == first ? own_first : owns(qa + (last - slot0));
        if (b1 - b0 == 4 && own_first && own_last) {
            *reinterpret_cast<unsigned*>(ring + a) = load_bytes<4>(p.slots, src + (a - r0));
        } else {
            for (int b = b0; b < b1; b++)
                if (b / F == first ? own_first : own_last) ring[b] = p.slots[src + (b - r0)];
        }
    }
}

// One wavefront per packet: the span positions beyond the tick that the packet covers are one run of bytes in its slot and one or two
// in the ring, which wraps at W.  After the gather and the count of the same tick (the unit's header comment).
__global__ void __launch_bounds__(256)
fx_rtp_deposit_kernel(const RtpSpan w)
{
    const RtpTick& p = w.t;
    const int lane = threadIdx.x & 63, i = (int) blockIdx.x * 4 + (int) (threadIdx.x >> 6);
    if (i >= p.P) return;
    const RtpHeldRange keep = w.held[i];
    if (keep.lo >= keep.hi) return;
    const int s = p.stream_of[i], F = p.streams[s].channels * p.B;
    const RtpRecord rec = p.records[i];
    const long long src = (long long) i * p.stride + rec.payload + (long long) (keep.lo - rec.d0) * F;
    const int at = span_slot(w, keep.lo), count = keep.hi - keep.lo;                // count <= W
    const int head = count < w.W - at ? count : w.W - at;
    deposit_run(w, s, i, F, lane, at * F, (at + head) * F, keep.lo, src);
    if (head < count) deposit_run(w, s, i, F, lane, 0, (count - head) * F, keep.lo + head, src + (long long) head * F);
}

// Before the tick number would wrap: every held position's stamp becomes the least one, which any later claim beats.
__global__ void __launch_bounds__(256)
fx_rtp_rebase_stamps_kernel(unsigned long long* stamps, long long count)
{
    const long long k = (long long) blockIdx.x * 256 + threadIdx.x;
    if (k < count && stamps[k] != 0ull) stamps[k] = 1ull;
}

// A tick's fill and launches, in the order the unit's header comment gives; w: the tick's span (w->t is p), null without a window.
hipError_t launch_rtp_kernels(const RtpTick& p, const RtpSpan* w /* null: no window */, hipStream_t stream)
{
    const long long gx = ((long long) p.n + PT_FRAMES - 1) / PT_FRAMES, gy = ((long long) p.C + PT_TRACKS - 1) / PT_TRACKS;
    if (gy > 65535) return hipErrorInvalidValue;
    // (owner and far are one allocation, [S][n] then [S][E]; no window: no far end)
    hipError_t e = hipMemsetAsync(p.owner, 0xff, sizeof(int) * (size_t) p.S * ((size_t) p.n + (size_t) (w ? w->E : 0)), stream);
    if (e != hipSuccess) return e;
    const dim3 packets((unsigned) ((p.P + 3) / 4)), tiles((unsigned) gx, (unsigned) gy);
    const dim3 rows((unsigned) p.S, (unsigned) (gx < 16 ? (gx + 3) / 4 : 4));
    const auto stages = [&](auto parse, auto gather2, auto gather3, auto count, const auto& arg) {
        const auto gather = p.B == 2 ? gather2 : gather3;
        if (p.P > 0) hipLaunchKernelGGL(parse, packets, dim3(256), 0, stream, arg);
        hipLaunchKernelGGL(gather, tiles, dim3(PT_THREADS), 0, stream, arg);
        hipLaunchKernelGGL(count, rows, dim3(256), 0, stream, arg);
    };
    if (!w) {
        stages(fx_rtp_parse_kernel, fx_rtp_gather_kernel<2>, fx_rtp_gather_kernel<3>, fx_rtp_count_kernel, p);
    } else {
        stages(fx_rtp_parse_span_kernel, fx_rtp_gather_span_kernel<2>, fx_rtp_gather_span_kernel<3>, fx_rtp_count_span_kernel, *w);
        if (p.P > 0) hipLaunchKernelGGL(fx_rtp_deposit_kernel, packets, dim3(256), 0, stream, *w);
    }
    return hipGetLastError();
}

} // namespace fxk

// The reorder window's device state: nothing of it exists while window == 0.  It is allocated whole by fx_rtp_set_window and never by
// a tick, so no tick's growing buffer can drop what is held.
struct fx_rtp_window {
    int      window = 0;                        // W
    int      head = 0;                          // the ring slot of the next tick's position 0
    unsigned tick_no = 1;                       // the next tick's number in the stamps
    unsigned char*      ring = nullptr;         // every stream's ring: W * channels * B bytes from a 4-byte boundary, 4 bytes of slack behind
    long long*          ring_base = nullptr;    // [S]
    unsigned long long* stamps = nullptr;       // [S][W]
    unsigned long long* wstats = nullptr;       // [2][S]: held, recovered
};

static void rtp_window_free(fx_rtp_window* w)
{
    fx_free_device({w->ring, w->ring_base, w->stamps, w->wstats});
    *w = fx_rtp_window();
}

// *out (empty on entry): a window of W > 0 sample times for these streams of B-byte samples, nothing held; a failure leaves it empty
static fx_status rtp_window_alloc(fx_rtp_window* out, const std::vector<fxk::RtpStream>& streams, int W, int B)
{
    const size_t S = streams.size();
    std::vector<long long> base;
    try {
        base.resize(S);
    } catch (const std::bad_alloc&) {
        return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    long long ring_bytes = 0;
    for (size_t k = 0; k < S; k++) {                    // each ring from a dword boundary, a dword of slack behind it
        base[k] = ring_bytes;
        ring_bytes += (((long long) W * streams[k].channels * B + 3) & ~3ll) + 4;
    }
    const size_t stamp_bytes = sizeof(unsigned long long) * S * (size_t) W, wstats_bytes = sizeof(unsigned long long) * fxk::WS_FIELDS * S;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&out->ring), (size_t) ring_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&out->ring_base), sizeof(long long) * S);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&out->stamps), stamp_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&out->wstats), wstats_bytes);
    if (e == hipSuccess) e = hipMemset(out->ring, 0, (size_t) ring_bytes);
    if (e == hipSuccess) e = hipMemset(out->stamps, 0, stamp_bytes);
    if (e == hipSuccess) e = hipMemset(out->wstats, 0, wstats_bytes);
    if (e == hipSuccess) e = hipMemcpy(out->ring_base, base.data(), sizeof(long long) * S, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        rtp_window_free(out);
        return fx_fail(fx_hip_status(e), "allocating a reorder window of %d sample times failed: %s", W, hipGetErrorString(e));
    }
    out->window = W;
    return FX_OK;
}

struct fx_rtp {
    int format = FX_RTP_L16;                    // FX_RTP_L16 / FX_RTP_L24
    std::vector<fxk::RtpStream> streams;        // [S]: the host's copy of the stream table
    std::vector<fxk::RtpTrack>  tracks;         // [C]
    unsigned advanced = 0;                      // samples per stream of all ticks so far (mod 2^32)
    int      last_n = 0;                        // the last tick's samples per track: what fx_rtp_get_block copies
    fxk::RtpStream* d_streams = nullptr;
    fxk::RtpTrack*  d_tracks = nullptr;
    unsigned long long* d_stats = nullptr;      // [S][6]
    // a tick's lengths and stream numbers, [2][P] ints: two lists in turn, each with the event of its last upload, so that a tick
    // fills one while the upload of the tick before may still read the other
    fx_staged_list meta[2];
    hipEvent_t     meta_done[2] = {nullptr, nullptr};
    int            meta_cur = 0;
    unsigned char* d_slots = nullptr;           // a host tick's datagrams
    unsigned char* d_disposition = nullptr;     // a host tick's disposition bytes before they go to the caller
    fxk::RtpRecord* d_records = nullptr;
    int*           d_owner = nullptr;
    unsigned char* d_planar = nullptr;          // the planar block handed to fx_push_block
    size_t slots_cap = 0, disposition_cap = 0, records_cap = 0, owner_cap = 0, planar_cap = 0;
    fx_rtp_window win;                          // the reorder window (fx_rtp_set_window)
    fxk::RtpHeldRange*  d_held = nullptr;       // [P], a tick's scratch with a window
    size_t held_cap = 0;

    int bytes() const { return format == FX_RTP_L16 ? 2 : 3; }
    int sample_format() const { return format == FX_RTP_L16 ? FX_SAMPLE_S16 : FX_SAMPLE_S24; }
};

namespace {

void rtp_release(fx_context* c)
{
    fx_rtp* s = c->rtp;
    if (!s) return;
    fx_free_device({s->d_streams, s->d_tracks, s->d_stats, s->d_slots, s->d_disposition, s->d_records, s->d_owner, s->d_planar, s->d_held});
    rtp_window_free(&s->win);
    for (int k = 0; k < 2; k++) {
        fx_release_list(&s->meta[k]);
        if (s->meta_done[k]) (void) hipEventDestroy(s->meta_done[k]);
    }
    delete s;
    c->rtp = nullptr;
}

fx_status rtp_configured(const fx_context* c, fx_rtp** out)
{
    if (!c->rtp) return fx_fail(FX_ERR_INVALID_ARGUMENT, "RTP input is not configured on this context (fx_rtp_configure)");
    *out = c->rtp;
    return FX_OK;
}

// the host's stream table to the device; the stream is idle
fx_status upload_streams(fx_rtp* s)
{
    HIP_TRY(hipMemcpy(s->d_streams, s->streams.data(), s->streams.size() * sizeof(fxk::RtpStream), hipMemcpyHostToDevice));
    return FX_OK;
}

} // namespace

extern "C" {

fx_status fx_rtp_configure(fx_context* c, int payload_format, int num_streams, const int* channels)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (payload_format != FX_RTP_L16 && payload_format != FX_RTP_L24) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown payload format %d", payload_format);
    if (num_streams < 0 || num_streams > FX_RTP_MAX_STREAMS)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d streams: a context takes 0 (none) to %d", num_streams, FX_RTP_MAX_STREAMS);
    if (num_streams > 0 && !channels) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null channel counts with %d streams", num_streams);
    for (int k = 0; k < num_streams; k++)
        if (channels[k] < 1 || channels[k] > FX_RTP_MAX_CHANNELS)
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "channels[%d] = %d: a stream carries 1 to %d channels", k, channels[k], FX_RTP_MAX_CHANNELS);
    if (num_streams == 0 && !c->rtp) return FX_OK;
    { const fx_status ds = fx_require_device(); if (ds != FX_OK) return ds; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // ticks in flight read the tables
    if (num_streams == 0) {
        rtp_release(c);
        return FX_OK;
    }
    // the new unit whole, then the old one goes: a failure leaves the context as it was
    fx_rtp* s = new (std::nothrow) fx_rtp();
    if (!s) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    fx_rtp* const old = c->rtp;
    c->rtp = s;                                         // (rtp_release frees what c->rtp names)
    const auto give_up = [&](fx_status st) { rtp_release(c); c->rtp = old; return st; };
    try {
        s->streams.resize((size_t) num_streams);
        s->tracks.assign((size_t) c->C, fxk::RtpTrack{-1, 0});
    } catch (const std::bad_alloc&) {
        return give_up(fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed"));
    }
    for (int k = 0; k < num_streams; k++) s->streams[(size_t) k] = fxk::RtpStream{channels[k], 0u, 0};
    s->format = payload_format;
    const size_t stream_bytes = sizeof(fxk::RtpStream) * (size_t) num_streams, track_bytes = sizeof(fxk::RtpTrack) * (size_t) c->C;
    const size_t stats_bytes = sizeof(fx_rtp_stats) * (size_t) num_streams;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_streams), stream_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->d_tracks), track_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->d_stats), stats_bytes);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&s->meta_done[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemcpy(s->d_streams, s->streams.data(), stream_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_tracks, s->tracks.data(), track_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(s->d_stats, 0, stats_bytes);
    if (e != hipSuccess) return give_up(fx_fail(fx_hip_status(e), "allocating the RTP tables failed: %s", hipGetErrorString(e)));
    c->rtp = old;
    rtp_release(c);
    c->rtp = s;
    c->rtp_release = rtp_release;
    return FX_OK;
}

fx_status fx_rtp_set_track_sources(fx_context* c, const int* tracks, int num_tracks, const int* stream, const int* channel)
{
    fx_status st = fx_check_channel_list(c, tracks, num_tracks);
    if (st != FX_OK || num_tracks == 0) return st;
    if (!stream || !channel) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null source list with %d entries", num_tracks);
    fx_rtp* s = nullptr;
    if ((st = rtp_configured(c, &s)) != FX_OK) return st;
    for (int i = 0; i < num_tracks; i++) {
        if (stream[i] == -1) continue;
        if (stream[i] < 0 || stream[i] >= (int) s->streams.size())
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: stream %d out of range [0,%d) (-1: none)", i, stream[i], (int) s->streams.size());
        if (channel[i] < 0 || channel[i] >= s->streams[(size_t) stream[i]].channels)
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: channel %d of stream %d, which carries %d", i, channel[i], stream[i], s->streams[(size_t) stream[i]].channels);
    }
    if ((st = fx_check_channel_entries(c, tracks, num_tracks)) != FX_OK) return st;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<fxk::RtpTrack> next;
    try {
        next = s->tracks;
    } catch (const std::bad_alloc&) {
        return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    for (int i = 0; i < num_tracks; i++) next[(size_t) tracks[i]] = fxk::RtpTrack{stream[i], stream[i] == -1 ? 0 : channel[i]};
    // ticks already pushed read the old table on the device: they finish before it is replaced
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(s->d_tracks, next.data(), next.size() * sizeof(fxk::RtpTrack), hipMemcpyHostToDevice));
    s->tracks.swap(next);
    return fx_clear_pending_channels(c, tracks, num_tracks);
}

fx_status fx_rtp_get_track_sources(fx_context* c, int* stream, int* channel)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    fx_rtp* s = nullptr;
    { const fx_status st = rtp_configured(c, &s); if (st != FX_OK) return st; }
    for (int t = 0; t < c->C; t++) {
        if (stream) stream[t] = s->tracks[(size_t) t].stream;
        if (channel) channel[t] = s->tracks[(size_t) t].channel;
    }
    return FX_OK;
}

fx_status fx_rtp_set_cursors(fx_context* c, const int* streams, int num, const unsigned* timestamp)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (num < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative stream count %d", num);
    if (num == 0) return FX_OK;
    if (!streams || !timestamp) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null stream or timestamp list with %d entries", num);
    fx_rtp* s = nullptr;
    { const fx_status st = rtp_configured(c, &s); if (st != FX_OK) return st; }
    for (int i = 0; i < num; i++)
        if (streams[i] < 0 || streams[i] >= (int) s->streams.size())
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: stream %d out of range [0,%d)", i, streams[i], (int) s->streams.size());
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < num; i++) {
        fxk::RtpStream& r = s->streams[(size_t) streams[i]];
        r.origin = timestamp[i] - s->advanced;
        r.running = 1;
    }
    if (s->win.window > 0) {
        // the listed streams' time base has moved: what they hold goes, run of consecutive streams by run
        std::vector<int> listed;
        try {
            listed.assign(streams, streams + num);
        } catch (const std::bad_alloc&) {
            return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
        }
        std::sort(listed.begin(), listed.end());
        for (size_t a = 0; a < listed.size();) {
            size_t b = a + 1;
            while (b < listed.size() && listed[b] <= listed[b - 1] + 1) b++;
            const size_t first = (size_t) listed[a], rows = (size_t) (listed[b - 1] - listed[a] + 1);
            HIP_TRY(hipMemset(s->win.stamps + first * (size_t) s->win.window, 0, rows * (size_t) s->win.window * sizeof(unsigned long long)));
            HIP_TRY(hipMemset(s->win.wstats + (size_t) fxk::WS_HELD * s->streams.size() + first, 0, rows * sizeof(unsigned long long)));
            a = b;
        }
    }
    return upload_streams(s);
}

fx_status fx_rtp_get_cursors(fx_context* c, unsigned* timestamp, int* running)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    fx_rtp* s = nullptr;
    { const fx_status st = rtp_configured(c, &s); if (st != FX_OK) return st; }
    for (size_t k = 0; k < s->streams.size(); k++) {
        if (timestamp) timestamp[k] = s->streams[k].running ? s->streams[k].origin + s->advanced : 0u;
        if (running) running[k] = s->streams[k].running;
    }
    return FX_OK;
}

fx_status fx_push_rtp(fx_context* c, const void* packets, const int* lengths, const int* stream_of, int num_packets, int slot_stride,
                      int num_samples, int mem_kind, float* out_raw, float* out_smoothed, int* frames_out, unsigned char* disposition)
{
    if (frames_out) *frames_out = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    c->num_launches = 0;
    if (num_samples < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative sample count");
    if (num_packets < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative packet count %d", num_packets);
    { const fx_status ks = fx_check_memory_kind(mem_kind); if (ks != FX_OK) return ks; }
    if (slot_stride < 12 || slot_stride > FX_RTP_MAX_SLOT_STRIDE || slot_stride % 4 != 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "slot stride %d: a multiple of 4 in [12, %d]", slot_stride, FX_RTP_MAX_SLOT_STRIDE);
    if (num_samples == 0) return FX_OK;
    if (num_packets > 0 && (!packets || !lengths || !stream_of)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null packets, lengths or stream list with %d packets", num_packets);
    if (num_packets > 0 && mem_kind == FX_MEM_DEVICE && reinterpret_cast<uintptr_t>(packets) % 4 != 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "device packets must be 4-byte aligned");
    fx_rtp* s = nullptr;
    fx_status st;
    if ((st = rtp_configured(c, &s)) != FX_OK) return st;
    const int S = (int) s->streams.size();
    for (int i = 0; i < num_packets; i++) {
        if (lengths[i] < 0 || lengths[i] > slot_stride) return fx_fail(FX_ERR_INVALID_ARGUMENT, "lengths[%d] = %d: a datagram holds 0 to %d (the slot stride) bytes", i, lengths[i], slot_stride);
        if (stream_of[i] < 0 || stream_of[i] >= S) return fx_fail(FX_ERR_INVALID_ARGUMENT, "stream_of[%d] = %d out of range [0,%d)", i, stream_of[i], S);
    }
    // fx_push_block's own refusals, before anything is launched: a refused call changes nothing
    const int format = s->sample_format(), B = s->bytes();
    { const fx_status rs = fx_block_refusal(c, num_samples, format); if (rs != FX_OK) return rs; }
    fx_rtp_window& win = s->win;
    const int W = win.window, E = num_samples < W ? num_samples : W;    // (E: the far end's claims, fxk::RtpSpan)
    if (W > 0 && num_samples > INT32_MAX - W) return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d samples and a window of %d: the span is too long for one call", num_samples, W);

    HIP_TRY(hipSetDevice(c->device));
    { const fx_status es = fx_check_device_error(c); if (es != FX_OK) return es; }
    // everything that can fail for want of memory before the first launch.  Growing a buffer drops what it held, so the block of the
    // tick before is gone from here on, also where one of these refuses the call.
    s->last_n = 0;
    const size_t P = (size_t) num_packets, slot_bytes = P * (size_t) slot_stride;
    const size_t planar_bytes = (size_t) c->C * (size_t) num_samples * (size_t) B;
    fx_staged_list& meta = s->meta[s->meta_cur];
    if ((st = fx_reserve_list(c, &meta, 2 * P > 0 ? 2 * P : 1, sizeof(int))) != FX_OK) return st;
    if ((st = fx_grow(&s->d_records, &s->records_cap, (P > 0 ? P : 1) * sizeof(fxk::RtpRecord))) != FX_OK) return st;
    if ((st = fx_grow(&s->d_owner, &s->owner_cap, sizeof(int) * (size_t) S * ((size_t) num_samples + (size_t) E))) != FX_OK) return st;
    if (W > 0 && (st = fx_grow(&s->d_held, &s->held_cap, (P > 0 ? P : 1) * sizeof(fxk::RtpHeldRange))) != FX_OK) return st;
    if ((st = fx_grow(&s->d_planar, &s->planar_cap, (planar_bytes + 15) & ~(size_t) 15)) != FX_OK) return st;
    if (mem_kind == FX_MEM_HOST && P > 0) {
        if ((st = fx_grow(&s->d_slots, &s->slots_cap, slot_bytes)) != FX_OK) return st;
        if (disposition && (st = fx_grow(&s->d_disposition, &s->disposition_cap, P)) != FX_OK) return st;
    }

    const unsigned char* d_slots = static_cast<const unsigned char*>(packets);
    unsigned char* d_disposition = disposition;
    if (P > 0) {
        HIP_TRY(hipEventSynchronize(s->meta_done[s->meta_cur]));        // the upload that last read this list has finished
        int* pinned = static_cast<int*>(meta.pinned);
        memcpy(pinned, lengths, P * sizeof(int));
        memcpy(pinned + P, stream_of, P * sizeof(int));
        HIP_TRY(hipMemcpyAsync(meta.device, meta.pinned, 2 * P * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(s->meta_done[s->meta_cur], c->stream));
        s->meta_cur ^= 1;
        if (mem_kind == FX_MEM_HOST) {
            HIP_TRY(hipMemcpyAsync(s->d_slots, packets, slot_bytes, hipMemcpyHostToDevice, c->stream));
            d_slots = s->d_slots;
            if (disposition) d_disposition = s->d_disposition;
        }
    }
    fxk::RtpTick p;
    p.slots = d_slots;
    p.lengths = static_cast<const int*>(meta.device);
    p.stream_of = p.lengths + P;
    p.streams = s->d_streams;
    p.tracks = s->d_tracks;
    p.records = s->d_records;
    p.owner = s->d_owner;
    p.disposition = d_disposition;
    p.stats = s->d_stats;
    p.out = s->d_planar;
    p.P = num_packets;
    p.stride = slot_stride;
    p.S = S;
    p.C = c->C;
    p.n = num_samples;
    p.B = B;
    p.advanced = s->advanced;
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_RTP, 0)) r->T = num_samples;
    if (W == 0) {
        HIP_TRY(fxk::launch_rtp_kernels(p, nullptr, c->stream));
    } else {
        // the stamps' tick numbers start over below every later one before they would wrap (FX_HOOK_RTP_FEW_TICK_NUMBERS, tests: after 3)
        if (win.tick_no >= ((c->test_hooks & FX_HOOK_RTP_FEW_TICK_NUMBERS) ? 4u : UINT32_MAX)) {
            const long long count = (long long) S * W;
            hipLaunchKernelGGL(fxk::fx_rtp_rebase_stamps_kernel, dim3((unsigned) ((count + 255) / 256)), dim3(256), 0, c->stream, win.stamps, count);
            HIP_TRY(hipGetLastError());
            win.tick_no = 1;
        }
        fxk::RtpSpan w;
        w.t = p;
        w.far = s->d_owner + (size_t) S * (size_t) num_samples;
        w.held = s->d_held;
        w.ring = win.ring;
        w.ring_base = win.ring_base;
        w.stamps = win.stamps;
        w.wstats = win.wstats;
        w.W = W;
        w.E = E;
        w.head = win.head;
        w.tick = win.tick_no;
        HIP_TRY(fxk::launch_rtp_kernels(w.t, &w, c->stream));
        win.head = (int) (((long long) win.head + num_samples) % W);
        win.tick_no++;
    }
    s->advanced += (unsigned) num_samples;              // every running stream's cursor
    s->last_n = num_samples;
    if (P > 0 && mem_kind == FX_MEM_HOST && disposition)
        HIP_TRY(hipMemcpyAsync(disposition, s->d_disposition, P, hipMemcpyDeviceToHost, c->stream));
    int frames = 0;
    st = fx_push_block(c, s->d_planar, num_samples, format, FX_MEM_DEVICE, mem_kind, out_raw, out_smoothed, &frames, true);
    if (st != FX_OK) {
        // the copies of the caller's host arrays are enqueued: they end before the caller has them back, whatever failed
        if (mem_kind == FX_MEM_HOST) (void) hipStreamSynchronize(c->stream);
        return st;
    }
    // the caller may reuse host packets, and read the disposition, on return
    if (mem_kind == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(c->stream));
    if (frames_out) *frames_out = frames;
    return FX_OK;
}

fx_status fx_rtp_get_block(fx_context* c, void* out, size_t capacity_bytes, int* num_samples, int* sample_format, int mem_kind)
{
    if (num_samples) *num_samples = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null output pointer");
    { const fx_status st = fx_check_memory_kind(mem_kind); if (st != FX_OK) return st; }
    fx_rtp* s = nullptr;
    { const fx_status st = rtp_configured(c, &s); if (st != FX_OK) return st; }
    if (num_samples) *num_samples = s->last_n;          // (also where the room is refused: a host learns what to bring)
    if (sample_format) *sample_format = s->sample_format();
    const size_t bytes = (size_t) c->C * (size_t) s->last_n * (size_t) s->bytes();
    if (capacity_bytes < bytes)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "capacity %zu bytes: the last tick's block holds %d samples per track, %zu bytes", capacity_bytes, s->last_n, bytes);
    if (bytes == 0) return FX_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, s->d_planar, bytes, mem_kind == FX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    if (mem_kind == FX_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fx_check_device_error(c);
    }
    return FX_OK;
}

fx_status fx_rtp_get_stats(fx_context* c, fx_rtp_stats* out)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null output pointer");
    fx_rtp* s = nullptr;
    { const fx_status st = rtp_configured(c, &s); if (st != FX_OK) return st; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, s->d_stats, sizeof(fx_rtp_stats) * s->streams.size(), hipMemcpyDeviceToHost));
    return fx_check_device_error(c);
}

fx_status fx_rtp_set_window(fx_context* c, int window)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (window < 0 || window > FX_RTP_MAX_WINDOW)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "window %d: a reorder window is 0 (none) to %d sample times", window, FX_RTP_MAX_WINDOW);
    fx_rtp* s = nullptr;
    { const fx_status st = rtp_configured(c, &s); if (st != FX_OK) return st; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // ticks in flight read and write the held state
    // the new window's state whole, then the old one goes: a failure leaves the unit as it was
    fx_rtp_window next;
    if (window > 0) {
        const fx_status st = rtp_window_alloc(&next, s->streams, window, s->bytes());
        if (st != FX_OK) return st;
    }
    rtp_window_free(&s->win);
    s->win = next;
    return FX_OK;
}

fx_status fx_rtp_get_window(fx_context* c, int* window, fx_rtp_window_stats* out)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    fx_rtp* s = nullptr;
    { const fx_status st = rtp_configured(c, &s); if (st != FX_OK) return st; }
    if (window) *window = s->win.window;
    if (!out) return FX_OK;
    const size_t S = s->streams.size();
    if (s->win.window == 0) {
        for (size_t k = 0; k < S; k++) out[k] = fx_rtp_window_stats{0, 0};
        return FX_OK;
    }
    std::vector<unsigned long long> got;
    try {
        got.resize(fxk::WS_FIELDS * S);
    } catch (const std::bad_alloc&) {
        return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(got.data(), s->win.wstats, sizeof(unsigned long long) * got.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < S; k++) out[k] = fx_rtp_window_stats{(long long) got[fxk::WS_HELD * S + k], (long long) got[fxk::WS_RECOVERED * S + k]};
    return fx_check_device_error(c);
}

} // extern "C"
