// fx_clips.hip -- file sources (include/fx.h: fx_create_clips .. fx_push_sources): tracks play device-resident clips, transport on the GPU.
//
// ref AudioFilePlayer.h:41-67 is a looping file behind play / pause / stop / restart, AnalyserTrackController.h:92-138 switches a track
// between the audio device and that player and clears the track's collectors when it does.  Here a file is a clip in device memory, a
// track's player one row of a table in device memory (ClipRow), and a tick is ONE launch of fx_clip_gather_kernel: it forms the planar
// block [C][n] that fx_push_samples takes -- track c's row from the caller's live block, from its clip (wrapping, or ending in
// silence) or as silence -- in a staging buffer, and advances every playing track's position.  fx_push_block (fx_capi.cpp) does the
// rest: the same launches, the same bits as fx_push_samples of that planar block.  Bytes only: no conversion, no gain (the analysis
// kernels' load stage does both, AudioDataCollector.h:88).
//
// A clip whose own sample rate is not the context's is RATED (fx_set_clip_rates): its track plays it through the windowed-sinc
// resampler include/fx.h specifies.  The gather renders such a track as silence and moves its output count k on; a second launch,
// fx_clip_resample_kernel, made only while a FILE track has a rated clip loaded, overwrites the staging rows of the rated tracks that
// play with fp32 samples.
//
// The table exists twice.  A launch reads one copy and writes every row of the other, so no workgroup can read a position that the same
// launch has advanced, exactly one thread writes a track's new row, and nothing needs an atomic (fx_display.hip keeps its state records
// the same way).  The command kernel (fx_transport_kernel) is a launch of its own and changes the current copy in place.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: the first call installs the context's release hook.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"

#pragma clang fp contract(off)

namespace fxk {

// (the load stage's widen_one: what the resampler makes of a clip's bytes is what the analysis kernels would)
#include "fx_wave.hip.h"          // f4
#include "fx_samples.hip.h"
#include "fx_blocks.hip.h"        // the shifted 16-byte read

namespace {

// A track's player.  All zeros is the default: source INPUT, no file.
struct __attribute__((aligned(16))) ClipRow {
    const unsigned char* base;      // the loaded clip's first byte (any alignment), null without one
    long long            length;    // L, samples; 0 without a clip
    long long            position;  // samples; < L while the clip can play, == L once a one-shot has FINISHED
    long long            laps;      // completed passes of a looping clip since it was loaded
    int                  source, state, loop, format;
    // a rated clip (taps > 0; all zeros otherwise): position and laps follow from k (include/fx.h, "A rated track's tick")
    long long            k;         // outputs rendered since the position was last set to 0
    double               ratio;     // r = the clip's rate / the context's, formed by the host: the device never divides
    double               rho;       // min(1, 1 / r)
    int                  taps;      // J = ceil(Z / rho)
    int                  pad;
};
static_assert(sizeof(ClipRow) == 80, "rows are five 16-byte pieces");

struct GatherParams {
    const ClipRow*       rows;      // [C], read
    ClipRow*             next;      // [C], the other copy: every row written, playing tracks advanced by n
    const unsigned char* live;      // [C][n] samples of B bytes, or null (then no track's source is INPUT)
    unsigned char*       out;       // [C][n] samples of B bytes, 16-byte aligned, capacity a multiple of 16
    long long            n;
    int                  C;
};

// Where a track's n * B bytes come from: byte i of the row is base[s + i] -- modulo `lim` for a looping clip, zero from `lim` on
// otherwise -- and silence for base == null.  The live row and a one-shot clip are the same thing, a run that ends.
struct RowStream {
    const unsigned char* base;
    long long            s, lim;
    bool                 loop;
};

template <int B> __device__ __forceinline__ RowStream row_stream(const GatherParams& p, long long c, long long row_bytes)
{
    const ClipRow& r = p.rows[c];
    if (r.source == FX_SOURCE_INPUT) return RowStream{p.live + c * row_bytes, 0, row_bytes, false};
    if (r.state != FX_TRANSPORT_PLAYING || r.taps > 0) return RowStream{nullptr, 0, 0, false};      // (rated: the resampler's row)
    return RowStream{r.base, r.position * B, r.length * B, r.loop != 0};
}

constexpr int GATHER_THREADS = 256;

// The staging buffer is one run of C * n * B bytes from a 16-byte boundary, and thread g of the launch writes its 16-byte piece g with
// one global_store_dwordx4 -- whatever n * B makes of the rows' alignment, and with every lane busy when rows are short (441 / 480 /
// 512 samples: the pieces of all tracks are dealt out in one run, as fx_reblock_rows_kernel deals them).  A piece that lies inside one
// row and whose 16 source bytes are one run of memory -- the live row, or a clip away from its seam -- is read as stream_piece16 reads
// its block: the aligned dwords around the bytes (every one of them holds a byte of the run, so nothing outside the clip's dwords is
// touched), shifted into place.  Every other piece is put together byte by byte: a piece across two or more rows (a row boundary at
// any byte; rows shorter than 16 bytes), across a clip's seam (inside a dword, inside a packed 24-bit sample), through several laps of
// a clip shorter than 16 bytes, or across a one-shot's end.  All offsets are 64-bit.
template <int B> __device__ __forceinline__ void gather_piece(const GatherParams& p, const long long g)
{
    const long long row_bytes = p.n * B;
    const long long total = (long long) p.C * row_bytes;

    // the table: thread g moves track g's row to the other copy (reads `rows`, which this launch does not write)
    if (g < p.C) {
        ClipRow r = p.rows[g];
        if (r.source == FX_SOURCE_FILE && r.state == FX_TRANSPORT_PLAYING && r.taps > 0) {
            r.k += p.n;
            const double x = (double) r.k * r.ratio;
            const long long whole = (long long) x;                                  // floor: x >= 0
            if (r.loop) {
                r.laps = whole / r.length;
                r.position = whole % r.length;
            } else {
                if (x >= (double) r.length) r.state = FX_TRANSPORT_FINISHED;
                r.position = whole < r.length ? whole : r.length;
            }
        } else if (r.source == FX_SOURCE_FILE && r.state == FX_TRANSPORT_PLAYING) {
            const long long t = r.position + p.n;
            if (r.loop) {
                r.laps += t / r.length;
                r.position = t % r.length;
            } else {
                if (t >= r.length) r.state = FX_TRANSPORT_FINISHED;
                r.position = t < r.length ? t : r.length;
            }
        }
        p.next[g] = r;
    }

    const long long f0 = 16 * g;
    if (f0 >= total) return;
    // (a 64-bit division per thread: dividing in 32 bits where the block allows it was tried and changed no measured time -- the
    // launch is bound by latency at live sizes and by HBM at long ones, profiles/clip_sources.txt)
    const long long c = f0 / row_bytes, off = f0 - c * row_bytes;
    unsigned v[4] = {0u, 0u, 0u, 0u};
    bool bytewise = off + 16 > row_bytes;
    if (!bytewise) {
        const RowStream st = row_stream<B>(p, c, row_bytes);
        if (st.base) {
            long long x = st.s + off;
            if (st.loop && x >= st.lim) x %= st.lim;
            if (x + 16 <= st.lim) {
                const unsigned char* at = st.base + x;
                const unsigned sh = (unsigned) (reinterpret_cast<uintptr_t>(at) & 3);
                // (clips and live blocks are device memory: load_raw_piece says so to the compiler, which sees only a pointer read from
                // the table, so that it emits global_load_dwordx4 and not a flat load.  sh == 0: the fifth dword holds no byte of the run)
                const uint4 q = shifted_piece(load_raw_piece(at - sh, sh), sh);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else if (st.loop || x < st.lim) {
                bytewise = true;                                                // a seam or an end inside the piece
            }
        }
    }
    if (bytewise) {
        long long cc = c, o = off;
        RowStream st = row_stream<B>(p, cc, row_bytes);
        long long x = st.s + o;
        if (st.loop && x >= st.lim) x %= st.lim;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (f0 + k < total) {
                if (o == row_bytes) {
                    cc++; o = 0;
                    st = row_stream<B>(p, cc, row_bytes);
                    x = st.s;
                }
                unsigned b = 0;
                if (st.base && x < st.lim) b = st.base[x];
                v[k >> 2] |= b << (8 * (k & 3));
                o++; x++;
                if (st.loop && x == st.lim) x = 0;
            }
        }
    }
    *reinterpret_cast<uint4*>(p.out + f0) = uint4{v[0], v[1], v[2], v[3]};
}

template <int B>
__global__ void __launch_bounds__(GATHER_THREADS)
fx_clip_gather_kernel(const GatherParams p)
{
    gather_piece<B>(p, (long long) blockIdx.x * GATHER_THREADS + threadIdx.x);
}

hipError_t launch_clip_gather_kernel(const GatherParams& p, int bytes_per_sample, hipStream_t stream)
{
    if (p.n <= 0 || p.C <= 0) return hipSuccess;
    const long long pieces = ((long long) p.C * p.n * bytes_per_sample + 15) / 16;
    const long long threads = pieces > p.C ? pieces : p.C;              // (rows of fewer than 16 bytes: a thread per track all the same)
    const long long wgs = (threads + GATHER_THREADS - 1) / GATHER_THREADS;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    const dim3 grid((unsigned) wgs), block(GATHER_THREADS);
    switch (bytes_per_sample) {
        case 4: hipLaunchKernelGGL(fx_clip_gather_kernel<4>, grid, block, 0, stream, p); break;
        case 3: hipLaunchKernelGGL(fx_clip_gather_kernel<3>, grid, block, 0, stream, p); break;
        case 2: hipLaunchKernelGGL(fx_clip_gather_kernel<2>, grid, block, 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- rated clips: the resampler of include/fx.h ("A rated track's tick"), whose operations and their order these lines keep ----
constexpr int RS_Z = 16, RS_P = 512;                            // zero crossings a side, phases between two of them
constexpr int RS_PAIRS = RS_Z * RS_P, RS_TABLE = RS_PAIRS + 2;
constexpr double RS_BETA = 9.0;
constexpr int RS_THREADS = 256;
constexpr int RS_CHUNKS = 4;                                    // runs of RS_THREADS outputs a workgroup renders on one copy of the table
constexpr int RS_MAX_TAPS = 128;                                // J at r = 8
// the clip samples 256 neighbouring outputs touch: floor(x) moves by at most floor(255 * 8) + 1 over them, and J - 1 taps lie before the
// first one's, J after the last one's
constexpr int RS_SPAN = 255 * 8 + 1 + 2 * RS_MAX_TAPS;
static_assert(RS_SPAN == 2297, "the span of a run of outputs at r = 8");

struct ResampleParams {
    const ClipRow* rows;        // [C]: the copy the tick's gather READ (k before the tick); no launch of the tick writes it
    const int*     tracks;      // [count]: the FILE tracks with a rated clip loaded
    const float2*  pairs;       // [RS_PAIRS]: (T[i], T[i + 1] - T[i])
    float*         out;         // [C][n] fp32, the staging block
    long long      n;
    int            count, wgs_per_track;
};

typedef const unsigned char __attribute__((address_space(1)))* GlobalBytes;

// span[idx] = the clip's sample lo + idx for idx < count, as the load stage widens it: modulo L for a looping clip; +0 outside a
// one-shot clip.  (A tap there "is not added": adding c * +0 instead leaves the same bits, because c is finite and the accumulator,
// which starts at +0, is never -0 -- a sum rounds to -0 only from two -0 terms.)
template <int FMT> __device__ __forceinline__ void fill_span(float* span, const ClipRow& row, long long lo, int count, int tid)
{
    const GlobalBytes base = (GlobalBytes) row.base;            // (clips are device memory: said to the compiler, as the gather says it)
    const unsigned long long L = (unsigned long long) row.length;
    unsigned long long start = 0;
    if (row.loop) {
        const long long m = lo % row.length;
        start = (unsigned long long) (m < 0 ? m + row.length : m);
    }
    for (int idx = tid; idx < count; idx += RS_THREADS) {
        float v = 0.0f;
        if (row.loop) {
            unsigned long long m = start + (unsigned) idx;
            if (m >= L) { m -= L; if (m >= L) m %= L; }         // (one lap is the rule; a 64-bit division only for clips shorter than the span)
            v = widen_one<FMT>((const void*) (base + m * (unsigned long long) sample_bytes(FMT)));
        } else {
            const long long m = lo + idx;
            if (m >= 0 && m < row.length) v = widen_one<FMT>((const void*) (base + (unsigned long long) m * (unsigned long long) sample_bytes(FMT)));
        }
        span[idx] = v;
    }
}

// Workgroup w renders outputs [part * 1024, +1024) of rated track tracks[w / wgs_per_track], 256 at a time, one output a lane.  The
// table lives in LDS as pairs for the whole workgroup (64 KB: two workgroups a CU); each run's span of the clip is widened into LDS
// once, since neighbouring lanes' taps overlap almost entirely.  Per tap a lane does the specification's fp64 steps and two LDS reads.
__global__ void __launch_bounds__(RS_THREADS)
fx_clip_resample_kernel(const ResampleParams p)
{
    __shared__ float2 tab[RS_PAIRS];
    __shared__ float span[RS_SPAN + 7];
    const int tid = (int) threadIdx.x;
    const int which = (int) (blockIdx.x / (unsigned) p.wgs_per_track), part = (int) (blockIdx.x % (unsigned) p.wgs_per_track);
    if (which >= p.count) return;
    const int track = p.tracks[which];
    const ClipRow& row = p.rows[track];
    // (uniform over the workgroup: the barriers below are reached by all of its lanes or by none)
    if (row.source != FX_SOURCE_FILE || row.state != FX_TRANSPORT_PLAYING || row.taps <= 0 || row.taps > RS_MAX_TAPS || row.length <= 0) return;
    {
        typedef unsigned __attribute__((vector_size(16))) piece;              // two pairs
        const piece __attribute__((address_space(1)))* src = (const piece __attribute__((address_space(1)))*) p.pairs;
        piece* dst = reinterpret_cast<piece*>(tab);
        for (int v = tid; v < RS_PAIRS / 2; v += RS_THREADS) dst[v] = src[v];
    }
    const double r = row.ratio, rho = row.rho;
    const int J = row.taps;
    const long long k = row.k;
    const float scale = (float) rho;
    float* out = p.out + (long long) track * p.n;
    const long long first = (long long) part * (RS_THREADS * RS_CHUNKS);
    for (int chunk = 0; chunk < RS_CHUNKS; chunk++) {
        const long long a = first + (long long) chunk * RS_THREADS;
        if (a >= p.n) break;
        const long long b = a + RS_THREADS - 1 < p.n ? a + RS_THREADS - 1 : p.n - 1;
        const long long lo = (long long) ((double) (k + a) * r) - (J - 1);
        const long long want = (long long) ((double) (k + b) * r) + J - lo + 1;
        const int count = want < RS_SPAN ? (int) want : RS_SPAN;
        __syncthreads();                                        // the run before has read its span
        FX_FORMAT(row.format, fill_span<FMT>(span, row, lo, count, tid));
        __syncthreads();
        const long long i = a + tid;
        if (i <= b) {
            const double x = (double) (k + i) * r;
            const long long i0 = (long long) x;                 // floor: x >= 0
            const double f = x - (double) i0;
            const int at = (int) (i0 - lo);                     // where tap j = 0 reads the span: >= J - 1
            float acc = 0.0f;
            for (int j = 1 - J; j <= J; j++) {
                const double d = fabs((double) j - f) * rho;
                if (d < (double) RS_Z) {
                    const double q = d * (double) RS_P;
                    const int ti = (int) q;                     // floor: 0 <= q < RS_PAIRS
                    const float t = (float) (q - (double) ti);
                    const float2 e = tab[ti];
                    const float c = e.x + t * e.y;
                    const unsigned si = (unsigned) (at + j);
                    const float s = si < (unsigned) RS_SPAN ? span[si] : 0.0f;
                    acc = acc + c * s;
                }
            }
            float o = acc * scale;
            if (!row.loop && x >= (double) row.length) o = 0.0f;
            out[i] = o;
        }
    }
}

hipError_t launch_clip_resample_kernel(ResampleParams p, hipStream_t stream)
{
    if (p.n <= 0 || p.count <= 0) return hipSuccess;
    const long long per = (p.n + RS_THREADS * RS_CHUNKS - 1) / (RS_THREADS * RS_CHUNKS);
    const long long wgs = per * p.count;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    p.wgs_per_track = (int) per;
    hipLaunchKernelGGL(fx_clip_resample_kernel, dim3((unsigned) wgs), dim3(RS_THREADS), 0, stream, p);
    return hipGetLastError();
}

// One command per list entry, applied to the current copy of the table in place.  FX_PLAY .. FX_RESTART are fx_transport's (every
// entry of a call carries the same one, so duplicates in the list store the same row twice); the setters' lists arrive with one entry
// per track (the host keeps a track's last one).
enum { CLIP_OP_SOURCE_INPUT = 4, CLIP_OP_SOURCE_FILE = 5, CLIP_OP_LOAD = 6 };
static_assert(FX_PLAY == 0 && FX_PAUSE == 1 && FX_STOP == 2 && FX_RESTART == 3, "the transport commands are the first four operations");
struct __attribute__((aligned(16))) ClipCommand {
    int                  track, op, loop, format;
    const unsigned char* base;      // CLIP_OP_LOAD: the clip, null for "no file"
    long long            length;
    double               ratio, rho;    // CLIP_OP_LOAD of a rated clip (taps > 0): ClipRow's
    int                  taps, pad[3];
};
static_assert(sizeof(ClipCommand) == 64, "commands are four 16-byte pieces");

__global__ void __launch_bounds__(256) fx_transport_kernel(ClipRow* rows, const ClipCommand* commands, int n, int C)
{
    const int i = (int) (blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const ClipCommand k = commands[i];
    if ((unsigned) k.track >= (unsigned) C) return;                     // (the host has checked every entry)
    ClipRow r = rows[k.track];
    const bool has_clip = r.length > 0;
    switch (k.op) {
        case FX_PLAY:
            if (r.state == FX_TRANSPORT_FINISHED) { r.position = 0; r.k = 0; }
            if (has_clip) r.state = FX_TRANSPORT_PLAYING;
            break;
        case FX_PAUSE:
            if (r.state == FX_TRANSPORT_PLAYING) r.state = FX_TRANSPORT_PAUSED;
            break;
        case FX_STOP:
            if (has_clip) { r.state = FX_TRANSPORT_STOPPED; r.position = 0; r.k = 0; }
            break;
        case FX_RESTART:
            r.position = 0; r.k = 0;
            if (r.state == FX_TRANSPORT_FINISHED) r.state = FX_TRANSPORT_STOPPED;
            break;
        case CLIP_OP_SOURCE_INPUT:
            r.source = FX_SOURCE_INPUT;
            r.state = has_clip ? FX_TRANSPORT_STOPPED : FX_TRANSPORT_NO_FILE;
            r.position = 0; r.k = 0;
            break;
        case CLIP_OP_SOURCE_FILE:
            r.source = FX_SOURCE_FILE;
            break;
        case CLIP_OP_LOAD:
            r.base = k.base; r.length = k.length; r.loop = k.loop; r.format = k.format;
            r.state = k.base ? FX_TRANSPORT_STOPPED : FX_TRANSPORT_NO_FILE;
            r.position = 0; r.laps = 0;
            r.k = 0; r.ratio = k.ratio; r.rho = k.rho; r.taps = k.taps;
            break;
        default: return;
    }
    rows[k.track] = r;
}

} // namespace
} // namespace fxk

namespace {

struct clip_bank {
    int                    first_id = 0, count = 0, format = FX_SAMPLE_F32;
    unsigned char*         mem = nullptr;
    bool                   owned = false;
    std::vector<long long> offset, length;      // per clip: its first byte in mem, its samples
    std::vector<double>    rate;                // per clip: its own sample rate in Hz, 0 = the context's (fx_set_clip_rates)
};

} // namespace

struct fx_clips {
    fxk::ClipRow*            d_rows[2] = {nullptr, nullptr};   // the table, twice: [C] each
    int                      cur = 0;                           // the copy in force
    // what the host knows of the table because only its own commands change it (state, position and laps live on the device alone)
    std::vector<int>         clip_of, source, format_of;       // [C]: loaded clip id or -1, FX_SOURCE_*, the clip's format or -1
    std::vector<char>        rated_of;                          // [C]: the loaded clip plays through the resampler
    std::vector<double>      loaded_under;                      // [C]: the context's rate when a clip with a rate of its own was loaded, else 0
    float2*                  d_pairs = nullptr;                 // the resampler's table as the kernel reads it; made with the first rated load
    int*                     d_rated = nullptr;                 // the FILE tracks with a rated clip loaded, [num_rated]
    int                      num_rated = 0;
    std::vector<clip_bank>   banks;
    int                      next_id = 0;
    fxk::ClipCommand*        d_commands = nullptr;
    size_t                   commands_cap = 0;                  // bytes
    unsigned char*           d_live = nullptr;                  // a host live block
    unsigned char*           d_planar = nullptr;                // the planar block handed to fx_push_block
    size_t                   live_cap = 0, planar_cap = 0;
};

namespace {

void clips_release(fx_context* c)
{
    fx_clips* s = c->clips;
    if (!s) return;
    for (clip_bank& b : s->banks) if (b.owned && b.mem) (void) hipFree(b.mem);
    fx_free_device({s->d_rows[0], s->d_rows[1], s->d_commands, s->d_live, s->d_planar, s->d_pairs, s->d_rated});
    delete s;
    c->clips = nullptr;
}

// the context's file-source state, with every track on its input and no file, on first use
fx_status clips_state(fx_context* c, fx_clips** out)
{
    if (!c->clips) {
        fx_clips* s = new (std::nothrow) fx_clips();
        if (!s) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
        const size_t bytes = sizeof(fxk::ClipRow) * (size_t) c->C;
        hipError_t e = hipSuccess;
        try {
            s->clip_of.assign((size_t) c->C, -1);
            s->source.assign((size_t) c->C, FX_SOURCE_INPUT);
            s->format_of.assign((size_t) c->C, -1);
            s->rated_of.assign((size_t) c->C, 0);
            s->loaded_under.assign((size_t) c->C, 0.0);
        } catch (const std::bad_alloc&) {
            delete s;
            return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
        }
        for (int k = 0; k < 2 && e == hipSuccess; k++) {
            void* q = nullptr;
            e = hipMalloc(&q, bytes);
            s->d_rows[k] = static_cast<fxk::ClipRow*>(q);
            if (e == hipSuccess) e = hipMemsetAsync(q, 0, bytes, c->stream);         // all zeros: source INPUT, no file
        }
        if (e != hipSuccess) {
            for (int k = 0; k < 2; k++) if (s->d_rows[k]) (void) hipFree(s->d_rows[k]);
            delete s;
            return fx_fail(fx_hip_status(e), "allocating the transport table failed: %s", hipGetErrorString(e));
        }
        c->clips = s;
        c->clips_release = clips_release;
    }
    *out = c->clips;
    return FX_OK;
}

// the bank that holds clip `id`, or null (no device use; the context may have no file-source state yet)
const clip_bank* bank_of(const fx_context* c, int id)
{
    if (!c->clips || id < 0) return nullptr;
    for (const clip_bank& b : c->clips->banks)
        if (id >= b.first_id && id - b.first_id < b.count) return &b;
    return nullptr;
}

// I0, the modified Bessel function of the first kind and order 0, by its power series (every term positive: no cancellation)
double bessel_i0(double x)
{
    const double h = x / 2.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= (h / k) * (h / k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

// The resampler's table (include/fx.h): one side of a Kaiser-windowed sinc, RS_P entries per zero crossing, computed in fp64 and
// rounded to fp32 once; the two entries past its end are +0.
const std::vector<float>& resampler_table()
{
    static const std::vector<float> table = [] {
        std::vector<float> t((size_t) fxk::RS_TABLE, 0.0f);
        const double pi = 3.14159265358979323846, at_beta = bessel_i0(fxk::RS_BETA);
        for (int i = 0; i < fxk::RS_PAIRS; i++) {
            const double x = (double) i / fxk::RS_P, y = pi * x;
            const double sinc = i == 0 ? 1.0 : std::sin(y) / y;
            const double u = (double) i / (double) fxk::RS_PAIRS;
            t[(size_t) i] = (float) (sinc * bessel_i0(fxk::RS_BETA * std::sqrt(1.0 - u * u)) / at_beta);
        }
        return t;
    }();
    return table;
}

// r, rho and J of a clip of `rate` Hz in a context of `context_rate` Hz; false for a clip that is not rated (taps 0)
struct rated_load { double ratio = 0.0, rho = 0.0; int taps = 0; };
bool rate_of_load(double rate, double context_rate, rated_load* out)
{
    *out = rated_load{};
    if (rate == 0.0 || rate == context_rate) return false;
    out->ratio = rate / context_rate;
    const double inverse = 1.0 / out->ratio;
    out->rho = inverse < 1.0 ? inverse : 1.0;
    out->taps = (int) std::ceil((double) fxk::RS_Z / out->rho);
    return true;
}

// what a context with a rated clip needs on the device: the table's copy and room for the list of rated tracks.  Made before the
// command that loads the first such clip is launched, so that a failed allocation changes nothing.
fx_status prepare_rated(fx_context* c, fx_clips* s)
{
    if (!s->d_pairs) {
        const std::vector<float>& t = resampler_table();
        std::vector<float2> pairs((size_t) fxk::RS_PAIRS);
        for (int i = 0; i < fxk::RS_PAIRS; i++) pairs[(size_t) i] = float2{t[(size_t) i], t[(size_t) i + 1] - t[(size_t) i]};
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, pairs.size() * sizeof(float2)));
        const hipError_t e = hipMemcpy(q, pairs.data(), pairs.size() * sizeof(float2), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void) hipFree(q);
            return fx_fail(FX_ERR_HIP, "copying the resampler's table failed: %s", hipGetErrorString(e));
        }
        s->d_pairs = static_cast<float2*>(q);
    }
    if (!s->d_rated) {
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, (size_t) c->C * sizeof(int)));
        s->d_rated = static_cast<int*>(q);
    }
    return FX_OK;
}

// the device's list of the FILE tracks with a rated clip loaded (the stream is idle; prepare_rated has run if there is one)
fx_status refresh_rated(fx_context* c, fx_clips* s)
{
    std::vector<int> list;
    for (int t = 0; t < c->C; t++)
        if (s->source[(size_t) t] == FX_SOURCE_FILE && s->rated_of[(size_t) t]) list.push_back(t);
    s->num_rated = 0;
    if (list.empty()) return FX_OK;
    HIP_TRY(hipMemcpy(s->d_rated, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice));
    s->num_rated = (int) list.size();
    return FX_OK;
}

// `commands` to the device and the one launch over them, on the context's stream (the stream is idle: every caller has synchronised)
fx_status run_commands(fx_context* c, fx_clips* s, const std::vector<fxk::ClipCommand>& commands)
{
    if (commands.empty()) return FX_OK;
    const size_t bytes = commands.size() * sizeof(fxk::ClipCommand);
    fx_status st;
    if ((st = fx_grow(&s->d_commands, &s->commands_cap, bytes)) != FX_OK) return st;
    HIP_TRY(hipMemcpy(s->d_commands, commands.data(), bytes, hipMemcpyHostToDevice));
    const unsigned wgs = (unsigned) ((commands.size() + 255) / 256);
    hipLaunchKernelGGL(fxk::fx_transport_kernel, dim3(wgs), dim3(256), 0, c->stream, s->d_rows[s->cur], s->d_commands, (int) commands.size(), c->C);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fx_fail(FX_ERR_HIP, "launching the transport commands failed: %s", hipGetErrorString(e));
    return FX_OK;
}

// the list with one entry per track, the LAST one of each: positions into the caller's arrays, in list order
std::vector<int> last_entries(const fx_context* c, const int* channels, int num_channels)
{
    std::vector<char> seen((size_t) c->C, 0);
    std::vector<int> keep;
    for (int i = num_channels - 1; i >= 0; i--)
        if (!seen[(size_t) channels[i]]) { seen[(size_t) channels[i]] = 1; keep.push_back(i); }
    return std::vector<int>(keep.rbegin(), keep.rend());
}

} // namespace

extern "C" {

fx_status fx_create_clips(fx_context* c, const void* samples, const long long* lengths, int num_clips, int sample_format, int mem_kind,
                          unsigned flags, int* first_id)
{
    if (first_id) *first_id = -1;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (num_clips < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d clips: a bank holds at least one", num_clips);
    { const fx_status cs = fx_check_call(sample_format, mem_kind, mem_kind); if (cs != FX_OK) return cs; }
    if (!samples || !lengths || !first_id) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~(unsigned) FX_CLIP_BORROW) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown flags %#x", flags);
    if ((flags & FX_CLIP_BORROW) && mem_kind != FX_MEM_DEVICE)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "FX_CLIP_BORROW needs device memory: a bank cannot refer to host memory");
    const long long esz = (long long) sample_size(sample_format);
    long long total = 0;
    for (int k = 0; k < num_clips; k++) {
        if (lengths[k] < 1) return fx_fail(FX_ERR_INVALID_ARGUMENT, "lengths[%d] = %lld: a clip holds at least one sample", k, lengths[k]);
        if (lengths[k] > (LLONG_MAX / 8 - total) / esz) return fx_fail(FX_ERR_INVALID_ARGUMENT, "lengths[%d] = %lld: the bank is too large", k, lengths[k]);
        total += lengths[k] * esz;
    }
    if (mem_kind == FX_MEM_DEVICE && reinterpret_cast<uintptr_t>(samples) % 4 != 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "a device bank must be 4-byte aligned");
    if (c->clips && c->clips->next_id > INT_MAX - num_clips) return fx_fail(FX_ERR_INVALID_ARGUMENT, "out of clip ids");

    HIP_TRY(hipSetDevice(c->device));
    fx_clips* s = nullptr;
    fx_status st;
    if ((st = clips_state(c, &s)) != FX_OK) return st;
    clip_bank b;
    try {
        b.offset.resize((size_t) num_clips);
        b.length.assign(lengths, lengths + num_clips);
        b.rate.assign((size_t) num_clips, 0.0);
        s->banks.reserve(s->banks.size() + 1);
    } catch (const std::bad_alloc&) {
        return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    }
    long long at = 0;
    for (int k = 0; k < num_clips; k++) { b.offset[(size_t) k] = at; at += lengths[k] * esz; }
    b.first_id = s->next_id;
    b.count = num_clips;
    b.format = sample_format;
    if (flags & FX_CLIP_BORROW) {
        b.mem = const_cast<unsigned char*>(static_cast<const unsigned char*>(samples));
    } else {
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, (size_t) total));
        const hipError_t e = hipMemcpyAsync(q, samples, (size_t) total, mem_kind == FX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
        // a host buffer may be reused on return
        const hipError_t w = e == hipSuccess && mem_kind == FX_MEM_HOST ? hipStreamSynchronize(c->stream) : e;
        if (w != hipSuccess) {
            (void) hipFree(q);
            return fx_fail(FX_ERR_HIP, "copying the bank failed: %s", hipGetErrorString(w));
        }
        b.mem = static_cast<unsigned char*>(q);
        b.owned = true;
    }
    s->banks.push_back(std::move(b));
    s->next_id += num_clips;
    *first_id = s->banks.back().first_id;
    return FX_OK;
}

fx_status fx_destroy_clips(fx_context* c, int first_id)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    const clip_bank* b = bank_of(c, first_id);
    if (!b || b->first_id != first_id) return fx_fail(FX_ERR_INVALID_ARGUMENT, "no bank starts at clip id %d", first_id);
    fx_clips* s = c->clips;
    for (int t = 0; t < c->C; t++)
        if (s->clip_of[(size_t) t] >= b->first_id && s->clip_of[(size_t) t] - b->first_id < b->count)
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d has clip %d of this bank loaded", t, s->clip_of[(size_t) t]);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // ticks in flight may read the bank (a paused track's clip is not read, but is loaded)
    const size_t at = (size_t) (b - s->banks.data());
    const hipError_t freed = b->owned ? hipFree(b->mem) : hipSuccess;
    s->banks.erase(s->banks.begin() + (long) at);
    HIP_TRY(freed);
    return FX_OK;
}

fx_status fx_set_channel_clips(fx_context* c, const int* channels, int num_channels, const int* clip_ids, const int* loop)
{
    fx_status st = fx_check_channel_list(c, channels, num_channels);
    if (st != FX_OK || num_channels == 0) return st;
    if (!clip_ids) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null clip id list with %d entries", num_channels);
    for (int i = 0; i < num_channels; i++)
        if (clip_ids[i] != -1 && !bank_of(c, clip_ids[i])) return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: unknown clip id %d", i, clip_ids[i]);
    if ((st = fx_check_channel_entries(c, channels, num_channels)) != FX_OK) return st;
    bool any_rated = false;
    for (int i = 0; i < num_channels; i++) {
        const clip_bank* b = bank_of(c, clip_ids[i]);
        rated_load rl;
        if (!b || !rate_of_load(b->rate[(size_t) (clip_ids[i] - b->first_id)], c->sample_rate, &rl)) continue;
        if (!(rl.ratio >= 0.125 && rl.ratio <= 8.0))
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: clip %d at %.17g Hz in a context at %.17g Hz: the ratio %.17g is outside [1/8, 8]", i, clip_ids[i],
                           b->rate[(size_t) (clip_ids[i] - b->first_id)], c->sample_rate, rl.ratio);
        any_rated = true;
    }
    HIP_TRY(hipSetDevice(c->device));
    fx_clips* s = nullptr;
    if ((st = clips_state(c, &s)) != FX_OK) return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (any_rated && (st = prepare_rated(c, s)) != FX_OK) return st;
    const std::vector<int> keep = last_entries(c, channels, num_channels);
    std::vector<fxk::ClipCommand> commands;
    std::vector<double> rates;
    for (int i : keep) {
        const clip_bank* b = bank_of(c, clip_ids[i]);
        fxk::ClipCommand k{channels[i], fxk::CLIP_OP_LOAD, !loop || loop[i] ? 1 : 0, b ? b->format : 0, nullptr, 0, 0.0, 0.0, 0, {0, 0, 0}};
        double rate = 0.0;
        if (b) {
            k.base = b->mem + b->offset[(size_t) (clip_ids[i] - b->first_id)];
            k.length = b->length[(size_t) (clip_ids[i] - b->first_id)];
            rate = b->rate[(size_t) (clip_ids[i] - b->first_id)];
            rated_load rl;
            if (rate_of_load(rate, c->sample_rate, &rl)) { k.ratio = rl.ratio; k.rho = rl.rho; k.taps = rl.taps; }
        }
        commands.push_back(k);
        rates.push_back(rate);
    }
    if ((st = run_commands(c, s, commands)) != FX_OK) return st;
    for (size_t j = 0; j < keep.size(); j++) {
        const size_t t = (size_t) commands[j].track;
        s->clip_of[t] = clip_ids[keep[j]];
        s->format_of[t] = commands[j].base ? commands[j].format : -1;
        s->rated_of[t] = commands[j].taps > 0;
        s->loaded_under[t] = rates[j] != 0.0 ? c->sample_rate : 0.0;
    }
    if ((st = refresh_rated(c, s)) != FX_OK) return st;
    return fx_clear_pending_channels(c, channels, num_channels);
}

fx_status fx_set_clip_rates(fx_context* c, const int* clip_ids, int num_clips, const double* sample_rates)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (num_clips < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative clip count %d", num_clips);
    if (num_clips == 0) return FX_OK;
    if (!clip_ids) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null clip id list with %d entries", num_clips);
    if (!sample_rates) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null sample rate list with %d entries", num_clips);
    for (int i = 0; i < num_clips; i++)
        if (!std::isfinite(sample_rates[i]) || sample_rates[i] < 0.0)
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: a sample rate is 0 (the context's) or a positive number of Hz, not %g", i, sample_rates[i]);
    for (int i = 0; i < num_clips; i++)
        if (!bank_of(c, clip_ids[i])) return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: unknown clip id %d", i, clip_ids[i]);
    // the rate is the file's: it is set before the clip is loaded
    for (int i = 0; i < num_clips; i++)
        for (int t = 0; t < c->C; t++)
            if (c->clips->clip_of[(size_t) t] == clip_ids[i])
                return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: track %d has clip %d loaded", i, t, clip_ids[i]);
    for (int i = 0; i < num_clips; i++) {
        clip_bank* b = const_cast<clip_bank*>(bank_of(c, clip_ids[i]));
        b->rate[(size_t) (clip_ids[i] - b->first_id)] = sample_rates[i];
    }
    return FX_OK;
}

fx_status fx_get_resampler_table(float* out, int capacity, int* zero_crossings, int* phases)
{
    if (zero_crossings) *zero_crossings = fxk::RS_Z;
    if (phases) *phases = fxk::RS_P;
    if (!out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null output pointer");
    if (capacity < fxk::RS_TABLE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "capacity %d: the table has %d entries", capacity, fxk::RS_TABLE);
    const std::vector<float>& t = resampler_table();
    for (int i = 0; i < fxk::RS_TABLE; i++) out[i] = t[(size_t) i];
    return FX_OK;
}

fx_status fx_set_channel_sources(fx_context* c, const int* channels, int num_channels, const int* types)
{
    fx_status st = fx_check_channel_list(c, channels, num_channels);
    if (st != FX_OK || num_channels == 0) return st;
    if (!types) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null source list with %d entries", num_channels);
    for (int i = 0; i < num_channels; i++)
        if (types[i] != FX_SOURCE_INPUT && types[i] != FX_SOURCE_FILE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: unknown source %d", i, types[i]);
    if ((st = fx_check_channel_entries(c, channels, num_channels)) != FX_OK) return st;
    HIP_TRY(hipSetDevice(c->device));
    fx_clips* s = nullptr;
    if ((st = clips_state(c, &s)) != FX_OK) return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<fxk::ClipCommand> commands;
    for (int i : last_entries(c, channels, num_channels))
        commands.push_back(fxk::ClipCommand{channels[i], types[i] == FX_SOURCE_INPUT ? fxk::CLIP_OP_SOURCE_INPUT : fxk::CLIP_OP_SOURCE_FILE, 0, 0, nullptr, 0, 0.0, 0.0, 0, {0, 0, 0}});
    if ((st = run_commands(c, s, commands)) != FX_OK) return st;
    for (int i = 0; i < num_channels; i++) s->source[(size_t) channels[i]] = types[i];
    if ((st = refresh_rated(c, s)) != FX_OK) return st;
    return fx_clear_pending_channels(c, channels, num_channels);
}

fx_status fx_transport(fx_context* c, const int* channels, int num_channels, int command)
{
    fx_status st = fx_check_channel_list(c, channels, num_channels);
    if (st != FX_OK) return st;
    if (command < FX_PLAY || command > FX_RESTART) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown transport command %d", command);
    if (num_channels == 0) return FX_OK;
    if ((st = fx_check_channel_entries(c, channels, num_channels)) != FX_OK) return st;
    if (command == FX_PLAY)
        for (int i = 0; i < num_channels; i++)
            if (!c->clips || c->clips->clip_of[(size_t) channels[i]] < 0)
                return fx_fail(FX_ERR_INVALID_ARGUMENT, "entry %d: track %d has no file to play", i, channels[i]);
    HIP_TRY(hipSetDevice(c->device));
    fx_clips* s = nullptr;
    if ((st = clips_state(c, &s)) != FX_OK) return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<fxk::ClipCommand> commands;
    for (int i = 0; i < num_channels; i++) commands.push_back(fxk::ClipCommand{channels[i], command, 0, 0, nullptr, 0, 0.0, 0.0, 0, {0, 0, 0}});
    if ((st = run_commands(c, s, commands)) != FX_OK) return st;
    // clearAnalysisBuffers with play, pause and stop (AnalyserTrackController.h:135-137); restart leaves the collectors alone (:138)
    return command == FX_RESTART ? FX_OK : fx_clear_pending_channels(c, channels, num_channels);
}

fx_status fx_get_transport(fx_context* c, int* source, int* state, long long* position, long long* laps)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    fx_clips* s = nullptr;
    fx_status st;
    if ((st = clips_state(c, &s)) != FX_OK) return st;
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<fxk::ClipRow> rows((size_t) c->C);
    HIP_TRY(hipMemcpy(rows.data(), s->d_rows[s->cur], rows.size() * sizeof(fxk::ClipRow), hipMemcpyDeviceToHost));
    for (int t = 0; t < c->C; t++) {
        const fxk::ClipRow& r = rows[(size_t) t];
        if (source) source[t] = r.source;
        if (state) state[t] = r.state;
        if (position) position[t] = r.position;
        if (laps) laps[t] = r.laps;
    }
    return fx_check_device_error(c);
}

fx_status fx_push_sources(fx_context* c, const void* live_block, int num_samples, int sample_format, int mem_kind,
                          float* out_raw, float* out_smoothed, int* frames_out)
{
    if (frames_out) *frames_out = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    c->num_launches = 0;
    if (num_samples < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative sample count");
    { const fx_status cs = fx_check_call(sample_format, mem_kind, mem_kind); if (cs != FX_OK) return cs; }
    if (num_samples == 0) return FX_OK;
    if (live_block && mem_kind == FX_MEM_DEVICE && reinterpret_cast<uintptr_t>(live_block) % 4 != 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "device input must be 4-byte aligned");
    // a rated clip on a FILE track makes the tick fp32, whatever is pending: that refusal names the track
    if (c->clips && sample_format != FX_SAMPLE_F32)
        for (int t = 0; t < c->C; t++)
            if (c->clips->source[(size_t) t] == FX_SOURCE_FILE && c->clips->rated_of[(size_t) t])
                return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: its clip is resampled to fp32, this call is in sample format %d", t, sample_format);
    // fx_push_block's own refusals first, then the table's, all before anything is launched: a refused call changes nothing
    { const fx_status rs = fx_block_refusal(c, num_samples, sample_format); if (rs != FX_OK) return rs; }
    for (int t = 0; t < c->C; t++) {
        const int source = c->clips ? c->clips->source[(size_t) t] : FX_SOURCE_INPUT;
        if (source == FX_SOURCE_INPUT) {
            if (!live_block) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null live block, and track %d's source is the input", t);
        } else if (c->clips->loaded_under[(size_t) t] != 0.0 && c->clips->loaded_under[(size_t) t] != c->sample_rate) {
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: its clip was loaded while the context ran at %.17g Hz, not %.17g: load it again", t,
                           c->clips->loaded_under[(size_t) t], c->sample_rate);
        } else if (c->clips->rated_of[(size_t) t]) {
            // (the call is fp32: checked above)
        } else if (c->clips->format_of[(size_t) t] >= 0 && c->clips->format_of[(size_t) t] != sample_format) {
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: its clip is in sample format %d, this call in %d", t, c->clips->format_of[(size_t) t], sample_format);
        }
    }

    HIP_TRY(hipSetDevice(c->device));
    { const fx_status es = fx_check_device_error(c); if (es != FX_OK) return es; }
    fx_clips* s = nullptr;
    fx_status st;
    if ((st = clips_state(c, &s)) != FX_OK) return st;
    const int esz = (int) sample_size(sample_format);
    const size_t planar_bytes = (size_t) c->C * (size_t) num_samples * (size_t) esz;
    const unsigned char* d_live = static_cast<const unsigned char*>(live_block);
    if (live_block && mem_kind == FX_MEM_HOST) {
        if ((st = fx_grow(&s->d_live, &s->live_cap, planar_bytes)) != FX_OK) return st;
        HIP_TRY(hipMemcpyAsync(s->d_live, live_block, planar_bytes, hipMemcpyHostToDevice, c->stream));
        d_live = s->d_live;
    }
    // (the last piece is stored whole; 32 bytes behind it for the monitor's loads: fx_context.h, monitor_launch)
    if ((st = fx_grow(&s->d_planar, &s->planar_cap, ((planar_bytes + 15) & ~(size_t) 15) + 32)) != FX_OK) return st;
    // (the monitor's room, and its listeners' fp32, before the gather moves the players on: a tick it cannot mix is refused with
    // nothing changed)
    if (c->monitor_prepare && (st = c->monitor_prepare(c, num_samples, sample_format)) != FX_OK) return st;
    fxk::GatherParams p;
    p.rows = s->d_rows[s->cur];
    p.next = s->d_rows[s->cur ^ 1];
    p.live = d_live;
    p.out = s->d_planar;
    p.n = num_samples;
    p.C = c->C;
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_SOURCES, 0)) r->T = num_samples;
    HIP_TRY(fxk::launch_clip_gather_kernel(p, esz, c->stream));
    s->cur ^= 1;            // the launch that wrote the other copy is enqueued: it holds the table
    if (s->num_rated > 0) {
        // (the call is in fp32: a rated FILE track refuses any other format above)
        fxk::ResampleParams rp{p.rows, s->d_rated, s->d_pairs, reinterpret_cast<float*>(s->d_planar), num_samples, s->num_rated, 0};
        if (fx_launch_record* r = note_launch(c, FX_LAUNCH_RESAMPLE, 0)) r->T = num_samples;
        HIP_TRY(fxk::launch_clip_resample_kernel(rp, c->stream));
    }
    // what every track plays is complete: the monitor (fx_monitor.hip) hears it before the analysers do, and the tracks that listen
    // to its output get the mix in place of their own row
    if (c->monitor_launch && (st = c->monitor_launch(c, s->d_planar, num_samples, sample_format)) != FX_OK) return st;
    int frames = 0;
    st = fx_push_block(c, s->d_planar, num_samples, sample_format, FX_MEM_DEVICE, mem_kind, out_raw, out_smoothed, &frames, true);
    if (st != FX_OK) return st;
    // the caller may reuse a host block on return (a call that analysed frames into host memory has synchronised already)
    if (live_block && mem_kind == FX_MEM_HOST && frames == 0) HIP_TRY(hipStreamSynchronize(c->stream));
    if (frames_out) *frames_out = frames;
    return FX_OK;
}

} // extern "C"
