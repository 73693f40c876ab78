// fx_kernels.h -- launch interface between the C-ABI shim (fx_capi.cpp, fx_plan.cpp, fx_stream.cpp) and the gfx950 kernels.
#ifndef FX_KERNELS_H
#define FX_KERNELS_H

#include <hip/hip_runtime.h>
#include "../../include/fx.h"

namespace fxk {

// Number of past frames of raw feature values kept per channel so that smoothing (10-deep
// ValueHistory) and onset detection (<= 32-deep histories of a 10-push RMS mean) of frame t can be
// evaluated without any sequential state: 32 + 9 rounded up.
constexpr int HLEN = 48;
constexpr int MAX_ONSET_WINDOW = 32;
// calls of at most this many frames per channel run finalise + smoothing/onset + history as one kernel (a quarter wavefront per channel)
constexpr int FUSED_TAIL_MAX_FRAMES = 8;

// bytes of one sample of a wire format (FX_SAMPLE_*, include/fx.h; what they widen to: fx_samples.hip.h)
__host__ __device__ constexpr int sample_bytes(int fmt) { return fmt == FX_SAMPLE_F32 ? 4 : (fmt == FX_SAMPLE_S24 ? 3 : 2); }

// What the frame kernel leaves per frame: every reduction over samples / bins / lags is done, the
// scalar tail (pow, log10, sqrt, a few divisions) is not.  One thread per frame finishes it in
// fx_finalise_kernel, where 64 frames share an instruction instead of one.
struct FramePart {
    double mag_sum;     // sum of re^2 over the M bins of the windowed spectrum
    double var;         // sum ((fc/nyq) - (centroid/nyq))^2 * mag (ref SpectralCharacteristics.h:137), summed as the reference writes it:
                        // valid only where `refined` is set; otherwise the finalise kernel forms it from the moments mag_sum, b1, b2
    double lhr;         // magnitudeSum at bin M/5 (inclusive)               (ref :86-87)
    double flux;        // sum of rectified differences, not yet / maxFlux   (ref :76-79)
    double flat_sum;    // flatnessMagnitudeSum                              (ref :91)
    double prod;        // magnitudeProduct with the serial IEEE semantics   (ref :92)
    double max_e;       // maxFFTMagnitude of the slope                      (ref :153-163)
    double b1;          // sum m * mag over the bins m: weightedMagnitudeSum (ref :95) = frpb * (b1 + mag_sum / 2), formed by the finalise kernel
    double vsum;        // sum (mag - mag_sum/M)^2
    double inh;         // inharmonicity before the log                      (ref HarmonicCharacteristics.h:239)
    double her_score;   // sum of the 18 probe maxima                        (ref :157-184)
    double sum_normed;  // sum of mag / max over all bins                    (ref :77); her = score / sum_normed
    double sum_sq;      // sum of the frame's squared samples: rms = (float) sqrt(sum_sq / N)  (ref RealTimeAnalyser.h:207)
    double b2;          // sum m^2 * mag: with mag_sum and b1 the moments the centroid (:127) and the spread (:135-141) are formed from
    float  cnt;         // numMagnitudesUsedInFlatnessCalculation
    float  lag;         // ref PitchAnalyser.h:188-189
    int    flags;       // bit 0: harmonic analyser ran past the 0.005 gate  (ref HarmonicCharacteristics.h:88)
    int    refined;     // bit 0: `var` holds the reference's own sum (the moment form was not trustworthy for this frame, or the pair kernel
                        // summed it); bits 1, 2: the centroid is the float above / below the moments' (fx_wave.hip.h, CENTROID_UP / _DOWN)
};
static_assert(sizeof(FramePart) == 128, "one 128-byte line per frame");

// Per-call scalars of a captured (hipGraph) analysis step.  A graph's kernel arguments are frozen at capture, so what
// changes from call to call lives here, in device memory, refreshed by a copy node at the head of the graph.
struct DynParams {
    double    nyquist;
    long long frames_before;
    long long onset_reset_frame;
    float     gain;
    float     onset_multiplier;
    int       onset_window;
    int       onset_type;
    int       hist_base;            // frames_before mod HLEN (EpilogueParams::hist_base)
};

// Per-track settings (fx_set_channel_gains / fx_set_channel_onset): one row per channel in device memory, allocated by the first
// per-track call.  Until then FrameParams::chan / EpilogueParams::chan are null and every kernel reads the context-wide values it
// always read.  The table's address never changes once it exists (a captured step keeps it); its contents are replaced by copies on
// the context's stream, so they are ordered with the analysis calls.
struct ChannelSettings {
    float     gain;
    float     onset_multiplier;
    int       onset_window;
    int       onset_type;
    long long onset_reset_frame;    // global index of the channel's first frame after its last onset-window reset
    long long first_frame;          // global index of the first frame of the channel's current stream (fx_reset_channels, fx_tracks.hip): what
                                    // the channel's histories hold is counted from here; 0 until the track is reset on its own
};
static_assert(sizeof(ChannelSettings) == 32, "rows are copied as they are");

constexpr int FX_MAX_CHUNKS = FX_MAX_UNITS;

struct FrameParams {
    const void*  in;            // frames [C][T][N] or hops [C][T][N/2]
    int          sample_format; // FX_SAMPLE_F32 / FX_SAMPLE_F16 / FX_SAMPLE_S16 / FX_SAMPLE_S24
    int          hop_mode;      // 1: `in` holds hops, windows are assembled from tail + hops
    int          T;             // frames (= hops) per channel in this call
    int          C;
    int          ch_per_wg;     // channels per workgroup (they share the twiddle table in LDS)
    int          waves_per_ch;  // wavefronts per channel = frames of a channel in flight
    int          direct_state;  // 1: a call of ONE frame per channel with both analysers -- the flux state is read and replaced in global
                                // memory (no LDS copy, no hand-over): T == 1, waves_per_ch == 1, num_chunks == 1
    // A long call over few channels is cut in time as well: num_chunks workgroups per channel group, each analysing
    // frames_per_chunk consecutive frames (many small work units keep every CU busy to the end of the launch; one
    // workgroup per channel is two rounds of 512 at the bench shape, and 8 % slower).  The one thing a chunk needs from
    // the one before it is the channel's flux state: workgroups take their (chunk, channel group) from a ticket counter,
    // chunk-major, so the predecessor's ticket is always lower -- held by a workgroup that is running or done -- and wait
    // for that channel's count of finished chunks.  queue: [0] the ticket counter, [1 + c] finished chunks of channel c;
    // zeroed before the launch.  num_chunks == 1: one workgroup per channel group, no queue.  Chunks need not be equal: long
    // ones first (little overhead), short ones last (the launch's tail is one short unit deep).
    int          num_chunks;
    unsigned*    queue;
    // A work unit that gives up waiting for its predecessor (after spin_limit polls) stores 1 here -- pinned host memory,
    // system scope -- and the host turns that into FX_ERR_HIP at the next synchronisation: a stale flux state is never
    // handed on silently.  debug_flags bit 0 (FX_HOOK_NO_HANDOVER, tests): units do not publish their hand-over, which forces the time-out.
    unsigned*    err;
    unsigned     spin_limit;
    unsigned     debug_flags;
    int          chunk_begin[FX_MAX_CHUNKS + 1];   // chunk k analyses frames [chunk_begin[k], chunk_begin[k + 1]); the last entry used is T
    float        gain;          // hop mode only (ref AudioDataCollector.h:88)
    const float* tail_in;       // [C][N/2] second half of the previous window (already gained)
    float*       tail_out;      // [C][N/2]
    float*       prev_re;       // [C][N/2] real parts of the last accepted spectral frame (flux state)
    const float* tw;            // [N][2] forward twiddles, (float)cos/sin of a double phase, in pass order (build_pass_twiddles)
    FramePart*   part;          // [C][T] per-frame partial results
    double       nyquist;
    double       bin_var;       // sum_i (i/M - 0.5)^2 / M, summed serially on the host (ref SpectralCharacteristics.h:182-189)
    float        lpf_a, lpf_b;  // ref RealTimeAudioAnalysis.h:122
    const DynParams* dyn;       // non-null in a captured step: overrides gain and nyquist
    const float* tw_image;      // 4096 points: the frame kernel's compact LDS image of `tw` (build_twiddle_image), copied as it is
    int          tw_quarter_turn;   // 4096 points: canonical[j + N/4] == (canonical[j].y, -canonical[j].x) bit for bit for the entries the
                                // frame kernel's compact twiddle image derives that way (twiddles_have_quarter_turn); 0: it reads them from `tw`
    float        tw_at_quarter[2];  // canonical[N/4] = ((float) cos(pi/2), -1): the one entry of those that is never a quarter turn of another
    float        first_tw[18];  // the <= 9 twiddles of the first FFT pass (re, im pairs): wave-uniform, so they travel as
                                // kernel arguments (SGPRs) instead of LDS reads; filled by fill_first_pass_twiddles
    // One-frame launches over a buffer of SEVERAL hops per channel (a call of two hops runs as two one-frame launches: measured faster than
    // the batch form at every size): hop-mode input is read as [C][in_hop_stride][N/2] at hop in_hop0 (+ t).  in_hop_stride == 0: [C][T][N/2].
    int          in_hop_stride, in_hop0;
    // fx_push_samples without the re-blocking pass (block_mode = 1; one-frame forms of windows >= 1024 points, both analysers: T == 1,
    // hop_mode == 1): `in` holds every channel's new BLOCK, rows of blk_in_row_bytes back to back; the hop a channel analyses is the
    // first N/2 samples of [its pending samples: blk_carry_in row, blk_carry_bytes valid | its block], and the kernel writes what is left
    // over to the channel's row of blk_carry_out (fx_blocks.hip.h).  Last in the struct: the other forms never look at these.
    int          block_mode;
    int          blk_hop0;      // the hop analysed is hop blk_hop0 of the stream (a call that completes two hops is two one-frame launches)
    int          blk_keep_rest; // this launch writes what the block leaves over (the call's last launch)
    int          blk_carry_bytes, blk_carry_row_bytes;
    long long    blk_in_row_bytes;
    const unsigned char* blk_carry_in;
    unsigned char*       blk_carry_out;
    const ChannelSettings* chan;    // per-track settings, or null: hop-mode input of channel c is scaled by chan[c].gain instead of `gain` (channel_gain)
    // The 1024-point batch form with both analysers (flux state by runs, fx_flux_runs.h): [C][waves_per_ch][N/2] floats, where a wavefront
    // parks the re of its run's first frame until its predecessor's run is over.  Scratch: nothing in it outlives the launch.
    float*       flux_park;
};

struct EpilogueParams {
    const FramePart* part;      // [C][T] from the frame kernel
    float*       raw;           // [C][T][12] raw values: written by fx_finalise_kernel, read by the smoothing kernel
    double       nyquist;
    double       bin_var;
    int          window;
    // what every frame's scalar tail would otherwise divide out for itself, all of it a function of the call's nyquist and window alone:
    // IEEE divisions and a square root done once on the host (the same correctly rounded values), see epilogue_constants()
    double       frpb;          // nyquist / (window / 2)                       (ref SpectralCharacteristics.h:64,105)
    double       inv_nyquist;   // 1.0 / nyquist
    double       inv_bins;      // 1.0 / (window / 2): a power of two, so x * inv_bins == x / (window / 2) exactly
    double       bin_std;       // sqrt(bin_var)                                 (ref :191)
    float*       hist;          // [C][HLEN][12] raw values of the newest HLEN frames, a RING per channel: the row of the frame with
                                // global index g (frames since the last state reset) is g mod HLEN, so a call only writes the rows of
                                // its own frames -- one row per channel for a one-hop call, not the whole table
    int          hist_base;     // frames_before mod HLEN: the ring row this call's first frame goes to
    float*       out_raw;       // [C][T][12] or nullptr
    float*       out_smoothed;  // [C][T][12] or nullptr
    int          out_stride;    // one-frame launches: the output buffers are [C][out_stride][12] and this launch's frame is number out_t0 of its
    int          out_t0;        // channel (a call of two hops = two one-frame launches); out_stride == 0: [C][T][12], frame t
    float*       latest;        // [C][12] smoothed values after the last frame
    int          C, T;
    long long    frames_before; // frames analysed since the last state reset, before this call
    long long    onset_reset_frame; // global index of the first frame after the last onset-window reset
    int          onset_window;  // history length of the OnsetDetector (default 5)
    int          onset_type;
    float        onset_multiplier;
    int          order_mode;    // FX_ORDER_*
    int          analysers;     // bit 0: spectral analyser runs, bit 1: harmonic analyser runs
    const DynParams* dyn;       // non-null in a captured step: overrides nyquist, frames_before, hist_base, onset_*
    unsigned*    clear_queue;   // a call cut in time (FrameParams::num_chunks > 1): its ticket counter and hand-over counts, which the step's
    int          clear_count;   // LAST kernel zeroes for the next call (a memset per call was two fill kernels and their gaps); else null
    const ChannelSettings* chan;    // per-track settings, or null: channel c's detector runs with chan[c] instead of onset_* above (onset_settings)
};

#if defined(__HIPCC__)
// The gain of channel c's hops.  Every caller's c is wave-uniform (a wavefront loads samples of one channel), so the table's value is
// read as a scalar: a load through the constant address space (the table does not change while a kernel runs: its uploads are ordered
// with the launches on the context's stream) at a uniform address is an s_load_dword into an SGPR, like the kernel argument it stands
// in for -- no vector register, no vector-memory instruction.
typedef const float __attribute__((address_space(4)))* UniformFloatPtr;
__device__ __forceinline__ float channel_gain(const ChannelSettings* chan, float gain, int c)
{
    if (!chan) return gain;
    return *(UniformFloatPtr) &chan[__builtin_amdgcn_readfirstlane(c)].gain;
}
__device__ __forceinline__ float channel_gain(const FrameParams& p, int c) { return channel_gain(p.chan, p.gain, c); }
// What channel c's onset detector runs with (not uniform: the tails hold several channels in a wavefront).
struct OnsetSettings { long long reset_frame; int window, type; float multiplier; };
__device__ __forceinline__ OnsetSettings onset_settings(const EpilogueParams& p, int c)
{
    if (!p.chan) return {p.onset_reset_frame, p.onset_window, p.onset_type, p.onset_multiplier};
    const ChannelSettings s = p.chan[c];
    return {s.onset_reset_frame, s.onset_window, s.onset_type, s.onset_multiplier};
}
// Frames of channel c's CURRENT stream analysed before this call: what decides how full its ValueHistorys are.  The ring row of a frame
// stays its global index mod HLEN; rows older than the track's first frame are never valid (RawView::valid), so a reset clears none.
__device__ __forceinline__ long long track_frames_before(const EpilogueParams& p, int c)
{
    return p.chan ? p.frames_before - p.chan[c].first_frame : p.frames_before;
}
#endif

// Completion signal of a one-hop call (fx_hop_kernel): workgroups count themselves in `arrivals` (device memory, zero
// between calls); the last one resets it and stores `seq` to `host_flag` (pinned host memory, system scope), after the
// results -- which the kernel writes to pinned host memory as well -- are visible there.
// (All pointers null: a one-hop call on device-resident input through fx_push_hops -- the stream orders it, nothing to signal.)
struct HopSignal {
    unsigned* arrivals;
    unsigned* host_flag;
    unsigned  seq;
    unsigned  pad_;
    void*     stage;        // device memory, one hop per channel: the kernel copies the hop out of the pinned slot once
                            // (coalesced) and its three wavefronts read it from there (the slot is un-cached memory across PCIe)
};

// fx_push_samples (fx_reblock.hip): per channel, the byte stream [carry_in row: carry_bytes][in row: in_row_bytes] is split into
// out_row_bytes of whole hops (a multiple of 16) for `hops_out` and the remainder (< carry_row_bytes) for `carry_out`.
struct ReblockParams {
    const unsigned char* in;        // [C][in_row_bytes]: the new block, rows back to back (any alignment from the second row on)
    const unsigned char* carry_in;  // [C][carry_row_bytes]: the pending samples of each channel, carry_bytes valid
    unsigned char*       hops_out;  // [C][out_row_bytes]
    unsigned char*       carry_out; // [C][carry_row_bytes]: the other of the context's two carry buffers
    long long            in_row_bytes, out_row_bytes;
    int                  carry_bytes, carry_row_bytes;
    int                  C;
};
constexpr int REBLOCK_THREADS = 256;
// which kernel launch_reblock_kernel runs for p: 0 = fx_reblock_rows_kernel (rows shorter than a workgroup of 16-byte pieces), else the
// pieces per thread of fx_reblock_kernel<1 / 2 / 4>
inline int reblock_form(const ReblockParams& p)
{
    const long long pieces = ((long long) p.carry_bytes + p.in_row_bytes + 15) / 16;
    return pieces < REBLOCK_THREADS ? 0 : (pieces >= 4 * REBLOCK_THREADS ? 4 : (pieces >= 2 * REBLOCK_THREADS ? 2 : 1));
}
hipError_t launch_reblock_kernel(const ReblockParams& p, hipStream_t stream);
hipError_t clear_carry(unsigned char* carry, size_t bytes, hipStream_t stream);

// fx_get_osc_datagrams (fx_osc.hip): message c = OSC message "<prefix><first_channel + c>" with the twelve values of latest[c] in wire
// order (ref OSCFeatureAnalysisOutput.h:107), written at out + c * stride
constexpr int FX_OSC_PREFIX_MAX = 64;
struct OscParams {
    const float*   latest;        // [C][12]
    unsigned char* out;           // [C][stride], 4-byte aligned
    int            C, stride;     // stride: a multiple of 4, >= the longest message
    int            first_channel; // >= 0
    int            prefix_len;    // <= FX_OSC_PREFIX_MAX
    unsigned char  prefix[FX_OSC_PREFIX_MAX];
};
hipError_t launch_osc_kernel(const OscParams& p, hipStream_t stream);

// fx_reset_channels / fx_clear_pending_channels (fx_tracks.hip): rows of the listed channels become zeros in the buffers `clear` names.
// prev / tail / carry rows are row_pieces 16-byte pieces (N/2 * 4 bytes), a latest row is three (12 floats).
enum { FX_CLEAR_PREV = 1, FX_CLEAR_TAIL = 2, FX_CLEAR_CARRY = 4, FX_CLEAR_LATEST = 8 };
struct ResetParams {
    const int* list;            // [n] channels, device memory; every entry in [0, C) (checked by the host, and again by the kernel)
    int        n, C;
    int        row_pieces;
    unsigned   clear;           // FX_CLEAR_*
    float*     prev;            // [C][N/2]
    float*     tail;            // [C][N/2]: the tail the next call reads
    unsigned char* carry;       // [C][N/2 * 4 bytes]: the pending rows the next call reads
    float*     latest;          // [C][12]
};
hipError_t launch_reset_channels_kernel(const ResetParams& p, hipStream_t stream);

// fx_export_channels / fx_import_channels (fx_track_state.hip): a track's whole state as one record of 16-byte pieces --
//   [header: 5][latest vector: 3][ring, 48 rows of 3 in TRACK order][flux row][tail row][pending row], the three rows N/8 pieces each
// -- 2432 + 6 N bytes.  The header is all a destination needs to refuse or to place the record; nothing in a record depends on the
// source context's frame index, ping-pong indices, channel count or slot.
constexpr unsigned TRACK_MAGIC = 0x54527846u;   // "FxRT" as the bytes lie
constexpr unsigned TRACK_LAYOUT_VERSION = 1;
struct TrackHeader {
    unsigned  magic, version;
    int       N;
    unsigned  flags;            // the create flags that shape state: FX_ORDER_MASK | FX_SPECTRAL_ONLY | FX_HARMONIC_ONLY
    int       family;           // wavefronts per frame in force (uses_pairs, fx_plan.h): 1 or 2
    int       pending;          // samples pending per channel (one per context) ...
    int       carry_format;     // ... and their format; FX_SAMPLE_F32 where nothing is pending
    int       onset_window;
    long long frames;           // the track's own frame count: frames_seen - first_frame
    long long onset_frames;     // frames_seen - onset_reset_frame
    float     gain, sensitivity, onset_multiplier;
    int       onset_type;
    unsigned  record_bytes;     // 2432 + 6 N
    unsigned  zero[3];
};
static_assert(sizeof(TrackHeader) == 80, "five 16-byte pieces");
constexpr int TRACK_HEADER_PIECES = 5, TRACK_LATEST_PIECES = FX_NUM_FEATURES / 4, TRACK_ROW_PIECES = FX_NUM_FEATURES / 4;
constexpr int TRACK_RING_PIECES = HLEN * TRACK_ROW_PIECES;
constexpr int TRACK_FIXED_PIECES = TRACK_HEADER_PIECES + TRACK_LATEST_PIECES + TRACK_RING_PIECES;      // 152
inline size_t track_record_pieces(int N) { return (size_t) TRACK_FIXED_PIECES + 3 * (size_t) (N / 8); }
// One list entry as the kernels read it (wave-uniform): the record's header as the host wrote it (export) or read it (import), and the slot.
struct TrackEntry {
    TrackHeader header;
    int         channel;
    int         pad_[3];
};
static_assert(sizeof(TrackEntry) == 96, "entries are 16-byte pieces");
// Where piece q of a record lives in the context's tables.  Ring: record row k holds the track's frame frames - HLEN + k, whose global
// index is frames_seen - HLEN + k, so it is ring row (hist_base + k) mod HLEN with hist_base = frames_seen mod HLEN -- the same
// rotation for every track of a context, and pieces map to pieces (a row is three).  `at`: the piece within the channel's row(s) of
// that table; ring_row: the RECORD's row k (its frame exists iff frames - HLEN + k >= 0).
enum { TRACK_IN_HEADER = 0, TRACK_IN_LATEST, TRACK_IN_RING, TRACK_IN_PREV, TRACK_IN_TAIL, TRACK_IN_CARRY };
struct TrackPiece { int where, at, ring_row; };
__host__ __device__ inline TrackPiece track_piece(int q, int row_pieces, int hist_base)
{
    if (q < TRACK_HEADER_PIECES) return {TRACK_IN_HEADER, q, 0};
    q -= TRACK_HEADER_PIECES;
    if (q < TRACK_LATEST_PIECES) return {TRACK_IN_LATEST, q, 0};
    q -= TRACK_LATEST_PIECES;
    if (q < TRACK_RING_PIECES) {
        const int k = q / TRACK_ROW_PIECES;
        int row = hist_base + k;
        if (row >= HLEN) row -= HLEN;
        return {TRACK_IN_RING, row * TRACK_ROW_PIECES + (q - k * TRACK_ROW_PIECES), k};
    }
    q -= TRACK_RING_PIECES;
    const int which = q / row_pieces;
    return {TRACK_IN_PREV + which, q - which * row_pieces, 0};
}
// the bytes of word w of piece `at` of a pending row that lie below carry_bytes, as a mask (the rest of a record's pending row is zeros)
__host__ __device__ inline unsigned track_carry_mask(int at, int w, int carry_bytes)
{
    const int left = carry_bytes - (at * 16 + w * 4);
    return left >= 4 ? 0xffffffffu : (left <= 0 ? 0u : (1u << (8 * left)) - 1u);
}
struct TrackStateParams {
    const TrackEntry* entries;  // [n], device memory; every channel in [0, C) (checked by the host, and again by the kernels)
    int        n, C;
    int        row_pieces;      // N / 8
    int        hist_base;       // frames_seen mod HLEN
    int        carry_bytes;     // pending samples x their size
    float*     prev;            // [C][N/2]
    float*     tail;            // [C][N/2]: the tail the next call reads
    unsigned char* carry;       // [C][N/2 * 4 bytes]: the pending rows the next call reads
    float*     hist;            // [C][HLEN][12]
    float*     latest;          // [C][12]
    unsigned char* records;     // [n][track_record_pieces x 16], 16-byte aligned
};
hipError_t launch_pack_tracks_kernel(const TrackStateParams& p, hipStream_t stream);      // tables -> records (writes every byte of them)
hipError_t launch_unpack_tracks_kernel(const TrackStateParams& p, hipStream_t stream);    // records -> tables (the header is the host's)

// Re-order the reference's N-entry twiddle table (canonical[i] = (re, im) of e^{-2*pi*i/N} as floats)
// into the order the FFT passes read it; `out` has room for window_size complex entries.
void build_pass_twiddles(int window_size, const float* canonical, float* out);
// the first pass's constants, taken from the same pass-ordered table
void fill_first_pass_twiddles(int window_size, const float* pass_ordered, float* out18);
bool first_pass_twiddles_hermitian(int window_size, const float* first18);   // must hold before any launch
// FrameParams::tw_image: the frame kernel's LDS twiddle image where it is not the pass-ordered table itself (4096 points: CompactTw,
// fx_fft.hip.h).  Returns the number of complex entries written to `out` (room for window_size), 0 where the kernel copies `tw`.
int build_twiddle_image(int window_size, const float* pass_ordered, float* out);
// FrameParams::tw_quarter_turn for this table (the reference's N-entry table, canonical order); true where the kernel does not ask
bool twiddles_have_quarter_turn(int window_size, const float* canonical);

size_t frame_kernel_lds_bytes(int window_size, int channels_per_wg, int waves_per_channel, bool direct_state = false);
int frame_kernel_max_waves(int window_size);     // the frame kernel's launch bound, in wavefronts per workgroup
// measured-best workgroup shape for a window size: channels per workgroup x wavefronts per channel
void frame_kernel_preferred_shape(int window_size, int* channels_per_wg, int* waves_per_channel);
// Launches ceil(C / p.ch_per_wg) workgroups of p.ch_per_wg * p.waves_per_ch wavefronts; returns hipSuccess or the launch error.
hipError_t launch_frame_kernel(int window_size, const FrameParams& p, int analysers, hipStream_t stream);
// fills EpilogueParams::frpb .. bin_std from nyquist, window and bin_var (host and device: a captured step re-derives them from its DynParams)
__host__ __device__ inline void epilogue_constants(EpilogueParams& p)
{
    const double bins = (double) (p.window / 2);
    p.frpb = p.nyquist / bins;
    p.inv_nyquist = 1.0 / p.nyquist;
    p.inv_bins = 1.0 / bins;
    p.bin_std = sqrt(p.bin_var);
}
// which kernels launch_epilogue_kernels runs for p: 1 = fx_tail_fused_kernel, 2 = fx_finalise_kernel + fx_epilogue_kernel + fx_history_kernel
inline int epilogue_form(const EpilogueParams& p) { return p.T <= FUSED_TAIL_MAX_FRAMES ? 1 : 2; }
// p.out_stride != 0 (the frame of a one-frame launch inside a longer call) is honoured by the one-frame tail only: other T are refused
hipError_t launch_epilogue_kernels(const EpilogueParams& p, hipStream_t stream);
// launch_frame_kernel (p.direct_state: one frame per channel, one wavefront each) and launch_epilogue_kernels in ONE launch: the
// workgroup's first wavefronts finish its channels' hops when the frames are done (fx_frame_tail_kernel)
hipError_t launch_frame_tail_kernel(int window_size, const FrameParams& p, const EpilogueParams& ep, hipStream_t stream);
bool frame_tail_kernel_available(int window_size);   // windows of 1024 points and more (below that it is not built: it loses to two launches)
hipError_t prepare_kernels(int window_size);   // raises the kernels' dynamic-LDS limit on the CURRENT device (every fx_create: the attribute is per device)
hipError_t prepare_hop_kernel(int window_size);   // the same for fx_hop_kernel; hipSuccess where there is none for this size
// One frame across a PAIR of wavefronts (windows of 2048 / 4096 points, both analysers): p.waves_per_ch is then the number
// of pairs (= frames of a channel in flight) and a workgroup has p.ch_per_wg * p.waves_per_ch * 128 threads.
bool pair_kernel_available(int window_size);
int pair_kernel_max_pairs(int window_size);
size_t pair_kernel_lds_bytes(int window_size, int channels_per_wg, int pairs_per_channel);
hipError_t prepare_pair_kernel(int window_size);
hipError_t launch_pair_kernel(int window_size, const FrameParams& p, hipStream_t stream);
// One hop per channel, whole step in one launch (three wavefronts per channel + the tail), results and completion flag
// written by the kernel itself; p.T must be 1, p.hop_mode 1, both analysers on.  Window sizes: hop_kernel_available().
bool hop_kernel_available(int window_size);
// pairs: windows of 2048 / 4096 points with every analyser on a pair of wavefronts (six per channel; fx_hop_pair_kernel)
hipError_t launch_hop_kernel(int window_size, const FrameParams& p, const EpilogueParams& ep, const HopSignal& sig, hipStream_t stream, bool pairs = false);

} // namespace fxk

// Test hooks, NOT part of the public ABI (include/fx.h does not declare this; the library exports it for tests/ only).  Bits:
//   0  work units of a cut launch do not publish their hand-over (forces the time-out that FX_ERR_HIP reports)
//   1  the 4096-point kernel takes no twiddle from a quarter turn of another (the path of a host whose cos / sin lack that
//      symmetry: same values, read from the whole table)
//   2 / 3  one-frame calls through the batch kernels never / always finish the hop's tail in the frame kernel (default: while the
//      chip holds the call's workgroups at once)
//   4  fx_push_samples never feeds a block to the one-frame kernels directly (FrameParams::block_mode): every call re-blocks first, as
//      calls that complete several hops do
//   5  a call of two hops per channel runs the batch kernels' two-frame form instead of two one-frame launches
//   6  fx_export_channels / fx_import_channels move a HOST buffer's records through the device scratch two at a time (default: 32 MB a chunk)
//   7  the RTP reorder window's tick numbers (fx_rtp.hip: the stamps' upper half) start over after 3 (default: after 2^32 - 1)
// None changes a result bit (bit 0 makes the call fail, as it must).
#define FX_HOOK_NO_HANDOVER      1u
#define FX_HOOK_NO_QUARTER_TURN  2u
#define FX_HOOK_TAIL_NEVER_FUSED 4u
#define FX_HOOK_TAIL_ALWAYS_FUSED 8u
#define FX_HOOK_NO_BLOCK_FEED    16u
#define FX_HOOK_NO_TWO_LAUNCHES  32u
#define FX_HOOK_SMALL_TRACK_CHUNKS 64u
#define FX_HOOK_RTP_FEW_TICK_NUMBERS 128u
extern "C" fx_status fx_set_tuning_internal(fx_context* ctx, unsigned test_hooks);

// Launch record, NOT part of the public ABI (tests only): the launches the context's last call made -- fx_push_hops, fx_process_frames,
// fx_push_samples, fx_stream_submit(_samples), fx_get_osc_datagrams each start a new one; a captured ring step replays the record it made
// at capture.  Fields that do not apply to a launcher are 0.  A taps launch (fx_taps.hip) records T = the channels it captures and
// block_mode = 1 when it reads [pending | block].  A de-interleave launch (fx_interleave.hip) records T = the block's samples per channel.
enum { FX_LAUNCH_FRAME = 1, FX_LAUNCH_FRAME_TAIL, FX_LAUNCH_HOP, FX_LAUNCH_HOP_PAIR, FX_LAUNCH_PAIR, FX_LAUNCH_EPILOGUE, FX_LAUNCH_REBLOCK,
       FX_LAUNCH_OSC, FX_LAUNCH_TAPS, FX_LAUNCH_DEINTERLEAVE };
// The onset event list's step (fx_events.hip), the last entry of an analysis call on a context with events enabled: ONE entry and one
// launch per call (counts, scan and records in one kernel), T = the frames per channel the call analysed.
constexpr int FX_LAUNCH_ONSET_EVENTS = 11;
// fx_get_osc_datagrams_addressed (fx_osc_table.hip): one launch of fx_osc_table_kernel; it starts a new record, as fx_get_osc_datagrams does.
constexpr int FX_LAUNCH_OSC_TABLE = 12;
// fx_get_osc_bundles / fx_get_osc_bundles_addressed (fx_osc_bundle.hip): one launch of fx_osc_bundle_kernel; it starts a new record too.
// T = the tracks per bundle.
constexpr int FX_LAUNCH_OSC_BUNDLE = 13;
// The audio display's step (fx_display.hip), the last entry of an analysis call on a context with the display enabled: ONE launch of
// fx_display_kernel per call, T = the frames per channel the call analysed.
constexpr int FX_LAUNCH_DISPLAY = 14;
// fx_push_sources (fx_clips.hip): one launch of fx_clip_gather_kernel, the FIRST entry of the call's record; T = the samples per track
// the call forms.  The entries after it are those of fx_push_samples on the planar block it made.
constexpr int FX_LAUNCH_SOURCES = 15;
// fx_push_sources while a FILE track has a rated clip loaded: one launch of fx_clip_resample_kernel, the SECOND entry of the call's
// record, after the gather; T = the samples per track.  A context without such a track records no entry of this kind.
constexpr int FX_LAUNCH_RESAMPLE = 16;
// fx_push_sources on a context with the monitor enabled (fx_monitor.hip): the mix of the tick's planar block, after the gather and the
// resampler and before the entries of fx_push_samples; ONE entry for its one or two launches (fx_monitor_mix_kernel, and
// fx_monitor_sum_kernel where the context has more than one group of FX_MONITOR_GROUP tracks); T = the samples per track.
constexpr int FX_LAUNCH_MONITOR = 17;
// fx_push_sources while a track listens to a monitor output (fx_set_channel_listen): one launch of fx_monitor_listen_kernel, the entry
// directly after the monitor's; T = the samples per track.  A context in which no track listens records no entry of this kind.
constexpr int FX_LAUNCH_LISTEN = 18;
// fx_push_rtp (fx_rtp.hip): the unpack of a tick's datagrams, the FIRST entry of the call's record; ONE entry for its launches (the
// owner table's fill, fx_rtp_parse_kernel where the tick has packets, fx_rtp_gather_kernel, fx_rtp_count_kernel); T = the samples per
// track the call forms.  The entries after it are those of fx_push_samples on the planar block it made.
constexpr int FX_LAUNCH_RTP = 19;
struct fx_launch_record {
    int kind;               // FX_LAUNCH_*
    int window, analysers;  // window size, analysers mask (bit 0 spectral, bit 1 harmonic)
    // frame, frame_tail, pair, hop, hop_pair: the FrameParams fields that choose the kernel's form (hop launches: one workgroup per channel,
    // ch_per_wg / waves_per_ch / num_chunks are not read and recorded as 0)
    int T, direct_state, block_mode, num_chunks, ch_per_wg, waves_per_ch, hop_pairs;
    int ep_T, out_stride;   // frame_tail, hop, hop_pair, epilogue: EpilogueParams::T, ::out_stride
    int ep_form;            // epilogue: fxk::epilogue_form
    int reblock;            // reblock: fxk::reblock_form
};
constexpr int FX_LAUNCH_RECORD_CAP = 8;
// copies up to `cap` records of the last call to `out`; returns how many launches that call made (more than cap: the rest were not kept)
extern "C" int fx_last_launches_internal(fx_context* ctx, fx_launch_record* out, int cap);
#endif
