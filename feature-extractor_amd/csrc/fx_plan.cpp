// fx_plan.cpp -- the call planner behind the C ABI (include/fx.h): what an analysis call of T frames per channel launches -- how it is
// cut in time, which kernels in which workgroup shape -- and fx_run, the one place that enqueues a planned call.  Host code only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fx_plan.h"

// Which kernel family a context runs (include/fx.h, FX_LOW_LATENCY): frames across a PAIR of wavefronts -- windows of 2048 / 4096
// points with both analysers -- when the create flag asks for it, or when the tuning knob forces either (experiments, tests).
bool uses_pairs(const fx_context* c, int waves_per_frame)
{
    if (!fxk::pair_kernel_available(c->N) || (c->flags & (FX_SPECTRAL_ONLY | FX_HARMONIC_ONLY))) return false;
    return waves_per_frame == 2 || (waves_per_frame == 0 && (c->flags & FX_LOW_LATENCY));
}

// Long calls are cut in time as well (FrameParams::num_chunks): work units of ~200 us -- long enough to carry a
// workgroup's prologue and the hand-over, short enough for many rounds of them.  Measured (1024 ch x 512 frames, best
// of three interleaved runs): 8 frames per wavefront for the full bundle at 1024 points (2.80 against 3.01 ms uncut),
// twice that with the harmonic analyser alone (1.93 / 2.04), more for the small windows (512 points +3 %, 256 points
// +2 %); nothing for the spectral analyser alone, and a LOSS of 3-8 % at 2048 and 4096 points, whose workgroups carry
// a 16-32 KB twiddle table each and already run in 4-8 rounds at their usual shapes: those are never cut.  Calls of up
// to 8 units are cut into equal units; longer ones into units of decreasing length -- a third of what is left each
// time (at most four units' worth), down to a quarter unit -- long units first (little overhead), short ones last (the
// launch's tail is one short unit deep): 512 frames = 168, 112, 80, 48, 32, 24, 16, 16, 16 (2.74 against 2.80 ms for
// eight units of 64 at the bench shape).  fx_tuning::frames_per_unit overrides the unit (0 = never cut), fx_tuning::unit_plan
// gives the lengths outright (experiments).  Host-only arithmetic, pure (no environment, no device): declared in
// include/fx.h so that the CPU tests can hold it to its invariants.
extern "C" int fx_plan_units(int window_size, unsigned flags, int waves_per_channel, int num_frames, const fx_tuning* tuning, int* sizes, int cap)
{
    const int k = waves_per_channel, T = num_frames;
    if (!sizes || cap < 1 || k < 1 || T < 1) return 0;
    if (T < 2 * k) { sizes[0] = T; return 1; }          // (a few hops: nothing to cut, and the one-hop path is latency-critical)
    int per_wave = window_size <= 256 ? 32 : (window_size == 512 ? 16 : 8);
    if (flags & FX_HARMONIC_ONLY) per_wave *= 2;
    int unit = (window_size > 1024 || (flags & FX_SPECTRAL_ONLY)) ? 0 : k * per_wave;
    if (tuning && tuning->frames_per_unit >= 0) unit = tuning->frames_per_unit;
    int n = 0;
    if (tuning && tuning->unit_plan_len > 0 && tuning->unit_plan_len <= cap && tuning->unit_plan_len <= FX_MAX_UNITS) {
        int sum = 0;
        for (int i = 0; i < tuning->unit_plan_len; i++) { const int v = tuning->unit_plan[i]; if (v <= 0) { sum = -1; break; } sizes[n++] = v; sum += v; }
        if (sum != T) n = 0;
    }
    if (n == 0 && unit >= k && unit > 0) {
        if (T >= 8 * unit) {
            const int least = unit / 4 > k ? unit / 4 / k * k : k;
            for (int rem = T; rem > 0 && n < cap; ) {
                int sz = (rem / 3 + k / 2) / k * k;
                if (sz < least) sz = least;
                if (sz > 4 * unit && T <= 4 * unit * (cap - 10)) sz = 4 * unit;       // (no unit longer than ~1 ms)
                if (rem - sz < least || n == cap - 1) sz = rem;
                sizes[n++] = sz;
                rem -= sz;
            }
        } else {
            const int cnt = (2 * T + unit) / (2 * unit);                  // T / unit, rounded
            if (cnt >= 2 && cnt <= cap) {
                int per = (T + cnt - 1) / cnt;
                per = (per + k - 1) / k * k;                               // whole rounds of the k wavefronts
                for (int at = 0; at < T; at += per) sizes[n++] = at + per < T ? per : T - at;
            }
        }
    }
    if (n < 2) { sizes[0] = T; n = 1; }
    return n;
}

// Plan the launches of a call of T frames per channel from the context's current state: no HIP call, no change to the context.  `part` /
// `raw` are the epilogue's scratch (the context's own for fx_run(); a captured step passes buffers it owns, because a graph keeps the
// addresses it was captured with); `dyn`: the per-call scalars a captured step reads from memory.
fx_status plan_call(const fx_context* c, const void* d_in, int T, int sample_format, int hop_mode, float* d_or, float* d_os,
                    const BlockFeed* blocks, const fxk::DynParams* dyn, fxk::FramePart* part, float* raw, Route route, Plan* plan)
{
    const int analysers = (c->flags & FX_SPECTRAL_ONLY) ? 1 : ((c->flags & FX_HARMONIC_ONLY) ? 2 : 3);
    // The low-latency family (opt-in: FX_LOW_LATENCY, or fx_tuning::waves_per_frame = 2): windows of 2048 / 4096 points with both
    // analysers run one frame across a PAIR of wavefronts -- fx_pair_kernel for calls of several frames, fx_hop_pair_kernel for
    // one frame per call.  The default family keeps a frame in one wavefront at every size (profiles/NOTEBOOK_design_r1-r5.md: pairs are the faster
    // path for one hop, not for throughput).
    const bool pair = uses_pairs(c, c->tuning.waves_per_frame);

    // A call of TWO hops per channel (a 1024-sample device buffer against a 1024-point window, 960-sample blocks every other call ...) runs
    // as two one-frame launches over the same buffers -- the second reads hop 1 and writes frame 1 (FrameParams::in_hop_stride / in_hop0,
    // EpilogueParams::out_stride / out_t0) -- and, like a one-frame call, records no timing events unless asked to.  Measured
    // (tools/device_blocks.py, us per call of two hops: batch form with its events / batch form without / two one-frame launches):
    // 8192 channels x 1024 points 144 / 136.6 / 133.8; 1024 x 1024 52 / 42.6 / 39.7; 4096 x 2048 165 / 154.9 / 157.1; 512 x 2048 - / 50.4 / 46.3;
    // 1024 x 4096 137 / 127.1 / 123.4; 256 x 4096 - / 66.7 / 57.1.  Most of what a two-hop call cost over two one-hop calls was the three event
    // records (barrier packets); the launches themselves are worth 0 - 14 %.  What this form really buys is the block feed: a block that
    // completes two hops is read by the kernels directly (1000-sample blocks at 8192 channels: 177 -> 132 us per call).
    const bool in_two = hop_mode && T == 2 && analysers == 3 && c->N >= 1024 && !pair && !(c->test_hooks & FX_HOOK_NO_TWO_LAUNCHES);
    const bool split = route == ROUTE_AUTO && (in_two || (blocks && T <= 2));   // (a block feed of more hops is ONE launch of the batch kernel's block-fed form)
    plan->parts = split ? T : 1;
    const int part_T = split ? 1 : T;
    // The three events fx_last_kernel_ms() reads.  Each is a barrier packet between launches, which a call of milliseconds does not
    // notice and a one-frame call does (back to back 27 us per call with them, 14.6 without): those record none unless asked to.
    // (a call made of one-frame launches is a live call: no events by default, like a one-frame call; a ring step records none)
    plan->timed = route == ROUTE_AUTO && (c->profiling || c->tuning.call_timing == 1 || (c->tuning.call_timing < 0 && part_T > 1));

    Launch base;
    base.analysers = analysers;
    fxk::FrameParams& fp = base.fp;
    fp.in = d_in;
    fp.sample_format = sample_format;
    fp.hop_mode = hop_mode;
    fp.T = part_T;
    fp.C = c->C;
    fp.gain = c->gain;
    fp.chan = c->d_chan;
    fp.prev_re = c->d_prev;
    fp.flux_park = c->d_flux_park;
    fp.tw = c->d_tw;
    fp.tw_image = c->d_tw + 2 * (size_t) c->N;
    fp.part = part;
    fp.nyquist = c->sample_rate / 2.0;          // ref RealTimeAudioAnalysis.h:251, RealTimeAnalyser.h:113
    fp.bin_var = c->bin_var;
    fp.lpf_a = c->lpf_a;
    fp.lpf_b = c->lpf_b;
    fp.dyn = dyn;
    for (int i = 0; i < 18; i++) fp.first_tw[i] = c->first_tw[i];
    fp.tw_quarter_turn = (c->tw_quarter_turn && !(c->test_hooks & FX_HOOK_NO_QUARTER_TURN)) ? 1 : 0;
    fp.tw_at_quarter[0] = c->tw_at_quarter[0]; fp.tw_at_quarter[1] = c->tw_at_quarter[1];
    fp.block_mode = 0; fp.blk_carry_bytes = fp.blk_carry_row_bytes = 0; fp.blk_in_row_bytes = 0; fp.blk_carry_in = nullptr; fp.blk_carry_out = nullptr;
    fp.blk_hop0 = 0; fp.blk_keep_rest = 0; fp.in_hop_stride = 0; fp.in_hop0 = 0;

    // Workgroup shape: channels per workgroup x wavefronts per channel (= frames of one channel in flight): the
    // measured-best shape for this window size, fewer waves when the call has fewer frames, fewer channels when the
    // context has fewer or the LDS holds fewer (one twiddle table per workgroup, one flux state per channel, one
    // transform buffer per wave).  fx_tuning overrides for experiments.
    const size_t lds_cu = 160 * 1024;
    const int kcap = pair ? fxk::pair_kernel_max_pairs(c->N) : fxk::frame_kernel_max_waves(c->N);
    // one frame per call through the batch kernels (both analysers): the flux state stays in global memory (FrameParams::direct_state)
    const bool direct = part_T == 1 && !pair && analysers == 3;
    fp.direct_state = direct ? 1 : 0;
    auto lds_bytes = [&](int ch_, int k_) { return pair ? fxk::pair_kernel_lds_bytes(c->N, ch_, k_) : fxk::frame_kernel_lds_bytes(c->N, ch_, k_, direct); };
    int ch = 1, k = 1;
    if (pair) { ch = 1; k = kcap; }
    else fxk::frame_kernel_preferred_shape(c->N, &ch, &k);
    if (c->tuning.waves_per_channel >= 1) k = c->tuning.waves_per_channel;
    if (c->tuning.channels_per_workgroup >= 1) ch = c->tuning.channels_per_workgroup;
    if (k > part_T) k = part_T;
    if (k > kcap) k = kcap;
    // one frame per call through the batch kernels: one wavefront per channel, so channels share a workgroup's twiddle table.
    // With the flux state in global memory (direct), up to 1024 points as many as a workgroup may hold (1024 points: 8 channels =
    // 76 KB, two workgroups and 16 wavefronts per CU -- what the LDS holds of the batch shape too); at the split sizes the registers
    // allow 8 wavefronts per CU whatever the shape, and a CU does better with two workgroups of four (staggered) than with one of
    // eight in lockstep (2048 points), or with one workgroup of eight from the channel count at which every CU has one (4096 points,
    // whose eight wavefronts are all a CU holds).  Measured, us per call of one hop per channel, channels per workgroup 4 / 8 --
    // profiles/r04_live_cadence.txt:
    //   1024 points  4096 ch 43.4 / 39.1   8192 ch 66.6 / 63.3   16384 ch 116.8 / 111.1
    //   2048 points  2048 ch 44.8 / 43.2   4096 ch 72.0 / 73.0    8192 ch 125.4 / 133.6
    //   4096 points  1024 ch 61.7 / 71.0   2048 ch 108.7 / 75.7   4096 ch 205.4 / 139.6
    // Without the direct form (one analyser only): four (2048 points, 4096 channels x 1 hop 152 us against 193 us with one).
    if (part_T == 1 && !pair && c->tuning.channels_per_workgroup < 1)
        ch = !direct ? 4 : (c->N <= 1024 ? kcap : (c->N == 2048 ? 4 : (c->C >= 2048 ? kcap : 4)));
    // Two frames per call (a 1024-sample device block against a 1024-point window: the live cadence of hosts with larger buffers): two channels
    // per workgroup share the twiddle table.  Measured (tools/device_blocks.py, us per call of two hops, channels per workgroup 1 / 2 / 4):
    // 8192 channels x 1024 points 164.8 / 144.4 / 183.3; 4096 channels x 2048 points 169.8 / 163.5 / 172.9.  Four frames per call: one.
    if (part_T == 2 && !pair && c->N <= 2048 && c->tuning.channels_per_workgroup < 1) ch = 2;
    if (ch > c->C) ch = c->C;
    while (ch > 1 && (ch * k > kcap || lds_bytes(ch, k) > lds_cu)) ch--;
    while (k > 1 && lds_bytes(ch, k) > lds_cu) k--;
    if (lds_bytes(ch, k) > lds_cu)
        return fx_fail(FX_ERR_UNSUPPORTED, "window size %d does not fit the LDS", c->N);
    if (blocks && (pair || analysers != 3)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "this context's kernels do not read blocks");
    fp.ch_per_wg = ch;
    fp.waves_per_ch = k;
    fp.num_chunks = 1;
    fp.queue = nullptr;
    fp.err = c->d_err;
    fp.spin_limit = c->tuning.handover_spin_limit > 0 ? (unsigned) c->tuning.handover_spin_limit : (1u << 22);
    fp.debug_flags = c->test_hooks;
    for (int i = 0; i <= fxk::FX_MAX_CHUNKS; i++) fp.chunk_begin[i] = 0;
    if (route != ROUTE_RING_CAPTURED) {
        int sizes[fxk::FX_MAX_CHUNKS];
        const int n = fx_plan_units(c->N, c->flags, k, part_T, &c->tuning, sizes, fxk::FX_MAX_CHUNKS);
        if (n >= 2) {
            fp.num_chunks = n;
            fp.queue = c->d_queue;
            for (int i = 0; i < n; i++) fp.chunk_begin[i + 1] = fp.chunk_begin[i] + sizes[i];
        }
    }

    fxk::EpilogueParams& ep = base.ep;
    ep.part = part;
    ep.raw = raw;
    ep.nyquist = c->sample_rate / 2.0;
    ep.bin_var = c->bin_var;
    ep.window = c->N;
    fxk::epilogue_constants(ep);
    ep.hist = c->d_hist;
    ep.out_raw = d_or;
    ep.out_smoothed = d_os;
    ep.out_stride = 0; ep.out_t0 = 0;
    ep.latest = c->d_latest;
    ep.C = c->C;
    ep.T = part_T;
    ep.onset_reset_frame = c->onset_reset_frame;
    ep.onset_window = c->onset_window;
    ep.onset_type = c->onset_type;
    ep.onset_multiplier = c->onset_multiplier;
    ep.chan = c->d_chan;
    ep.order_mode = (int) (c->flags & FX_ORDER_MASK);
    ep.analysers = analysers;
    ep.dyn = dyn;
    ep.clear_queue = fp.num_chunks > 1 ? c->d_queue : nullptr;
    ep.clear_count = 1 + c->C;

    // ONE frame per channel -- the reference's own cadence, an analysis per hop as it arrives (AudioDataCollector.h:66-94,
    // RealTimeAnalyser.h:201-234) -- is one launch of fx_hop_kernel: three wavefronts per channel (pitch / spectral /
    // harmonic) and the hop's tail, instead of one wavefront per channel and a second launch.
    // (measured, tools/live_cadence.py, profiles/r04_live_cadence.txt: once the call holds more than the chip takes in one round of
    // workgroups -- 1024 channels of 1024 points, 512 of 2048, and 1024 of 4096 since a 4096-point workgroup is 80 KB and a CU holds two --
    // the batch kernels take over: one wavefront per channel with the flux state left in global memory (direct_state above), then the fused
    // tail on a quarter wavefront per channel: 63 against 120 us at 8192 channels x 1024-pt, 76 against 186 us at 2048 channels x 4096-pt;
    // below it the hop kernel wins, 19.9 against 22.9 us at 1024 x 1024-pt, 58.7 against 61.8 us at 1024 x 4096-pt.  The pair family's
    // hop kernel -- six wavefronts and 100 KB per channel -- keeps 2^20 at every size)
    const bool one_hop = route == ROUTE_RING_HOP ||
                         (route == ROUTE_AUTO && part_T == 1 && analysers == 3 && fxk::hop_kernel_available(c->N) &&
                          (c->tuning.one_hop_kernel == 1 || (c->tuning.one_hop_kernel < 0 && (long long) c->C * c->N <= ((c->N == 4096 && !pair) ? (1ll << 22) : (1ll << 20)))));
    // One frame per channel through the batch kernels: frames and tails in ONE launch (fx_frame_tail_kernel) while the chip holds all
    // of the call's workgroups at once -- two per CU at these sizes, one of eight channels at 4096 points.  Beyond that a workgroup whose
    // first wavefronts are finishing its hops keeps the LDS the next workgroup is waiting for, and the tail is better off as a launch
    // of its own.  Measured (us per call, one launch / two; profiles/r04_live_cadence.txt): 1024 points 2048 channels 26.8 / 28.6, 4096
    // channels 41.0 / 41.7, 8192 channels 70.2 / 68.2; 2048 points 2048 channels 44.9 / 45.7, 4096 channels 77.5 / 73.8; windows of 512
    // points and fewer lose either way (4096 channels 34.7 / 33.2): their frames are no longer than the tail.
    const long long groups = ((long long) c->C + ch - 1) / ch;
    const long long one_round = (long long) c->compute_units * ((c->N == 4096 && ch > 4) ? 1 : 2);
    const bool one_launch = route == ROUTE_AUTO && direct && fxk::frame_tail_kernel_available(c->N) &&
                            ((c->test_hooks & FX_HOOK_TAIL_ALWAYS_FUSED) || (!(c->test_hooks & FX_HOOK_TAIL_NEVER_FUSED) && groups <= one_round));
    const int frames_kind = one_hop ? (pair ? FX_LAUNCH_HOP_PAIR : FX_LAUNCH_HOP) : (one_launch ? FX_LAUNCH_FRAME_TAIL : (pair ? FX_LAUNCH_PAIR : FX_LAUNCH_FRAME));

    plan->n = 0;
    for (int p = 0; p < plan->parts; p++) {
        // part p runs on the state as parts 0 .. p-1 leave it
        Launch l = base;
        l.fp.tail_in = c->d_tail[c->cur ^ (p & 1)];
        l.fp.tail_out = c->d_tail[c->cur ^ (p & 1) ^ 1];
        l.ep.frames_before = c->frames_seen + p;
        l.ep.hist_base = (int) ((c->frames_seen + p) % fxk::HLEN);
        if (plan->parts > 1) {
            l.fp.in_hop_stride = T; l.fp.in_hop0 = p;
            l.ep.out_stride = T;    l.ep.out_t0 = p;
        }
        if (blocks) {
            l.fp.block_mode = 1;
            l.fp.blk_hop0 = p;
            l.fp.blk_keep_rest = p == plan->parts - 1 ? 1 : 0;
            l.fp.blk_carry_in = blocks->carry_in;
            l.fp.blk_carry_out = blocks->carry_out;
            l.fp.blk_carry_bytes = blocks->carry_bytes;
            l.fp.blk_carry_row_bytes = blocks->carry_row_bytes;
            l.fp.blk_in_row_bytes = blocks->in_row_bytes;
        }
        l.kind = frames_kind;
        plan->launch[plan->n++] = l;
        if (frames_kind == FX_LAUNCH_FRAME || frames_kind == FX_LAUNCH_PAIR) {
            l.kind = FX_LAUNCH_EPILOGUE;
            plan->launch[plan->n++] = l;
        }
    }
    return FX_OK;
}

// The launch record entry of a planned launch (a captured ring step writes these again each time its graph is replayed)
void note_planned(fx_context* c, const Launch& l)
{
    fx_launch_record* r = note_launch(c, l.kind, l.analysers);
    if (!r) return;
    const bool hop = l.kind == FX_LAUNCH_HOP || l.kind == FX_LAUNCH_HOP_PAIR;
    if (l.kind != FX_LAUNCH_EPILOGUE) {
        r->T = l.fp.T; r->direct_state = l.fp.direct_state; r->block_mode = l.fp.block_mode;
        if (!hop) { r->num_chunks = l.fp.num_chunks; r->ch_per_wg = l.fp.ch_per_wg; r->waves_per_ch = l.fp.waves_per_ch; }
        else r->hop_pairs = l.kind == FX_LAUNCH_HOP_PAIR ? 1 : 0;
    }
    if (l.kind != FX_LAUNCH_FRAME && l.kind != FX_LAUNCH_PAIR) { r->ep_T = l.ep.T; r->out_stride = l.ep.out_stride; }
    if (l.kind == FX_LAUNCH_EPILOGUE) r->ep_form = fxk::epilogue_form(l.ep);
}

// Enqueue one planned launch on the context's stream, and record it.  `sig`: the ring's hop kernel signals its slot.
hipError_t enqueue(fx_context* c, const Launch& l, const fxk::HopSignal& sig)
{
    note_planned(c, l);
    switch (l.kind) {
    case FX_LAUNCH_FRAME:      return fxk::launch_frame_kernel(c->N, l.fp, l.analysers, c->stream);
    case FX_LAUNCH_PAIR:       return fxk::launch_pair_kernel(c->N, l.fp, c->stream);
    case FX_LAUNCH_FRAME_TAIL: return fxk::launch_frame_tail_kernel(c->N, l.fp, l.ep, c->stream);
    case FX_LAUNCH_EPILOGUE:   return fxk::launch_epilogue_kernels(l.ep, c->stream);
    case FX_LAUNCH_HOP:
    case FX_LAUNCH_HOP_PAIR:   return fxk::launch_hop_kernel(c->N, l.fp, l.ep, sig, c->stream, l.kind == FX_LAUNCH_HOP_PAIR);
    default:                   return hipErrorInvalidValue;       // (a kind plan_call does not make)
    }
}

void fill_dyn(const fx_context* c, fxk::DynParams* d)
{
    d->nyquist = c->sample_rate / 2.0;
    d->frames_before = c->frames_seen;
    d->hist_base = (int) (c->frames_seen % fxk::HLEN);
    d->onset_reset_frame = c->onset_reset_frame;
    d->gain = c->gain;
    d->onset_multiplier = c->onset_multiplier;
    d->onset_window = c->onset_window;
    d->onset_type = c->onset_type;
}

// once a part's launches are enqueued: the state they leave
void advance(fx_context* c, int T)
{
    c->cur ^= 1;
    c->frames_seen += T;
}

// Whether this context's one-hop calls can take blocks directly: windows from 1024 points, both analysers, the default kernel family
// (the pair family and the single-analyser forms read hops: those calls go through fx_reblock_kernel).
bool blocks_feed_kernels(const fx_context* c)
{
    return c->N >= 1024 && !(c->flags & (FX_SPECTRAL_ONLY | FX_HARMONIC_ONLY)) && !uses_pairs(c, c->tuning.waves_per_frame) &&
           !(c->test_hooks & FX_HOOK_NO_BLOCK_FEED);
}

// Bytes of FrameParams::flux_park a call of T frames per channel may need: the 1024-point batch kernel with both analysers keeps the flux
// state by runs (csrc/fx_flux_runs.h), and a wavefront parks its run's first frame there -- a row of N/2 floats per wavefront of every
// channel, at most as many wavefronts as the call has frames.  0: no kernel of this call parks (whoever plans such a call grows
// fx_context::d_flux_park to this first; plan_call() itself allocates nothing).
size_t flux_park_need(const fx_context* c, int T)
{
    if (c->N != 1024 || (c->flags & (FX_SPECTRAL_ONLY | FX_HARMONIC_ONLY)) || T < 2 || uses_pairs(c, c->tuning.waves_per_frame)) return 0;
    const int kcap = fxk::frame_kernel_max_waves(c->N);
    return sizeof(float) * (size_t) c->C * (size_t) (T < kcap ? T : kcap) * (size_t) (c->N / 2);
}

// in_kind / out_kind: where the caller's samples and result buffers live (fx_push_samples hands over hops it has assembled in device
// memory with results that may go to the host)
fx_status fx_run(fx_context* c, const void* in, int T, int sample_format, int in_kind, int out_kind, int hop_mode,
                 float* out_raw, float* out_smoothed, const BlockFeed* blocks, bool taps, bool events)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (T < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative frame count");
    if (T == 0) return FX_OK;
    if (!in) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null input buffer");
    { const fx_status cs = fx_check_call(sample_format, in_kind, out_kind); if (cs != FX_OK) return cs; }
    HIP_TRY(hipSetDevice(c->device));
    { const fx_status es = fx_check_device_error(c); if (es != FX_OK) return es; }     // sticky: an earlier call's hand-over failed

    const size_t esz = sample_size(sample_format);
    const size_t per_frame = hop_mode ? (size_t) c->N / 2 : (size_t) c->N;
    const size_t in_bytes = (size_t) c->C * T * per_frame * esz;
    const size_t out_elems = (size_t) c->C * T * FX_NUM_FEATURES;

    fx_status st;
    const size_t raw_bytes = out_elems * sizeof(float);
    if ((st = fx_grow(&c->d_raw, &c->raw_cap, raw_bytes)) != FX_OK) return st;
    if ((st = fx_grow(&c->d_part, &c->part_cap, (size_t) c->C * T * sizeof(fxk::FramePart))) != FX_OK) return st;
    if ((st = fx_grow(&c->d_flux_park, &c->flux_park_cap, flux_park_need(c, T))) != FX_OK) return st;

    const void* d_in = in;
    float* d_or = out_raw;
    float* d_os = out_smoothed;
    // the onset event list (fx_enable_onset_events) reads the raw vectors where the tails write them: with the list enabled they
    // always get a device out_raw, the context's staging where the caller gave none (copied back only if the caller asked)
    const bool list_events = events && c->events_launch;
    if (out_kind == FX_MEM_HOST || (list_events && !out_raw)) {
        if (out_raw || out_smoothed || list_events) {
            // one allocation, two halves
            if ((st = fx_grow(&c->d_out_raw, &c->out_cap, 2 * raw_bytes)) != FX_OK) return st;
            c->d_out_sm = c->d_out_raw + out_elems;
        }
        d_or = out_raw || list_events ? c->d_out_raw : nullptr;
        if (out_kind == FX_MEM_HOST) d_os = out_smoothed ? c->d_out_sm : nullptr;
    }
    if (in_kind == FX_MEM_HOST) {
        if ((st = fx_grow(&c->d_in, &c->in_cap, in_bytes)) != FX_OK) return st;
        HIP_TRY(hipMemcpyAsync(c->d_in, in, in_bytes, hipMemcpyHostToDevice, c->stream));
        d_in = c->d_in;
    } else {
        if (reinterpret_cast<uintptr_t>(in) % (blocks ? 4 : 16) != 0)
            return fx_fail(FX_ERR_INVALID_ARGUMENT, "device input must be %d-byte aligned", blocks ? 4 : 16);
    }
    if (blocks && (T < 1 || T > 4096 || !hop_mode || in_kind != FX_MEM_DEVICE)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "a block feed is 1 .. 4096 hops per channel from device memory");
    Plan plan;
    if ((st = plan_call(c, d_in, T, sample_format, hop_mode, d_or, d_os, blocks, nullptr, c->d_part, c->d_raw, ROUTE_AUTO, &plan)) != FX_OK) return st;
    const fx_tap_source src = {d_in, sample_format, hop_mode, blocks ? blocks->in_row_bytes : (long long) (T * per_frame * esz),
                               blocks ? blocks->carry_in : nullptr, blocks ? blocks->carry_bytes : 0, blocks ? blocks->carry_row_bytes : 0};
    // armed taps (fx_request_taps): their launch reads this call's first frame before any launch of the call changes the context's state
    if (taps && c->taps_armed && c->taps_launch && (st = c->taps_launch(c, src)) != FX_OK) return st;

    // timed: e0 before the first launch, e1 after the last launch that analyses frames, e2 after the last launch (frame-kernel time is
    // only split out of calls of one part)
    hipEvent_t e0 = c->ev[0], e1 = c->ev[1], e2 = c->ev[2];
    bool last_valid = plan.timed;
    if (c->profiling && c->prof_used + 3 <= 3 * 4096) {
        while (c->prof_events.size() < c->prof_used + 3) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            c->prof_events.push_back(e);
        }
        e0 = c->prof_events[c->prof_used]; e1 = c->prof_events[c->prof_used + 1]; e2 = c->prof_events[c->prof_used + 2];
        c->prof_used += 3;
        last_valid = false;
    }
    auto mark = [&](hipEvent_t e) { return plan.timed ? hipEventRecord(e, c->stream) : hipSuccess; };
    int last_frames = plan.n - 1;
    while (plan.launch[last_frames].kind == FX_LAUNCH_EPILOGUE) last_frames--;
    HIP_TRY(mark(e0));
    for (int i = 0; i < plan.n; i++) {
        HIP_TRY(enqueue(c, plan.launch[i]));
        if (i == last_frames) HIP_TRY(mark(e1));
        // a part's launches are enqueued: the context holds the state they leave, whatever happens to the rest of the call
        if (i + 1 == plan.n || plan.launch[i + 1].kind != FX_LAUNCH_EPILOGUE) advance(c, T / plan.parts);
    }
    HIP_TRY(mark(e2));
    c->ev_valid = last_valid;
    // every frame's raw vector is on its way to d_or: the list's one launch (a failure leaves the stream to fx_reset_state)
    if (list_events && (st = c->events_launch(c, d_or, T, c->frames_seen - T)) != FX_OK) return st;
    // the audio display (fx_enable_display) reads the call's samples where the launches above read them: its one launch (a block
    // feed's launches wrote the OTHER carry buffer; the pending rows they read stand until the next call)
    if (events && c->display_launch && (st = c->display_launch(c, src, T)) != FX_OK) return st;

    if (out_kind == FX_MEM_HOST) {
        if (out_raw) HIP_TRY(hipMemcpyAsync(out_raw, c->d_out_raw, raw_bytes, hipMemcpyDeviceToHost, c->stream));
        if (out_smoothed) HIP_TRY(hipMemcpyAsync(out_smoothed, c->d_out_sm, raw_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fx_check_device_error(c);
    }
    return FX_OK;
}
