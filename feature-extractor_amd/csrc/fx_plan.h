// fx_plan.h -- the call planner (fx_plan.cpp) as the entry points (fx_capi.cpp) and the streaming ring (fx_stream.cpp) use it.  Internal.
#ifndef FX_PLAN_H
#define FX_PLAN_H

#include "fx_context.h"

// One launch of an analysis call: which launcher (FX_LAUNCH_*: frame, pair, frame_tail, hop, hop_pair, epilogue) and its arguments.
struct Launch {
    int kind = 0;
    fxk::FrameParams    fp;
    fxk::EpilogueParams ep;
    int analysers = 3;
};
// Everything one analysis call launches, in order, and whether fx_last_kernel_ms times it.  Built whole before anything is enqueued.
struct Plan {
    Launch launch[4];
    int n = 0;
    int parts = 1;          // steps of the context's state: a call cut into one-frame launches takes one per frame, others one
    bool timed = false;
};
// route: the library picks the kernels (fx_run()), or a ring step fixes them: the one-launch hop kernel, or the captured step (frame or
// pair kernel + epilogue, never cut in time or in frames: a graph replays what it was captured with)
enum Route { ROUTE_AUTO, ROUTE_RING_HOP, ROUTE_RING_CAPTURED };

// fx_push_samples' call that completes exactly one hop, without the re-blocking pass: `in` of fx_run() is then the device BLOCK of every
// channel (rows of in_row_bytes) and the one-frame kernels read the hop from [pending samples | block] themselves and write the new
// pending samples (FrameParams::block_mode, csrc/fx_blocks.hip.h)
struct BlockFeed {
    const unsigned char* carry_in;
    unsigned char*       carry_out;
    int                  carry_bytes, carry_row_bytes;
    long long            in_row_bytes;
};

// each entry point that launches starts the launch record (fx_context.h, note_launch) anew
inline void begin_launches(fx_context* c) { if (c) c->num_launches = 0; }

// fx_plan.cpp, where each is described
bool uses_pairs(const fx_context* c, int waves_per_frame);
bool blocks_feed_kernels(const fx_context* c);
size_t flux_park_need(const fx_context* c, int T);
fx_status plan_call(const fx_context* c, const void* d_in, int T, int sample_format, int hop_mode, float* d_or, float* d_os,
                    const BlockFeed* blocks, const fxk::DynParams* dyn, fxk::FramePart* part, float* raw, Route route, Plan* plan);
void note_planned(fx_context* c, const Launch& l);
hipError_t enqueue(fx_context* c, const Launch& l, const fxk::HopSignal& sig = {});
void fill_dyn(const fx_context* c, fxk::DynParams* d);
void advance(fx_context* c, int T);
fx_status fx_run(fx_context* c, const void* in, int T, int sample_format, int in_kind, int out_kind, int hop_mode,
                 float* out_raw, float* out_smoothed, const BlockFeed* blocks = nullptr, bool taps = false, bool events = false);

// fx_push_samples (fx_capi.cpp); `taps`: whether the call serves armed taps (the ring's submissions do not, include/fx.h)
fx_status push_samples(fx_context* c, const void* samples, int num_samples, int sample_format, int mem_kind,
                       float* out_raw, float* out_smoothed, int* frames_out, bool taps);

#endif
