// fx_events.hip -- the onset event list: every track's onset callback as one list made on the GPU (include/fx.h,
// fx_enable_onset_events / fx_get_onset_events).
//
// ref RealTimeAnalyser.h:228-229, :256: RealTimeSpectralAnalyser::run calls onsetDetectedCallback() after any frame whose onset slot is
// above zero, and AnalyserTrackController.h:80-84 binds that callback per track.  getValue(enOnset) has history length 1, so the
// condition is the raw slot of the frame just analysed: raw[FX_ONSET] == 1.0f.  Here an enabled context appends one record per
// (track, frame) with that value to a list in device memory, ordered by (call, frame of the call, channel), and the host drains the list
// when it likes.  A record's `frame` is the track's own index: the call's stream index less the track's first_frame (fx_tracks.hip).
//
// One launch of fx_onset_events_kernel per analysis call, after the call's last analysis launch (the tails have then written every
// frame's raw vector to the call's device out_raw, [C][T][12]).  A wavefront reads the onset slot of 64 consecutive channels of one
// frame -- lane = channel -- and __ballot turns them into one 64-bit mask per (frame, channel group); the masks, in list order
// (frame-major), go to a scratch table.  The workgroup that arrives last (one counter, one agent-scope add per workgroup) then
// places the events: __popcll of a mask is its group's count, an exclusive scan over the groups in list order gives every group its
// offset behind the events already stored, and the set bits of a mask, lowest first, are its events in channel order.  The order is
// therefore a function of the flags alone, never of which workgroup ran when.  The stored / dropped counts live in device memory and
// only this kernel's last workgroup (and a drain, which synchronises) writes them: no host wait per call.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: fx_enable_onset_events installs the context's three hooks (fx_context.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"

static_assert(sizeof(fx_onset_event) == 16, "a record is one 16-byte store");

namespace fxk {
namespace {

constexpr int EV_THREADS = 256, EV_WAVES = EV_THREADS / 64;
constexpr int EV_GROUPS_PER_WAVE = 2;                           // two flag loads in flight per lane
constexpr int EV_GROUPS_PER_WG = EV_WAVES * EV_GROUPS_PER_WAVE;

// Device state of the list.  count / dropped are written by the kernel's last workgroup and by a drain; arrivals is zero between launches.
struct EventsState {
    unsigned long long dropped;     // events lost to overflow since the last drain
    unsigned           count;       // events stored: ring[head .. head + count) modulo capacity
    unsigned           arrivals;    // workgroups of the running launch that have published their masks
};
static_assert(sizeof(EventsState) == 16, "cleared and copied as one 16-byte block");

struct EventsParams {
    const float*        raw;        // [C][T][12] of the call: slot FX_ONSET of every row is read
    unsigned long long* masks;      // [T][G]: bit i of masks[t * G + g] = channel 64 g + i has an onset in frame t
    fx_onset_event*     ring;       // [capacity]
    EventsState*        state;
    long long           frame0;     // stream index of the call's first frame
    const ChannelSettings* chan;    // per-track rows or null: a track's `frame` counts from its own first_frame (fx_reset_channels)
    int                 C, T, G;    // G = ceil(C / 64)
    int                 capacity, head;     // head < capacity: only a drain moves it, and a drain synchronises
};

typedef __attribute__((address_space(1))) unsigned long long* GlobalU64;
typedef __attribute__((address_space(1))) unsigned* GlobalU32;

// exclusive scan of one value per thread over the workgroup (scratch: EV_WAVES + 1 words); *total = the sum
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* scratch, unsigned* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    __syncthreads();                            // (scratch may still be read by the previous round)
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < EV_WAVES; w++) {
        const unsigned s = scratch[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return before + incl - v;
}

} // namespace

// (named in fxk itself, like the analysis kernels: tools/kernel_resources.py tabulates it for DESIGN.md 3.8)
__global__ void __launch_bounds__(EV_THREADS) fx_onset_events_kernel(const EventsParams p)
{
    __shared__ unsigned scan_scratch[EV_WAVES];
    __shared__ unsigned last_flag;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long groups = (long long) p.T * p.G;

    // ---- every workgroup: the masks of its groups ----
    {
        const long long g0 = ((long long) blockIdx.x * EV_WAVES + wave) * EV_GROUPS_PER_WAVE;
        float flag[EV_GROUPS_PER_WAVE];
#pragma unroll
        for (int k = 0; k < EV_GROUPS_PER_WAVE; k++) {
            const long long g = g0 + k;
            flag[k] = 0.0f;
            if (g < groups) {
                const int t = (int) (g / p.G), c = (int) (g - (long long) t * p.G) * 64 + lane;
                if (c < p.C) flag[k] = p.raw[((long long) c * p.T + t) * FX_NUM_FEATURES + FX_ONSET];
            }
        }
#pragma unroll
        for (int k = 0; k < EV_GROUPS_PER_WAVE; k++) {
            const unsigned long long m = __ballot(flag[k] == 1.0f);
            // (one lane, one 8-byte write-through store: what the last workgroup reads back below)
            if (lane == 0 && g0 + k < groups) __hip_atomic_store((GlobalU64) (p.masks + g0 + k), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // ---- which workgroup is last: every storing wave drains its stores, then one lane counts the workgroup in ----
    if (gridDim.x > 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned n = __hip_atomic_fetch_add((GlobalU32) &p.state->arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last_flag = n + 1 == gridDim.x;
            if (n + 1 == gridDim.x) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if (!last_flag) return;
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ---- the last workgroup: counts, scan, records ----
    const unsigned base = p.state->count;                  // (left by the launch or the drain before this one)
    unsigned long long running = 0;                         // events of this call in the groups before the current round
    for (long long r0 = 0; r0 < groups; r0 += EV_THREADS) {
        const long long g = r0 + threadIdx.x;
        unsigned long long m = 0;
        if (g < groups) m = __hip_atomic_load((GlobalU64) (p.masks + g), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned total = 0;
        const unsigned before = block_exclusive_scan((unsigned) __popcll(m), scan_scratch, &total);
        if (m) {
            const int t = (int) (g / p.G), c0 = (int) (g - (long long) t * p.G) * 64;
            unsigned long long pos = (unsigned long long) base + running + before;
            while (m && pos < (unsigned long long) p.capacity) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                long long at = (long long) p.head + (long long) pos;
                if (at >= p.capacity) at -= p.capacity;
                const long long frame = p.frame0 + t - (p.chan ? p.chan[c0 + bit].first_frame : 0);
                uint4 rec;
                rec.x = (unsigned) ((unsigned long long) frame & 0xffffffffull);
                rec.y = (unsigned) ((unsigned long long) frame >> 32);
                rec.z = (unsigned) (c0 + bit);
                rec.w = (unsigned) t;
                *reinterpret_cast<uint4*>(p.ring + at) = rec;
                pos++;
            }
        }
        running += total;
    }
    if (threadIdx.x == 0) {
        const unsigned long long room = (unsigned long long) p.capacity - base;
        const unsigned long long kept = running < room ? running : room;
        p.state->count = base + (unsigned) kept;
        p.state->dropped += running - kept;
        if (gridDim.x > 1) __hip_atomic_store((GlobalU32) &p.state->arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace fxk

struct fx_events {
    fx_onset_event*     d_ring = nullptr;
    fxk::EventsState*   d_state = nullptr;
    unsigned long long* d_masks = nullptr;
    size_t              masks_cap = 0;      // bytes
    int                 capacity = 0;
    int                 head = 0;           // the oldest stored event's place in the ring
};

namespace {

constexpr int MAX_CAPACITY = 1 << 26;

void events_release(fx_context* c)
{
    fx_events* e = c->events;
    if (!e) return;
    fx_free_device({e->d_ring, e->d_state, e->d_masks});
    delete e;
    c->events = nullptr;
}

// fx_reset_state (the stream is idle): an empty list, nothing dropped; capacity and memory stay
fx_status events_reset(fx_context* c)
{
    fx_events* e = c->events;
    if (!e) return FX_OK;
    e->head = 0;
    HIP_TRY(hipMemsetAsync(e->d_state, 0, sizeof(fxk::EventsState), c->stream));
    return FX_OK;
}

// after the last analysis launch of a call of T frames per channel whose raw vectors are in d_raw [C][T][12] (device memory);
// frame0: the stream index of the call's first frame
fx_status events_launch(fx_context* c, const float* d_raw, int T, long long frame0)
{
    fx_events* e = c->events;
    if (!e || T <= 0) return FX_OK;
    const int G = (c->C + 63) / 64;
    const long long groups = (long long) T * G;
    const long long wgs = (groups + fxk::EV_GROUPS_PER_WG - 1) / fxk::EV_GROUPS_PER_WG;
    if (wgs > 0x7fffffffll) return fx_fail(FX_ERR_INVALID_ARGUMENT, "call of %d frames x %d channels is too long for the onset event list", T, c->C);
    const size_t need = (size_t) groups * sizeof(unsigned long long);
    // (growing frees the old table: hipFree waits for the launches that read it)
    { const fx_status st = fx_grow(&e->d_masks, &e->masks_cap, need); if (st != FX_OK) return st; }
    fxk::EventsParams p;
    p.raw = d_raw;
    p.masks = e->d_masks;
    p.ring = e->d_ring;
    p.state = e->d_state;
    p.frame0 = frame0;
    p.chan = c->d_chan;
    p.C = c->C;
    p.T = T;
    p.G = G;
    p.capacity = e->capacity;
    p.head = e->head;
    // ONE launch (the scan runs in its last workgroup)
    if (fx_launch_record* r = note_launch(c, FX_LAUNCH_ONSET_EVENTS, 0)) r->T = T;
    hipLaunchKernelGGL(fxk::fx_onset_events_kernel, dim3((unsigned) wgs), dim3(fxk::EV_THREADS), 0, c->stream, p);
    HIP_TRY(hipGetLastError());
    return FX_OK;
}

} // namespace

extern "C" {

fx_status fx_enable_onset_events(fx_context* c, int capacity)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (capacity < 0 || capacity > MAX_CAPACITY)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "capacity %d: the onset event list holds 1 .. %d events (0 disables it)", capacity, MAX_CAPACITY);
    if (capacity == 0 && !c->events) return FX_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));        // launches in flight write the list that is about to go
    events_release(c);
    c->events_launch = nullptr;
    c->events_reset = nullptr;
    c->events_release = nullptr;
    if (capacity == 0) return FX_OK;
    fx_events* e = new (std::nothrow) fx_events();
    if (!e) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    c->events = e;                                   // (from here a failure leaves what was allocated to events_release)
    c->events_release = events_release;
    fx_status st = FX_OK;
    auto build = [&]() -> fx_status {
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, (size_t) capacity * sizeof(fx_onset_event)));
        e->d_ring = static_cast<fx_onset_event*>(q);
        q = nullptr;
        HIP_TRY(hipMalloc(&q, sizeof(fxk::EventsState)));
        e->d_state = static_cast<fxk::EventsState*>(q);
        HIP_TRY(hipMemsetAsync(e->d_state, 0, sizeof(fxk::EventsState), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return FX_OK;
    };
    if ((st = build()) != FX_OK) {
        events_release(c);
        c->events_release = nullptr;
        return st;
    }
    e->capacity = capacity;
    c->events_launch = events_launch;
    c->events_reset = events_reset;
    return FX_OK;
}

fx_status fx_get_onset_events(fx_context* c, fx_onset_event* out, int cap, int* count, long long* dropped)
{
    if (count) *count = 0;
    if (dropped) *dropped = 0;
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    if (cap < 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "negative cap");
    if (!out && cap > 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null out with cap %d", cap);
    fx_events* e = c->events;
    if (!e) return fx_fail(FX_ERR_INVALID_ARGUMENT, "onset events are not enabled on this context (fx_enable_onset_events)");
    HIP_TRY(hipSetDevice(c->device));
    fxk::EventsState s;
    HIP_TRY(hipMemcpyAsync(&s, e->d_state, sizeof s, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    { const fx_status es = fx_check_device_error(c); if (es != FX_OK) return es; }
    const int stored = (int) s.count;
    if (!out) {                                     // cap == 0: how many are stored; nothing is removed, nothing cleared
        if (count) *count = stored;
        if (dropped) *dropped = (long long) s.dropped;
        return FX_OK;
    }
    const int n = stored < cap ? stored : cap;
    const int first = n < e->capacity - e->head ? n : e->capacity - e->head;       // the ring wraps at most once
    if (first > 0) HIP_TRY(hipMemcpyAsync(out, e->d_ring + e->head, (size_t) first * sizeof(fx_onset_event), hipMemcpyDeviceToHost, c->stream));
    if (n > first) HIP_TRY(hipMemcpyAsync(out + first, e->d_ring, (size_t) (n - first) * sizeof(fx_onset_event), hipMemcpyDeviceToHost, c->stream));
    // the list keeps the rest; the overflow count starts again
    const fxk::EventsState next = {0ull, (unsigned) (stored - n), 0u};
    HIP_TRY(hipMemcpyAsync(e->d_state, &next, sizeof next, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    e->head = (int) (((long long) e->head + n) % e->capacity);
    if (count) *count = n;
    if (dropped) *dropped = (long long) s.dropped;
    return FX_OK;
}

} // extern "C"
