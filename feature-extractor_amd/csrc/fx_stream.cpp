// fx_stream.cpp -- streaming ingest (fx_stream_*, include/fx.h): pinned host ring, H2D on a side stream, analysis behind an event.
// Uses the planner (fx_plan.h) and the context (fx_context.h); nothing in fx_capi.cpp or fx_plan.cpp refers to this unit.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "fx_plan.h"

// The producer's copy into a pinned slot, by several host threads (fx_stream_push): a caller whose audio sits in ordinary memory
// has to move every sample once more before PCIe sees it, and one memcpy thread moves ~12 GB/s where the link takes 55.  A small
// persistent pool: workers sleep on a generation counter, each copies its share of the bytes, the last one wakes the caller.
// A slot is written once by the producer and read next by the DMA engine, never again by the core that wrote it: non-temporal stores
// skip the read-for-ownership of every destination line (a third of the copy's memory traffic; glibc's memcpy only switches to them
// far above the ~8 MB a fill thread copies).  x86-64 only; elsewhere, and for the head / tail of a piece, plain memcpy.
#if defined(__x86_64__)
#include <emmintrin.h>
static void copy_streaming(unsigned char* d, const unsigned char* s, size_t n)
{
    size_t head = (64 - (reinterpret_cast<uintptr_t>(d) & 63)) & 63;
    if (head > n) head = n;
    memcpy(d, s, head); d += head; s += head; n -= head;
    for (size_t blocks = n / 64; blocks > 0; blocks--) {
        const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s)), b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 16)),
                      c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 32)), e = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + 48));
        _mm_stream_si128(reinterpret_cast<__m128i*>(d), a); _mm_stream_si128(reinterpret_cast<__m128i*>(d + 16), b);
        _mm_stream_si128(reinterpret_cast<__m128i*>(d + 32), c); _mm_stream_si128(reinterpret_cast<__m128i*>(d + 48), e);
        s += 64; d += 64;
    }
    _mm_sfence();
    memcpy(d, s, n & 63);
}
#else
static void copy_streaming(unsigned char* d, const unsigned char* s, size_t n) { memcpy(d, s, n); }
#endif

class FillPool {
public:
    ~FillPool() { resize(0); }
    bool streaming = true;          // fx_tuning::stream_fill_streaming (taken by fx_stream_create)
    void copy(void* dst, const void* src, size_t bytes, int threads)
    {
        if (threads <= 1 || bytes < (1u << 20)) { memcpy(dst, src, bytes); return; }
        if ((int) workers_.size() != threads - 1) resize(threads - 1);
        const size_t piece = ((bytes + (size_t) threads - 1) / (size_t) threads + 4095) & ~(size_t) 4095;
        {
            std::lock_guard<std::mutex> g(m_);
            dst_ = static_cast<unsigned char*>(dst); src_ = static_cast<const unsigned char*>(src); bytes_ = bytes; piece_ = piece;
            pending_ = (int) workers_.size();
            generation_++;
        }
        wake_.notify_all();
        slice(threads - 1);                                   // the caller copies the last piece itself
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [&] { return pending_ == 0; });
    }
private:
    void slice(int k)
    {
        const size_t at = piece_ * (size_t) k;
        if (at >= bytes_) return;
        const size_t n = bytes_ - at < piece_ ? bytes_ - at : piece_;
        if (streaming) copy_streaming(dst_ + at, src_ + at, n);
        else memcpy(dst_ + at, src_ + at, n);
    }
    void resize(int n)
    {
        {
            std::lock_guard<std::mutex> g(m_);
            quit_ = true;
        }
        wake_.notify_all();
        for (auto& t : workers_) t.join();
        workers_.clear();
        quit_ = false;
        const unsigned long long born = generation_;           // (read here, by the caller: a worker that starts late must not miss the first job)
        for (int k = 0; k < n; k++)
            workers_.emplace_back([this, k, born] {
                unsigned long long seen = born;
                for (;;) {
                    std::unique_lock<std::mutex> g(m_);
                    wake_.wait(g, [&] { return quit_ || generation_ != seen; });
                    if (quit_) return;
                    seen = generation_;
                    g.unlock();
                    slice(k);
                    g.lock();
                    if (--pending_ == 0) done_.notify_one();
                }
            });
    }
    std::mutex m_;
    std::condition_variable wake_, done_;
    std::vector<std::thread> workers_;
    unsigned char* dst_ = nullptr; const unsigned char* src_ = nullptr;
    size_t bytes_ = 0, piece_ = 0;
    unsigned long long generation_ = 0;
    int pending_ = 0;
    bool quit_ = false;
};

struct fx_stream {
    fx_context* ctx = nullptr;
    FillPool fill;
    int hops = 0, slots = 0, fmt = FX_SAMPLE_F32;
    size_t in_bytes = 0, out_bytes = 0;
    // Large batches: three queues, so that PCIe runs in both directions while the kernels run -- `copy` carries batch k+1's samples
    // to the device, the context's stream analyses batch k, `back` returns batch k-1's vectors.  (Until round 4 the results went
    // back on `copy`: the next batch's samples then queued behind a copy that waits for the analysis before it, and nothing overlapped.)
    hipStream_t copy = nullptr, back = nullptr;
    // Small batches are launch-bound (one 4096-pt hop: four kernels, three copies and five events cost ~150 us of host
    // and dispatch time for ~40 us of GPU work): there the whole step -- input copy, per-call scalars, the four
    // kernels, result copies -- is captured once per ring slot and buffer parity into a hipGraph and replayed.
    bool use_graph = false;
    // One hop per call (BASELINE configs[4]) is all latency: there the whole step is ONE launch of fx_hop_kernel
    // (csrc/fx_hop_kernel.hip.h: three wavefronts per channel + the tail), which reads the hop from the pinned slot,
    // writes the 12-float vectors back to it and then stores the call's sequence number to the slot's flag; collect
    // polls that flag.  No graph, no event, no second kernel.
    bool use_hop_kernel = false;
    bool zero_copy = false;               // captured step: kernels read / write the pinned slot directly (a few KB per step)
    unsigned* d_arrivals = nullptr;       // workgroups of the running hop kernel that have finished (zero between calls)
    void*     d_stage = nullptr;          // [C][N/2] samples: the hop kernel's device copy of the hop it is analysing
    unsigned  next_seq = 0;
    fxk::FramePart* g_part = nullptr;     // scratch the captured kernels own (a graph keeps its addresses)
    float*          g_raw = nullptr;
    struct Slot {
        void*  h_in = nullptr;  void* d_in = nullptr;
        float* d_raw = nullptr; float* d_sm = nullptr;
        float* h_raw = nullptr; float* h_sm = nullptr;
        hipEvent_t copied = nullptr, done = nullptr, out = nullptr;
        unsigned* h_flag = nullptr;       // pinned, coherent: sequence number of the last hop-kernel call that completed in this slot
        const void* dev_in = nullptr; float* dev_raw = nullptr; float* dev_sm = nullptr; unsigned* dev_flag = nullptr;   // device views of the pinned buffers
        unsigned  seq = 0;                // sequence number of the call in flight in this slot
        int       frames = 0;             // analysis frames per channel of the batch in flight in this slot (hops_per_batch, or what fx_stream_submit_samples made of its block)
        bool      by_event = false;       // the batch in flight completes with the `out` event (every path but the one-launch hop kernel, which raises a flag)
        fxk::DynParams* h_dyn = nullptr;  // pinned: what changes from call to call
        fxk::DynParams* d_dyn = nullptr;
        hipGraphExec_t  exec[2] = {nullptr, nullptr};     // per parity of the context's ping-pong buffers
        Plan      captured[2];            // what each of them launches (noted in the launch record at every replay)
    };
    std::vector<Slot> ring;
    int head = 0;        // next slot to acquire
    int tail = 0;        // oldest slot in flight
    int in_flight = 0;
    bool acquired = false;
    int since_release = 0;   // batches of the three-queue path collected since the streams were last synchronised (fx_stream_collect_samples)
};

// A submit holds the acquired slot: every return hands it back (the caller may fill and submit it again: the ring never wedges on "a
// slot is already acquired").  A failed one first waits for the streams it has given work that reads the slot.
struct SlotGuard {
    fx_stream* s;
    hipStream_t readers[2] = {nullptr, nullptr};
    bool ok = false;
    ~SlotGuard()
    {
        if (!ok) for (hipStream_t q : readers) if (q) (void) hipStreamSynchronize(q);
        s->acquired = false;
    }
};

// A submitted slot joins the batches in flight: what collect needs to know of it, and the ring moves on.
static void commit_slot(fx_stream* s, fx_stream::Slot& sl, int frames, bool by_event)
{
    sl.frames = frames; sl.by_event = by_event;
    s->head = (s->head + 1) % s->slots;
    s->in_flight++;
}

// The device views of a slot's pinned buffers: the hop, both result tables, and `pinned` -- the captured step's scalars (h_dyn) or the
// hop kernel's flag (h_flag), whose view is stored last: the hop-kernel path takes a slot's views once and knows by dev_flag that it has.
template <typename T> static fx_status slot_views(const fx_stream::Slot& sl, T* pinned, const void** in, float** raw, float** sm, T** last)
{
    void* q = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&q, sl.h_in, 0));  *in = q;
    HIP_TRY(hipHostGetDevicePointer(&q, sl.h_raw, 0)); *raw = static_cast<float*>(q);
    HIP_TRY(hipHostGetDevicePointer(&q, sl.h_sm, 0));  *sm = static_cast<float*>(q);
    HIP_TRY(hipHostGetDevicePointer(&q, pinned, 0));   *last = static_cast<T*>(q);
    return FX_OK;
}

// The large-batch form of a submit: samples in on `copy`, analysis on the context's stream behind an event, vectors back on `back`.
// num_samples < 0: the slot holds hops_per_batch whole hops per channel; else a block of num_samples samples per channel
// ([C][num_samples], rows back to back), which fx_push_samples cuts into hops with the context's pending samples.
// A failure before the analysis is enqueued loses nothing; after it the context has moved on and the batch's results are lost with the
// error.  Either way the streams named in g.readers are waited for before the slot is handed back.
static fx_status submit_large(fx_stream* s, SlotGuard& g, fx_stream::Slot& sl, size_t in_bytes, int num_samples)
{
    fx_context* c = s->ctx;
    if (in_bytes) HIP_TRY(hipMemcpyAsync(sl.d_in, sl.h_in, in_bytes, hipMemcpyHostToDevice, s->copy));
    g.readers[0] = s->copy;
    HIP_TRY(hipEventRecord(sl.copied, s->copy));
    HIP_TRY(hipStreamWaitEvent(c->stream, sl.copied, 0));
    // fx_push_samples may launch its re-blocking kernel on the context's stream and then fail: that kernel reads the slot too.  The ring
    // stays usable; the STREAM of a samples submit does not: the pending samples have moved on without the hops this block completed
    // (fx_push_samples' contract) -- fx_reset_state, not a re-submit of the same block.
    if (num_samples >= 0) g.readers[1] = c->stream;
    int frames = s->hops;
    const fx_status st = num_samples < 0 ? fx_run(c, sl.d_in, s->hops, s->fmt, FX_MEM_DEVICE, FX_MEM_DEVICE, 1, sl.d_raw, sl.d_sm)
                                         : push_samples(c, sl.d_in, num_samples, s->fmt, FX_MEM_DEVICE, sl.d_raw, sl.d_sm, &frames, false);
    if (st != FX_OK) return st;
    const size_t out_bytes = (size_t) c->C * (size_t) frames * FX_NUM_FEATURES * sizeof(float);
    // from here on the analysis is enqueued behind the copy: the context's stream has all the work that reads the slot, then `back`
    g.readers[0] = c->stream; g.readers[1] = nullptr;
    HIP_TRY(hipEventRecord(sl.done, c->stream));
    HIP_TRY(hipStreamWaitEvent(s->back, sl.done, 0));
    if (out_bytes) HIP_TRY(hipMemcpyAsync(sl.h_raw, sl.d_raw, out_bytes, hipMemcpyDeviceToHost, s->back));
    g.readers[1] = s->back;
    if (out_bytes) HIP_TRY(hipMemcpyAsync(sl.h_sm, sl.d_sm, out_bytes, hipMemcpyDeviceToHost, s->back));
    HIP_TRY(hipEventRecord(sl.out, s->back));
    commit_slot(s, sl, frames, true);
    g.ok = true;
    return FX_OK;
}

extern "C" {

fx_status fx_stream_destroy(fx_stream* s)
{
    if (!s) return FX_OK;
    if (s->ctx) (void) hipSetDevice(s->ctx->device);
    if (s->copy) (void) hipStreamSynchronize(s->copy);
    if (s->ctx && s->ctx->stream) (void) hipStreamSynchronize(s->ctx->stream);
    if (s->back) (void) hipStreamSynchronize(s->back);
    for (auto& sl : s->ring) {
        if (sl.h_in) (void) hipHostFree(sl.h_in);
        if (sl.h_raw) (void) hipHostFree(sl.h_raw);
        if (sl.h_sm) (void) hipHostFree(sl.h_sm);
        if (sl.d_in) (void) hipFree(sl.d_in);
        if (sl.d_raw) (void) hipFree(sl.d_raw);
        if (sl.d_sm) (void) hipFree(sl.d_sm);
        for (int q = 0; q < 2; q++) if (sl.exec[q]) (void) hipGraphExecDestroy(sl.exec[q]);
        if (sl.h_dyn) (void) hipHostFree(sl.h_dyn);
        if (sl.h_flag) (void) hipHostFree(sl.h_flag);
        if (sl.d_dyn) (void) hipFree(sl.d_dyn);
        if (sl.copied) (void) hipEventDestroy(sl.copied);
        if (sl.done) (void) hipEventDestroy(sl.done);
        if (sl.out) (void) hipEventDestroy(sl.out);
    }
    if (s->d_arrivals) (void) hipFree(s->d_arrivals);
    if (s->d_stage) (void) hipFree(s->d_stage);
    if (s->g_part) (void) hipFree(s->g_part);
    if (s->g_raw) (void) hipFree(s->g_raw);
    if (s->copy) (void) hipStreamDestroy(s->copy);
    if (s->back) (void) hipStreamDestroy(s->back);
    delete s;
    return FX_OK;
}

fx_status fx_stream_create(fx_context* c, int hops_per_batch, int slots, int sample_format, fx_stream** out)
{
    if (!c || !out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (hops_per_batch < 1 || slots < 1 || slots > 64) return fx_fail(FX_ERR_INVALID_ARGUMENT, "hops_per_batch >= 1 and 1 <= slots <= 64 required");
    { const fx_status cs = fx_check_call(sample_format); if (cs != FX_OK) return cs; }
    HIP_TRY(hipSetDevice(c->device));
    fx_stream* s = new (std::nothrow) fx_stream();
    if (!s) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
    std::unique_ptr<fx_stream, fx_status (*)(fx_stream*)> half_built(s, fx_stream_destroy);    // destroyed on every return but the last
    s->ctx = c; s->hops = hops_per_batch; s->slots = slots; s->fmt = sample_format;
    s->fill.streaming = c->tuning.stream_fill_streaming != 0;
    s->in_bytes = (size_t) c->C * hops_per_batch * (c->N / 2) * sample_size(sample_format);
    s->out_bytes = (size_t) c->C * hops_per_batch * FX_NUM_FEATURES * sizeof(float);
    s->ring.resize((size_t) slots);
    HIP_TRY(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&s->back, hipStreamNonBlocking));
    // which of the equivalent paths runs: by batch size, unless the context's tuning forces one (experiments, tests)
    s->use_graph = c->tuning.stream_graph >= 0 ? c->tuning.stream_graph != 0 : (size_t) c->C * hops_per_batch <= 4096;
    // (up to 1 MiB of hops per call: the kernel reads each hop out of the pinned slot exactly once, 16 bytes per lane)
    s->use_hop_kernel = hops_per_batch == 1 && s->in_bytes <= 1024 * 1024 && fxk::hop_kernel_available(c->N)
                        && !(c->flags & (FX_SPECTRAL_ONLY | FX_HARMONIC_ONLY)) && c->tuning.stream_hop_kernel != 0 && s->use_graph;
    if (s->use_hop_kernel) s->use_graph = false;
    s->zero_copy = c->tuning.stream_zero_copy >= 0 ? c->tuning.stream_zero_copy != 0 : s->in_bytes <= 64 * 1024;
    if (s->use_hop_kernel) {
        HIP_TRY(hipMalloc((void**) &s->d_arrivals, sizeof(unsigned)));
        HIP_TRY(hipMemsetAsync(s->d_arrivals, 0, sizeof(unsigned), c->stream));
        HIP_TRY(hipMalloc(&s->d_stage, s->in_bytes));
    }
    // the hop kernel's results and flag are read by the host while the kernel may still be running: coherent (fine-grained) memory
    const unsigned host_flags = s->use_hop_kernel ? hipHostMallocCoherent : hipHostMallocDefault;
    if (s->use_graph) {
        HIP_TRY(hipMalloc((void**) &s->g_part, (size_t) c->C * hops_per_batch * sizeof(fxk::FramePart)));
        HIP_TRY(hipMalloc((void**) &s->g_raw, s->out_bytes));
    }
    for (auto& sl : s->ring) {
        if (s->use_graph) {
            HIP_TRY(hipHostMalloc((void**) &sl.h_dyn, sizeof(fxk::DynParams), hipHostMallocDefault));
            HIP_TRY(hipMalloc((void**) &sl.d_dyn, sizeof(fxk::DynParams)));
        }
        if (s->use_hop_kernel) {
            HIP_TRY(hipHostMalloc((void**) &sl.h_flag, 64, hipHostMallocCoherent));
            *sl.h_flag = 0;
        }
        HIP_TRY(hipHostMalloc(&sl.h_in, s->in_bytes, host_flags));
        HIP_TRY(hipHostMalloc((void**) &sl.h_raw, s->out_bytes, host_flags));
        HIP_TRY(hipHostMalloc((void**) &sl.h_sm, s->out_bytes, host_flags));
        HIP_TRY(hipMalloc(&sl.d_in, s->in_bytes));
        HIP_TRY(hipMalloc((void**) &sl.d_raw, s->out_bytes));
        HIP_TRY(hipMalloc((void**) &sl.d_sm, s->out_bytes));
        HIP_TRY(hipEventCreateWithFlags(&sl.copied, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&sl.out, hipEventDisableTiming));
    }
    *out = half_built.release();
    return FX_OK;
}

int fx_stream_in_flight(fx_stream* s) { return s ? s->in_flight : 0; }

fx_status fx_stream_acquire(fx_stream* s, void** host_slot)
{
    if (!s || !host_slot) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (s->acquired) return fx_fail(FX_ERR_INVALID_ARGUMENT, "a slot is already acquired; submit it first");
    HIP_TRY(hipSetDevice(s->ctx->device));
    if (s->in_flight == s->slots)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "all %d slots are in flight; collect a batch first", s->slots);
    *host_slot = s->ring[(size_t) s->head].h_in;
    s->acquired = true;
    return FX_OK;
}

fx_status fx_stream_submit(fx_stream* s)
{
    if (!s) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null stream");
    if (!s->acquired) return fx_fail(FX_ERR_INVALID_ARGUMENT, "no slot acquired");
    SlotGuard g{s};
    fx_context* c = s->ctx;
    begin_launches(c);
    HIP_TRY(hipSetDevice(c->device));
    fx_stream::Slot& sl = s->ring[(size_t) s->head];
    fx_status st;
    if ((st = fx_check_device_error(c)) != FX_OK) return st;
    if (c->carry_count > 0)
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "%d samples per channel are pending from fx_stream_submit_samples / fx_push_samples; whole hops would overtake them", c->carry_count);
    if (s->use_hop_kernel) {
        if (!sl.dev_flag && (st = slot_views(sl, sl.h_flag, &sl.dev_in, &sl.dev_raw, &sl.dev_sm, &sl.dev_flag)) != FX_OK) return st;
        Plan plan;
        if ((st = plan_call(c, sl.dev_in, 1, s->fmt, 1, sl.dev_raw, sl.dev_sm, nullptr, nullptr, nullptr, nullptr, ROUTE_RING_HOP, &plan)) != FX_OK) return st;
        if (++s->next_seq == 0) s->next_seq = 1;            // 0 = "nothing completed yet"
        sl.seq = s->next_seq;
        const fxk::HopSignal sig = {s->d_arrivals, sl.dev_flag, sl.seq, 0u, s->d_stage};
        const hipError_t e = enqueue(c, plan.launch[0], sig);
        if (e != hipSuccess) return fx_fail(FX_ERR_HIP, "launching the hop kernel failed: %s", hipGetErrorString(e));
        c->ev_valid = false;
        advance(c, 1);
        commit_slot(s, sl, 1, false);
        return FX_OK;
    }
    if (s->use_graph) {
        const int par = c->cur;
        fill_dyn(c, sl.h_dyn);
        // a graph keeps the addresses it was captured with: a step captured before the per-track table existed is captured once more
        // (likewise the scratch of the batch kernel's flux runs, which follows the largest call the context has seen)
        if ((st = fx_grow(&c->d_flux_park, &c->flux_park_cap, flux_park_need(c, s->hops))) != FX_OK) return st;
        if (sl.exec[par] && (sl.captured[par].launch[0].fp.chan != c->d_chan || sl.captured[par].launch[0].fp.flux_park != c->d_flux_park)) {
            const hipGraphExec_t old = sl.exec[par];
            sl.exec[par] = nullptr;
            HIP_TRY(hipGraphExecDestroy(old));
        }
        if (!sl.exec[par]) {
            // capture the step once for this slot and parity: everything below is recorded, not executed
            // A few KB per step: the kernels read the hop and the per-call scalars straight from the pinned host slot and
            // write the 12-float vectors straight back (zero copy), so the graph is two kernel nodes and no copy nodes;
            // larger batches keep explicit copies (PCIe is read best in bulk).
            const bool zero_copy = s->zero_copy;
            const void* in_dev = sl.d_in;
            float* raw_dev = sl.d_raw; float* sm_dev = sl.d_sm;
            fxk::DynParams* dyn_dev = sl.d_dyn;
            if (zero_copy && (st = slot_views(sl, sl.h_dyn, &in_dev, &raw_dev, &sm_dev, &dyn_dev)) != FX_OK) return st;
            Plan plan;
            if ((st = plan_call(c, in_dev, s->hops, s->fmt, 1, raw_dev, sm_dev, nullptr, dyn_dev, s->g_part, s->g_raw, ROUTE_RING_CAPTURED, &plan)) != FX_OK) return st;
            hipGraph_t graph = nullptr;
            HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            hipError_t e = hipSuccess;
            if (!zero_copy) {
                e = hipMemcpyAsync(sl.d_in, sl.h_in, s->in_bytes, hipMemcpyHostToDevice, c->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(sl.d_dyn, sl.h_dyn, sizeof(fxk::DynParams), hipMemcpyHostToDevice, c->stream);
            }
            for (int i = 0; i < plan.n && e == hipSuccess; i++) e = enqueue(c, plan.launch[i]);
            if (!zero_copy) {
                if (e == hipSuccess) e = hipMemcpyAsync(sl.h_raw, sl.d_raw, s->out_bytes, hipMemcpyDeviceToHost, c->stream);
                if (e == hipSuccess) e = hipMemcpyAsync(sl.h_sm, sl.d_sm, s->out_bytes, hipMemcpyDeviceToHost, c->stream);
            }
            const hipError_t e2 = hipStreamEndCapture(c->stream, &graph);       // (always: a failed step must not leave the capture open)
            if (e == hipSuccess) e = e2;
            if (e == hipSuccess) e = hipGraphInstantiate(&sl.exec[par], graph, nullptr, nullptr, 0);
            if (graph) (void) hipGraphDestroy(graph);
            if (e != hipSuccess) {
                sl.exec[par] = nullptr;
                return fx_fail(FX_ERR_HIP, "capturing the streaming step failed: %s", hipGetErrorString(e));
            }
            sl.captured[par] = plan;        // (kept with the graph only: a capture that failed is planned afresh when it is tried again)
        } else {
            for (int i = 0; i < sl.captured[par].n; i++) note_planned(c, sl.captured[par].launch[i]);     // what the graph launches each time it is replayed
        }
        HIP_TRY(hipGraphLaunch(sl.exec[par], c->stream));
        // the step is enqueued: the context has moved on whatever happens to the bookkeeping event below
        c->ev_valid = false;
        advance(c, s->hops);
        const hipError_t er = hipEventRecord(sl.out, c->stream);
        commit_slot(s, sl, s->hops, true);
        if (er != hipSuccess) return fx_fail(FX_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(er));
        return FX_OK;
    }
    return submit_large(s, g, sl, s->in_bytes, -1);
}

fx_status fx_stream_submit_samples(fx_stream* s, int num_samples)
{
    if (!s) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null stream");
    if (!s->acquired) return fx_fail(FX_ERR_INVALID_ARGUMENT, "no slot acquired");
    SlotGuard g{s};
    fx_context* c = s->ctx;
    begin_launches(c);
    if (num_samples < 0 || (long long) num_samples > (long long) s->hops * (c->N / 2))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "a slot holds 0 .. %lld samples per channel, got %d", (long long) s->hops * (c->N / 2), num_samples);
    HIP_TRY(hipSetDevice(c->device));
    { const fx_status es = fx_check_device_error(c); if (es != FX_OK) return es; }
    return submit_large(s, g, s->ring[(size_t) s->head], (size_t) c->C * (size_t) num_samples * sample_size(s->fmt), num_samples);
}

fx_status fx_stream_push(fx_stream* s, const void* hops, int fill_threads)
{
    if (!s || !hops) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (fill_threads < 1 || fill_threads > 64) return fx_fail(FX_ERR_INVALID_ARGUMENT, "fill_threads must be in [1, 64]");
    void* slot = nullptr;
    const fx_status st = fx_stream_acquire(s, &slot);
    if (st != FX_OK) return st;
    s->fill.copy(slot, hops, s->in_bytes, fill_threads);
    return fx_stream_submit(s);
}

fx_status fx_stream_push_samples(fx_stream* s, const void* samples, int num_samples, int fill_threads)
{
    if (!s || (!samples && num_samples > 0)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (fill_threads < 1 || fill_threads > 64) return fx_fail(FX_ERR_INVALID_ARGUMENT, "fill_threads must be in [1, 64]");
    if (num_samples < 0 || (long long) num_samples > (long long) s->hops * (s->ctx->N / 2))
        return fx_fail(FX_ERR_INVALID_ARGUMENT, "a slot holds 0 .. %lld samples per channel, got %d", (long long) s->hops * (s->ctx->N / 2), num_samples);
    void* slot = nullptr;
    const fx_status st = fx_stream_acquire(s, &slot);
    if (st != FX_OK) return st;
    if (num_samples > 0) s->fill.copy(slot, samples, (size_t) s->ctx->C * (size_t) num_samples * sample_size(s->fmt), fill_threads);
    return fx_stream_submit_samples(s, num_samples);
}

fx_status fx_stream_collect(fx_stream* s, float* out_raw, float* out_smoothed)
{
    return fx_stream_collect_samples(s, out_raw, out_smoothed, nullptr);
}

fx_status fx_stream_collect_samples(fx_stream* s, float* out_raw, float* out_smoothed, int* frames_out)
{
    if (frames_out) *frames_out = 0;
    if (!s) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null stream");
    if (s->in_flight == 0) return fx_fail(FX_ERR_INVALID_ARGUMENT, "nothing in flight");
    HIP_TRY(hipSetDevice(s->ctx->device));
    fx_stream::Slot& sl = s->ring[(size_t) s->tail];
    if (!sl.by_event) {
        // the kernel stores the call's sequence number after its results: poll it (a hop takes tens of microseconds,
        // an event wait costs as much again); if it does not show up soon -- a large grid, a busy device -- wait for the stream
        volatile unsigned* flag = sl.h_flag;
        bool seen = false;
        for (int spin = 0; spin < 200000; spin++) {
            if (*flag == sl.seq) { seen = true; break; }
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
        }
        if (!seen) HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    } else {
        HIP_TRY(hipEventSynchronize(sl.out));
    }
    const size_t got_bytes = (size_t) s->ctx->C * (size_t) sl.frames * FX_NUM_FEATURES * sizeof(float);
    if (out_raw && got_bytes) memcpy(out_raw, sl.h_raw, got_bytes);
    if (out_smoothed && got_bytes) memcpy(out_smoothed, sl.h_sm, got_bytes);
    if (frames_out) *frames_out = sl.frames;
    s->tail = (s->tail + 1) % s->slots;
    s->in_flight--;
    if (sl.by_event && ++s->since_release >= 64 && (s->in_flight == 0 || s->since_release >= 4096)) {
        // The three-queue path orders its work with events alone and never synchronises a stream; the HIP runtime keeps what it has
        // submitted to a stream on record until somebody does (measured: 1.9 KB of host memory per batch, 37 MB per 20 000 blocks of a live
        // stream -- tools/rss_probe.py).  With the ring drained every queue is idle and the three calls return at once; a ring that never
        // drains gets them every 4096 batches, where they wait for the batches still in flight.
        s->since_release = 0;
        HIP_TRY(hipStreamSynchronize(s->copy));
        HIP_TRY(hipStreamSynchronize(s->ctx->stream));
        HIP_TRY(hipStreamSynchronize(s->back));
    }
    return fx_check_device_error(s->ctx);
}

} // extern "C"
