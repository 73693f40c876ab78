// fx_osc_table.hip -- per-track OSC addresses for the sink at scale (include/fx.h: fx_set_osc_addresses, fx_osc_address_stride,
// fx_get_osc_datagrams_addressed).
//
// ref AnalyserTrackController.h:17,22-23: every track is built with (ip, secondaryIP, bundle) and the GUI edits them per track
// (:140-147, setBundleAddressChangedCallback); each of its OSCFeatureAnalysisOutput senders sends bundleAddress
// (OSCFeatureAnalysisOutput.h:107).  fx_get_osc_datagrams (fx_osc.hip) knows one address shape, "<prefix><channel number>"; here the
// addresses are a table in device memory -- zero-padded rows of 128 bytes and int len[C] -- so that a track may be "/Mixer/Drums/Kick"
// and the address part of its message is aligned word copies.  The targets per track are the sender's (fx_osc_sender_set_routes).
//
// fx_osc_table_kernel: one thread per 4-byte word of output, as fx_osc_kernel; a word is a word of the track's row, one of the four
// tag words or a byte-swapped float of `latest` (osc_table_word, fx_osc_words.h: the same function a host program runs).  Pure byte
// movement: at most 192 B out and 48 + 128 B in per track, no LDS.
//
// Nothing in the shim's host units (build.py, HOST_SOURCES) refers to this unit: fx_set_osc_addresses installs the context's release
// hook (fx_context.h).  The table is a setting: fx_reset_state and fx_reset_channels never touch it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "fx_kernels.h"
#include "fx_context.h"
#include "fx_osc_words.h"

namespace fxk {

constexpr int OSC_TABLE_THREADS = 256;

__global__ void __launch_bounds__(OSC_TABLE_THREADS) fx_osc_table_kernel(const OscTableParams p)
{
    const int words = p.stride >> 2;
    const long long g = (long long) blockIdx.x * OSC_TABLE_THREADS + threadIdx.x;
    if (g >= (long long) p.C * words) return;
    const int c = (int) (g / words), w = (int) (g - (long long) c * words);
    const unsigned v = osc_table_word(p.rows + (size_t) c * FX_OSC_ROW_WORDS, p.len[c], p.latest + (size_t) c * FX_NUM_FEATURES, w);
    reinterpret_cast<unsigned*>(p.out + (size_t) c * (size_t) p.stride)[w] = v;
}

// stride: a multiple of 4 that holds the longest message of the table (the caller has checked it against the table's lengths, so a
// thread reads words [0, (len + 4) / 4) <= FX_OSC_ROW_WORDS of its row only)
static hipError_t launch_osc_table_kernel(const OscTableParams& p, hipStream_t stream)
{
    if (p.C <= 0) return hipSuccess;
    if (p.stride < 4 || (p.stride & 3) || !p.latest || !p.rows || !p.len || !p.out || (reinterpret_cast<uintptr_t>(p.out) & 3)) return hipErrorInvalidValue;
    const long long total = (long long) p.C * (p.stride >> 2);
    const long long wgs = (total + OSC_TABLE_THREADS - 1) / OSC_TABLE_THREADS;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fx_osc_table_kernel, dim3((unsigned) wgs), dim3(OSC_TABLE_THREADS), 0, stream, p);
    return hipGetLastError();
}

} // namespace fxk

namespace {

void osc_table_release(fx_context* c)
{
    fx_osc_table* t = c->osc_table;
    if (!t) return;
    if (t->d_table) (void) hipFree(t->d_table);
    delete t;
    c->osc_table = nullptr;
}

} // namespace

extern "C" {

fx_status fx_set_osc_addresses(fx_context* c, const char* const* addresses)
{
    if (!c) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null context");
    const size_t C = (size_t) c->C;
    const size_t rows_bytes = C * fxk::FX_OSC_ROW_BYTES, bytes = rows_bytes + C * sizeof(int);
    fx_osc_table* fresh = nullptr;
    std::vector<unsigned char> image;
    if (addresses) {
        // every entry is checked, and the image and the lengths are made, before anything is touched: no device use
        fresh = new (std::nothrow) fx_osc_table();
        if (!fresh) return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed");
        try {
            image.assign(bytes, 0);
            fresh->message_bytes.resize(C);
        } catch (const std::bad_alloc&) { delete fresh; return fx_fail(FX_ERR_OUT_OF_MEMORY, "host allocation failed"); }
        for (size_t i = 0; i < C; i++) {
            int alen = 0;
            if (const char* fault = fxk::osc_address_fault(addresses[i], &alen)) {
                delete fresh;
                return fx_fail(FX_ERR_INVALID_ARGUMENT, "track %d: the OSC address %s", (int) i, fault);
            }
            memcpy(image.data() + i * fxk::FX_OSC_ROW_BYTES, addresses[i], (size_t) alen);
            memcpy(image.data() + rows_bytes + i * sizeof(int), &alen, sizeof(int));
            fresh->message_bytes[i] = fxk::osc_addressed_bytes(alen);
            if (fresh->message_bytes[i] > fresh->longest) fresh->longest = fresh->message_bytes[i];
        }
    }
    std::unique_ptr<fx_osc_table, void (*)(fx_osc_table*)> guard(fresh, [](fx_osc_table* t) { if (t) { if (t->d_table) (void) hipFree(t->d_table); delete t; } });
    HIP_TRY(hipSetDevice(c->device));
    if (fresh) {
        // the new table is whole on the device before the old one goes: a failed allocation or upload leaves the old table in force
        HIP_TRY(hipMalloc((void**) &fresh->d_table, bytes));
        HIP_TRY(hipMemcpyAsync(fresh->d_table, image.data(), bytes, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));       // (nothing in flight reads the old table after this, and `image` is free)
    osc_table_release(c);
    c->osc_table = guard.release();
    if (c->osc_table) c->osc_table_release = osc_table_release;
    return FX_OK;
}

int fx_osc_address_stride(fx_context* c)
{
    return c && c->osc_table ? c->osc_table->longest : -1;
}

// ref OSCFeatureAnalysisOutput.h:89-113 for every track at once, each with its own bundleAddress (:107)
fx_status fx_get_osc_datagrams_addressed(fx_context* c, unsigned char* out, int stride, int* lengths, int mem_kind)
{
    if (!c || !out) return fx_fail(FX_ERR_INVALID_ARGUMENT, "null argument");
    if (mem_kind != FX_MEM_HOST && mem_kind != FX_MEM_DEVICE) return fx_fail(FX_ERR_INVALID_ARGUMENT, "unknown memory kind %d", mem_kind);
    const fx_osc_table* t = c->osc_table;
    if (!t) return fx_fail(FX_ERR_INVALID_ARGUMENT, "the context has no OSC address table (fx_set_osc_addresses)");
    if (stride < t->longest || (stride & 3)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "stride %d: must be a multiple of 4 and hold the longest message (%d bytes)", stride, t->longest);
    if (mem_kind == FX_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 3)) return fx_fail(FX_ERR_INVALID_ARGUMENT, "a device buffer of messages must start on a 4-byte boundary");
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = (size_t) c->C * (size_t) stride;
    if (mem_kind == FX_MEM_HOST) { const fx_status st = fx_grow(&c->d_osc, &c->osc_cap, bytes); if (st != FX_OK) return st; }
    fxk::OscTableParams p = {};
    p.latest = c->d_latest;
    p.rows = reinterpret_cast<const unsigned*>(t->d_table);
    p.len = reinterpret_cast<const int*>(t->d_table + (size_t) c->C * fxk::FX_OSC_ROW_BYTES);
    p.out = mem_kind == FX_MEM_HOST ? c->d_osc : out;
    p.C = c->C;
    p.stride = stride;
    c->num_launches = 0;                            // an entry point that launches starts the launch record anew
    note_launch(c, FX_LAUNCH_OSC_TABLE, 0);
    HIP_TRY(fxk::launch_osc_table_kernel(p, c->stream));
    if (lengths) memcpy(lengths, t->message_bytes.data(), (size_t) c->C * sizeof(int));
    if (mem_kind == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, c->d_osc, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fx_check_device_error(c);
    }
    return FX_OK;
}

} // extern "C"
