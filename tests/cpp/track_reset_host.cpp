// track_reset_host.cpp -- the host side of the per-track reset and clear (fx_reset_channels / fx_clear_pending_channels /
// fx_get_channel_frames, csrc/fx_tracks.hip) against tests/cpp/fake_hip/, under ASan + UBSan (tests/test_track_reset_cpu.py builds and
// runs it; fx_tracks.hip is compiled as C++, its kernel left out, and the launcher below stands in for it).  Part 1: argument
// validation -- a null context, a bad list, an entry out of range is named and nothing changes, no device use.  Part 2: one scenario
// (resets on a context without and with a per-track table, under a captured ring step, with samples pending, duplicates, a clear, a
// state reset) walked once per HIP call with that call failing: a call that fails reports FX_ERR_HIP / FX_ERR_OUT_OF_MEMORY, the
// tracks it did not list keep their host-side rows (frame count and settings), the next call works, nothing leaks.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "fx.h"
#include "fx_kernels.h"

extern "C" {
void fake_hip_reset(void);
void fake_hip_fail_at(long call);
long fake_hip_calls(void);
long fake_hip_live(void);
int fake_hip_failed(void);
const char* fake_hip_failed_name(void);
}

namespace {
int g_problems = 0;
const char* g_where = "";
long g_launches = 0;
bool g_bad_launch = false;
void problem(const char* what, const char* more = "")
{
    std::printf("PROBLEM [%s]: %s %s\n", g_where, what, more);
    g_problems++;
}
#define EXPECT(cond) do { if (!(cond)) problem("expected", #cond); } while (0)
constexpr int C = 6, N = 1024;
}

// the launcher fx_tracks.hip leaves to hipcc: counted and failable like every other launch of the fake; the fake's device memory is host
// memory, so the list the shim uploaded can be read here (the copy is made at once)
namespace fxk {
hipError_t launch_reset_channels_kernel(const ResetParams& p, hipStream_t)
{
    const hipError_t e = fake_hip_count("launch_reset_channels_kernel");
    if (e != hipSuccess) return e;
    g_launches++;
    if (p.n <= 0 || p.C != C || p.row_pieces != N / 8 || !p.list || !p.prev || !p.tail || !p.carry || !p.latest || !p.clear) g_bad_launch = true;
    for (int i = 0; p.list && i < p.n; i++) if (p.list[i] < 0 || p.list[i] >= C) g_bad_launch = true;
    return hipSuccess;
}
}

namespace {

struct Rows {
    std::vector<long long> frames = std::vector<long long>(C);
    std::vector<float> gain = std::vector<float>(C), sens = std::vector<float>(C);
    std::vector<int> window = std::vector<int>(C), type = std::vector<int>(C);
};
Rows get(fx_context* c)
{
    Rows r;
    if (fx_get_channel_frames(c, r.frames.data()) != FX_OK) problem("fx_get_channel_frames");
    if (fx_get_channel_settings(c, r.gain.data(), r.sens.data(), r.window.data(), r.type.data()) != FX_OK) problem("fx_get_channel_settings");
    return r;
}
bool same_settings(const Rows& a, const Rows& b)
{
    return !memcmp(a.gain.data(), b.gain.data(), C * 4) && !memcmp(a.sens.data(), b.sens.data(), C * 4) && a.window == b.window && a.type == b.type;
}

void validation()
{
    g_where = "validation";
    const int list[3] = {1, 4, 4};
    long long frames[C];
    EXPECT(fx_reset_channels(nullptr, list, 3) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "null context"));
    EXPECT(fx_clear_pending_channels(nullptr, list, 3) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_get_channel_frames(nullptr, frames) == FX_ERR_INVALID_ARGUMENT);
    fake_hip_reset();
    fx_context* c = nullptr;
    if (fx_create(&c, 0, C, N, 48000.0, 0) != FX_OK) { problem("fx_create"); return; }
    const Rows before = get(c);
    const long calls = fake_hip_calls();
    const int high[3] = {0, 2, C}, low[2] = {3, -1};
    EXPECT(fx_reset_channels(c, nullptr, 0) == FX_OK && fx_clear_pending_channels(c, nullptr, 0) == FX_OK && fx_reset_channels(c, list, 0) == FX_OK);
    EXPECT(fx_reset_channels(c, nullptr, 2) == FX_ERR_INVALID_ARGUMENT && fx_clear_pending_channels(c, nullptr, 1) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_reset_channels(c, list, -1) == FX_ERR_INVALID_ARGUMENT && fx_clear_pending_channels(c, list, -3) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_reset_channels(c, high, 3) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "entry 2"));
    EXPECT(fx_clear_pending_channels(c, low, 2) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "entry 1"));
    EXPECT(fx_get_channel_frames(c, nullptr) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fake_hip_calls() == calls && g_launches == 0);           // nothing of it touched the device
    const Rows after = get(c);
    EXPECT(after.frames == before.frames && same_settings(after, before));
    EXPECT(fx_destroy(c) == FX_OK && fake_hip_live() == 0);
}

// a reset takes effect whole, or the tracks it did not list keep their rows; returns its status
fx_status reset_checked(fx_context* c, const std::vector<int>& list, const char* what)
{
    const Rows before = get(c);
    const fx_status st = fx_reset_channels(c, list.data(), (int) list.size());
    const Rows after = get(c);
    std::vector<bool> listed(C, false);
    for (int ch : list) listed[(size_t) ch] = true;
    if (!same_settings(after, before)) problem(what, "changed a setting");
    if (st != FX_OK && st != FX_ERR_HIP && st != FX_ERR_OUT_OF_MEMORY) problem(what, "failed with a status that is not a device failure");
    for (int i = 0; i < C; i++) {
        if (!listed[(size_t) i]) { if (after.frames[(size_t) i] != before.frames[(size_t) i]) problem(what, "moved a track it did not list"); }
        else if (st == FX_OK) { if (after.frames[(size_t) i] != 0) problem(what, "succeeded and a listed track does not start at frame 0"); }
        else if (after.frames[(size_t) i] != 0 && after.frames[(size_t) i] != before.frames[(size_t) i]) problem(what, "failed and left a frame count that is neither");
    }
    return st;
}

bool scenario(fx_context** ctx_out, fx_stream** ring_out)
{
    bool ok = true;
    fx_context* c = nullptr;
    if (fx_create(&c, 0, C, N, 48000.0, 0) != FX_OK) return false;
    *ctx_out = c;
    fx_tuning t;
    if (fx_get_tuning(c, &t) != FX_OK) return false;
    t.stream_hop_kernel = 0;                    // the ring's one-hop step is then the captured step (hipGraph)
    ok &= fx_set_tuning(c, &t) == FX_OK;
    std::vector<float> hops((size_t) C * 4 * (N / 2), 0.25f), raw((size_t) C * 4 * FX_NUM_FEATURES), sm(raw.size());
    ok &= fx_push_hops(c, hops.data(), 3, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data()) == FX_OK;
    fx_stream* ring = nullptr;
    if (fx_stream_create(c, 1, 2, FX_SAMPLE_F32, &ring) == FX_OK) *ring_out = ring; else ok = false;
    auto ring_steps = [&](int n) {
        for (int i = 0; ring && i < n; i++) {
            if (fx_stream_push(ring, hops.data(), 1) != FX_OK) { ok = false; continue; }
            ok &= fx_stream_collect(ring, raw.data(), sm.data()) == FX_OK;
        }
    };
    ring_steps(3);                              // both parities of the step captured without a table
    ok &= reset_checked(c, {1, 4}, "fx_reset_channels (first: the table appears)") == FX_OK;
    ring_steps(3);                              // captured once more with the table's address
    const float g[C] = {1, 0, -1, 2, 0.5f, 4};
    ok &= fx_set_channel_gains(c, g) == FX_OK;
    ok &= reset_checked(c, {5}, "fx_reset_channels over a table") == FX_OK;
    int frames = 0;
    ok &= fx_push_samples(c, hops.data(), 700, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data(), &frames) == FX_OK;
    const int pending = fx_pending_samples(c);
    ok &= reset_checked(c, {4, 4, 0}, "fx_reset_channels with samples pending and a duplicate") == FX_OK;
    const int two[2] = {2, 3};
    {
        const Rows before = get(c);
        const fx_status st = fx_clear_pending_channels(c, two, 2);
        const Rows after = get(c);
        if (after.frames != before.frames || !same_settings(after, before)) problem("fx_clear_pending_channels", "changed a row");
        if (st != FX_OK && st != FX_ERR_HIP && st != FX_ERR_OUT_OF_MEMORY) problem("fx_clear_pending_channels", "failed with a status that is not a device failure");
        ok &= st == FX_OK;
    }
    if (fx_pending_samples(c) != pending) problem("the pending count moved");
    ok &= fx_push_samples(c, hops.data(), 400, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data(), &frames) == FX_OK;
    std::vector<int> all;
    for (int i = 0; i < C; i++) all.push_back(i);
    ok &= reset_checked(c, all, "fx_reset_channels of every track") == FX_OK;
    if (fx_reset_state(c) == FX_OK) {
        const Rows r = get(c);
        for (int i = 0; i < C; i++) if (r.frames[(size_t) i] != 0) problem("fx_reset_state", "left a track's frame index above 0");
    } else ok = false;
    ok &= fx_push_hops(c, hops.data(), 2, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data()) == FX_OK;
    return ok;
}

void finish(fx_context* c, fx_stream* ring)
{
    fake_hip_fail_at(0);
    if (c) {
        // with the fault gone the calls work, whatever it interrupted
        const int list[2] = {0, 5};
        if (fx_reset_channels(c, list, 2) != FX_OK) problem("fx_reset_channels after the fault");
        if (fx_clear_pending_channels(c, list, 1) != FX_OK) problem("fx_clear_pending_channels after the fault");
        const Rows r = get(c);
        if (r.frames[0] != 0 || r.frames[5] != 0) problem("the tracks reset after the fault do not start at frame 0");
    }
    if (ring && fx_stream_destroy(ring) != FX_OK) problem("fx_stream_destroy");
    if (c && fx_destroy(c) != FX_OK) problem("fx_destroy");
    if (fake_hip_live() != 0) problem("device objects left behind");
}

void walk()
{
    g_where = "clean run";
    fake_hip_reset();
    fx_context* c = nullptr; fx_stream* ring = nullptr;
    if (!scenario(&c, &ring)) problem("the scenario fails without any injected failure:", fx_last_error());
    if (c) {
        // (clean run only) the frame counts after the scenario's last two hops
        const Rows r = get(c);
        for (int i = 0; i < C; i++) if (r.frames[(size_t) i] != 2) problem("frame counts after fx_reset_state and two hops");
    }
    const long calls = fake_hip_calls();
    finish(c, ring);
    if (g_launches < 6) problem("the reset kernel was not launched once per call");
    int reported = 0;
    for (long k = 1; k <= calls; k++) {
        char tag[128];
        fake_hip_reset();
        fake_hip_fail_at(k);
        std::snprintf(tag, sizeof tag, "HIP call %ld failing", k);
        g_where = tag;
        c = nullptr; ring = nullptr;
        const bool fine = scenario(&c, &ring);
        if (fake_hip_failed() && !fine) reported++;
        std::snprintf(tag, sizeof tag, "HIP call %ld (%s) failing", k, fake_hip_failed() ? fake_hip_failed_name() : "not reached");
        finish(c, ring);
    }
    if (g_bad_launch) problem("a launch of the reset kernel had a bad argument");
    std::printf("scenario: %ld HIP calls, each failed once, %d reported to the caller\n", calls, reported);
}

} // namespace

int main()
{
    validation();
    walk();
    std::printf("%s: %d problems\n", g_problems ? "FAILED" : "ok", g_problems);
    return g_problems ? 1 : 0;
}
