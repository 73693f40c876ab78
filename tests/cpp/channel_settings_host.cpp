// channel_settings_host.cpp -- the host side of the per-track settings (fx_set_channel_gains / fx_set_channel_onset /
// fx_get_channel_settings, csrc/fx_capi.cpp) against tests/cpp/fake_hip/, under ASan + UBSan (tests/test_channel_settings_cpu.py builds
// and runs it).  Part 1: argument validation -- a null context, a bad entry names its track and changes nothing -- and the round trip
// through per-track and context-wide setters.  Part 2: one scenario (calls, the table appearing under a captured ring step, updates,
// a state reset) walked once per HIP call with that call failing: a setter that fails reports FX_ERR_HIP / FX_ERR_OUT_OF_MEMORY and
// leaves the old settings in force, the next one works, nothing leaks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fx.h"

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
void problem(const char* what, const char* more = "")
{
    std::printf("PROBLEM [%s]: %s %s\n", g_where, what, more);
    g_problems++;
}
#define EXPECT(cond) do { if (!(cond)) problem("expected", #cond); } while (0)

constexpr int C = 6, N = 1024;

struct Settings {
    std::vector<float> gain = std::vector<float>(C), sens = std::vector<float>(C);
    std::vector<int> window = std::vector<int>(C), type = std::vector<int>(C);
    bool operator==(const Settings& o) const
    {
        return !memcmp(gain.data(), o.gain.data(), C * 4) && !memcmp(sens.data(), o.sens.data(), C * 4) && window == o.window && type == o.type;
    }
};
Settings get(fx_context* c)
{
    Settings s;
    if (fx_get_channel_settings(c, s.gain.data(), s.sens.data(), s.window.data(), s.type.data()) != FX_OK) problem("fx_get_channel_settings");
    return s;
}

void validation()
{
    g_where = "validation";
    const float g[C] = {1, 0, -1, 2, 3, 4};
    EXPECT(fx_set_channel_gains(nullptr, g) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_set_channel_onset(nullptr, g, nullptr, nullptr) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_get_channel_settings(nullptr, nullptr, nullptr, nullptr, nullptr) == FX_ERR_INVALID_ARGUMENT);
    fake_hip_reset();
    fx_context* c = nullptr;
    if (fx_create(&c, 0, C, N, 48000.0, 0) != FX_OK) { problem("fx_create"); return; }
    const Settings d = get(c);
    for (int i = 0; i < C; i++) EXPECT(d.gain[i] == 1.0f && d.sens[i] == 0.7f && d.window[i] == 5 && d.type[i] == FX_ONSET_AMPLITUDE);
    // all-NULL calls and nothing-to-do calls touch no device
    long before = fake_hip_calls();
    EXPECT(fx_set_channel_gains(c, nullptr) == FX_OK && fx_set_channel_onset(c, nullptr, nullptr, nullptr) == FX_OK);
    EXPECT(fake_hip_calls() == before);
    // bad entries: refused before any device use, the track named, nothing changed
    const float sens[C] = {0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f};
    float bad_sens[C]; memcpy(bad_sens, sens, sizeof sens); bad_sens[4] = -0.5f;
    float nan_sens[C]; memcpy(nan_sens, sens, sizeof sens); nan_sens[1] = NAN;
    const int win[C] = {1, 3, -1, 21, 32, -7};
    int bad_win[C]; memcpy(bad_win, win, sizeof win); bad_win[2] = 0;
    int big_win[C]; memcpy(big_win, win, sizeof win); big_win[5] = 33;
    const int type[C] = {0, 1, 2, 0, 1, 2};
    int bad_type[C]; memcpy(bad_type, type, sizeof type); bad_type[3] = 3;
    int neg_type[C]; memcpy(neg_type, type, sizeof type); neg_type[0] = -1;
    before = fake_hip_calls();
    EXPECT(fx_set_channel_onset(c, bad_sens, win, type) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "track 4"));
    EXPECT(fx_set_channel_onset(c, nan_sens, nullptr, nullptr) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "track 1"));
    EXPECT(fx_set_channel_onset(c, sens, bad_win, type) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "track 2"));
    EXPECT(fx_set_channel_onset(c, nullptr, big_win, nullptr) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "track 5"));
    EXPECT(fx_set_channel_onset(c, sens, win, bad_type) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "track 3"));
    EXPECT(fx_set_channel_onset(c, nullptr, nullptr, neg_type) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "track 0"));
    EXPECT(fake_hip_calls() == before);
    EXPECT(get(c) == d);
    // the round trip; window < 0 keeps the track's window
    EXPECT(fx_set_channel_gains(c, g) == FX_OK);
    EXPECT(fx_set_channel_onset(c, sens, win, type) == FX_OK);
    Settings s = get(c);
    for (int i = 0; i < C; i++) EXPECT(s.gain[i] == g[i] && s.sens[i] == sens[i] && s.window[i] == (win[i] > 0 ? win[i] : 5) && s.type[i] == type[i]);
    EXPECT(fx_set_channel_onset(c, bad_sens, win, type) == FX_ERR_INVALID_ARGUMENT && get(c) == s);      // with a table as well
    // gains are any float, as fx_set_gain takes them
    const float odd[C] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 1e30f};
    EXPECT(fx_set_channel_gains(c, odd) == FX_OK);
    EXPECT(!memcmp(get(c).gain.data(), odd, sizeof odd));
    // the context-wide setters set every track; fx_reset_state keeps the settings
    EXPECT(fx_set_gain(c, 0.5f) == FX_OK && fx_set_onset_window(c, 9) == FX_OK && fx_set_onset_type(c, FX_ONSET_SPECTRAL) == FX_OK);
    EXPECT(fx_set_onset_sensitivity(c, 0.25f) == FX_OK);
    EXPECT(fx_set_onset_window(c, 0) == FX_ERR_INVALID_ARGUMENT && fx_set_onset_sensitivity(c, -1.0f) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_reset_state(c) == FX_OK);
    s = get(c);
    for (int i = 0; i < C; i++) EXPECT(s.gain[i] == 0.5f && s.sens[i] == 0.25f && s.window[i] == 9 && s.type[i] == FX_ONSET_SPECTRAL);
    EXPECT(fx_destroy(c) == FX_OK);
    EXPECT(fake_hip_live() == 0);
}

// a setter either takes effect whole or leaves what was there; returns its status
template <typename F> fx_status all_or_nothing(fx_context* c, const Settings& want, F call, const char* what)
{
    const Settings before = get(c);
    const fx_status st = call();
    const Settings after = get(c);
    if (st == FX_OK) { if (!(after == want)) problem(what, "succeeded and the settings are not the new ones"); }
    else {
        if (st != FX_ERR_HIP && st != FX_ERR_OUT_OF_MEMORY) problem(what, "failed with a status that is not a device failure");
        if (!(after == before)) problem(what, "failed and the settings changed");
    }
    return st;
}

// every call may fail (one HIP call is made to); returns whether all succeeded
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
    ok &= fx_push_hops(c, hops.data(), 4, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data()) == FX_OK;
    fx_stream* ring = nullptr;
    if (fx_stream_create(c, 1, 2, FX_SAMPLE_F32, &ring) == FX_OK) *ring_out = ring; else ok = false;
    auto ring_steps = [&](int n) {
        for (int i = 0; ring && i < n; i++) {
            if (fx_stream_push(ring, hops.data(), 1) != FX_OK) { ok = false; continue; }
            ok &= fx_stream_collect(ring, raw.data(), sm.data()) == FX_OK;
        }
    };
    ring_steps(3);                              // both parities of the step captured without a table
    Settings want = get(c);
    const float g[C] = {1, 0, -1, 2, 0.5f, 4};
    for (int i = 0; i < C; i++) want.gain[i] = g[i];
    ok &= all_or_nothing(c, want, [&] { return fx_set_channel_gains(c, g); }, "fx_set_channel_gains (first: the table appears)") == FX_OK;
    ring_steps(3);                              // captured once more with the table's address
    const float sens[C] = {0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f};
    const int win[C] = {1, 3, -1, 21, 32, 5}, type[C] = {0, 1, 2, 0, 1, 2};
    want = get(c);
    for (int i = 0; i < C; i++) { want.sens[i] = sens[i]; if (win[i] > 0) want.window[i] = win[i]; want.type[i] = type[i]; }
    ok &= all_or_nothing(c, want, [&] { return fx_set_channel_onset(c, sens, win, type); }, "fx_set_channel_onset") == FX_OK;
    ring_steps(2);
    ok &= fx_push_hops(c, hops.data(), 1, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data()) == FX_OK;
    want = get(c);
    for (int i = 0; i < C; i++) want.gain[i] = 0.5f;
    ok &= all_or_nothing(c, want, [&] { return fx_set_gain(c, 0.5f); }, "fx_set_gain over a table") == FX_OK;
    want = get(c);
    for (int i = 0; i < C; i++) want.window[i] = 7;
    ok &= all_or_nothing(c, want, [&] { return fx_set_onset_window(c, 7); }, "fx_set_onset_window over a table") == FX_OK;
    want = get(c);
    ok &= all_or_nothing(c, want, [&] { return fx_reset_state(c); }, "fx_reset_state") == FX_OK;
    ok &= fx_push_hops(c, hops.data(), 2, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data()) == FX_OK;
    return ok;
}

void finish(fx_context* c, fx_stream* ring)
{
    fake_hip_fail_at(0);
    if (c) {
        // with the fault gone the setters work, whatever it interrupted
        const float g[C] = {2, 2, 2, 2, 2, 3};
        const int win[C] = {4, 4, 4, 4, 4, 4};
        if (fx_set_channel_gains(c, g) != FX_OK) problem("fx_set_channel_gains after the fault");
        if (fx_set_channel_onset(c, nullptr, win, nullptr) != FX_OK) problem("fx_set_channel_onset after the fault");
        const Settings s = get(c);
        if (s.gain[5] != 3.0f || s.window[0] != 4) problem("the settings after the fault are not the ones set");
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
    const long calls = fake_hip_calls();
    finish(c, ring);
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
