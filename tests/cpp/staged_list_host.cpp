// staged_list_host.cpp -- the pinned and device list pair the list-taking units share (csrc/fx_context.h: fx_staged_list,
// fx_reserve_list, fx_release_list) against tests/cpp/fake_hip/, under ASan + UBSan (tests/test_staged_list_cpu.py builds and runs it
// with the shim's host units of build.HOST_SOURCES).  Part 1: a list grows from nothing, by at least half again, makes no HIP call
// while a request fits, and lets go of everything.  Part 2: every HIP call of a growing reserve failed once -- the status is the
// call's, a failed allocation leaves the old pair in place and usable, a failed free leaves the new pair in place, nothing leaks.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "fx.h"
#include "fx_context.h"

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

constexpr size_t ENTRY = 24;            // bytes an entry (no power of two: a size computed in entries instead of bytes would show)
constexpr int GROW_CALLS = 5;           // hipStreamSynchronize, hipHostMalloc, hipMalloc, hipFree, hipHostFree
const char* const GROW_NAMES[GROW_CALLS] = {"hipStreamSynchronize", "hipHostMalloc", "hipMalloc", "hipFree", "hipHostFree"};

// both lists hold `entries` entries: every byte is written (ASan checks the room)
void use(const fx_staged_list& l, size_t entries, int value)
{
    memset(l.pinned, value, entries * ENTRY);
    memset(l.device, value, entries * ENTRY);
}
bool holds(const fx_staged_list& l, size_t entries, int value)
{
    for (size_t i = 0; i < entries * ENTRY; i++)
        if (static_cast<unsigned char*>(l.pinned)[i] != (unsigned char) value || static_cast<unsigned char*>(l.device)[i] != (unsigned char) value) return false;
    return true;
}

void clean(fx_context* c, long base)
{
    g_where = "clean run";
    fx_staged_list l;
    long calls = fake_hip_calls();
    fx_release_list(&l);                                            // an empty list: nothing to do
    EXPECT(fx_reserve_list(c, &l, 0, ENTRY) == FX_OK);              // and room for nothing is there already
    EXPECT(fake_hip_calls() == calls && !l.pinned && !l.device && l.cap == 0);
    // from nothing: exactly what was asked for, and no free
    EXPECT(fx_reserve_list(c, &l, 10, ENTRY) == FX_OK);
    EXPECT(fake_hip_calls() == calls + 3 && l.pinned && l.device && l.pinned != l.device && l.cap == 10 && fake_hip_live() == base + 2);
    use(l, 10, 0x11);
    // within capacity: no HIP call, the lists stay where they are and keep what they hold
    calls = fake_hip_calls();
    const fx_staged_list first = l;
    EXPECT(fx_reserve_list(c, &l, 10, ENTRY) == FX_OK && fx_reserve_list(c, &l, 7, ENTRY) == FX_OK && fx_reserve_list(c, &l, 0, ENTRY) == FX_OK);
    EXPECT(fake_hip_calls() == calls && l.pinned == first.pinned && l.device == first.device && l.cap == 10 && holds(l, 10, 0x11));
    // a request below half again grows to half again: the whole sequence of calls, one pair live afterwards
    EXPECT(fx_reserve_list(c, &l, 11, ENTRY) == FX_OK);
    EXPECT(fake_hip_calls() == calls + GROW_CALLS && l.cap == 15 && l.pinned != first.pinned && l.device != first.device && fake_hip_live() == base + 2);
    use(l, 15, 0x22);
    // a request beyond half again gets what it asks for
    EXPECT(fx_reserve_list(c, &l, 40, ENTRY) == FX_OK && l.cap == 40 && fake_hip_live() == base + 2);
    use(l, 40, 0x33);
    calls = fake_hip_calls();
    fx_release_list(&l);
    EXPECT(fake_hip_calls() == calls + 2 && !l.pinned && !l.device && l.cap == 0 && fake_hip_live() == base);
    fx_release_list(&l);
    EXPECT(fake_hip_calls() == calls + 2);
}

// a reserve that grows a list of `have` entries (0: from nothing) to hold 11, with its k-th HIP call failing
void failing(fx_context* c, long base, size_t have, int k)
{
    char tag[96];
    std::snprintf(tag, sizeof tag, "call %d (%s) of a reserve over %zu entries failing", k, GROW_NAMES[k - 1], have);
    g_where = tag;
    fx_staged_list l;
    if (have && fx_reserve_list(c, &l, have, ENTRY) != FX_OK) { problem("the first reserve"); return; }
    if (have) use(l, have, 0x44);
    const fx_staged_list old = l;
    fake_hip_fail_at(fake_hip_calls() + k);
    const fx_status st = fx_reserve_list(c, &l, 11, ENTRY);
    const bool fired = fake_hip_failed() != 0;
    const bool named = !strcmp(fake_hip_failed_name(), GROW_NAMES[k - 1]);
    fake_hip_fail_at(0);
    EXPECT(fired && named);
    // an allocation that fails is out of memory, any other call a HIP failure; the device allocation's message is the lists' own
    const bool allocation = k == 2 || k == 3;
    EXPECT(st == (allocation ? FX_ERR_OUT_OF_MEMORY : FX_ERR_HIP));
    if (k == 3) EXPECT(strstr(fx_last_error(), "allocating the track list failed: ") == fx_last_error());
    else EXPECT((k >= 4 || strstr(fx_last_error(), GROW_NAMES[k - 1]) != nullptr) && strstr(fx_last_error(), " failed: ") != nullptr);
    if (k <= 3) {
        // nothing has changed: the old pair is in place, holds what it held and can be used
        EXPECT(l.pinned == old.pinned && l.device == old.device && l.cap == have && fake_hip_live() == base + (have ? 2 : 0));
        if (have) { EXPECT(holds(l, have, 0x44)); use(l, have, 0x55); }
    } else {
        // both frees were attempted and the new pair is in place
        EXPECT(l.pinned && l.device && l.pinned != old.pinned && l.device != old.device && l.cap == 15 && fake_hip_live() == base + 2);
        use(l, l.cap, 0x55);
    }
    // with the fault gone the list grows
    EXPECT(fx_reserve_list(c, &l, 30, ENTRY) == FX_OK && l.cap == 30 && fake_hip_live() == base + 2);
    use(l, 30, 0x66);
    fx_release_list(&l);
    EXPECT(!l.pinned && !l.device && l.cap == 0 && fake_hip_live() == base);
}

} // namespace

int main()
{
    fake_hip_reset();
    fx_context* c = nullptr;
    if (fx_create(&c, 0, 2, 1024, 48000.0, 0) != FX_OK) { std::printf("FAILED: fx_create: %s\n", fx_last_error()); return 1; }
    const long base = fake_hip_live();
    clean(c, base);
    for (int k = 1; k <= 3; k++) failing(c, base, 0, k);            // from nothing there is nothing to free
    for (int k = 1; k <= GROW_CALLS; k++) failing(c, base, 10, k);
    g_where = "the end";
    EXPECT(fx_destroy(c) == FX_OK && fake_hip_live() == 0);
    std::printf("reserve: %d HIP calls, each failed once\n", GROW_CALLS);
    std::printf("%s: %d problems\n", g_problems ? "FAILED" : "ok", g_problems);
    return g_problems ? 1 : 0;
}
