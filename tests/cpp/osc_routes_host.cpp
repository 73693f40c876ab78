// osc_routes_host -- per-track targets of the batch sender (fx_osc_sender_set_routes, csrc/fx_osc_sender.cpp; ref
// AnalyserTrackController.h:17,22-23: every track's own ip and secondaryIP) over loopback, against three counting receivers.
// A stand-alone program, built twice by tests/test_osc_routes_cpp.py: with -fsanitize=address,undefined and with -fsanitize=thread.
//
// 37 tracks of fx_osc_encode_batch messages ("/Audio/A<n>", so the receivers keep the newest message per track), routes that scatter the
// tracks over the three receivers, some without a secondary; sender threads 1, 3, 4, segmented sends on and off.  After k manual ticks
// each receiver holds exactly k x (its primary + secondary tracks) datagrams, the newest bytes of exactly its tracks and nothing of
// the others.  Routes are changed while the timer runs; bad arguments leave the old routes in force; routes that send every track to
// the create-time target cost the datagrams and system calls of a sender without routes.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fx.h"

static int problems = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { problems++; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

namespace {

constexpr int C = 37, R = 3;

struct Messages {
    std::vector<unsigned char> data;
    std::vector<int> len;
    int stride = 0;
    explicit Messages(unsigned seed)
    {
        std::vector<float> v((size_t) C * FX_NUM_FEATURES);
        for (float& x : v) { seed = seed * 1664525u + 1013904223u; x = (float) ((int) (seed >> 8) % 20001 - 10000) * 1e-3f; }
        stride = fx_osc_message_bytes("/Audio/A", C - 1);
        data.resize((size_t) C * (size_t) stride);
        len.resize((size_t) C);
        EXPECT(fx_osc_encode_batch("/Audio/A", 0, C, v.data(), data.data(), stride, len.data()) == C, "fx_osc_encode_batch");
    }
};

struct Receivers {
    fx_osc_receiver* rx[R] = {nullptr, nullptr, nullptr};
    std::string target[R];
    Receivers()
    {
        for (int r = 0; r < R; r++) {
            EXPECT(fx_osc_receiver_create(&rx[r], "127.0.0.1:0", 1, "/Audio/A", C, r == 1 ? FX_OSC_RECEIVER_NO_GRO : 0u) == FX_OK, "receiver %d: %s", r, fx_last_error());
            target[r] = "127.0.0.1:" + std::to_string(fx_osc_receiver_port(rx[r]));
        }
    }
    ~Receivers() { for (int r = 0; r < R; r++) fx_osc_receiver_destroy(rx[r]); }
    long long datagrams(int r) const { long long n = 0, bad = 0; fx_osc_receiver_get_stats(rx[r], &n, nullptr, &bad); EXPECT(bad == 0, "receiver %d: %lld malformed", r, bad); return n; }
    // polls at most 2 s for receiver r to have counted `want` datagrams; returns what it has then
    long long wait_for(int r, long long want) const
    {
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(2);
        long long n = datagrams(r);
        while (n < want && std::chrono::steady_clock::now() < deadline) { std::this_thread::sleep_for(std::chrono::milliseconds(1)); n = datagrams(r); }
        return n;
    }
    const char* targets3(const char** list) const { for (int r = 0; r < R; r++) list[r] = target[r].c_str(); return list[0]; }
};

struct RouteTable {
    std::vector<int> primary, secondary;
    int per_target[R] = {0, 0, 0};
    explicit RouteTable(int variant) : primary((size_t) C), secondary((size_t) C)
    {
        for (int i = 0; i < C; i++) {
            primary[(size_t) i] = (i + variant) % R;
            secondary[(size_t) i] = (i % 4 == 0) ? -1 : (primary[(size_t) i] + 1 + (i % 2)) % R;      // never the primary again
            per_target[primary[(size_t) i]]++;
            if (secondary[(size_t) i] >= 0) per_target[secondary[(size_t) i]]++;
        }
    }
    bool serves(int r, int i) const { return primary[(size_t) i] == r || secondary[(size_t) i] == r; }
};

long long tick(fx_osc_sender* s)
{
    long long sent = -1;
    EXPECT(fx_osc_sender_send(s, &sent) == FX_OK, "send: %s", fx_last_error());
    return sent;
}

void scatter(int threads, bool gso)
{
    Receivers rcv;
    const char* targets[R];
    rcv.targets3(targets);
    const RouteTable routes(0);
    const Messages a(1u), b(2u);
    fx_osc_sender* s = nullptr;
    EXPECT(fx_osc_sender_create(&s, "127.0.0.1:9", nullptr, threads, gso ? FX_OSC_SENDER_GSO : 0u) == FX_OK, "create: %s", fx_last_error());
    if (!s) return;
    EXPECT(fx_osc_sender_set_routes(s, targets, R, routes.primary.data(), routes.secondary.data(), C) == FX_OK, "set_routes: %s", fx_last_error());
    EXPECT(tick(s) == 0, "a tick before any publication sent something");
    EXPECT(fx_osc_sender_update(s, a.data.data(), a.stride, a.len.data(), C) == FX_OK, "update: %s", fx_last_error());
    const long long per_tick = routes.per_target[0] + routes.per_target[1] + routes.per_target[2];
    const int k = 3;
    EXPECT(tick(s) == per_tick && tick(s) == per_tick, "threads %d gso %d: a tick did not send %lld datagrams", threads, (int) gso, per_tick);
    EXPECT(fx_osc_sender_update(s, b.data.data(), b.stride, b.len.data(), C) == FX_OK, "update: %s", fx_last_error());
    EXPECT(tick(s) == per_tick, "threads %d gso %d: the third tick", threads, (int) gso);
    for (int r = 0; r < R; r++) {
        const long long want = (long long) k * routes.per_target[r];
        const long long got = rcv.wait_for(r, want);
        EXPECT(got == want, "threads %d gso %d: receiver %d counted %lld datagrams, not %lld", threads, (int) gso, r, got, want);
        for (int i = 0; i < C; i++) {
            unsigned char last[160];
            int n = -1;
            EXPECT(fx_osc_receiver_last(rcv.rx[r], i, last, (int) sizeof last, &n) == FX_OK, "last: %s", fx_last_error());
            if (routes.serves(r, i))
                EXPECT(n == b.len[(size_t) i] && std::memcmp(last, b.data.data() + (size_t) i * (size_t) b.stride, (size_t) n) == 0,
                       "threads %d gso %d: receiver %d does not hold the newest message of its track %d", threads, (int) gso, r, i);
            else
                EXPECT(n == 0, "threads %d gso %d: receiver %d holds a message of track %d, which is not routed to it", threads, (int) gso, r, i);
        }
    }
    fx_osc_sender_stats st;
    EXPECT(fx_osc_sender_get_stats(s, &st) == FX_OK && st.datagrams == k * per_tick && st.dropped == 0, "threads %d gso %d: %lld datagrams, %lld dropped", threads, (int) gso, st.datagrams, st.dropped);

    // bad arguments: the old routes stay in force (the next tick is distributed as before)
    std::vector<int> bad = routes.primary;
    bad[C - 1] = R;
    EXPECT(fx_osc_sender_set_routes(s, targets, R, bad.data(), routes.secondary.data(), C) == FX_ERR_INVALID_ARGUMENT, "a primary index past the targets accepted");
    bad[C - 1] = -1;
    EXPECT(fx_osc_sender_set_routes(s, targets, R, bad.data(), nullptr, C) == FX_ERR_INVALID_ARGUMENT, "a negative primary index accepted");
    bad = routes.secondary;
    bad[5] = -2;
    EXPECT(fx_osc_sender_set_routes(s, targets, R, routes.primary.data(), bad.data(), C) == FX_ERR_INVALID_ARGUMENT, "a secondary index of -2 accepted");
    bad[5] = R;
    EXPECT(fx_osc_sender_set_routes(s, targets, R, routes.primary.data(), bad.data(), C) == FX_ERR_INVALID_ARGUMENT, "a secondary index past the targets accepted");
    const char* unparsable[R] = {targets[0], "not an address", targets[2]};
    EXPECT(fx_osc_sender_set_routes(s, unparsable, R, routes.primary.data(), routes.secondary.data(), C) == FX_ERR_INVALID_ARGUMENT, "an unparsable target accepted");
    const char* with_null[R] = {targets[0], nullptr, targets[2]};
    EXPECT(fx_osc_sender_set_routes(s, with_null, R, routes.primary.data(), routes.secondary.data(), C) == FX_ERR_INVALID_ARGUMENT, "a null target accepted");
    EXPECT(fx_osc_sender_set_routes(s, targets, 0, routes.primary.data(), nullptr, C) == FX_ERR_INVALID_ARGUMENT, "no targets accepted");
    EXPECT(fx_osc_sender_set_routes(s, targets, FX_OSC_SENDER_MAX_TARGETS + 1, routes.primary.data(), nullptr, C) == FX_ERR_INVALID_ARGUMENT, "65 targets accepted");
    EXPECT(fx_osc_sender_set_routes(s, targets, R, nullptr, nullptr, C) == FX_ERR_INVALID_ARGUMENT, "a null primary list accepted");
    EXPECT(fx_osc_sender_set_routes(s, targets, R, routes.primary.data(), routes.secondary.data(), C - 1) == FX_ERR_INVALID_ARGUMENT, "routes for another count than what is published accepted");
    EXPECT(fx_osc_sender_set_routes(nullptr, targets, R, routes.primary.data(), nullptr, C) == FX_ERR_INVALID_ARGUMENT, "a null sender accepted");
    EXPECT(fx_osc_sender_update(s, a.data.data(), a.stride, a.len.data(), C - 1) == FX_ERR_INVALID_ARGUMENT, "a publication of another count accepted while routes are set");
    EXPECT(tick(s) == per_tick, "threads %d gso %d: the tick after the refused calls", threads, (int) gso);
    for (int r = 0; r < R; r++) {
        const long long want = (long long) (k + 1) * routes.per_target[r];
        EXPECT(rcv.wait_for(r, want) == want, "threads %d gso %d: receiver %d after the refused calls", threads, (int) gso, r);
    }

    // other routes: the next tick follows them; a track whose two targets are one goes there twice
    std::vector<int> all1((size_t) C, 1);
    EXPECT(fx_osc_sender_set_routes(s, targets, R, all1.data(), all1.data(), C) == FX_OK, "set_routes: %s", fx_last_error());
    EXPECT(tick(s) == 2 * C, "primary == secondary: a tick did not send every message twice");
    EXPECT(rcv.wait_for(1, (long long) (k + 1) * routes.per_target[1] + 2 * C) == (long long) (k + 1) * routes.per_target[1] + 2 * C, "receiver 1 after every track was routed to it twice");
    EXPECT(rcv.datagrams(0) == (long long) (k + 1) * routes.per_target[0] && rcv.datagrams(2) == (long long) (k + 1) * routes.per_target[2], "receivers 0 and 2 got datagrams routed to 1");
    // NULL: back to the create-time target (the discard port: nobody listens there), and any count may be published again
    EXPECT(fx_osc_sender_set_routes(s, nullptr, 0, nullptr, nullptr, 0) == FX_OK, "dropping the routes: %s", fx_last_error());
    EXPECT(fx_osc_sender_update(s, a.data.data(), a.stride, a.len.data(), C - 1) == FX_OK, "update after the routes were dropped: %s", fx_last_error());
    (void) tick(s);
    EXPECT(rcv.datagrams(1) == (long long) (k + 1) * routes.per_target[1] + 2 * C, "a receiver got datagrams after the routes were dropped");
    fx_osc_sender_destroy(s);
}

// routes replaced (and dropped, and a new publication made) while the 60 Hz timer sends
void change_while_the_timer_runs(int threads, bool gso)
{
    Receivers rcv;
    const char* targets[R];
    rcv.targets3(targets);
    const RouteTable r0(0), r1(1);
    const Messages a(3u), b(4u);
    fx_osc_sender* s = nullptr;
    EXPECT(fx_osc_sender_create(&s, targets[0], nullptr, threads, gso ? FX_OSC_SENDER_GSO : 0u) == FX_OK, "create: %s", fx_last_error());
    if (!s) return;
    EXPECT(fx_osc_sender_update(s, a.data.data(), a.stride, a.len.data(), C) == FX_OK, "update: %s", fx_last_error());
    EXPECT(fx_osc_sender_start(s, 60.0) == FX_OK, "start: %s", fx_last_error());
    for (int round = 0; round < 24; round++) {
        const RouteTable& r = round % 2 ? r1 : r0;
        if (round % 6 == 5) EXPECT(fx_osc_sender_set_routes(s, nullptr, 0, nullptr, nullptr, 0) == FX_OK, "dropping the routes: %s", fx_last_error());
        else EXPECT(fx_osc_sender_set_routes(s, targets, R, r.primary.data(), round % 3 ? r.secondary.data() : nullptr, C) == FX_OK, "set_routes: %s", fx_last_error());
        const Messages& m = round % 2 ? b : a;
        EXPECT(fx_osc_sender_update(s, m.data.data(), m.stride, m.len.data(), C) == FX_OK, "update: %s", fx_last_error());
        (void) tick(s);                                         // a manual tick against the timer's
        std::this_thread::sleep_for(std::chrono::milliseconds(5));
    }
    EXPECT(fx_osc_sender_stop(s) == FX_OK, "stop");
    fx_osc_sender_stats st;
    EXPECT(fx_osc_sender_get_stats(s, &st) == FX_OK && st.dropped == 0 && st.ticks >= 24, "%lld ticks, %lld dropped", st.ticks, st.dropped);
    // every datagram the kernel accepted arrived at one of the three
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(2);
    long long got = 0;
    do { got = rcv.datagrams(0) + rcv.datagrams(1) + rcv.datagrams(2); if (got >= st.datagrams) break; std::this_thread::sleep_for(std::chrono::milliseconds(1)); } while (std::chrono::steady_clock::now() < deadline);
    EXPECT(got == st.datagrams, "threads %d gso %d: %lld datagrams sent while the routes changed, %lld received", threads, (int) gso, st.datagrams, got);
    fx_osc_sender_destroy(s);
}

// routes that send every track to the create-time target: the datagrams and system calls of a sender without routes, tick by tick
void same_cost_as_no_routes(int threads, bool gso)
{
    Receivers rcv;
    const char* targets[R];
    rcv.targets3(targets);
    const Messages a(5u);
    fx_osc_sender* plain = nullptr;
    fx_osc_sender* routed = nullptr;
    EXPECT(fx_osc_sender_create(&plain, targets[0], nullptr, threads, gso ? FX_OSC_SENDER_GSO : 0u) == FX_OK, "create: %s", fx_last_error());
    EXPECT(fx_osc_sender_create(&routed, targets[0], nullptr, threads, gso ? FX_OSC_SENDER_GSO : 0u) == FX_OK, "create: %s", fx_last_error());
    if (!plain || !routed) return;
    const std::vector<int> all0((size_t) C, 0);
    EXPECT(fx_osc_sender_set_routes(routed, targets, 1, all0.data(), nullptr, C) == FX_OK, "set_routes: %s", fx_last_error());
    fx_osc_sender_stats before[2] = {}, after[2] = {};
    fx_osc_sender* both[2] = {plain, routed};
    for (fx_osc_sender* s : both) EXPECT(fx_osc_sender_update(s, a.data.data(), a.stride, a.len.data(), C) == FX_OK, "update: %s", fx_last_error());
    for (int t = 0; t < 3; t++) {
        for (int i = 0; i < 2; i++) {
            fx_osc_sender_get_stats(both[i], &before[i]);
            EXPECT(tick(both[i]) == C, "a tick did not send %d datagrams", C);
            fx_osc_sender_get_stats(both[i], &after[i]);
        }
        EXPECT(after[0].datagrams - before[0].datagrams == after[1].datagrams - before[1].datagrams && after[0].syscalls - before[0].syscalls == after[1].syscalls - before[1].syscalls,
               "threads %d gso %d tick %d: without routes %lld datagrams in %lld system calls, with routes to the same target %lld in %lld", threads, (int) gso, t,
               after[0].datagrams - before[0].datagrams, after[0].syscalls - before[0].syscalls, after[1].datagrams - before[1].datagrams, after[1].syscalls - before[1].syscalls);
    }
    EXPECT(rcv.wait_for(0, 6 * C) == 6 * C, "the receiver of both senders");
    fx_osc_sender_destroy(plain);
    fx_osc_sender_destroy(routed);
}

} // namespace

int main()
{
    const int thread_counts[] = {1, 3, 4};
    for (int threads : thread_counts)
        for (int gso = 0; gso < 2; gso++) {
            scatter(threads, gso != 0);
            same_cost_as_no_routes(threads, gso != 0);
        }
    change_while_the_timer_runs(3, false);
    change_while_the_timer_runs(4, true);
    std::printf("%s: %d problems\n", problems ? "FAILED" : "ok", problems);
    return problems ? 1 : 0;
}
