// osc_bundles_host -- OSC bundles on the host, in a stand-alone program built twice by tests/test_osc_bundles_cpp.py (with
// -fsanitize=address,undefined and with -fsanitize=thread) from the shim's host units and tests/cpp/fake_hip:
//   * osc_bundle_word (csrc/fx_osc_words.h), the function fx_osc_bundle_kernel runs per output word, run here for whole bundles
//     through the host encoders and compared with bundles put together from fx_osc_encode messages (ref OSCFeatureAnalysisOutput.h:107)
//     by this file's own few lines;
//   * fx::OSCBatchSender::setBundling publishing while the 60 Hz timer sends, into a receiver made with FX_OSC_RECEIVER_BUNDLES;
//   * that receiver's bundle parser fed hostile datagrams over a real socket.
#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fx.h"
#include "fx_realtime.hpp"
#include "fx_osc_words.h"

static int problems = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { problems++; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

namespace {

const unsigned long long kTag = 0xE9B1C2D340000001ull;

std::vector<float> vectors(int n, unsigned seed)
{
    std::vector<float> v((size_t) n * FX_NUM_FEATURES);
    for (float& x : v) { seed = seed * 1664525u + 1013904223u; x = (float) ((int) (seed >> 8) % 20001 - 10000) * 1e-3f; }
    const unsigned special[] = {0x7F800000u, 0xFF800000u, 0x7FC12345u, 0xFFA00001u, 0x80000000u, 0x00000001u, 0x807FFFFFu};   // inf, NaNs, -0.0, denormals
    for (size_t k = 0; k < sizeof special / sizeof special[0]; k++) std::memcpy(&v[(k * 5) % v.size()], &special[k], 4);
    return v;
}

void put_be32(std::vector<unsigned char>& d, unsigned v) { for (int s = 24; s >= 0; s -= 8) d.push_back((unsigned char) (v >> s)); }

// the bundles of these addresses, put together from fx_osc_encode's messages
std::vector<std::vector<unsigned char>> expected(const std::vector<std::string>& addresses, const std::vector<float>& v, int max_bytes, int* K_out)
{
    int longest = 0;
    std::vector<std::vector<unsigned char>> messages;
    for (size_t c = 0; c < addresses.size(); c++) {
        unsigned char m[256];
        const int n = fx_osc_encode(addresses[c].c_str(), v.data() + c * FX_NUM_FEATURES, m, (int) sizeof m);
        messages.emplace_back(m, m + (n > 0 ? n : 0));
        if (n > longest) longest = n;
    }
    int K = (max_bytes - 16) / (4 + longest);
    if (K > (int) addresses.size()) K = (int) addresses.size();
    if (K > 1024) K = 1024;
    *K_out = K;
    std::vector<std::vector<unsigned char>> out;
    for (size_t at = 0; K > 0 && at < messages.size(); at += (size_t) K) {
        std::vector<unsigned char> d = {'#', 'b', 'u', 'n', 'd', 'l', 'e', 0};
        put_be32(d, (unsigned) (kTag >> 32));
        put_be32(d, (unsigned) kTag);
        for (size_t c = at; c < messages.size() && c < at + (size_t) K; c++) { put_be32(d, (unsigned) messages[c].size()); d.insert(d.end(), messages[c].begin(), messages[c].end()); }
        out.push_back(d);
    }
    return out;
}

void compare(const char* what, int n, int max_bytes, const std::vector<std::vector<unsigned char>>& want, int K, int bundles, const std::vector<unsigned char>& out, int stride,
             const std::vector<int>& lengths)
{
    EXPECT(bundles == (int) want.size(), "%s n %d max %d: %d bundles, not %d", what, n, max_bytes, bundles, (int) want.size());
    if (bundles != (int) want.size()) return;
    for (int b = 0; b < bundles; b++) {
        const unsigned char* slot = out.data() + (size_t) b * (size_t) stride;
        const bool same = lengths[(size_t) b] == (int) want[(size_t) b].size() && std::memcmp(slot, want[(size_t) b].data(), want[(size_t) b].size()) == 0;
        EXPECT(same, "%s n %d max %d K %d: bundle %d differs (length %d, expected %d)", what, n, max_bytes, K, b, lengths[(size_t) b], (int) want[(size_t) b].size());
        bool zeros = true;
        for (int k = lengths[(size_t) b]; k < stride; k++) zeros = zeros && slot[k] == 0;
        EXPECT(zeros, "%s n %d max %d: the remainder of slot %d is not zeros", what, n, max_bytes, b);
    }
    EXPECT(out[(size_t) bundles * (size_t) stride] == 0xA5, "%s n %d max %d: a byte past the last slot was written", what, n, max_bytes);
}

void prefix_case(const char* prefix, int first, int n, int max_bytes)
{
    const std::vector<float> v = vectors(n, (unsigned) (first + n));
    std::vector<std::string> addresses;
    for (int c = 0; c < n; c++) addresses.push_back(std::string(prefix) + std::to_string(first + c));
    int K = 0;
    const auto want = expected(addresses, v, max_bytes, &K);
    int planK = 0, bundles = 0, stride = 0;
    const fx_status st = fx_osc_bundle_plan(fx_osc_message_bytes(prefix, first + n - 1), n, max_bytes, &planK, &bundles, &stride);
    if (K < 1) { EXPECT(st == FX_ERR_INVALID_ARGUMENT, "%s %d n %d max %d: a plan without room for one message", prefix, first, n, max_bytes); return; }
    EXPECT(st == FX_OK && planK == K, "%s %d n %d max %d: plan K %d, expected %d", prefix, first, n, max_bytes, planK, K);
    if (st != FX_OK) return;
    std::vector<unsigned char> out((size_t) bundles * (size_t) stride + 1, 0xA5);
    std::vector<int> lengths((size_t) bundles, -1);
    const int made = fx_osc_encode_bundles(prefix, first, n, v.data(), kTag, max_bytes, out.data(), stride, lengths.data());
    compare(prefix, n, max_bytes, want, K, made, out, stride, lengths);
}

std::string address_of(int length, int track)
{
    static const char fill[] = "Mixer/Drums/Kick_0123456789-ABCDEFGHIJKLMNOPQRSTUVWXYZ~!#";
    std::string a = "/";
    for (int k = 0; k < length - 1; k++) a += fill[(size_t) (track * 7 + k) % (sizeof fill - 1)];
    return a;
}

void addressed_case(bool extremes, int n, int max_bytes)
{
    const std::vector<float> v = vectors(n, (unsigned) (1000 + n));
    std::vector<std::string> addresses;
    for (int c = 0; c < n; c++) addresses.push_back(address_of(extremes ? (c % 2 ? 124 : 1) : 1 + c % 8, c));
    std::vector<const char*> list;
    int longest = 0;
    for (const std::string& a : addresses) { list.push_back(a.c_str()); const int m = (((int) a.size() + 4) & ~3) + 64; if (m > longest) longest = m; }
    int K = 0;
    const auto want = expected(addresses, v, max_bytes, &K);
    int planK = 0, bundles = 0, stride = 0;
    const fx_status st = fx_osc_bundle_plan(longest, n, max_bytes, &planK, &bundles, &stride);
    if (K < 1) { EXPECT(st == FX_ERR_INVALID_ARGUMENT, "addressed n %d max %d: a plan without room for one message", n, max_bytes); return; }
    EXPECT(st == FX_OK && planK == K, "addressed n %d max %d: plan K %d, expected %d", n, max_bytes, planK, K);
    if (st != FX_OK) return;
    std::vector<unsigned char> out((size_t) bundles * (size_t) stride + 1, 0xA5);
    std::vector<int> lengths((size_t) bundles, -1);
    const int made = fx_osc_encode_bundles_addressed(list.data(), n, v.data(), kTag, max_bytes, out.data(), stride, lengths.data());
    compare(extremes ? "addresses 1/124" : "addresses 1..8", n, max_bytes, want, K, made, out, stride, lengths);
}

void word_function()
{
    const int sizes[] = {96, 176, 212, 408, 1472, 5216, 20576, 65507};
    for (int max_bytes : sizes) {
        const int K = (max_bytes - 16) / 80 > 1024 ? 1024 : (max_bytes - 16) / 80;
        const int counts[] = {1, K - 1, K, K + 1, 2 * K + 1};
        for (int n : counts) {
            if (n < 1) continue;
            prefix_case("/Audio/A", 0, n, max_bytes);
            prefix_case("/Audio/A", 95, n, max_bytes);
            prefix_case("/Audio/A", 9999990, n, max_bytes);
            addressed_case(false, n, max_bytes);
            addressed_case(true, n, max_bytes);
        }
        prefix_case("/Aud/A", 5, 12, max_bytes);
    }
    // the word function itself, past a bundle's end and with a single element
    fxk::OscBundleParams p = {};
    const std::vector<float> v = vectors(1, 3u);
    p.latest = v.data();
    p.C = 1; p.K = 1; p.stride = 96;
    p.timetag_hi = 1u; p.timetag_lo = 2u;
    p.prefix_len = 8;
    std::memcpy(p.prefix, "/Audio/A", 8);
    const int off[2] = {fxk::FX_OSC_BUNDLE_HEADER_WORDS, fxk::FX_OSC_BUNDLE_HEADER_WORDS + 1 + fxk::osc_bundle_element_words(p, 0)};
    EXPECT(off[1] == 24, "one 76-byte message: %d words", off[1]);
    EXPECT(fxk::osc_bundle_word(p, 0, off, 1, 2) == 0x01000000u && fxk::osc_bundle_word(p, 0, off, 1, 3) == 0x02000000u, "time tag words");
    EXPECT(fxk::osc_bundle_word(p, 0, off, 1, 4) == 0x4C000000u, "size word");
    EXPECT(fxk::osc_bundle_word(p, 0, off, 1, 24) == 0u && fxk::osc_bundle_word(p, 0, off, 1, 1000) == 0u, "words past the bundle");
}

long long wait_for(fx_osc_receiver* rx, long long want_elements)
{
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(3);
    long long n = 0;
    do { fx_osc_receiver_get_bundle_stats(rx, nullptr, &n, nullptr); if (n >= want_elements) break; std::this_thread::sleep_for(std::chrono::milliseconds(1)); } while (std::chrono::steady_clock::now() < deadline);
    return n;
}

// setBundling publishing from this thread while the 60 Hz timer sends from the sender's
void batch_sender(int threads)
{
    constexpr int C = 700;
    fx_osc_receiver* rx = nullptr;
    EXPECT(fx_osc_receiver_create(&rx, "127.0.0.1:0", 2, "/Audio/A", C, FX_OSC_RECEIVER_BUNDLES) == FX_OK, "receiver: %s", fx_last_error());
    if (!rx) return;
    try {
        fx::OSCBatchSender sender("127.0.0.1:" + std::to_string(fx_osc_receiver_port(rx)), "", threads, false);
        sender.setBundling(1472, true);
        const std::vector<float> a = vectors(C, 7u), b = vectors(C, 8u);
        sender.updateFeatures("/Audio/A", 0, a.data(), C);
        int perBundle = 0, bundles = 0;
        EXPECT(fx_osc_bundle_plan(76, C, 1472, &perBundle, &bundles, nullptr) == FX_OK && perBundle == 18 && bundles == 39, "plan");
        EXPECT(sender.sendNow() == bundles, "a tick did not send %d datagrams", bundles);
        sender.startTimerHz(60);
        for (int round = 0; round < 20; round++) {
            if (round == 10) sender.setBundling(1472, false);
            sender.updateFeatures("/Audio/A", 0, (round % 2 ? a : b).data(), C);
            (void) sender.sendNow();
            std::this_thread::sleep_for(std::chrono::milliseconds(4));
        }
        sender.stopTimer();
        sender.updateFeatures("/Audio/A", 0, b.data(), C);          // the last word: time tag "immediately"
        EXPECT(sender.sendNow() == bundles, "the last tick");
        const fx_osc_sender_stats st = sender.getStats();
        EXPECT(st.dropped == 0 && st.datagrams % bundles == 0, "%lld datagrams, %lld dropped", st.datagrams, st.dropped);
        const long long want = st.datagrams / bundles * C;
        EXPECT(wait_for(rx, want) == want, "the receiver has %lld elements, not %lld", wait_for(rx, want), want);
        long long datagrams = 0, bad = 0, seen = 0;
        unsigned long long tag = 0;
        fx_osc_receiver_get_stats(rx, &datagrams, nullptr, &bad);
        fx_osc_receiver_get_bundle_stats(rx, &seen, nullptr, &tag);
        EXPECT(datagrams == st.datagrams && seen == st.datagrams && bad == 0, "%lld datagrams received (%lld bundles, %lld malformed), %lld sent", datagrams, seen, bad, st.datagrams);
        EXPECT(tag == FX_OSC_TIMETAG_IMMEDIATE, "the newest time tag is %llx", tag);
        for (int c : {0, 17, 18, C - 1}) {
            unsigned char last[160], want_m[160];
            int n = -1;
            const int m = fx_osc_encode(("/Audio/A" + std::to_string(c)).c_str(), b.data() + (size_t) c * FX_NUM_FEATURES, want_m, (int) sizeof want_m);
            EXPECT(fx_osc_receiver_last(rx, c, last, (int) sizeof last, &n) == FX_OK && n == m && std::memcmp(last, want_m, (size_t) m) == 0, "track %d's newest message", c);
        }
        // bundling off again: one message per datagram, as before
        sender.setBundling(0, false);
        sender.updateFeatures("/Audio/A", 0, a.data(), C);
        EXPECT(sender.sendNow() == C, "bundling off: a tick of %d datagrams", C);
        bool refused = false;
        try { sender.setBundling(65508, false); } catch (const fx::Error&) { refused = true; }
        EXPECT(refused, "bundles of 65508 bytes accepted");
    } catch (const std::exception& e) { EXPECT(false, "exception: %s", e.what()); }
    fx_osc_receiver_destroy(rx);
}

std::vector<unsigned char> whole_bundle(int elements, unsigned seed)
{
    const std::vector<float> v = vectors(elements, seed);
    std::vector<unsigned char> d = {'#', 'b', 'u', 'n', 'd', 'l', 'e', 0, 0, 0, 0, 0, 0, 0, 0, 1};
    for (int c = 0; c < elements; c++) {
        unsigned char m[160];
        const int n = fx_osc_encode(("/Audio/A" + std::to_string(c)).c_str(), v.data() + (size_t) c * FX_NUM_FEATURES, m, (int) sizeof m);
        put_be32(d, (unsigned) n);
        d.insert(d.end(), m, m + n);
    }
    return d;
}

void hostile_datagrams()
{
    fx_osc_receiver* rx = nullptr;
    EXPECT(fx_osc_receiver_create(&rx, "127.0.0.1:0", 1, "/Audio/A", 8, FX_OSC_RECEIVER_BUNDLES | FX_OSC_RECEIVER_NO_GRO) == FX_OK, "receiver: %s", fx_last_error());
    if (!rx) return;
    const int fd = socket(AF_INET, SOCK_DGRAM, 0);
    sockaddr_in to = sockaddr_in();
    to.sin_family = AF_INET;
    to.sin_port = htons((unsigned short) fx_osc_receiver_port(rx));
    inet_pton(AF_INET, "127.0.0.1", &to.sin_addr);
    EXPECT(fd >= 0 && connect(fd, reinterpret_cast<const sockaddr*>(&to), sizeof to) == 0, "socket");
    const std::vector<unsigned char> kept = whole_bundle(3, 5u), good = whole_bundle(3, 6u);     // (the hostile ones are made of `good`, with other values than `kept`)
    std::vector<std::vector<unsigned char>> bad;
    bad.emplace_back(good.begin(), good.begin() + 12);                                  // truncated header
    bad.emplace_back(good.begin(), good.begin() + 16);                                  // empty
    { auto d = good; d[16] = d[17] = d[18] = 0xFF; d[19] = 0xFC; bad.push_back(d); }    // size -4
    { auto d = good; d[16] = d[17] = d[18] = 0; d[19] = 2; bad.push_back(d); }          // size 2
    { auto d = good; d[16 + 80 + 3] = 200; bad.push_back(d); }                          // the second size runs past the end
    bad.emplace_back(good.begin(), good.end() - 4);                                     // the last element cut short
    { std::vector<unsigned char> d(good.begin(), good.begin() + 16); put_be32(d, (unsigned) good.size()); d.insert(d.end(), good.begin(), good.end()); bad.push_back(d); }   // nested
    { auto d = good; d[20] = 'A'; bad.push_back(d); }                                   // an element that is no feature message
    { std::vector<unsigned char> d(65507, 0); std::memcpy(d.data(), "#bundle", 8); bad.push_back(d); }
    { std::vector<unsigned char> d(65504, 0); std::memcpy(d.data(), "#bundle", 8); bad.push_back(d); }
    long long sent = 1;
    EXPECT(send(fd, kept.data(), kept.size(), 0) == (ssize_t) kept.size(), "send");
    for (const auto& d : bad) { EXPECT(send(fd, d.data(), d.size(), 0) == (ssize_t) d.size(), "send of %zu bytes", d.size()); sent++; }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(3);
    long long datagrams = 0, malformed = 0, bundles = 0, elements = 0;
    do { fx_osc_receiver_get_stats(rx, &datagrams, nullptr, &malformed); if (datagrams >= sent) break; std::this_thread::sleep_for(std::chrono::milliseconds(1)); } while (std::chrono::steady_clock::now() < deadline);
    fx_osc_receiver_get_bundle_stats(rx, &bundles, &elements, nullptr);
    EXPECT(datagrams == sent && malformed == sent - 1, "%lld datagrams, %lld malformed (sent %lld, one of them good)", datagrams, malformed, sent);
    EXPECT(bundles == 1 && elements == 3, "%lld bundles, %lld elements", bundles, elements);
    for (int c = 0; c < 8; c++) {                               // nothing of a bad bundle was kept: tracks 0 .. 2 still hold the first bundle's messages
        unsigned char last[160];
        int n = -1;
        EXPECT(fx_osc_receiver_last(rx, c, last, (int) sizeof last, &n) == FX_OK && n == (c < 3 ? 76 : 0), "track %d holds %d bytes", c, n);
        if (c < 3 && n == 76) EXPECT(std::memcmp(last, kept.data() + 16 + c * 80 + 4, 76) == 0, "track %d's message", c);
    }
    close(fd);
    fx_osc_receiver_destroy(rx);
}

} // namespace

int main()
{
    word_function();
    batch_sender(1);
    batch_sender(3);
    hostile_datagrams();
    std::printf("%s: %d problems\n", problems ? "FAILED" : "ok", problems);
    return problems ? 1 : 0;
}
