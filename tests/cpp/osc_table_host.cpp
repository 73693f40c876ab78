// osc_table_host -- the word-forming function of fx_osc_table_kernel (csrc/fx_osc_words.h: fxk::osc_table_word, the very code every
// thread of the kernel runs) on the host, for every word of every track, against fx_osc_encode.  A stand-alone program: built by g++
// with -fsanitize=address,undefined from the shim's host units and tests/cpp/fake_hip (tests/test_osc_addresses_cpu.py), so an index
// past a table row, a latest vector or the tag words is an error here, where it can be seen, before the kernel runs on a device.
//
// The table is built as fx_set_osc_addresses builds it: zero-padded rows of FX_OSC_ROW_BYTES bytes and int len[C]; the launch shape is
// the kernel's: "thread" g = c * (stride / 4) + w writes word w of slot c.  Addresses: the set of tests/osc_address_cases.py (lengths
// 1 .. 124, every residue mod 4); values: noise with NaN, +-inf and -0.0, and NaN vectors (a context before its first frame).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "fx.h"
#include "fx_osc_words.h"

static int problems = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { problems++; std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const int kLengths[] = {1, 2, 3, 4, 5, 7, 8, 15, 16, 63, 64, 65, 123, 124};
static const char kFill[] = "Mixer/Drums/Kick_0123456789-ABCDEFGHIJKLMNOPQRSTUVWXYZ~!#";

static std::string address(int length, int track)
{
    std::string a = "/";
    const int fill = (int) sizeof kFill - 1;
    for (int k = 0; k < length - 1; k++) a += kFill[(track * 7 + k) % fill];
    return a;
}

int main()
{
    const int C = 71;                                           // five times through the lengths and one more: neighbours differ
    std::vector<std::string> addr;
    for (int c = 0; c < C; c++) addr.push_back(address(kLengths[c % 14], c));

    // the table as fx_set_osc_addresses uploads it (exactly C rows: a read past the last row is a read past the allocation)
    std::vector<unsigned> rows((size_t) C * fxk::FX_OSC_ROW_WORDS, 0u);
    std::vector<int> len((size_t) C);
    int longest = 0;
    for (int c = 0; c < C; c++) {
        int alen = -1;
        const char* fault = fxk::osc_address_fault(addr[(size_t) c].c_str(), &alen);
        EXPECT(fault == nullptr && alen == (int) addr[(size_t) c].size(), "track %d: a valid address refused (%s)", c, fault ? fault : "length");
        std::memcpy(reinterpret_cast<unsigned char*>(rows.data()) + (size_t) c * fxk::FX_OSC_ROW_BYTES, addr[(size_t) c].data(), (size_t) alen);
        len[(size_t) c] = alen;
        if (fxk::osc_addressed_bytes(alen) > longest) longest = fxk::osc_addressed_bytes(alen);
    }
    EXPECT(longest == 192, "the longest message is %d bytes", longest);

    long long words_checked = 0;
    for (int values = 0; values < 2; values++) {
        std::vector<float> latest((size_t) C * FX_NUM_FEATURES);
        unsigned seed = 12345u;
        for (float& x : latest) { seed = seed * 1664525u + 1013904223u; x = values == 0 ? (float) ((int) (seed >> 8) % 20001 - 10000) * 1e-3f : std::numeric_limits<float>::quiet_NaN(); }
        if (values == 0) {
            latest[FX_FLATNESS] = std::numeric_limits<float>::infinity();
            latest[(size_t) (C / 2) * FX_NUM_FEATURES + FX_F0] = std::numeric_limits<float>::quiet_NaN();
            latest[(size_t) (C - 1) * FX_NUM_FEATURES + FX_FLUX] = -std::numeric_limits<float>::infinity();
            latest[(size_t) (C - 1) * FX_NUM_FEATURES + FX_ONSET] = -0.0f;
        }
        for (int stride : {longest, longest + 12}) {
            std::vector<unsigned> out((size_t) C * (size_t) (stride / 4), 0xEEEEEEEEu);       // exactly C slots
            const int words = stride >> 2;
            for (long long g = 0; g < (long long) C * words; g++) {                          // the kernel's index arithmetic
                const int c = (int) (g / words), w = (int) (g - (long long) c * words);
                out[(size_t) c * (size_t) words + (size_t) w] =
                    fxk::osc_table_word(rows.data() + (size_t) c * fxk::FX_OSC_ROW_WORDS, len[(size_t) c], latest.data() + (size_t) c * FX_NUM_FEATURES, w);
                words_checked++;
            }
            for (int c = 0; c < C; c++) {
                unsigned char want[256];
                std::memset(want, 0, sizeof want);
                const int n = fx_osc_encode(addr[(size_t) c].c_str(), latest.data() + (size_t) c * FX_NUM_FEATURES, want, (int) sizeof want);
                EXPECT(n == fxk::osc_addressed_bytes(len[(size_t) c]) && n <= stride, "track %d: fx_osc_encode gives %d bytes", c, n);
                const unsigned char* got = reinterpret_cast<const unsigned char*>(out.data()) + (size_t) c * (size_t) stride;
                EXPECT(std::memcmp(got, want, (size_t) stride) == 0, "track %d (address of %d bytes), stride %d, values %d: the words are not fx_osc_encode's message and zeros", c,
                       len[(size_t) c], stride, values);
            }
        }
    }

    // the address rules, class by class
    int alen = 0;
    const std::string too_long = "/" + std::string(124, 'x');
    for (const char* bad : {"", "Audio/A", "/Audio A", "/Audio/\x7f", too_long.c_str(), "/Audio/\xe9", "/a\tb"})
        EXPECT(fxk::osc_address_fault(bad, &alen) != nullptr, "'%s' accepted", bad);
    EXPECT(fxk::osc_address_fault(nullptr, &alen) != nullptr, "a null address accepted");
    const std::string longest_ok = "/" + std::string(123, '~');
    EXPECT(fxk::osc_address_fault(longest_ok.c_str(), &alen) == nullptr && alen == 124, "124 bytes refused");
    EXPECT(fxk::osc_address_fault("/", &alen) == nullptr && alen == 1, "'/' refused");

    std::printf("words checked: %lld\n", words_checked);
    std::printf("%s: %d problems\n", problems ? "FAILED" : "ok", problems);
    return problems ? 1 : 0;
}
