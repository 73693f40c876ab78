// rtp_packet_host.cpp -- the parser and the placement arithmetic of csrc/fx_rtp_packet.h on the host, under AddressSanitizer and
// UBSan (tests/test_rtp_cpu.py builds and runs it, and holds what it prints to tests/rtp_model.py).
//
// Every length 0 .. 96 of a few header patterns and of pseudo-random bytes, each datagram in a heap buffer of exactly its length:
// a read at or beyond the length is a heap-buffer-overflow the sanitizer reports (the reader does read whatever it is asked for).
// The reader also counts such indices itself; built with -DRTP_HOST_COUNT_ONLY it only counts them and touches nothing outside, which
// is how the test of a deliberately wrong parser runs it.
//   stdout, one line per case:   p <hex bytes or -> <frame bytes> <M | T h m>
//                                 q <T> <cursor> <m> <n> <d0> <lo> <hi> <bits>
//                                 <cases> datagrams, <n> reads outside
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../feature-extractor_amd/csrc/fx_rtp_packet.h"

static long long outside = 0;

struct Checked {
    const unsigned char* at;
    int                  len;
    unsigned operator()(int k) const
    {
        if (k < 0 || k >= len) {
            outside++;
#ifdef RTP_HOST_COUNT_ONLY
            return 0;
#endif
        }
        return at[k];
    }
};

static uint32_t lcg_state = 12345u;
static unsigned next_byte()
{
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 24;
}

struct Pattern {
    int first;          // b[0]; -1: as the generator gives it
    int ext_words;      // X patterns: the extension's length field; -1: as the generator gives it
    int pad;            // P patterns: the last byte; -1: as the generator gives it
};

int main()
{
    static const Pattern patterns[] = {
        {0x80, -1, -1}, {0x81, -1, -1}, {0x8F, -1, -1},                 // CC = 0 / 1 / 15
        {0x90, 0, -1},  {0x90, 3, -1},  {0x91, 3, -1},  {0x90, 0xFFFF, -1}, {0x90, -1, -1},     // extensions of 0 and 3 words, one that lies
        {0xA0, -1, 1},  {0xA0, -1, 2},  {0xA0, -1, 3},  {0xA0, -1, 0},  {0xA0, -1, 200}, {0xA0, -1, -1},    // padding 1 - 3, none, too much
        {0xB1, 3, 2},   {0xBF, 0, 1},                                   // all of it at once
        {0x40, -1, -1}, {0xC0, -1, -1}, {0x00, -1, -1},                 // not version 2
        {-1, -1, -1},   {-1, -1, -1},   {-1, -1, -1},                   // pseudo-random bytes
    };
    static const int frames[] = {2, 3, 6, 9, 24, 192};
    long long cases = 0;
    for (const Pattern& pt : patterns) {
        for (int len = 0; len <= 96; len++) {
            unsigned char* b = static_cast<unsigned char*>(malloc((size_t) len));       // exactly len bytes
            if (!b && len > 0) return 2;
            for (int k = 0; k < len; k++) b[k] = (unsigned char) next_byte();
            if (pt.first >= 0 && len > 0) b[0] = (unsigned char) pt.first;
            if (pt.ext_words >= 0 && len > 0) {
                const int h = 12 + 4 * (b[0] & 15);
                if (h + 2 < len) b[h + 2] = (unsigned char) (pt.ext_words >> 8);
                if (h + 3 < len) b[h + 3] = (unsigned char) (pt.ext_words & 255);
            }
            if (pt.pad >= 0 && len > 0) b[len - 1] = (unsigned char) pt.pad;
            const int F = frames[(len + (int) (&pt - patterns)) % 6];
            fx_rtp_parsed got;
            const bool ok = fx_rtp_parse(Checked{b, len}, len, F, &got);
            printf("p ");
            if (len == 0) printf("-");
            for (int k = 0; k < len; k++) printf("%02x", b[k]);
            if (ok) printf(" %d %u %d %d\n", F, got.timestamp, got.payload, got.sample_times);
            else printf(" %d M\n", F);
            free(b);
            cases++;
        }
    }
    static const uint32_t cursors[] = {0u, 1000u, 0x7FFFFFF0u, 0x80000000u, 0xFFFFFFC0u, 0xFFFFFFFFu};
    static const int offsets[] = {-70000, -65, -64, -1, 0, 1, 63, 199, 200, 201, 70000};
    static const int lengths[] = {1, 6, 48, 64, 65536};
    static const int ticks[] = {1, 63, 200};
    for (uint32_t cursor : cursors)
        for (int off : offsets)
            for (int m : lengths)
                for (int n : ticks) {
                    const uint32_t T = cursor + (uint32_t) off;
                    const fx_rtp_placement at = fx_rtp_place(T, cursor, m, n);
                    printf("q %u %u %d %d %d %d %d %u\n", T, cursor, m, n, at.d0, at.lo, at.hi, at.bits);
                }
    // the far side of the circle: 2^31 away is read as negative
    {
        const fx_rtp_placement at = fx_rtp_place(0x80000000u, 0u, 48, 200);
        printf("q %u %u %d %d %d %d %d %u\n", 0x80000000u, 0u, 48, 200, at.d0, at.lo, at.hi, at.bits);
    }
    printf("%lld datagrams, %lld reads outside\n", cases, outside);
    return outside == 0 ? 0 : 1;
}
