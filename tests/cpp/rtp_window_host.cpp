// rtp_window_host.cpp -- fx_rtp_place_span of csrc/fx_rtp_packet.h on the host, under AddressSanitizer and UBSan
// (tests/test_rtp_window_cpu.py builds and runs it, and holds what it prints to tests/rtp_window_model.py).
//   stdin, one case per line:    <T> <cursor> <m> <n> <W>
//   stdout, one line per case:   s <T> <cursor> <m> <n> <W> <d0> <lo> <hi> <bits>
//                                 <cases> cases
// With W == 0 the line also carries fx_rtp_place's answer for the same packet, which must be the same:
//                                 s ... <bits> = <d0> <lo> <hi> <bits>
#include <stdio.h>

#include "../../feature-extractor_amd/csrc/fx_rtp_packet.h"

int main()
{
    unsigned T, cursor;
    int m, n, W;
    long long cases = 0;
    while (scanf("%u %u %d %d %d", &T, &cursor, &m, &n, &W) == 5) {
        const fx_rtp_span_placement at = fx_rtp_place_span(T, cursor, m, n, W);
        printf("s %u %u %d %d %d %d %lld %lld %u", T, cursor, m, n, W, at.d0, at.lo, at.hi, at.bits);
        if (W == 0) {
            const fx_rtp_placement old = fx_rtp_place(T, cursor, m, n);
            printf(" = %d %d %d %u", old.d0, old.lo, old.hi, old.bits);
        }
        printf("\n");
        cases++;
    }
    printf("%lld cases\n", cases);
    return 0;
}
