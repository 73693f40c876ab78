// The run split of the 1024-point batch frame kernel (csrc/fx_flux_runs.h) on the host: for every unit length n <= 600 and every
// wavefront count k <= 8 the runs cover the unit exactly, keep frame order and differ in length by at most one; the last wavefront
// with a run is the one whose flux image is the channel's state after the unit.  Also the compile-time check of the image's place.
#include <cstdio>
#include "../../feature-extractor_amd/csrc/fx_flux_runs.h"

static_assert(flux_run_begin(40, 8, 0) == 0 && flux_run_begin(40, 8, 8) == 40 && flux_run_begin(16, 8, 3) == 6 && flux_run_begin(8, 8, 5) == 5, "runs of 5, 2 and 1");
static_assert(flux_run_begin(13, 8, 5) == 10 && flux_run_begin(13, 8, 6) == 11, "13 frames on 8 wavefronts: five runs of 2, three of 1");
static_assert(FLUX_IMAGE_1024.fits(8720, 3072, 5632) && !FLUX_IMAGE_1024.fits(8720, 3072, 5648) && !FLUX_IMAGE_1024.fits(8688, 3072, 5632), "the image's place");

int main()
{
    int wrong = 0, cases = 0;
    for (int k = 1; k <= 8; k++)
        for (int n = 1; n <= 600; n++) {
            cases++;
            bool ok = flux_run_begin(n, k, 0) == 0 && flux_run_begin(n, k, k) == n;
            int shortest = n, longest = 0, last = 0;
            for (int s = 0; s < k; s++) {
                const int len = flux_run_begin(n, k, s + 1) - flux_run_begin(n, k, s);      // (begin of s + 1 == end of s: order and cover)
                if (len < 0) ok = false;
                if (len < shortest) shortest = len;
                if (len > longest) longest = len;
                if (len > 0) last = s;
                if (len > 0 && s > 0 && flux_run_begin(n, k, s) == flux_run_begin(n, k, s - 1)) ok = false;   // no run behind an empty one
            }
            if (longest - shortest > 1 || last != flux_last_slot(n, k)) ok = false;
            if (!ok) { wrong++; std::printf("n = %d, k = %d\n", n, k); }
        }
    std::printf("%d splits, %d wrong\n", cases, wrong);
    return wrong != 0;
}
