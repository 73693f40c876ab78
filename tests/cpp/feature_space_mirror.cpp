// feature_space_mirror.cpp -- fx::FeatureSpace (include/fx_realtime.hpp) on the inputs of tests/golden/offline/feature_stats.npz's fold
// cases, in the format of tools/refdiff/refdiff_stats.cpp's op 4 (ref AudioFeatures.h:319-349): no GPU involved.
//   feature_space_mirror <in.bin> <out.bin>
//   in : int32 n; float32 [n][7] = attack, centroid (start, end), slope (start, end), zero crosses (start, end)
//   out: float32 [n][8] = space 0's four (start, end) as constructed and after compareAndUpdateRanges with each later space
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fx_realtime.hpp"

static void put (FILE* o, const fx::FeatureSpace& s)
{
    const float v[8] = { s.attackRange.getStart(), s.attackRange.getEnd(), s.spectralCentroidRange.getStart(), s.spectralCentroidRange.getEnd(),
                         s.spectralSlopeRange.getStart(), s.spectralSlopeRange.getEnd(), s.zeroCrossesRange.getStart(), s.zeroCrossesRange.getEnd() };
    fwrite (v, 4, 8, o);
}

int main (int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen (argv[1], "rb");
    if (! f) return 2;
    int32_t n = 0;
    if (fread (&n, 4, 1, f) != 1 || n < 1) return 2;
    std::vector<float> in ((std::size_t) n * 7);
    if (fread (in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose (f);
    FILE* o = fopen (argv[2], "wb");
    if (! o) return 2;
    // the same spaces through fromRanges: ranges [FX_OFFLINE_ZERO_CROSSES + 1][n][2] with space s as channel s
    std::vector<float> ranges ((std::size_t) (FX_OFFLINE_ZERO_CROSSES + 1) * n * 2, 0.0f), attack ((std::size_t) n);
    const int rows[3] = { FX_OFFLINE_CENTROID, FX_OFFLINE_SLOPE, FX_OFFLINE_ZERO_CROSSES };
    for (int s = 0; s < n; s++) {
        attack[(std::size_t) s] = in[(std::size_t) s * 7];
        for (int k = 0; k < 3; k++)
            for (int e = 0; e < 2; e++) ranges[((std::size_t) rows[k] * n + s) * 2 + e] = in[(std::size_t) s * 7 + 1 + 2 * k + e];
    }
    const float* p = in.data();
    fx::FeatureSpace existing (p[0], fx::Range (p[1], p[2]), fx::Range (p[3], p[4]), fx::Range (p[5], p[6]));
    fx::FeatureSpace twin = fx::FeatureSpace::fromRanges (ranges.data(), attack.data(), n, 0);
    put (o, existing);
    for (int s = 1; s < n; s++) {
        p = in.data() + (std::size_t) s * 7;
        fx::FeatureSpace next (p[0], fx::Range (p[1], p[2]), fx::Range (p[3], p[4]), fx::Range (p[5], p[6]));
        fx::FeatureSpace::compareAndUpdateRanges (existing.attackRange, next.attackRange);
        fx::FeatureSpace::compareAndUpdateRanges (existing.spectralCentroidRange, next.spectralCentroidRange);
        fx::FeatureSpace::compareAndUpdateRanges (existing.spectralSlopeRange, next.spectralSlopeRange);
        fx::FeatureSpace::compareAndUpdateRanges (existing.zeroCrossesRange, next.zeroCrossesRange);
        put (o, existing);
        fx::FeatureSpace other = fx::FeatureSpace::fromRanges (ranges.data(), attack.data(), n, s);
        fx::FeatureSpace::compareAndUpdateRanges (twin.attackRange, other.attackRange);
        fx::FeatureSpace::compareAndUpdateRanges (twin.spectralCentroidRange, other.spectralCentroidRange);
        fx::FeatureSpace::compareAndUpdateRanges (twin.spectralSlopeRange, other.spectralSlopeRange);
        fx::FeatureSpace::compareAndUpdateRanges (twin.zeroCrossesRange, other.zeroCrossesRange);
    }
    put (o, twin);                                        // (row n: the fromRanges route's last fold)
    fclose (o);
    fx::FeatureSpace empty;
    if (empty.attackRange.getStart() != 0.0f || empty.zeroCrossesRange.getEnd() != 0.0f) return 3;
    std::printf ("feature_space_mirror: ok\n");
    return 0;
}
