// refdiff_stats.cpp -- what the reference derives from a ConcatenatedFeatureBuffer (AudioFeatures.h:208-240, :319-349, :356-421), compiled
// UNMODIFIED from where it lies under /root/reference/Source against tools/refdiff/juce_standin.h and run on given one-channel inputs, so that
// the model of fx_offline_feature_ranges / _distribution / _smooth_rows and of fx::FeatureSpace (tests/offline_stats_model.py) can be diffed
// against it.  Build container only (tools/refdiff/README.md); nothing of the reference is copied: the header is #included by path at
// compile time.
//
//   refdiff_stats <in.bin> <out.bin>
//   in : int32 op, a, b, c; then float32 payload
//   op 1 range        : a = downsamples; payload row[a] -> getFeatureRange: float32 start, end
//   op 2 distribution : a = downsamples, b = brackets; payload row[a] (no NaN: std::sort) -> getDiscreteFeatureDistribution: float32 [b]
//   op 3 smoothing    : a = depth, b = updates; payload new[b][9] -> SmoothedFeatures (a), then per update (a one-sample buffer holding new[u])
//                       updateValues: float32 currentFeatureValues[9]; at the end float32 featureHistory[9][a]
//   op 4 feature space: a = spaces; payload [a][7] = attack, centroid (start, end), slope (start, end), zero crosses (start, end) ->
//                       FeatureSpace (attack, Range (..), Range (..), Range (..)) of each; space 0 is the existing one, every later one is folded
//                       into it by compareAndUpdateRanges on the four ranges: float32 [a][8] = the existing space's four (start, end) as
//                       constructed (space 0) and after each fold
#define DBG(x) do { } while (0)
#include "juce_standin.h"

#include <cstdint>
#include <cstdio>
#include <iostream>

#include "AudioFeatures.h"

struct Header { int32_t op, a, b, c; };

static void put (FILE* o, float v) { fwrite (&v, 4, 1, o); }
static void put (FILE* o, FeatureSpace& s)
{
    put (o, s.attackRange.getStart()); put (o, s.attackRange.getEnd());
    put (o, s.spectralCentroidRange.getStart()); put (o, s.spectralCentroidRange.getEnd());
    put (o, s.spectralSlopeRange.getStart()); put (o, s.spectralSlopeRange.getEnd());
    put (o, s.zeroCrossesRange.getStart()); put (o, s.zeroCrossesRange.getEnd());
}

int main (int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen (argv[1], "rb");
    if (! f) return 2;
    Header h;
    if (fread (&h, sizeof h, 1, f) != 1) return 2;
    const size_t n = h.op == 3 ? (size_t) h.b * 9 : (h.op == 4 ? (size_t) h.a * 7 : (size_t) h.a);
    std::vector<float> in (n);
    if (fread (in.data(), 4, n, f) != n) return 2;
    fclose (f);
    FILE* o = fopen (argv[2], "wb");
    if (! o) return 2;
    typedef ConcatenatedFeatureBuffer::Feature Feature;
    if (h.op == 1 || h.op == 2) {
        ConcatenatedFeatureBuffer features (1, h.a, h.a, 0, 0.0, 48000.0);
        features.setFeatureArray (Feature::Centroid, in.data(), 0);
        if (h.op == 1) {
            const Range<float> r = features.getFeatureRange (Feature::Centroid);
            put (o, r.getStart()); put (o, r.getEnd());
        } else {
            const std::vector<float> d = features.getDiscreteFeatureDistribution (Feature::Centroid, h.b);
            if ((int) d.size() != h.b) return 3;
            for (float v : d) put (o, v);
        }
    } else if (h.op == 3) {
        SmoothedFeatures smoothed (h.a);
        for (int u = 0; u < h.b; u++) {
            ConcatenatedFeatureBuffer features (1, 1, 1, 0, 0.0, 48000.0);
            for (int i = 0; i < 9; i++) features.setFeatureSample ((Feature) i, 0, in[(size_t) u * 9 + i], 0);
            smoothed.updateValues (features);
            if (smoothed.currentFeatureValues.size() != 9) return 3;
            for (float v : smoothed.currentFeatureValues) put (o, v);
        }
        for (int i = 0; i < 9; i++) for (int k = 0; k < h.a; k++) put (o, smoothed.featureHistory[(size_t) i][(size_t) k]);
    } else if (h.op == 4) {
        const float* p = in.data();
        FeatureSpace existing (p[0], Range<float> (p[1], p[2]), Range<float> (p[3], p[4]), Range<float> (p[5], p[6]));
        put (o, existing);
        for (int s = 1; s < h.a; s++) {
            p = in.data() + (size_t) s * 7;
            FeatureSpace next (p[0], Range<float> (p[1], p[2]), Range<float> (p[3], p[4]), Range<float> (p[5], p[6]));
            FeatureSpace::compareAndUpdateRanges (existing.attackRange, next.attackRange);
            FeatureSpace::compareAndUpdateRanges (existing.spectralCentroidRange, next.spectralCentroidRange);
            FeatureSpace::compareAndUpdateRanges (existing.spectralSlopeRange, next.spectralSlopeRange);
            FeatureSpace::compareAndUpdateRanges (existing.zeroCrossesRange, next.zeroCrossesRange);
            put (o, existing);
        }
    } else return 2;
    fclose (o);
    return 0;
}
