// refdiff_buffer.cpp -- the live parts of the reference's offline analysis that end in a ConcatenatedFeatureBuffer (AudioAnalysis.h:129-251,
// AudioFeatures.h:14-314), compiled UNMODIFIED from where they lie under /root/reference/Source against tools/refdiff/juce_standin.h and run on
// given one-channel inputs, so that the offline driver's model (tests/offline_analyse_model.py) can be diffed against them.  Build container
// only (tools/refdiff/README.md); nothing of the reference is copied: the headers are #included by path at compile time.
//
//   refdiff_buffer <in.bin> <out.bin>
//   in : int32 op, samples, downsamples, window; then float32 audio[samples]
//   op 1 last frame : AudioAnalyser (window, 1 channel, harmonic analysis OFF, so no transform runs)::performSpectralAnalysis
//                     -> float32 fftIn[window]: the last frame's windowed input (frame indexing, zero padding, scaleBufferWithBartlettWindowing)
//   op 2 audio row  : ConcatenatedFeatureBuffer::fillDownsampledRMSAudioChannels -> float32 row[downsamples]; then normaliseAudioChannels
//                     -> float32 row[downsamples] again
#define DBG(x) do { } while (0)
#include "juce_standin.h"

#include <cstdint>
#include <cstdio>
#include <iostream>

#include "AudioFeatures.h"
#include "AudioAnalysis.h"

struct Header { int32_t op, samples, downsamples, window; };

int main (int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen (argv[1], "rb");
    if (! f) return 2;
    Header h;
    if (fread (&h, sizeof h, 1, f) != 1) return 2;
    std::vector<float> in ((size_t) h.samples);
    if (fread (in.data(), 4, in.size(), f) != in.size()) return 2;
    fclose (f);
    FILE* o = fopen (argv[2], "wb");
    if (! o) return 2;
    typedef ConcatenatedFeatureBuffer::Feature Feature;
    if (h.op == 1) {
        ConcatenatedFeatureBuffer features (1, h.samples, h.downsamples, h.window / 2 + 1, 0.0, 48000.0);
        features.audioOutput.copyFrom (0, 0, in.data(), h.samples);
        AudioAnalyser an (h.window, 1, 24000.0, true, false);
        an.performSpectralAnalysis (features);
        fwrite (an.fftIn.getReadPointer (0), 4, (size_t) h.window, o);
    } else if (h.op == 2) {
        ConcatenatedFeatureBuffer features (1, h.samples, h.downsamples, 0, 0.0, 48000.0);
        features.audioOutput.copyFrom (0, 0, in.data(), h.samples);
        features.fillDownsampledRMSAudioChannels();
        for (int i = 0; i < h.downsamples; i++) { const float v = features.getFeatureSample (Feature::Audio, 0, i); fwrite (&v, 4, 1, o); }
        features.normaliseAudioChannels();
        for (int i = 0; i < h.downsamples; i++) { const float v = features.getFeatureSample (Feature::Audio, 0, i); fwrite (&v, 4, 1, o); }
    } else return 2;
    fclose (o);
    return 0;
}
