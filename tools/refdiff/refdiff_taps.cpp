// refdiff_taps.cpp -- the reference's display buffers, read through its own getters: the hot-path headers compiled unmodified
// (included from where they lie under the reference's Source/, against juce_standin.h) single-step both analysers of one channel over a
// hop stream; before each chosen hop every display flag is armed, and after the step the buffers are read back.  What include/fx.h's
// fx_get_taps returns is pinned to these (tests/golden/taps/make_taps.py).  Build container only; see README.md.
//
//   refdiff_taps <in.bin> <out.bin>
//   in : int32 N, T, K; float32 gain; float64 sample_rate; int32 capture_hops[K] (ascending); float32 hops[T][N/2]
//   out: per capture, float32 window[N], spectrum[2N], pitch_spectrum[2N], autocorrelation[N], cnd[N], lag_position[2]
//   The two analysers' overlapped windows (getBufferToDraw) must be equal; the driver fails otherwise.
#include "juce_standin.h"

#include "AudioDataCollector.h"
#include "RealTimeAudioAnalysis.h"
#include "PitchAnalyser.h"
#include "SpectralCharacteristics.h"
#include "HarmonicCharacteristics.h"
#include "RealTimeAnalyser.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

struct Header { int32_t N, T, K; float gain; double sample_rate; };

static void feed (AudioDataCollector& c, const float* hop, int n)
{
    const float* in[1] = { hop };
    c.audioDeviceIOCallback (in, 1, nullptr, 0, n);
}

static void put (std::vector<float>& out, const AudioSampleBuffer& b, int n)
{
    const float* p = b.getReadPointer (0);
    out.insert (out.end(), p, p + n);
}

int main (int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen (argv[1], "rb");
    if (! f) return 2;
    Header h;
    if (fread (&h, sizeof h, 1, f) != 1) return 2;
    const int N = h.N, half = N / 2;
    std::vector<int32_t> at ((size_t) h.K);
    if (fread (at.data(), sizeof (int32_t), at.size(), f) != at.size()) return 2;
    std::vector<float> hops ((size_t) h.T * half);
    if (fread (hops.data(), sizeof (float), hops.size(), f) != hops.size()) return 2;
    fclose (f);

    // one AnalyserTrackController's analysis half (ref AnalyserTrackController.h:199-206)
    AudioDataCollector specCollector (0), harmCollector (0);
    specCollector.setExpectedSamplesPerBlock (half);
    harmCollector.setExpectedSamplesPerBlock (half);
    specCollector.setGain (h.gain);
    harmCollector.setGain (h.gain);
    AudioFeatures shared;
    RealTimeSpectralAnalyser spectral (specCollector, shared, N, h.sample_rate);
    RealTimeHarmonicAnalyser harmonic (harmCollector, shared, N, h.sample_rate);

    std::vector<float> out;
    size_t next = 0;
    for (int t = 0; t < h.T && next < at.size(); t++)
    {
        const bool capture = at[next] == t;
        if (capture)
        {
            spectral.getOverlapper().enableBufferToDrawNeedsUpdating();
            harmonic.getOverlapper().enableBufferToDrawNeedsUpdating();
            spectral.getFFTAnalyser().enableFFTBufferToDrawNeedsUpdating();
            harmonic.getFFTAnalyser().enableFFTBufferToDrawNeedsUpdating();
            harmonic.getPitchAnalyser().enableAutoCorrelationBufferToDrawNeedsUpdating();
            harmonic.getPitchAnalyser().enableCumulativeDifferenceBufferNeedsUpdating();
        }
        const float* hop = hops.data() + (size_t) t * half;
        feed (specCollector, hop, half);
        feed (harmCollector, hop, half);
        spectral.step();
        harmonic.step();
        if (! capture) continue;
        next++;
        const AudioSampleBuffer ws = spectral.getOverlapper().getBufferToDraw();
        const AudioSampleBuffer wh = harmonic.getOverlapper().getBufferToDraw();
        if (ws.getNumSamples() != N || wh.getNumSamples() != N
             || memcmp (ws.getReadPointer (0), wh.getReadPointer (0), sizeof (float) * (size_t) N) != 0)
        {
            fprintf (stderr, "hop %d: the two analysers' windows differ\n", t);
            return 3;
        }
        put (out, ws, N);
        put (out, spectral.getFFTAnalyser().getFFTBufferToDraw(), 2 * N);
        put (out, harmonic.getFFTAnalyser().getFFTBufferToDraw(), 2 * N);
        put (out, harmonic.getPitchAnalyser().getAutoCorrelationBufferToDraw(), N);
        put (out, harmonic.getPitchAnalyser().getCumulativeDifferenceBufferToDraw(), N);
        const Point<float> lag = harmonic.getPitchAnalyser().getNormalisedLagPosition();
        out.push_back (lag.getX());
        out.push_back (lag.getY());
    }
    if (next != at.size()) return 4;
    f = fopen (argv[2], "wb");
    if (! f) return 2;
    fwrite (out.data(), sizeof (float), out.size(), f);
    fclose (f);
    return 0;
}
