// clip_rates_mirror -- fx::AudioFilePlayer::createClips with the files' own sample rates and setClipRates (include/fx_realtime.hpp),
// compiled with g++ against libfx_hip.so.
//
// Two analysers: one plays 16-bit files of 44.1, 96 and 22.05 kHz in a 48 kHz context on the GPU (pushSources), the other is given, by
// pushBlock, the fp32 planar block a host model makes of the same tick.  The model is the resampler's specification (include/fx.h,
// "CLIPS AT THEIR OWN RATE") as a loop over taps, with the table read from the library (fx_get_resampler_table); it is compiled
// without contraction, so every operation is the stated IEEE one.  Frame counts, raw and smoothed vectors must be the same bits and
// the transport the library reports must be the model's.  Needs a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fx_realtime.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf ("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool sameBits (const float* a, const float* b, std::size_t n) { return n == 0 || std::memcmp (a, b, n * sizeof (float)) == 0; }

static std::vector<float> table;
static int Z = 0, P = 0;

struct ModelTrack
{
    bool loop = true, rated = false;
    int state = FX_TRANSPORT_NO_FILE, taps = 0;
    std::vector<float> clip;                                        // widened: v / 2^15
    long long position = 0, laps = 0, k = 0;
    double r = 1.0, rho = 1.0;

    void load (const std::vector<std::int16_t>& samples, double clipRate, double contextRate, bool looping)
    {
        clip.clear();
        for (std::int16_t v : samples) clip.push_back ((float) (int) v * (1.0f / 32768.0f));
        loop = looping; state = FX_TRANSPORT_STOPPED; position = laps = k = 0;
        rated = clipRate != 0.0 && clipRate != contextRate;
        r = rated ? clipRate / contextRate : 1.0;
        const double inverse = 1.0 / r;
        rho = inverse < 1.0 ? inverse : 1.0;
        taps = (int) std::ceil ((double) Z / rho);
    }
    float sample (long long kk) const                                // output kk of a rated track
    {
        const long long L = (long long) clip.size();
        const double x = (double) kk * r;
        const double whole = std::floor (x);
        const double f = x - whole;
        const long long i0 = (long long) whole;
        float acc = 0.0f;
        for (int j = -(taps - 1); j <= taps; ++j)
        {
            const double a = std::fabs ((double) j - f) * rho;
            if (a >= (double) Z) continue;
            const double q = a * (double) P;
            const double qi = std::floor (q);
            const float t = (float) (q - qi);
            const std::size_t i = (std::size_t) qi;
            const float d = table[i + 1] - table[i];
            const float td = t * d;
            const float c = table[i] + td;
            const long long m = i0 + j;
            float s;
            if (loop) s = clip[(std::size_t) (((m % L) + L) % L)];
            else if (m >= 0 && m < L) s = clip[(std::size_t) m];
            else continue;
            const float cs = c * s;
            acc = acc + cs;
        }
        const float out = acc * (float) rho;
        return (! loop && x >= (double) L) ? 0.0f : out;
    }
    void render (float* out, int n)
    {
        for (int i = 0; i < n; ++i) out[i] = 0.0f;
        if (state != FX_TRANSPORT_PLAYING) return;
        const long long L = (long long) clip.size();
        for (int i = 0; i < n; ++i) out[i] = sample (k + i);
        k += n;
        const double x = (double) k * r;
        const long long whole = (long long) std::floor (x);
        if (loop) { position = whole % L; laps = whole / L; }
        else { position = whole < L ? whole : L; if (x >= (double) L) state = FX_TRANSPORT_FINISHED; }
    }
};

int main()
{
    const int C = 5, N = 1024, block = 480, ticks = 24;
    const double contextRate = 48000.0;
    const std::vector<long long> lengths = { 1000, 7, 2333, 600 };
    const std::vector<double> rates = { 44100.0, 96000.0, 22050.0, 0.0 };
    std::vector<std::vector<std::int16_t>> clips;
    std::vector<std::int16_t> bank;
    for (std::size_t k = 0; k < lengths.size(); ++k)
    {
        clips.emplace_back();
        for (long long i = 0; i < lengths[k]; ++i)
            clips.back().push_back ((std::int16_t) std::lrint (9000.0 * std::sin (0.05 * (double) (k + 1) * (double) i) + 500.0 * std::sin (1.7 * (double) i)));
        bank.insert (bank.end(), clips.back().begin(), clips.back().end());
    }
    std::vector<float> live ((std::size_t) C * block * ticks);
    for (std::size_t i = 0; i < live.size(); ++i) live[i] = (float) (0.2 * std::sin (0.021 * (double) i));
    try
    {
        int z = 0, p = 0;
        table.assign (4, 0.0f);
        EXPECT (fx_get_resampler_table (table.data(), (int) table.size(), &z, &p) == FX_ERR_INVALID_ARGUMENT);    // too small: refused, the sizes reported
        EXPECT (z == 16 && p == 512);
        table.assign ((std::size_t) z * (std::size_t) p + 2, -1.0f);
        fx::check (fx_get_resampler_table (table.data(), (int) table.size(), &Z, &P));
        EXPECT (table[0] == 1.0f && table[table.size() - 1] == 0.0f && table[table.size() - 2] == 0.0f);

        fx::RealTimeBatchAnalyser a (C, N), b (C, N);
        a.setGain (0.75f); b.setGain (0.75f);
        fx::AudioDataCollector sources (a), planar (b);
        fx::AudioFilePlayer loops (a, { 1, 2 }), shot (a, { 3 }), late (a, { 4 });
        std::vector<ModelTrack> model ((std::size_t) C);

        bool refused = false;
        try { loops.createClips (bank.data(), lengths, FX_SAMPLE_S16, { 44100.0 }); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused);                                                       // one rate per clip
        const int first = loops.createClips (bank.data(), lengths, FX_SAMPLE_S16, rates);
        auto load = [&] (fx::AudioFilePlayer& player, const std::vector<int>& which, const std::vector<double>& clipRates, bool looping) {
            std::vector<int> ids;
            for (int k : which) ids.push_back (first + k);
            player.loadFileIntoTransport (ids, looping);
            player.setFileSource (true);
            for (std::size_t i = 0; i < which.size(); ++i)
            {
                const int track = player.getTracks()[i];
                model[(std::size_t) track].load (clips[(std::size_t) which[i]], clipRates[i], contextRate, looping);
                planar.clearBuffer (track);
            }
        };
        auto command = [&] (fx::AudioFilePlayer& player, int which) {
            switch (which) { case FX_PLAY: player.play(); break; case FX_PAUSE: player.pause(); break; case FX_STOP: player.stop(); break; default: player.restart(); }
            for (int t : player.getTracks())
            {
                ModelTrack& m = model[(std::size_t) t];
                if (which == FX_PLAY)         { if (m.state == FX_TRANSPORT_FINISHED) { m.position = 0; m.k = 0; } m.state = FX_TRANSPORT_PLAYING; }
                else if (which == FX_PAUSE)   { if (m.state == FX_TRANSPORT_PLAYING) m.state = FX_TRANSPORT_PAUSED; }
                else if (which == FX_STOP)    { m.state = FX_TRANSPORT_STOPPED; m.position = 0; m.k = 0; }
                else                          { m.position = 0; m.k = 0; if (m.state == FX_TRANSPORT_FINISHED) m.state = FX_TRANSPORT_STOPPED; }
                if (which != FX_RESTART) planar.clearBuffer (t);
            }
        };

        load (loops, { 0, 1 }, { 44100.0, 96000.0 }, true);
        load (shot, { 2 }, { 22050.0 }, false);
        // a loaded clip's rate cannot change; an unloaded one's can, and the next load plays at it
        refused = false;
        try { loops.setClipRates ({ first + 3, first + 0 }, { 32000.0, 48000.0 }); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused);
        late.setClipRates ({ first + 3 }, { 32000.0 });
        load (late, { 3 }, { 32000.0 }, true);
        // a tick in the clips' own format is refused while they are rated: the resampler renders fp32
        std::vector<std::int16_t> words ((std::size_t) C * block, 0);
        refused = false;
        try { sources.pushSources (words.data(), block, FX_SAMPLE_S16); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused && sources.getNumPendingSamples() == 0);

        std::vector<float> rows ((std::size_t) C * block);
        int frames = 0;
        for (int tick = 0; tick < ticks; ++tick)
        {
            if (tick == 1)  { command (loops, FX_PLAY); command (shot, FX_PLAY); command (late, FX_PLAY); }
            if (tick == 4)  command (loops, FX_PAUSE);
            if (tick == 5)  command (loops, FX_PLAY);                           // the phase kept
            if (tick == 8)  command (loops, FX_RESTART);                        // while playing: back to 0, plays on
            if (tick == 12) command (shot, FX_PLAY);                            // from FINISHED (2333 samples at 22.05 kHz: 5079 outputs): from the top
            if (tick == 14) command (late, FX_STOP);
            if (tick == 15) command (late, FX_PLAY);
            const float* in = live.data() + (std::size_t) tick * C * block;
            for (int c = 0; c < C; ++c)
            {
                float* row = rows.data() + (std::size_t) c * block;
                if (c == 0) std::memcpy (row, in, (std::size_t) block * sizeof (float));       // track 0 listens to the input
                else model[(std::size_t) c].render (row, block);
            }
            const int na = sources.pushSources (in, block, FX_SAMPLE_F32);
            const int nb = planar.pushBlock (rows.data(), block, FX_SAMPLE_F32);
            EXPECT (na == nb);
            EXPECT (sources.getNumPendingSamples() == planar.getNumPendingSamples());
            const std::size_t n = (std::size_t) C * (std::size_t) na * FX_NUM_FEATURES;
            EXPECT (sameBits (sources.raw(), planar.raw(), n));
            EXPECT (sameBits (sources.smoothed(), planar.smoothed(), n));
            frames += na;
            if (tick == 11) EXPECT (model[3].state == FX_TRANSPORT_FINISHED);
            for (fx::AudioFilePlayer* player : { &loops, &shot, &late })
            {
                const fx::AudioFilePlayer::Transport t = player->getTransport();
                for (std::size_t i = 0; i < player->getTracks().size(); ++i)
                {
                    const ModelTrack& m = model[(std::size_t) player->getTracks()[i]];
                    EXPECT (t.source[i] == FX_SOURCE_FILE);
                    EXPECT (t.state[i] == m.state && t.position[i] == m.position && t.laps[i] == m.laps);
                }
            }
        }
        EXPECT (frames == block * ticks / (N / 2));
        EXPECT (model[2].laps > 1000 && model[1].laps > 5);
        for (int c = 0; c < C; ++c) EXPECT (a.getValues (c) == b.getValues (c));
        loops.loadFileIntoTransport (-1); shot.loadFileIntoTransport (-1); late.loadFileIntoTransport (-1);
        loops.destroyClips (first);
    }
    catch (const fx::Error& e)
    {
        std::printf ("clip_rates_mirror: %s\n", e.what());
        return 1;
    }
    std::printf (failures ? "clip_rates_mirror: %d failure(s)\n" : "clip_rates_mirror: ok\n", failures);
    return failures ? 1 : 0;
}
