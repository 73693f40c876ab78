// clip_mirror -- fx::AudioFilePlayer and AudioDataCollector::pushSources (include/fx_realtime.hpp), compiled with g++ against libfx_hip.so.
//
// Two analysers: one plays files on the GPU (clips in device memory, transport commands, pushSources), the other is given, by
// pushBlock, the planar block a host model makes of the same tick -- the model is a loop over a std::vector per track, with the
// reference's transport (AudioFilePlayer.h:41-67: a looping reader behind play / pause / stop / restart) and our one-shot clips --
// and has the tracks' collectors cleared where the reference's buttons clear them (AnalyserTrackController.h:135-137).  Every frame
// count, raw and smoothed vector must be the same bits, and the transport the library reports must be the model's.  Needs a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fx_realtime.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf ("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool sameBits (const float* a, const float* b, std::size_t n) { return n == 0 || std::memcmp (a, b, n * sizeof (float)) == 0; }

struct ModelTrack
{
    bool file = false, loop = true;
    int state = FX_TRANSPORT_NO_FILE;
    std::vector<std::int16_t> clip;
    long long position = 0, laps = 0;

    std::int16_t next()                                             // one sample of a track whose source is its file
    {
        if (state != FX_TRANSPORT_PLAYING) return 0;
        const std::int16_t v = clip[(std::size_t) position];
        if (++position == (long long) clip.size())
        {
            if (loop) { position = 0; ++laps; }
            else state = FX_TRANSPORT_FINISHED;
        }
        return v;
    }
};

int main()
{
    const int C = 6, N = 1024, block = 480, ticks = 30;
    const std::vector<long long> lengths = { 1000, 7, 333, 1 };
    std::vector<std::int16_t> bank;
    for (std::size_t k = 0; k < lengths.size(); ++k)
        for (long long i = 0; i < lengths[k]; ++i)
            bank.push_back ((std::int16_t) std::lrint (9000.0 * std::sin (0.05 * (double) (k + 1) * (double) i) + 500.0 * std::sin (1.7 * (double) i)));
    std::vector<std::int16_t> live ((std::size_t) C * block * ticks);
    for (std::size_t i = 0; i < live.size(); ++i) live[i] = (std::int16_t) std::lrint (7000.0 * std::sin (0.021 * (double) i));
    try
    {
        fx::RealTimeBatchAnalyser a (C, N), b (C, N);
        a.setGain (0.75f); b.setGain (0.75f);
        fx::AudioDataCollector sources (a), planar (b);
        fx::AudioFilePlayer loops (a, { 1, 2 }), shot (a, { 3 }), single (a, { 4 }), empty (a, { 5 });
        std::vector<ModelTrack> model ((std::size_t) C);
        EXPECT (! loops.hasFile());

        const int first = loops.createClips (bank.data(), lengths, FX_SAMPLE_S16);
        auto clipOf = [&] (int k) {
            std::size_t at = 0;
            for (int j = 0; j < k; ++j) at += (std::size_t) lengths[(std::size_t) j];
            return std::vector<std::int16_t> (bank.begin() + (long) at, bank.begin() + (long) (at + (std::size_t) lengths[(std::size_t) k]));
        };
        auto load = [&] (int track, int k, bool loop) {
            ModelTrack& m = model[(std::size_t) track];
            m.clip = clipOf (k); m.loop = loop; m.state = FX_TRANSPORT_STOPPED; m.position = m.laps = 0;
            planar.clearBuffer (track);
        };
        auto command = [&] (fx::AudioFilePlayer& p, int which) {
            switch (which) { case FX_PLAY: p.play(); break; case FX_PAUSE: p.pause(); break; case FX_STOP: p.stop(); break; default: p.restart(); }
            for (int t : p.getTracks())
            {
                ModelTrack& m = model[(std::size_t) t];
                if (which == FX_PLAY)         { if (m.state == FX_TRANSPORT_FINISHED) m.position = 0; m.state = FX_TRANSPORT_PLAYING; }
                else if (which == FX_PAUSE)   { if (m.state == FX_TRANSPORT_PLAYING) m.state = FX_TRANSPORT_PAUSED; }
                else if (which == FX_STOP)    { if (! m.clip.empty()) { m.state = FX_TRANSPORT_STOPPED; m.position = 0; } }
                else                          { m.position = 0; if (m.state == FX_TRANSPORT_FINISHED) m.state = FX_TRANSPORT_STOPPED; }
                if (which != FX_RESTART) planar.clearBuffer (t);
            }
        };
        auto toFile = [&] (fx::AudioFilePlayer& p) {
            p.setFileSource (true);
            for (int t : p.getTracks()) { model[(std::size_t) t].file = true; planar.clearBuffer (t); }
        };

        loops.loadFileIntoTransport ({ first + 0, first + 1 });          load (1, 0, true); load (2, 1, true);
        shot.loadFileIntoTransport (first + 2, false);                   load (3, 2, false);
        single.loadFileIntoTransport (first + 3);                        load (4, 3, true);
        EXPECT (loops.hasFile() && shot.hasFile() && ! empty.hasFile());
        toFile (loops); toFile (shot); toFile (single); toFile (empty);
        bool refused = false;
        try { empty.play(); } catch (const fx::Error&) { refused = true; }      // no file: refused, nothing changes
        EXPECT (refused);

        std::vector<std::int16_t> rows ((std::size_t) C * block);
        int frames = 0;
        for (int tick = 0; tick < ticks; ++tick)
        {
            if (tick == 1)  { command (loops, FX_PLAY); command (shot, FX_PLAY); command (single, FX_PLAY); }
            if (tick == 4)  command (loops, FX_PAUSE);
            if (tick == 5)  command (loops, FX_RESTART);                        // while paused: position 0, still paused
            if (tick == 6)  command (loops, FX_PLAY);
            if (tick == 8)  command (shot, FX_PLAY);                            // from FINISHED: from the top
            if (tick == 9)  command (shot, FX_RESTART);                         // from FINISHED: stopped at 0
            if (tick == 10) command (shot, FX_PLAY);
            if (tick == 11) command (loops, FX_RESTART);                        // while playing: back to 0, plays on
            if (tick == 12) command (single, FX_STOP);
            if (tick == 20) { loops.setFileSource (false); for (int t : loops.getTracks()) { ModelTrack& m = model[(std::size_t) t]; m.file = false; m.state = FX_TRANSPORT_STOPPED; m.position = 0; planar.clearBuffer (t); } }
            const std::int16_t* in = live.data() + (std::size_t) tick * C * block;
            for (int c = 0; c < C; ++c)
                for (int i = 0; i < block; ++i)
                    rows[(std::size_t) c * block + (std::size_t) i] = model[(std::size_t) c].file ? model[(std::size_t) c].next() : in[(std::size_t) c * block + (std::size_t) i];
            const int na = sources.pushSources (in, block, FX_SAMPLE_S16);
            const int nb = planar.pushBlock (rows.data(), block, FX_SAMPLE_S16);
            EXPECT (na == nb);
            EXPECT (sources.getNumPendingSamples() == planar.getNumPendingSamples());
            const std::size_t n = (std::size_t) C * (std::size_t) na * FX_NUM_FEATURES;
            EXPECT (sameBits (sources.raw(), planar.raw(), n));
            EXPECT (sameBits (sources.smoothed(), planar.smoothed(), n));
            frames += na;
            for (fx::AudioFilePlayer* p : { &loops, &shot, &single, &empty })
            {
                const fx::AudioFilePlayer::Transport t = p->getTransport();
                for (std::size_t i = 0; i < p->getTracks().size(); ++i)
                {
                    const ModelTrack& m = model[(std::size_t) p->getTracks()[i]];
                    EXPECT (t.source[i] == (m.file ? FX_SOURCE_FILE : FX_SOURCE_INPUT));
                    EXPECT (t.state[i] == m.state && t.position[i] == m.position && t.laps[i] == m.laps);
                }
            }
        }
        EXPECT (frames == block * ticks / (N / 2));
        EXPECT (model[2].laps > 100 && model[3].state == FX_TRANSPORT_FINISHED);
        for (int c = 0; c < C; ++c) EXPECT (a.getValues (c) == b.getValues (c));

        // a bank is freed only once nobody has one of its clips loaded
        refused = false;
        try { loops.destroyClips (first); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused);
        loops.loadFileIntoTransport (-1); shot.loadFileIntoTransport (-1); single.loadFileIntoTransport (-1);
        EXPECT (! loops.hasFile());
        loops.destroyClips (first);
    }
    catch (const fx::Error& e)
    {
        std::printf ("clip_mirror: %s\n", e.what());
        return 1;
    }
    std::printf (failures ? "clip_mirror: %d failure(s)\n" : "clip_mirror: ok\n", failures);
    return failures ? 1 : 0;
}
