// monitor_mirror -- the monitor operations of fx::AudioFilePlayer (include/fx_realtime.hpp), compiled with g++ against libfx_hip.so.
//
// One analyser of 70 tracks (a partial second group of 64): two players' tracks loop 16-bit clips, the rest listen to the live
// block.  The mix the library returns must be, bit for bit, the sum fx.h specifies, which a loop over floats states here: tracks
// ascending inside groups of FX_MONITOR_GROUP, then the groups, every product and sum rounded to float (this file is compiled without
// contraction: x86-64 has no fused multiply-add unless asked for).  Needs a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fx_realtime.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf ("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

int main()
{
    const int C = 70, N = 1024, block = 441, ticks = 4;
    const std::vector<long long> lengths = { 1000, 7, 333 };
    std::vector<std::int16_t> bank;
    for (std::size_t k = 0; k < lengths.size(); ++k)
        for (long long i = 0; i < lengths[k]; ++i)
            bank.push_back ((std::int16_t) std::lrint (9000.0 * std::sin (0.05 * (double) (k + 1) * (double) i) + 3.0 * std::sin (1.7 * (double) i)));
    std::vector<std::int16_t> live ((std::size_t) C * block * ticks);
    for (std::size_t i = 0; i < live.size(); ++i) live[i] = (std::int16_t) std::lrint (7000.0 * std::sin (0.021 * (double) i) * std::sin (0.0003 * (double) i));
    try
    {
        fx::RealTimeBatchAnalyser a (C, N);
        a.setGain (0.25f);                                              // the analysers' gain: not heard
        fx::AudioDataCollector sources (a);
        fx::AudioFilePlayer loops (a, { 1, 2, 66 }), rest (a, { 0, 3, 4, 5, 64, 65, 69 });
        std::vector<float> left, right;

        bool refused = false;
        try { loops.setMonitor (true); } catch (const fx::Error&) { refused = true; }      // no monitor yet
        EXPECT (refused);
        loops.enableMonitor();
        EXPECT (loops.getMonitor (left, right) == 0 && left.empty() && right.empty());
        fx::AudioFilePlayer::Sends s = loops.getMonitorSends();
        EXPECT (s.on == std::vector<int> (3, 0) && s.left == std::vector<float> (3, 1.0f) && s.right == std::vector<float> (3, 1.0f));

        const int first = loops.createClips (bank.data(), lengths, FX_SAMPLE_S16);
        loops.loadFileIntoTransport ({ first + 0, first + 1, first + 2 });
        loops.setFileSource (true);
        loops.play();
        loops.setMonitor (true, { 0.5f, -1.25f, 2.0f }, { 1.0f });
        rest.setMonitor (true, { 0.75f }, { -0.3f, 0.0f, 1.0f, 1.5f, -2.0f, 0.125f, 1e-36f });
        rest.enableMonitor();                                           // enabled already: the sends stay
        s = loops.getMonitorSends();
        EXPECT (s.on == std::vector<int> (3, 1) && s.left == std::vector<float> ({ 0.5f, -1.25f, 2.0f }) && s.right == std::vector<float> (3, 1.0f));

        // the model: every track's send, and the loops' positions
        std::vector<int> on ((std::size_t) C, 0);
        std::vector<float> gl ((std::size_t) C, 1.0f), gr ((std::size_t) C, 1.0f);
        for (fx::AudioFilePlayer* p : { &loops, &rest })
        {
            const fx::AudioFilePlayer::Sends t = p->getMonitorSends();
            for (std::size_t i = 0; i < p->getTracks().size(); ++i)
            {
                const std::size_t c = (std::size_t) p->getTracks()[i];
                on[c] = t.on[i]; gl[c] = t.left[i]; gr[c] = t.right[i];
            }
        }
        const int clipOfTrack[3] = { 0, 1, 2 };
        long long position[3] = { 0, 0, 0 };
        std::vector<long long> start (lengths.size(), 0);
        for (std::size_t k = 1; k < lengths.size(); ++k) start[k] = start[k - 1] + lengths[k - 1];

        std::vector<float> x ((std::size_t) C * block);
        for (int tick = 0; tick < ticks; ++tick)
        {
            const std::int16_t* in = live.data() + (std::size_t) tick * C * block;
            for (int c = 0; c < C; ++c)
                for (int i = 0; i < block; ++i)
                    x[(std::size_t) c * block + (std::size_t) i] = (float) in[(std::size_t) c * block + (std::size_t) i] * (1.0f / 32768.0f);
            for (int j = 0; j < 3; ++j)
            {
                const int c = loops.getTracks()[(std::size_t) j], k = clipOfTrack[j];
                for (int i = 0; i < block; ++i)
                {
                    x[(std::size_t) c * block + (std::size_t) i] = (float) bank[(std::size_t) (start[(std::size_t) k] + position[j])] * (1.0f / 32768.0f);
                    position[j] = (position[j] + 1) % lengths[(std::size_t) k];
                }
            }
            sources.pushSources (in, block, FX_SAMPLE_S16);
            EXPECT (loops.getMonitor (left, right) == block && (int) left.size() == block && (int) right.size() == block);
            for (int ch = 0; ch < 2 && left.size() == (std::size_t) block; ++ch)
            {
                const std::vector<float>& gain = ch ? gr : gl;
                const std::vector<float>& got = ch ? right : left;
                int wrong = 0;
                for (int i = 0; i < block; ++i)
                {
                    volatile float total = 0.0f;                        // (volatile: every step a float in memory, whatever the optimiser thinks)
                    for (int g = 0; g < C; g += FX_MONITOR_GROUP)
                    {
                        volatile float part = 0.0f;
                        for (int c = g; c < C && c < g + FX_MONITOR_GROUP; ++c)
                            if (on[(std::size_t) c])
                            {
                                volatile float product = gain[(std::size_t) c] * x[(std::size_t) c * block + (std::size_t) i];
                                part = part + product;
                            }
                        total = total + part;
                    }
                    const float want = total;
                    if (std::memcmp (&want, &got[(std::size_t) i], sizeof (float)) != 0) ++wrong;
                }
                EXPECT (wrong == 0);
            }
        }
        float loudest = 0.0f;
        for (float v : left) loudest = std::fmax (loudest, std::fabs (v));
        EXPECT (loudest > 0.01f);

        rest.setMonitor (false);
        loops.setMonitor (false);
        sources.pushSources (live.data(), block, FX_SAMPLE_S16);
        EXPECT (loops.getMonitor (left, right) == block);
        for (float v : left) EXPECT (v == 0.0f && ! std::signbit (v));
        loops.enableMonitor (false);
        refused = false;
        try { loops.getMonitor (left, right); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused);
        loops.loadFileIntoTransport (-1);
        loops.destroyClips (first);
    }
    catch (const fx::Error& e)
    {
        std::printf ("monitor_mirror: %s\n", e.what());
        return 1;
    }
    std::printf (failures ? "monitor_mirror: %d failure(s)\n" : "monitor_mirror: ok\n", failures);
    return failures ? 1 : 0;
}
