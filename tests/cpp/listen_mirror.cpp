// listen_mirror -- toggleCollectInput / setListen / getListens of fx::AudioFilePlayer (include/fx_realtime.hpp), compiled with g++
// against libfx_hip.so.
//
// Two analysers of 6 tracks get the same ticks.  `a` is driven through the C++ mirror as the reference's source-type callback drives
// a track (AnalyserTrackController.h:92-107: to "audio file" and back), `b` through the C calls the mirror is said to make:
// fx_set_channel_sources + fx_set_channel_listen.  Raw and smoothed features, the mix and the listens must be the same bits after
// every tick.  Beside that, what only a working copy gives: two tracks with different files that listen to the same output return
// the same features, and another output gives others.  Needs a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fx_realtime.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf ("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)
#define OK(call) EXPECT ((call) == FX_OK)

static bool sameTrack (const float* values, int frames, int t, int u)
{
    return std::memcmp (values + (std::size_t) t * frames * FX_NUM_FEATURES, values + (std::size_t) u * frames * FX_NUM_FEATURES,
                        sizeof (float) * (std::size_t) frames * FX_NUM_FEATURES) == 0;
}

int main()
{
    const int C = 6, N = 1024, block = 441, ticks = 6;
    const std::vector<long long> lengths = { 1000, 333 };
    std::vector<float> bank;
    for (std::size_t k = 0; k < lengths.size(); ++k)
        for (long long i = 0; i < lengths[k]; ++i)
            bank.push_back ((float) (0.3 * std::sin (0.05 * (double) (k + 1) * (double) i) + 0.01 * std::sin (1.7 * (double) i)));
    std::vector<float> live ((std::size_t) C * block * ticks);
    for (std::size_t i = 0; i < live.size(); ++i) live[i] = (float) (0.2 * std::sin (0.021 * (double) i) * std::sin (0.0003 * (double) i));
    try
    {
        fx::RealTimeBatchAnalyser a (C, N), b (C, N);
        fx::AudioDataCollector ticksA (a), ticksB (b);
        fx::AudioFilePlayer files (a, { 1, 2 }), other (a, { 4 }), filesB (b, { 1, 2 }), otherB (b, { 4 });
        const int pair[2] = { 1, 2 }, single[1] = { 4 };

        // without a monitor a track can only go back to the input
        bool refused = false;
        try { files.toggleCollectInput (false, 0); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused && files.getTransport().source == std::vector<int> (2, FX_SOURCE_INPUT));       // (and nothing changed)
        files.toggleCollectInput (true);
        EXPECT (files.getTransport().source == std::vector<int> (2, FX_SOURCE_INPUT));

        // the same players and the same monitor on both
        int firstA = -1, firstB = -1;
        for (int which = 0; which < 2; ++which)
        {
            fx::AudioFilePlayer& p = which ? filesB : files;
            fx::AudioFilePlayer& q = which ? otherB : other;
            const int first = p.createClips (bank.data(), lengths);
            (which ? firstB : firstA) = first;
            p.loadFileIntoTransport ({ first + 0, first + 1 });
            q.loadFileIntoTransport (first + 1);
            p.enableMonitor();
            p.setMonitor (true, { 0.5f, -1.25f }, { 1.0f });
            q.setMonitor (true, { 0.75f }, { -0.3f });
        }
        EXPECT (files.getListens() == std::vector<int> (2, FX_LISTEN_SELF));

        // to "audio file": the mirror on a, the C calls on b
        files.toggleCollectInput (false, 0);
        other.toggleCollectInput (false, 1);
        const int file2[2] = { FX_SOURCE_FILE, FX_SOURCE_FILE }, left2[2] = { FX_LISTEN_LEFT, FX_LISTEN_LEFT }, right1[1] = { FX_LISTEN_RIGHT };
        OK (fx_set_channel_listen (b.handle(), pair, 2, left2));
        OK (fx_set_channel_sources (b.handle(), pair, 2, file2));
        OK (fx_set_channel_listen (b.handle(), single, 1, right1));
        OK (fx_set_channel_sources (b.handle(), single, 1, file2));
        files.play(); other.play(); filesB.play(); otherB.play();
        EXPECT (files.getListens() == std::vector<int> (2, FX_LISTEN_LEFT) && other.getListens() == std::vector<int> (1, FX_LISTEN_RIGHT));
        std::vector<int> all ((std::size_t) C, -1);
        OK (fx_get_channel_listen (b.handle(), all.data()));
        EXPECT (all == std::vector<int> ({ 0, 1, 1, 0, 2, 0 }));
        EXPECT (files.getTransport().source == std::vector<int> (2, FX_SOURCE_FILE));

        // the monitor is not freed under a listener
        refused = false;
        try { files.enableMonitor (false); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused && files.getListens() == std::vector<int> (2, FX_LISTEN_LEFT));

        std::vector<float> leftA, rightA, leftB, rightB;
        int framesSeen = 0;
        for (int tick = 0; tick < ticks; ++tick)
        {
            const float* in = live.data() + (std::size_t) tick * C * block;
            const int fa = ticksA.pushSources (in, block), fb = ticksB.pushSources (in, block);
            EXPECT (fa == fb);
            const std::size_t bytes = sizeof (float) * (std::size_t) C * (std::size_t) fa * FX_NUM_FEATURES;
            EXPECT (std::memcmp (ticksA.raw(), ticksB.raw(), bytes) == 0 && std::memcmp (ticksA.smoothed(), ticksB.smoothed(), bytes) == 0);
            EXPECT (files.getMonitor (leftA, rightA) == block && filesB.getMonitor (leftB, rightB) == block);
            EXPECT (leftA.size() == leftB.size() && std::memcmp (leftA.data(), leftB.data(), sizeof (float) * leftA.size()) == 0);
            EXPECT (rightA.size() == rightB.size() && std::memcmp (rightA.data(), rightB.data(), sizeof (float) * rightA.size()) == 0);
            if (fa > 0)
            {
                // tracks 1 and 2 play different files and hear the same output; track 4 hears the other one; 0 and 3 hear themselves
                EXPECT (sameTrack (ticksA.raw(), fa, 1, 2) && ! sameTrack (ticksA.raw(), fa, 1, 4) && ! sameTrack (ticksA.raw(), fa, 1, 0));
                framesSeen += fa;
            }
        }
        EXPECT (framesSeen == (block * ticks) / (N / 2));
        float loudest = 0.0f;
        for (float v : leftA) loudest = std::fmax (loudest, std::fabs (v));
        EXPECT (loudest > 0.01f);

        // back to the input: the players stop, everybody hears itself, and the monitor may go
        files.toggleCollectInput (true);
        other.toggleCollectInput (true);
        const int input2[2] = { FX_SOURCE_INPUT, FX_SOURCE_INPUT }, self2[2] = { FX_LISTEN_SELF, FX_LISTEN_SELF };
        OK (fx_set_channel_sources (b.handle(), pair, 2, input2));
        OK (fx_set_channel_listen (b.handle(), pair, 2, self2));
        OK (fx_set_channel_sources (b.handle(), single, 1, input2));
        OK (fx_set_channel_listen (b.handle(), single, 1, self2));
        EXPECT (files.getListens() == std::vector<int> (2, FX_LISTEN_SELF) && other.getListens() == std::vector<int> (1, FX_LISTEN_SELF));
        EXPECT (files.getTransport().source == std::vector<int> (2, FX_SOURCE_INPUT) && files.getTransport().state == std::vector<int> (2, FX_TRANSPORT_STOPPED));
        for (int tick = 0; tick < 3; ++tick)
        {
            const float* in = live.data() + (std::size_t) tick * C * block;
            const int fa = ticksA.pushSources (in, block), fb = ticksB.pushSources (in, block);
            EXPECT (fa == fb);
            const std::size_t bytes = sizeof (float) * (std::size_t) C * (std::size_t) fa * FX_NUM_FEATURES;
            EXPECT (std::memcmp (ticksA.raw(), ticksB.raw(), bytes) == 0 && std::memcmp (ticksA.smoothed(), ticksB.smoothed(), bytes) == 0);
            if (fa > 0) EXPECT (! sameTrack (ticksA.raw(), fa, 1, 2));
        }
        // setListen on its own: the source stays
        files.setListen (FX_LISTEN_RIGHT);
        EXPECT (files.getListens() == std::vector<int> (2, FX_LISTEN_RIGHT) && files.getTransport().source == std::vector<int> (2, FX_SOURCE_INPUT));
        refused = false;
        try { files.setListen (3); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused && files.getListens() == std::vector<int> (2, FX_LISTEN_RIGHT));
        files.setListen (FX_LISTEN_SELF);
        files.enableMonitor (false);
        filesB.enableMonitor (false);
        for (fx::AudioFilePlayer* p : { &files, &other, &filesB, &otherB }) p->loadFileIntoTransport (-1);
        files.destroyClips (firstA);
        filesB.destroyClips (firstB);
    }
    catch (const fx::Error& e)
    {
        std::printf ("listen_mirror: %s\n", e.what());
        return 1;
    }
    std::printf (failures ? "listen_mirror: %d failure(s)\n" : "listen_mirror: ok\n", failures);
    return failures ? 1 : 0;
}
