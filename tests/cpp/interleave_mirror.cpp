// interleave_mirror -- fx::AudioDataCollector with a channel map (include/fx_realtime.hpp), compiled with g++ against libfx_hip.so.
//
// Two collectors are given the same device channels to collect (setChannelToCollect, ref AudioDataCollector.h:123), one of them
// changed while samples are pending.  One takes each block interleaved, as a device or a file delivers it (pushInterleaved: de-interleaved
// on the GPU), the other JUCE's per-channel pointers (audioDeviceIOCallback: inputChannelData[channel collected], on the host).  Every
// frame count, raw and smoothed vector must be the same bits.  Then 16-bit PCM: pushInterleaved against pushBlock of the planar block.
// Needs a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fx_realtime.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf ("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool sameBits (const float* a, const float* b, std::size_t n) { return n == 0 || std::memcmp (a, b, n * sizeof (float)) == 0; }

int main()
{
    const int C = 5, K = 8, N = 1024, total = 9000;
    std::vector<float> interleaved ((std::size_t) total * K);
    std::vector<std::vector<float>> channels ((std::size_t) K, std::vector<float> ((std::size_t) total));
    for (int i = 0; i < total; ++i)
        for (int k = 0; k < K; ++k)
        {
            const float v = 0.4f * std::sin (0.013f * (float) (k + 1) * (float) i) + 0.05f * std::sin (0.9f * (float) (i * (k + 3) % 97));
            interleaved[(std::size_t) i * K + (std::size_t) k] = v;
            channels[(std::size_t) k][(std::size_t) i] = v;
        }
    try
    {
        fx::RealTimeBatchAnalyser a (C, N), b (C, N);
        a.setGain (0.75f); b.setGain (0.75f);
        fx::AudioDataCollector byFrames (a), byChannel (b);
        EXPECT (byFrames.getChannelToCollect (3) == 3);
        for (fx::AudioDataCollector* col : { &byFrames, &byChannel })
        {
            col->setChannelToCollect (0, 7);
            col->setChannelToCollect (2, 7);
            col->setChannelToCollect (4, 1);
        }
        EXPECT (byFrames.getChannelToCollect (0) == 7 && byFrames.getChannelToCollect (1) == 1 && byFrames.getChannelToCollect (4) == 1);
        std::vector<const float*> inputs ((std::size_t) K);
        int frames = 0, block = 0;
        for (int at = 0; at < total; at += 481, ++block)
        {
            const int len = total - at < 481 ? total - at : 481;
            if (block == 5)
            {
                EXPECT (byFrames.getNumPendingSamples() > 0);            // the move comes while samples are pending: they are kept
                byFrames.setChannelToCollect (1, 6);
                byChannel.setChannelToCollect (1, 6);
            }
            for (int k = 0; k < K; ++k) inputs[(std::size_t) k] = channels[(std::size_t) k].data() + at;
            const int na = byFrames.pushInterleaved (interleaved.data() + (std::size_t) at * K, K, len, FX_SAMPLE_F32);
            const int nb = byChannel.audioDeviceIOCallback (inputs.data(), K, len);
            EXPECT (na == nb);
            EXPECT (byFrames.getNumPendingSamples() == byChannel.getNumPendingSamples());
            const std::size_t n = (std::size_t) C * (std::size_t) na * FX_NUM_FEATURES;
            EXPECT (sameBits (byFrames.raw(), byChannel.raw(), n));
            EXPECT (sameBits (byFrames.smoothed(), byChannel.smoothed(), n));
            frames += na;
        }
        EXPECT (frames == total / (N / 2));
        for (int c = 0; c < C; ++c) EXPECT (a.getValues (c) == b.getValues (c));
        // a source the block does not have is refused, and changes nothing
        bool refused = false;
        try { byFrames.pushInterleaved (interleaved.data(), 7, 10, FX_SAMPLE_F32); } catch (const fx::Error&) { refused = true; }
        EXPECT (refused && byFrames.getNumPendingSamples() == byChannel.getNumPendingSamples());
        refused = false;
        try { byChannel.audioDeviceIOCallback (inputs.data(), 7, 10); }
        catch (const fx::Error& e) { refused = std::strstr (e.what(), "input channel 7") != nullptr; }
        EXPECT (refused);

        // one map for both entry points: a collector built on an analyser whose map was set before it reads that map
        fx::RealTimeBatchAnalyser e (C, N), f (C, N);
        const std::vector<int> preset = { 6, 6, 0, 2, 5 };
        e.setChannelMap (preset);
        f.setChannelMap (preset);
        fx::AudioDataCollector lateFrames (e), lateChannel (f);
        for (int c = 0; c < C; ++c) EXPECT (lateChannel.getChannelToCollect (c) == preset[(std::size_t) c]);
        EXPECT (f.getHighestSourceChannel() == 6);
        for (int at = 0; at < 3000; at += 700)
        {
            for (int k = 0; k < K; ++k) inputs[(std::size_t) k] = channels[(std::size_t) k].data() + at;
            const int na = lateFrames.pushInterleaved (interleaved.data() + (std::size_t) at * K, K, 700, FX_SAMPLE_F32);
            const int nb = lateChannel.audioDeviceIOCallback (inputs.data(), K, 700);
            EXPECT (na == nb);
            const std::size_t n = (std::size_t) C * (std::size_t) na * FX_NUM_FEATURES;
            EXPECT (sameBits (lateFrames.raw(), lateChannel.raw(), n));
            EXPECT (sameBits (lateFrames.smoothed(), lateChannel.smoothed(), n));
        }

        // 16-bit PCM as a file's data chunk holds it, against the planar block the map makes of it
        fx::RealTimeBatchAnalyser c16 (C, N), d16 (C, N);
        fx::AudioDataCollector inter16 (c16), planar16 (d16);
        inter16.setChannelToCollect (3, 0);
        const int map[C] = { 0, 1, 2, 0, 4 };
        std::vector<std::int16_t> pcm ((std::size_t) total * K);
        for (std::size_t i = 0; i < pcm.size(); ++i) pcm[i] = (std::int16_t) std::lrint (interleaved[i] * 32767.0f);
        std::vector<std::int16_t> rows;
        for (int at = 0; at < total; at += 1000)
        {
            const int len = total - at < 1000 ? total - at : 1000;
            rows.assign ((std::size_t) C * (std::size_t) len, 0);
            for (int c = 0; c < C; ++c)
                for (int i = 0; i < len; ++i) rows[(std::size_t) c * (std::size_t) len + (std::size_t) i] = pcm[((std::size_t) (at + i)) * K + (std::size_t) map[c]];
            const int na = inter16.pushInterleaved (pcm.data() + (std::size_t) at * K, K, len, FX_SAMPLE_S16);
            const int nb = planar16.pushBlock (rows.data(), len, FX_SAMPLE_S16);
            EXPECT (na == nb);
            const std::size_t n = (std::size_t) C * (std::size_t) na * FX_NUM_FEATURES;
            EXPECT (sameBits (inter16.raw(), planar16.raw(), n));
            EXPECT (sameBits (inter16.smoothed(), planar16.smoothed(), n));
        }
    }
    catch (const fx::Error& e)
    {
        std::printf ("interleave_mirror: %s\n", e.what());
        return 1;
    }
    std::printf (failures ? "interleave_mirror: %d failure(s)\n" : "interleave_mirror: ok\n", failures);
    return failures ? 1 : 0;
}
