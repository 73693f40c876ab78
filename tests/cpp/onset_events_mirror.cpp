// The onset event list through include/fx_realtime.hpp (tests/test_onset_events_cpp.py builds and runs this):
//   onset_events_mirror        : what needs no GPU -- the record's layout and the entries' refusals
//   onset_events_mirror --gpu  : a fx::LiveAnalyser with ONLY an onset callback, fed 481-sample blocks against a 1024-point window.
//                                The (track, frame) sequence the callback saw must be the list of a synchronous fx_push_samples run
//                                over the same blocks, which in turn must be the ones of that run's raw onset column.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>

#include "fx_realtime.hpp"

static int failures = 0;
#define EXPECT(cond) do { if (! (cond)) { std::printf ("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main (int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp (argv[1], "--gpu") == 0;
    static_assert (sizeof (fx_onset_event) == 16, "the record is 16 bytes");
    {
        fx_onset_event e[2]; int n = 7; long long lost = 7;
        EXPECT (fx_enable_onset_events (nullptr, 16) == FX_ERR_INVALID_ARGUMENT);
        EXPECT (std::strstr (fx_last_error(), "null context") != nullptr);
        EXPECT (fx_get_onset_events (nullptr, e, 2, &n, &lost) == FX_ERR_INVALID_ARGUMENT && n == 0 && lost == 0);
        EXPECT ((char*) &e[0].channel - (char*) &e[0] == 8 && (char*) &e[0].call_frame - (char*) &e[0] == 12);
    }
    if (! gpu)
    {
        std::printf (failures ? "onset_events_mirror: %d failure(s)\n" : "onset_events_mirror: ok\n", failures);
        return failures ? 1 : 0;
    }

    const int C = 70, N = 1024, H = N / 2, BLOCK = 481, BLOCKS = 80;          // 70 tracks: one full 64-lane group and a ragged one
    const int total = BLOCK * BLOCKS, frames = total / H;
    // tone bursts gated per track and hop, silence between them
    std::vector<float> stream ((size_t) C * total);
    unsigned s = 2463534242u;
    for (int c = 0; c < C; c++)
        for (int h = 0; h * H < total; h++)
        {
            s = s * 1664525u + 1013904223u;
            const float level = (s >> 16) % 3 == 0 ? 0.6f : 0.0f;
            for (int i = h * H; i < (h + 1) * H && i < total; i++)
                stream[(size_t) c * total + i] = level * std::sin (0.02f * (float) (c + 3) * (float) i);
        }
    std::vector<std::vector<float>> blocks ((size_t) BLOCKS, std::vector<float> ((size_t) C * BLOCK));
    for (int b = 0; b < BLOCKS; b++)
        for (int c = 0; c < C; c++)
            std::memcpy (&blocks[(size_t) b][(size_t) c * BLOCK], &stream[(size_t) c * total + (size_t) b * BLOCK], sizeof (float) * BLOCK);

    try
    {
        // the synchronous run: the list, and the raw column it must be the ones of
        std::vector<std::pair<int, long long>> want, column;
        {
            fx::RealTimeBatchAnalyser an (C, N);
            an.enableOnsetEvents (C * frames);
            std::vector<float> raw ((size_t) C * 2 * 12), sm (raw.size());
            long long before = 0;
            for (int b = 0; b < BLOCKS; b++)
            {
                int got = 0;
                fx::check (fx_push_samples (an.handle(), blocks[(size_t) b].data(), BLOCK, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data(), &got));
                EXPECT (got <= 2);
                for (int t = 0; t < got; t++)
                    for (int c = 0; c < C; c++)
                        if (raw[((size_t) c * (size_t) got + (size_t) t) * 12 + FX_ONSET] == 1.0f) column.push_back ({ c, before + t });
                before += got;
            }
            EXPECT (before == frames);
            long long lost = -1;
            for (const fx_onset_event& e : an.getOnsetEvents (&lost)) want.push_back ({ e.channel, e.frame });
            EXPECT (lost == 0);
            EXPECT (an.getOnsetEvents().empty());
        }
        EXPECT (want == column);
        EXPECT (want.size() >= 50);                       // (the signal switches 70 tracks on and off for 75 frames)
        std::printf ("synchronous run: %d events in %d frames of %d tracks\n", (int) want.size(), frames, C);

        // the live engine with an onset callback and nothing else
        std::vector<std::pair<int, long long>> seen;
        {
            fx::RealTimeBatchAnalyser an (C, N);
            fx::LiveAnalyser live (an, BLOCK);
            live.setOnsetDetectedCallback ([&] (int track, long long frame) { seen.push_back ({ track, frame }); });
            for (int b = 0; b < BLOCKS; b++)
                while (! live.pushBlock (blocks[(size_t) b].data(), BLOCK)) std::this_thread::sleep_for (std::chrono::milliseconds (1));
            live.drain();
            const fx::LiveAnalyser::Stats st = live.getStats();
            EXPECT (st.errors == 0);
            EXPECT (st.blocksAnalysed == BLOCKS && st.framesPerChannel == frames);
            EXPECT (live.latestSmoothed().empty());       // the vectors never came back: nobody asked for them
            live.stop();
            // ... and the values are there all the same, for the GUI's getValue queries
            EXPECT (an.getValues (0).size() == 12);
        }
        EXPECT (seen == want);
    }
    catch (const fx::Error& e)
    {
        std::printf ("fx::Error %d: %s\n", (int) e.code, e.what());
        failures++;
    }
    std::printf (failures ? "onset_events_mirror --gpu: %d failure(s)\n" : "onset_events_mirror --gpu: ok\n", failures);
    return failures ? 1 : 0;
}
