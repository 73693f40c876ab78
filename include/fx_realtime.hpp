// fx_realtime.hpp -- header-only C++ host side above the C ABI (fx.h).
//
// Mirrors the reference's own interface for this path so that existing C++ callers read the same:
//   * AudioFeatures                 -- ref Source/RealTimeAnalyser.h:14-92 (same enum, updateFeature,
//                                      getValue, getFeatureName minus juce::String)
//   * fx::RealTimeBatchAnalyser     -- the pair RealTimeSpectralAnalyser + RealTimeHarmonicAnalyser
//                                      (ref RealTimeAnalyser.h:133-269) for many channels on one GPU;
//                                      setter names are the reference's.
//   * fx::AudioDataCollector        -- ref Source/AudioDataCollector.h:18-138: audioDeviceIOCallback takes device blocks of ANY
//                                      length for all channels; whole hops are analysed as they complete (fx_push_samples).
//   * fx::OSCFeatureMessage         -- ref Source/OSCFeatureAnalysisOutput.h:89-113 wire format.
//   * fx::OSCFeatureAnalysisOutput  -- ref Source/OSCFeatureAnalysisOutput.h:23-145: the 60 Hz timer that sends a track's latest values.
//   * fx::OSCBatchSender            -- the same sink for thousands of tracks: formed datagrams, sendmmsg, sender threads, one 60 Hz timer.
//   * fx::LiveAnalyser              -- the live engine: audioDeviceIOCallback on the audio thread NEVER blocks (a copy into a FIFO, as the
//                                      reference's collector copies into its ring, AudioDataCollector.h:36-70); a worker thread analyses
//                                      each block straight from its page-locked FIFO slot and publishes (callback, OSCBatchSender).
// No JUCE.  Errors are thrown as fx::Error (the reference only jasserts).
#ifndef FX_REALTIME_HPP
#define FX_REALTIME_HPP

#include <cstddef>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "fx.h"

// ---- ValueHistory, ref Source/RealTimeAudioAnalysis.h:40-96 -----------------------------------
struct ValueHistory
{
    explicit ValueHistory (int historyLength) : recordedHistory (0) { setHistoryLength (historyLength); }

    float getTotal() const
    {
        float total = 0.0f;
        for (std::size_t i = 0; i < history.size(); i++) total += history[i];
        return total;
    }
    void insertNewValueAndupdateHistory (float newValue)
    {
        for (std::size_t i = 0; i + 1 < history.size(); i++) history[i] = history[i + 1];
        if (! history.empty()) history[history.size() - 1] = newValue;
        if (recordedHistory < (int) history.size()) recordedHistory++;
    }
    void setHistoryLength (int historyLength)
    {
        recordedHistory = 0;
        history.assign ((std::size_t) (historyLength > 0 ? historyLength : 0), 0.0f);
    }
    std::vector<float> history;
    int recordedHistory;
};

// ---- AudioFeatures, ref Source/RealTimeAnalyser.h:14-92 ---------------------------------------
struct AudioFeatures
{
    enum eAudioFeature
    {
        enOnset = FX_ONSET, enRMS = FX_RMS, enF0 = FX_F0, enCentroid = FX_CENTROID, enSpread = FX_SPREAD,
        enFlatness = FX_FLATNESS, enLER = FX_LER, enFlux = FX_FLUX, enSlope = FX_SLOPE,
        enHarmonicEnergyRatio = FX_HER, enOddEvenHarmonicRatio = FX_OER, enInharmonicity = FX_INHARM,
        numFeatures = FX_NUM_FEATURES
    };

    static const char* getFeatureName (eAudioFeature f)          // ref :34-63
    {
        static const char* names[numFeatures] = { "Onset", "Amp.", "Pitch", "Centroid", "Spread", "Flatness",
                                                  "L.E.R", "Flux", "Slope", "H.E.R", "O.E.R", "Inharm." };
        return (f >= 0 && f < numFeatures) ? names[f] : "UNKNOWN";
    }
    static float getMaxValueForFeature (eAudioFeature) { return 1.0f; }     // ref :65-68

    AudioFeatures()                                               // ref :70-74
    {
        for (int f = 0; f < numFeatures; f++)
            smoothedFeatures.push_back (ValueHistory (f == enOnset || f == enFlux ? 1 : 10));
    }
    void updateFeature (eAudioFeature f, float v) { smoothedFeatures[(std::size_t) f].insertNewValueAndupdateHistory (v); }
    float getValue (eAudioFeature f) const                        // ref :84-88
    {
        const ValueHistory& h = smoothedFeatures[(std::size_t) f];
        return h.getTotal() / (float) h.recordedHistory;
    }

private:
    std::vector<ValueHistory> smoothedFeatures;
};

namespace fx
{
struct Error : std::runtime_error
{
    Error (fx_status c, const char* what) : std::runtime_error (what), code (c) {}
    fx_status code;
};

inline void check (fx_status s) { if (s != FX_OK) throw Error (s, fx_last_error()); }

// OnsetDetector::eOnsetDetectionType, ref Source/SpectralCharacteristics.h:213-219
enum eOnsetDetectionType { enSpectral = FX_ONSET_SPECTRAL, enAmplitude = FX_ONSET_AMPLITUDE, enCombination = FX_ONSET_COMBINATION };

class RealTimeBatchAnalyser
{
public:
    // ref RealTimeAnalyser.h:100 (AudioDataCollector&, AudioFeatures&, int windowSize, double sampleRate = 48000.0)
    RealTimeBatchAnalyser (int numChannels, int windowSize = 2048, double sampleRate = 48000.0, int deviceId = 0,
                           unsigned flags = FX_ORDER_SPECTRAL_THEN_HARMONIC)
        : channels (numChannels), window (windowSize), channelMap ((std::size_t) (numChannels > 0 ? numChannels : 0))
    {
        check (fx_create (&ctx, deviceId, numChannels, windowSize, sampleRate, flags));
        for (int c = 0; c < channels; ++c) channelMap[(std::size_t) c] = c;
    }
    ~RealTimeBatchAnalyser() { fx_destroy (ctx); }
    RealTimeBatchAnalyser (const RealTimeBatchAnalyser&) = delete;
    RealTimeBatchAnalyser& operator= (const RealTimeBatchAnalyser&) = delete;

    void sampleRateChanged (double sr)                         { check (fx_set_sample_rate (ctx, sr)); }          // ref :111
    void setOnsetDetectionSensitivity (float s)                { check (fx_set_onset_sensitivity (ctx, s)); }     // ref :244
    void setOnsetWindowLength (int length)                     { check (fx_set_onset_window (ctx, length)); }     // ref :250
    void setOnsetDetectionType (eOnsetDetectionType t)         { check (fx_set_onset_type (ctx, (int) t)); }      // ref :258
    void setGain (float g)                                     { check (fx_set_gain (ctx, g)); }                  // AudioDataCollector.h:124
    void reset()                                               { check (fx_reset_state (ctx)); }
    // The same four per track, as each AnalyserTrackController has its own (AnalyserTrackController.h:126-134): fx_set_channel_gains /
    // fx_set_channel_onset.  One track: the others keep what they have (and their onset histories).  The context-wide forms above
    // still set every track.  A setting: reset() keeps it.
    void setGain (int track, float g)
    {
        std::vector<float> v = perTrack().gain; v[at (track)] = g; setGains (v);
    }
    void setOnsetDetectionSensitivity (int track, float s)
    {
        std::vector<float> v = perTrack().sensitivity; v[at (track)] = s; setOnsetSettings (&v, nullptr, nullptr);
    }
    void setOnsetWindowLength (int track, int length)
    {
        std::vector<int> v ((std::size_t) channels, -1); v[at (track)] = length; setOnsetSettings (nullptr, &v, nullptr);
    }
    void setOnsetDetectionType (int track, eOnsetDetectionType t)
    {
        std::vector<int> v = perTrack().type; v[at (track)] = (int) t; setOnsetSettings (nullptr, nullptr, &v);
    }
    // A new AnalyserTrackController in one slot or several (ref MainComponent.cpp:137-186: tracks are destroyed and built one at a
    // time): fx_reset_channels.  The tracks' tail, flux state, histories, latest vector and pending samples are a new context's, their
    // frame index starts at 0 again; settings stay, the other tracks are untouched.
    void resetTrack (int track)                                { const int t = at (track); resetTracks (&t, 1); }
    void resetTracks (const int* tracks, int count)            { check (fx_reset_channels (ctx, tracks, count)); }
    // A track that leaves for another analyser or arrives from one (fx_export_channels / fx_import_channels): the reference moves an
    // AnalyserTrackController by its pointer; here its whole state travels as one record of trackStateBytes() per track, and the track
    // goes on in its new slot exactly as it would have in the old one.  Host memory; record i belongs to tracks[i].
    std::size_t trackStateBytes() const                        { return fx_track_state_bytes (ctx); }
    std::vector<unsigned char> exportTracks (const int* tracks, int count)
    {
        std::vector<unsigned char> records ((std::size_t) (count > 0 ? count : 0) * trackStateBytes());
        check (fx_export_channels (ctx, tracks, count, records.data(), records.size(), FX_MEM_HOST));
        return records;
    }
    void importTracks (const int* tracks, int count, const std::vector<unsigned char>& records)
    {
        check (fx_import_channels (ctx, tracks, count, records.data(), records.size(), FX_MEM_HOST));
    }
    std::vector<long long> trackFrames() const                 // frames each track has analysed since it was created or last reset
    {
        std::vector<long long> f ((std::size_t) channels);
        check (fx_get_channel_frames (ctx, f.data()));
        return f;
    }
    // array forms, one entry per track; a null vector leaves that setting alone, a window entry < 0 leaves that track's window and
    // histories alone
    void setGains (const std::vector<float>& gains)
    {
        if ((int) gains.size() != channels) throw Error (FX_ERR_INVALID_ARGUMENT, "per-track gains have one entry per track");
        check (fx_set_channel_gains (ctx, gains.data()));
    }
    void setOnsetSettings (const std::vector<float>* sensitivity, const std::vector<int>* windowLength, const std::vector<int>* type)
    {
        if ((sensitivity && (int) sensitivity->size() != channels) || (windowLength && (int) windowLength->size() != channels)
            || (type && (int) type->size() != channels))
            throw Error (FX_ERR_INVALID_ARGUMENT, "per-track onset settings have one entry per track");
        check (fx_set_channel_onset (ctx, sensitivity ? sensitivity->data() : nullptr, windowLength ? windowLength->data() : nullptr,
                                     type ? type->data() : nullptr));
    }
    struct TrackSettings { std::vector<float> gain, sensitivity; std::vector<int> windowLength, type; };
    TrackSettings perTrack() const                             // what each track runs with now (fx_get_channel_settings)
    {
        const std::size_t n = (std::size_t) channels;
        TrackSettings t { std::vector<float> (n), std::vector<float> (n), std::vector<int> (n), std::vector<int> (n) };
        check (fx_get_channel_settings (ctx, t.gain.data(), t.sensitivity.data(), t.windowLength.data(), t.type.data()));
        return t;
    }
    // AudioDataCollector::setChannelToCollect (AudioDataCollector.h:123) for every track at once (fx_set_channel_map): track c
    // collects source channel map[c]; an empty map restores the identity.  A setting: reset() keeps it.  The analyser keeps the map it
    // gave the context, and every AudioDataCollector on it reads that copy: change the map here or through a collector, not with
    // fx_set_channel_map on handle().
    void setChannelMap (const std::vector<int>& map)
    {
        if (! map.empty() && (int) map.size() != channels) throw Error (FX_ERR_INVALID_ARGUMENT, "a channel map has one entry per track");
        check (fx_set_channel_map (ctx, map.empty() ? nullptr : map.data()));
        highestSource = map.empty() ? channels - 1 : 0;
        for (int c = 0; c < channels; ++c)
        {
            channelMap[(std::size_t) c] = map.empty() ? c : map[(std::size_t) c];
            if (channelMap[(std::size_t) c] > highestSource) highestSource = channelMap[(std::size_t) c];
        }
    }
    const std::vector<int>& getChannelMap() const { return channelMap; }
    int getHighestSourceChannel() const           { return highestSource; }      // the highest source channel the map reads

    // RTP audio in (fx.h, "RTP audio in"): a tick's L16 / L24 datagrams, as a receiver collected them in slots of one stride, unpacked
    // to the tracks and analysed on the GPU.  Thin forms of fx_rtp_configure .. fx_rtp_get_stats, host memory; the socket side (which
    // fills the slots and chooses the streams' first timestamps) is the caller's.
    void rtpConfigure (int payloadFormat, const std::vector<int>& channelsPerStream)
    {
        check (fx_rtp_configure (ctx, payloadFormat, (int) channelsPerStream.size(), channelsPerStream.empty() ? nullptr : channelsPerStream.data()));
        rtpStreams = (int) channelsPerStream.size();
    }
    void setRtpSources (const std::vector<int>& tracks, const std::vector<int>& stream, const std::vector<int>& channel)
    {
        if (stream.size() != tracks.size() || channel.size() != tracks.size()) throw Error (FX_ERR_INVALID_ARGUMENT, "one stream and one channel per listed track");
        check (fx_rtp_set_track_sources (ctx, tracks.data(), (int) tracks.size(), stream.data(), channel.data()));
    }
    void rtpSources (std::vector<int>& stream, std::vector<int>& channel) const
    {
        stream.resize ((std::size_t) channels); channel.resize ((std::size_t) channels);
        check (fx_rtp_get_track_sources (ctx, stream.data(), channel.data()));
    }
    void setRtpTimestamps (const std::vector<int>& streams, const std::vector<unsigned>& timestamps)
    {
        if (timestamps.size() != streams.size()) throw Error (FX_ERR_INVALID_ARGUMENT, "one timestamp per listed stream");
        check (fx_rtp_set_cursors (ctx, streams.data(), (int) streams.size(), timestamps.data()));
    }
    void rtpTimestamps (std::vector<unsigned>& timestamps, std::vector<int>& running) const
    {
        timestamps.resize ((std::size_t) rtpStreams); running.resize ((std::size_t) rtpStreams);
        check (fx_rtp_get_cursors (ctx, timestamps.data(), running.data()));
    }
    // one tick of numSamples per track -> the frames analysed; raw / smoothed [channels][frames][12] (null: not wanted), disposition one
    // byte of FX_RTP_* bits per packet (null: not wanted)
    int pushRtp (const void* slots, const int* lengths, const int* streamOf, int numPackets, int slotStride, int numSamples,
                 float* raw, float* smoothed, unsigned char* disposition = nullptr)
    {
        int frames = 0;
        check (fx_push_rtp (ctx, slots, lengths, streamOf, numPackets, slotStride, numSamples, FX_MEM_HOST, raw, smoothed, &frames, disposition));
        return frames;
    }
    // the last tick's planar block [channels][n] as fx_push_samples takes it (FX_SAMPLE_S16 / FX_SAMPLE_S24 bytes) -> n
    int rtpBlock (std::vector<unsigned char>& block, int* sampleFormat = nullptr)
    {
        int n = 0, format = 0;
        unsigned char none = 0;
        const fx_status probe = fx_rtp_get_block (ctx, &none, 0, &n, &format, FX_MEM_HOST);      // (no room: refused, the count reported)
        if (probe != FX_OK && n == 0) check (probe);
        block.resize ((std::size_t) channels * (std::size_t) n * (format == FX_SAMPLE_S16 ? 2u : 3u));
        if (n > 0) check (fx_rtp_get_block (ctx, block.data(), block.size(), &n, &format, FX_MEM_HOST));
        if (sampleFormat != nullptr) *sampleFormat = format;
        return n;
    }
    std::vector<fx_rtp_stats> rtpStats() const
    {
        std::vector<fx_rtp_stats> stats ((std::size_t) rtpStreams);       // (not configured: no streams, and the entry says so)
        if (rtpStreams == 0) throw Error (FX_ERR_INVALID_ARGUMENT, "RTP input is not configured (rtpConfigure)");
        check (fx_rtp_get_stats (ctx, stats.data()));
        return stats;
    }
    // the reorder window (fx.h, "the RTP reorder window"): what a tick's packets own up to `window` sample times beyond the tick is
    // held on the device for the tick that covers it, so a packet is pushed once, when it arrives.  Discards everything held; 0: none.
    void setRtpWindow (int window) { check (fx_rtp_set_window (ctx, window)); }
    // -> the window; stats (optional): per stream, the positions held now and the block positions recovered from the held state
    int rtpWindow (std::vector<fx_rtp_window_stats>* stats = nullptr) const
    {
        int window = 0;
        if (stats != nullptr) stats->resize ((std::size_t) rtpStreams);
        check (fx_rtp_get_window (ctx, &window, stats != nullptr && rtpStreams > 0 ? stats->data() : nullptr));
        return window;
    }

    // The analysers' display buffers (fx_request_taps / fx_get_taps): what RealTimeAudioDataOverlapper, both FFTAnalysers and the
    // PitchAnalyser hand out after their enable...NeedsUpdating flags (RealTimeAudioAnalysis.h:221-232,268-283, PitchAnalyser.h:30-72).
    // requestDisplayBuffers arms every flag of these channels; the next analysis call that analyses a frame captures its first frame.
    struct DisplayBuffers
    {
        std::vector<float> bufferToDraw;                      // [N]  getBufferToDraw
        std::vector<float> fftBufferToDraw;                   // [2N] the spectral analyser's getFFTBufferToDraw
        std::vector<float> pitchFFTBufferToDraw;              // [2N] the harmonic analyser's getFFTBufferToDraw
        std::vector<float> autoCorrelationBufferToDraw;       // [N]  getAutoCorrelationBufferToDraw
        std::vector<float> cumulativeDifferenceBufferToDraw;  // [N]  getCumulativeDifferenceBufferToDraw
        float normalisedLagPosition[2];                       // getNormalisedLagPosition (x, y)
        long long frameIndex;                                 // which frame of the channel's stream was captured
    };
    void requestDisplayBuffers (std::vector<int> channelsToArm)
    {
        check (fx_request_taps (ctx, channelsToArm.data(), (int) channelsToArm.size()));
    }
    DisplayBuffers getDisplayBuffers (int channel)
    {
        DisplayBuffers b;
        b.bufferToDraw.resize ((size_t) window);
        b.fftBufferToDraw.resize (2 * (size_t) window);
        b.pitchFFTBufferToDraw.resize (2 * (size_t) window);
        b.autoCorrelationBufferToDraw.resize ((size_t) window);
        b.cumulativeDifferenceBufferToDraw.resize ((size_t) window);
        b.frameIndex = -1;
        check (fx_get_taps (ctx, channel, b.bufferToDraw.data(), b.fftBufferToDraw.data(), b.pitchFFTBufferToDraw.data(),
                            b.autoCorrelationBufferToDraw.data(), b.cumulativeDifferenceBufferToDraw.data(), b.normalisedLagPosition,
                            &b.frameIndex));
        return b;
    }

    // The onset callback of every track as one list (fx_enable_onset_events / fx_get_onset_events): the reference's analysis thread
    // calls onsetDetectedCallback() after a frame whose onset slot is above zero (RealTimeAnalyser.h:228-229, :256), one callback
    // per track (AnalyserTrackController.h:80-84).  Once enabled, every analysis call appends its (track, frame) onsets on the GPU,
    // in (frame, track) order; getOnsetEvents drains what is stored (all of it) and reports what overflowed since the last drain.
    void enableOnsetEvents (int capacity)                       { check (fx_enable_onset_events (ctx, capacity)); }
    std::vector<fx_onset_event> getOnsetEvents (long long* droppedSinceLastCall = nullptr)
    {
        int stored = 0, got = 0;
        long long lost = 0;
        check (fx_get_onset_events (ctx, nullptr, 0, &stored, nullptr));
        std::vector<fx_onset_event> events ((std::size_t) (stored > 0 ? stored : 1));
        check (fx_get_onset_events (ctx, events.data(), stored, &got, &lost));
        events.resize ((std::size_t) got);
        if (droppedSinceLastCall != nullptr) *droppedSinceLastCall = lost;
        return events;
    }

    // The scrolling audio display of every track (fx_enable_display / fx_get_display): the AudioVisualiserComponent the reference
    // feeds with every gained hop (AnalyserTrackController.h:74-78, AnalyserTrack.h:27-29,148-157), kept on the GPU.  Once enabled,
    // every analysis call folds its hops into the tracks' (lo, hi) levels; getDisplayLevels returns the listed tracks' rings (an
    // empty list: all tracks) in drawing order, oldest first, [tracks][bufferSize][2].
    void enableDisplay (int samplesPerBlock = 256, int bufferSize = 1024)
    {
        check (fx_enable_display (ctx, samplesPerBlock, bufferSize));
        displayLength = bufferSize;
    }
    void setSamplesPerBlock (int samplesPerBlock)               { check (fx_set_display_samples_per_block (ctx, samplesPerBlock)); }   // ref AnalyserTrackController.h:154-158
    void clearDisplay (const std::vector<int>& tracks)          { check (fx_clear_display_channels (ctx, tracks.data(), (int) tracks.size())); }   // ref :105,114
    std::vector<float> getDisplayLevels (const std::vector<int>& tracks = {})
    {
        const int n = tracks.empty() ? channels : (int) tracks.size();
        std::vector<float> levels ((std::size_t) n * (std::size_t) displayLength * 2 + 1);      // (never a null pointer)
        check (fx_get_display (ctx, tracks.empty() ? nullptr : tracks.data(), n, levels.data(), FX_MEM_HOST));
        levels.resize (levels.size() - 1);
        return levels;
    }

    // hops [channels][numHops][window/2] host floats -> raw / smoothed [channels][numHops][12]
    void pushHops (const float* hops, int numHops, float* raw, float* smoothed)
    {
        check (fx_push_hops (ctx, hops, numHops, FX_SAMPLE_F32, FX_MEM_HOST, raw, smoothed));
    }
    // the same hops as 16-bit PCM (FX_SAMPLE_S16: v / 32768 in the kernels' load stage -- what JUCE's WAV reader makes of a 16-bit
    // file before AudioDataCollector sees it, ref AudioFilePlayer.h:41-61): half the bytes across PCIe, the same bits out
    void pushHopsPCM16 (const std::int16_t* hops, int numHops, float* raw, float* smoothed)
    {
        check (fx_push_hops (ctx, hops, numHops, FX_SAMPLE_S16, FX_MEM_HOST, raw, smoothed));
    }
    // ... and as packed 24-bit PCM, three bytes per sample, little endian (FX_SAMPLE_S24: v / 8388608)
    void pushHopsPCM24 (const unsigned char* hops, int numHops, float* raw, float* smoothed)
    {
        check (fx_push_hops (ctx, hops, numHops, FX_SAMPLE_S24, FX_MEM_HOST, raw, smoothed));
    }
    void processFrames (const float* frames, int numFrames, float* raw, float* smoothed)
    {
        check (fx_process_frames (ctx, frames, numFrames, FX_SAMPLE_F32, FX_MEM_HOST, raw, smoothed));
    }
    // device-resident variants (pointers from hipMalloc); asynchronous until sync()
    void pushHopsDevice (const void* hops, int numHops, int sampleFormat, float* raw, float* smoothed)
    {
        check (fx_push_hops (ctx, hops, numHops, sampleFormat, FX_MEM_DEVICE, raw, smoothed));
    }
    void sync() { check (fx_sync (ctx)); }

    // latest AudioFeatures::getValue of every slot of one channel, as the OSC timer would read them
    std::vector<float> getValues (int channel)
    {
        latest.resize ((std::size_t) channels * FX_NUM_FEATURES);
        check (fx_get_smoothed (ctx, latest.data(), FX_MEM_HOST));
        return std::vector<float> (latest.begin() + (std::ptrdiff_t) channel * FX_NUM_FEATURES,
                                   latest.begin() + (std::ptrdiff_t) (channel + 1) * FX_NUM_FEATURES);
    }
    float getValue (int channel, AudioFeatures::eAudioFeature f) { return getValues (channel)[(std::size_t) f]; }

    // launch-shape knobs (struct fx_tuning of fx.h).  No knob changes a result bit within a kernel family; the family itself is a
    // constructor flag (FX_LOW_LATENCY: every frame on a pair of wavefronts, the lower one-hop latency at 2048 / 4096 points).
    fx_tuning getTuning()                  { fx_tuning t; check (fx_get_tuning (ctx, &t)); return t; }
    void setTuning (const fx_tuning& t)    { check (fx_set_tuning (ctx, &t)); }

    int getNumChannels() const { return channels; }
    int getWindowSize() const  { return window; }
    fx_context* handle()       { return ctx; }

private:
    std::size_t at (int track) const
    {
        if (track < 0 || track >= channels) throw Error (FX_ERR_INVALID_ARGUMENT, "no such track");
        return (std::size_t) track;
    }
    fx_context* ctx = nullptr;
    int channels, window;
    std::vector<int> channelMap;             // [track]: what fx_set_channel_map was last given (the identity by default)
    int highestSource = channels - 1;
    int displayLength = 0;                   // levels per track of the audio display (0: not enabled)
    int rtpStreams = 0;                      // streams of the RTP unit (0: not configured)
    std::vector<float> latest;
};

// AudioDataCollector, ref Source/AudioDataCollector.h:18-138, for every channel of a RealTimeBatchAnalyser at once.  The reference's
// collector copies each device block -- whatever length the audio device delivers -- into a 4096-sample ring and notifies the analysis
// thread, which reads window/2 samples (times the gain) whenever they are there (:36-94).  Here audioDeviceIOCallback hands the block of
// all channels to fx_push_samples: the library keeps what is left over (< window/2 samples per channel, in device memory), analyses the
// hops that completed and the frames' values are handed to the callback the analysis threads' updateFeature calls stood for.
class AudioDataCollector
{
public:
    explicit AudioDataCollector (RealTimeBatchAnalyser& analyserToFeed)
        : analyser (analyserToFeed), channels (analyserToFeed.getNumChannels()), hop (analyserToFeed.getWindowSize() / 2) {}

    // ref :36-70.  inputChannelData[k] points at `numberOfSamples` floats of device channel k (JUCE's layout); track c collects
    // inputChannelData[channel c collects] (setChannelToCollect; by default track c <- channel c).  Returns the number of analysis
    // frames per channel this block completed (0 is normal for blocks shorter than a hop).  Their values: raw() / smoothed(),
    // [channel][frame][12], and the callback set below is called once per block that completed at least one frame.
    int audioDeviceIOCallback (const float* const* inputChannelData, int numInputChannels, int numberOfSamples)
    {
        const int highest = analyser.getHighestSourceChannel();
        if (numInputChannels <= highest)                                                                          // jassert, :44-47
            throw Error (FX_ERR_INVALID_ARGUMENT, ((highest == channels - 1 ? std::string ("fewer input channels than the analyser has")
                                                                            : std::string ("fewer input channels than the channel map reads"))
                                                  + " (it collects input channel " + std::to_string (highest) + ", the device gives "
                                                  + std::to_string (numInputChannels) + ")").c_str());
        const std::vector<int>& map = analyser.getChannelMap();
        block.resize ((std::size_t) channels * (std::size_t) numberOfSamples);
        for (int c = 0; c < channels; ++c)
            if (numberOfSamples > 0) std::memcpy (block.data() + (std::size_t) c * (std::size_t) numberOfSamples, inputChannelData[map[(std::size_t) c]], sizeof (float) * (std::size_t) numberOfSamples);
        return pushBlock (block.data(), numberOfSamples, FX_SAMPLE_F32);
    }
    // ref :123: track `track` collects device channel `source` from the next block on (pending samples are kept).  The map is the
    // context's (fx_set_channel_map): pushInterleaved reads it on the GPU, audioDeviceIOCallback on the host.
    void setChannelToCollect (int track, int source)
    {
        if (track < 0 || track >= channels || source < 0) throw Error (FX_ERR_INVALID_ARGUMENT, "no such track, or a negative channel");
        std::vector<int> map = analyser.getChannelMap();
        map[(std::size_t) track] = source;
        analyser.setChannelMap (map);
    }
    int getChannelToCollect (int track) const { return analyser.getChannelMap().at ((std::size_t) track); }
    // an interleaved block as a device or file delivers it: `frames` holds numberOfSamples frames of numSourceChannels samples in
    // sampleFormat ([frame][source]; 3 bytes per sample for FX_SAMPLE_S24), de-interleaved on the GPU (fx_push_interleaved)
    int pushInterleaved (const void* frames, int numSourceChannels, int numberOfSamples, int sampleFormat = FX_SAMPLE_F32)
    {
        const std::size_t most = (std::size_t) ((fx_pending_samples (analyser.handle()) + numberOfSamples) / hop);
        rawValues.resize ((std::size_t) channels * most * FX_NUM_FEATURES);
        smoothedValues.resize (rawValues.size());
        int got = 0;
        check (fx_push_interleaved (analyser.handle(), frames, numberOfSamples, numSourceChannels, sampleFormat, FX_MEM_HOST,
                                    most ? rawValues.data() : nullptr, most ? smoothedValues.data() : nullptr, &got));
        lastFrames = got;
        if (got > 0 && framesAnalysed) framesAnalysed (got);
        if (got > 0) reportOnsets();
        return got;
    }
    // the same for a block that is already [channel][numberOfSamples] in one piece, in any sample format of fx.h
    int pushBlock (const void* samples, int numberOfSamples, int sampleFormat = FX_SAMPLE_F32)
    {
        const std::size_t most = (std::size_t) ((fx_pending_samples (analyser.handle()) + numberOfSamples) / hop);
        rawValues.resize ((std::size_t) channels * most * FX_NUM_FEATURES);
        smoothedValues.resize (rawValues.size());
        int frames = 0;
        check (fx_push_samples (analyser.handle(), samples, numberOfSamples, sampleFormat, FX_MEM_HOST,
                                most ? rawValues.data() : nullptr, most ? smoothedValues.data() : nullptr, &frames));
        lastFrames = frames;
        if (frames > 0 && framesAnalysed) framesAnalysed (frames);      // where the reference calls notifyAnalysisThread(), :68-69
        if (frames > 0) reportOnsets();
        return frames;
    }
    // one tick of a context whose tracks listen to the device or to their AudioFilePlayer (below; fx_push_sources): `liveBlock` is the
    // block pushBlock takes -- read by the tracks whose source is the input, and may be null while there is none -- and every track
    // that plays a file gets its clip's next numberOfSamples samples on the GPU
    int pushSources (const void* liveBlock, int numberOfSamples, int sampleFormat = FX_SAMPLE_F32)
    {
        const std::size_t most = (std::size_t) ((fx_pending_samples (analyser.handle()) + numberOfSamples) / hop);
        rawValues.resize ((std::size_t) channels * most * FX_NUM_FEATURES);
        smoothedValues.resize (rawValues.size());
        int frames = 0;
        check (fx_push_sources (analyser.handle(), liveBlock, numberOfSamples, sampleFormat, FX_MEM_HOST,
                                most ? rawValues.data() : nullptr, most ? smoothedValues.data() : nullptr, &frames));
        lastFrames = frames;
        if (frames > 0 && framesAnalysed) framesAnalysed (frames);
        if (frames > 0) reportOnsets();
        return frames;
    }
    void setNotifyAnalysisThreadCallback (std::function<void (int)> f)  { framesAnalysed = f; }    // ref :107 (argument: frames per channel)
    // The tracks' onsetDetectedCallback (RealTimeAnalyser.h:256, AnalyserTrackController.h:80-84) as one callback: after each block
    // that completed frames it is called once per (track, frame) whose onset slot is 1, in (frame, track) order.  Setting it enables
    // the analyser's onset event list (room for `capacity` events between two blocks; what does not fit is lost and counted by the list).
    void setOnsetDetectedCallback (std::function<void (int track, long long frame)> f, int capacity = 1 << 16)
    {
        onsetDetected = f;
        analyser.enableOnsetEvents (f ? capacity : 0);
        drainOnsets = [this] { return analyser.getOnsetEvents(); };
    }
    void setGain (float g)       { analyser.setGain (g); }                                          // ref :124
    void clearBuffer()           { check (fx_clear_pending (analyser.handle())); }                  // ref :122
    void clearBuffer (int track) { check (fx_clear_pending_channels (analyser.handle(), &track, 1)); }   // one track's collector (AnalyserTrackController.h:135-137)
    int  getNumPendingSamples()  { return fx_pending_samples (analyser.handle()); }
    int  getNumFrames() const    { return lastFrames; }
    const float* raw() const      { return rawValues.data(); }        // [channel][getNumFrames()][12] of the last block
    const float* smoothed() const { return smoothedValues.data(); }

private:
    void reportOnsets()
    {
        // (through drainOnsets: a host that never sets the callback needs no symbol of the event list from the library)
        if (! onsetDetected || ! drainOnsets) return;
        for (const fx_onset_event& e : drainOnsets()) onsetDetected (e.channel, e.frame);
    }
    RealTimeBatchAnalyser& analyser;
    int channels, hop, lastFrames = 0;
    std::vector<float> block, rawValues, smoothedValues;
    std::function<void (int)> framesAnalysed;
    std::function<void (int, long long)> onsetDetected;
    std::function<std::vector<fx_onset_event>()> drainOnsets;
};

// AudioFilePlayer, ref Source/AudioFilePlayer.h:41-67 with the file half of AnalyserTrackController.h:92-138, for a SET of tracks of a
// RealTimeBatchAnalyser: the tracks' players are rows of the context's transport table (fx.h, file sources), their files clips in
// device memory.  One object per track is the reference's shape; one object for a group that is started and stopped together costs
// one launch per command instead of one per track.  The audio itself moves in AudioDataCollector::pushSources, once per tick for the
// whole context.  As in the reference the transport buttons clear the tracks' collectors (play, pause, stop; not restart), and
// restart keeps the state (AudioFilePlayer.h:65).  Differences from the reference are those fx.h lists: no fade, a resampler of our own,
// a track hears its own player until it is told to listen to the monitor output (toggleCollectInput); one-shot playback
// (setLooping (false)) ends in FX_TRANSPORT_FINISHED.
class AudioFilePlayer
{
public:
    AudioFilePlayer (RealTimeBatchAnalyser& analyserToPlayInto, std::vector<int> tracksToPlay)
        : analyser (analyserToPlayInto), tracks (std::move (tracksToPlay)), clipOf (tracks.size(), -1) {}

    // Files for any player of the context: `lengths.size()` clips back to back in host memory -> the first clip's id (fx_create_clips).
    // `sampleRates`: the files' own rates in Hz, one per clip (the reader->sampleRate the reference hands to setSource "for sample
    // rate correction", ref AudioFilePlayer.h:55-58); empty or 0: the context's rate.
    int createClips (const void* samples, const std::vector<long long>& lengths, int sampleFormat = FX_SAMPLE_F32,
                     const std::vector<double>& sampleRates = std::vector<double>())
    {
        if (! sampleRates.empty() && sampleRates.size() != lengths.size()) throw Error (FX_ERR_INVALID_ARGUMENT, "one sample rate per clip");
        int first = -1;
        check (fx_create_clips (analyser.handle(), samples, lengths.data(), (int) lengths.size(), sampleFormat, FX_MEM_HOST, 0, &first));
        if (! sampleRates.empty())
        {
            std::vector<int> ids (lengths.size());
            for (std::size_t i = 0; i < ids.size(); ++i) ids[i] = first + (int) i;
            setClipRates (ids, sampleRates);
        }
        return first;
    }
    // fx_set_clip_rates: refused while a listed clip is loaded on a track -- the rate is the file's and is set before loading
    void setClipRates (const std::vector<int>& clipIds, const std::vector<double>& sampleRates)
    {
        if (clipIds.size() != sampleRates.size()) throw Error (FX_ERR_INVALID_ARGUMENT, "one sample rate per clip");
        check (fx_set_clip_rates (analyser.handle(), clipIds.data(), (int) clipIds.size(), sampleRates.data()));
    }
    void destroyClips (int firstId) { check (fx_destroy_clips (analyser.handle(), firstId)); }

    // ref AudioFilePlayer.h:41-57 (and the file-dropped callback, AnalyserTrackController.h:109-124): every track of the set loads
    // clipIds[i] (one id: all load the same clip; -1: no file), looping as the reference's reader source does unless told otherwise.
    // The tracks stop at position 0 and their collectors are cleared.
    void loadFileIntoTransport (const std::vector<int>& clipIds, bool looping = true)
    {
        if (clipIds.size() != tracks.size() && clipIds.size() != 1) throw Error (FX_ERR_INVALID_ARGUMENT, "one clip per track of the player, or one for all");
        std::vector<int> ids (tracks.size()), loop (tracks.size(), looping ? 1 : 0);
        for (std::size_t i = 0; i < tracks.size(); ++i) ids[i] = clipIds[clipIds.size() == 1 ? 0 : i];
        check (fx_set_channel_clips (analyser.handle(), tracks.data(), (int) tracks.size(), ids.data(), loop.data()));
        clipOf = ids;
    }
    void loadFileIntoTransport (int clipId, bool looping = true) { loadFileIntoTransport (std::vector<int> (1, clipId), looping); }
    bool hasFile() const                                                                            // ref :67: every track of the set has one
    {
        for (int id : clipOf) if (id < 0) return false;
        return ! clipOf.empty();
    }
    // AnalyserTrackController.h:92-107: the tracks listen to their player (true) or to the audio device (false, which stops the player)
    void setFileSource (bool listenToFile)
    {
        const std::vector<int> types (tracks.size(), listenToFile ? FX_SOURCE_FILE : FX_SOURCE_INPUT);
        check (fx_set_channel_sources (analyser.handle(), tracks.data(), (int) tracks.size(), types.data()));
    }
    void play()    { command (FX_PLAY); }                       // ref :59-63; refused (fx::Error) while a track of the set has no file
    void pause()   { command (FX_PAUSE); }
    void stop()    { command (FX_STOP); }
    void restart() { command (FX_RESTART); }                    // ref :65: position 0, the state kept

    struct Transport { std::vector<int> source, state; std::vector<long long> position, laps; };   // one entry per track of the set
    Transport getTransport() const
    {
        const std::size_t all = (std::size_t) analyser.getNumChannels();
        std::vector<int> source (all), state (all);
        std::vector<long long> position (all), laps (all);
        check (fx_get_transport (analyser.handle(), source.data(), state.data(), position.data(), laps.data()));
        Transport t;
        for (int c : tracks) {
            t.source.push_back (source[(std::size_t) c]); t.state.push_back (state[(std::size_t) c]);
            t.position.push_back (position[(std::size_t) c]); t.laps.push_back (laps[(std::size_t) c]);
        }
        return t;
    }
    const std::vector<int>& getTracks() const { return tracks; }

    // ref AudioFilePlayer.h:30-34: the player is an AudioSourcePlayer on the device manager, so the file is HEARD.  Here that is the
    // context's monitor mix (fx.h, monitor mix): every pushSources tick also sums the tracks whose send is on to a stereo output in
    // device memory.  The monitor is the context's, the sends are these tracks'; the collector's gain does not change what is heard.
    void enableMonitor (bool enable = true) { check (fx_enable_monitor (analyser.handle(), enable ? 1 : 0)); }
    // the set's sends on or off, and -- where given, one per track of the set or one for all -- their left / right gains
    void setMonitor (bool on, const std::vector<float>& left = std::vector<float>(), const std::vector<float>& right = std::vector<float>())
    {
        const std::vector<int> flags (tracks.size(), on ? 1 : 0);
        const std::vector<float> l = perTrack (left), r = perTrack (right);
        check (fx_set_channel_monitor (analyser.handle(), tracks.data(), (int) tracks.size(), flags.data(),
                                       left.empty() ? nullptr : l.data(), right.empty() ? nullptr : r.data()));
    }
    struct Sends { std::vector<int> on; std::vector<float> left, right; };                         // one entry per track of the set
    Sends getMonitorSends() const
    {
        const std::size_t all = (std::size_t) analyser.getNumChannels();
        std::vector<int> on (all);
        std::vector<float> left (all), right (all);
        check (fx_get_channel_monitor (analyser.handle(), on.data(), left.data(), right.data()));
        Sends s;
        for (int c : tracks) { s.on.push_back (on[(std::size_t) c]); s.left.push_back (left[(std::size_t) c]); s.right.push_back (right[(std::size_t) c]); }
        return s;
    }
    // the last tick's mix of the whole context: `left` and `right` get that tick's samples (what an audio device's output callback
    // copies into its two channels) -> their number, 0 before the first tick
    int getMonitor (std::vector<float>& left, std::vector<float>& right) const
    {
        int n = 0;
        float none = 0.0f;
        const fx_status probe = fx_get_monitor (analyser.handle(), &none, 0, &n, FX_MEM_HOST);      // (no room: refused, the count reported)
        if (probe != FX_OK && n == 0) check (probe);
        std::vector<float> both (2 * (std::size_t) n);
        if (n > 0) check (fx_get_monitor (analyser.handle(), both.data(), n, &n, FX_MEM_HOST));
        left.assign (both.begin(), both.begin() + n);
        right.assign (both.begin() + n, both.end());
        return n;
    }

    // ref AudioDataCollector.h:42,53,119 (fx.h, listening tracks): the set's analysers hear their own rows (FX_LISTEN_SELF) or one
    // output of the monitor mix (FX_LISTEN_LEFT / FX_LISTEN_RIGHT), from the next tick on; the collectors are cleared either way.
    // Needs the monitor (enableMonitor).
    void setListen (int output)
    {
        const std::vector<int> listen (tracks.size(), output);
        check (fx_set_channel_listen (analyser.handle(), tracks.data(), (int) tracks.size(), listen.data()));
    }
    std::vector<int> getListens() const                                                             // one entry per track of the set
    {
        std::vector<int> all ((std::size_t) analyser.getNumChannels()), mine;
        check (fx_get_channel_listen (analyser.handle(), all.data()));
        for (int c : tracks) mine.push_back (all[(std::size_t) c]);
        return mine;
    }
    // What the reference's source-type callback does (AnalyserTrackController.h:92-107).  true: the tracks collect the audio device's
    // input -- their source is the input (which stops their players) and they hear their own rows.  false: their source is the file
    // and, as the reference's collectors do from then on, they hear channel `outputChannel` (0 left, 1 right) of the device's output,
    // the monitor mix.  A context without a monitor can only go to the input.
    void toggleCollectInput (bool shouldCollectInput, int outputChannel = 0)
    {
        if (! shouldCollectInput && outputChannel != 0 && outputChannel != 1) throw Error (FX_ERR_INVALID_ARGUMENT, "the monitor has output channels 0 and 1");
        if (! shouldCollectInput)
        {
            setListen (outputChannel == 0 ? FX_LISTEN_LEFT : FX_LISTEN_RIGHT);                       // (refused without a monitor, before the source changes)
            setFileSource (true);
            return;
        }
        setFileSource (false);
        std::vector<int> all ((std::size_t) analyser.getNumChannels());
        if (fx_get_channel_listen (analyser.handle(), all.data()) == FX_OK) setListen (FX_LISTEN_SELF);     // (no monitor: nobody listens)
    }

private:
    std::vector<float> perTrack (const std::vector<float>& gains) const
    {
        if (! gains.empty() && gains.size() != tracks.size() && gains.size() != 1) throw Error (FX_ERR_INVALID_ARGUMENT, "one gain per track of the player, or one for all");
        std::vector<float> v (tracks.size(), gains.size() == 1 ? gains[0] : 0.0f);
        if (gains.size() == tracks.size()) v = gains;
        return v;
    }
    void command (int which) { check (fx_transport (analyser.handle(), tracks.data(), (int) tracks.size(), which)); }
    RealTimeBatchAnalyser& analyser;
    std::vector<int> tracks, clipOf;
};

// The stand-in for AudioDataCollector's ring (ref Source/AudioDataCollector.h:24,36-94: the audio thread writes a ring, the analysis thread
// spins until a hop is there) for hosts that batch: a ring of pinned host batches of `hopsPerBatch` hops per channel (fx_stream_*).  The producer writes into
// nextSlot() and submit()s it -- or push()es a batch from ordinary memory, copied by `fillThreads` host threads inside the library --
// and collect()s the results in submission order; samples in, kernels and results back overlap.  One hop per batch is the reference's
// own cadence: a submit is then ONE kernel launch and collect() polls a flag (32-33 us round trip for a 4096-point window on MI355X).
// Destroy the ring before its analyser.
class HopRing
{
public:
    HopRing (RealTimeBatchAnalyser& analyser, int hopsPerBatch, int slots = 3, int sampleFormat = FX_SAMPLE_F32)
        : values ((std::size_t) analyser.getNumChannels() * (std::size_t) hopsPerBatch * FX_NUM_FEATURES)
    {
        check (fx_stream_create (analyser.handle(), hopsPerBatch, slots, sampleFormat, &ring));
    }
    ~HopRing() { fx_stream_destroy (ring); }
    HopRing (const HopRing&) = delete;
    HopRing& operator= (const HopRing&) = delete;

    void* nextSlot()                                   { void* p = nullptr; check (fx_stream_acquire (ring, &p)); return p; }
    void submit()                                      { check (fx_stream_submit (ring)); }
    void push (const void* hops, int fillThreads = 1)  { check (fx_stream_push (ring, hops, fillThreads)); }
    // a block of ANY length up to a slot's capacity, [channels][numSamples] (fx_stream_submit_samples / fx_stream_push_samples)
    void submitSamples (int numSamples)                { check (fx_stream_submit_samples (ring, numSamples)); }
    void pushSamples (const void* samples, int numSamples, int fillThreads = 1) { check (fx_stream_push_samples (ring, samples, numSamples, fillThreads)); }
    int  collectSamples (float* raw, float* smoothed)  { int frames = 0; check (fx_stream_collect_samples (ring, raw, smoothed, &frames)); return frames; }
    int  inFlight() const                              { return fx_stream_in_flight (ring); }
    // the oldest batch's values: raw / smoothed [channels][hopsPerBatch][12], either may be null
    void collect (float* raw, float* smoothed)         { check (fx_stream_collect (ring, raw, smoothed)); }
    std::size_t valuesPerBatch() const                 { return values; }

private:
    fx_stream* ring = nullptr;
    std::size_t values;
};

// The reference's LEGACY offline analyser (struct AudioAnalyser, ref Source/AudioAnalysis.h), one per channel, on the GPU: the
// members a host would have called, with the reference's names.  Buffers are host memory, [numChannels][...] row-major.
class AudioAnalyser
{
public:
    struct HarmonicCharacteristics { float f0, harmonicEnergyRatio, inharmonicity; };     // ref AudioAnalysis.h:31-42

    AudioAnalyser (int numberOfChannels, double nyquistFrequency, int deviceId = 0) : channels (numberOfChannels)   // ref :107
    {
        check (fx_offline_create (&off, deviceId, numberOfChannels, nyquistFrequency));
    }
    ~AudioAnalyser() { fx_offline_destroy (off); }
    AudioAnalyser (const AudioAnalyser&) = delete;
    AudioAnalyser& operator= (const AudioAnalyser&) = delete;

    // ref :517-541: audio [channels][numSamples] -> the ZeroCrosses feature row [channels][numDownsamples]
    std::vector<float> analyseNormalisedZeroCrosses (const float* audio, int numSamples, int numDownsamples)
    {
        std::vector<float> out ((std::size_t) channels * numDownsamples);
        check (fx_offline_zero_crosses (off, audio, numSamples, numDownsamples, out.data(), FX_MEM_HOST));
        return out;
    }
    // ref :611-622: channel 0 of the energy envelope -> estimatedLogAttackTime
    float setLogAttackTime (const float* energyEnvelope, int numEnvelopeSamples, int numInputSamples, int numDownsamples, int sampleRate)
    {
        float v = 0.0f;
        check (fx_offline_log_attack_time (off, energyEnvelope, numEnvelopeSamples, numInputSamples, numDownsamples, sampleRate, &v, FX_MEM_HOST));
        return v;
    }
    // ref :543-564 (the reference prints these): bits [channels][numBins], the last bin over the threshold / numBins, the share of bins over it
    void calculateFFTLBP (const float* fftResults, const float* previousFFTFrame, int numBins, unsigned char* bits, float* highestRatio, float* activityRatio)
    {
        check (fx_offline_fft_lbp (off, fftResults, previousFFTFrame, numBins, bits, highestRatio, activityRatio, FX_MEM_HOST));
    }
    // ref :253-303: magnitudes [channels][numBins] of one frame; previousF0 is kept per channel across calls
    std::vector<HarmonicCharacteristics> calculateHarmonicCharacteristics (const float* fftResults, int numBins)
    {
        std::vector<float> raw ((std::size_t) channels * 3);
        check (fx_offline_harmonic_characteristics (off, fftResults, numBins, raw.data(), FX_MEM_HOST));
        std::vector<HarmonicCharacteristics> out ((std::size_t) channels);
        for (int c = 0; c < channels; c++) out[(std::size_t) c] = { raw[3 * (std::size_t) c], raw[3 * (std::size_t) c + 1], raw[3 * (std::size_t) c + 2] };
        return out;
    }
    // ref :463-515 (legacy full-spectrum form): magnitudes [channels][numBins] -> per channel centroid / nyquist, spread, flatness, flux;
    // previousBinMagnitudes is kept per channel across calls
    struct SpectralCharacteristics { float centroid, spread, flatness, flux; };             // ref AudioAnalysis.h:17-29
    std::vector<SpectralCharacteristics> calculateSpectralCharacteristics (const float* fftResults, int numBins)
    {
        std::vector<float> raw ((std::size_t) channels * 4);
        check (fx_offline_spectral_characteristics (off, fftResults, numBins, raw.data(), FX_MEM_HOST));
        std::vector<SpectralCharacteristics> out ((std::size_t) channels);
        for (int c = 0; c < channels; c++) out[(std::size_t) c] = { raw[4 * (std::size_t) c], raw[4 * (std::size_t) c + 1], raw[4 * (std::size_t) c + 2], raw[4 * (std::size_t) c + 3] };
        return out;
    }
    // ref :566-609
    std::vector<float> calculateNormalisedSpectralSlope (const float* fftResults, int numBins)
    {
        std::vector<float> out ((std::size_t) channels);
        check (fx_offline_spectral_slope (off, fftResults, numBins, out.data(), FX_MEM_HOST));
        return out;
    }
    // ref :623-665: data [channels][numItems] (r, i) pairs, replaced in place by item x conjugate; returns the frequency estimates the reference prints
    std::vector<double> analyseAutoCorrelation (float* data, int numItems, std::vector<int>* peakBins = nullptr)
    {
        std::vector<int> peaks ((std::size_t) channels);
        std::vector<double> freqs ((std::size_t) channels);
        check (fx_offline_auto_correlation (off, data, numItems, peaks.data(), freqs.data(), FX_MEM_HOST));
        if (peakBins != nullptr) *peakBins = peaks;
        return freqs;
    }
    // ref AudioFeatures.h:208-213, per row and channel: rows [numRows][channels][numDownsamples] -> [numRows][channels][2] = (start, end)
    std::vector<float> getFeatureRanges (const float* rows, int numRows, int numDownsamples)
    {
        std::vector<float> out ((std::size_t) numRows * channels * 2);
        check (fx_offline_feature_ranges (off, rows, numRows, numDownsamples, out.data(), FX_MEM_HOST));
        return out;
    }
    // ref AudioFeatures.h:215-240, per row and channel: -> [numRows][channels][numBrackets]
    std::vector<float> getDiscreteFeatureDistribution (const float* rows, int numRows, int numDownsamples, int numBrackets)
    {
        std::vector<float> out ((std::size_t) numRows * channels * (std::size_t) (numBrackets > 0 ? numBrackets : 0));
        check (fx_offline_feature_distribution (off, rows, numRows, numDownsamples, numBrackets, out.data(), FX_MEM_HOST));
        return out;
    }
    fx_offline* handle() { return off; }

private:
    fx_offline* off = nullptr;
    int channels;
};

// JUCE's Range<float> as far as FeatureSpace uses it: the constructor keeps end >= start, and each setter moves the other end along.
class Range
{
public:
    Range() = default;
    Range (float rangeStart, float rangeEnd) : start (rangeStart), end (rangeEnd < rangeStart ? rangeStart : rangeEnd) {}
    float getStart() const { return start; }
    float getEnd() const { return end; }
    void setStart (float newStart) { start = newStart; if (end < newStart) end = newStart; }
    void setEnd (float newEnd) { end = newEnd; if (newEnd < start) start = newEnd; }

private:
    float start = 0.0f, end = 0.0f;
};

// ref Source/AudioFeatures.h:319-349: four ranges that describe a file, folded over a corpus by compareAndUpdateRanges.  A handful of
// floats per file, so it stays on the host; fx_offline_feature_ranges feeds it (fromRanges).
struct FeatureSpace
{
    FeatureSpace() = default;
    FeatureSpace (float attack, Range centroidRange, Range slopeRange, Range crossesRange)                  // ref :327-335
    :   attackRange (Range (attack, 0.0f)), spectralCentroidRange (centroidRange), spectralSlopeRange (slopeRange), zeroCrossesRange (crossesRange)
    {}
    // ref :337-343, as written: both tests are `<`, and the setters couple the two ends
    static void compareAndUpdateRanges (Range& existingRange, Range& newRange)
    {
        if (newRange.getStart() < existingRange.getStart()) existingRange.setStart (newRange.getStart());
        if (newRange.getEnd() < existingRange.getEnd()) existingRange.setEnd (newRange.getEnd());
    }
    // one channel (a mono file) of an analysed buffer: ranges [>= FX_OFFLINE_ZERO_CROSSES + 1][numChannels][2] of fx_offline_feature_ranges
    // on fx_offline_analyse's features, logAttackTime [numChannels]
    static FeatureSpace fromRanges (const float* ranges, const float* logAttackTime, int numChannels, int channel)
    {
        auto range = [&] (int row) { const float* p = ranges + ((std::size_t) row * numChannels + channel) * 2; return Range (p[0], p[1]); };
        return FeatureSpace (logAttackTime[channel], range (FX_OFFLINE_CENTROID), range (FX_OFFLINE_SLOPE), range (FX_OFFLINE_ZERO_CROSSES));
    }

    Range attackRange, spectralCentroidRange, spectralSlopeRange, zeroCrossesRange;
};

// The datagram OSCSender::send (bundleAddress, onset, rmsLevel, f0, centroid, slope, spread, flatness,
// ler, flux, her, oer, inharm) emits -- ref Source/OSCFeatureAnalysisOutput.h:107
inline std::string OSCFeatureMessage (const std::string& address, const float* features12)
{
    unsigned char buf[512];
    const int n = fx_osc_encode (address.c_str(), features12, buf, (int) sizeof buf);
    if (n < 0) throw Error (FX_ERR_INVALID_ARGUMENT, "OSC address too long");
    return std::string (reinterpret_cast<const char*> (buf), (std::size_t) n);
}
} // namespace fx

// ---- UDP sender for the feature message (POSIX sockets; ref OSCFeatureAnalysisOutput.h:115-136) ----
#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <unistd.h>

namespace fx
{
class OSCFeatureSender
{
public:
    OSCFeatureSender() = default;
    ~OSCFeatureSender() { if (fd >= 0) ::close (fd); }
    OSCFeatureSender (const OSCFeatureSender&) = delete;
    OSCFeatureSender& operator= (const OSCFeatureSender&) = delete;

    // "ip[:port]", port defaults to 9000 -- same parsing as connectToAddress (ref :115-123)
    bool connectToAddress (const std::string& newAddress)
    {
        int port = 9000;
        const std::size_t sep = newAddress.rfind (':');
        if (sep != std::string::npos) port = std::atoi (newAddress.c_str() + sep + 1);
        const std::string ip = newAddress.substr (0, newAddress.find (':'));
        if (fd < 0) fd = ::socket (AF_INET, SOCK_DGRAM, 0);
        if (fd < 0) return false;
        dest = sockaddr_in();
        dest.sin_family = AF_INET;
        dest.sin_port = htons ((unsigned short) port);
        connected = ::inet_pton (AF_INET, ip.c_str(), &dest.sin_addr) == 1;
        return connected;
    }

    // one sendSpectralFeaturesViaOSC (ref :89-113): features12 in AudioFeatures slot order
    bool send (const std::string& bundleAddress, const float* features12)
    {
        if (! connected) return false;
        const std::string msg = OSCFeatureMessage (bundleAddress, features12);
        return ::sendto (fd, msg.data(), msg.size(), 0, reinterpret_cast<const sockaddr*> (&dest), sizeof dest) == (ssize_t) msg.size();
    }

private:
    int fd = -1;
    bool connected = false;
    sockaddr_in dest {};
};
} // namespace fx

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>

// The device bundle calls live in a library unit of their own (csrc/fx_osc_bundle.hip).  Weak here: OSCBatchSender::updateFromContext
// refers to them, and a host built from the library's host units alone (tests/cpp) still links; there the addresses are null.
extern "C" {
fx_status fx_get_osc_bundles (fx_context*, const char*, int, unsigned long long, int, unsigned char*, int, int*, int) __attribute__ ((weak));
fx_status fx_get_osc_bundles_addressed (fx_context*, unsigned long long, int, unsigned char*, int, int*, int) __attribute__ ((weak));
}

namespace fx
{
// OSCFeatureAnalysisOutput, ref Source/OSCFeatureAnalysisOutput.h:23-145: a 60 Hz timer that reads the track's AudioFeatures::getValue of
// every slot and sends them as one OSC message to ip[:port] (:89-113, :133).  The reference's timer reads the AudioFeatures object the
// analysis threads are writing, unsynchronised; here the analysis side hands over a snapshot -- updateFeatures (smoothed12), the
// `smoothed` vector of the channel's newest frame -- and the timer thread sends the latest snapshot, so a datagram is always the twelve
// values of ONE frame.  One object per track and target, as the reference builds them (AnalyserTrackController.h:22-23: two per track).
// That shape -- a thread, a socket and a system call per track and tick -- is kept for source compatibility and is meant for the
// reference's own scale (up to ~100 tracks); a host with thousands of tracks uses fx::OSCBatchSender below.
class OSCFeatureAnalysisOutput
{
public:
    OSCFeatureAnalysisOutput (const std::string& ip, const std::string& bundle) : bundleAddress (bundle)
    {
        for (float& v : latest) v = 0.0f;
        if (! bundle.empty()) connectToAddress (ip);                                   // ref :79-80
    }
    ~OSCFeatureAnalysisOutput() { stopTimer(); }
    OSCFeatureAnalysisOutput (const OSCFeatureAnalysisOutput&) = delete;
    OSCFeatureAnalysisOutput& operator= (const OSCFeatureAnalysisOutput&) = delete;

    // the analysis side: the smoothed vector (AudioFeatures::getValue of every slot) after the channel's newest frame
    void updateFeatures (const float* smoothed12)
    {
        std::lock_guard<std::mutex> g (lock);
        for (int i = 0; i < FX_NUM_FEATURES; i++) latest[i] = smoothed12[i];
        have = true;
    }
    // ref :89-113: one message with what getValue returns right now (nothing before the first frame: the reference would send 0/0 = NaN)
    bool sendSpectralFeaturesViaOSC()
    {
        float v[FX_NUM_FEATURES];
        {
            std::lock_guard<std::mutex> g (lock);
            if (! have) return false;
            for (int i = 0; i < FX_NUM_FEATURES; i++) v[i] = latest[i];
        }
        if (! sender.send (bundleAddress, v)) return false;
        sent++;
        return true;
    }
    // ref :115-136: "ip[:port]" (port 9000 by default); a successful connect starts the 60 Hz timer
    bool connectToAddress (const std::string& newAddress)
    {
        stopTimer();
        if (! sender.connectToAddress (newAddress)) return false;
        startTimerHz (60);
        return true;
    }
    void startTimerHz (int hz)
    {
        stopTimer();
        running = true;
        timer = std::thread ([this, hz] {
            const std::chrono::nanoseconds period (1000000000ll / (hz > 0 ? hz : 60));
            std::chrono::steady_clock::time_point next = std::chrono::steady_clock::now() + period;
            while (running.load())
            {
                std::this_thread::sleep_until (next);
                next += period;
                if (running.load()) (void) sendSpectralFeaturesViaOSC();                  // timerCallback, ref :84-87
            }
        });
    }
    void stopTimer()
    {
        running = false;
        if (timer.joinable()) timer.join();
    }
    long getNumMessagesSent() const { return sent.load(); }

private:
    OSCFeatureSender sender;
    std::string bundleAddress { "/Audio/Features" };                                    // ref :144
    std::mutex lock;
    float latest[FX_NUM_FEATURES];
    bool have = false;
    std::atomic<bool> running { false };
    std::atomic<long> sent { 0 };
    std::thread timer;
};

// The sink at scale: ONE object for all tracks.  A tick's messages arrive formed -- fx_get_osc_datagrams writes them on the GPU from the
// context's latest vectors, fx_osc_encode_batch on the host -- and go out in sendmmsg batches from `threads` sender threads to a primary
// and an optional secondary target, paced by a 60 Hz timer (ref OSCFeatureAnalysisOutput.h:84-136, AnalyserTrackController.h:22-23).
// A track's own address and targets (the reference's per-track ip, secondaryIP, bundle): setBundleAddresses, setRoutes.
// Thin wrapper of the fx_osc_sender_* entries of include/fx.h.
class OSCBatchSender
{
public:
    OSCBatchSender (const std::string& primary, const std::string& secondary = std::string(), int threads = 1, bool segmentedSends = false)
    {
        check (fx_osc_sender_create (&sender, primary.c_str(), secondary.empty() ? nullptr : secondary.c_str(), threads, segmentedSends ? FX_OSC_SENDER_GSO : 0u));
    }
    ~OSCBatchSender() { fx_osc_sender_destroy (sender); }
    OSCBatchSender (const OSCBatchSender&) = delete;
    OSCBatchSender& operator= (const OSCBatchSender&) = delete;

    // publish formed messages: message i at datagrams + i * stride, messageLengths[i] bytes (copied)
    void updateDatagrams (const unsigned char* datagrams, int stride, const int* messageLengths, int count) { check (fx_osc_sender_update (sender, datagrams, stride, messageLengths, count)); }
    // publish smoothed vectors [count][12] (AudioFeatures slot order) of tracks "<prefix><firstChannel + i>", formed on the host
    void updateFeatures (const std::string& prefix, int firstChannel, const float* smoothed12, int count)
    {
        const int stride = fx_osc_message_bytes (prefix.c_str(), firstChannel + (count > 0 ? count - 1 : 0));
        if (stride < 0) throw Error (FX_ERR_INVALID_ARGUMENT, "OSC prefix too long or a negative channel number");
        if (bundleBytes > 0 && count > 0)
        {
            const int bundles = planBundles (stride, count);
            if (fx_osc_encode_bundles (prefix.c_str(), firstChannel, count, smoothed12, stamp(), bundleBytes, scratch.data(), bundleStride, lengths.data()) != bundles)
                throw Error (FX_ERR_INVALID_ARGUMENT, fx_last_error());
            updateDatagrams (scratch.data(), bundleStride, lengths.data(), bundles);
            return;
        }
        scratch.resize ((std::size_t) count * (std::size_t) stride);
        lengths.resize ((std::size_t) count);
        if (fx_osc_encode_batch (prefix.c_str(), firstChannel, count, smoothed12, scratch.data(), stride, lengths.data()) != count)
            throw Error (FX_ERR_INVALID_ARGUMENT, "fx_osc_encode_batch refused its arguments");
        updateDatagrams (scratch.data(), stride, lengths.data(), count);
    }
    // Every track's own bundleAddress (ref AnalyserTrackController.h:17,146 setBundleAddressChangedCallback): one address per track of
    // the context, or an empty list to go back to "<prefix><channel>".  fx_set_osc_addresses: call it where the context's other calls are
    // made (with a LiveAnalyser: callOnWorker).  From then on updateFromContext publishes the table's messages.
    void setBundleAddresses (fx_context* ctx, const std::vector<std::string>& addresses)
    {
        std::vector<const char*> list;
        for (const std::string& a : addresses) list.push_back (a.c_str());
        check (fx_set_osc_addresses (ctx, list.empty() ? nullptr : list.data()));
        addressStride = &fx_osc_address_stride;                 // (a host that never calls this needs no symbol of the address table)
        addressedDatagrams = &fx_get_osc_datagrams_addressed;
    }
    // Every track's own targets (ref AnalyserTrackController.h:17,22-23 ip / secondaryIP, :140-145 the GUI's two address callbacks):
    // message i goes to targets[primary[i]] and, where secondary[i] >= 0, to targets[secondary[i]] (secondary may be empty: none).
    // An empty target list restores the constructor's pair.  Safe while the timer runs.
    void setRoutes (const std::vector<std::string>& targets, const std::vector<int>& primary, const std::vector<int>& secondary = std::vector<int>())
    {
        if (! secondary.empty() && secondary.size() != primary.size()) throw Error (FX_ERR_INVALID_ARGUMENT, "primary and secondary have one entry per track");
        std::vector<const char*> list;
        for (const std::string& t : targets) list.push_back (t.c_str());
        check (fx_osc_sender_set_routes (sender, list.empty() ? nullptr : list.data(), (int) list.size(), primary.data(),
                                         secondary.empty() ? nullptr : secondary.data(), (int) primary.size()));
    }
    // Bundling (OSC 1.0 #bundle): updateFeatures and updateFromContext publish bundles of at most maxDatagramBytes, about 17 tracks'
    // messages per datagram at 1472, instead of one message per datagram; stampWithNow: the time tag is the time of the publication,
    // else "immediately".  0 = off, the default: the reference's wire format.  Switch it on where the receiver takes bundles (Max,
    // SuperCollider, TouchDesigner, liblo, juce::OSCReceiver all do); routes (setRoutes) are then per bundle.
    void setBundling (int maxDatagramBytes, bool stampWithNow)
    {
        if (maxDatagramBytes < 0 || maxDatagramBytes > 65507) throw Error (FX_ERR_INVALID_ARGUMENT, "bundles of 0 (off) .. 65507 bytes");
        bundleBytes = maxDatagramBytes;
        bundleStamp = stampWithNow;
    }
    // publish the context's latest vectors, formed on the device (the copy to the host is the datagrams): with the addresses of
    // setBundleAddresses where a table is set, else "<prefix><firstChannel + i>"
    void updateFromContext (fx_context* ctx, int numChannels, const std::string& prefix, int firstChannel)
    {
        const int tableStride = addressStride != nullptr ? addressStride (ctx) : -1;
        if (bundleBytes > 0 && numChannels > 0)
        {
            // (weak references, declared above: a host linked without the library's bundle unit gets an Error, not a link failure)
            if (&fx_get_osc_bundles == nullptr || &fx_get_osc_bundles_addressed == nullptr) throw Error (FX_ERR_UNSUPPORTED, "this library has no fx_get_osc_bundles");
            const int longest = tableStride >= 0 ? tableStride : fx_osc_message_bytes (prefix.c_str(), firstChannel + numChannels - 1);
            if (longest < 0) throw Error (FX_ERR_INVALID_ARGUMENT, "OSC prefix too long or a negative channel number");
            const int bundles = planBundles (longest, numChannels);
            if (tableStride >= 0) check (fx_get_osc_bundles_addressed (ctx, stamp(), bundleBytes, scratch.data(), bundleStride, lengths.data(), FX_MEM_HOST));
            else check (fx_get_osc_bundles (ctx, prefix.c_str(), firstChannel, stamp(), bundleBytes, scratch.data(), bundleStride, lengths.data(), FX_MEM_HOST));
            updateDatagrams (scratch.data(), bundleStride, lengths.data(), bundles);
            return;
        }
        if (tableStride >= 0)
        {
            scratch.resize ((std::size_t) numChannels * (std::size_t) tableStride);
            lengths.resize ((std::size_t) numChannels);
            check (addressedDatagrams (ctx, scratch.data(), tableStride, lengths.data(), FX_MEM_HOST));
            updateDatagrams (scratch.data(), tableStride, lengths.data(), numChannels);
            return;
        }
        const int stride = fx_osc_message_bytes (prefix.c_str(), firstChannel + (numChannels > 0 ? numChannels - 1 : 0));
        if (stride < 0) throw Error (FX_ERR_INVALID_ARGUMENT, "OSC prefix too long or a negative channel number");
        scratch.resize ((std::size_t) numChannels * (std::size_t) stride);
        lengths.resize ((std::size_t) numChannels);
        check (fx_get_osc_datagrams (ctx, prefix.c_str(), firstChannel, scratch.data(), stride, lengths.data(), FX_MEM_HOST));
        updateDatagrams (scratch.data(), stride, lengths.data(), numChannels);
    }
    long long sendNow() { long long n = 0; check (fx_osc_sender_send (sender, &n)); return n; }          // one timerCallback for every track
    void startTimerHz (int hz) { check (fx_osc_sender_start (sender, (double) hz)); }                    // ref :133
    void stopTimer() { check (fx_osc_sender_stop (sender)); }
    fx_osc_sender_stats getStats() const { fx_osc_sender_stats st; check (fx_osc_sender_get_stats (sender, &st)); return st; }
    fx_osc_sender* handle() { return sender; }

private:
    // sizes scratch and lengths for the bundles of `count` tracks whose longest message is `longest` bytes; returns their number
    int planBundles (int longest, int count)
    {
        int perBundle = 0, bundles = 0;
        check (fx_osc_bundle_plan (longest, count, bundleBytes, &perBundle, &bundles, &bundleStride));
        scratch.resize ((std::size_t) bundles * (std::size_t) bundleStride);
        lengths.resize ((std::size_t) bundles);
        return bundles;
    }
    unsigned long long stamp() const
    {
        if (! bundleStamp) return FX_OSC_TIMETAG_IMMEDIATE;
        return fx_osc_timetag (std::chrono::duration<double> (std::chrono::system_clock::now().time_since_epoch()).count());
    }

    fx_osc_sender* sender = nullptr;
    std::vector<unsigned char> scratch;
    std::vector<int> lengths;
    int bundleBytes = 0, bundleStride = 0;
    bool bundleStamp = false;
    int (*addressStride) (fx_context*) = nullptr;
    fx_status (*addressedDatagrams) (fx_context*, unsigned char*, int, int*, int) = nullptr;
};

// The live engine.  The reference's audio callback copies the device block into the collector's ring and notify()s the analysis thread
// (AudioDataCollector.h:36-70); the analysis thread takes window/2 samples when they are there, analyses and writes AudioFeatures
// (RealTimeAnalyser.h:141-177, :201-234).  Same split here, for all channels at once:
//   audio thread   audioDeviceIOCallback / pushBlock: ONE copy of the block into a preallocated FIFO slot and a notify -- no allocation, no
//                  HIP call, never waits for the GPU.  A full FIFO (the worker has fallen `fifoBlocks` blocks behind) drops the block and
//                  counts it, where the reference's writer would overrun the reader (AudioDataCollector.h:96-105).
//   worker thread  owns every call on the context (fx.h: calls on one context are serialised by the caller): fx_push_samples of the next
//                  block STRAIGHT from its FIFO slot -- the slots are page-locked (fx_host_alloc), so the copy to the GPU is the link's DMA
//                  and there is no second host copy; a block that completes one hop is read by the analysis kernels directly -- then the
//                  publication: the frames callback (the place of the run() loops' updateFeature calls) and, if an OSCBatchSender is
//                  attached, every channel's message formed on the GPU from the latest vectors.
// Latency is recorded per block that completed frames: arrival on the audio thread -> publication.
// Construct after the analyser, destroy before it.  Link with -pthread.
class LiveAnalyser
{
public:
    typedef std::function<void (int frames, const float* raw, const float* smoothed)> FramesCallback;   // [channels][frames][12], worker thread
    typedef std::function<void (int track, long long frame)> OnsetCallback;                              // worker thread

    // sampleFormat: what pushBlock's blocks hold -- FX_SAMPLE_F32 (JUCE's float callbacks; audioDeviceIOCallback needs it), or the device's own
    // integers as they are (FX_SAMPLE_S16, packed FX_SAMPLE_S24) or FX_SAMPLE_F16: half / three quarters of the bytes across the link, the same
    // result bits as the floats JUCE would have made of them (fx.h, sample formats)
    LiveAnalyser (RealTimeBatchAnalyser& analyserToFeed, int maxBlockSamples, int fifoBlocks = 8, int sampleFormat = FX_SAMPLE_F32)
        : analyser (analyserToFeed), channels (analyserToFeed.getNumChannels()), hop (analyserToFeed.getWindowSize() / 2),
          maxBlock (maxBlockSamples), format (sampleFormat),
          sampleBytes (sampleFormat == FX_SAMPLE_F32 ? 4 : (sampleFormat == FX_SAMPLE_S24 ? 3 : 2)), slots ((std::size_t) (fifoBlocks > 1 ? fifoBlocks : 2)),
          mostFrames ((maxBlockSamples > 0 ? maxBlockSamples + analyserToFeed.getWindowSize() / 2 - 1 : 0) / (analyserToFeed.getWindowSize() / 2) + 1)
    {
        if (maxBlockSamples < 1) throw Error (FX_ERR_INVALID_ARGUMENT, "maxBlockSamples must be positive");
        if (sampleFormat != FX_SAMPLE_F32 && sampleFormat != FX_SAMPLE_F16 && sampleFormat != FX_SAMPLE_S16 && sampleFormat != FX_SAMPLE_S24)
            throw Error (FX_ERR_INVALID_ARGUMENT, "unknown sample format");
        const std::size_t most = (std::size_t) ((maxBlockSamples + hop - 1) / hop + 1);            // frames a block plus the pending samples can complete
        const std::size_t values = (std::size_t) channels * most * FX_NUM_FEATURES * sizeof (float);
        try
        {
            for (Slot& s : slots) { void* p = nullptr; check (fx_host_alloc (&p, sampleBytes * (std::size_t) channels * (std::size_t) maxBlockSamples)); s.samples = static_cast<unsigned char*> (p); }
            void* p = nullptr;
            check (fx_host_alloc (&p, values)); rawValues = static_cast<float*> (p);
            check (fx_host_alloc (&p, values)); smoothedValues = static_cast<float*> (p);
            latencies.reserve (1 << 20);
            running = true;
            worker = std::thread ([this] { run(); });
        }
        catch (...) { running = false; release(); throw; }           // (the destructor of a half-built engine never runs: give the page-locked memory back here)
    }
    ~LiveAnalyser()
    {
        stop();
        release();
    }
    LiveAnalyser (const LiveAnalyser&) = delete;
    LiveAnalyser& operator= (const LiveAnalyser&) = delete;

    // AUDIO THREAD, ref AudioDataCollector.h:36-70: inputChannelData[c] -> numberOfSamples floats of channel c.  false: the block was dropped.
    bool audioDeviceIOCallback (const float* const* inputChannelData, int numInputChannels, int numberOfSamples)
    {
        if (format != FX_SAMPLE_F32 || numInputChannels < channels || numberOfSamples < 0 || numberOfSamples > maxBlock) { dropped++; return false; }
        Slot* s = claim();
        if (s == nullptr) return false;
        for (int c = 0; c < channels; ++c)
            std::memcpy (s->samples + sizeof (float) * (std::size_t) c * (std::size_t) numberOfSamples, inputChannelData[c], sizeof (float) * (std::size_t) numberOfSamples);
        publish (s, numberOfSamples);
        return true;
    }
    // the same for a block that is already [channels][numberOfSamples] in one piece, in the engine's sample format
    bool pushBlock (const void* samples, int numberOfSamples)
    {
        if (numberOfSamples < 0 || numberOfSamples > maxBlock) { dropped++; return false; }
        Slot* s = claim();
        if (s == nullptr) return false;
        std::memcpy (s->samples, samples, sampleBytes * (std::size_t) channels * (std::size_t) numberOfSamples);
        publish (s, numberOfSamples);
        return true;
    }

    // set before the first block (not synchronised against the worker)
    void setFramesAnalysedCallback (FramesCallback f)                               { framesAnalysed = f; }
    // The tracks' onsetDetectedCallback (RealTimeAnalyser.h:256, AnalyserTrackController.h:80-84) as one callback: the worker drains
    // the analyser's onset event list after each block that completed frames and calls `f` once per (track, frame) whose onset
    // slot is 1, in (frame, track) order.  Setting it enables the list on the analyser, with room for every onset one block can
    // hold.  With this callback and NO frames callback the engine asks for neither result buffer: the block's vectors never cross
    // the link (latestSmoothed() then stays empty; an attached OSC sender still gets its messages, formed on the GPU).
    void setOnsetDetectedCallback (OnsetCallback f)
    {
        onsetDetected = f;
        const long long room = (long long) channels * (long long) mostFrames;
        analyser.enableOnsetEvents (f ? (int) (room < (1ll << 26) ? room : (1ll << 26)) : 0);
        drainOnsets = [this] { return analyser.getOnsetEvents(); };       // (the worker's only way to the list: see analyse())
    }
    void attachOSCSender (OSCBatchSender* sender, const std::string& bundlePrefix = "/Audio/A", int firstChannel = 0)
    {
        osc = sender; oscPrefix = bundlePrefix; oscFirst = firstChannel;
    }

    // Anything else that touches the analyser while the engine runs -- setGain, setOnsetDetectionType, sampleRateChanged, clearBuffer ... from a
    // GUI / message thread -- goes through here: the call is queued and the WORKER makes it before it takes the next block, so that the
    // context still has one caller (fx.h).  Not for the audio thread (it takes a lock).
    void callOnWorker (std::function<void (RealTimeBatchAnalyser&)> f)
    {
        { std::lock_guard<std::mutex> g (wake); commands.push_back (std::move (f)); }
        ready.notify_one();
    }

    // A track handed to a new source while the engine runs (RealTimeBatchAnalyser::resetTracks): queued like any other command, so the
    // worker makes the call between two blocks and the audio thread is never involved.  The list is copied.
    void resetTracks (const int* tracks, int count)
    {
        // refused here as fx_reset_channels refuses them, on the caller's thread: a bad count, a null list, a track out of range
        if (count < 0 || (count > 0 && tracks == nullptr)) throw Error (FX_ERR_INVALID_ARGUMENT, "bad track list");
        for (int i = 0; i < count; ++i)
            if (tracks[i] < 0 || tracks[i] >= analyser.getNumChannels()) throw Error (FX_ERR_INVALID_ARGUMENT, "no such track");
        if (count == 0) return;
        std::vector<int> list (tracks, tracks + count);
        callOnWorker ([list] (RealTimeBatchAnalyser& a) { a.resetTracks (list.data(), (int) list.size()); });
    }

    // A track that leaves for another analyser or arrives from one while the engine runs (RealTimeBatchAnalyser::exportTracks /
    // importTracks): the worker makes the call between two blocks, so the record is the track's state at a block boundary; the caller
    // waits for the result (an Error is thrown here, on the caller's thread).  The audio thread is not involved.  The lists are copied.
    std::vector<unsigned char> exportTracks (const int* tracks, int count)
    {
        const std::vector<int> list = checkedTracks (tracks, count);
        std::vector<unsigned char> records;
        waitOnWorker ([&list, &records] (RealTimeBatchAnalyser& a) { records = a.exportTracks (list.data(), (int) list.size()); });
        return records;
    }
    void importTracks (const int* tracks, int count, const std::vector<unsigned char>& records)
    {
        const std::vector<int> list = checkedTracks (tracks, count);
        waitOnWorker ([&list, &records] (RealTimeBatchAnalyser& a) { a.importTracks (list.data(), (int) list.size(), records); });
    }

    // wait until everything pushed so far has been analysed and published (not for the audio thread)
    void drain()
    {
        std::unique_lock<std::mutex> g (wake);
        idle.wait (g, [this] { return written.load() == consumed.load() && commands.empty() && ! busyNow; });
    }
    void stop()
    {
        if (! running.exchange (false)) return;
        { std::lock_guard<std::mutex> g (wake); }
        ready.notify_all();
        if (worker.joinable()) worker.join();
    }

    struct Stats
    {
        long long blocksIn, blocksDropped, blocksAnalysed, framesPerChannel, errors;
        double latencyMsP50, latencyMsP99, latencyMsMax;      // audio-thread arrival -> publication, over the blocks that completed frames
        double workerBusySeconds;                              // time the worker spent between taking a block and having published it
    };
    Stats getStats()
    {
        Stats st;
        st.blocksIn = written.load(); st.blocksDropped = dropped.load(); st.blocksAnalysed = consumed.load();
        std::lock_guard<std::mutex> g (statLock);
        st.framesPerChannel = frames; st.errors = errors; st.workerBusySeconds = busy;
        std::vector<float> v (latencies);
        std::sort (v.begin(), v.end());
        st.latencyMsP50 = v.empty() ? 0.0 : v[v.size() / 2];
        st.latencyMsP99 = v.empty() ? 0.0 : v[(std::size_t) ((double) (v.size() - 1) * 0.99)];
        st.latencyMsMax = v.empty() ? 0.0 : v.back();
        return st;
    }
    std::string lastError() { std::lock_guard<std::mutex> g (statLock); return errorText; }
    // the latest smoothed vectors [channels][12] as the worker last published them (a copy; any thread)
    std::vector<float> latestSmoothed() { std::lock_guard<std::mutex> g (statLock); return latest; }

private:
    typedef std::chrono::steady_clock Clock;
    struct Slot { unsigned char* samples = nullptr; int count = 0; Clock::time_point arrived; };

    void release()
    {
        for (Slot& s : slots) { if (s.samples != nullptr) fx_host_free (s.samples); s.samples = nullptr; }
        if (rawValues != nullptr) fx_host_free (rawValues);
        if (smoothedValues != nullptr) fx_host_free (smoothedValues);
        rawValues = smoothedValues = nullptr;
    }
    // single producer (the audio thread), single consumer (the worker): `written` / `consumed` count blocks, a slot is index mod size
    Slot* claim()
    {
        const long long w = written.load (std::memory_order_relaxed);
        if (w - consumed.load (std::memory_order_acquire) >= (long long) slots.size()) { dropped++; return nullptr; }
        return &slots[(std::size_t) (w % (long long) slots.size())];
    }
    void publish (Slot* s, int numberOfSamples)
    {
        s->count = numberOfSamples;
        s->arrived = Clock::now();
        written.fetch_add (1, std::memory_order_release);
        { std::lock_guard<std::mutex> g (wake); }                                   // (the worker holds it only around its look at the counters, never while it works)
        ready.notify_one();                                                         // notify(), ref AudioDataCollector.h:68-69
    }

    std::vector<int> checkedTracks (const int* tracks, int count) const
    {
        if (count < 0 || (count > 0 && tracks == nullptr)) throw Error (FX_ERR_INVALID_ARGUMENT, "bad track list");
        for (int i = 0; i < count; ++i)
            if (tracks[i] < 0 || tracks[i] >= analyser.getNumChannels()) throw Error (FX_ERR_INVALID_ARGUMENT, "no such track");
        return std::vector<int> (tracks, tracks + count);
    }
    // callOnWorker for a call whose result the caller needs: returns when the worker has made it, and throws what it threw (whatever
    // it threw) on the caller's thread.  The command is queued under the lock the worker leaves its loop under, so an engine that
    // stops meanwhile either still makes the call or refuses it here; on the worker thread itself (a framesAnalysed / onsetDetected
    // callback) the call is made at once -- that thread is between two blocks already and must not wait for itself.
    void waitOnWorker (const std::function<void (RealTimeBatchAnalyser&)>& f)
    {
        if (std::this_thread::get_id() == worker.get_id()) { f (analyser); return; }
        struct Reply { std::mutex m; std::condition_variable cv; bool done = false; std::exception_ptr thrown; };
        auto reply = std::make_shared<Reply>();
        {
            std::lock_guard<std::mutex> g (wake);
            if (! running.load()) throw Error (FX_ERR_INVALID_ARGUMENT, "the engine is not running");
            commands.push_back ([reply, &f] (RealTimeBatchAnalyser& a)
            {
                std::exception_ptr thrown;
                try { f (a); } catch (...) { thrown = std::current_exception(); }
                { std::lock_guard<std::mutex> r (reply->m); reply->done = true; reply->thrown = thrown; }
                reply->cv.notify_all();
            });
        }
        ready.notify_one();
        std::unique_lock<std::mutex> g (reply->m);
        reply->cv.wait (g, [&reply] { return reply->done; });
        if (reply->thrown) std::rethrow_exception (reply->thrown);
    }
    void fail (const char* what)
    {
        std::lock_guard<std::mutex> g (statLock);
        errors++;
        errorText = std::string (what) + ": " + fx_last_error();
    }
    // one block: analysed straight from its page-locked FIFO slot, then what it completed is published
    void analyse (Slot& s)
    {
        int got = 0;
        const bool onsetsOnly = onsetDetected && ! framesAnalysed;      // nobody reads the vectors: they stay on the GPU
        if (fx_push_samples (analyser.handle(), s.samples, s.count, format, FX_MEM_HOST, onsetsOnly ? nullptr : rawValues,
                             onsetsOnly ? nullptr : smoothedValues, &got) != FX_OK) { fail ("fx_push_samples"); return; }
        if (got <= 0) return;
        if (framesAnalysed) framesAnalysed (got, rawValues, smoothedValues);
        if (onsetDetected && drainOnsets)       // (a host that never sets the callback needs no symbol of the event list from the library)
        {
            try { for (const fx_onset_event& e : drainOnsets()) onsetDetected (e.channel, e.frame); }
            catch (const Error&) { fail ("fx_get_onset_events"); }
        }
        if (osc != nullptr)
        {
            try { osc->updateFromContext (analyser.handle(), channels, oscPrefix, oscFirst); }
            catch (const Error&) { fail ("fx_get_osc_datagrams"); }
        }
        const double ms = std::chrono::duration<double, std::milli> (Clock::now() - s.arrived).count();
        std::lock_guard<std::mutex> g (statLock);
        frames += got;
        if (latencies.size() < latencies.capacity()) latencies.push_back ((float) ms);
        if (onsetsOnly) return;
        latest.resize ((std::size_t) channels * FX_NUM_FEATURES);
        for (int c = 0; c < channels; ++c)
            std::memcpy (&latest[(std::size_t) c * FX_NUM_FEATURES], &smoothedValues[((std::size_t) c * (std::size_t) got + (std::size_t) (got - 1)) * FX_NUM_FEATURES], sizeof (float) * FX_NUM_FEATURES);
    }
    void run()
    {
        for (;;)
        {
            std::vector<std::function<void (RealTimeBatchAnalyser&)>> todo;
            {
                std::unique_lock<std::mutex> g (wake);
                busyNow = false;
                if (written.load() == consumed.load() && commands.empty()) idle.notify_all();
                ready.wait (g, [this] { return ! running.load() || written.load() != consumed.load() || ! commands.empty(); });
                if (! running.load() && written.load() == consumed.load() && commands.empty()) return;
                todo.swap (commands);
                busyNow = true;
            }
            for (auto& f : todo)                                                    // the other threads' setter calls, in order, between blocks
            {
                try { f (analyser); } catch (const Error&) { fail ("a call queued with callOnWorker"); }
            }
            if (written.load (std::memory_order_acquire) == consumed.load()) continue;
            const Clock::time_point t0 = Clock::now();
            analyse (slots[(std::size_t) (consumed.load() % (long long) slots.size())]);
            consumed.fetch_add (1, std::memory_order_release);                      // the slot is the audio thread's again
            const double dt = std::chrono::duration<double> (Clock::now() - t0).count();
            std::lock_guard<std::mutex> g (statLock);
            busy += dt;
        }
    }

    RealTimeBatchAnalyser& analyser;
    int channels, hop, maxBlock, format;
    std::size_t sampleBytes;
    std::vector<Slot> slots;
    int mostFrames;                      // frames per channel a block plus the pending samples can complete
    std::atomic<long long> written { 0 }, consumed { 0 }, dropped { 0 };
    std::mutex wake;
    std::condition_variable ready, idle;
    std::vector<std::function<void (RealTimeBatchAnalyser&)>> commands;   // guarded by `wake`
    bool busyNow = false;                                                  // guarded by `wake`: the worker is between taking work and having finished it
    std::atomic<bool> running { false };
    std::thread worker;
    FramesCallback framesAnalysed;
    OnsetCallback onsetDetected;
    std::function<std::vector<fx_onset_event>()> drainOnsets;
    OSCBatchSender* osc = nullptr;
    std::string oscPrefix;
    int oscFirst = 0;
    float* rawValues = nullptr;          // page-locked: fx_push_samples copies the vectors back without a staging copy
    float* smoothedValues = nullptr;
    std::mutex statLock;
    long long frames = 0, errors = 0;
    double busy = 0.0;
    std::vector<float> latencies, latest;
    std::string errorText;
};
} // namespace fx

#endif // FX_REALTIME_HPP
