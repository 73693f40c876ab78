/*
 * fx.h -- C ABI of libfx_hip.so: the MI355X (gfx950) implementation of the
 * reference's per-frame audio feature path
 *     RealTimeAnalyser -> SpectralCharacteristics / HarmonicCharacteristics /
 *     PitchAnalyser  ->  AudioFeatures (12 floats)  ->  OSC feature message.
 *
 * The reference (SeanSoraghan/Feature-Extractor) has no FFI layer; the seam this
 * library replaces is "analysis window in -> AudioFeatures::updateFeature out".
 * Every entry point cites the reference interface it stands in for; paths are
 * relative to the reference's Source/ directory.
 *
 * Conventions
 *   - plain C types only; every function returns an fx_status (0 = FX_OK) and
 *     fx_last_error() returns a description of the last failure on this thread.
 *   - a context analyses `num_channels` independent mono channels (one
 *     AnalyserTrackController each, AnalyserTrackController.h:199-206) on ONE
 *     GPU.  Calls on one context must be externally serialised.
 *   - all work is enqueued on the context's HIP stream; fx_sync() waits for it.
 *   - feature vectors use the AudioFeatures slot order (RealTimeAnalyser.h:19-30).
 *   - numeric behaviour (NaN, inf, values > 1) is the reference's; nothing is
 *     clamped or "fixed".  The reference defines no answer for the harmonic energy
 *     ratio, the odd/even ratio and the inharmonicity of a frame whose raw f0 is
 *     not > 0 (it indexes bins out of bounds, HarmonicCharacteristics.h:161-166,205):
 *     those three slots are deterministic there, nothing more.  Every other slot,
 *     and every slot of a FX_SPECTRAL_ONLY context, is the reference's for every input.
 *   - there is NO CPU fallback: if no gfx950 device is usable every call fails
 *     with FX_ERR_NO_DEVICE.
 */
#ifndef FX_H
#define FX_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FX_ABI_VERSION 6

typedef int fx_status;
enum {
    FX_OK = 0,
    FX_ERR_INVALID_ARGUMENT = 1,
    FX_ERR_NO_DEVICE = 2,
    FX_ERR_HIP = 3,
    FX_ERR_OUT_OF_MEMORY = 4,
    FX_ERR_UNSUPPORTED = 5
};

/* AudioFeatures::eAudioFeature, RealTimeAnalyser.h:17-32 */
enum {
    FX_ONSET = 0, FX_RMS, FX_F0, FX_CENTROID, FX_SPREAD, FX_FLATNESS, FX_LER,
    FX_FLUX, FX_SLOPE, FX_HER, FX_OER, FX_INHARM, FX_NUM_FEATURES
};

/* OnsetDetector::eOnsetDetectionType, SpectralCharacteristics.h:213-219 */
enum { FX_ONSET_SPECTRAL = 0, FX_ONSET_AMPLITUDE = 1, FX_ONSET_COMBINATION = 2 };

/* Where a caller buffer lives. */
enum { FX_MEM_HOST = 0, FX_MEM_DEVICE = 1 };

/* Sample formats accepted for audio input.  FX_SAMPLE_S16 is 16-bit signed PCM, little endian as the host has it: the load
 * stage of the kernels turns a sample v into the float v / 32768 -- exactly what JUCE's WAV reader (and include/fx_wav.hpp)
 * makes of a 16-bit file before AudioDataCollector sees it (AudioFilePlayer.h:41-61, AudioDataCollector.h:42-64) -- so an
 * integer source crosses PCIe at two bytes per sample and every result is bit for bit that of the decoded floats.
 * FX_SAMPLE_S24 is 24-bit signed PCM PACKED in three bytes per sample, little endian (the layout of a 24-bit WAV file's data
 * chunk): v / 8388608, again the reader's float exactly; a hop of window_size/2 samples is window_size/2 * 3 bytes. */
enum { FX_SAMPLE_F32 = 0, FX_SAMPLE_F16 = 1, FX_SAMPLE_S16 = 2, FX_SAMPLE_S24 = 3 };

/* fx_create flags.  The first three fix the order in which the reference's two
 * analysis threads write the ONE shared AudioFeatures object per hop
 * (AnalyserTrackController.h:20-21; a data race in the reference):            */
#define FX_ORDER_SPECTRAL_THEN_HARMONIC 0u   /* default */
#define FX_ORDER_HARMONIC_THEN_SPECTRAL 1u
#define FX_ORDER_ISOLATED               2u   /* one AudioFeatures per analyser */
#define FX_ORDER_MASK                   3u
/* Construct only one of the two analysers (the reference builds both, AnalyserTrackController.h:20-21).
 * Slots the absent analyser would write keep their initial state: raw 0, getValue NaN (0.0f / 0, as
 * AudioFeatures::getValue returns before any insert, RealTimeAnalyser.h:84-88). */
#define FX_SPECTRAL_ONLY                4u   /* RealTimeSpectralAnalyser only: RMS, centroid..slope, onset */
#define FX_HARMONIC_ONLY                8u   /* RealTimeHarmonicAnalyser only: RMS, F0, HER, OER, inharmonicity */
/* The low-latency kernel family, for hosts that run the reference's own cadence -- one analysis per hop as it arrives
 * (AudioDataCollector.h:66-94) -- and care about the round trip of that one hop rather than about frames per second.
 * Windows of 2048 and 4096 points (both analysers): every analysis frame is spread over a PAIR of wavefronts, which halves the
 * arithmetic on a hop's critical path (4096-point hop 35 -> 31 us) and costs throughput on long calls (2048 points: -25 %).
 * Results: every discrete decision (onset, pitch lag, peaks, gates) is identical to the default family's; the continuous slots
 * may differ from it in the last bit (sums over bins are added in another order).  One family per context, from fx_create to
 * fx_destroy, so a channel's smoothing history never mixes the two.  No effect on other window sizes or with one analyser. */
#define FX_LOW_LATENCY                  16u

typedef struct fx_context fx_context;

/* Replaces the RealTimeSpectralAnalyser + RealTimeHarmonicAnalyser constructor
 * pair, (AudioDataCollector&, AudioFeatures&, int windowSize, double sampleRate)
 * -- RealTimeAnalyser.h:100,136,196 -- for `num_channels` channels at once.
 * window_size: power of two in [256, 4096] (the collector ring is 4096,
 * AudioDataCollector.h:24; the app uses 2048, AnalyserTrackController.h:20-21). */
fx_status fx_create(fx_context** out, int device_id, int num_channels,
                    int window_size, double sample_rate, unsigned flags);
fx_status fx_destroy(fx_context* ctx);

/* Zero overlap buffers, flux state and every ValueHistory (a freshly
 * constructed AnalyserTrackController); settings are kept.  Every track's
 * frame index is 0 again (fx_get_channel_frames). */
fx_status fx_reset_state(fx_context* ctx);

/* RealTimeAnalyser::sampleRateChanged, RealTimeAnalyser.h:111-114 */
fx_status fx_set_sample_rate(fx_context* ctx, double sample_rate);
/* RealTimeSpectralAnalyser::setOnsetDetectionSensitivity, RealTimeAnalyser.h:244-248 */
fx_status fx_set_onset_sensitivity(fx_context* ctx, float sensitivity);
/* RealTimeSpectralAnalyser::setOnsetWindowLength, RealTimeAnalyser.h:250-254
 * (both onset histories are emptied, as ValueHistory::setHistoryLength does);
 * 1 <= length <= 32 (the GUI offers 3..21, AudioFeaturesListComponent.h:142-156) */
fx_status fx_set_onset_window(fx_context* ctx, int length);
/* RealTimeSpectralAnalyser::setOnsetDetectionType, RealTimeAnalyser.h:258 */
fx_status fx_set_onset_type(fx_context* ctx, int type);
/* AudioDataCollector::setGain, AudioDataCollector.h:124 (applied to hops only,
 * as AudioDataCollector::getAnalysisBuffer does at :88) */
fx_status fx_set_gain(fx_context* ctx, float gain);

/* ---- the same settings per track ----
 * In the reference every track is an AnalyserTrackController with its own gain slider and its own onset controls
 * (AnalyserTrackController.h:126-134).  These take whole-context arrays in host memory, one entry per track; NULL leaves that
 * setting alone.  A context on which none of them was ever called runs exactly as before; a track given values here produces, bit
 * for bit, what it produces in a context that has those values context-wide.  Like the context-wide setters they take effect for
 * the hops analysed by the next call, in stream order (the gain where a hop is read: pending samples are kept un-gained, the stored
 * window tail is already gained), fx_reset_state keeps them, and the caller may free or reuse the arrays on return.  The
 * context-wide setters above keep their meaning "set it on every track": fx_set_gain(ctx, g) after these leaves every track with g.
 * A bad entry fails the whole call with FX_ERR_INVALID_ARGUMENT (fx_last_error names the track) and changes nothing; a failed
 * upload reports FX_ERR_HIP and leaves the old settings in force.  They synchronise the context's stream.
 * Not per track: the NUMBER of pending samples (tracks would hold different numbers of them -- ragged blocks), the sample rate, the
 * window size and the analysers' order; those stay one per context.  (Files of different lengths share a context all the same:
 * every track gets n samples per tick, and a clip that has ended renders silence -- file sources, fx_push_sources below.) */
/* AudioDataCollector::setGain per track (AnalyserTrackController.h:126-130).  gain [num_channels]; any float, as fx_set_gain. */
fx_status fx_set_channel_gains(fx_context* ctx, const float* gain);
/* setOnsetDetectionSensitivity / setOnsetWindowLength / setOnsetDetectionType per track (AnalyserTrackController.h:132-134).
 * Each array is [num_channels] or NULL (unchanged).  sensitivity >= 0; type FX_ONSET_*.  window: an entry < 0 leaves that track's
 * window AND its onset histories alone; an entry in [1, 32] is a setHistoryLength call on that track (histories emptied even when
 * the length is the one it had, RealTimeAudioAnalysis.h:73-81); 0 and entries above 32 are refused. */
fx_status fx_set_channel_onset(fx_context* ctx, const float* sensitivity, const int* window, const int* type);
/* What each track runs with now ([num_channels] each; any pointer may be NULL): after a context-wide setter, its value on every track. */
fx_status fx_get_channel_settings(fx_context* ctx, float* gain, float* sensitivity, int* window, int* type);

/* ---- per-track reset and clear: replace one track without touching the rest ----
 * In the reference tracks are destroyed and built again one object at a time (MainComponent.cpp:137-186), and the transport buttons
 * and a dropped file call clearBuffer() on THAT track's collectors only (AnalyserTrackController.h:109-112,135-137,167-171).  Both
 * calls take a list of tracks in host memory (the caller may free or reuse it on return) and follow the same rules:
 *   - they take effect in stream order for the analysis calls that follow, and they synchronise the context's stream, as the
 *     per-track setters do.  With a fx_stream_* ring on the context they are therefore ordered after the batches already submitted
 *     and reach every batch submitted later, the captured one-hop step included.
 *   - num_channels == 0 is a no-op; duplicates are allowed.  A null context, a null list with num_channels > 0, num_channels < 0 or
 *     an entry outside [0, num_channels of the context) is FX_ERR_INVALID_ARGUMENT before any device use: fx_last_error names the
 *     entry, nothing changes.
 *   - a failed allocation, upload or launch reports FX_ERR_OUT_OF_MEMORY / FX_ERR_HIP.  The tracks NOT listed are untouched in every
 *     case.  The listed tracks may then be part old, part new, as after a failed analysis launch: repeat the call, or fx_reset_state.
 *   - a context on which neither was ever called makes exactly the launches it made before and returns the bits it returned before.
 * A new AnalyserTrackController in these slots: overlap tail, flux state, every ValueHistory, both onset histories and the latest
 * vector become those of fx_create; the tracks' pending samples become zeros (a new collector's ring).  The pending COUNT stays (it is
 * one per context).  Settings -- gain, onset settings, channel map -- are kept, as fx_reset_state keeps them.  The tracks' frame index
 * (fx_get_taps frame_index, fx_onset_event::frame) starts at 0 again.  So a listed track produces, bit for bit, what the same track
 * of a freshly created context with the same settings produces when that context is first given fx_pending_samples() zeros and then
 * the same input; every other track produces what it produces in a context where the call was never made.  The first call on a
 * context without a per-track table creates it with the context-wide values, as the first per-track setter does. */
fx_status fx_reset_channels(fx_context* ctx, const int* channels, int num_channels);
/* AudioDataCollector::clearBuffer (AudioDataCollector.h:119,122) on these tracks only: their pending samples become zeros, nothing
 * else changes (fx_clear_pending is the same for every track). */
fx_status fx_clear_pending_channels(fx_context* ctx, const int* channels, int num_channels);
/* Frames each track has analysed since fx_create / fx_reset_state / its last fx_reset_channels; frames [num_channels], host memory.
 * No device use. */
fx_status fx_get_channel_frames(fx_context* ctx, long long* frames);

/* ---- moving tracks between contexts: export and import a track's whole state ----
 * The reference's tracks are heap objects (AnalyserTrackController.h) that a host moves by moving a pointer; here a track is a row of
 * the context's tables, and a RECORD of fx_track_state_bytes() bytes is the way back out: rebalancing shards, draining a GPU, a
 * context with another num_channels, a restart that keeps every track's analysis state.  A record holds all of it -- flux state,
 * overlap tail, pending samples, the 48 newest frames' raw values (every ValueHistory and both onset histories), the latest vector,
 * gain, onset sensitivity / window / type, the track's frame count and the frames since its last onset-window reset -- so a track
 * imported into any slot of any compatible context goes on, bit for bit, as it would have where it was: raw and smoothed values,
 * fx_get_channel_frames, fx_get_taps frame_index and fx_onset_event::frame included.  The sample rate is the context's and does not
 * travel; OSC addresses, sender routes and the channel map belong to the slot and do not travel either.
 *
 * A record is canonical: its bytes depend on the track's state alone, not on the source context's frame index, num_channels or the
 * slot -- export, import anywhere compatible, export again gives the same bytes.  Every part starts on a 16-byte boundary:
 *   header (80 bytes): uint32 magic, layout version; int32 window_size; uint32 create flags that shape state (order, analyser bits);
 *     int32 kernel family in force (1, or 2 for the FX_LOW_LATENCY pairs), pending count, pending format, onset window; int64 frames,
 *     onset_frames; float gain, sensitivity, onset multiplier; int32 onset type; uint32 record bytes; three zero words
 *   latest vector [12] | ring [48][12]: row k = the raw values of the track's frame frames - 48 + k, zeros before its first frame |
 *   flux row [N/2] | tail row [N/2] | pending row (N/2 * 4 bytes, zeros beyond the pending samples)
 *
 * channels / num_channels follow fx_reset_channels: host memory, num_channels == 0 is a no-op, every entry is checked before
 * anything is touched and fx_last_error names the bad one.  Record i belongs to channels[i]; records lie back to back.  Duplicates are
 * allowed on export and refused on import.  The buffer is FX_MEM_HOST or FX_MEM_DEVICE (16-byte aligned), at least num_channels *
 * fx_track_state_bytes() bytes, and valid on return either way: both calls synchronise the context's stream, as the per-track setters
 * do, so with a fx_stream_* ring they come after the batches submitted and before every later one, the captured step included.
 * A device buffer is read and written on the context's stream only (the records' headers too): what the caller queued on
 * fx_get_stream() to fill it, or made that stream wait for, comes first.  A host buffer's records pass through at most 32 MB of
 * device scratch, a chunk at a time.
 * Export changes nothing in the context.
 *
 * Import: the context must match each record in window_size, those flags, the kernel family, the pending count and -- where samples
 * are pending -- their format; otherwise, or for a bad magic or version, FX_ERR_INVALID_ARGUMENT names the record and the field.  All
 * of this is decided before any change (for a host buffer before any device use).  A valid import creates the per-track table if
 * there is none, as the first per-track setter does.  Failures are fx_reset_channels': tracks not listed are untouched in every case;
 * after a failed upload or launch the listed ones may be part old, part new. */
size_t    fx_track_state_bytes(fx_context* ctx);   /* bytes of one track's record; a multiple of 16; 0 for a null context */
fx_status fx_export_channels(fx_context* ctx, const int* channels, int num_channels, void* out, size_t out_bytes, int mem_kind);
fx_status fx_import_channels(fx_context* ctx, const int* channels, int num_channels, const void* in, size_t in_bytes, int mem_kind);

/* Replaces RealTimeAudioDataOverlapper::getNextBuffer (RealTimeAudioAnalysis.h:
 * 205-228) + both run() loops (RealTimeAnalyser.h:141-177, :201-234) for
 * `num_hops` consecutive hops of window_size/2 samples per channel.
 *   hops         [num_channels][num_hops][window_size/2]  samples (sample_format)
 *   out_raw      [num_channels][num_hops][12]  values passed to updateFeature,
 *                or NULL
 *   out_smoothed [num_channels][num_hops][12]  AudioFeatures::getValue of every
 *                slot after each hop (RealTimeAnalyser.h:84-88), or NULL
 * Buffers are caller-owned and, for FX_MEM_DEVICE, must stay valid until the
 * stream reaches this call's work (fx_sync); a FX_MEM_DEVICE input must start on a
 * 16-byte boundary in every sample format (FX_ERR_INVALID_ARGUMENT otherwise: the
 * kernels read 16 bytes per lane, and a packed 24-bit sample may sit at any byte of
 * them).  FX_MEM_HOST buffers are copied synchronously. */
fx_status fx_push_hops(fx_context* ctx, const void* hops, int num_hops, int sample_format,
                       int mem_kind, float* out_raw, float* out_smoothed);

/* The collector's own interface: a device block of ANY length.  Replaces AudioDataCollector::audioDeviceIOCallback
 * (AudioDataCollector.h:36-70: whatever `numberOfSamples` the audio device delivers -- 441, 480, 512 ... -- goes into the ring)
 * together with the reader that pulls window_size/2 samples whenever they are there (getAnalysisBuffer, :72-94, called by
 * RealTimeAudioDataOverlapper::getNextBuffer, RealTimeAudioAnalysis.h:205-219) for all channels at once.
 *   samples      [num_channels][num_samples]  the block of every channel, rows back to back; num_samples >= 0
 * The context keeps what a block leaves over -- fewer than window_size/2 samples per channel, un-gained, in device memory --
 * analyses floor((pending + num_samples) / (window_size/2)) hops exactly as fx_push_hops would analyse the same samples cut
 * into hops (bit for bit), and keeps the rest.  The gain (fx_set_gain) is applied when a hop is analysed, as getAnalysisBuffer
 * applies it at read time (:88): a change reaches samples that are still pending.
 *   out_raw / out_smoothed  [num_channels][frames][12] with frames = (fx_pending_samples() + num_samples) / (window_size/2),
 *                           or NULL;  *frames_out (may be NULL) receives that count (0 is not an error)
 * FX_MEM_DEVICE blocks must start on a 4-byte boundary (on a 16-byte boundary with whole hops and nothing pending they are
 * analysed in place).  A block that completes one or two hops -- an audio device's 441 / 480 / 512 / 960 / 1024 samples against
 * windows of 1024 points and more -- is read by the analysis kernels directly, and so is a block of any length up to 4096 hops
 * against a 1024-point window; other calls pass through a re-blocking kernel first (same results, one more pass over the
 * samples).  Every channel's block has the same length (one device callback feeds all collectors,
 * AnalyserTrackController.h:31-41).
 * If the analysis of the completed hops fails (an allocation, a launch), the error is returned and those hops are lost -- the pending
 * samples have already moved on -- so the stream is no longer the caller's: fx_reset_state.  The sample format may change only while nothing is pending.  While samples are pending, fx_push_hops,
 * fx_process_frames and fx_stream_submit refuse (whole hops would overtake them); fx_reset_state drops them. */
fx_status fx_push_samples(fx_context* ctx, const void* samples, int num_samples, int sample_format, int mem_kind,
                          float* out_raw, float* out_smoothed, int* frames_out);
/* ---- interleaved input through a per-track channel map ----
 * The reference builds one track per active input of the audio device, and each track's AudioDataCollector collects one
 * device channel, channelData[channelToCollect] (MainComponent.cpp:140-170, AudioDataCollector.h:21-23,36-70).
 * AudioDataCollector::setChannelToCollect (AudioDataCollector.h:123) for every track at once: track c collects source channel
 * map[c] of the interleaved blocks given to fx_push_interleaved.  map == NULL restores the identity (track c <- source c).
 * 0 <= map[c]; duplicates allowed; a source need not be used.  Takes effect for blocks pushed after it; pending samples and every
 * history are kept (the reference's ring is not cleared).  A setting: fx_reset_state keeps it.  Synchronises the context's stream
 * (blocks already pushed read the old map); the caller may free or reuse `map` on return. */
fx_status fx_set_channel_map(fx_context* ctx, const int* map /*[num_channels] or NULL*/);
/* fx_push_samples for an INTERLEAVED block: `samples` holds num_samples frames of num_source_channels samples each
 * ([num_samples][num_source_channels], packed 24-bit: 3 bytes per sample).  Every result, the pending samples and the launch
 * sequence after the de-interleave are those of fx_push_samples on the planar block [c][i] = samples[i][map[c]], bit for bit.
 * The rules of fx_push_samples hold: any num_samples >= 0 (0 is a no-op), device input 4-byte aligned, the format may change only
 * while nothing is pending, mem_kind covers the input and the outputs, and a failure after samples have moved on leaves the
 * stream as fx_push_samples describes.  FX_ERR_INVALID_ARGUMENT if some map[c] >= num_source_channels (nothing is changed then).
 * The caller may reuse a host block on return.  The block passes through one de-interleave kernel into a planar staging buffer
 * on the device: with host input only the interleaved block crosses to the device. */
fx_status fx_push_interleaved(fx_context* ctx, const void* samples, int num_samples, int num_source_channels,
                              int sample_format, int mem_kind, float* out_raw, float* out_smoothed, int* frames_out);
/* samples per channel held back by fx_push_samples / fx_stream_submit_samples, 0 <= n < window_size/2 */
int fx_pending_samples(fx_context* ctx);
/* AudioDataCollector::clearBuffer (AudioDataCollector.h:122; the transport buttons, AnalyserTrackController.h:135-137,167-171):
 * the pending samples become zeros; their count, like the ring's indices, stays. */
fx_status fx_clear_pending(fx_context* ctx);

/* ---- RTP audio in: a tick's L16 / L24 datagrams unpacked to tracks on the GPU ----
 * Audio in the numbers this library is built for arrives over the network (AES67, ST 2110-30, Dante in AES67 mode, Ravenna), and
 * all of these are one wire format: RTP datagrams (RFC 3550) whose payload is L16 or L24 (RFC 3551 4.5.11, RFC 3190), big-endian
 * signed PCM, a stream's channels interleaved per sample time.  A receiver collects the datagrams of one tick in slots of one
 * stride and says which stream each came from; fx_push_rtp parses the headers, places the payloads by their RTP time, fills what is
 * lost with zeros, reverses the bytes and analyses the planar block as fx_push_samples would -- all of it on the device, and the
 * result a pure function of the arguments and the cursors.
 *
 *   fx_rtp_configure   S streams (1 .. FX_RTP_MAX_STREAMS), stream s of channels[s] (1 .. FX_RTP_MAX_CHANNELS) channels, all in one
 *                      payload format (a planar block has one sample format).  Every stream starts not running, every track's
 *                      source is none, the statistics are zero -- also when a configured context is configured again.
 *                      num_streams == 0 frees the unit.  Synchronises the context's stream.
 *   fx_rtp_set_track_sources  a track list under fx_reset_channels' rules (host memory, duplicates allowed and the last entry
 *                      wins, 0 entries a no-op, every entry checked before anything changes): track tracks[i] hears channel
 *                      channel[i] of stream stream[i]; stream[i] == -1: none, the track hears zeros.  The listed tracks' pending
 *                      samples become zeros, also where nothing changes (as fx_set_channel_sources: toggleCollectInput,
 *                      AudioDataCollector.h:119).  Takes effect for the ticks pushed after it; synchronises the stream.
 *   fx_rtp_set_cursors stream streams[i] becomes running with cursor rtp_time[i]: the RTP time (the header's 32-bit sample clock,
 *                      RFC 3550 5.1) of the first sample time of the next tick.  (A receiver takes it from a stream's first
 *                      packet, less its latency; that policy is the caller's.)  Every tick moves every running stream's cursor
 *                      on by its num_samples, modulo 2^32; the host keeps the cursors, so fx_rtp_get_cursors uses no device
 *                      (0 for a stream that is not running).
 *
 * fx_push_rtp -- one tick.  `packets` holds num_packets slots of slot_stride bytes (a multiple of 4 in [12, FX_RTP_MAX_SLOT_STRIDE])
 * in mem_kind memory, device memory 4-byte aligned; datagram i is the first lengths[i] (0 .. slot_stride) bytes of slot i and came
 * from stream stream_of[i].  lengths and stream_of are host arrays and are judged before anything is launched, as are
 * fx_push_samples' own refusals (the block's format is FX_SAMPLE_S16 for L16, FX_SAMPLE_S24 for L24): a refused call names the
 * entry and changes nothing.  num_packets == 0 is a tick of pure loss; num_samples == 0 is a no-op.  mem_kind covers the packets,
 * the results and `disposition` (optional: one byte of FX_RTP_* bits per packet, any alignment).  The caller may reuse host
 * arrays on return.  With n = num_samples:
 *   1. Packet i of length len, bytes b, is MALFORMED if len < 12 or b[0] >> 6 != 2.  P = bit 5 of b[0], X = bit 4, CC = b[0] & 15,
 *      T = the big-endian 32 bits b[4..8); marker, payload type, sequence number and SSRC are not interpreted.  h = 12 + 4 CC; if X:
 *      malformed if h + 4 > len, else h += 4 + 4 * (big-endian 16 bits b[h+2..h+4)).  Malformed if h > len.  pad = P ? b[len-1] : 0;
 *      malformed if P and (pad == 0 or h + pad > len).  With F = channels[s] * B (B = 2 or 3 bytes) and payload = len - h - pad:
 *      malformed unless payload is a positive multiple of F; m = payload / F sample times.  No byte at or beyond len is read.
 *   2. A valid packet of a stream that is not running is IGNORED.  Otherwise d0 = (int32) (T - cursor), a wrapping subtraction
 *      read as signed (a stream may sit anywhere within 2^31 of its cursor and cross 2^32), and the packet covers the positions
 *      d0 .. d0 + m - 1: LATE if d0 < 0, EARLY if d0 + m > n (the caller submits such a packet again with the next tick, where its
 *      part before the new cursor is ignored), PLACED if any position lies in [0, n).
 *   3. Position q of stream s belongs to the valid, placed packet of the GREATEST index i that covers it; with none, it is missing.
 *   4. The block [C][n], rows back to back, samples of B bytes: for a track with source (s, j), s running and q owned by packet i,
 *      the B bytes at payload offset (q - d0_i) * F + j * B in reversed order (big to little endian); otherwise B zero bytes.
 *   5. Every result, the pending samples and the launch sequence after the unpack's entry are those of fx_push_samples on that
 *      block, bit for bit -- taps, onset events and the display included; a failure after samples have moved on leaves the stream
 *      as fx_push_samples describes.
 *
 * fx_rtp_get_block copies the last tick's block [C][n] (as fx_get_monitor the mix: *num_samples = n also where the capacity is
 * refused; host memory synchronous, device memory asynchronous on the context's stream).  fx_rtp_get_stats: per stream, summed
 * over the ticks since fx_rtp_configure with integer atomics on the device (synchronises): valid packets (ignored ones included),
 * malformed packets (of the stream stream_of names), valid packets entirely before / entirely after their tick, positions owned
 * and positions missing (running streams only).
 *
 * The unit is the slot's, not the analysers': fx_reset_state and fx_reset_channels do not touch it, fx_export_channels /
 * fx_import_channels do not carry it.  fx_push_samples, fx_push_interleaved, fx_push_sources, the fx_stream_* ring and the monitor do
 * not consult it, and a context that never calls fx_rtp_configure makes the launches it always made.
 * Not here: sockets (recvmmsg into pinned slots, multicast joins: the receiver this unit is fed by; what arrives early or out of
 * order it pushes as it comes, the reorder window below holds it), RTCP, SDP, filtering by SSRC or payload type, mixed formats in one context, AM824 / L32, and a fx_stream_* ring form. */
enum { FX_RTP_L16 = 0, FX_RTP_L24 = 1 };
enum { FX_RTP_PLACED = 1, FX_RTP_LATE = 2, FX_RTP_EARLY = 4, FX_RTP_MALFORMED = 8, FX_RTP_IGNORED = 16, FX_RTP_HELD = 32 };
#define FX_RTP_MAX_STREAMS 65536
#define FX_RTP_MAX_CHANNELS 64
#define FX_RTP_MAX_SLOT_STRIDE 65536
#define FX_RTP_MAX_WINDOW 65536            /* sample times: 1.37 s at 48 kHz */
typedef struct fx_rtp_stats {
    long long packets, malformed, late_packets, early_packets, samples_placed, samples_missing;
} fx_rtp_stats;
fx_status fx_rtp_configure(fx_context* ctx, int payload_format, int num_streams, const int* channels /*[num_streams]*/);
fx_status fx_rtp_set_track_sources(fx_context* ctx, const int* tracks, int num_tracks, const int* stream, const int* channel);
fx_status fx_rtp_get_track_sources(fx_context* ctx, int* stream /*[num_channels]*/, int* channel /*[num_channels]*/);
fx_status fx_rtp_set_cursors(fx_context* ctx, const int* streams, int num, const unsigned* rtp_time);
fx_status fx_rtp_get_cursors(fx_context* ctx, unsigned* rtp_time /*[num_streams]*/, int* running /*[num_streams]*/);
fx_status fx_push_rtp(fx_context* ctx, const void* packets, const int* lengths, const int* stream_of, int num_packets, int slot_stride,
                      int num_samples, int mem_kind, float* out_raw, float* out_smoothed, int* frames_out, unsigned char* disposition);
fx_status fx_rtp_get_block(fx_context* ctx, void* out, size_t capacity_bytes, int* num_samples, int* sample_format, int mem_kind);
fx_status fx_rtp_get_stats(fx_context* ctx, fx_rtp_stats* out /*[num_streams]*/);

/* ---- the RTP reorder window: early packets held on the GPU until their tick ----
 * On a network packets arrive ahead of the tick they belong to, and out of order.  With a window of W sample times the unit keeps,
 * per stream and in device memory, what a tick's packets own up to W sample times beyond the tick, and the tick that covers those
 * positions hears them: a packet is submitted once, when it arrives, in whichever tick and whatever order.  W = 0, where
 * fx_rtp_configure starts every unit (a re-configured one included, nothing held), is fx_push_rtp exactly as defined above: the same
 * launches, disposition bytes and statistics.
 *
 *   fx_rtp_set_window  window in 0 .. FX_RTP_MAX_WINDOW (judged before any device use), on a configured unit.  Synchronises the
 *                      context's stream and discards everything held, also when `window` is the current value.  What the new
 *                      window needs is allocated before the old state goes: a failure (FX_ERR_OUT_OF_MEMORY) leaves the unit as
 *                      it was.
 *   fx_rtp_get_window  the window and, where `out` is not NULL, per stream: `held`, the owned positions the stream holds now, and
 *                      `recovered`, the block positions, summed over the ticks since fx_rtp_configure or fx_rtp_set_window, that
 *                      were owned only through the held state.  Synchronises, as fx_rtp_get_stats.
 *
 * A tick (fx_push_rtp with n = num_samples > 0) of a running stream s works on a SPAN of n + W positions:
 *   1. Header validity is rule 1 above, unchanged.
 *   2. Position q of the span has RTP time cursor + q.  Before the tick's packets are looked at, positions [0, W) carry what the
 *      unit holds for s from earlier ticks, each either owned, with its wire bytes, or empty; positions [W, n + W) are empty.
 *   3. A valid packet i of a running stream, d0 = (int32) (T - cursor), m sample times, covers d0 .. d0 + m - 1: LATE if d0 < 0,
 *      EARLY if d0 + m > n + W, PLACED if any covered position lies in [0, n), HELD if any lies in [n, n + W).  (W = 0: rule 2
 *      above, and HELD never appears.)  MALFORMED and IGNORED are unchanged; packets of a stream that is not running are never held.
 *   4. A span position covered by one or more of this tick's valid packets belongs to the one of the greatest index, whose bytes
 *      replace whatever was held there; every other position keeps what 2. gave it.  The most recently submitted packet owns a
 *      position: a later tick beats an earlier one, within a tick the greater index wins.
 *   5. The block is rule 4 above over span positions [0, n): an owned position gives its bytes reversed, whether they came from a
 *      packet of this tick or from the held state, an empty one zeros.  Span positions [n, n + W) become the held positions
 *      [0, W) of the next tick, and the cursor moves on by n.  (n > W is legal: everything held is consumed.)
 *   6. Rule 5 above stands: from the unpack's entry on the tick is fx_push_samples of that block, bit for bit.
 *   7. fx_rtp_stats: packets and malformed as above, each datagram counted once, in the tick that received it; late_packets /
 *      early_packets count the valid packets of running streams that have no position in [0, n + W) and are LATE / EARLY;
 *      samples_placed counts, per tick, the owned positions of [0, n), whichever source they came from, samples_missing the empty.
 *
 * fx_rtp_set_cursors discards what the LISTED streams hold (their time base has moved); streams not listed keep theirs.  A tick
 * with num_samples == 0 stays a no-op: its packets are not looked at.  fx_rtp_set_track_sources does not touch the held state (it
 * is per stream and holds wire bytes: a track that changes source hears the new stream's held samples from its next tick on), nor
 * do fx_reset_state, fx_reset_channels, export / import or the other push calls.  A refused tick changes nothing, the held state
 * included; a failure after samples have moved on leaves the stream as fx_push_samples describes.
 * So: if no two packets of a stream overlap, and every packet is submitted in some tick whose span covers it whole, the blocks and
 * all analysis results do not depend on which tick each packet was submitted in, or on the order within a tick. */
typedef struct fx_rtp_window_stats { long long held, recovered; } fx_rtp_window_stats;
fx_status fx_rtp_set_window(fx_context* ctx, int window /* 0 .. FX_RTP_MAX_WINDOW sample times */);
fx_status fx_rtp_get_window(fx_context* ctx, int* window, fx_rtp_window_stats* out /*[num_streams], may be NULL*/);

/* ---- file sources: tracks play device-resident clips, transport on the GPU ----
 * In the reference every track listens either to the audio device or to its own AudioFilePlayer, a looping file behind play / pause /
 * stop / restart buttons (AudioFilePlayer.h:41-67, AnalyserTrackController.h:92-138, AudioFileTransportComponent.h:133-179).  Here a
 * file is a CLIP in device memory, a track's player is a row of a per-track table in device memory, and one call per tick,
 * fx_push_sources, gives every track its next n samples -- from the caller's live block or from the track's clip -- and analyses
 * them as fx_push_samples would.  So thousands of tracks play thousands of files of different lengths in one context, and no file
 * sample crosses the host link after its bank was made.
 *
 * CLIPS.  A clip is L >= 1 samples of one FX_SAMPLE_* format in device memory, at the context's sample rate unless
 * fx_set_clip_rates says otherwise (CLIPS AT THEIR OWN RATE, below).  Clips are made in
 * banks, one allocation and one copy per bank: `samples` holds num_clips (>= 1) clips back to back, lengths[k] samples each, in
 * FX_MEM_HOST or FX_MEM_DEVICE memory (device memory from a 4-byte boundary); the clips get the ids *first_id, *first_id + 1, ...
 * With FX_CLIP_BORROW (FX_MEM_DEVICE only) the bank is not copied: it refers to the caller's memory, which must stay valid and
 * unchanged until fx_destroy_clips.  Otherwise the copy is made on the context's stream: a host buffer may be reused on return, a
 * device buffer once the stream has reached the copy (fx_sync).  fx_destroy_clips takes the first id of a bank; it is refused
 * (FX_ERR_INVALID_ARGUMENT, nothing changes) while any track has one of the bank's clips loaded.  fx_destroy releases every bank.
 *
 * THE TABLE, one row per track, made by the first call of this section (a context on which none was made runs exactly the launches
 * it ran before):
 *   source    FX_SOURCE_INPUT (default) or FX_SOURCE_FILE
 *   state     FX_TRANSPORT_NO_FILE, _PLAYING, _PAUSED, _STOPPED (the reference's enum, in its order) and our own _FINISHED
 *   loop      1: the reference's setLooping(true) (AudioFilePlayer.h:53); 0: one-shot
 *   clip      the loaded clip's address and length L;  position (int64, samples);  laps (int64, completed passes of a looping clip)
 *
 * A TICK.  fx_push_sources forms num_samples samples for every track c:
 *   source INPUT:                row c of live_block, [num_channels][num_samples] as fx_push_samples takes it (FX_MEM_DEVICE: 4-byte
 *                                aligned).  live_block == NULL is allowed only while no track's source is INPUT.
 *   FILE, PLAYING, looping:      out[i] = clip[(position + i) mod L];  then laps += (position + n) div L, position = (position + n) mod L
 *   FILE, PLAYING, one-shot:     out[i] = clip[position + i] while position + i < L, zero samples after;  then position =
 *                                min(position + n, L), and the state becomes FINISHED if the old position + n >= L
 *   FILE in any other state:     n zero samples (all bytes zero in every format), as a stopped AudioTransportSource renders silence
 * and hands that planar block to the path of fx_push_samples: every result, the pending samples and the launch sequence after the
 * first launch (the gather) are those of fx_push_samples on the same block, bit for bit -- taps, onset events and the display
 * included.  The gain is the collector's: the load stage applies it to file audio as to live audio (AudioDataCollector.h:88).
 * fx_push_samples' rules and refusals hold unchanged, and all refusals come before any launch: a refused call changes nothing.
 * Every FILE track's loaded clip must have the call's sample_format, whatever its state (FX_ERR_INVALID_ARGUMENT names the track).
 * mem_kind covers live_block and the results.  Clip bytes and the table are read on the context's stream only.
 * fx_push_samples and fx_push_interleaved do not consult the table and advance no position.
 *
 * COMMANDS take a list of tracks under fx_reset_channels' rules: host memory, duplicates allowed (for the two setters the last
 * entry of a track wins), num_channels == 0 is a no-op, every entry -- track, clip id, source, command -- is checked before
 * anything changes and before any device use (FX_ERR_INVALID_ARGUMENT, fx_last_error names the entry); they synchronise the
 * context's stream and take effect in stream order.
 *   fx_set_channel_clips    the file-dropped callback (AnalyserTrackController.h:109-124): track channels[i] loads clip clip_ids[i]
 *                           (-1: no file), loop[i] != 0 looping (loop == NULL: all looping).  The state becomes STOPPED (NO_FILE for
 *                           -1), position and laps 0, and the tracks' pending samples become zeros.  The source is not changed.
 *   fx_set_channel_sources  (:92-107) types[i] is FX_SOURCE_INPUT or FX_SOURCE_FILE.  Going to INPUT stops the player (STOPPED if it
 *                           has a clip, position 0); going to FILE keeps the player's state.  Either way the tracks' pending samples
 *                           become zeros, even when the type does not change (toggleCollectInput, AudioDataCollector.h:119).
 *   fx_transport            FX_PLAY     STOPPED or PAUSED -> PLAYING; FINISHED -> position 0, PLAYING; PLAYING stays.  A listed
 *                                       track without a clip refuses the whole call.
 *                           FX_PAUSE    PLAYING -> PAUSED; other states unchanged
 *                           FX_STOP     any state with a clip -> STOPPED, position 0
 *                           FX_RESTART  position 0; FINISHED -> STOPPED, otherwise the state is kept
 *                           PLAY, PAUSE and STOP zero the tracks' pending samples (clearAnalysisBuffers, :135-137); RESTART does not
 *                           (:138).  RESTART keeping the state is the engine's behaviour (AudioFilePlayer.h:65), not the GUI's label
 *                           (AudioFileTransportComponent.h:165 shows "playing" after a restart while paused).  FINISHED is known on
 *                           the device only: one launch over the list applies the command there.
 *   fx_get_transport        the whole table, [num_channels] each in host memory; any pointer may be NULL.  Synchronises.
 * None of these calls touches the display (pair them with fx_clear_display_channels where the reference's GUI does).
 * fx_reset_state and fx_reset_channels leave the table alone: it is the player's state, not the analysers'.  Records of
 * fx_export_channels do not carry it: like the display it belongs to the slot.
 *
 * CLIPS AT THEIR OWN RATE.  The reference hands the reader's rate to its transport source "for sample rate correction"
 * (AudioFilePlayer.h:55-58): a 44.1 kHz file keeps its pitch on a 48 kHz device.  fx_set_clip_rates gives clip clip_ids[i] the rate
 * sample_rates[i] in Hz; 0, every clip's default, means the context's rate.  The lists follow fx_reset_channels' rules (host memory,
 * num_clips == 0 is a no-op, of a duplicate id the last entry wins); every entry is checked before anything changes and before
 * any device use (an unknown id; a rate that is NaN, infinite or negative); and the call is refused, naming the track, while a
 * listed clip is loaded on any track: the rate is the file's and is set before loading.
 *   At fx_set_channel_clips a track is RATED if its clip's rate is neither 0 nor the context's sample rate.  The host forms
 * r = clip rate / context rate and rho = min(1, 1/r) in fp64 and J = ceil(Z / rho); they go into the track's row, so the device never
 * divides.  r outside [1/8, 8] refuses the load, naming the entry.  The host remembers the context's rate at the load of every clip
 * with a rate of its own: after a later fx_set_sample_rate, fx_push_sources is refused (FX_ERR_INVALID_ARGUMENT names the track,
 * nothing changes) while a FILE track holds such a clip, until the clip is loaded again.
 *   A rated clip may be in any FX_SAMPLE_* format: the resampler widens it as the load stage would and renders fp32.  So while any
 * FILE track has a rated clip loaded, whatever its state, a tick must be FX_SAMPLE_F32 (refused otherwise, naming the track); the
 * unrated FILE clips keep their rule.  The launch record then holds the resampler's launch after the gather's; a context without a
 * rated clip on a FILE track runs exactly the launches it ran before.
 *   The resampler is ours (JUCE's is not in the reference tree) and this is its specification.  THE TABLE is one side of a
 * Kaiser-windowed sinc with Z = 16 zero crossings, P = 512 phases and beta = 9:
 *   T[i] = fl32(sinc(i/P) * I0(beta * sqrt(1 - (i/(P*Z))^2)) / I0(beta)) for 0 <= i < Z*P, computed on the host in fp64;
 *   T[Z*P] = T[Z*P + 1] = +0: Z*P + 2 entries.  fx_get_resampler_table copies them to out[capacity] (host only: no device, no
 *   context; refused if capacity < Z*P + 2) and reports Z and P.  The kernel reads a device copy of the same table.
 * A rated track's row carries k (int64), the outputs rendered since its position was last set to 0: a load, FX_STOP, FX_RESTART,
 * a switch to INPUT and FX_PLAY from FINISHED set k to 0, FX_PAUSE keeps it.  A tick of n samples renders, while the track is
 * PLAYING (zeros otherwise, as for any FILE track), output k' = k + i for 0 <= i < n, every operation IEEE in the stated type, none
 * contracted:
 *   x = fl64(k') * r;  i0 = floor(x);  f = x - i0;  acc = +0 (fp32);  for j = -(J-1) .. J, ascending:
 *     a = |fl64(j) - f| * rho; a tap with a >= Z is not added;  q = a * P;  i = floor(q);  t = fl32(q - i);
 *     c = T[i] + t * (T[i+1] - T[i]) (fp32);  m = i0 + j;  looping: s = widen(clip[m mod L]), the mathematical modulo; one-shot: a tap
 *     with m outside [0, L) is not added;  acc = acc + c * s (fp32)
 *   out = acc * fl32(rho), and for a one-shot out = +0 where x >= L.
 * After the tick k = k + n and, with x' = fl64(k) * r: looping: position = floor(x') mod L, laps = floor(x') div L; one-shot: position
 * = min(floor(x'), L) and the state is FINISHED iff x' >= L.  fx_get_transport reports these.  The gain stays the load stage's.
 * x depends on the absolute k' alone, so any cut of a stream into ticks gives the same samples bit for bit.  The phase resolution
 * falls as k grows: ulp(x) is 2^-20 source samples after 2^32 outputs.  The tests reach no k beyond what their ticks add up to: the
 * conversion of a 64-bit k to fp64 is untested on the device beyond that.
 *
 * Deliberate differences from the reference.  JUCE's AudioTransportSource is not part of the reference tree: its fade on stop and
 * its read-ahead buffer are not reproduced, and its sample-rate correction (JUCE's ResamplingAudioSource, absent as well) is
 * replaced by the windowed-sinc resampler specified above, so a rated clip's samples are ours, not JUCE's.  By default each track's
 * ANALYSERS hear its own player; in the reference every player renders into the sound card's shared output buffers and a file
 * track's collectors read one channel of those.  The shared output is the monitor mix (next section), and a track is told to hear
 * it with fx_set_channel_listen ("Listening tracks" there).  One-shot playback and FINISHED are ours. */
enum { FX_SOURCE_INPUT = 0, FX_SOURCE_FILE = 1 };
enum { FX_TRANSPORT_NO_FILE = 0, FX_TRANSPORT_PLAYING = 1, FX_TRANSPORT_PAUSED = 2, FX_TRANSPORT_STOPPED = 3, FX_TRANSPORT_FINISHED = 4 };
enum { FX_PLAY = 0, FX_PAUSE = 1, FX_STOP = 2, FX_RESTART = 3 };
enum { FX_CLIP_BORROW = 1 };
fx_status fx_create_clips(fx_context* ctx, const void* samples, const long long* lengths, int num_clips, int sample_format,
                          int mem_kind, unsigned flags, int* first_id);
fx_status fx_destroy_clips(fx_context* ctx, int first_id);
fx_status fx_set_channel_clips(fx_context* ctx, const int* channels, int num_channels, const int* clip_ids, const int* loop);
fx_status fx_set_clip_rates(fx_context* ctx, const int* clip_ids, int num_clips, const double* sample_rates);
fx_status fx_get_resampler_table(float* out, int capacity, int* zero_crossings, int* phases);
fx_status fx_set_channel_sources(fx_context* ctx, const int* channels, int num_channels, const int* types);
fx_status fx_transport(fx_context* ctx, const int* channels, int num_channels, int command);
fx_status fx_get_transport(fx_context* ctx, int* source, int* state, long long* position, long long* laps);
fx_status fx_push_sources(fx_context* ctx, const void* live_block, int num_samples, int sample_format, int mem_kind,
                          float* out_raw, float* out_smoothed, int* frames_out);

/* ---- monitor mix: every tick's tracks summed to a stereo output on the GPU ----
 * The reference's AudioFilePlayer is an AudioSourcePlayer on the device manager (AudioFilePlayer.h:30-34): a file is heard, every
 * player renders into the sound card's output buffers and the speakers carry the sum of the tracks that play.  The MONITOR is that
 * output, opt-in: while it is enabled every fx_push_sources tick also mixes the tick's planar block [C][n] down to two output
 * channels [2][n] of fp32 in device memory, through a per-track SEND table (on / off, left gain, right gain), at the cost of one
 * more launch record on the context's stream.  A context that never enables it makes exactly the launches it made before; an
 * enabled context returns exactly the analysis bits it returned before.
 *
 *   fx_enable_monitor       enable != 0 makes the monitor: every track's send off with gains 1.0 / 1.0, no tick yet (num_samples 0).
 *                           enable == 0 frees it.  Enabling an enabled monitor keeps the sends.  Synchronises the stream.  A failed
 *                           allocation is FX_ERR_OUT_OF_MEMORY and changes nothing.
 *   fx_set_channel_monitor  a list under fx_reset_channels' rules (host memory, duplicates allowed and the last entry of a track
 *                           wins, num_channels == 0 is a no-op): on[i] != 0 puts track channels[i] on (on == NULL: every listed
 *                           track on); left == NULL and / or right == NULL keep that gain.  Every entry is checked before anything
 *                           changes and before any device use, fx_last_error names the entry: a gain that is NaN or infinite, a
 *                           track out of range.  Refused without a monitor.  Takes effect in stream order, at the next tick.
 *   fx_get_channel_monitor  the whole table, [num_channels] each in host memory; any pointer may be NULL.
 *   fx_get_monitor          copies the last tick's mix: out[0 .. n) is left and out[capacity .. capacity + n) right, n that tick's
 *                           num_samples, reported in *num_samples.  capacity < n is refused (the error names both numbers, and
 *                           *num_samples still reports n: a host learns what room to bring).
 *                           FX_MEM_HOST returns when the bytes are there; FX_MEM_DEVICE needs 4-byte alignment and is
 *                           asynchronous on the context's stream.  Refused before any device use: a null context, a null out,
 *                           an unknown memory kind, a context without a monitor.
 *
 * THE MIX.  x_c[i] is sample i of track c's row of the tick's planar block, after the gather and, if it ran, the resampler, widened
 * exactly as the analysis kernels' load stage widens it: f32 as is, f16 the exact float, s16 v / 32768, s24 v / 8388608.  The
 * collector's gain (fx_set_gain, fx_set_channel_gains) is the analysers' and is NOT applied: the reference's gain slider does not
 * change what is heard either.  The track groups are g = 0 .. ceil(C / FX_MONITOR_GROUP) - 1, group g holds tracks 64 g .. 64 g + 63.
 * For each output channel ch with gains gain_ch and each sample i:
 *   P_g = +0;  for c ascending over group g's tracks whose send is on:  P_g = P_g + (gain_ch[c] * x_c[i])
 *   out = +0;  for g ascending:                                         out = out + P_g
 * Every operation is IEEE fp32, round to nearest, none contracted.  A track whose send is off contributes nothing: it is not added
 * as 0 * x, so an inf or NaN in an off track never reaches the output.  A group with no track on adds +0, which changes no bit (the
 * accumulators start at +0 and are never -0).  The fixed two-level order makes the result one defined bit pattern whatever the
 * launch geometry: a flat sequential sum over 65 536 tracks would serialise the kernel, float atomics would make the bits depend
 * on timing -- there are none.
 *   What is mixed is whatever the tick gave each track: an INPUT track's live row (so "input monitoring" is turning an INPUT
 * track's send on), a playing clip, zeros for a FILE track in any other state.  fx_push_samples, fx_push_interleaved, fx_push_hops,
 * fx_process_frames and the fx_stream_* ring do not feed the monitor, and a tick of num_samples == 0 leaves the last mix alone.
 * Like the players' table the sends belong to the slot: fx_reset_state and fx_reset_channels leave them, records of
 * fx_export_channels do not carry them.
 *   In a tick the mix follows the gather and the resampler and precedes everything fx_push_samples does; whatever can fail (the
 * partial sums' and the output's memory among it) fails before the gather is launched: a refused tick changes nothing, the
 * monitor included.  Not here: more than two outputs, a history beyond the last tick, fades, a master gain.  Tracks hearing each
 * other's players: "Listening tracks", below.
 *
 * LISTENING TRACKS.  Switching a track of the reference to "audio file" calls toggleCollectInput (false) on both of its collectors
 * (AnalyserTrackController.h:92-107): from then on audioDeviceIOCallback copies outputChannelData[channelToCollect], not the input
 * (AudioDataCollector.h:42,53), with the collector's gain applied on the way in as always (:88).  A file track's analysers never
 * read their own player: they read one channel of the device's output buffer, the sum of every player.  Here a track is told to
 * LISTEN to the left or the right monitor output, and its analysers, taps, display, onset events and pending samples see what
 * those collectors would see; no sample leaves device memory on the way.
 *
 *   fx_set_channel_listen   a list under fx_set_channel_monitor's rules (host memory, duplicates allowed and the last entry of a
 *                           track wins, num_channels == 0 is a no-op): track channels[i] hears listen[i], FX_LISTEN_SELF (its own
 *                           row, the default), FX_LISTEN_LEFT or FX_LISTEN_RIGHT.  Every entry is checked before anything changes
 *                           and before any device use, fx_last_error names the entry.  Refused: a null context, a negative count,
 *                           a null list, a null `listen`, a value outside {0, 1, 2}, a track out of range, a context without a
 *                           monitor.  Takes effect in stream order, at the next tick.  Zeroes the listed tracks' pending samples
 *                           (fx_clear_pending_channels), also where the value does not change: toggleCollectInput clears the
 *                           collector whichever way it is switched (AudioDataCollector.h:119).
 *   fx_get_channel_listen   the whole column, [num_channels] in host memory.  Refused: a null context, a null `listen`, a context
 *                           without a monitor.
 *
 *   1. Where a listen lives.  It is a column of the send table, FX_LISTEN_SELF when the monitor is made.  Like the sends it belongs
 * to the slot: fx_reset_state, fx_reset_channels and fx_export_channels / fx_import_channels neither touch nor carry it.
 *   2. fx_enable_monitor (ctx, 0) is refused with FX_ERR_INVALID_ARGUMENT, naming the first such track, while any track listens to
 * an output, and changes nothing -- the rule fx_destroy_clips applies to loaded clips.  Disabling a monitor nobody listens to
 * behaves as before.
 *   3. The tick.  For every track c with listen != FX_LISTEN_SELF, row c of the tick's planar block becomes the mix:
 * planar[c][i] = out[listen - 1][i] for 0 <= i < n, bit for bit -- a NaN or inf in the mix is heard as it is.  This happens after the
 * mix and the groups' sum and before anything fx_push_samples would do.  The mix is formed from every track's OWN row first (live
 * row, clip, resampler output or silence): a listening track's send still contributes its own source, nothing feeds back, and the
 * mix of a tick is the same bits whether anybody listens or not.  No byte of a non-listening track's row changes.  Everything
 * downstream equals fx_push_samples on that modified block: the load stage with the track's collector gain, taps, display, onset
 * events, pending samples.
 *   4. Sample format.  The mix is fp32: while any track listens an fx_push_sources tick must be FX_SAMPLE_F32; any other is refused
 * before any launch, naming the first listening track, and changes nothing (the rule of rated clips).  A tick of num_samples == 0
 * does nothing.
 *   5. Launches.  A context in which no track listens makes exactly the launches it made before.  With a listener a tick makes one
 * more, directly after the monitor's.
 *   6. Ticks only.  fx_push_samples, fx_push_interleaved, fx_push_hops, fx_process_frames and the fx_stream_* ring do not consult the
 * listens.
 *   7. A documented difference: -0.  With one send on at gains (1, 0), a track listening FX_LISTEN_LEFT hears its own player, except
 * that a -0 sample arrives as +0: the accumulators start at +0, and +0 + -0 is +0. */
#define FX_MONITOR_GROUP 64
enum { FX_LISTEN_SELF = 0, FX_LISTEN_LEFT = 1, FX_LISTEN_RIGHT = 2 };
fx_status fx_enable_monitor(fx_context* ctx, int enable);
fx_status fx_set_channel_monitor(fx_context* ctx, const int* channels, int num_channels, const int* on, const float* left,
                                 const float* right);
fx_status fx_get_channel_monitor(fx_context* ctx, int* on, float* left, float* right);
fx_status fx_get_monitor(fx_context* ctx, float* out, int capacity, int* num_samples, int mem_kind);
fx_status fx_set_channel_listen(fx_context* ctx, const int* channels, int num_channels, const int* listen);
fx_status fx_get_channel_listen(fx_context* ctx, int* listen);   /* [num_channels], host */

/* Same analysis on already assembled windows (the `audioWindow` each run()
 * loop sees, RealTimeAnalyser.h:147,206): frames [num_channels][num_frames]
 * [window_size].  Gain is not applied.  The overlap state is left holding the
 * second half of each channel's last frame. */
fx_status fx_process_frames(fx_context* ctx, const void* frames, int num_frames, int sample_format,
                            int mem_kind, float* out_raw, float* out_smoothed);

/* Latest AudioFeatures::getValue of every slot, [num_channels][12]
 * (what OSCFeatureAnalysisOutput::sendSpectralFeaturesViaOSC samples,
 * OSCFeatureAnalysisOutput.h:91-104). */
fx_status fx_get_smoothed(fx_context* ctx, float* out, int mem_kind);

/* Page-locked host memory for buffers a host hands to the FX_MEM_HOST entry points again and again (a live engine's block FIFO, its result
 * buffers): copies to and from it run at the link's rate, where ordinary memory goes through the runtime's staging copy first.  Needs a
 * device (FX_ERR_NO_DEVICE without one); any thread; free with fx_host_free.  Using it is optional: every entry accepts ordinary memory. */
fx_status fx_host_alloc(void** out, size_t bytes);
fx_status fx_host_free(void* p);

/* Wait for all enqueued work of this context.  FX_ERR_HIP if a kernel of this context reported a failed
 * hand-over between work units (the results of that call and of the calls after it are not valid;
 * fx_reset_state clears the condition). */
fx_status fx_sync(fx_context* ctx);

/* The context's hipStream_t (as void*), so callers can order their own copies. */
fx_status fx_get_stream(fx_context* ctx, void** stream);

/* Device time of the analysis kernels of the most recent fx_push_hops /
 * fx_process_frames / fx_push_samples call that analysed frames, measured with HIP
 * events on the context's stream (milliseconds; synchronises). kernel 0 = frame
 * kernel, 1 = smoothing/onset. FX_ERR_INVALID_ARGUMENT if that call recorded none:
 * by default calls made of one-frame launches do not (fx_tuning::call_timing). */
fx_status fx_last_kernel_ms(fx_context* ctx, float* frame_kernel_ms, float* epilogue_kernel_ms);

/* ---- analysis taps: the analysers' display buffers, what PitchEstimationVisualiser.h draws ----
 * The reference hands a host what its analysers saw through one-shot flags: each enable...NeedsUpdating call makes the next frame
 * analysed copy one buffer, and clears the flag (RealTimeAudioAnalysis.h:221-232, :268-283; PitchAnalyser.h:30-53,66-72,187).
 * Here one request arms all five of them for a set of channels:
 *   - requests accumulate: channels armed by calls before an analysis call are served together by that call; arming a channel that
 *     is already armed changes nothing.  More than FX_MAX_TAP_CHANNELS distinct armed channels, a channel outside [0, num_channels)
 *     or a null context is FX_ERR_INVALID_ARGUMENT, before any device use.
 *   - the first later fx_push_hops, fx_process_frames or fx_push_samples call that analyses at least one frame serves every armed
 *     channel: it captures the FIRST frame it analyses (the reference's one-shot flag), and the request is cleared.  A fx_push_samples
 *     call that completes no hop leaves the request armed, and so do the fx_stream_* ring submissions (their captured steps are not
 *     changed by taps).
 *   - the capture is made by one extra launch on the context's stream, enqueued before anything of the call that changes the
 *     context's state; if it fails the call returns the error with the context untouched and the request still armed.  With nothing
 *     armed an analysis call makes exactly the launches it makes without taps.
 *   - one capture at a time: a new capture replaces the old one whole.  fx_reset_state drops the request and the capture.
 *   - every buffer is formed whatever analysers the context runs (FX_SPECTRAL_ONLY, FX_HARMONIC_ONLY, FX_LOW_LATENCY): the buffers
 *     depend on the window alone, and each is bit for bit what the reference's arithmetic makes of that window. */
#define FX_MAX_TAP_CHANNELS 64
/* Arm the display buffers of these channels (the reference's enable...NeedsUpdating calls, all five at once). */
fx_status fx_request_taps(fx_context* ctx, const int* channels, int num_channels);
/* Host copies of the latest capture for `channel`; any pointer may be NULL.  FX_ERR_INVALID_ARGUMENT if the latest capture does
 * not hold `channel` (or there is none).  May synchronise the context's stream.
 *   window          [N]   the overlapped window of the captured frame, RealTimeAudioDataOverlapper::getBufferToDraw: the channel's
 *                         carried second half, then the first new hop times the gain (fx_push_hops; fx_push_samples: the first N/2
 *                         samples of [pending | block]), or the frame as given, without gain (fx_process_frames); not windowed
 *   spectrum        [2N]  (re, im) pairs of the Bartlett-windowed window's transform: the spectral analyser's getFFTBufferToDraw
 *   pitch_spectrum  [2N]  the same of the low-passed, windowed window: the harmonic analyser's getFFTBufferToDraw
 *                         (its first getFrequencyData, RealTimeAnalyser.h:160)
 *   autocorrelation [N]   getAutoCorrelationBufferToDraw: v[s] = d[s] * d[s] * s of the inverse transform d of the squared real parts
 *   cnd             [N]   getCumulativeDifferenceBufferToDraw: the cumulative normalised difference of v
 *   lag_position    [2]   getNormalisedLagPosition: (lag / 2N, cnd[lag]), or (-1 / 2N, 100) when no value fell below the threshold
 *   frame_index     which frame of the channel's stream was captured: frames analysed since fx_create / fx_reset_state / the channel's
 *                   last fx_reset_channels, 0-based */
fx_status fx_get_taps(fx_context* ctx, int channel, float* window, float* spectrum, float* pitch_spectrum,
                      float* autocorrelation, float* cnd, float* lag_position, long long* frame_index);

/* ---- onset events: every track's onset callback as one list made on the GPU ----
 * RealTimeSpectralAnalyser::run calls onsetDetectedCallback() after any frame whose onset slot is above zero
 * (RealTimeAnalyser.h:228-229, :256), and AnalyserTrackController.h:80-84 binds that callback per track.  Here a context on which
 * the list is enabled appends one record per (track, frame) to a list in device memory, and the host drains it when it likes:
 *   - an event is exactly raw[FX_ONSET] == 1.0f of a frame analysed by fx_push_hops, fx_process_frames, fx_push_samples or
 *     fx_push_interleaved: the reference's condition, since getValue(enOnset) has history length 1 and so equals the value just
 *     inserted.  A FX_HARMONIC_ONLY context never produces one (the reference never writes its onset slot, and NaN > 0 is false).
 *   - `frame` is the frame's 0-based index in the track's OWN stream since fx_create / fx_reset_state / the track's last
 *     fx_reset_channels, the count fx_get_taps reports as frame_index; `call_frame` its index within the call that analysed it;
 *     `channel` the track.
 *   - order: events of earlier calls first, within a call by ascending call_frame, then ascending channel.  While no track was
 *     reset on its own the whole list is therefore sorted by (frame, channel); it can always be replayed in time order.  The order
 *     is part of the contract: it is a function of the onset slots alone.
 *   - events beyond `capacity` are not stored and are counted: the stored ones are the earliest.
 *   - the list is made by one extra launch on the context's stream after the call's last analysis launch.  The number of events
 *     stored lives in device memory: an analysis call on an enabled context makes no host wait it does not make otherwise, and
 *     the results it returns are the bits it returns with the list disabled.  The call's raw vectors need not go to the caller:
 *     out_raw (and out_smoothed) may be NULL.  If that launch fails the analysis call returns FX_ERR_HIP and, as after a failed
 *     analysis launch of fx_push_samples, the stream is fx_reset_state's.  On a context that never enabled the list an analysis
 *     call makes exactly the launches it made before.
 *   - fx_reset_state empties the list and zeroes the overflow count; the list stays enabled and keeps its capacity.
 *   - the fx_stream_* ring does not produce events, as it does not serve taps: its captured steps stay as they are. */
typedef struct fx_onset_event { long long frame; int channel; int call_frame; } fx_onset_event;   /* 16 bytes */
/* capacity > 0: enable the list with room for `capacity` events, or resize it (the events stored are dropped); 0: disable it and
 * free its memory.  Synchronises the context's stream.  A null context, a negative capacity or one above 2^26 is
 * FX_ERR_INVALID_ARGUMENT, before any device use. */
fx_status fx_enable_onset_events(fx_context* ctx, int capacity);
/* Synchronises the context's stream, copies the min(stored, cap) oldest events to `out`, removes exactly those from the list (the
 * rest stay for the next call) and sets *count to their number; *dropped = the events lost to overflow since the previous drain,
 * and that count starts again.  out == NULL with cap == 0 only reports: *count = the events stored, *dropped = the count so far,
 * nothing removed or cleared.  count and dropped may be NULL.  FX_ERR_INVALID_ARGUMENT, before any device use: a null context,
 * cap < 0, out == NULL with cap > 0, a context on which the list is not enabled. */
fx_status fx_get_onset_events(fx_context* ctx, fx_onset_event* out, int cap, int* count, long long* dropped);

/* ---- audio display levels: every track's scrolling waveform, made on the GPU ----
 * AnalyserTrackController.h:74-78 binds setBufferToDrawUpdatedCallback on the harmonic collector; AudioDataCollector::getAnalysisBuffer
 * (AudioDataCollector.h:88-91) calls it with every gained hop it hands out, and AnalyserTrack::updateBufferToPush (AnalyserTrack.h:148-157)
 * pushes that hop into an AudioVisualiserComponent set up with setSamplesPerBlock (256) and setBufferSize (1024) (AnalyserTrack.h:27-29).
 * Per track the component keeps a ring levels[L] of (lo, hi) pairs, a running pair `value`, and the ints `sub` and `next`, all zero in
 * a new component, and runs for every sample x of every hop, in order:
 *     if (--sub <= 0) { next %= L; levels[next++] = value; sub = samplesPerBlock; value = (x, x); }
 *     else { lo' = lo < x ? lo : x;  t = x < hi ? hi : x;  hi' = lo' < t ? t : lo';  value = (lo', hi'); }
 * Here a context on which the display is enabled keeps that state per track in device memory, bit for bit:
 *   - a block is published one sample late, when the first sample of the next block arrives; the first entry published by a new or
 *     cleared component is (0, 0); equal values take the newer sample (so the sign of a zero is the latest one's); a NaN sample makes
 *     both ends NaN, and the next sample replaces both.
 *   - the display receives exactly the hops a call analyses, as the analysers read them: fx_push_hops, fx_push_samples and
 *     fx_push_interleaved show each analysed hop's N/2 samples, widened as the load stage widens them and times the gain in force
 *     for that track (the float the `window` tap shows in its second half); fx_process_frames shows the second half of each frame
 *     as given, without gain.  Pending samples are not shown until their hop completes.  The fx_stream_* ring does not feed the
 *     display, as it does not serve taps or events.
 *   - it is made by one extra launch on the context's stream per analysis call; the results an enabled context returns are the bits
 *     it returns with the display disabled, and a context that never enabled it makes exactly the launches it made before.
 *   - fx_reset_state makes every track a new component, fx_reset_channels the listed tracks (sub and next are per track, so tracks
 *     may stand at different phases); fx_clear_pending* does not touch the display.  The display belongs to the slot:
 *     fx_export_channels / fx_import_channels records do not carry it. */
/* buffer_size in [1, 4096]: enable the display with rings of buffer_size levels, or resize it; every track becomes a new component
 * publishing every samples_per_block (in [1, 65536]) samples.  buffer_size 0: disable it and free its memory.  Memory:
 * num_channels x buffer_size x 8 bytes, and two 16-byte state records per track (a call reads one and writes the other).  A failed
 * allocation is FX_ERR_OUT_OF_MEMORY and leaves the old display in force.  Synchronises the context's stream.  A null context or a
 * value out of range is FX_ERR_INVALID_ARGUMENT, before any device use. */
fx_status fx_enable_display(fx_context* ctx, int samples_per_block, int buffer_size);
/* setSamplesPerBlock (AnalyserTrackController.h:154-158): only the int is replaced -- the running block keeps its `sub` -- and the
 * new value takes effect with the next sample in stream order.  FX_ERR_INVALID_ARGUMENT, before any device use: a null context, a
 * value outside [1, 65536], a context without a display. */
fx_status fx_set_display_samples_per_block(fx_context* ctx, int samples_per_block);
/* clear() on the listed tracks (clearAudioDisplayData, AnalyserTrackController.h:105,114): levels, value and sub become zero, next
 * stays.  channels / num_channels follow fx_reset_channels.  FX_ERR_INVALID_ARGUMENT, before any device use: a null context, a bad
 * list (fx_last_error names the entry), a context without a display. */
fx_status fx_clear_display_channels(fx_context* ctx, const int* channels, int num_channels);
/* The listed tracks' rings in drawing order, oldest first -- levels[(next + k) % L] for k = 0 .. L-1, as the component draws them
 * -- to levels [num_channels][L][2] floats, after the analysis calls made so far.  channels == NULL with num_channels == the
 * context's channel count means all tracks.  FX_MEM_HOST returns when the bytes are there; FX_MEM_DEVICE (4-byte aligned) is
 * asynchronous on the context's stream.  FX_ERR_INVALID_ARGUMENT, before any device use: a null context or buffer, an unknown
 * memory kind, a bad list (fx_last_error names the entry), a context without a display. */
fx_status fx_get_display(fx_context* ctx, const int* channels, int num_channels, float* levels, int mem_kind);

/* ---- streaming ingest: replaces AudioDataCollector's ring + busy-wait reader ----
 * (AudioDataCollector.h:24,36-94: audio thread writes a 4096-sample ring, the analysis thread spins
 * until a hop is available.)  Here the producer owns a ring of `slots` PINNED host batches, each
 * [num_channels][hops_per_batch][window_size/2] samples of `sample_format` (any of FX_SAMPLE_*).
 * fx_stream_submit() enqueues the H2D copy of the filled slot on a side HIP stream, its analysis on the
 * context's stream behind an event and the copy of the vectors back on a third stream, so the samples
 * of batch k+1, the kernels of batch k and the results of batch k-1 travel at the same time (PCIe in
 * both directions while the kernels run: 94-98 % of the pinned-memcpy rate on MI355X for batches of
 * tens of megabytes); results return in submission order.
 * With hops_per_batch == 1 -- the reference's own cadence, one analysis per hop as it arrives -- a
 * submit is ONE kernel launch that reads the hop from the pinned slot, writes the vectors back to it
 * and raises a flag that fx_stream_collect() polls (32-33 us per 4096-sample window on MI355X; 29 us
 * with FX_LOW_LATENCY). */
typedef struct fx_stream fx_stream;
fx_status fx_stream_create(fx_context* ctx, int hops_per_batch, int slots, int sample_format, fx_stream** out);
fx_status fx_stream_destroy(fx_stream* s);
/* Next free slot to fill (pinned host memory).  Never blocks: FX_ERR_INVALID_ARGUMENT while every slot is still in flight
 * (fx_stream_collect frees the oldest) or while an acquired slot has not been submitted. */
fx_status fx_stream_acquire(fx_stream* s, void** host_slot);
/* Hand the acquired slot to the GPU (asynchronous). */
fx_status fx_stream_submit(fx_stream* s);
/* acquire + copy + submit for a producer whose batch sits in ordinary host memory: `hops` ([num_channels][hops_per_batch]
 * [window_size/2] samples of the stream's format) is copied into the next pinned slot by `fill_threads` host threads (1..64; a
 * persistent pool inside the stream: one memcpy thread moves ~12 GB/s, PCIe Gen5 takes 55) and the slot is submitted.  A
 * producer that can write its samples into the slot directly (fx_stream_acquire) saves that copy altogether. */
fx_status fx_stream_push(fx_stream* s, const void* hops, int fill_threads);
/* Wait for the OLDEST submitted batch and copy its results out: raw / smoothed
 * [num_channels][hops_per_batch][12] host floats (either may be NULL).  FX_ERR_INVALID_ARGUMENT
 * if nothing is in flight. */
fx_status fx_stream_collect(fx_stream* s, float* out_raw, float* out_smoothed);
/* The ring's form of fx_push_samples: the acquired slot holds a block of num_samples samples per channel, [num_channels]
 * [num_samples] with rows back to back, 0 <= num_samples <= hops_per_batch * window_size/2 (a device callback's block, or several
 * of them); the context's pending samples and the block are cut into hops on the device, analysed, and the rest is kept.  The
 * batch yields frames = (pending + num_samples) / (window_size/2) vectors per channel, which fx_stream_collect_samples reports.
 * Always the three-queue path (samples in, kernels, vectors back).  If it fails the slot is handed back and the ring stays usable, but -- as
 * with fx_push_samples -- the pending samples may have moved on without the hops this block completed: fx_reset_state, do not submit the
 * same block again. */
fx_status fx_stream_submit_samples(fx_stream* s, int num_samples);
/* acquire + copy (fill_threads host threads) + fx_stream_submit_samples for a block in ordinary host memory */
fx_status fx_stream_push_samples(fx_stream* s, const void* samples, int num_samples, int fill_threads);
/* fx_stream_collect that also says how many frames per channel the batch produced: raw / smoothed [num_channels][frames][12]
 * (room for hops_per_batch frames per channel is always enough) */
fx_status fx_stream_collect_samples(fx_stream* s, float* out_raw, float* out_smoothed, int* frames_out);
/* Number of submitted batches not yet collected. */
int fx_stream_in_flight(fx_stream* s);

/* ---- launch-shape knobs (experiments, tests) ----
 * Within a kernel family none of these changes a result bit (tests/test_gpu_parity.py pins that); they choose workgroup
 * shapes, how long calls are cut into work units, and which of the equivalent streaming paths runs.  The one knob that
 * selects a FAMILY is waves_per_frame (see FX_LOW_LATENCY): fx_set_tuning refuses to change it once the context has
 * analysed frames (FX_ERR_INVALID_ARGUMENT until fx_reset_state), so the two are never mixed in one history.  A context
 * takes its knobs ONCE, in fx_create, from the FX_* environment variables named below (later changes of
 * the environment have no effect: no entry point on the analysis path reads the environment);
 * fx_set_tuning replaces them explicitly.  A stream takes the stream_* knobs in fx_stream_create. */
#define FX_MAX_UNITS 24
typedef struct fx_tuning {
    int waves_per_channel;       /* FX_WAVES: frames of one channel in flight in a workgroup; 0 = measured best */
    int channels_per_workgroup;  /* FX_CHANNELS_PER_WG; 0 = measured best */
    int waves_per_frame;         /* FX_WAVES_PER_FRAME: kernel family -- 1 = a frame lives in one wavefront, 2 = in a pair of wavefronts
                                    (windows >= 2048 only); 0 = as the create flags say (pairs with FX_LOW_LATENCY, else one) */
    int frames_per_unit;         /* FX_FRAMES_PER_CHUNK: work-unit length of a call cut in time; 0 = never cut; -1 = measured best */
    int unit_plan_len;           /* FX_CHUNK_PLAN=a,b,...: explicit unit lengths (used when they add up to the call's frames) */
    int unit_plan[FX_MAX_UNITS];
    int stream_graph;            /* FX_STREAM_GRAPH: 1 / 0 force / forbid the captured hipGraph step; -1 = by batch size */
    int stream_hop_kernel;       /* FX_STREAM_HOP_KERNEL: 0 forbids the one-launch hop kernel in the ring; -1 = when it applies */
    int stream_zero_copy;        /* FX_STREAM_ZEROCOPY: 1 / 0 force / forbid zero-copy slots in the captured step; -1 = by size */
    int one_hop_kernel;          /* FX_ONE_HOP_KERNEL: 0 / 1 = fx_push_hops / fx_process_frames of ONE frame per channel never / always run
                                    the one-launch hop kernel; -1 = where it is the faster of the two (channels x window <= 2^20 samples; 2^22 for 4096-point windows on the default family) */
    int call_timing;             /* FX_CALL_TIMING: whether an analysis call records the three events fx_last_kernel_ms() reads: 1 / 0 = every /
                                    no call; -1 = calls whose launches analyse more than one frame per channel each.  A one-frame call is the live,
                                    latency-critical case (the events cost it 13 of its 27 us back to back: each is a barrier packet between
                                    launches), and so is a call of two hops that runs as two one-frame launches (windows of 1024 points and
                                    more, both analysers, the default family): neither is timed by default.
                                    Calls between fx_profile_begin / fx_profile_end are timed regardless */
    int handover_spin_limit;     /* FX_HANDOVER_SPINS: polls a work unit spends waiting for its predecessor's flux state
                                    before it gives up and the call is reported failed (FX_ERR_HIP); 0 = default (1 << 22) */
    int stream_fill_streaming;   /* FX_STREAM_FILL_STREAMING: fx_stream_push's fill threads write the pinned slot with non-temporal stores
                                    (1, and -1 = default) or with memcpy (0) */
} fx_tuning;
void fx_tuning_defaults(fx_tuning* t);     /* every knob "measured best" */
void fx_tuning_from_env(fx_tuning* t);     /* defaults overridden by the FX_* variables set right now */
fx_status fx_get_tuning(fx_context* ctx, fx_tuning* out);
fx_status fx_set_tuning(fx_context* ctx, const fx_tuning* t);

/* Host-only arithmetic, exposed for testing: how a call of `num_frames` frames per channel is cut into
 * work units for the frame kernel (several workgroups per channel, each analysing a run of consecutive
 * frames and handing the channel's flux state -- previousBinMagnitudes, SpectralCharacteristics.h:203 --
 * to the next through device memory).  Writes the unit lengths to sizes[0..n) and returns n (1 = one
 * workgroup per channel); the lengths are positive and add up to num_frames.  `tuning` may be NULL
 * (defaults).  Pure: reads neither the environment nor a device. */
int fx_plan_units(int window_size, unsigned flags, int waves_per_channel, int num_frames,
                  const fx_tuning* tuning, int* sizes, int cap);

/* Host-only, exposed for testing: which symmetries THIS host's cos / sin give the reference's float twiddle table
 * (juce::FFT's table: phase in double, entries rounded to float; ref SURVEY.md App. A.1) for a window size.
 * bit 0: the mirror symmetry of the 16-point first pass's constants -- the kernels rely on it and fx_create refuses a
 *        host without it (FX_ERR_UNSUPPORTED);
 * bit 1: table[j + N/4] == (table[j].im, -table[j].re) for the entries the 4096-point kernel's compact twiddle image
 *        forms that way -- a host without it gets them read from the whole table instead (slower, same values).
 * Sizes that use neither report the bit as set.  Pure: no device. */
int fx_twiddle_symmetry(int window_size);

/* Kernel-time accounting over a region of calls: fx_profile_begin() starts recording a HIP event
 * triple per analysis call on the context's stream (no synchronisation, at most 4096 calls);
 * fx_profile_end() synchronises and returns the summed device time of the frame kernel and of the
 * smoothing/onset kernels and the number of calls recorded. */
fx_status fx_profile_begin(fx_context* ctx);
fx_status fx_profile_end(fx_context* ctx, double* frame_kernel_ms, double* epilogue_kernel_ms, int* calls);

/* ---- multi-GPU: one process per GPU, channels sharded by contiguous blocks ----
 * Channels are independent (one AnalyserTrackController each, AnalyserTrackController.h:199-210), so
 * the analysis itself needs no exchange.  The only collective on the path is the gather of every
 * rank's latest smoothed vectors to the rank that owns the OSC sink -- the two OSCFeatureAnalysisOutput
 * senders of a track (AnalyserTrackController.h:22-23) sample AudioFeatures::getValue at 60 Hz and
 * send it (OSCFeatureAnalysisOutput.h:89-136).  It runs over RCCL (xGMI between the GPUs of a node).
 *
 *   rank 0:     fx_comm_unique_id(id)  -> hand the FX_COMM_ID_BYTES bytes to every rank (any channel)
 *   every rank: fx_comm_create(ctx, rank, world, id, FX_COMM_ID_BYTES)       (collective)
 *   per step:   fx_gather_smoothed(ctx, dst_rank, out, mem_kind)             (collective, asynchronous)
 *               fx_comm_sync(ctx) before reading `out`
 */
#define FX_COMM_ID_BYTES 128
/* ncclGetUniqueId.  librccl is loaded on first use of an fx_comm_* entry (single-GPU users never map it);
 * FX_ERR_UNSUPPORTED if it cannot be loaded. */
fx_status fx_comm_unique_id(void* id_out, int id_bytes);
/* Join this context to a communicator of `world_size` ranks (ncclCommInitRank on the context's
 * device; every rank calls it with the same id).  Ranks may own different channel counts; the
 * counts are exchanged here.  One communicator per context. */
fx_status fx_comm_create(fx_context* ctx, int rank, int world_size, const void* unique_id, int id_bytes);
fx_status fx_comm_destroy(fx_context* ctx);
/* Channels of all ranks (sum of their num_channels) and the channel offset of `rank`'s block. */
fx_status fx_comm_layout(fx_context* ctx, int* total_channels, int* first_channel_of_rank /*[world_size] or NULL*/);
/* Snapshot this rank's latest smoothed vectors [num_channels][12] (ordered after the analysis
 * calls made so far) and gather all ranks' blocks, in rank order, to `dst_rank`:
 *   out [total_channels][12] floats on dst_rank (FX_MEM_DEVICE or FX_MEM_HOST), ignored elsewhere.
 * The exchange runs on a side stream behind an event, double-buffered, so it overlaps the kernels of
 * the next analysis call; nothing blocks the host.  `out` is valid after fx_comm_sync().  */
fx_status fx_gather_smoothed(fx_context* ctx, int dst_rank, float* out, int mem_kind);
/* Wait for every gather issued so far on this context. */
fx_status fx_comm_sync(fx_context* ctx);
/* What a scaling run wants to see of the exchange: RCCL's own rank count of the communicator (ncclCommCount), the gathers issued, how many
 * of them were timed (HIP events around the send / receive group on the side stream; a gather still running when its staging slot comes
 * round again is not counted), and their summed and longest device time in milliseconds.  Any pointer may be NULL. */
fx_status fx_comm_stats(fx_context* ctx, int* rccl_ranks, int* gathers, int* gathers_timed, double* total_ms, double* max_ms);

/* ---- the reference's LEGACY offline analyser: struct AudioAnalyser (AudioAnalysis.h), SURVEY.md 8(f) rank 4 ----
 * Never instantiated by the reference application (AudioAnalysis.h:221-246 is commented out); provided for hosts that
 * want its features.  An fx_offline stands for `num_channels` AudioAnalyser objects (one per channel: the histogram-F0
 * estimate keeps `previousF0`, AudioAnalysis.h:109,273-293,697) on one GPU.  Buffers are [num_channels][...] row-major,
 * FX_MEM_HOST (copied synchronously) or FX_MEM_DEVICE (asynchronous on the object's stream; fx_offline_sync waits). */
typedef struct fx_offline fx_offline;
/* AudioAnalyser (windowSize, numChannels, nyquistFrequency, ...), AudioAnalysis.h:107-125 */
fx_status fx_offline_create(fx_offline** out, int device_id, int num_channels, double nyquist);
fx_status fx_offline_destroy(fx_offline* o);
fx_status fx_offline_reset(fx_offline* o);                         /* previousF0 := 0, as constructed (AudioAnalysis.h:109) */
fx_status fx_offline_sync(fx_offline* o);
fx_status fx_offline_get_previous_f0(fx_offline* o, double* out /*[num_channels]*/);
/* AudioAnalyser::analyseNormalisedZeroCrosses, AudioAnalysis.h:517-541: audio [C][num_samples] ->
 * out [C][num_downsamples] (the ZeroCrosses feature row, AudioAnalysis.h:538) */
fx_status fx_offline_zero_crosses(fx_offline* o, const float* audio, int num_samples, int num_downsamples, float* out, int mem_kind);
/* AudioAnalyser::setLogAttackTime, AudioAnalysis.h:611-622: envelope [n] (channel 0 of the energy envelope), the length of the
 * analysed audio, its number of downsamples and the (integer, AudioFeatures.h:303) sample rate -> estimatedLogAttackTime */
fx_status fx_offline_log_attack_time(fx_offline* o, const float* envelope, int n, int num_input_samples, int num_downsamples,
                                     int sample_rate, float* out, int mem_kind);
/* AudioAnalyser::calculateFFTLBP, AudioAnalysis.h:543-564 (which only prints): cur, prev [C][num_bins] magnitude frames ->
 * bits [C][num_bins] (|cur - prev| > 0.1f), highest_ratio [C] (last bin over the threshold / num_bins), activity_ratio [C] */
fx_status fx_offline_fft_lbp(fx_offline* o, const float* cur, const float* prev, int num_bins, unsigned char* bits,
                             float* highest_ratio, float* activity_ratio, int mem_kind);
/* AudioAnalyser::calculateHarmonicCharacteristics, AudioAnalysis.h:253-303 (peaks :350-393, frequency histogram :395-417,
 * estimateF0AndHERFromFrequencyHistogram :419-441, the octave rule :273-291, calculateInharmonicity :305-336):
 * magnitudes [C][num_bins] of one frame -> out3 [C][3] = f0, harmonicEnergyRatio, inharmonicity; 4 <= num_bins <= 4097 */
fx_status fx_offline_harmonic_characteristics(fx_offline* o, const float* magnitudes, int num_bins, float* out3, int mem_kind);
/* AudioAnalyser::calculateSpectralCharacteristics, AudioAnalysis.h:463-515 (the legacy full-spectrum form): magnitudes [C][num_bins] of one
 * frame -> out4 [C][4] = centroid / nyquist, spread, flatness, flux (AudioAnalysis.h:17-29).  Each channel's previousBinMagnitudes
 * (:120-121, :510, :700) is kept across calls and replaced only by frames that pass the 0.001 gate (:498-500); its length is fixed by
 * the first call (an analyser's window size) until fx_offline_reset.  1 <= num_bins <= 4097 */
fx_status fx_offline_spectral_characteristics(fx_offline* o, const float* magnitudes, int num_bins, float* out4, int mem_kind);
fx_status fx_offline_get_previous_bins(fx_offline* o, double* out /*[num_channels][num_bins]*/, int num_bins);
/* AudioAnalyser::calculateNormalisedSpectralSlope, AudioAnalysis.h:566-609: magnitudes [C][num_bins] -> out [C] */
fx_status fx_offline_spectral_slope(fx_offline* o, const float* magnitudes, int num_bins, float* out, int mem_kind);
/* AudioAnalyser::getConjugateComplexMultiplicationInPlace + analyseAutoCorrelation (+ getMaxIndex), AudioAnalysis.h:623-665:
 * data [C][num_items][2] interleaved (r, i) is replaced IN PLACE by each item times its conjugate; peak_bin [C] = the first item holding
 * the largest real part of the products, frequency [C] (doubles) = the estimate the reference prints for it,
 * peak_bin * (nyquist / num_items) + half a bin */
fx_status fx_offline_auto_correlation(fx_offline* o, float* data, int num_items, int* peak_bin, double* frequency, int mem_kind);

/* ---- the offline driver: AudioAnalyser::performSpectralAnalysis (AudioAnalysis.h:129-251) into a ConcatenatedFeatureBuffer
 * (AudioFeatures.h:14-314): audio in, the reference's feature buffer out ----
 * What the reference pins (live code, held to the unmodified header by tests/golden/offline/feature_buffer.npz): the frame indexing and
 * padding (:146-181, observable in the public member fftIn), scaleBufferWithBartlettWindowing (:667-676), analyseNormalisedZeroCrosses,
 * setLogAttackTime, ConcatenatedFeatureBuffer::fillDownsampledRMSAudioChannels / normaliseAudioChannels and the buffer's layout
 * (AudioFeatures.h:124-195).  What is OURS, specified here: AudioAnalysis.h:219-246 is commented out, so the reference never fills fftOut and
 * its energyEnvelope sums uninitialised memory; this driver does what that block states, its calls in its order.  JUCE's
 * performFrequencyOnlyForwardTransform is not in the reference tree; its arithmetic is taken as tools/refdiff/juce_standin.h states it (the
 * forward transform, then sqrt (re * re + im * im) in float).
 *
 * An fx_offline stands for C = num_channels independent MONO analysers: where the reference sums (sumAccrossChannels, :705-716) or
 * normalises (AudioFeatures.h:186-195) across the channels of one file, this is done per channel.
 * audio [C][S] fp32; S = num_samples, D = num_downsamples, N = window_size in {256, 512, 1024, 2048, 4096}, B = N / 2 + 1.  mem_kind covers
 * every buffer of a call: FX_MEM_HOST buffers are copied synchronously, FX_MEM_DEVICE buffers are 4-byte aligned and used asynchronously on
 * the object's stream (fx_offline_sync waits).
 *
 * Frames (:146-181).  step = S div D.  If D == 1: win[j] = audio[j], 0 <= j < N.  Otherwise, for frame f: i = f * step + j - N / 2 and
 * win[j] = audio[i] if 0 <= i < S, else +0.  Then x[j] = win[j] * w[j] with w[j] = 2j / N for j < N / 2 and 2 - 2j / N for j >= N / 2 (what
 * the two applyGainRamp calls accumulate; exact in float).  The product is always formed: an inf under w[0] = 0 becomes NaN.
 * Magnitudes.  X = the forward transform of x by the reference FFT's butterfly DAG (radix 4 while it divides, then one radix 2; decimation in
 * time; table twiddles, phase in double rounded to float; plain fp32, nothing fused) -- the DAG of every transform in this library.  For
 * 0 <= b <= N / 2: m[b] = sqrt (fl32 (fl32 (re * re) + fl32 (im * im))), the square root correctly rounded.  Frame f of channel c lies at
 * magnitudes[(f * C + c) * B + b]: frame-major, so that every frame is the [C][B] block the per-frame entries above take.
 * Energy (:249, :705-716 for one channel).  e = +0; for b ascending e = fl32 (e + m[b]); stored at energy[c * D + f]. */
enum { FX_OFFLINE_CENTROID = 0, FX_OFFLINE_SLOPE, FX_OFFLINE_SPREAD, FX_OFFLINE_FLATNESS, FX_OFFLINE_FLUX, FX_OFFLINE_ZERO_CROSSES,
       FX_OFFLINE_F0, FX_OFFLINE_HER, FX_OFFLINE_INHARMONICITY, FX_OFFLINE_AUDIO, FX_OFFLINE_FEATURE_ROWS };   /* AudioFeatures.h:20-31, less FFT */
enum { FX_OFFLINE_DO_SPECTRAL = 1, FX_OFFLINE_DO_HARMONIC = 2, FX_OFFLINE_DO_ZERO_CROSSES = 4, FX_OFFLINE_DO_AUDIO = 8,
       FX_OFFLINE_DO_NORMALISE_AUDIO = 16, FX_OFFLINE_DO_LOG_ATTACK = 32 };
#define FX_OFFLINE_SCRATCH_BYTES (16u << 20)
/* The frame / window / magnitude stage alone.  Refused (FX_ERR_INVALID_ARGUMENT, fx_last_error names the value; nothing launched): a null
 * o, audio or magnitudes; S < 1; D < 1; D > S (step 0, the reference's jassert); N outside the set; D == 1 with N > S (:157); an unknown
 * mem_kind. */
fx_status fx_offline_frames(fx_offline* o, const float* audio, int num_samples, int num_downsamples, int window_size,
                            float* magnitudes /* [D][C][N/2+1] */, float* energy /* [C][D] or NULL */, int mem_kind);
/* The whole analysis; bit-identical to calling the pieces.  For f ascending, on frame f's [C][B] block: (1) fx_offline_spectral_characteristics,
 * out4 -> rows CENTROID, SPREAD, FLATNESS, FLUX at index f; (2) fx_offline_spectral_slope -> row SLOPE; (3) fx_offline_harmonic_characteristics,
 * out3 -> rows F0, HER, INHARMONICITY (the order of :229-246); (1)-(2) under DO_SPECTRAL, (3) under DO_HARMONIC.  The object's state
 * (previousBinMagnitudes, previousF0) enters the call as it stands and leaves as the last frame left it.  Then, independent of the loop:
 *   DO_ZERO_CROSSES     fx_offline_zero_crosses into row ZERO_CROSSES.
 *   DO_AUDIO            fillDownsampledRMSAudioChannels (AudioFeatures.h:158-184), spb = S div D.  If spb == 1: row[i] = audio[i], i < D.
 *                       Otherwise row[i] = fl32 (sqrt_f64 (sum / fl64 (spb))), sum = +0.0 (fp64) and, for s ascending over the step,
 *                       sum += fl64 (fl32 (a * a)); the sum is serial.
 *   DO_NORMALISE_AUDIO  (needs DO_AUDIO) AudioFeatures.h:186-195 with the stand-in's findMinMax: lo = hi = row[0]; for i >= 1: if
 *                       row[i] < lo then lo = row[i]; if row[i] > hi then hi = row[i]; m = jmax (|lo|, |hi|) with jmax (a, b) = a < b ? b : a;
 *                       row[i] = row[i] * (1.0f / m).  Exactly these comparisons: they fix what a NaN does; an all-zero row becomes NaN.
 *   DO_LOG_ATTACK       setLogAttackTime (:611-622) of each channel's energy row into log_attack_time[c].
 * features[(r * C + c) * D + i] is the reference's arrayStartIndex with numFeatureChannels = C; rows not asked for are +0.
 * With magnitudes != NULL the whole [D][C][B] goes to the caller; with NULL the call works through a scratch the object owns, in chunks of
 * F = max (1, FX_OFFLINE_SCRATCH_BYTES div (4 * C * B)) frames: the same bits either way.
 * Refused before any launch or state change, besides fx_offline_frames' list (features takes the place of magnitudes): DO_NORMALISE_AUDIO
 * without DO_AUDIO; DO_LOG_ATTACK with a null log_attack_time or sample_rate < 1000 (fx_offline_log_attack_time's rule); DO_SPECTRAL while
 * the object's previousBinMagnitudes holds another number of bins (fx_offline_spectral_characteristics' rule). */
fx_status fx_offline_analyse(fx_offline* o, const float* audio, int num_samples, int num_downsamples, int window_size, int sample_rate,
                             unsigned what, float* features /* [10][C][D] */, float* energy /* [C][D] or NULL */,
                             float* log_attack_time /* [C] or NULL */, float* magnitudes /* [D][C][N/2+1] or NULL */, int mem_kind);

/* A LIBRARY of files in one call: C = num_channels files of DIFFERENT lengths (and sample rates), as the reference gives every file its own
 * ConcatenatedFeatureBuffer with its own number of samples, step and rate.  samples is a bank exactly as fx_create_clips takes it: the files
 * back to back, file c being S_c = lengths[c] samples of sample_format (FX_SAMPLE_F32 / F16 / S16 / packed S24) starting at sample index
 * sum (lengths[0 .. c)), formed in 64 bits.  mem_kind covers samples and the results; a host bank is staged in its wire format and widened by
 * the kernels.  A device bank starts at a 4-byte boundary; the files inside it start wherever they fall (any 2-byte boundary for the 16-bit
 * formats, any byte for S24), and no load touches a byte outside the bank.  lengths and sample_rates are host memory, read before the call
 * returns; sample_rates is needed only with DO_LOG_ATTACK.
 * With a_c[i] the widening (csrc/fx_samples.hip.h: the one statement of it) of sample i of file c, every output of channel c is what
 * fx_offline_analyse specifies for that channel with S_c in place of S wherever S occurs -- the frame indexing and zero padding, step, the
 * D == 1 form, spb of the Audio row, the zero crossings, num_input_samples of the log attack time -- and sample_rates[c] in place of
 * sample_rate.  The same as there: the frame order, the state carried in and out, the chunking through the object's scratch, "rows not asked
 * for are +0", the output layouts ([10][C][D], [C][D], [C], [D][C][B]: one num_downsamples for every file).  what == 0 with magnitudes != NULL
 * is the frame stage alone.  Each analyser's nyquist is the object's (fx_offline_set_nyquists below): a library with files at different rates
 * sets them and passes sample_rates; nothing is resampled.
 * Refused (FX_ERR_INVALID_ARGUMENT; fx_last_error names the value and, where there is one, the file; before any launch, copy or state
 * change): what fx_offline_analyse refuses that still applies; a null lengths; lengths[c] < 1 or > 2^31 - 1; num_downsamples > S_c for some c
 * (that file's step would be 0); num_downsamples == 1 with window_size > S_c; an unknown sample_format; a device bank off a 4-byte boundary;
 * DO_LOG_ATTACK with null sample_rates or a rate below 1000.
 * Not tested on a device: a bank of more than 2^31 samples (the offsets are 64-bit throughout; a bank that large is not analysed in the
 * seconds a test has) -- as for the clips' 64-bit sample counter above. */
fx_status fx_offline_analyse_files(fx_offline* o, const void* samples, const long long* lengths /* [C], host */, int sample_format,
                                   int num_downsamples, int window_size, const int* sample_rates /* [C], host, or NULL */, unsigned what,
                                   float* features /* [10][C][D] */, float* energy /* [C][D] or NULL */, float* log_attack_time /* [C] or NULL */,
                                   float* magnitudes /* [D][C][N/2+1] or NULL */, int mem_kind);
/* Each channel's analyser has a nyquistFrequency of its own (AudioAnalysis.h:107): files of one library come at 44.1 and 48 kHz.  The setter
 * takes [C] host values, refuses per entry what fx_offline_create refuses for its one value (naming the channel, changing nothing), and
 * takes effect in stream order: fx_offline_spectral_characteristics, fx_offline_harmonic_characteristics, fx_offline_auto_correlation and
 * the two whole-analysis entries read the channel's value from then on.  previousF0 and previousBinMagnitudes are left alone.  An object
 * never set reads the creation value in every channel, which is what the getter returns until the first set. */
fx_status fx_offline_set_nyquists(fx_offline* o, const double* nyquist /* [C], host */);
fx_status fx_offline_get_nyquists(fx_offline* o, double* out /* [C], host */);

/* ---- what the reference derives from a feature buffer: ranges, discrete distributions, smoothed features (AudioFeatures.h:208-240,
 * :356-421) ----
 * rows is [R][C][D] fp32, any R = num_rows rows of a feature buffer: rows[(r * C + c) * D + i] is the reference's arrayStartIndex with
 * numFeatureChannels = C (fx_offline_analyse's features with R = FX_OFFLINE_FEATURE_ROWS is the whole buffer).  As everywhere in the
 * driver a channel is a mono file: what the reference takes over numDownsamples * numFeatureChannels samples is taken per channel.
 * FX_MEM_HOST buffers are copied synchronously, FX_MEM_DEVICE buffers are 4-byte aligned and used asynchronously on the object's stream
 * (fx_offline_sync waits).  Every entry refuses (FX_ERR_INVALID_ARGUMENT, fx_last_error names the value; nothing launched, no state
 * changed): a null argument, num_rows < 1, num_downsamples < 1, num_rows * C > 2^31 - 1, an unknown mem_kind, and what it lists itself. */
/* getFeatureRange (AudioFeatures.h:208-213) of every row and channel, with the stand-in's findMinMax (the chain DO_NORMALISE_AUDIO states):
 * lo = hi = row[0]; for i >= 1 ascending: if row[i] < lo then lo = row[i]; if row[i] > hi then hi = row[i].  out[(r * C + c) * 2] = lo,
 * [.. + 1] = hi.  Exactly these comparisons: a NaN at row[0] is both ends for ever; a NaN elsewhere is stepped over; among values that
 * compare equal the FIRST occurrence wins, which decides the sign of a zero extreme (+0, -0 gives lo = +0; -0, +0 gives lo = -0). */
fx_status fx_offline_feature_ranges(fx_offline* o, const float* rows, int num_rows, int num_downsamples, float* out /* [R][C][2] */, int mem_kind);
/* getDiscreteFeatureDistribution (AudioFeatures.h:215-240) of every (row, channel): sorted = the row's D values ascending; step = D div
 * num_brackets; for bracket b: av = +0.0f; for s from b * step to (b + 1) * step - 1 ascending av = fl32 (av + sorted[s]);
 * out[(r * C + c) * num_brackets + b] = fl32 (av / fl32 (step)).  The sum is serial fp32 in sorted order; the D - num_brackets * step largest
 * values are not used; step == 0 (num_brackets > D) is 0.0f / 0.0f: every bracket NaN, as in the reference.
 * Where the reference is undefined, OURS: the order is by value (-0 and +0 in either order: from av = +0.0f it cannot change a sum); every
 * NaN sorts after +inf (std::sort on a NaN is undefined); subnormals are ordered as the numbers they are, never flushed (the sort key is
 * the float's bits: b ^ 0x80000000 for b >= 0, ~b for b < 0, 0xFFFFFFFF for a NaN).
 * A row of up to FX_OFFLINE_SORT_CHUNK values is sorted by one workgroup wholly in LDS, which then walks the brackets, a lane each.  8192
 * keys = 32 KiB at the most (five workgroups in a CU's 160 KiB, where 16384 keys would leave two), and the allocation is the row's power
 * of two: the common D of a few thousand takes 16 KiB or less, so the CU's 32 waves, not its LDS, bound it at eight workgroups.  Longer rows are padded to a power of two P in the object's scratch,
 * max (1, FX_OFFLINE_SCRATCH_BYTES div (4 * P)) rows at a time: chunks sorted in LDS, bitonic steps of stride >= chunk in global memory, the
 * rest of each merge in LDS again.  The same bits whichever path and however the rows are grouped.
 * Refused as well: num_brackets < 1; num_downsamples > FX_OFFLINE_SCRATCH_BYTES / 4 (one padded row exceeds the scratch). */
#define FX_OFFLINE_SORT_CHUNK 8192
fx_status fx_offline_feature_distribution(fx_offline* o, const float* rows, int num_rows, int num_downsamples, int num_brackets,
                                          float* out /* [R][C][num_brackets] */, int mem_kind);
/* SmoothedFeatures (AudioFeatures.h:356-421), one per channel, its state on the device.  depth in [1, 64] constructs every channel's
 * smoother anew (:358-369): currentFeatureValues[9] = 0, featureHistory[9][depth] = 0; depth 0 frees it; anything else is refused (the
 * reference's historyLength - 1 on a size_t makes 0 a crash there).  Another object than the analyser in the reference: fx_offline_reset
 * does not touch it.  Synchronises the object's stream. */
fx_status fx_offline_smoothing(fx_offline* o, int depth);
/* updateValues (AudioFeatures.h:371-379) for i = first .. first + count - 1 ascending, on the buffer whose sample 0 is column i of rows
 * (R >= 9 rows, CENTROID .. INHARMONICITY leading; new = rows[(f * C + c) * D + i]).  updateHistory (:399-409): history[k] = history[k + 1]
 * for k < depth - 1, history[depth - 1] = current.  Then for features f = 0 .. 8 (:387-394, :411-420): av = +0.0f; av = fl32 (av + history[k])
 * for k ascending; av = fl32 (av / fl32 (fl32 (depth) + 1)) (:418, (float) historyLength + 1); current = fl32 (av + fl32 (fl32 (new - av) *
 * 0.5f)) (JUCE_LIVE_CONSTANT (0.5f); nothing fused).  out[(f * C + c) * count + (i - first)] = current after update i; out may be NULL.
 * first = 0, count = 1 is the reference's call; count = D smooths whole rows in one launch.  The state carries from call to call.
 * Refused as well: no smoother constructed; first < 0; count < 1; first + count > D. */
fx_status fx_offline_smooth_rows(fx_offline* o, const float* rows, int num_downsamples, int first, int count,
                                 float* out /* [9][C][count] or NULL */, int mem_kind);
/* The smoothers' state (AudioFeatures.h:382-383) on the host, after everything enqueued so far: currentFeatureValues and featureHistory
 * (oldest entry first); either may be NULL.  FX_ERR_INVALID_ARGUMENT without a smoother. */
fx_status fx_offline_get_smoothing(fx_offline* o, float* current /* [9][C] */, float* history /* [9][C][depth] */);

/* ---- OSC sink helpers (host side, no GPU) ---- */
/* Re-order one 12-slot vector into the wire order of
 * sender.send(bundleAddress, onset, rms, f0, centroid, slope, spread, flatness,
 * ler, flux, her, oer, inharm)  -- OSCFeatureAnalysisOutput.h:107 */
void fx_pack_osc12(const float* features12, float* out12);
/* README.md:57 order: onset, rms, f0, centroid, slope, spread, flatness, flux, her, inharm */
void fx_pack_osc10(const float* features12, float* out10);
/* Encode the OSC 1.0 message OSCSender::send(address, 12 floats) emits.
 * Returns the byte count (76 for "/Audio/A0") or -1 if cap is too small. */
int fx_osc_encode(const char* address, const float* features12, unsigned char* out, int cap);


/* ---- the sink at scale: every track's message in one call, every tick's datagrams in a few system calls ----
 * The reference sends one message per track per 60 Hz tick (OSCFeatureAnalysisOutput.h:84-113,133), from two senders per track
 * (AnalyserTrackController.h:22-23), addressed "/Audio/A<row>" (MainComponent.cpp:170).  At configs[3] that is 65 536 x 60 = 3.9e6
 * datagrams a second: they are formatted in bulk (on the GPU, straight from the context's latest vectors, so that the copy to the host
 * is already the datagrams) and handed to the kernel in batches (sendmmsg), by a few threads, paced at 60 Hz. */
/* Bytes of the message for address "<prefix><channel>" (76 for "/Audio/A", 0): address + NUL padded to 4, 16 bytes of type tags,
 * 48 of floats.  -1 if prefix is NULL, longer than 64 bytes, or channel < 0. */
int fx_osc_message_bytes(const char* prefix, int channel);
/* fx_osc_encode for num_channels tracks at once, on the host: message c = "<prefix><first_channel + c>" with smoothed[c][12]
 * (AudioFeatures slot order) is written at out + c * stride and its length to lengths[c] (lengths may be NULL); the rest of each
 * slot is zeroed.  stride: a multiple of 4, >= fx_osc_message_bytes(prefix, first_channel + num_channels - 1).
 * Returns num_channels, or -1 on a bad argument. */
int fx_osc_encode_batch(const char* prefix, int first_channel, int num_channels, const float* smoothed12,
                        unsigned char* out, int stride, int* lengths);
/* The same bytes for every channel of the context, formed ON THE DEVICE from the latest AudioFeatures::getValue vectors (what
 * fx_get_smoothed returns), ordered after the analysis calls made so far.  out: [num_channels][stride] bytes, FX_MEM_HOST (the call
 * returns when they are there) or FX_MEM_DEVICE (4-byte aligned; asynchronous on the context's stream -- pinned host memory mapped
 * into the device works the same way); lengths: host array [num_channels] or NULL. */
fx_status fx_get_osc_datagrams(fx_context* ctx, const char* prefix, int first_channel, unsigned char* out, int stride,
                               int* lengths, int mem_kind);

/* ---- per-track addresses: every track's own bundleAddress ----
 * The reference builds each track with (ip, secondaryIP, bundle) (AnalyserTrackController.h:17,22-23) and the GUI edits the three per
 * track (:140-147); both of a track's senders send `bundleAddress` (OSCFeatureAnalysisOutput.h:107) to their own host (:115-136).
 * The address is this table; the two hosts are the sender's routes (fx_osc_sender_set_routes below). */
#define FX_OSC_ADDRESS_MAX 124   /* bytes of an address: padded it is at most 128 bytes, a message at most 192 */
/* Every track's address (ref AnalyserTrackController.h:17,146 setBundleAddressChangedCallback): addresses [num_channels] C strings in
 * host memory, copied (the caller may free them on return), or NULL to drop the table.  An address has 1 .. FX_OSC_ADDRESS_MAX bytes,
 * starts with '/', every byte in 0x21 .. 0x7E; a bad one fails the whole call with FX_ERR_INVALID_ARGUMENT before any device use
 * (fx_last_error names the track) and nothing changes; a failed allocation or upload leaves the old table in force.  A setting:
 * fx_reset_state and fx_reset_channels keep it.  Synchronises the context's stream, as the other per-track setters do. */
fx_status fx_set_osc_addresses(fx_context* ctx, const char* const* addresses);
/* The smallest legal stride of fx_get_osc_datagrams_addressed: the longest message (OSCFeatureAnalysisOutput.h:107) of the table;
 * -1 without a table. */
int fx_osc_address_stride(fx_context* ctx);
/* fx_get_osc_datagrams with the table's addresses (ref OSCFeatureAnalysisOutput.h:107): message c, at out + c * stride, is byte for
 * byte fx_osc_encode(address[c], latest[c]) and the rest of its slot zeros; lengths (host, or NULL) come from the table.  Ordering,
 * FX_MEM_HOST / FX_MEM_DEVICE and the 4-byte alignment of a device buffer as fx_get_osc_datagrams; stride: a multiple of 4,
 * >= fx_osc_address_stride.  FX_ERR_INVALID_ARGUMENT without a table. */
fx_status fx_get_osc_datagrams_addressed(fx_context* ctx, unsigned char* out, int stride, int* lengths, int mem_kind);
/* The same bytes formed on the host (no GPU) for n tracks: addresses [n] under the rules above, smoothed12 [n][12] in AudioFeatures
 * slot order (ref OSCFeatureAnalysisOutput.h:107).  Returns n, or -1 on a bad argument (fx_last_error names a bad address's track). */
int fx_osc_encode_addressed(const char* const* addresses, int n, const float* smoothed12, unsigned char* out, int stride, int* lengths);

/* ---- bundles: many tracks' messages per datagram ----
 * One message per track per tick (OSCFeatureAnalysisOutput.h:107) is one datagram, one trip through the network stack and one receiver
 * wake-up per track; OSC 1.0 has the #bundle for that.  A bundle datagram here is "#bundle\0" (8 bytes), a 64-bit big-endian NTP time
 * tag, then per element a big-endian int32 size and that many bytes (OSC 1.0, "OSC Bundles"); every element is byte for byte the message
 * fx_osc_encode makes for its track (OSCFeatureAnalysisOutput.h:107).  Bundle b of a call holds tracks [b * K, min(n, (b + 1) * K)) in
 * ascending order, K the same for every bundle of the call (so which tracks share a datagram depends on K alone and the sender's
 * per-datagram routes keep their meaning); the last bundle may be short; bundles are never nested.  Opt-in: the entries above keep their
 * bytes and their launches. */
#define FX_OSC_BUNDLE_MAX_ELEMENTS 1024
#define FX_OSC_TIMETAG_IMMEDIATE 1ull   /* OSC 1.0: "immediately" */
/* The layout of a call's bundles (host arithmetic): K = min(num_tracks, FX_OSC_BUNDLE_MAX_ELEMENTS, (max_datagram_bytes - 16) /
 * (4 + longest_message_bytes)) tracks per bundle (OSCFeatureAnalysisOutput.h:107 messages as the elements of an OSC 1.0 bundle),
 * num_bundles = ceil(num_tracks / K), stride = 16 + K * (4 + longest) bytes per output slot.  longest_message_bytes: from
 * fx_osc_message_bytes(prefix, first + n - 1) or fx_osc_address_stride (a multiple of 4, 68 .. 192).  FX_ERR_INVALID_ARGUMENT when K would
 * be 0, max_datagram_bytes > 65507 or num_tracks < 1.  Any output pointer may be NULL. */
fx_status fx_osc_bundle_plan(int longest_message_bytes, int num_tracks, int max_datagram_bytes, int* tracks_per_bundle, int* num_bundles, int* stride);
/* The OSC 1.0 bundle time tag of a Unix time: NTP seconds since 1900 in the high word, the fraction of a second in the low word
 * (what marks the OSCFeatureAnalysisOutput.h:107 messages of many tracks as one analysis instant). */
unsigned long long fx_osc_timetag(double unix_seconds);
/* fx_osc_encode_batch as bundles, on the host: tracks "<prefix><first_channel + c>" with smoothed12 [n][12] (OSCFeatureAnalysisOutput.h:107
 * messages in OSC 1.0 bundles, laid out by fx_osc_bundle_plan for the longest of these messages); bundle b at out + b * stride,
 * lengths[b] (may be NULL) its bytes, the rest of each slot zeros.  stride: a multiple of 4, >= the plan's.  Returns the number of
 * bundles, or -1 on a bad argument. */
int fx_osc_encode_bundles(const char* prefix, int first_channel, int n, const float* smoothed12, unsigned long long timetag,
                          int max_datagram_bytes, unsigned char* out, int stride, int* lengths);
/* fx_osc_encode_addressed as bundles (OSCFeatureAnalysisOutput.h:107 messages with the tracks' own addresses in OSC 1.0 bundles); the
 * plan is made for the longest message of `addresses`. */
int fx_osc_encode_bundles_addressed(const char* const* addresses, int n, const float* smoothed12, unsigned long long timetag,
                                    int max_datagram_bytes, unsigned char* out, int stride, int* lengths);
/* The same bundles for every channel of the context, formed ON THE DEVICE from `latest` in one launch (OSCFeatureAnalysisOutput.h:107
 * messages, OSC 1.0 bundle layout), ordered after the analysis calls made so far.  out: [num_bundles][stride] bytes as
 * fx_osc_bundle_plan(fx_osc_message_bytes(prefix, first_channel + num_channels - 1), num_channels, max_datagram_bytes) lays them out;
 * stride: a multiple of 4, >= the plan's; not one byte past num_bundles * stride is written.  FX_MEM_HOST returns when the bytes are
 * there; FX_MEM_DEVICE needs a 4-byte-aligned buffer and is asynchronous on the context's stream.  lengths: host array [num_bundles] or
 * NULL.  Nothing is kept between calls: timetag, max_datagram_bytes and the prefix may change from call to call at no cost.  Bad
 * arguments are refused before any device use. */
fx_status fx_get_osc_bundles(fx_context* ctx, const char* prefix, int first_channel, unsigned long long timetag, int max_datagram_bytes,
                             unsigned char* out, int stride, int* lengths, int mem_kind);
/* fx_get_osc_bundles with the addresses of fx_set_osc_addresses (OSCFeatureAnalysisOutput.h:107 bundleAddress per track, OSC 1.0
 * bundle layout): the plan is made for fx_osc_address_stride.  FX_ERR_INVALID_ARGUMENT without a table. */
fx_status fx_get_osc_bundles_addressed(fx_context* ctx, unsigned long long timetag, int max_datagram_bytes, unsigned char* out, int stride,
                                       int* lengths, int mem_kind);

/* The sender: one UDP socket per target and thread, sendmmsg in chunks, `threads` sender threads each owning a slice of the tracks,
 * a 60 Hz timer (OSCFeatureAnalysisOutput::startTimerHz (60), :133) and a primary plus an optional secondary target
 * (AnalyserTrackController.h:22-23); targets are "ip[:port]", port 9000 by default, parsed as connectToAddress does (:115-123).
 * No GPU involved.  Like the reference's timer, a tick sends whatever was published last: a vector may go out twice, or never. */
typedef struct fx_osc_sender fx_osc_sender;
#define FX_OSC_SENDER_GSO 1u   /* runs of equal-length messages go to the kernel as ONE segmented send (UDP_SEGMENT) where the host's
                                  kernel supports it; the datagrams on the wire are the same */
fx_status fx_osc_sender_create(fx_osc_sender** out, const char* primary, const char* secondary /* or NULL */, int threads, unsigned flags);
fx_status fx_osc_sender_destroy(fx_osc_sender* s);
/* Publish the datagrams the next ticks send: `count` messages, message i at datagrams + i * stride, lengths[i] bytes.  Copied.
 * A "message" is whatever one datagram carries, up to 65507 bytes: a bundle of fx_get_osc_bundles is published as it is, count =
 * num_bundles. */
fx_status fx_osc_sender_update(fx_osc_sender* s, const unsigned char* datagrams, int stride, const int* lengths, int count);
/* One tick, now, on the caller's thread + the sender's threads: every published message to every target; *sent (may be NULL) =
 * datagrams the kernel accepted. */
fx_status fx_osc_sender_send(fx_osc_sender* s, long long* sent);
/* startTimerHz / stopTimer */
fx_status fx_osc_sender_start(fx_osc_sender* s, double rate_hz);
fx_status fx_osc_sender_stop(fx_osc_sender* s);
typedef struct fx_osc_sender_stats {
    long long ticks;            /* timer ticks and fx_osc_sender_send calls so far */
    long long late_ticks;       /* timer ticks that began after the next one was due (the sender does not keep up with the rate) */
    long long datagrams;        /* accepted by the kernel */
    long long dropped;          /* refused by the kernel (full socket buffer: EAGAIN / ENOBUFS) or failed */
    long long syscalls;         /* sendmmsg / sendmsg calls */
    double    last_tick_ms, max_tick_ms, total_tick_ms;   /* time to hand a tick's datagrams to the kernel */
} fx_osc_sender_stats;
fx_status fx_osc_sender_get_stats(fx_osc_sender* s, fx_osc_sender_stats* out);
/* Per-track targets (ref AnalyserTrackController.h:17,22-23: each track's ip and secondaryIP; :140-145 the GUI's address callbacks;
 * OSCFeatureAnalysisOutput.h:115-136 connectToAddress): targets [num_targets <= FX_OSC_SENDER_MAX_TARGETS] "ip[:port]" strings parsed
 * as at create; message i of a publication goes to targets[primary[i]] and, where secondary is not NULL and secondary[i] >= 0, to
 * targets[secondary[i]] as well; `count` = the messages of a publication.  targets == NULL restores the create-time pair.  Each
 * sender thread keeps one connected socket per target it serves and orders its slice's messages by target HERE, not per tick; per
 * target the messages keep ascending track order.  While routes are set, a publication (fx_osc_sender_update) of another count is
 * FX_ERR_INVALID_ARGUMENT, and so are routes of another count than what is published.  Bad indices or unparsable targets change
 * nothing.  Safe while the timer runs.  Where bundles are published the routes are per bundle: bundle b holds tracks [b * K, (b + 1) * K). */
#define FX_OSC_SENDER_MAX_TARGETS 64
fx_status fx_osc_sender_set_routes(fx_osc_sender* s, const char* const* targets, int num_targets, const int* primary,
                                   const int* secondary /* or NULL */, int count);

/* A counting receiver for tests, benchmarks and soak runs of the sender (loopback diagnostics, not part of the analysis path):
 * `threads` sockets bound to bind_address ("127.0.0.1:0" = any free port) with SO_REUSEPORT, drained by recvmmsg.  With
 * keep_channels > 0 and a prefix it also keeps the newest message of every address "<prefix><n>", n < keep_channels. */
typedef struct fx_osc_receiver fx_osc_receiver;
#define FX_OSC_RECEIVER_NO_GRO 1u   /* do not ask for UDP_GRO: every datagram makes its own way through the receiving stack, as it would from a
                                       remote sender (with it, a segmented send over loopback arrives whole and is split in user space) */
#define FX_OSC_RECEIVER_BUNDLES 2u  /* 65 536 bytes of room per datagram, and a datagram that starts with "#bundle\0" is parsed (OSC 1.0 bundle
                                       layout): each element is taken as a message of its own (OSCFeatureAnalysisOutput.h:107), so that
                                       fx_osc_receiver_last keeps working.  A bundle counts once as malformed when a size is no multiple of 4
                                       or runs past the end, when it is nested or empty, or when an element is no twelve-float message. */
fx_status fx_osc_receiver_create(fx_osc_receiver** out, const char* bind_address, int threads, const char* prefix, int keep_channels, unsigned flags);
fx_status fx_osc_receiver_destroy(fx_osc_receiver* r);
int fx_osc_receiver_port(fx_osc_receiver* r);
/* datagrams and bytes received so far, and those that were not an OSC message of twelve floats; any pointer may be NULL */
fx_status fx_osc_receiver_get_stats(fx_osc_receiver* r, long long* datagrams, long long* bytes, long long* malformed);
/* FX_OSC_RECEIVER_BUNDLES: well-formed bundles (OSC 1.0) received so far, the messages (OSCFeatureAnalysisOutput.h:107) they held and
 * the time tag of the newest one; any pointer may be NULL.  All 0 without the flag. */
fx_status fx_osc_receiver_get_bundle_stats(fx_osc_receiver* r, long long* bundles, long long* elements, unsigned long long* last_timetag);
/* newest message kept for `channel`: copied to out (cap bytes), its length to *len (0 = none seen yet) */
fx_status fx_osc_receiver_last(fx_osc_receiver* r, int channel, unsigned char* out, int cap, int* len);

const char* fx_last_error(void);
int fx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FX_H */
