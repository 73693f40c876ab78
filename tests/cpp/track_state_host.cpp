// track_state_host.cpp -- the host side of moving tracks between contexts (fx_track_state_bytes / fx_export_channels /
// fx_import_channels, csrc/fx_track_state.hip) against tests/cpp/fake_hip/, under ASan + UBSan (tests/test_track_state_cpu.py builds and
// runs it; fx_track_state.hip is compiled as C++, its kernels left out, and the launchers below stand in for them: the pack and the
// unpack on the host, written from the same track_piece() the kernels use, so ASan checks every bound the shim hands over).
// Part 1: argument validation -- a null context, a bad list, a duplicate destination, a short or null buffer, a record that does not
// fit: named, nothing changes, and for a host buffer no device use.  Part 2: a round trip between two contexts at different frame
// indices with known table contents: the ring's rotation, both index translations (a track with MORE frames than its destination has
// seen included) and the canonical bytes.  Part 3: one scenario walked once per HIP call with that call failing: a failure is
// reported as FX_ERR_HIP / FX_ERR_OUT_OF_MEMORY, an export changes nothing, the tracks an import did not list keep every row, the
// host mirror of the per-track table equals the device table, the next call works, nothing leaks.  Host buffers go through the device
// scratch in chunks (two records each here).  Part 4: fx::LiveAnalyser's pair on two running engines.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include <unistd.h>

#include <atomic>
#include <thread>

#include "fx.h"
#include "fx_kernels.h"
#include "fx_context.h"
#include "fx_realtime.hpp"        // fx::LiveAnalyser::exportTracks / importTracks: made by the worker, the caller waits

namespace { hipStream_t g_header_copy_stream = nullptr; }
// (the fake runtime has no strided copy; the shim makes it on the context's stream, which is recorded here)
extern "C" hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t stream)
{
    const hipError_t e = fake_hip_count("hipMemcpy2DAsync");
    g_header_copy_stream = stream;
    if (e != hipSuccess) return e;
    for (size_t r = 0; r < height; r++) memcpy(static_cast<unsigned char*>(dst) + r * dpitch, static_cast<const unsigned char*>(src) + r * spitch, width);
    return hipSuccess;
}

namespace {
int g_problems = 0;
const char* g_where = "";
long g_packs = 0, g_unpacks = 0;
bool g_bad_launch = false;
void problem(const char* what, const char* more = "")
{
    std::printf("PROBLEM [%s]: %s %s\n", g_where, what, more);
    g_problems++;
}
#define EXPECT(cond) do { if (!(cond)) problem("expected", #cond); } while (0)
constexpr int N = 1024, H = N / 2, ROW = N / 8;
constexpr int HLEN = fxk::HLEN;

bool sane(const fxk::TrackStateParams& p)
{
    if (p.n <= 0 || p.C <= 0 || p.row_pieces != ROW || p.hist_base < 0 || p.hist_base >= HLEN || p.carry_bytes < 0 || p.carry_bytes >= H * 4) return false;
    if (!p.entries || !p.prev || !p.tail || !p.carry || !p.hist || !p.latest || !p.records) return false;
    for (int i = 0; i < p.n; i++) if (p.entries[i].channel < 0 || p.entries[i].channel >= p.C) return false;
    return true;
}
struct Piece { unsigned w[4]; };
// piece `at` of channel c's row(s) of the table track_piece names
Piece* table_piece(const fxk::TrackStateParams& p, const fxk::TrackPiece& t, int c)
{
    switch (t.where) {
    case fxk::TRACK_IN_LATEST: return reinterpret_cast<Piece*>(p.latest) + (size_t) c * fxk::TRACK_LATEST_PIECES + t.at;
    case fxk::TRACK_IN_RING: return reinterpret_cast<Piece*>(p.hist) + (size_t) c * fxk::TRACK_RING_PIECES + t.at;
    case fxk::TRACK_IN_PREV: return reinterpret_cast<Piece*>(p.prev) + (size_t) c * p.row_pieces + t.at;
    case fxk::TRACK_IN_TAIL: return reinterpret_cast<Piece*>(p.tail) + (size_t) c * p.row_pieces + t.at;
    default: return reinterpret_cast<Piece*>(p.carry) + (size_t) c * p.row_pieces + t.at;
    }
}
}

namespace fxk {
// (fx_tracks.hip is linked for fx_reset_channels / fx_get_channel_frames; its kernel's stand-in only counts)
hipError_t launch_reset_channels_kernel(const ResetParams&, hipStream_t) { return fake_hip_count("launch_reset_channels_kernel"); }
hipError_t launch_pack_tracks_kernel(const TrackStateParams& p, hipStream_t)
{
    const hipError_t e = fake_hip_count("launch_pack_tracks_kernel");
    if (e != hipSuccess) return e;
    g_packs++;
    if (!sane(p)) { g_bad_launch = true; return hipSuccess; }
    const int rec = (int) track_record_pieces(p.row_pieces * 8);
    for (int i = 0; i < p.n; i++)
        for (int q = 0; q < rec; q++) {
            const TrackPiece t = track_piece(q, p.row_pieces, p.hist_base);
            const int c = p.entries[i].channel;
            Piece v = {{0, 0, 0, 0}};
            if (t.where == TRACK_IN_HEADER) memcpy(&v, reinterpret_cast<const unsigned char*>(&p.entries[i].header) + 16 * t.at, 16);
            else if (t.where == TRACK_IN_RING) { if (p.entries[i].header.frames - HLEN + t.ring_row >= 0) v = *table_piece(p, t, c); }
            else if (t.where == TRACK_IN_CARRY) {
                if (t.at * 16 < p.carry_bytes) { v = *table_piece(p, t, c); for (int w = 0; w < 4; w++) v.w[w] &= track_carry_mask(t.at, w, p.carry_bytes); }
            }
            else v = *table_piece(p, t, c);
            memcpy(p.records + ((size_t) i * rec + q) * 16, &v, 16);
        }
    return hipSuccess;
}
hipError_t launch_unpack_tracks_kernel(const TrackStateParams& p, hipStream_t)
{
    const hipError_t e = fake_hip_count("launch_unpack_tracks_kernel");
    if (e != hipSuccess) return e;
    g_unpacks++;
    if (!sane(p)) { g_bad_launch = true; return hipSuccess; }
    const int rec = (int) track_record_pieces(p.row_pieces * 8);
    for (int i = 0; i < p.n; i++)
        for (int q = TRACK_HEADER_PIECES; q < rec; q++) {
            const TrackPiece t = track_piece(q, p.row_pieces, p.hist_base);
            memcpy(table_piece(p, t, p.entries[i].channel), p.records + ((size_t) i * rec + q) * 16, 16);
        }
    return hipSuccess;
}
}

namespace {

// ---- known table contents (the fake's device memory is host memory) ----
float ring_value(int track_id, long long track_frame, int s) { return (float) (track_id * 100000 + track_frame * 16 + s + 1); }
// what a track with identity `id` that has analysed `frames` frames would have left in slot c of context x
void plant(fx_context* x, int c, int id, long long frames)
{
    for (int r = 0; r < HLEN; r++) {
        // the newest global frame g < frames_seen with g mod HLEN == r
        long long g = x->frames_seen - 1 - ((x->frames_seen - 1 - r) % HLEN + HLEN) % HLEN;
        const long long f = g - (x->frames_seen - frames);              // the track's own index of that frame
        for (int s = 0; s < FX_NUM_FEATURES; s++)
            x->d_hist[((size_t) c * HLEN + r) * FX_NUM_FEATURES + s] = f >= 0 ? ring_value(id, f, s) : -777.0f;   // (rows before the track's first: stale, never valid)
    }
    for (int s = 0; s < FX_NUM_FEATURES; s++) x->d_latest[(size_t) c * FX_NUM_FEATURES + s] = (float) (id * 1000 + s);
    for (int j = 0; j < H; j++) {
        x->d_prev[(size_t) c * H + j] = (float) (id * 7 + j);
        x->d_tail[x->cur][(size_t) c * H + j] = (float) (id * 11 - j);
    }
    for (int j = 0; j < H * 4; j++) x->d_carry[x->carry_cur][(size_t) c * H * 4 + j] = (unsigned char) (id * 13 + j + 1);
}
std::vector<unsigned char> rows_of(const fx_context* x, int c)
{
    std::vector<unsigned char> v;
    auto add = [&v](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); v.insert(v.end(), b, b + n); };
    add(x->d_hist + (size_t) c * HLEN * FX_NUM_FEATURES, HLEN * FX_NUM_FEATURES * 4);
    add(x->d_latest + (size_t) c * FX_NUM_FEATURES, FX_NUM_FEATURES * 4);
    add(x->d_prev + (size_t) c * H, H * 4);
    add(x->d_tail[x->cur] + (size_t) c * H, H * 4);
    add(x->d_carry[x->carry_cur] + (size_t) c * H * 4, H * 4);
    return v;
}
struct Rows {
    std::vector<long long> frames;
    std::vector<float> gain, sens;
    std::vector<int> window, type;
    bool operator==(const Rows& o) const { return frames == o.frames && gain == o.gain && sens == o.sens && window == o.window && type == o.type; }
};
Rows get(fx_context* c, int C)
{
    Rows r;
    r.frames.resize((size_t) C); r.gain.resize((size_t) C); r.sens.resize((size_t) C); r.window.resize((size_t) C); r.type.resize((size_t) C);
    if (fx_get_channel_frames(c, r.frames.data()) != FX_OK) problem("fx_get_channel_frames");
    if (fx_get_channel_settings(c, r.gain.data(), r.sens.data(), r.window.data(), r.type.data()) != FX_OK) problem("fx_get_channel_settings");
    return r;
}
bool mirror_equals_table(const fx_context* c)
{
    if (c->chan.empty()) return c->d_chan == nullptr;
    return c->d_chan && !memcmp(c->d_chan, c->chan.data(), c->chan.size() * sizeof(fxk::ChannelSettings));
}
bool push(fx_context* c, int C, int hops)
{
    std::vector<float> in((size_t) C * hops * H, 0.25f), raw((size_t) C * hops * FX_NUM_FEATURES), sm(raw.size());
    return fx_push_hops(c, in.data(), hops, FX_SAMPLE_F32, FX_MEM_HOST, raw.data(), sm.data()) == FX_OK;
}
bool is_device_failure(fx_status st) { return st == FX_ERR_HIP || st == FX_ERR_OUT_OF_MEMORY; }

void validation()
{
    g_where = "validation";
    const int list[3] = {1, 4, 4}, two[2] = {1, 4};
    std::vector<unsigned char> buf(4 * (2432 + 6 * N));
    EXPECT(fx_track_state_bytes(nullptr) == 0);
    EXPECT(fx_export_channels(nullptr, list, 3, buf.data(), buf.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "null context"));
    EXPECT(fx_import_channels(nullptr, list, 0, nullptr, 0, FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT);
    fake_hip_reset();
    fx_context* c = nullptr; fx_context* other = nullptr; fx_context* pending = nullptr;
    if (fx_create(&c, 0, 6, N, 48000.0, 0) != FX_OK || fx_create(&other, 0, 6, N, 48000.0, FX_ORDER_HARMONIC_THEN_SPECTRAL) != FX_OK
        || fx_create(&pending, 0, 6, N, 48000.0, 0) != FX_OK) { problem("fx_create"); return; }
    const size_t size = fx_track_state_bytes(c);
    EXPECT(size == 2432 + 6 * N && size % 16 == 0);
    int frames = 0;
    std::vector<float> blk((size_t) 6 * 100, 0.5f);
    EXPECT(fx_push_samples(pending, blk.data(), 100, FX_SAMPLE_F32, FX_MEM_HOST, nullptr, nullptr, &frames) == FX_OK && fx_pending_samples(pending) == 100);
    std::vector<unsigned char> good(2 * size), flagged(2 * size), held(2 * size);
    EXPECT(fx_export_channels(c, two, 2, good.data(), good.size(), FX_MEM_HOST) == FX_OK);
    EXPECT(fx_export_channels(other, two, 2, flagged.data(), flagged.size(), FX_MEM_HOST) == FX_OK);
    EXPECT(fx_export_channels(pending, two, 2, held.data(), held.size(), FX_MEM_HOST) == FX_OK);
    const Rows before = get(c, 6);
    const long calls = fake_hip_calls(), packs = g_packs;
    const int high[3] = {0, 2, 6}, low[2] = {3, -1}, twice[3] = {2, 5, 2};
    EXPECT(fx_export_channels(c, nullptr, 0, nullptr, 0, FX_MEM_HOST) == FX_OK && fx_import_channels(c, list, 0, nullptr, 0, FX_MEM_DEVICE) == FX_OK);
    EXPECT(fx_export_channels(c, nullptr, 2, buf.data(), buf.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_import_channels(c, list, -1, buf.data(), buf.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_export_channels(c, high, 3, buf.data(), buf.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "entry 2"));
    EXPECT(fx_import_channels(c, low, 2, good.data(), good.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "entry 1"));
    EXPECT(fx_import_channels(c, twice, 3, buf.data(), buf.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "entry 2"));
    EXPECT(fx_export_channels(c, list, 3, buf.data(), 3 * size - 1, FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_import_channels(c, two, 2, good.data(), 2 * size - 1, FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_import_channels(c, two, 2, nullptr, 2 * size, FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_export_channels(c, two, 2, buf.data(), buf.size(), 7) == FX_ERR_INVALID_ARGUMENT);
    EXPECT(fx_export_channels(c, two, 2, buf.data() + 8, 2 * size, FX_MEM_DEVICE) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "16-byte"));
    EXPECT(fx_import_channels(c, two, 2, buf.data() + 8, 2 * size, FX_MEM_DEVICE) == FX_ERR_INVALID_ARGUMENT);
    // records that do not fit, from a host buffer: refused before any device use
    EXPECT(fx_import_channels(c, two, 2, flagged.data(), flagged.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "record 0") && strstr(fx_last_error(), "flags"));
    EXPECT(fx_import_channels(c, two, 2, held.data(), held.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "pending count"));
    std::vector<unsigned char> bad = good;
    bad[size + 1] ^= 0x10;
    EXPECT(fx_import_channels(c, two, 2, bad.data(), bad.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "record 1") && strstr(fx_last_error(), "magic"));
    bad = good;
    bad[4] = 2;
    EXPECT(fx_import_channels(c, two, 2, bad.data(), bad.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "version"));
    bad = good;
    const int n2 = 2048;
    memcpy(&bad[8], &n2, 4);
    EXPECT(fx_import_channels(c, two, 2, bad.data(), bad.size(), FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "window size"));
    EXPECT(fake_hip_calls() == calls && g_packs == packs && g_unpacks == 0);           // nothing of it touched the device
    EXPECT(get(c, 6) == before && c->chan.empty());
    // from a device buffer the headers come back in ONE strided copy, and a refusal stops there
    EXPECT(fx_import_channels(c, two, 2, flagged.data(), flagged.size(), FX_MEM_DEVICE) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "flags"));
    EXPECT(fake_hip_calls() == calls + 3 && g_unpacks == 0 && c->chan.empty());        // hipSetDevice, hipMemcpy2DAsync, hipStreamSynchronize
    EXPECT(g_header_copy_stream == c->stream && c->stream != nullptr);                 // ordered with what the caller queued on the context's stream
    EXPECT(fx_destroy(c) == FX_OK && fx_destroy(other) == FX_OK && fx_destroy(pending) == FX_OK && fake_hip_live() == 0);
}

// A (6 tracks, 60 frames: ring lapped) -> B (4 tracks, 3 frames: the moved tracks have MORE frames than B has seen) -> D (3 tracks,
// 100 frames), with a young track (5 frames: invalid ring rows) among them
void round_trip()
{
    g_where = "round trip";
    fake_hip_reset();
    fx_context* a = nullptr; fx_context* b = nullptr; fx_context* d = nullptr;
    if (fx_create(&a, 0, 6, N, 48000.0, 0) != FX_OK || fx_create(&b, 0, 4, N, 48000.0, 0) != FX_OK || fx_create(&d, 0, 3, N, 48000.0, 0) != FX_OK) { problem("fx_create"); return; }
    const float gains[6] = {1, 0.5f, -1, 2, 0.25f, 4};
    const float sens[6] = {0.7f, 0.3f, 0.1f, 0.2f, 0.5f, 0.15f};
    const int windows[6] = {5, 3, 1, 8, 21, 5}, types[6] = {1, 0, 2, 1, 0, 1};
    bool ok = push(a, 6, 30) && push(a, 6, 25);
    ok &= fx_set_channel_gains(a, gains) == FX_OK && fx_set_channel_onset(a, sens, windows, types) == FX_OK;   // onset windows reset at frame 55
    const int young[1] = {3};
    ok &= fx_reset_channels(a, young, 1) == FX_OK;                                    // track 3 starts at frame 55
    ok &= push(a, 6, 5) && push(b, 4, 3) && push(d, 3, 100);
    if (!ok) { problem("preparing the contexts:", fx_last_error()); return; }
    EXPECT(a->frames_seen == 60 && b->frames_seen == 3 && d->frames_seen == 100);
    // host buffers go through the device scratch two records at a time: the three-record export below is two chunks
    EXPECT(fx_set_tuning_internal(a, FX_HOOK_SMALL_TRACK_CHUNKS) == FX_OK && fx_set_tuning_internal(d, FX_HOOK_SMALL_TRACK_CHUNKS) == FX_OK);
    for (int c = 0; c < 6; c++) plant(a, c, 10 + c, c == 3 ? 5 : 60);
    for (int c = 0; c < 4; c++) plant(b, c, 20 + c, 3);
    for (int c = 0; c < 3; c++) plant(d, c, 30 + c, 100);
    const size_t size = fx_track_state_bytes(a);
    const int from_a[3] = {1, 3, 3}, into_b[2] = {2, 0}, into_d[2] = {1, 2};
    std::vector<unsigned char> rec(3 * size), again(2 * size), third(2 * size);
    std::vector<std::vector<unsigned char>> a_rows, b_rows;
    for (int c = 0; c < 6; c++) a_rows.push_back(rows_of(a, c));
    for (int c = 0; c < 4; c++) b_rows.push_back(rows_of(b, c));
    const Rows a_before = get(a, 6), b_before = get(b, 4);
    const long packs_before = g_packs;
    EXPECT(fx_export_channels(a, from_a, 3, rec.data(), rec.size(), FX_MEM_HOST) == FX_OK);
    EXPECT(g_packs == packs_before + 2 && a->track_state && a->track_state_release);
    for (int c = 0; c < 6; c++) EXPECT(rows_of(a, c) == a_rows[(size_t) c]);            // an export changes nothing
    EXPECT(get(a, 6) == a_before && mirror_equals_table(a));
    EXPECT(!memcmp(&rec[size], &rec[2 * size], size));
    // the record itself: header, then the ring in TRACK order with zeros before the track's first frame
    for (int i = 0; i < 2; i++) {
        const int track = from_a[i];
        const long long frames = track == 3 ? 5 : 60;
        fxk::TrackHeader h;
        memcpy(&h, &rec[(size_t) i * size], sizeof h);
        EXPECT(h.magic == fxk::TRACK_MAGIC && h.N == N && h.family == 1 && h.pending == 0 && h.frames == frames && h.onset_frames == 5);
        EXPECT(h.gain == gains[track] && h.sensitivity == sens[track] && h.onset_window == windows[track] && h.onset_type == types[track] && h.record_bytes == size);
        const float* ring = reinterpret_cast<const float*>(&rec[(size_t) i * size + 128]);
        for (int k = 0; k < HLEN; k++)
            for (int s = 0; s < FX_NUM_FEATURES; s++) {
                const long long f = frames - HLEN + k;
                if (ring[k * FX_NUM_FEATURES + s] != (f >= 0 ? ring_value(10 + track, f, s) : 0.0f)) { problem("a ring row of the record is not the track's frame frames - 48 + k"); k = HLEN; break; }
            }
    }
    EXPECT(fx_import_channels(b, into_b, 2, rec.data(), 2 * size, FX_MEM_HOST) == FX_OK);
    for (int c : {1, 3}) EXPECT(rows_of(b, c) == b_rows[(size_t) c]);                  // the tracks not listed
    const Rows b_after = get(b, 4);
    EXPECT(b_after.frames == (std::vector<long long>{5, 3, 60, 3}) && mirror_equals_table(b));
    EXPECT(b->chan[2].first_frame == 3 - 60 && b->chan[2].onset_reset_frame == 3 - 5 && b->chan[0].first_frame == -2 && b->chan[1].first_frame == 0);
    EXPECT(b_after.gain[2] == gains[1] && b_after.sens[0] == sens[3] && b_after.window[2] == 3 && b_after.type[0] == 1 && b_after.gain[1] == b_before.gain[1]);
    // B's ring: the row of global frame g is g mod 48, and global g is the track's frame g - first_frame
    for (int s = 0; s < FX_NUM_FEATURES; s++) {
        EXPECT(b->d_hist[((size_t) 2 * HLEN + 2) * FX_NUM_FEATURES + s] == ring_value(11, 59, s));               // global 2 = the track's frame 59
        EXPECT(b->d_hist[((size_t) 2 * HLEN + 3) * FX_NUM_FEATURES + s] == ring_value(11, 12, s));               // global -45 = row 3: frame 12, the oldest kept
        EXPECT(b->d_hist[((size_t) 0 * HLEN + 2) * FX_NUM_FEATURES + s] == ring_value(13, 4, s));                // the young track's newest
        EXPECT(b->d_hist[((size_t) 0 * HLEN + 20) * FX_NUM_FEATURES + s] == 0.0f);                               // ... and a row before its first
    }
    EXPECT(fx_export_channels(b, into_b, 2, again.data(), again.size(), FX_MEM_HOST) == FX_OK && !memcmp(again.data(), rec.data(), 2 * size));
    // on through a DEVICE buffer (the fake's device memory) into D, which has lapped its ring twice
    void* dev = nullptr;
    if (hipMalloc(&dev, 2 * size) != hipSuccess) { problem("hipMalloc"); return; }
    EXPECT(fx_export_channels(b, into_b, 2, dev, 2 * size, FX_MEM_DEVICE) == FX_OK && !memcmp(dev, rec.data(), 2 * size));
    EXPECT(fx_import_channels(d, into_d, 2, dev, 2 * size, FX_MEM_DEVICE) == FX_OK);
    EXPECT(fx_export_channels(d, into_d, 2, third.data(), third.size(), FX_MEM_HOST) == FX_OK && !memcmp(third.data(), rec.data(), 2 * size));
    EXPECT(get(d, 3).frames == (std::vector<long long>{100, 60, 5}) && d->chan[1].first_frame == 40 && d->chan[2].onset_reset_frame == 95);
    // the moved tracks count on from where they were
    EXPECT(push(b, 4, 2) && get(b, 4).frames == (std::vector<long long>{7, 5, 62, 5}));
    EXPECT(hipFree(dev) == hipSuccess);
    EXPECT(fx_destroy(a) == FX_OK && fx_destroy(b) == FX_OK && fx_destroy(d) == FX_OK && fake_hip_live() == 0);

    // samples pending: 100 of 16-bit PCM = 200 bytes, which end inside a 16-byte piece; the record keeps those and zeroes the rest
    g_where = "round trip with samples pending";
    fx_context* p = nullptr; fx_context* q = nullptr;
    if (fx_create(&p, 0, 2, N, 48000.0, 0) != FX_OK || fx_create(&q, 0, 5, N, 48000.0, 0) != FX_OK) { problem("fx_create"); return; }
    std::vector<short> pcm((size_t) 5 * 100, 1234);
    int frames = 0;
    EXPECT(fx_push_samples(p, pcm.data(), 100, FX_SAMPLE_S16, FX_MEM_HOST, nullptr, nullptr, &frames) == FX_OK);
    EXPECT(push(q, 5, 4) && fx_push_samples(q, pcm.data(), 100, FX_SAMPLE_S16, FX_MEM_HOST, nullptr, nullptr, &frames) == FX_OK);
    plant(p, 1, 41, 0);
    plant(q, 4, 42, 4);
    const std::vector<unsigned char> q4 = rows_of(q, 4);
    const int one[1] = {1}, four[1] = {3};
    std::vector<unsigned char> r1(size), r2(size);
    EXPECT(fx_export_channels(p, one, 1, r1.data(), size, FX_MEM_HOST) == FX_OK);
    const unsigned char* carry = &r1[2432 + 4 * N];
    bool kept = true, zeroed = true;
    for (int j = 0; j < H * 4; j++) {
        if (j < 200) kept &= carry[j] == (unsigned char) (41 * 13 + j + 1);
        else zeroed &= carry[j] == 0;
    }
    EXPECT(kept && zeroed);
    EXPECT(fx_import_channels(q, four, 1, r1.data(), size, FX_MEM_HOST) == FX_OK && rows_of(q, 4) == q4);
    EXPECT(fx_export_channels(q, four, 1, r2.data(), size, FX_MEM_HOST) == FX_OK && r1 == r2);
    EXPECT(get(q, 5).frames == (std::vector<long long>{4, 4, 4, 0, 4}));
    // ... and the same count of another format is refused
    fx_context* f32 = nullptr;
    std::vector<float> blk((size_t) 2 * 100, 0.5f);
    if (fx_create(&f32, 0, 2, N, 48000.0, 0) != FX_OK) { problem("fx_create"); return; }
    EXPECT(fx_push_samples(f32, blk.data(), 100, FX_SAMPLE_F32, FX_MEM_HOST, nullptr, nullptr, &frames) == FX_OK);
    EXPECT(fx_import_channels(f32, one, 1, r1.data(), size, FX_MEM_HOST) == FX_ERR_INVALID_ARGUMENT && strstr(fx_last_error(), "carry format"));
    EXPECT(fx_destroy(p) == FX_OK && fx_destroy(q) == FX_OK && fx_destroy(f32) == FX_OK && fake_hip_live() == 0);
}

struct Scene { fx_context* a = nullptr; fx_context* b = nullptr; fx_stream* ring = nullptr; void* dev = nullptr; };

// an import takes effect whole, or the tracks it did not list keep every row; returns its status
fx_status import_checked(fx_context* b, const std::vector<int>& list, const void* in, size_t bytes, int kind, const char* what)
{
    const int C = b->C;
    std::vector<bool> listed((size_t) C, false);
    for (int ch : list) listed[(size_t) ch] = true;
    const Rows before = get(b, C);
    std::vector<std::vector<unsigned char>> rows;
    for (int c = 0; c < C; c++) rows.push_back(rows_of(b, c));
    const fx_status st = fx_import_channels(b, list.data(), (int) list.size(), in, bytes, kind);
    const Rows after = get(b, C);
    if (st != FX_OK && !is_device_failure(st)) problem(what, "failed with a status that is not a device failure");
    if (!mirror_equals_table(b)) problem(what, "left the host mirror and the device table different");
    for (int c = 0; c < C; c++) {
        if (listed[(size_t) c]) continue;
        if (rows_of(b, c) != rows[(size_t) c]) problem(what, "changed a row of a track it did not list");
        if (after.frames[(size_t) c] != before.frames[(size_t) c] || after.gain[(size_t) c] != before.gain[(size_t) c] || after.sens[(size_t) c] != before.sens[(size_t) c]
            || after.window[(size_t) c] != before.window[(size_t) c] || after.type[(size_t) c] != before.type[(size_t) c]) problem(what, "changed the settings of a track it did not list");
    }
    return st;
}
fx_status export_checked(fx_context* a, const std::vector<int>& list, void* out, size_t bytes, int kind, const char* what)
{
    const int C = a->C;
    const Rows before = get(a, C);
    std::vector<std::vector<unsigned char>> rows;
    for (int c = 0; c < C; c++) rows.push_back(rows_of(a, c));
    const fx_status st = fx_export_channels(a, list.data(), (int) list.size(), out, bytes, kind);
    if (st != FX_OK && !is_device_failure(st)) problem(what, "failed with a status that is not a device failure");
    if (!(get(a, C) == before) || !mirror_equals_table(a)) problem(what, "changed a setting or a frame count");
    for (int c = 0; c < C; c++) if (rows_of(a, c) != rows[(size_t) c]) problem(what, "changed a row");
    return st;
}

bool scenario(Scene* s)
{
    bool ok = true;
    if (fx_create(&s->a, 0, 6, N, 48000.0, 0) != FX_OK) return false;
    if (fx_create(&s->b, 0, 4, N, 48000.0, 0) != FX_OK) return false;
    fx_context* a = s->a; fx_context* b = s->b;
    fx_tuning t;
    if (fx_get_tuning(b, &t) != FX_OK) return false;
    t.stream_hop_kernel = 0;                    // the ring's one-hop step is then the captured step (hipGraph)
    ok &= fx_set_tuning(b, &t) == FX_OK;
    ok &= fx_set_tuning_internal(a, FX_HOOK_SMALL_TRACK_CHUNKS) == FX_OK;      // the three-record host export: two chunks through the scratch
    const float gains[6] = {1, 0.5f, -1, 2, 0.25f, 4};
    ok &= fx_set_channel_gains(a, gains) == FX_OK;
    ok &= push(a, 6, 7) && push(b, 4, 2);
    std::vector<float> hop((size_t) 4 * H, 0.25f), raw((size_t) 4 * FX_NUM_FEATURES), sm(raw.size());
    if (fx_stream_create(b, 1, 2, FX_SAMPLE_F32, &s->ring) != FX_OK) ok = false;
    auto ring_steps = [&](int n) {
        for (int i = 0; s->ring && i < n; i++) {
            if (fx_stream_push(s->ring, hop.data(), 1) != FX_OK) { ok = false; continue; }
            ok &= fx_stream_collect(s->ring, raw.data(), sm.data()) == FX_OK;
        }
    };
    ring_steps(3);                              // both parities of the step captured without a table
    const size_t size = fx_track_state_bytes(a);
    std::vector<unsigned char> rec(3 * size, 0xee);
    // (records of an export that failed are not records: the import that would take them is left out)
    const bool first = export_checked(a, {1, 3, 3}, rec.data(), rec.size(), FX_MEM_HOST, "fx_export_channels to a host buffer") == FX_OK;
    ok &= first && import_checked(b, {2, 0}, rec.data(), 2 * size, FX_MEM_HOST, "fx_import_channels (first: the table appears)") == FX_OK;
    ring_steps(3);                              // captured once more with the table's address
    if (hipMalloc(&s->dev, 5 * size) != hipSuccess) return false;
    const bool second = export_checked(a, {0, 1, 2, 4, 5}, s->dev, 5 * size, FX_MEM_DEVICE, "fx_export_channels of a longer list to a device buffer") == FX_OK;
    ok &= second && import_checked(b, {3, 1, 0}, s->dev, 3 * size, FX_MEM_DEVICE, "fx_import_channels from a device buffer over a table") == FX_OK;
    ok &= export_checked(b, {0, 1, 2, 3}, s->dev, 4 * size, FX_MEM_DEVICE, "fx_export_channels of the destination") == FX_OK;
    ok &= push(b, 4, 2);
    return ok;
}

void finish(Scene* s)
{
    fake_hip_fail_at(0);
    if (s->a && s->b) {
        // with the fault gone the calls work, whatever it interrupted
        const size_t size = fx_track_state_bytes(s->a);
        std::vector<unsigned char> rec(2 * size);
        const int from[2] = {5, 0}, into[2] = {1, 3};
        if (fx_export_channels(s->a, from, 2, rec.data(), rec.size(), FX_MEM_HOST) != FX_OK) problem("fx_export_channels after the fault");
        if (fx_import_channels(s->b, into, 2, rec.data(), rec.size(), FX_MEM_HOST) != FX_OK) problem("fx_import_channels after the fault");
        long long fa[6], fb[4];
        if (fx_get_channel_frames(s->a, fa) != FX_OK || fx_get_channel_frames(s->b, fb) != FX_OK || fb[1] != fa[5] || fb[3] != fa[0]) problem("the tracks moved after the fault do not carry their frame counts");
        if (!mirror_equals_table(s->b)) problem("mirror and table differ after the fault");
    }
    if (s->dev) (void) hipFree(s->dev);
    if (s->ring && fx_stream_destroy(s->ring) != FX_OK) problem("fx_stream_destroy");
    if (s->a && fx_destroy(s->a) != FX_OK) problem("fx_destroy");
    if (s->b && fx_destroy(s->b) != FX_OK) problem("fx_destroy");
    if (fake_hip_live() != 0) problem("device objects left behind");
}

void walk()
{
    g_where = "clean run";
    fake_hip_reset();
    Scene s;
    if (!scenario(&s)) problem("the scenario fails without any injected failure:", fx_last_error());
    const long calls = fake_hip_calls();
    finish(&s);
    if (g_packs < 5 || g_unpacks < 3) problem("the pack / unpack kernels were not launched once per call");
    int reported = 0;
    for (long k = 1; k <= calls; k++) {
        char tag[128];
        fake_hip_reset();
        fake_hip_fail_at(k);
        std::snprintf(tag, sizeof tag, "HIP call %ld failing", k);
        g_where = tag;
        Scene f;
        const bool fine = scenario(&f);
        if (fake_hip_failed() && !fine) reported++;
        std::snprintf(tag, sizeof tag, "HIP call %ld (%s) failing", k, fake_hip_failed() ? fake_hip_failed_name() : "not reached");
        finish(&f);
    }
    if (g_bad_launch) problem("a launch of the pack / unpack kernels had a bad argument");
    std::printf("scenario: %ld HIP calls, each failed once, %d reported to the caller\n", calls, reported);
}

// fx::LiveAnalyser::exportTracks / importTracks (include/fx_realtime.hpp) while both engines take blocks: the worker makes the call
// between two blocks and the caller gets the result or the error; from a worker callback the call is made at once; a stopped engine
// refuses instead of waiting for ever.
void live_engines()
{
    g_where = "live engines";
    fake_hip_reset();
    try {
        fx::RealTimeBatchAnalyser src(6, N), dst(4, N);
        {
            fx::LiveAnalyser from(src, H, 4), into(dst, H, 4);
            std::atomic<int> inside{0};
            std::vector<unsigned char> fromCallback;
            from.setFramesAnalysedCallback([&](int, const float*, const float*) {
                if (inside.fetch_add(1) == 0) { const int t[1] = {2}; fromCallback = from.exportTracks(t, 1); }     // on the worker: made at once
            });
            std::vector<float> six((size_t) 6 * H, 0.25f), four((size_t) 4 * H, 0.5f);
            std::atomic<bool> feeding{true};
            std::thread audio([&] { while (feeding.load()) { (void) from.pushBlock(six.data(), H); (void) into.pushBlock(four.data(), H); usleep(100); } });
            const int tracks[3] = {1, 3, 3}, slots[2] = {2, 0};
            for (int round = 0; round < 20; round++) {
                std::vector<unsigned char> records = from.exportTracks(tracks, 3);
                EXPECT(records.size() == 3 * src.trackStateBytes() && !memcmp(&records[src.trackStateBytes()], &records[2 * src.trackStateBytes()], src.trackStateBytes()));
                records.resize(2 * src.trackStateBytes());
                into.importTracks(slots, 2, records);
                fxk::TrackHeader h;
                memcpy(&h, records.data(), sizeof h);
                const std::vector<unsigned char> back = into.exportTracks(slots, 1);
                fxk::TrackHeader g;
                memcpy(&g, back.data(), sizeof g);
                EXPECT(g.frames >= h.frames && g.frames - h.frames < 1000 && g.magic == fxk::TRACK_MAGIC);     // the track counts on in its new engine
            }
            bool refused = false;
            try { const int twice[2] = {1, 1}; std::vector<unsigned char> r = from.exportTracks(twice, 2); into.importTracks(twice, 2, r); }
            catch (const fx::Error& e) { refused = e.code == FX_ERR_INVALID_ARGUMENT && strstr(e.what(), "listed twice"); }
            EXPECT(refused);
            bool outOfRange = false;
            try { const int bad[1] = {6}; (void) from.exportTracks(bad, 1); } catch (const fx::Error& e) { outOfRange = e.code == FX_ERR_INVALID_ARGUMENT; }
            EXPECT(outOfRange);
            feeding = false;
            audio.join();
            from.drain(); into.drain();
            EXPECT(inside.load() > 0 && fromCallback.size() == src.trackStateBytes());
            EXPECT(from.getStats().errors == 0 && into.getStats().errors == 0);
            from.stop();
            bool stopped = false;
            try { (void) from.exportTracks(tracks, 3); } catch (const fx::Error&) { stopped = true; }
            EXPECT(stopped);
            into.stop();
        }
    } catch (const std::exception& e) { problem("the live engines threw:", e.what()); }
    EXPECT(fake_hip_live() == 0);
}

} // namespace

int main()
{
    validation();
    round_trip();
    live_engines();
    walk();
    std::printf("%s: %d problems\n", g_problems ? "FAILED" : "ok", g_problems);
    return g_problems ? 1 : 0;
}
