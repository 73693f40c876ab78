// fx_osc_words.h -- the OSC feature message of a track with an address of its own (ref AnalyserTrackController.h:17,22-23: every
// track's (ip, secondaryIP, bundle); OSCFeatureAnalysisOutput.h:107: sender.send (bundleAddress, twelve floats)), formed one 4-byte
// word at a time.  fx_osc_table_kernel (fx_osc_table.hip) runs osc_table_word once per thread; a host program can call the very same
// function (tests/cpp/osc_table_host.cpp), and fx_osc_encode_addressed (fx_capi.cpp) shares the address rules.  No HIP header needed.
// osc_bundle_word, below, is the same for a whole datagram of many tracks' messages: fx_osc_bundle_kernel (fx_osc_bundle.hip) and the
// host encoders fx_osc_encode_bundles* (fx_capi.cpp) call it.
//
// A message (fx_osc_encode, fx_capi.cpp, is the per-track host form of the same bytes):
//   address, NUL, zero-padded to a multiple of 4 | ",ffffffffffff" NUL NUL NUL (16 bytes) | twelve big-endian float32 in wire order
// The address table holds one zero-padded row of FX_OSC_ROW_BYTES bytes per track, so the address part of a message is whole aligned
// words of the row: an address of at most FX_OSC_ADDRESS_MAX = 124 bytes pads to at most 128, a message is at most 192 bytes.
#ifndef FX_OSC_WORDS_H
#define FX_OSC_WORDS_H

#include "../../include/fx.h"

#if defined(__HIPCC__)
#define FX_OSC_HD __host__ __device__
#else
#define FX_OSC_HD
#endif

namespace fxk {

constexpr int FX_OSC_ROW_BYTES = 128, FX_OSC_ROW_WORDS = FX_OSC_ROW_BYTES / 4;
static_assert(FX_OSC_ADDRESS_MAX + 4 <= FX_OSC_ROW_BYTES && FX_OSC_ADDRESS_MAX % 4 == 0, "a row holds the longest address, its NUL and the padding");

// wire position -> AudioFeatures slot (ref OSCFeatureAnalysisOutput.h:107), four bits each
constexpr unsigned long long osc_wire_nibble(int position, int slot) { return (unsigned long long) slot << (4 * position); }
constexpr unsigned long long k_osc_wire_slots =
    osc_wire_nibble(0, FX_ONSET) | osc_wire_nibble(1, FX_RMS) | osc_wire_nibble(2, FX_F0) | osc_wire_nibble(3, FX_CENTROID) |
    osc_wire_nibble(4, FX_SLOPE) | osc_wire_nibble(5, FX_SPREAD) | osc_wire_nibble(6, FX_FLATNESS) | osc_wire_nibble(7, FX_LER) |
    osc_wire_nibble(8, FX_FLUX) | osc_wire_nibble(9, FX_HER) | osc_wire_nibble(10, FX_OER) | osc_wire_nibble(11, FX_INHARM);
static_assert(FX_NUM_FEATURES == 12, "twelve floats on the wire");

// bytes of the message of an address of `alen` bytes
FX_OSC_HD inline int osc_addressed_bytes(int alen) { return ((alen + 4) & ~3) + 16 + 48; }

// Word w (little-endian, as a 4-byte load or store of the bytes sees it) of the message of the track whose table row is `row`
// (FX_OSC_ROW_WORDS words: the address, then zeros), whose address has `alen` bytes and whose latest vector is `latest12` (AudioFeatures
// slot order).  Words past the message are zero: a slot's remainder.
FX_OSC_HD inline unsigned osc_table_word(const unsigned* row, int alen, const float* latest12, int w)
{
    const int awords = (alen + 4) >> 2;
    if (w < awords) return row[w];
    const int t = w - awords;
    if (t < 4) return t == 0 ? 0x6666662Cu : (t == 3 ? 0x00000066u : 0x66666666u);      // ",ffffffffffff" and three NULs
    if (t >= 16) return 0u;
    const int slot = (int) ((k_osc_wire_slots >> (4 * (t - 4))) & 15u);
    unsigned bits;
    __builtin_memcpy(&bits, latest12 + slot, 4);
    return __builtin_bswap32(bits);
}

// What is wrong with an address (the rules of fx_set_osc_addresses, include/fx.h), or null and its length in *alen.  Host only.
inline const char* osc_address_fault(const char* address, int* alen)
{
    if (!address) return "is null";
    if (address[0] != '/') return address[0] ? "does not start with '/'" : "is empty";
    int n = 0;
    for (; address[n]; n++) {
        if (n >= FX_OSC_ADDRESS_MAX) return "is longer than FX_OSC_ADDRESS_MAX (124) bytes";
        const unsigned char b = (unsigned char) address[n];
        if (b < 0x21 || b > 0x7E) return "holds a byte outside 0x21 .. 0x7E";
    }
    *alen = n;
    return nullptr;
}

// fx_osc_table_kernel's arguments
struct OscTableParams {
    const float*    latest;     // [C][12]
    const unsigned* rows;       // [C][FX_OSC_ROW_WORDS]
    const int*      len;        // [C]: address bytes
    unsigned char*  out;        // [C][stride], 4-byte aligned
    int             C, stride;
};

// ---- bundles (include/fx.h: fx_osc_bundle_plan, fx_get_osc_bundles*, fx_osc_encode_bundles*) ----
// A bundle datagram (OSC 1.0): "#bundle\0" | 64-bit big-endian NTP time tag | per element: big-endian int32 size, then the element, which
// is byte for byte a track's message (ref OSCFeatureAnalysisOutput.h:107).  Bundle b of a call holds tracks [b * K, min(C, (b + 1) * K)).
constexpr int FX_OSC_PREFIX_BYTES = 64;             // = FX_OSC_PREFIX_MAX (fx_kernels.h)
constexpr int FX_OSC_BUNDLE_HEADER_WORDS = 4;

// What fx_osc_bundle_kernel and the host encoders form bundles from.  rows != null: the table form (osc_table_word); else the prefix
// form, "<prefix><first_channel + c>".  On the device the pointers are device memory, on the host the caller's arrays.
struct OscBundleParams {
    const float*    latest;         // [C][12]
    const unsigned* rows;           // [C][FX_OSC_ROW_WORDS] or null
    const int*      len;            // [C]: address bytes (table form)
    unsigned char*  out;            // [num_bundles][stride], 4-byte aligned
    int             C, K, stride;   // K tracks per bundle, 1 .. FX_OSC_BUNDLE_MAX_ELEMENTS; stride a multiple of 4 that holds the fullest bundle
    unsigned        timetag_hi, timetag_lo;
    int             first_channel;  // >= 0, first_channel + C - 1 <= INT_MAX
    int             prefix_len;     // <= FX_OSC_PREFIX_BYTES
    unsigned char   prefix[FX_OSC_PREFIX_BYTES];
};

FX_OSC_HD inline int osc_decimal_digits(unsigned n) { int d = 1; for (; n >= 10u; n /= 10u) d++; return d; }

// Word w of the message "<prefix><n>" (the prefix form of osc_table_word; fx_osc_kernel, fx_osc.hip, writes the same bytes)
FX_OSC_HD inline unsigned osc_prefix_word(const unsigned char* prefix, int prefix_len, unsigned n, const float* latest12, int w)
{
    const int alen = prefix_len + osc_decimal_digits(n), awords = (alen + 4) >> 2;
    if (w >= awords) return osc_table_word(nullptr, alen, latest12, w);     // (the row is read for address words only)
    unsigned v = 0;
    for (int j = 0; j < 4; j++) {
        const int b = 4 * w + j;
        unsigned ch = 0;
        if (b < prefix_len) ch = prefix[b];
        else if (b < alen) {
            unsigned t = n;
            for (int k = alen - 1 - b; k > 0; k--) t /= 10u;
            ch = '0' + t % 10u;
        }
        v |= ch << (8 * j);
    }
    return v;
}

// 4-byte words of track c's message
FX_OSC_HD inline int osc_bundle_element_words(const OscBundleParams& p, int c)
{
    const int alen = p.rows ? p.len[c] : p.prefix_len + osc_decimal_digits((unsigned) (p.first_channel + c));
    return osc_addressed_bytes(alen) >> 2;
}

// Word w (little-endian, as a 4-byte store sees it) of the output slot of bundle b.  off[0 .. count]: the word at which element e's size
// word sits, off[0] = FX_OSC_BUNDLE_HEADER_WORDS, off[e + 1] = off[e] + 1 + osc_bundle_element_words(track b * K + e), count = the
// bundle's elements, so off[count] = the bundle's words; words from there on are zero.  A header word, a size word or a message word.
FX_OSC_HD inline unsigned osc_bundle_word(const OscBundleParams& p, int b, const int* off, int count, int w)
{
    if (w < FX_OSC_BUNDLE_HEADER_WORDS)
        return w == 0 ? 0x6E756223u : (w == 1 ? 0x00656C64u : __builtin_bswap32(w == 2 ? p.timetag_hi : p.timetag_lo));       // "#bun" "dle\0"
    if (w >= off[count]) return 0u;
    int lo = 0, hi = count - 1;                     // the last element whose size word is at or before w
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= w) lo = mid; else hi = mid - 1;
    }
    const int at = w - off[lo] - 1;
    if (at < 0) return __builtin_bswap32((unsigned) (off[lo + 1] - off[lo] - 1) << 2);
    const int c = b * p.K + lo;
    const float* latest12 = p.latest + (size_t) c * FX_NUM_FEATURES;
    if (p.rows) return osc_table_word(p.rows + (size_t) c * FX_OSC_ROW_WORDS, p.len[c], latest12, at);
    return osc_prefix_word(p.prefix, p.prefix_len, (unsigned) (p.first_channel + c), latest12, at);
}

// fx_osc_bundle_plan's arithmetic; K = 0: no plan (the datagram does not hold one message, or the arguments are out of range)
inline int osc_bundle_tracks(int longest, int num_tracks, int max_datagram_bytes)
{
    if (longest < 4 || longest > 65507 || num_tracks < 1 || max_datagram_bytes > 65507 || max_datagram_bytes < 16 + 4 + longest) return 0;
    int K = (max_datagram_bytes - 16) / (4 + longest);
    if (K > FX_OSC_BUNDLE_MAX_ELEMENTS) K = FX_OSC_BUNDLE_MAX_ELEMENTS;
    return K > num_tracks ? num_tracks : K;
}

} // namespace fxk

#endif
