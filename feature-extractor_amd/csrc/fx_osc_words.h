// fx_osc_words.h -- the OSC feature message of a track with an address of its own (ref AnalyserTrackController.h:17,22-23: every
// track's (ip, secondaryIP, bundle); OSCFeatureAnalysisOutput.h:107: sender.send (bundleAddress, twelve floats)), formed one 4-byte
// word at a time.  fx_osc_table_kernel (fx_osc_table.hip) runs osc_table_word once per thread; a host program can call the very same
// function (tests/cpp/osc_table_host.cpp), and fx_osc_encode_addressed (fx_capi.cpp) shares the address rules.  No HIP header needed.
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

} // namespace fxk

#endif
