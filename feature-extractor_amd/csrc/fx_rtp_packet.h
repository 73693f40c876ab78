// fx_rtp_packet.h -- one RTP datagram with an L16 / L24 payload (RFC 3550 5.1, RFC 3551 4.5.11, RFC 3190), stated once: what makes it
// malformed, where its payload starts and how many sample times it holds, and where those land in a tick (include/fx.h, fx_push_rtp).
// Plain host/device functions, in the manner of fx_flux_runs.h and fx_osc_words.h: fx_rtp_parse_kernel (fx_rtp.hip), and the
// stand-alone host programs that hold them to the models (tests/cpp/rtp_packet_host.cpp, rtp_window_host.cpp) include this one statement.
//
// A packet is read through `byte(k)`, 0 <= k < len: any callable that returns byte k.  fx_rtp_parse asks for no k at or beyond len,
// whatever the bytes say, so a datagram that lies about its extension or its padding is refused without a read outside it.
#ifndef FX_RTP_PACKET_H
#define FX_RTP_PACKET_H

#if defined(__HIPCC__)
#define FX_RTP_FN __host__ __device__ inline
#else
#define FX_RTP_FN inline
#endif

// the disposition bits (FX_RTP_* of include/fx.h; this header stands alone)
enum { FX_RTP_BIT_PLACED = 1, FX_RTP_BIT_LATE = 2, FX_RTP_BIT_EARLY = 4, FX_RTP_BIT_MALFORMED = 8, FX_RTP_BIT_IGNORED = 16, FX_RTP_BIT_HELD = 32 };

struct fx_rtp_parsed {
    unsigned timestamp;     // T: the RTP timestamp of the first sample time
    int      payload;       // h: the payload's offset in the datagram
    int      sample_times;  // m >= 1
};

// false: malformed.  frame_bytes = the stream's channels x the bytes per sample: a sample time's bytes.
template <typename Byte>
FX_RTP_FN bool fx_rtp_parse(const Byte& byte, int len, int frame_bytes, fx_rtp_parsed* out)
{
    if (len < 12) return false;
    const unsigned b0 = byte(0);
    if ((b0 >> 6) != 2) return false;                                   // version 2
    int h = 12 + 4 * (int) (b0 & 15);                                   // the fixed header and CC contributing sources
    if (b0 & 0x10) {                                                    // X: a header extension, its length in 32-bit words
        if (h + 4 > len) return false;
        h += 4 + 4 * (int) ((byte(h + 2) << 8) | byte(h + 3));
    }
    if (h > len) return false;
    int pad = 0;
    if (b0 & 0x20) {                                                    // P: the last byte counts the padding, itself included
        pad = (int) byte(len - 1);
        if (pad == 0 || h + pad > len) return false;
    }
    const int payload = len - h - pad;
    if (payload <= 0 || payload % frame_bytes != 0) return false;
    out->timestamp = (byte(4) << 24) | (byte(5) << 16) | (byte(6) << 8) | byte(7);
    out->payload = h;
    out->sample_times = payload / frame_bytes;
    return true;
}

struct fx_rtp_placement {
    int      d0;            // the tick position of the packet's first sample time: (int32) (T - cursor), wrapping
    int      lo, hi;        // the positions it covers inside the tick, [lo, hi); empty unless PLACED
    unsigned bits;          // FX_RTP_BIT_PLACED / LATE / EARLY
};

struct fx_rtp_span_placement {
    int       d0;           // as fx_rtp_placement
    long long lo, hi;       // the positions it covers inside the span [0, n + W), [lo, hi); empty unless PLACED or HELD
    unsigned  bits;         // FX_RTP_BIT_PLACED / HELD / LATE / EARLY
};

// a valid packet of m sample times at timestamp T, in a tick of n positions whose first has timestamp `cursor`, with a reorder window
// of W sample times (include/fx.h, "the reorder window"; 0: none): the span is the tick's n positions and the W beyond them.  64-bit
// ends: neither d0 + m nor n + W overflows.
FX_RTP_FN fx_rtp_span_placement fx_rtp_place_span(unsigned T, unsigned cursor, int m, int n, int W)
{
    fx_rtp_span_placement p;
    p.d0 = (int) (T - cursor);
    const long long end = (long long) p.d0 + m, span = (long long) n + W;
    p.lo = p.d0 > 0 ? p.d0 : 0;
    p.hi = end < span ? end : span;
    const unsigned late = FX_RTP_BIT_LATE, early = FX_RTP_BIT_EARLY, placed = FX_RTP_BIT_PLACED, held = FX_RTP_BIT_HELD;
    const bool some = p.lo < end && p.lo < span;        // lo < hi, asked of the two ends: without a window nothing 64-bit but `end` is left
    p.bits = (p.d0 < 0 ? late : 0u) | (end > span ? early : 0u) | (some && p.lo < n ? placed : 0u) | (some && p.hi > n ? held : 0u);
    if (!some) p.lo = p.hi = 0;
    return p;
}

// the same without a window: the span is the tick, so hi <= n fits an int and HELD is never set
FX_RTP_FN fx_rtp_placement fx_rtp_place(unsigned T, unsigned cursor, int m, int n)
{
    const fx_rtp_span_placement p = fx_rtp_place_span(T, cursor, m, n, 0);
    return fx_rtp_placement{p.d0, (int) p.lo, (int) p.hi, p.bits};
}

#endif
