"""RTP datagrams with L16 / L24 payloads (RFC 3550, RFC 3551 4.5.11, RFC 3190) made on the host: what a sender puts on the wire
for the planar samples it is given, in the slots BatchAnalyser.push_rtp takes.  Host only -- for examples, tests and the tests of a
receiver; the unpacking is fx_push_rtp's (include/fx.h)."""
import numpy as np


def big_endian_bytes(planar_int, bytes_per_sample):
    """integer samples [..., n] -> uint8 [..., n, B]: each sample's low B bytes, most significant first (two's complement)"""
    v = np.asarray(planar_int).astype(np.int64)
    shifts = 8 * np.arange(bytes_per_sample - 1, -1, -1, dtype=np.int64)
    return ((v[..., None] >> shifts) & 0xFF).astype(np.uint8)


def packetise(planar_int, channels_per_stream, samples_per_packet, first_timestamps, csrc=0, extension_words=None, padding=0, bytes_per_sample=3,
              payload_type=97, ssrc=0x46580000):
    """The streams' datagrams for the samples planar_int [sum(channels_per_stream)][n] (integers; the low bytes_per_sample bytes of
    each are sent: 2 = L16, 3 = L24), rows in stream order: stream s carries the next channels_per_stream[s] rows, samples_per_packet
    sample times per datagram (the last one what is left), the first with RTP timestamp first_timestamps[s] (mod 2^32).
    csrc: contributing sources per header (0 .. 15); extension_words: None, or the words of a header extension (0 is a legal
    extension of no words); padding: 0, or the padding bytes at the end of every datagram (1 .. 255, the last one their count).
    -> (slots uint8 [P][stride], lengths int32 [P], stream_of int32 [P]), packets in stream order then time order, stride the
    longest datagram rounded up to a multiple of 4."""
    x = np.asarray(planar_int)
    chans = [int(k) for k in channels_per_stream]
    if x.ndim != 2 or x.shape[0] != sum(chans):
        raise ValueError("planar_int is [sum(channels_per_stream)][n]")
    if not 0 <= int(csrc) <= 15 or not 0 <= int(padding) <= 255 or int(samples_per_packet) < 1:
        raise ValueError("csrc 0..15, padding 0..255, samples_per_packet >= 1")
    n, B, m = x.shape[1], int(bytes_per_sample), int(samples_per_packet)
    first = np.broadcast_to(np.asarray(first_timestamps, dtype=np.int64), (len(chans),))
    wire = big_endian_bytes(x, B)                                                   # [rows][n][B]
    packets, stream_of = [], []
    row = 0
    for s, K in enumerate(chans):
        frames = np.ascontiguousarray(wire[row:row + K].transpose(1, 0, 2)).reshape(n, K * B)      # [n][K * B]: a sample time's bytes
        row += K
        for seq, q in enumerate(range(0, n, m)):
            t = (int(first[s]) + q) & 0xFFFFFFFF
            head = bytearray(12)
            head[0] = 0x80 | (0x20 if padding else 0) | (0x10 if extension_words is not None else 0) | int(csrc)
            head[1] = int(payload_type) & 0x7F
            head[2:4] = (seq & 0xFFFF).to_bytes(2, "big")
            head[4:8] = t.to_bytes(4, "big")
            head[8:12] = ((int(ssrc) + s) & 0xFFFFFFFF).to_bytes(4, "big")
            for k in range(int(csrc)):
                head += (0xC0000000 + k).to_bytes(4, "big")
            if extension_words is not None:
                head += (0xBEDE).to_bytes(2, "big") + int(extension_words).to_bytes(2, "big") + bytes(4 * int(extension_words))
            tail = (bytes(int(padding) - 1) + bytes([int(padding)])) if padding else b""
            packets.append(bytes(head) + frames[q:q + m].tobytes() + tail)
            stream_of.append(s)
    return slots_of(packets) + (np.asarray(stream_of, np.int32),)


def timestamps_of(slots):
    """slots uint8 [P][stride] of datagrams with a whole fixed header -> their RTP timestamps, int64 [P]"""
    s = np.asarray(slots, np.uint8)[:, 4:8].astype(np.int64)
    return (s[:, 0] << 24) | (s[:, 1] << 16) | (s[:, 2] << 8) | s[:, 3]


def arrival_ticks(positions, ahead, samples_per_tick):
    """The tick in which a receiver submits each packet: the packet's first sample time is `positions[i]` sample times after the
    first tick's cursor, the network delivers it `ahead[i]` sample times before that moment, and ticks are samples_per_tick long
    -> int64 [P], never below 0.  With a reorder window W (BatchAnalyser.rtp_set_window) a packet of m sample times that arrives
    0 .. W - m ahead lies whole in the span of its tick."""
    at = np.asarray(positions, np.int64) - np.asarray(ahead, np.int64)
    return np.maximum(at, 0) // int(samples_per_tick)


def cut_into_ticks(slots, lengths, stream_of, arrival, num_ticks=None):
    """One list of packets cut into ticks by an arrival schedule: packet i is submitted in tick arrival[i]
    -> [(slots, lengths, stream_of)] * num_ticks (None: up to the last arrival), each tick's packets in the order of the list.
    Reorder a tick's packets by indexing the three arrays alike."""
    arrival = np.asarray(arrival, np.int64).ravel()
    slots, lengths, stream_of = np.asarray(slots, np.uint8), np.asarray(lengths, np.int32), np.asarray(stream_of, np.int32)
    if not (arrival.size == slots.shape[0] == lengths.size == stream_of.size):
        raise ValueError("one arrival, length and stream per slot")
    if arrival.size and arrival.min() < 0:
        raise ValueError("a packet arrives in tick 0 or later")
    count = int(num_ticks) if num_ticks is not None else (int(arrival.max()) + 1 if arrival.size else 0)
    return [(slots[arrival == k], lengths[arrival == k], stream_of[arrival == k]) for k in range(count)]


def slots_of(packets, stride=None):
    """datagrams (bytes each) -> (slots uint8 [P][stride], lengths int32 [P]); stride None: the longest, rounded up to a multiple of 4
    (at least 12)"""
    lengths = np.asarray([len(p) for p in packets], np.int32)
    if stride is None:
        stride = max(12, (int(lengths.max()) + 3) & ~3) if len(packets) else 12
    slots = np.zeros((len(packets), int(stride)), np.uint8)
    for i, p in enumerate(packets):
        slots[i, :len(p)] = np.frombuffer(p, np.uint8)
    return slots, lengths
