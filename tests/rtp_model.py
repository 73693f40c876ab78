"""fx_push_rtp's definition of a tick (include/fx.h, "RTP audio in") restated in numpy and plain Python: what is malformed, where a
packet lands, who owns a position, the block's bytes, the disposition bits, the statistics and the cursors.  The tests hold the
library (tests/test_gpu_rtp.py) and the parser of csrc/fx_rtp_packet.h (tests/test_rtp_cpu.py, through tests/cpp/rtp_packet_host.cpp)
to this file."""
import numpy as np

PLACED, LATE, EARLY, MALFORMED, IGNORED = 1, 2, 4, 8, 16
STATS = ["packets", "malformed", "late_packets", "early_packets", "samples_placed", "samples_missing"]


def parse(b, frame_bytes):
    """datagram b (bytes) of a stream whose sample time is frame_bytes bytes -> None (malformed) or (T, payload offset h, sample
    times m).  Indexing `b` raises IndexError beyond its length: the definition never asks for such a byte."""
    b = bytes(b)
    n = len(b)
    if n < 12 or b[0] >> 6 != 2:
        return None
    P, X, CC = (b[0] >> 5) & 1, (b[0] >> 4) & 1, b[0] & 15
    h = 12 + 4 * CC
    if X:
        if h + 4 > n:
            return None
        h += 4 + 4 * ((b[h + 2] << 8) | b[h + 3])
    if h > n:
        return None
    pad = b[n - 1] if P else 0
    if P and (pad == 0 or h + pad > n):
        return None
    payload = n - h - pad
    if payload <= 0 or payload % frame_bytes:
        return None
    return int.from_bytes(b[4:8], "big"), h, payload // frame_bytes


def signed32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def place(T, cursor, m, n):
    """-> (d0, lo, hi, bits): the packet covers tick positions [lo, hi) (empty unless PLACED)"""
    d0 = signed32(T - cursor)
    lo, hi = max(d0, 0), min(d0 + m, n)
    bits = (LATE if d0 < 0 else 0) | (EARLY if d0 + m > n else 0) | (PLACED if lo < hi else 0)
    return d0, lo, hi, bits


class Model:
    """the unit's whole state: configure = the constructor"""

    def __init__(self, bytes_per_sample, channels_per_stream, num_tracks):
        self.B = int(bytes_per_sample)
        self.channels = [int(k) for k in channels_per_stream]
        self.C = int(num_tracks)
        S = len(self.channels)
        self.stream = np.full(self.C, -1, np.int64)
        self.channel = np.zeros(self.C, np.int64)
        self.cursor = [0] * S
        self.running = [False] * S
        self.stats = np.zeros((S, len(STATS)), np.int64)

    def set_sources(self, tracks, stream, channel):
        for t, s, j in zip(tracks, stream, channel):            # in order: of a track listed twice the last entry wins
            self.stream[t], self.channel[t] = (-1, 0) if s in (-1, None) else (s, j)

    def set_timestamps(self, streams, timestamps):
        for s, t in zip(streams, timestamps):
            self.cursor[s], self.running[s] = int(t) & 0xFFFFFFFF, True

    def tick(self, slots, lengths, stream_of, n):
        """-> (block uint8 [C][n * B], disposition uint8 [P])"""
        B, S = self.B, len(self.channels)
        heard = [np.zeros((n, K, B), np.uint8) for K in self.channels]      # per stream: the bytes on the wire of every owned position
        owned = np.zeros((S, n), bool)
        disposition = np.zeros(len(lengths), np.uint8)
        for i in range(len(lengths)):                       # in index order, each writing over the ones before: the greatest index owns
            s, K = int(stream_of[i]), self.channels[int(stream_of[i])]
            b = bytes(np.asarray(slots[i], np.uint8)[:int(lengths[i])])
            got = parse(b, K * B)
            if got is None:
                disposition[i] = MALFORMED
                self.stats[s, 1] += 1
                continue
            self.stats[s, 0] += 1
            if not self.running[s]:
                disposition[i] = IGNORED
                continue
            T, h, m = got
            d0, lo, hi, bits = place(T, self.cursor[s], m, n)
            disposition[i] = bits
            if not bits & PLACED:
                self.stats[s, 2] += 1 if bits & LATE else 0
                self.stats[s, 3] += 1 if bits & EARLY else 0
                continue
            payload = np.frombuffer(b, np.uint8, m * K * B, h).reshape(m, K, B)
            heard[s][lo:hi] = payload[lo - d0:hi - d0]
            owned[s, lo:hi] = True
        block = np.zeros((self.C, n, B), np.uint8)
        for c in range(self.C):
            s, j = int(self.stream[c]), int(self.channel[c])
            if s >= 0 and self.running[s]:
                block[c] = heard[s][:, j, ::-1]             # big endian on the wire, little endian in the block
        for s in range(S):
            if self.running[s]:
                self.stats[s, 4] += int(owned[s].sum())
                self.stats[s, 5] += n - int(owned[s].sum())
                self.cursor[s] = (self.cursor[s] + n) & 0xFFFFFFFF
        return block.reshape(self.C, n * B), disposition

    def stats_dict(self):
        return {name: self.stats[:, k].copy() for k, name in enumerate(STATS)}


def little_endian_bytes(planar_int, bytes_per_sample):
    """integer samples [C][n] -> uint8 [C][n * B]: the planar block fx_push_samples takes in s16 / s24"""
    v = np.asarray(planar_int).astype(np.int64)
    shifts = 8 * np.arange(bytes_per_sample, dtype=np.int64)
    return ((v[..., None] >> shifts) & 0xFF).astype(np.uint8).reshape(v.shape[0], -1)
