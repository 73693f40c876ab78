"""The RTP reorder window's definition (include/fx.h, "the RTP reorder window") restated in numpy and plain Python on top of
tests/rtp_model.py: a tick works on a span of n + W positions, the first W of which carry what the unit holds from earlier ticks;
the most recently submitted packet owns a position; positions [n, n + W) are the held state of the next tick.  The tests hold the
library (tests/test_gpu_rtp_window.py) and fx_rtp_place_span of csrc/fx_rtp_packet.h (tests/test_rtp_window_cpu.py, through
tests/cpp/rtp_window_host.cpp) to this file."""
import numpy as np

import rtp_model as rm
from rtp_model import EARLY, IGNORED, LATE, MALFORMED, PLACED, STATS  # noqa: F401

HELD = 32
MAX_WINDOW = 65536
WINDOW_STATS = ["held", "recovered"]


def place(T, cursor, m, n, W):
    """-> (d0, lo, hi, bits): the packet covers span positions [lo, hi) of [0, n + W) (empty unless PLACED or HELD)"""
    d0 = rm.signed32(T - cursor)
    lo, hi = max(d0, 0), min(d0 + m, n + W)
    inside = lo < hi
    bits = (LATE if d0 < 0 else 0) | (EARLY if d0 + m > n + W else 0) | (PLACED if inside and lo < n else 0) | (HELD if inside and hi > n else 0)
    return (d0, lo, hi, bits) if inside else (d0, 0, 0, bits)


class Model(rm.Model):
    """rtp_model.Model and the held state: configure = the constructor, W = 0 and nothing held"""

    def __init__(self, bytes_per_sample, channels_per_stream, num_tracks):
        super().__init__(bytes_per_sample, channels_per_stream, num_tracks)
        self.set_window(0)

    def set_window(self, W):
        W = int(W)
        if not 0 <= W <= MAX_WINDOW:
            raise ValueError("window %d" % W)
        self.W = W
        self.held_bytes = [np.zeros((W, K, self.B), np.uint8) for K in self.channels]       # per stream: the wire bytes of the held positions
        self.held_owned = np.zeros((len(self.channels), W), bool)
        self.recovered = np.zeros(len(self.channels), np.int64)

    def set_timestamps(self, streams, timestamps):
        super().set_timestamps(streams, timestamps)
        for s in streams:                                   # the listed streams' time base has moved
            self.held_owned[s] = False

    def tick(self, slots, lengths, stream_of, n):
        """-> (block uint8 [C][n * B], disposition uint8 [P])"""
        B, S, W = self.B, len(self.channels), self.W
        if n == 0:
            return np.zeros((self.C, 0), np.uint8), np.zeros(len(lengths), np.uint8)
        span = [np.concatenate([self.held_bytes[s], np.zeros((n, K, B), np.uint8)]) for s, K in enumerate(self.channels)]
        owned = np.concatenate([self.held_owned, np.zeros((S, n), bool)], axis=1)
        fresh = np.zeros((S, n + W), bool)                  # owned by a packet of this tick
        disposition = np.zeros(len(lengths), np.uint8)
        for i in range(len(lengths)):                       # in index order, each writing over the ones before and over what was held
            s, K = int(stream_of[i]), self.channels[int(stream_of[i])]
            b = bytes(np.asarray(slots[i], np.uint8)[:int(lengths[i])])
            got = rm.parse(b, K * B)
            if got is None:
                disposition[i] = MALFORMED
                self.stats[s, 1] += 1
                continue
            self.stats[s, 0] += 1
            if not self.running[s]:
                disposition[i] = IGNORED
                continue
            T, h, m = got
            d0, lo, hi, bits = place(T, self.cursor[s], m, n, W)
            disposition[i] = bits
            if not bits & (PLACED | HELD):
                self.stats[s, 2] += 1 if bits & LATE else 0
                self.stats[s, 3] += 1 if bits & EARLY else 0
                continue
            payload = np.frombuffer(b, np.uint8, m * K * B, h).reshape(m, K, B)
            span[s][lo:hi] = payload[lo - d0:hi - d0]
            owned[s, lo:hi] = True
            fresh[s, lo:hi] = True
        block = np.zeros((self.C, n, B), np.uint8)
        for c in range(self.C):
            s, j = int(self.stream[c]), int(self.channel[c])
            if s >= 0 and self.running[s]:
                block[c] = np.where(owned[s, :n, None], span[s][:n, j, ::-1], 0)
        for s in range(S):
            if self.running[s]:
                self.stats[s, 4] += int(owned[s, :n].sum())
                self.stats[s, 5] += n - int(owned[s, :n].sum())
                self.recovered[s] += int((owned[s, :n] & ~fresh[s, :n]).sum())
                self.cursor[s] = (self.cursor[s] + n) & 0xFFFFFFFF
                self.held_bytes[s] = span[s][n:].copy()
                self.held_owned[s] = owned[s, n:]
        return block.reshape(self.C, n * B), disposition

    def window_dict(self):
        return {"window": self.W, "held": self.held_owned.sum(axis=1).astype(np.int64), "recovered": self.recovered.copy()}
