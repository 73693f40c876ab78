"""Test traffic for the RTP reorder window (tests/test_rtp_window_cpu.py, tests/test_gpu_rtp_window.py): a timeline of samples per
stream cut into packets, and arrival schedules that say in which tick a receiver submits each of them."""
import numpy as np

import rtp_model as rm

EXTREMES = {2: [-0x8000, 0x7FFF, -1, 0, 1, 0x0102, -0x0102], 3: [-0x800000, 0x7FFFFF, -1, 0, 1, 0x010203, -0x010203]}


def samples(rng, rows, n, B, scale=1):
    """integer samples [rows][n] over the range of B bytes (divided by scale), the extremes in every row at another place"""
    x = rng.integers(-(1 << (8 * B - 1)), 1 << (8 * B - 1), (rows, n), dtype=np.int64)
    for k, v in enumerate(EXTREMES[B][:n]):
        x[:, k] = v
    return np.stack([np.roll(r, i) for i, r in enumerate(x)]) // scale


def packets_of(rtp, x, chans, per_packet, first, B):
    """the timeline x [sum(chans)][L] as packets, stream s in packets of per_packet[s] sample times from RTP time first[s]
    -> (slots, lengths, stream_of, position, sample_times): position[i] = packet i's first sample time, counted from first[s]"""
    parts, row = [], 0
    for s, K in enumerate(chans):
        slots, lengths, _ = rtp.packetise(x[row:row + K], [K], per_packet[s], [first[s]], bytes_per_sample=B)
        row += K
        m = (lengths - 12) // (K * B)
        parts.append((slots, lengths, np.full(len(lengths), s, np.int32), np.arange(len(lengths), dtype=np.int64) * per_packet[s], m.astype(np.int64)))
    width = max(p[0].shape[1] for p in parts)
    slots = np.concatenate([np.pad(p[0], ((0, 0), (0, width - p[0].shape[1]))) for p in parts])
    return (slots,) + tuple(np.concatenate([p[k] for p in parts]) for k in range(1, 5))


def tick_of(position, ticks):
    """the tick (index into `ticks`, the ticks' lengths) that holds sample time `position`; beyond the last tick: len(ticks)"""
    return np.searchsorted(np.cumsum(ticks), np.asarray(position, np.int64), side="right")


def whole_in_span(position, m, arrival, ticks, W):
    """True where packet i, submitted in tick arrival[i], lies whole in that tick's span of ticks[k] + W positions"""
    start = np.concatenate([[0], np.cumsum(ticks)])[arrival]
    return (position >= start) & (position + m <= start + np.asarray(ticks, np.int64)[arrival] + W)


def submit(packets, arrival, k, order=None):
    """tick k's packets of (slots, lengths, stream_of, ...) under the schedule `arrival`, in list order or permuted by `order`"""
    idx = np.flatnonzero(np.asarray(arrival) == k)
    if order is not None:
        idx = idx[order(len(idx))]
    return packets[0][idx], packets[1][idx], packets[2][idx]


def resubmitting(model, slots, lengths, stream_of, n, carried):
    """a tick of an rtp_model.Model (no window) the way a receiver without one has to do it: the packets that were EARLY in the
    tick before, in their order, in front of this tick's own -> (block, disposition of all, the packets to carry on)"""
    if carried is not None and len(carried[1]):
        width = max(slots.shape[1], carried[0].shape[1])
        pad = lambda a: np.pad(a, ((0, 0), (0, width - a.shape[1])))
        slots, lengths, stream_of = np.concatenate([pad(carried[0]), pad(slots)]), np.concatenate([carried[1], lengths]), np.concatenate([carried[2], stream_of])
    block, disposition = model.tick(slots, lengths, stream_of, n)
    early = (disposition & rm.EARLY) != 0
    return block, disposition, (slots[early], lengths[early], stream_of[early])
