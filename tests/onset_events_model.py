"""The contract of the onset event list (include/fx.h, fx_enable_onset_events / fx_get_onset_events) as plain Python: what the list
holds after a sequence of analysis calls, drains, resets and resizes, given only each call's 0/1 onset flags.  No arithmetic of the
analysers is in here: the flags of a call are raw[:, :, ONSET] == 1 of that call, wherever they come from (the GPU's own output, the
oracle's).  tests/test_onset_events_cpu.py holds the model to hand-written cases; tests/test_gpu_onset_events.py holds the library
to the model."""
import numpy as np

EVENT_DTYPE = np.dtype([("frame", np.int64), ("channel", np.int32), ("call_frame", np.int32)])
MAX_CAPACITY = 1 << 26


def events_of_call(flags, frames_before=0):
    """[(frame, channel, call_frame)] of one call: flags [C][T] (anything whose == 1 marks an onset), in the list's order --
    ascending frame, then ascending channel."""
    on = np.asarray(flags) == 1
    assert on.ndim == 2
    t, c = np.nonzero(on.T)                          # row-major over [T][C]: frame by frame, channels ascending
    return [(frames_before + int(ti), int(ci), int(ti)) for ti, ci in zip(t, c)]


def as_array(events):
    a = np.empty(len(events), EVENT_DTYPE)
    for i, (f, c, t) in enumerate(events):
        a[i] = (f, c, t)
    return a


def as_tuples(events):
    """a structured array (BatchAnalyser.onset_events) as the model's list of tuples"""
    return [(int(e["frame"]), int(e["channel"]), int(e["call_frame"])) for e in events]


class EventList:
    """The list of one context.  capacity 0: disabled (calls append nothing, drain is an error)."""

    def __init__(self, capacity=0):
        self.capacity = 0
        self.stored = []
        self.dropped = 0
        self.frames_seen = 0            # the context's, kept whether the list is enabled or not
        if capacity:
            self.enable(capacity)

    def enable(self, capacity):
        """capacity > 0: allocate / resize, dropping what is stored (and the overflow count with it); 0: disable"""
        if capacity < 0 or capacity > MAX_CAPACITY:
            raise ValueError("capacity")
        self.capacity = capacity
        self.stored = []
        self.dropped = 0

    def call(self, flags):
        """one analysis call over flags [C][T]"""
        flags = np.asarray(flags)
        ev = events_of_call(flags, self.frames_seen)
        self.frames_seen += flags.shape[1]
        if not self.capacity:
            return
        room = self.capacity - len(self.stored)
        self.stored += ev[:room]                      # the earliest are kept
        self.dropped += max(0, len(ev) - room)

    def count(self):
        """out == NULL, cap == 0: how many are stored; nothing removed, nothing cleared"""
        if not self.capacity:
            raise ValueError("not enabled")
        return len(self.stored)

    def drain(self, cap=None):
        """(events, dropped): the min(stored, cap) oldest leave the list, the rest stay; the overflow count starts again"""
        if not self.capacity:
            raise ValueError("not enabled")
        if cap is not None and cap < 0:
            raise ValueError("cap")
        n = len(self.stored) if cap is None else min(cap, len(self.stored))
        out, self.stored = self.stored[:n], self.stored[n:]
        dropped, self.dropped = self.dropped, 0
        return out, dropped

    def reset(self):
        """fx_reset_state: an empty list, nothing dropped, frames count from 0; still enabled, same capacity"""
        self.stored = []
        self.dropped = 0
        self.frames_seen = 0


def simulate(calls, capacity, drains):
    """calls: a list of [C][T] 0/1 matrices; drains: {index of a call: cap or None} -- a drain after that call.
    -> [(events, dropped)] of the drains, in order."""
    lst = EventList(capacity)
    out = []
    for i, flags in enumerate(calls):
        lst.call(flags)
        if i in drains:
            out.append(lst.drain(drains[i]))
    return out
