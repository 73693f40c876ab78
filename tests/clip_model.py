"""Host model of file sources (include/fx.h, fx_create_clips .. fx_push_sources) over raw sample bytes: every track's player (source,
state, loop, clip, position, laps), what each command makes of it and which tracks' pending samples it zeroes, and the planar block
[C][n] a tick forms -- what fx_push_samples is given in the twin runs of tests/test_gpu_clips.py.  render() is the vectorised statement
of a tick for one track; render_naive() is the same sample by sample, the definition render() is held to (tests/test_clips_cpu.py)."""
import numpy as np

FORMATS = ("f32", "f16", "s16", "s24")
BYTES = {"f32": 4, "f16": 2, "s16": 2, "s24": 3}
DTYPES = {"f32": np.float32, "f16": np.float16, "s16": np.int16, "s24": np.uint8}
INPUT, FILE = 0, 1
NO_FILE, PLAYING, PAUSED, STOPPED, FINISHED = range(5)
PLAY, PAUSE, STOP, RESTART = range(4)


def raw(x):
    """the bytes of an encoded array, row by row: [..][n] of a dtype -> uint8 [..][n * itemsize]"""
    x = np.ascontiguousarray(x)
    return x.view(np.uint8).reshape(x.shape[:-1] + (x.shape[-1] * x.itemsize,))


def typed(block, fmt):
    """uint8 [C][n * B] -> the array push_samples takes for `fmt` (s24: the bytes, to be passed with sample_format="s24")"""
    block = np.ascontiguousarray(block)
    return block if fmt == "s24" else block.view(DTYPES[fmt])


class Player:
    def __init__(self):
        self.source, self.state, self.loop = INPUT, NO_FILE, 1
        self.clip, self.L, self.position, self.laps = None, 0, 0, 0

    def copy(self):
        p = Player()
        p.__dict__.update(self.__dict__)
        return p


def render(p, n, B):
    """a FILE track's tick: (uint8 [n * B], position, laps, state) after it"""
    out = np.zeros(n * B, np.uint8)
    if p.state != PLAYING:
        return out, p.position, p.laps, p.state
    if p.loop:
        idx = (p.position + np.arange(n, dtype=np.int64)) % p.L
        out = p.clip.reshape(p.L, B)[idx].reshape(-1)
        t = p.position + n
        return out, t % p.L, p.laps + t // p.L, PLAYING
    have = min(n, p.L - p.position)
    out[:have * B] = p.clip[p.position * B:(p.position + have) * B]
    return out, min(p.position + n, p.L), p.laps, FINISHED if p.position + n >= p.L else PLAYING


def render_naive(p, n, B):
    """the same, one sample and one byte at a time"""
    out = bytearray(n * B)
    position, laps, state = p.position, p.laps, p.state
    if state != PLAYING:
        return np.frombuffer(bytes(out), np.uint8), position, laps, state
    for i in range(n):
        if p.loop:
            for b in range(B):
                out[i * B + b] = int(p.clip[position * B + b])
            position += 1
            if position == p.L:
                position, laps = 0, laps + 1
        else:
            if position < p.L:
                for b in range(B):
                    out[i * B + b] = int(p.clip[position * B + b])
                position += 1
            if position == p.L:
                state = FINISHED
    return np.frombuffer(bytes(out), np.uint8), position, laps, state


class Refused(Exception):
    """a command the library refuses: nothing has changed"""


class Model:
    """C players.  Every command returns the tracks whose pending samples it zeroes (the twin's clear_pending_channels)."""

    def __init__(self, C, fmt):
        self.C, self.fmt, self.B = C, fmt, BYTES[fmt]
        self.players = [Player() for _ in range(C)]

    def _check(self, channels):
        for i, c in enumerate(channels):
            if not 0 <= c < self.C:
                raise Refused("entry %d" % i)

    @staticmethod
    def _last(channels):
        """(entry, track) with one entry per track, its last one: the two setters' rule for duplicates"""
        last = {c: i for i, c in enumerate(channels)}
        return [(i, c) for i, c in enumerate(channels) if last[c] == i]

    def load(self, channels, clips, loop=None):
        """clips[i]: uint8 bytes of the clip, or None for no file"""
        self._check(channels)
        for i, c in self._last(channels):
            p = self.players[c]
            clip = clips[i]
            p.clip = None if clip is None else np.ascontiguousarray(clip, np.uint8).reshape(-1)
            p.L = 0 if clip is None else p.clip.size // self.B
            p.loop = 1 if loop is None else int(bool(loop[i]))
            p.state, p.position, p.laps = (NO_FILE if clip is None else STOPPED), 0, 0
        return list(channels)

    def set_sources(self, channels, types):
        self._check(channels)
        for t in types:
            if t not in (INPUT, FILE):
                raise Refused("source")
        for i, c in self._last(channels):
            p, t = self.players[c], types[i]
            p.source = t
            if t == INPUT:
                p.state, p.position = (STOPPED if p.clip is not None else NO_FILE), 0
        return list(channels)

    def transport(self, channels, command):
        self._check(channels)
        if command not in (PLAY, PAUSE, STOP, RESTART):
            raise Refused("command")
        if command == PLAY and any(self.players[c].clip is None for c in channels):
            raise Refused("no file")
        for c in channels:
            p = self.players[c]
            if command == PLAY:
                if p.state == FINISHED:
                    p.position = 0
                p.state = PLAYING
            elif command == PAUSE:
                if p.state == PLAYING:
                    p.state = PAUSED
            elif command == STOP:
                if p.clip is not None:
                    p.state, p.position = STOPPED, 0
            else:
                p.position = 0
                if p.state == FINISHED:
                    p.state = STOPPED
        return [] if command == RESTART else list(channels)

    def tick(self, live, n, naive=False):
        """live: uint8 [C][n * B] or None -> the planar block uint8 [C][n * B]; FILE tracks that play move on"""
        if live is None and any(p.source == INPUT for p in self.players):
            raise Refused("null live block")
        out = np.zeros((self.C, n * self.B), np.uint8)
        for c, p in enumerate(self.players):
            if p.source == INPUT:
                out[c] = live[c]
            else:
                out[c], p.position, p.laps, p.state = (render_naive if naive else render)(p, n, self.B)
        return out

    def table(self):
        return {"source": np.array([p.source for p in self.players], np.int32), "state": np.array([p.state for p in self.players], np.int32),
                "position": np.array([p.position for p in self.players], np.int64), "laps": np.array([p.laps for p in self.players], np.int64)}
