"""Host model of clips at their own sample rate (include/fx.h, "CLIPS AT THEIR OWN RATE"): the resampler's specification restated in
numpy, one IEEE operation at a time in the stated type (float64 and float32 arrays; numpy fuses nothing).  The table is an argument:
the tests hand in the library's own (fx_get_resampler_table), and table_formula() is the formula it is held to.  render() is a
tick of one rated track vectorised over its outputs; render_naive() the same sample by sample and tap by tap, the definition
render() is held to (tests/test_resample_cpu.py).  Model extends clip_model.Model with rated players: a context whose ticks are fp32,
whose unrated clips are fp32 and whose rated clips are in any format -- the planar fp32 block of a tick is what the twin run of
tests/test_gpu_resample.py is given."""
import math

import numpy as np

import clip_model as cm
from clip_model import FILE, FINISHED, INPUT, PAUSE, PLAY, PLAYING, RESTART, STOP, Refused  # noqa: F401  (the tests speak these)

Z, P, BETA = 16, 512, 9.0
TABLE_SIZE = Z * P + 2


def table_formula():
    """T[i] = fl32(sinc(i/P) * I0(beta * sqrt(1 - (i/(P*Z))^2)) / I0(beta)) for i < Z*P, then two zeros"""
    i = np.arange(Z * P, dtype=np.float64)
    t = np.sinc(i / P) * np.i0(BETA * np.sqrt(1.0 - (i / (P * Z)) ** 2)) / np.i0(BETA)
    return np.concatenate([t.astype(np.float32), np.zeros(2, np.float32)])


def widen(clip, fmt):
    """the bytes of a clip (uint8) -> its samples as the load stage widens them, float32 [L]"""
    b = np.ascontiguousarray(clip, np.uint8).reshape(-1)
    if fmt == "f32":
        return b.view(np.float32).copy()
    if fmt == "f16":
        return b.view(np.float16).astype(np.float32)
    if fmt == "s16":
        return b.view(np.int16).astype(np.float32) * np.float32(1.0 / 32768.0)
    t = b.reshape(-1, 3).astype(np.uint32)
    left = ((t[:, 0] << 8) | (t[:, 1] << 16) | (t[:, 2] << 24)).astype(np.uint32).view(np.int32)
    return left.astype(np.float32) * np.float32(1.0 / 2147483648.0)


def rate_params(clip_rate, context_rate):
    """(r, rho, J) of a rated load in fp64 as the host forms them; None for a clip that is not rated; Refused outside [1/8, 8]"""
    clip_rate, context_rate = float(clip_rate), float(context_rate)
    if clip_rate == 0.0 or clip_rate == context_rate:
        return None
    r = clip_rate / context_rate
    if not 0.125 <= r <= 8.0:
        raise Refused("ratio %r" % r)
    rho = min(1.0, 1.0 / r)
    return r, rho, int(math.ceil(Z / rho))


def rated_player(samples, r, rho, J, loop=1, k=0):
    """a FILE track that plays `samples` (float32 [L]) at ratio r"""
    p = cm.Player()
    p.source, p.state, p.loop = FILE, PLAYING, int(bool(loop))
    p.samples, p.L, p.r, p.rho, p.J, p.k, p.rated = np.asarray(samples, np.float32), len(samples), float(r), float(rho), int(J), int(k), True
    return p


def _after(p, n):
    """(position, laps, state, k) after n more outputs of a playing rated track"""
    k = p.k + n
    x = np.float64(k) * np.float64(p.r)
    whole = int(np.floor(x))
    if p.loop:
        return whole % p.L, whole // p.L, PLAYING, k
    return min(whole, p.L), p.laps, (FINISHED if x >= p.L else PLAYING), k


def render(p, n, T):
    """a rated FILE track's tick: (float32 [n], position, laps, state, k) after it"""
    if p.state != PLAYING:
        return np.zeros(n, np.float32), p.position, p.laps, p.state, p.k
    T = np.asarray(T, np.float32)
    r, rho, L = np.float64(p.r), np.float64(p.rho), p.L
    x = (p.k + np.arange(n, dtype=np.int64)).astype(np.float64) * r
    whole = np.floor(x)
    f = x - whole
    i0 = whole.astype(np.int64)
    acc = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        # every tap's product at once, [taps][n] (elementwise operations: each is the scalar one); the sum runs over the taps in order
        j = np.arange(-(p.J - 1), p.J + 1, dtype=np.int64)[:, None]
        a = np.abs(j.astype(np.float64) - f[None, :]) * rho
        add = a < Z
        q = a * np.float64(P)
        qi = np.floor(q)
        t = (q - qi).astype(np.float32)
        i = np.where(add, qi, 0.0).astype(np.int64)
        c = T[i] + t * (T[i + 1] - T[i])
        m = i0[None, :] + j
        if p.loop:
            s = p.samples[m % L]
        else:
            add = add & (m >= 0) & (m < L)
            s = p.samples[np.clip(m, 0, L - 1)]
        product = c * s
        assert product.dtype == np.float32
        for tap in range(product.shape[0]):
            acc = np.where(add[tap], acc + product[tap], acc)
        out = acc * np.float32(rho)
    if not p.loop:
        out = np.where(x >= L, np.float32(0.0), out)
    return (out.astype(np.float32),) + _after(p, n)


def render_naive(p, n, T):
    """the same, one output and one tap at a time"""
    if p.state != PLAYING:
        return np.zeros(n, np.float32), p.position, p.laps, p.state, p.k
    out = np.zeros(n, np.float32)
    r, rho, L = np.float64(p.r), np.float64(p.rho), p.L
    with np.errstate(all="ignore"):
        for n_i in range(n):
            x = np.float64(p.k + n_i) * r
            i0 = int(math.floor(x))
            f = x - np.float64(i0)
            acc = np.float32(0.0)
            for j in range(-(p.J - 1), p.J + 1):
                a = abs(np.float64(j) - f) * rho
                if a >= Z:
                    continue
                q = a * np.float64(P)
                i = int(math.floor(q))
                t = np.float32(q - np.float64(i))
                c = np.float32(T[i]) + t * (np.float32(T[i + 1]) - np.float32(T[i]))
                m = i0 + j
                if p.loop:
                    s = np.float32(p.samples[m % L])
                elif 0 <= m < L:
                    s = np.float32(p.samples[m])
                else:
                    continue
                acc = np.float32(acc + np.float32(c * s))
            o = np.float32(acc * np.float32(rho))
            if not p.loop and x >= L:
                o = np.float32(0.0)
            out[n_i] = o
    return (out,) + _after(p, n)


class Model(cm.Model):
    """C players of a context whose ticks are fp32.  load() takes each clip's format and rate; a clip whose rate is neither 0 nor the
    context's makes its track rated.  Every command returns the tracks whose pending samples it zeroes, as clip_model.Model does."""

    def __init__(self, C, table, sample_rate=48000.0):
        super().__init__(C, "f32")
        self.T, self.sample_rate = np.asarray(table, np.float32), float(sample_rate)
        for p in self.players:
            p.rated, p.k = False, 0

    def load(self, channels, clips, loop=None, fmts=None, rates=None):
        """clips[i]: uint8 bytes or None; fmts[i]: its format ("f32" if not given); rates[i]: its rate in Hz (0: the context's)"""
        self._check(channels)
        fmts = ["f32"] * len(channels) if fmts is None else fmts
        rates = [0.0] * len(channels) if rates is None else rates
        params = [None if clips[i] is None else rate_params(rates[i], self.sample_rate) for i in range(len(channels))]   # Refused: nothing changed
        cleared = super().load(channels, clips, loop)
        for i, c in self._last(channels):
            p = self.players[c]
            p.rated, p.k, p.fmt = params[i] is not None, 0, fmts[i]
            if p.rated:
                p.r, p.rho, p.J = params[i]
                p.samples = widen(p.clip, fmts[i])
                p.L = p.samples.size
            elif p.clip is not None:
                assert fmts[i] == "f32", "an unrated clip is in the tick's format"
        return cleared

    def set_sources(self, channels, types):
        cleared = super().set_sources(channels, types)
        for i, c in self._last(channels):
            if types[i] == INPUT:
                self.players[c].k = 0
        return cleared

    def transport(self, channels, command):
        self._check(channels)
        before = [self.players[c].state for c in channels]
        cleared = super().transport(channels, command)
        for c, state in zip(channels, before):
            p = self.players[c]
            if command == RESTART or (command == STOP and p.clip is not None) or (command == PLAY and state == FINISHED):
                p.k = 0
        return cleared

    def tick(self, live, n, naive=False):
        """live: float32 [C][n] or None -> the planar block float32 [C][n]; FILE tracks that play move on"""
        if live is None and any(p.source == INPUT for p in self.players):
            raise Refused("null live block")
        out = np.zeros((self.C, n), np.float32)
        for c, p in enumerate(self.players):
            if p.source == INPUT:
                out[c] = live[c]
            elif p.rated:
                out[c], p.position, p.laps, p.state, p.k = (render_naive if naive else render)(p, n, self.T)
            else:
                raw, p.position, p.laps, p.state = cm.render(p, n, 4)
                out[c] = raw.view(np.float32)
        return out
