"""An exact model of the reference's TAIL: what its AudioFeatures and OnsetDetector make of the values the two analysers
write.  Input: the raw stream [C][T][12] in frame order (what each frame passed to updateFeature), an event timeline and the
order mode / analysers.  Output: the smoothed vectors [C][T][12] (getValue of every slot after the frame) and the onset
column, bit for bit.

The model simulates the reference's objects one by one, in fp32 numpy vectors over the channels, every sum strictly left to
right.  It is written from the reference's headers (citations as "ref:", relative to the reference's Source/ directory), not
from the kernels' ring arithmetic: it keeps each history as the reference keeps it, a shifted vector of `length` floats and
a recordedHistory count.  Sample rate and gain change no tail value, so events that set them are accepted and ignored.

Events are (frame, name[, value]): the event runs before frame `frame` is written.  Names: "onset_type", "onset_window",
"sensitivity", "reset", and the no-ops "gain", "sample_rate"."""
import numpy as np

ONSET, RMS, F0, CENTROID, SPREAD, FLATNESS, LER, FLUX, SLOPE, HER, OER, INHARM = range(12)
NUM_FEATURES = 12
ONSET_SPECTRAL, ONSET_AMPLITUDE, ONSET_COMBINATION = 0, 1, 2
SPECTRAL_THEN_HARMONIC, HARMONIC_THEN_SPECTRAL, ISOLATED = 0, 1, 2

_F = np.float32


class ValueHistory:
    """ref: RealTimeAudioAnalysis.h:40-96, one per channel, side by side"""

    def __init__(self, C, length):
        self.C = C
        self.set_length(length)

    def set_length(self, length):                   # ref :73-81 -- recordedHistory = 0, `length` zeros
        self.h = np.zeros((self.C, int(length)), _F)
        self.recorded = 0

    def total(self):                                # ref :49-57 -- float total, added from index 0 up
        t = np.zeros(self.C, _F)
        for i in range(self.h.shape[1]):
            t = (t + self.h[:, i]).astype(_F)
        return t

    def insert(self, v):                            # ref :59-71 -- shift down by one, newest at the end
        n = self.h.shape[1]
        for i in range(n - 1):
            self.h[:, i] = self.h[:, i + 1]
        self.h[:, n - 1] = v
        if self.recorded < n:
            self.recorded += 1


class AudioFeatures:
    """ref: RealTimeAnalyser.h:70-88"""

    def __init__(self, C):
        self.hist = [ValueHistory(C, 1 if f in (ONSET, FLUX) else 10) for f in range(NUM_FEATURES)]   # ref :70-74

    def update(self, f, v):                         # ref :76-82
        self.hist[f].insert(v)

    def value(self, f):                             # ref :84-88 -- float total / int recordedHistory; 0/0 = NaN before any insert
        h = self.hist[f]
        with np.errstate(invalid="ignore", divide="ignore"):
            return (h.total() / _F(h.recorded)).astype(_F)


class OnsetDetector:
    """ref: SpectralCharacteristics.h:210-312"""

    def __init__(self, C):
        self.flux = ValueHistory(C, 5)              # ref :238-241
        self.amp = ValueHistory(C, 5)
        self.type = ONSET_AMPLITUDE
        self.multiplier = _F(1.7)                   # ref :311
        self.candidates = []                        # (candidate amplitude, channels that reached the 0.01 gate) per detection

    def add(self, sf, amp):                         # ref :243-247
        self.flux.insert(sf)
        self.amp.insert(amp)

    def detect(self):                               # ref :249-306
        sf, am = self.flux, self.amp
        n = sf.h.shape[1]
        C = sf.C
        if am.recorded == 0 or sf.recorded == 0:
            return np.zeros(C, bool)
        if sf.recorded < n or am.recorded < n:
            return np.zeros(C, bool)
        mean_sf = (sf.total() / _F(sf.recorded)).astype(_F)
        mean_amp = (am.total() / _F(am.recorded)).astype(_F)
        cand = n // 2 if self.type in (ONSET_SPECTRAL, ONSET_COMBINATION) else n - 1
        cand_sf = sf.h[:, cand]
        cand_amp = am.h[:, cand]
        self.candidates.append(cand_amp.copy())
        alive = ~(cand_amp < _F(0.01))
        for i in range(n):
            if i == cand:
                continue
            if self.type in (ONSET_AMPLITUDE, ONSET_COMBINATION):
                alive &= ~(am.h[:, i] >= cand_amp)
            if self.type in (ONSET_SPECTRAL, ONSET_COMBINATION):
                alive &= ~(sf.h[:, i] >= cand_sf)
        on_sf = cand_sf > (mean_sf * self.multiplier).astype(_F)
        on_amp = cand_amp > (mean_amp * self.multiplier).astype(_F)
        if self.type == ONSET_AMPLITUDE:
            return alive & on_amp
        if self.type == ONSET_SPECTRAL:
            return alive & on_sf
        if self.type == ONSET_COMBINATION:
            return alive & on_amp & on_sf
        return np.zeros(C, bool)


class Tail:
    """One context's tail: the shared AudioFeatures (two when isolated) and the spectral analyser's OnsetDetector"""

    def __init__(self, C, order=SPECTRAL_THEN_HARMONIC, analysers=3):
        self.C, self.order, self.analysers = C, int(order), int(analysers)
        self.detector = OnsetDetector(C)
        self._fresh_features()

    def _fresh_features(self):
        self.fs = AudioFeatures(self.C)
        self.fh = AudioFeatures(self.C) if self.order == ISOLATED else self.fs

    def event(self, name, value=None):
        if name == "onset_type":                    # ref RealTimeAnalyser.h:258
            self.detector.type = int(value)
        elif name == "sensitivity":                 # ref RealTimeAnalyser.h:244-248
            self.detector.multiplier = _F(_F(1.0) + _F(value))
        elif name == "onset_window":                # ref RealTimeAnalyser.h:250-254 -- both onset histories, no feature history
            self.detector.amp.set_length(value)
            self.detector.flux.set_length(value)
        elif name == "reset":                       # a fresh track: every history empty, the detector's settings kept
            self._fresh_features()
            n = self.detector.flux.h.shape[1]
            self.detector.amp.set_length(n)
            self.detector.flux.set_length(n)
        elif name not in ("gain", "sample_rate"):
            raise ValueError("unknown event %r" % (name,))

    def _harmonic(self, raw):                       # ref RealTimeAnalyser.h:150,166,170-172
        f = self.fh
        f.update(RMS, raw[:, RMS])
        for s in (F0, HER, OER, INHARM):
            f.update(s, raw[:, s])

    def _spectral(self, raw):                       # ref RealTimeAnalyser.h:209,219-226,228,236-242
        f = self.fs
        f.update(RMS, raw[:, RMS])
        for s in (CENTROID, FLATNESS, LER, SPREAD, FLUX, SLOPE):
            f.update(s, raw[:, s])
        self.detector.add(f.value(FLUX), f.value(RMS))      # detectOnset: getValue at this moment
        onset = np.where(self.detector.detect(), _F(1.0), _F(0.0)).astype(_F)
        f.update(ONSET, onset)
        return onset

    def frame(self, raw):
        """raw [C][12] of one frame -> (onset [C], smoothed [C][12])"""
        raw = np.asarray(raw, _F)
        do_spec, do_harm = self.analysers & 1, self.analysers & 2
        onset = np.zeros(self.C, _F)
        if self.order == HARMONIC_THEN_SPECTRAL:
            if do_harm:
                self._harmonic(raw)
            if do_spec:
                onset = self._spectral(raw)
        else:
            if do_spec:
                onset = self._spectral(raw)
            if do_harm:
                self._harmonic(raw)
        sm = np.empty((self.C, NUM_FEATURES), _F)
        for s in range(NUM_FEATURES):
            src = self.fh if s in (F0, HER, OER, INHARM) or (s == RMS and not do_spec) else self.fs
            sm[:, s] = src.value(s)
        return onset, sm


def run(raw, events=(), order=SPECTRAL_THEN_HARMONIC, analysers=3, tail=None):
    """raw [C][T][12] -> (smoothed [C][T][12], onset [C][T]).  Pass `tail` to carry a context's state across calls (its
    events are then frame indices into this call's raw)."""
    raw = np.asarray(raw, _F)
    C, T = raw.shape[0], raw.shape[1]
    tail = tail if tail is not None else Tail(C, order, analysers)
    ev = sorted(((int(e[0]), i, e) for i, e in enumerate(events)))
    sm = np.empty((C, T, NUM_FEATURES), _F)
    onset = np.empty((C, T), _F)
    k = 0
    for t in range(T):
        while k < len(ev) and ev[k][0] <= t:
            e = ev[k][2]
            tail.event(e[1], e[2] if len(e) > 2 else None)
            k += 1
        onset[:, t], sm[:, t] = tail.frame(raw[:, t])
    while k < len(ev):                              # events after the last frame still change the state a later call sees
        e = ev[k][2]
        tail.event(e[1], e[2] if len(e) > 2 else None)
        k += 1
    return sm, onset


def assert_tail_exact(raw, sm, events=(), order=SPECTRAL_THEN_HARMONIC, analysers=3, what=""):
    """sm and raw[..., 0] are, bit for bit, what the reference's tail makes of raw; returns the number of onsets"""
    raw = np.asarray(raw)
    msm, mon = run(raw, events, order, analysers)
    bad = np.argwhere(raw[..., 0] != mon)
    assert not bad.size, "%s: onset column differs from the tail model at %d (channel, frame)s, first %s: got %r model %r" % (
        what, len(bad), tuple(bad[0]), raw[tuple(bad[0]) + (0,)], mon[tuple(bad[0])])
    same = (np.asarray(sm).view(np.uint32) == msm.view(np.uint32)) | (np.isnan(sm) & np.isnan(msm))
    if not same.all():
        c, t, f = np.argwhere(~same)[0]
        raise AssertionError("%s: %d smoothed values differ from the tail model; first channel %d frame %d slot %d: got %r model %r"
                             % (what, int((~same).sum()), c, t, f, sm[c, t, f], msm[c, t, f]))
    return int(mon.sum())
