"""Writes tests/golden/taps/*.npz: the reference's display buffers, read through its own getters (build container only: needs the
reference sources tools/refdiff compiles).

tools/refdiff/refdiff_taps.cpp single-steps the reference's unmodified RealTimeSpectralAnalyser and RealTimeHarmonicAnalyser over one
channel's hop stream; before each capture hop it arms every display flag (the overlappers' enableBufferToDrawNeedsUpdating, both
FFTAnalysers' enableFFTBufferToDrawNeedsUpdating, the PitchAnalyser's autocorrelation and cumulative-difference flags), steps, and reads
the buffers back with getBufferToDraw, getFFTBufferToDraw, getAutoCorrelationBufferToDraw, getCumulativeDifferenceBufferToDraw and
getNormalisedLagPosition -- what include/fx.h's fx_get_taps returns for the same hop.
Usage: python3 tests/golden/taps/make_taps.py   (from the repository root)
"""
import glob
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools", "refdiff"))

import refdiff  # noqa: E402
import signals  # noqa: E402

SOURCE = ("reference headers (tools/refdiff: AudioDataCollector, RealTimeAudioAnalysis, PitchAnalyser, SpectralCharacteristics, "
          "HarmonicCharacteristics, RealTimeAnalyser, unmodified) compiled against tools/refdiff/juce_standin.h; tools/refdiff/refdiff_taps.cpp "
          "arms every display flag before each capture hop and reads the buffers through the reference's getters")
FIELDS = ("window", "spectrum", "pitch_spectrum", "autocorrelation", "cnd", "lag_position")


def _loud_noise(T, N):
    x = signals.loud_noise(1, T, N)[0]
    x[T // 2, 3] = np.float32(3e38)             # a sample whose square overflows: inf / NaN through the transforms
    return x


# name: (window size, hops [T][N/2] of one channel, capture hops, gain)
def cases():
    return {
        "tone_256": (256, signals.tone_vibrato_noise(1, 12, 256)[0], [0, 5, 11], 1.0),
        "tone_gain_1024": (1024, signals.tone_vibrato_noise(1, 10, 1024)[0], [0, 3, 9], 0.37),
        "impulse_on_boundary_1024": (1024, signals.impulse_on_boundary(1, 10, 1024)[0], [2, 3, 4, 5], 1.0),
        "silence_2048": (2048, signals.silence(1, 6, 2048)[0], [0, 4], 1.0),
        "loud_noise_2048": (2048, _loud_noise(8, 2048), [1, 4, 7], 1.0),
        "low_tones_4096": (4096, signals.low_tones(1, 8, 4096)[0], [0, 3, 7], 1.0),
        "tone_4096": (4096, signals.tone_vibrato_noise(1, 6, 4096, seed=11)[0], [1, 5], 1.0),
    }


def driver():
    """g++ on refdiff_taps.cpp, the reference headers included from where they lie"""
    os.makedirs(refdiff.BUILD, exist_ok=True)
    exe = os.path.join(refdiff.BUILD, "refdiff_taps")
    srcs = [os.path.join(refdiff.HERE, "refdiff_taps.cpp"), os.path.join(refdiff.HERE, "juce_standin.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in srcs)):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-ffp-contract=off", "-fno-fast-math", "-I", refdiff.REFERENCE, "-I", refdiff.HERE,
                               srcs[0], "-o", exe])
    return exe


def run(hops, window_size, captures, gain=1.0, sample_rate=48000.0):
    """hops [T][N/2] of one channel -> {field: [K][...]} the reference's display buffers at each capture hop"""
    hops = np.ascontiguousarray(hops, np.float32)
    T, half = hops.shape
    N = window_size
    assert half * 2 == N
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<3ifd", N, T, len(captures), gain, sample_rate))
            f.write(np.asarray(captures, np.int32).tobytes())
            f.write(hops.tobytes())
        subprocess.run([driver(), fin, fout], check=True, timeout=120)
        out = np.fromfile(fout, np.float32).reshape(len(captures), 7 * N + 2)
    return {"window": out[:, :N], "spectrum": out[:, N:3 * N], "pitch_spectrum": out[:, 3 * N:5 * N],
            "autocorrelation": out[:, 5 * N:6 * N], "cnd": out[:, 6 * N:7 * N], "lag_position": out[:, 7 * N:]}


def paths():
    return sorted(glob.glob(os.path.join(HERE, "*.npz")))


def main():
    assert refdiff.available(), "the reference sources are not at %s" % refdiff.REFERENCE
    for name, (N, hops, captures, gain) in cases().items():
        got = run(hops, N, captures, gain)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), hops=hops.astype(np.float32), window_size=N, gain=np.float32(gain),
                            sample_rate=48000.0, captures=np.asarray(captures, np.int32), source=np.asarray(SOURCE), **got)
        print(name, N, captures)


if __name__ == "__main__":
    main()
