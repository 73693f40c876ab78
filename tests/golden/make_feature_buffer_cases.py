"""Build container only: what the reference's own headers (AudioAnalysis.h, AudioFeatures.h, compiled unmodified against
tools/refdiff/juce_standin.h by tools/refdiff/refdiff_buffer.cpp) make of seeded one-channel inputs on the way to a ConcatenatedFeatureBuffer
-> tests/golden/offline/feature_buffer.npz: the last frame's windowed input (the public member fftIn after performSpectralAnalysis) and the
Audio row after fillDownsampledRMSAudioChannels and after normaliseAudioChannels.  Inputs are regenerated from the seed by
feature_buffer_inputs() (the tests import it), so the fixture holds expected outputs only.  Frames other than the last are seen through
(samples, downsamples) pairs whose last frame is the wanted one.

    python tests/golden/make_feature_buffer_cases.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "refdiff"))


def feature_buffer_inputs():
    """{"frames": [(audio [S], downsamples, window), ...], "rows": [(audio [S], downsamples), ...]}"""
    rng = np.random.default_rng(20260517)
    noise = rng.normal(0, 0.3, 3 * 4096 + 7).astype(np.float32)
    frames = [(noise[:3 * n + 7], 5, n) for n in (256, 512, 1024, 2048, 4096)]         # the last frame runs past the end
    frames += [(noise[:1024], 1, 1024), (noise[:1025], 1, 1024), (noise[:775], 1, 256)]  # one frame: not centred
    frames += [(noise[:700], 20, 1024),                                                  # step 35, S < N: padded on both sides
               (noise[:5000], 4, 256),                                                   # step 1250 > N
               (noise[:300], 200, 256),                                                  # step 1
               (noise[:200], 2, 256),                                                    # frame 1 of 2: padded on both sides
               (noise[:2000], 2, 256)]                                                   # frame 1 of 2: inside the audio
    bad = noise[:775].copy()
    bad[4 * 155 - 128] = np.inf                                                          # sample 0 of the last frame: under the gain 0
    bad[4 * 155 - 128 + 8] = np.nan
    bad[4 * 155 - 128 + 9] = -np.inf
    frames.append((bad, 5, 256))
    rows = [(noise[:300], 200), (noise[:7 * 30 + 3], 30), (noise[:640], 10), (noise[:655], 10)]          # samples per step 1, 7, 64, 65
    peak = noise[:300].copy(); peak[5] = -3.0                                            # the normalising maximum comes from |lo|
    nan0 = noise[:300].copy(); nan0[0] = np.nan                                          # findMinMax starts from a NaN
    nan7 = noise[:300].copy(); nan7[7] = np.nan                                          # ... or steps over one
    nanstep = noise[:213].copy(); nanstep[100] = np.nan                                  # a NaN inside a step of 7
    rows += [(peak, 200), (np.zeros(640, np.float32), 10), (nan0, 200), (nan7, 200), (nanstep, 30), (noise[:5], 5), (noise[:9], 1)]
    return {"frames": frames, "rows": rows}


def main():
    import refdiff
    assert refdiff.legacy_available(), "needs /root/reference"
    cases = feature_buffer_inputs()
    out = {"source": "AudioAnalyser::performSpectralAnalysis (ref AudioAnalysis.h) and ConcatenatedFeatureBuffer (ref AudioFeatures.h) compiled "
                     "unmodified against tools/refdiff/juce_standin.h; tools/refdiff/refdiff_buffer.cpp"}
    for k, (audio, nd, n) in enumerate(cases["frames"]):
        out["fftin_%d" % k] = refdiff.buffer_last_frame(audio, nd, n)
    for k, (audio, nd) in enumerate(cases["rows"]):
        out["audio_%d_raw" % k], out["audio_%d_norm" % k] = refdiff.buffer_audio_row(audio, nd)
    path = os.path.join(ROOT, "tests", "golden", "offline", "feature_buffer.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
