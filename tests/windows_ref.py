"""The windowed decode's layout rule in a few lines of numpy, and the streams
the window tests share (tests/test_windows_cpu.py, tests/test_gpu_windows.py).
"""
import numpy as np

from mp3g import synth


def layout(headers, start, T):
    """(h, n, lead, skip, n_valid) of the window (start, T) of a stream whose
    full scan has the granule headers `headers`: the decoded run is granules
    [h, h + n), include/mp3g.h "sample-windowed decode"."""
    G = len(headers)
    if T == 0 or start >= 576 * G:
        return 0, 0, 0, 0, 0
    lo, skip = divmod(start, 576)
    hi = min(-(-(start + T) // 576), G)
    stereo = np.nonzero(((np.asarray(headers, np.uint32)[:lo] >> 6) & 3) != 3)[0]
    h = max(lo - 2, 0)
    if len(stereo) >= 2:
        h = min(h, int(stereo[-2]))
    elif len(stereo) == 1:
        h = min(h, int(stereo[-1]))
    return h, hi - h, lo - h, skip, min(T, 576 * G - start)


def switching_stream(seed=40):
    """Stereo and mono runs in one stream (every piece starts with an empty reservoir)."""
    parts = [(synth.MODE_JOINT, 10), (synth.MODE_MONO, 8), (synth.MODE_JOINT, 1), (synth.MODE_MONO, 9),
             (synth.MODE_JOINT, 12)]
    return b"".join(synth.encode_stream(seed + i, n, mode=m) for i, (m, n) in enumerate(parts))


def starts_for(n_samples):
    """The start offsets of the layout test for a stream of n_samples."""
    return [0, 1, 575, 576, 577, n_samples // 2 + 123, n_samples - 1, n_samples, n_samples + 1]


def switching_lsf_stream(seed=60):
    """MPEG-2 LSF (one granule per frame): a single stereo granule between mono runs."""
    parts = [(synth.MODE_MONO, 6), (synth.MODE_JOINT, 1), (synth.MODE_MONO, 12), (synth.MODE_JOINT, 5)]
    return b"".join(synth.encode_stream(seed + i, n, mode=m, lsf=True) for i, (m, n) in enumerate(parts))
