"""An independent float64 statement of the sliding-window CMN, the energy VAD
and the voiced-frame selection (include/mp3g.h "Sliding-window CMN, energy VAD
and voiced-frame selection").  The window rule is restated
from the header's text; every window is summed directly with math.fsum -- no
prefix differences and no blocks.  Nothing here calls the library."""
import math

import numpy as np


def window(t, n, W, min_window, center):
    """[s, e) of frame t in a row of n frames."""
    if center:
        s = t - W // 2
        e = s + W
    else:
        s = t - W
        e = t + 1
    if s < 0:
        e -= s
        s = 0
    if not center and e > t:
        e = max(t + 1, min_window)
    if e > n:
        s -= e - n
        e = n
        s = max(s, 0)
    return s, e


def planes_of(x, lengths):
    """(plane view [F, S] of y, n) over the rows and planes of y [B, (C,) F, S]."""
    F = x.shape[-2]
    for b in range(x.shape[0]):
        n = min(int(lengths[b]), F)
        for p in ([x[b]] if x.ndim == 3 else list(x[b])):
            yield p, n


def sliding_cmn64(x, lengths, W, min_window, center, norm_vars, n_cols=None):
    """A float64 normalised copy of x [B, (C,) F, S]; the mean and the mean
    square of each window are correctly rounded (math.fsum of exact terms)."""
    x = np.asarray(x, np.float32)
    y = np.array(x, dtype=np.float64)
    cols = y.shape[-1] if n_cols is None else n_cols
    for (yp, n), (xp, _) in zip(planes_of(y, lengths), planes_of(x.astype(np.float64), lengths)):
        for c in range(cols):
            col = [float(v) for v in xp[:n, c]]
            sq = [v * v for v in col]  # (exact: the products of two float32)
            for t in range(n):
                s, e = window(t, n, W, min_window, center)
                mean = math.fsum(col[s:e]) / (e - s)
                v = col[t] - mean
                if norm_vars:
                    var = math.fsum(sq[s:e]) / (e - s) - mean * mean
                    v = v / math.sqrt(max(var, 1e-10))
                yp[t, c] = v
    return y


def vad64(x, lengths, energy_threshold, energy_mean_scale, proportion_threshold, frames_context, col=0):
    """(voiced uint8 [B, (C,) F], counts [B, (C)], thr float64 [B, (C)]): the
    threshold from a correctly rounded mean; the proportion is compared as
    Kaldi compares it, a float32 product against a float32 count."""
    x = np.asarray(x, np.float32)
    voiced = np.zeros(x.shape[:-1], np.uint8)
    thr = np.zeros(int(np.prod(x.shape[:-2])))
    k = 0
    for (vp, n), (xp, _) in zip(planes_of(voiced[..., None], lengths), planes_of(x, lengths)):
        e = [float(v) for v in xp[:n, col]]
        th = float(np.float32(energy_threshold))
        if energy_mean_scale != 0 and n:
            th += float(np.float32(energy_mean_scale)) * (math.fsum(e) / n)
        thr[k] = th
        k += 1
        for t in range(n):
            lo, hi = max(0, t - frames_context), min(n - 1, t + frames_context)
            num = sum(1 for t2 in range(lo, hi + 1) if e[t2] > th)
            den = hi - lo + 1
            vp[t, 0] = np.float32(num) >= np.float32(den) * np.float32(proportion_threshold)
    counts = voiced.sum(axis=-1).astype(np.int64)
    return voiced, counts, thr.reshape(x.shape[:-2])


def select(x, voiced, lengths, n_frames_out, n_cols=None):
    """(out float32 [B, (C,) n_frames_out, S] zeros elsewhere, lengths_out): numpy boolean indexing."""
    x = np.asarray(x, np.float32)
    cols = x.shape[-1] if n_cols is None else n_cols
    out = np.zeros(x.shape[:-2] + (n_frames_out, x.shape[-1]), np.float32)
    m = np.zeros(int(np.prod(x.shape[:-2])), np.int64)
    k = 0
    for (op, _), (xp, n), (vp, _) in zip(planes_of(out, lengths), planes_of(x, lengths),
                                         planes_of(np.asarray(voiced)[..., None], lengths)):
        keep = xp[:n][vp[:n, 0] != 0][:n_frames_out]
        op[:len(keep), :cols] = keep[:, :cols]
        m[k] = len(keep)
        k += 1
    return out, m.reshape(x.shape[:-2])
