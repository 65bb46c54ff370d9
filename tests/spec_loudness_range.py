"""An independent float64 statement of the momentary and short-term maxima and
the loudness range (include/mp3g.h "Momentary and short-term maxima, loudness
range"; EBU Tech 3341 / 3342): spec_loudness.py's K-weighting run SEQUENTIALLY
over the whole row with scipy.signal.lfilter, numpy sums of 4 and 30 segments,
the two gates, np.sort and the nearest-rank percentiles, np.log10.  Shares no
code with the library."""
import numpy as np
from scipy.signal import lfilter

from spec_loudness import ABS_GATE, k_weighting, segment

WIN = 30  # segments of a short-term block


def segment_energies(x, rate, length=None):
    """[C, nseg]: sum of squares of the K-weighted samples per 100 ms segment."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[-1] if length is None else min(int(length), x.shape[-1])
    H = segment(rate)
    nseg = n // H
    shelf, highpass = k_weighting(rate)
    e = np.zeros((x.shape[0], nseg))
    for c, ch in enumerate(x):
        w = lfilter(highpass[0], highpass[1], lfilter(shelf[0], shelf[1], ch[:nseg * H]))
        e[c] = (w * w).reshape(nseg, H).sum(axis=1)
    return e


def windows(e, width, H):
    """Mean energies of every `width` consecutive segments, channels summed."""
    nseg = e.shape[1]
    if nseg < width:
        return np.zeros(0)
    tot = e.sum(axis=0)
    return np.array([tot[k:k + width].sum() for k in range(nseg - width + 1)]) / (width * H)


def lufs(v):
    return -0.691 + 10.0 * np.log10(v) if v > 0 else -np.inf


def loudness_range(x, rate, length=None):
    """dict of one row: momentary_max, shortterm_max, lra, range_lo, range_hi
    (LUFS / LU), n_short, n_range, v_lo, v_hi (the selected energies), S (the
    short-term energies), margin (the smallest relative distance of a
    short-term energy to a gate) and rank_gap (the smallest relative distance
    of a selected value to a neighbour in the sorted gated set)."""
    H = segment(rate)
    e = segment_energies(x, rate, length)
    z = windows(e, 4, H)
    S = windows(e, WIN, H)
    out = {"momentary_max": lufs(z.max()) if len(z) else -np.inf,
           "shortterm_max": lufs(S.max()) if len(S) else -np.inf, "n_short": len(S), "S": S}
    a = S[S >= ABS_GATE]
    margin = np.abs(S / ABS_GATE - 1.0).min() if len(S) else np.inf
    g = np.zeros(0)
    if len(a):
        rel = 0.01 * a.mean()
        margin = min(margin, np.abs(a / rel - 1.0).min())
        g = np.sort(a[a >= rel])
    out["n_range"] = len(g)
    gap = np.inf
    if len(g):
        lo, hi = ((len(g) - 1) * 10 + 50) // 100, ((len(g) - 1) * 95 + 50) // 100
        for r in {lo, hi}:
            for q in (r - 1, r + 1):
                if 0 <= q < len(g):
                    gap = min(gap, abs(g[q] / g[r] - 1.0))
        out.update(v_lo=g[lo], v_hi=g[hi], range_lo=lufs(g[lo]), range_hi=lufs(g[hi]),
                   lra=lufs(g[hi]) - lufs(g[lo]))
    else:
        out.update(v_lo=0.0, v_hi=0.0, range_lo=-np.inf, range_hi=-np.inf, lra=0.0)
    out["margin"] = margin
    out["rank_gap"] = gap
    return out
