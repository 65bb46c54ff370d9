"""An independent float64 statement of the resampler (include/mp3g.h
"sample-rate conversion of decoded rows"): the filter formula with numpy's
np.i0 and np.sinc, and y[n] as a direct dot product per output with Python
integers for the indices.  Shared by the CPU and GPU resampler tests."""
import math

import numpy as np

PAIRS = ((44100, 16000), (32000, 44100), (48000, 16000), (24000, 16000), (22050, 16000), (48000, 44100))
FAST = (16, 0.85, 8.555504641634386)
BEST = (64, 0.9475937167399596, 14.769656459379492)


def params(fi, fo, zeros, rolloff):
    """(L, M, W, c) of the filter fi -> fo."""
    g = math.gcd(fi, fo)
    M, L = fi // g, fo // g
    c = rolloff * min(1.0, L / M)
    return L, M, int(math.ceil(zeros / c)), c


def taps64(fi, fo, zeros, rolloff, beta):
    """h[r][k] = c sinc(c t) kaiser(t / W), t = k - (W - 1) - r / L, in float64."""
    L, M, W, c = params(fi, fo, zeros, rolloff)
    r = np.arange(L, dtype=np.float64)[:, None]
    k = np.arange(2 * W, dtype=np.float64)[None, :]
    t = k - (W - 1) - r / L
    u = t / W
    kaiser = np.where(np.abs(u) <= 1.0, np.i0(beta * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(beta), 0.0)
    return c * np.sinc(c * t) * kaiser


def resample64(h, L, M, x, src_origin, out_start, n_out):
    """(y, mag) in float64 for outputs [out_start, out_start + n_out): y[n] =
    sum_k h[r][k] x[q - W + 1 + k] with (q, r) = divmod(n M, L) -- Python
    integers -- and source sample j = x[j - src_origin] inside the array, 0
    elsewhere; mag[n] = sum_k |h[r][k] x[.]| (the scale of the rounding bound)."""
    h = np.asarray(h, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    W = h.shape[1] // 2
    y, mag = np.zeros(n_out), np.zeros(n_out)
    for i in range(n_out):
        q, r = divmod((out_start + i) * M, L)
        base = q - W + 1 - src_origin  # index into x of tap 0
        k0, k1 = max(0, -base), min(2 * W, len(x) - base)
        if k1 > k0:
            p = h[r, k0:k1] * x[base + k0:base + k1]
            y[i], mag[i] = p.sum(), np.abs(p).sum()
    return y, mag


def out_len(N, L, M):
    return -((-N * L) // M)
