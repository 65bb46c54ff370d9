"""An independent float64 statement of the true peak (include/mp3g.h "True peak
of decoded rows"): libebur128's 49-tap, factor-4 Hann-windowed sinc from its
formula, numpy convolutions of the whole plane, and the error bound of the
library's float32 fmaf chains.  Shares no code with the library."""
import numpy as np

TAPS, FACTOR = 49, 4
U = 2.0 ** -24  # float32 unit roundoff


def design():
    """c[j], j = 0..48, in float64."""
    j = np.arange(TAPS)
    m = j - TAPS // 2
    arg = m * np.pi / FACTOR
    sinc = np.where(m == 0, 1.0, np.sin(arg) / np.where(m == 0, 1.0, arg))
    return sinc * 0.5 * (1.0 - np.cos(2.0 * np.pi * j / (TAPS - 1)))


def phases():
    """{f: (delays, coefficients)} of the taps with |c| > 1e-6, f = 0..3."""
    c = design()
    out = {}
    for f in range(FACTOR):
        jj = np.arange(f, TAPS, FACTOR)
        keep = np.abs(c[jj]) > 1e-6
        out[f] = (jj[keep] // FACTOR, c[jj][keep])
    return out


def interpolated(x, n=None):
    """[3, n]: y_f of one plane's first n samples, f = 1..3, in float64 (x[k] = 0 for k < 0, no tail)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x) if n is None else min(int(n), len(x))
    ph = phases()
    y = np.zeros((3, n))
    for f in (1, 2, 3):
        t, c = ph[f]
        assert t.tolist() == list(range(12))
        y[f - 1] = np.convolve(x[:n], c)[:n]
    return y


def true_peak(x, length=None):
    """The true peak of the row x [C, T] (or [T]) over its first `length` samples, float64."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[-1] if length is None else min(int(length), x.shape[-1])
    tp = 0.0
    for ch in x:
        if n:
            tp = max(tp, np.abs(ch[:n]).max(), np.abs(interpolated(ch, n)).max())
    return tp


def error_bound(x, length=None):
    """How far a float32 evaluation may lie from true_peak.  Per output, a chain
    of 12 fmaf's from 0 is a recursive sum of 12 products: its error is at most
    gamma_12 sum_t |c_t| |x[n-t]| (Higham, Accuracy and Stability, 3.1);
    gamma_13 is taken, gamma_k = k u / (1 - k u), u = 2^-24.  The coefficients
    are float32 roundings of these float64 ones: at most u |c_t| each, another
    u sum_t |c_t| |x[n-t]|.  Twelve subnormal roundings add 12 * 2^-150.  Two
    maxima whose terms differ by at most b(n) differ by at most max_n b(n)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[-1] if length is None else min(int(length), x.shape[-1])
    if n == 0:
        return 0.0
    gamma13 = 13 * U / (1 - 13 * U)
    ph = phases()
    worst = 0.0
    for ch in x:
        for f in (1, 2, 3):
            mag = np.convolve(np.abs(ch[:n]), np.abs(ph[f][1]))[:n]
            worst = max(worst, mag.max())
    return (gamma13 + U) * worst + 12 * 2.0 ** -150
