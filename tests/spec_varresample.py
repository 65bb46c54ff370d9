"""An independent float64 statement of the variable-ratio resampler
(include/mp3g.h "variable-ratio resampling of decoded rows"): the prototype
table's formulae with numpy's np.i0 and np.sinc, and the ANALYTIC value of an
output,

    y[n] = c * sum_j f(c * (j - n num / den)) * x[j],    c = I / 2^P,

with Python integers for every index and ratio -- no table, no interpolation.
Shared by the CPU and GPU tests of the variable-ratio resampler."""
import numpy as np

FAST = (16, 0.85, 8.555504641634386)
BEST = (64, 0.9475937167399596, 14.769656459379492)


def f(v, zeros, beta):
    """sinc(v) kaiser(v / zeros) in float64; 0 for |v| >= zeros."""
    v = np.asarray(v, dtype=np.float64)
    u = v / zeros
    k = np.i0(beta * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(beta)
    return np.where(np.abs(u) < 1.0, np.sinc(v) * k, 0.0)


def params(zeros, rolloff, P, num, den):
    """(Z, R, I, Wr) of a row: Z = zeros << P, R = floor(rolloff 2^P), I = R or
    floor(R den / num), Wr = ceil(Z / I)."""
    Z = zeros << P
    R = int(np.floor(rolloff * (1 << P)))
    I = R if num <= den else R * den // num
    return Z, R, I, (-(-Z // I) if I else 0)


def table64(zeros, beta, P):
    """(F, D) in float64: F[i] = f(i / 2^P), F[Z] = 0; D[i] = f((i + 1) / 2^P)
    - f(i / 2^P), D[Z] = 0."""
    Z = zeros << P
    g = f(np.arange(Z + 2) / float(1 << P), zeros, beta)
    g[Z:] = 0.0
    return g[:Z + 1].copy(), np.concatenate([g[1:Z + 1] - g[:Z], [0.0]])


def max_f2(zeros, beta, h=1e-3):
    """max |f''| over the support, by second differences of the analytic f on a
    grid of step h (v = 0, where the maximum pi^2 / 3 + ... lies, is a grid
    point), with 1e-4 of it added for the grid."""
    v = np.arange(0.0, zeros + h, h)
    d2 = (f(v + h, zeros, beta) - 2.0 * f(v, zeros, beta) + f(v - h, zeros, beta)) / (h * h)
    return float(np.abs(d2).max()) * (1.0 + 1e-4)


def out_len(N, num, den):
    return -((-N * den) // num)


def analytic(x, src_origin, out_start, n_out, num, den, zeros, rolloff, beta, P, support=None):
    """(y, sum_abs_x, sum_abs_wx, taps) in float64 for outputs [out_start,
    out_start + n_out): y the analytic value above over the source samples j =
    x[j - src_origin] (0 elsewhere); sum_abs_x = sum |x_j| and sum_abs_wx = sum
    |f(.) x_j| over the taps that exist (|c (j - n num / den)| < zeros) and lie
    inside the array; taps = how many exist, inside or not.  The argument of f
    is the exact rational I (j den - n num) / (den 2^P), divided once.
    support = (a, b): x is known to be zero outside x[a:b]."""
    x = np.asarray(x, dtype=np.float64)
    Z, _, I, Wr = params(zeros, rolloff, P, num, den)
    c = I / float(1 << P)
    a0, b0 = (0, len(x)) if support is None else support
    y, sx, swx, taps = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, np.int64)
    for i in range(n_out):
        n = out_start + i
        q, r = divmod(n * num, den)
        # left taps k = 0 .. nL-1 at I (k den + r) < Z den; right taps at I (k den + den - r) < Z den
        nL = -(-(Z * den - I * r) // (I * den))
        nR = max(0, -(-(Z * den - I * (den - r)) // (I * den)))
        taps[i] = nL + nR
        lo = max(q - nL + 1 - src_origin, a0)
        hi = min(q + nR + 1 - src_origin, b0)
        if hi <= lo:
            continue
        j = np.arange(lo, hi) + (src_origin - q)      # j - q, small integers
        arg = (I * (j * den - r)).astype(np.float64) / float(den << P) if den < (1 << 20) else \
            np.array([I * (int(t) * den - r) / (den << P) for t in j])
        w = f(arg, zeros, beta)
        p = w * x[lo:hi]
        y[i], sx[i], swx[i] = c * p.sum(), np.abs(x[lo:hi]).sum(), np.abs(p).sum()
    return y, sx, swx, taps


def bound(sx, swx, taps, I, P, M2):
    """The bound on |host - analytic|: linear interpolation of f at step 2^-P
    (M2 / (8 4^P)), the float32 roundings of F, D and the weight (3 2^-24), and
    the length-T FMA chain with the two final multiplications (gamma)."""
    u = 2.0 ** -24
    c = I / float(1 << P)
    gamma = (taps + 2) * u / (1.0 - (taps + 2) * u)
    return c * sx * (M2 / (8.0 * 4.0 ** P) + 3.0 * u) + gamma * c * swx
