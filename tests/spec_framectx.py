"""The statement of the delta features and the frame context (include/mp3g.h
"Delta features and frame context") that the tests hold
the library to: the delta scales as exact fractions and as a numpy float32
transcription of the recurrence, the error bounds that follow from the
roundings, the deltas in float64, the gather as an index computation, and a
transcription of FunASR's apply_lfr loop.  Pure numpy; no library call.

The bounds are derived here, not fitted.  u = 2^-24 is float32's unit roundoff
and gamma(T) = T u / (1 - T u) the usual bound on T compounded roundings.

Scales.  r = (float)(1.0 / (double)norm) is 1 / norm with a relative error of at
most U1 = u + 2^-52 (the float64 quotient, then the conversion).  Order i is made
from the computed order i - 1 (error E[i-1][k] per entry, E[0] = 0):
  cur[x] = the float32 sum, in the recurrence's order, of the T[x] terms
           (float)j * prev[k] with j + k = x: every term is rounded once as a
           product and at most T[x] - 1 times in the additions, so
           |cur[x] - sum j exact[k]| <= sum |j| E[i-1][k]
                                        + gamma(T[x]) * sum |j| (|exact[k]| + E[i-1][k])
  s[x] = fl(cur[x] * r):  with G = (1 + U1)(1 + u) - 1,
           E[i][x] = (the above) * (1 + G) / norm + |exact_i[x]| * G
Order 1 has single-term sums of small integers, so E[1][x] = |x / norm| * G: about
two roundings.  All of it is evaluated in exact fractions by scale_bounds().

A delta word of order i over T nonzero taps is a chain of T fmaf, one rounding
each: term j is rounded at most T times, so against the float64 statement
(itself off by at most (T + 2) 2^-53 of the same sum, scales included)
  |y - y64| <= sum_j (E[i][j] + (gamma(T) + (T + 2) 2^-53) (|s_j| + E[i][j])) |x_j| + 2^-149
the last term for a result in the subnormal range.

Order 1 against a float32 convolution of the same 2 W + 1 products in another
order (torch's conv1d): each side is within gamma(2 W + 1) sum |s_j x_j| of the
exact sum of ITS float32 scales times x, and the scales are the same bits, so
the two differ by at most 2 gamma(2 W + 1) sum |s_j| |x_j|.
"""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 24)
U1 = U + Fraction(1, 2 ** 52)
G = (1 + U1) * (1 + U) - 1

# (order, window): the last has a halo of 32 frames, longer than most test rows
DELTA_SETS = [(0, 1), (1, 2), (2, 2), (2, 3), (3, 1), (1, 9), (4, 8)]
# (left, right, step, first)
STACK_SETS = {"splice_3_3": (3, 3, 1, 0), "splice_0_0": (0, 0, 1, 0), "lfr_7_6": (3, 3, 6, 0), "lfr_5_1": (2, 2, 1, 0),
              "subsample_3_0": (0, 0, 3, 0), "subsample_3_2": (0, 0, 3, 2)}


def gamma(T):
    return T * U / (1 - T * U)


def norm_of(window):
    return sum(j * j for j in range(-window, window + 1))


def scales_exact(order, window):
    """[order + 1] lists of Fractions: the integer recurrence over norm^i."""
    out = [[Fraction(1)]]
    norm = norm_of(window)
    for _ in range(order):
        prev = out[-1]
        cur = [Fraction(0)] * (len(prev) + 2 * window)
        for j in range(-window, window + 1):
            for k, p in enumerate(prev):
                cur[j + window + k] += j * p
        out.append([c / norm for c in cur])
    return out


def scales_f32(order, window):
    """The recurrence transcribed in numpy float32, operation for operation."""
    out = [np.ones(1, np.float32)]
    normalizer = np.float32(1.0 / float(norm_of(window)))
    for _ in range(order):
        prev = out[-1]
        cur = np.zeros(len(prev) + 2 * window, np.float32)
        for j in range(-window, window + 1):
            for k in range(len(prev)):
                term = np.float32(np.float32(j) * prev[k])
                cur[j + window + k] = np.float32(cur[j + window + k] + term)
        out.append((cur * normalizer).astype(np.float32))
    return out


def scale_bounds(order, window):
    """E[i][x] of the module docstring, as Fractions."""
    exact = scales_exact(order, window)
    norm = norm_of(window)
    E = [[Fraction(0)]]
    for i in range(1, order + 1):
        prev, pe = exact[i - 1], E[i - 1]
        size = len(prev) + 2 * window
        carried, mass, terms = [Fraction(0)] * size, [Fraction(0)] * size, [0] * size
        for j in range(-window, window + 1):
            for k in range(len(prev)):
                x = j + window + k
                carried[x] += abs(j) * pe[k]
                mass[x] += abs(j) * (abs(prev[k]) + pe[k])
                terms[x] += 1
        E.append([(carried[x] + gamma(terms[x]) * mass[x]) * (1 + G) / norm + abs(exact[i][x]) * G
                  for x in range(size)])
    return E


def clamp_index(t, n):
    return np.clip(t, 0, n - 1)


def deltas_spec(x, n, order, window, scales):
    """(y64, bound) [F, order + 1, cols] of one plane x [F, cols] float32 whose first
    n frames are live: the float64 statement from the float32 `scales` the library
    reports (a tap of exactly 0 skipped), and the bound of the module docstring with
    E = scale_bounds.  Block 0 of y64 is x itself; frames t >= n are 0."""
    F, cols = x.shape
    n = min(n, F)
    y = np.zeros((F, order + 1, cols), np.float64)
    bound = np.zeros((F, order + 1, cols), np.float64)
    if n == 0:
        return y, bound
    y[:n, 0] = x[:n]
    E = scale_bounds(order, window)
    exact = scales_exact(order, window)
    t = np.arange(n)
    xd = x.astype(np.float64)
    for i in range(1, order + 1):
        h = i * window
        s = np.asarray(scales[i], np.float32)
        taps = [j for j in range(-h, h + 1) if s[j + h] != 0]
        T = len(taps)
        per_term = float(gamma(T)) + (T + 2) * 2.0 ** -53
        for j in taps:
            src = xd[clamp_index(t + j, n)]
            # the statement uses the EXACT scale: the float32 one's error is in the bound
            y[:n, i] += float(exact[i][j + h]) * src
            e = float(E[i][j + h])
            bound[:n, i] += (e + per_term * (abs(float(exact[i][j + h])) + e)) * np.abs(src)
        bound[:n, i] += 2.0 ** -149
    return y, bound


def conv_bound(x, n, window, s1):
    """2 gamma(2 W + 1) sum |s_j| |x_j| per word of the first n frames of x [F, cols]."""
    t = np.arange(n)
    total = np.zeros((n, x.shape[1]), np.float64)
    for j in range(-window, window + 1):
        total += abs(float(s1[j + window])) * np.abs(x[clamp_index(t + j, n)].astype(np.float64))
    return 2 * float(gamma(2 * window + 1)) * total


def n_out(n, step, first):
    return 0 if n <= first else -(-(n - first) // step)


def stack_spec(x, n, left, right, step, first, n_frames_out):
    """(bits uint32 [n_frames_out, (left + right + 1) * cols], m) of one plane x [F, cols]."""
    F, cols = x.shape
    n = min(n, F)
    m = min(n_out(n, step, first), n_frames_out)
    ctx = left + right + 1
    out = np.zeros((n_frames_out, ctx, cols), np.uint32)
    xb = np.ascontiguousarray(x).view(np.uint32)
    for j in range(m):
        t = first + j * step
        for k in range(ctx):
            out[j, k] = xb[min(max(t - left + k, 0), n - 1)]
    return out.reshape(n_frames_out, ctx * cols), m


def apply_lfr(inputs, lfr_m, lfr_n):
    """FunASR's apply_lfr as its front end runs it: pad on the left with (lfr_m - 1)
    // 2 copies of the first frame, take ceil(T / lfr_n) windows of lfr_m frames at a
    stride of lfr_n, and fill a window that runs off the end with the last frame."""
    T = inputs.shape[0]
    T_lfr = int(np.ceil(T / lfr_n))
    pad = (lfr_m - 1) // 2
    padded = np.vstack([np.tile(inputs[0], (pad, 1)), inputs])
    T = T + pad
    rows = []
    for i in range(T_lfr):
        if lfr_m <= T - i * lfr_n:
            rows.append(padded[i * lfr_n:i * lfr_n + lfr_m].reshape(1, -1))
        else:
            missing = lfr_m - (T - i * lfr_n)
            frame = padded[i * lfr_n:].reshape(-1)
            for _ in range(missing):
                frame = np.hstack([frame, padded[-1]])
            rows.append(frame.reshape(1, -1))
    return np.vstack(rows)


def special_values(x):
    """Plants -0, +-Inf and NaNs with payloads in the float32 array x (in place) and returns it."""
    flat = x.reshape(-1).view(np.uint32)
    for at, bits in ((3, 0x80000000), (11, 0x7F800000), (17, 0xFF800000), (23, 0x7FC12345), (29, 0xFFA00001),
                     (31, 0x00000001)):
        if at < flat.size:
            flat[at] = bits
    return x
