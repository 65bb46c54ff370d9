"""An independent float64 statement of SpecAugment (include/mp3g.h
"SpecAugment: time warp, frequency and time masks"): the descriptor's reading
with Python integers, the warped frame's position as an exact rational, Keys'
cubic weights from that rational, and the mean fill with math.fsum.  No float32
anywhere, so what the library computes in float32 is compared against it within
the bounds derived below.  Shared by the CPU and GPU tests."""
from fractions import Fraction
import math

import numpy as np

MAX_TIME, MAX_FREQ = 16, 4
U = 2.0 ** -24  # float32's unit roundoff
PAST, COPY, FILL, WARP = 0, 1, 2, 3

# ---- the error bound of a warped word --------------------------------------------
# The library forms t32 = fl(r / (2 n_out)) from two exact operands: |t32 - t| <= U
# (t < 1).  The weights' arguments t, fl(1 - t), fl(t + 1), fl(2 - t) are then off
# by at most U, 2 U, 3 U, 3 U (one more rounding of a value <= 2).
#   c1(x) = (1.25 x - 2.25) x^2 + 1 on [0, 1]: |c1'| = |3.75 x^2 - 4.5 x| <= 1.35
#   c2(x) = ((-0.75 x + 3.75) x - 6) x + 3 on [1, 2]: |c2'| = |-2.25 x^2 + 7.5 x - 6| <= 0.75
# so the arguments cost 1.35 U (w1), 2.7 U (w2) and 2.25 U (w0, w3).  The
# evaluations' own roundings, each at most U |value|:
#   c1: the inner fmaf (|value| <= 2.25) carried by x^2 <= 1: 2.25 U; x * x rounded,
#       carried by the inner value: 2.25 U; the outer fmaf (|value| <= 1): U.  5.5 U
#   c2: s1 = fmaf(-0.75, x, 3.75) in [2.25, 3]: 3 U; s2 = fmaf(s1, x, -6) in [-3,
#       -1.5]: 3 U + 3 U x <= 9 U; s3 = fmaf(s2, x, 3), |s3| <= 0.12: 0.12 U + 9 U x
#       <= 18.12 U
# Absolute weight errors: w0, w3 <= 20.37 U; w1, w2 <= 8.2 U.
# The tap chain fmaf(w3, x3, fmaf(w2, x2, fmaf(w1, x1, w0 x0))) rounds four times,
# each partial sum at most sum |w_k| |x_k| in magnitude (up to second order).
# Second-order terms are covered by the factor 1 + 2^-10.
E_OUTER, E_INNER = 20.37 * U, 8.2 * U


def warps(c, w, n):
    return n >= 2 and 1 <= c <= n - 1 and 1 <= w <= n - 1


def clip(start, width, extent):
    hi = min(int(start) + int(width), extent)
    return min(int(start), hi), hi


def masked_set(masks, count, cap, extent):
    m = np.zeros(extent, bool)
    for k in range(min(int(count), cap)):
        lo, hi = clip(masks[k][0], masks[k][1], extent)
        m[lo:hi] = True
    return m


def c1(x):
    return (Fraction(5, 4) * x - Fraction(9, 4)) * x * x + 1


def c2(x):
    return ((Fraction(-3, 4) * x + Fraction(15, 4)) * x - 6) * x + 3


def tap(j, c, w, n):
    """(src[4], weights[4] as float64) of destination frame j < n of a row warped by (c, w)."""
    if j < w:
        jj, n_in, n_out, base = j, c, w, 0
    else:
        jj, n_in, n_out, base = j - w, n - c, n - w, c
    p = (2 * jj + 1) * n_in - n_out
    i = p // (2 * n_out)  # (Python's floor division)
    t = Fraction(p - i * 2 * n_out, 2 * n_out)
    assert i >= -1 and 0 <= t < 1
    ws = [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]
    assert sum(ws) == 1
    src = [base + min(max(i - 1 + k, 0), n_in - 1) for k in range(4)]
    return src, np.array([float(v) for v in ws])


def mean_fill(xp, n):
    """The float64 mean of the live region xp[:n] ([F, bins], float64), exactly
    summed, and sum |x| for the test's bound."""
    if n == 0 or xp.shape[1] == 0:
        return 0.0, 0.0
    live = xp[:n].reshape(-1)
    return math.fsum(live) / (n * xp.shape[1]), math.fsum(np.abs(live))


def specaug64(x, lengths, rows, fill=0.0, warp=True, fills=None):
    """SpecAugment of x, float [B, C, F, bins] TIME-MAJOR with every column live
    (the callers transpose and cut).  Returns (kind, value, bound), each [B, C,
    F, bins]: kind PAST or COPY -- the word is the input's, bit for bit; FILL --
    the word is the fill (`fill`, or fills[b, c] when given); WARP -- the word is
    within bound of value."""
    x = np.asarray(x, np.float64)
    B, C, F, nb = x.shape
    kind = np.zeros(x.shape, np.uint8)
    value = x.copy()
    bound = np.zeros(x.shape)
    for b in range(B):
        n = min(int(lengths[b]), F)
        d = rows[b]
        tm = masked_set(d["time"], d["n_time"], MAX_TIME, n)
        fm = masked_set(d["freq"], d["n_freq"], MAX_FREQ, nb)
        c, w = int(d["warp_center"]), int(d["warp_to"])
        do_warp = warp and warps(c, w, n)
        kind[b, :, :n] = WARP if do_warp else COPY
        if do_warp:
            for j in range(n):
                src, ws = tap(j, c, w, n)
                xs = x[b][:, src, :]  # [C, 4, bins]
                value[b, :, j] = np.einsum("k,ckb->cb", ws, xs)
                ax = np.abs(xs)
                bound[b, :, j] = ((E_OUTER * (ax[:, 0] + ax[:, 3]) + E_INNER * (ax[:, 1] + ax[:, 2])
                                   + 4.0 * U * np.einsum("k,ckb->cb", np.abs(ws), ax)) * (1.0 + 2.0 ** -10))
        m = tm[:, None] | fm[None, :]  # [n, bins]
        for p in range(C):
            kind[b, p, :n][m] = FILL
            value[b, p, :n][m] = fill if fills is None else float(fills[b, p])
            bound[b, p, :n][m] = 0.0
    return kind, value, bound


# ---- the descriptors' edge cases, shared by the CPU and GPU tests -----------------
def warp_cases(n):
    """(c, w) pairs for a row of n frames: the extreme warps, c == w, a plain
    one, no warp, and warps out of range (which are copies)."""
    return [(1, n - 1), (n - 1, 1), (n // 2, n // 2), (max(n // 3, 1), max(n // 3, 1) + 1), (0, 0), (n, 1), (1, n),
            (0, n // 2), (2 ** 32 - 1, 1)]


def mask_cases(n, nb):
    """(n_time, time[], n_freq, freq[]) sets: no mask, zero width, full extent,
    clipped, starts at and past the end, an end above 2^32, overlapping masks,
    16 + 4 masks and counts above the maxima."""
    big = 2 ** 32 - 1
    every_t = [(2 * k, 1) for k in range(16)]
    every_f = [(3 * k, 1) for k in range(4)]
    return [
        (0, [], 0, []),
        (1, [(min(3, n), 0)], 1, [(min(1, nb), 0)]),
        (1, [(0, n)], 0, []),
        (0, [], 1, [(0, nb)]),
        (1, [(max(n, 1) - 1, 5)], 1, [(max(nb, 1) - 1, 9)]),
        (2, [(n, 3), (n + 7, 2)], 2, [(nb, 1), (nb + 3, 2)]),
        (2, [(1, big), (big, big)], 2, [(2, big - 1), (big, 1)]),
        (2, [(2, 4), (4, 5)], 2, [(0, 3), (2, 2)]),
        (16, every_t, 4, every_f),
        (1000, every_t, 77, every_f),
        (16, [(0, 1)] + [(big, big)] * 14 + [(n // 2, 2)], 4, [(big, 0)] * 3 + [(nb // 2, 1)]),
    ]


def edge_rows(dtype, lengths, n_frames, nb, shift=0):
    """One descriptor per row: row b takes warp case (b + shift) and mask case
    (3 b + shift) of its own length, so neighbouring rows differ in both."""
    rows = np.zeros(len(lengths), dtype)
    for b, length in enumerate(lengths):
        n = min(int(length), n_frames)
        wc, mc = warp_cases(n), mask_cases(n, nb)
        rows[b]["warp_center"], rows[b]["warp_to"] = [v % 2 ** 32 for v in wc[(b + shift) % len(wc)]]
        nt, tm, nf, fm = mc[(3 * b + shift) % len(mc)]
        rows[b]["n_time"], rows[b]["n_freq"] = nt, nf
        for k, v in enumerate(tm):
            rows[b]["time"][k] = v
        for k, v in enumerate(fm):
            rows[b]["freq"][k] = v
    return rows
