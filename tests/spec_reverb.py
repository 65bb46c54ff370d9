"""The reverberation and noise mixing of include/mp3g.h ("Room reverberation and
noise at an SNR"), restated from its words alone in numpy float64: direct
np.convolve, math.fsum for every power, no FFT and no blocks.  Beside it, for
the tolerance of the convolved samples, an INDEPENDENT float32 formulation: the
same uniformly partitioned overlap-save written with numpy.fft on complex64."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def rir_info(h, fs):
    """(peak, es, ee, P) of the response h (1-D) at rate fs."""
    h = np.asarray(h)
    L = len(h)
    peak = int(np.argmax(h))  # the first index of the largest value
    es = max(0, peak - fs // 1000)
    ee = min(L, peak + fs // 20)
    return peak, es, ee, (L + 1023) // 1024


def power(v):
    """sum(v^2) / len, exactly summed; no samples: 0."""
    v = np.asarray(v, dtype=F64)
    return math.fsum((v * v).tolist()) / len(v) if len(v) else 0.0


def reverberate(x, h, fs):
    """Steps 1 and 2 for the n samples x: (y float64 [n], power_before, signal_power)."""
    x = np.asarray(x, dtype=F64)
    n = len(x)
    pb = power(x)
    if h is None or n == 0:
        return x.copy(), pb, pb
    h = np.asarray(h, dtype=F64)
    peak, es, ee, _ = rir_info(h, fs)
    y = np.convolve(x, h)[peak:peak + n]
    early = np.convolve(x, h[es:ee])  # the whole of x * h_e: n + (ee - es) - 1 values
    assert len(early) == n + (ee - es) - 1
    return y, pb, math.fsum((early * early).tolist()) / len(early)


def gain(snr_db, signal_power, noise_power):
    """The slot's gain in float64 (the library rounds it to float32)."""
    return math.sqrt(10.0 ** (-snr_db / 10.0) * signal_power / noise_power)


def fmaf32(g, a, v):
    """float32 fma(g, a, v), correctly rounded, for float32 arrays: the product
    is exact in float64, TwoSum gives the sum's error, and a float64 sum that is
    a tie of two float32 values is sent where the error points."""
    p = np.asarray(g, F32).astype(F64) * np.asarray(a, F32).astype(F64)
    v64 = np.asarray(v, F32).astype(F64)
    s = p + v64
    bb = s - p
    err = (p - (s - bb)) + (v64 - bb)
    r = s.astype(F32)
    d = s - r.astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        up, dn = np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))
        tie_up = (d > 0) & (d == (up.astype(F64) - r.astype(F64)) / 2)
        tie_dn = (d < 0) & (-d == (r.astype(F64) - dn.astype(F64)) / 2)
    r = np.where(tie_up & (err > 0), up, r)
    return np.where(tie_dn & (err < 0), dn, r).astype(F32)


def mix(y32, slots):
    """Step 3 on the float32 samples y32 [n]: slots is a list of (g float32,
    noise float32 [len], start, offset, wrap) in order; the float32 fmaf chain."""
    v = np.asarray(y32, F32).copy()
    n = len(v)
    for g, noise, start, offset, wrap in slots:
        if start >= n:
            continue
        ln = len(noise)
        count = n - start if wrap else min(ln - offset, n - start)
        at = (offset + np.arange(count)) % ln
        v[start:start + count] = fmaf32(np.full(count, g, F32), noise[at], v[start:start + count])
    return v


def normalize(v32, power_before):
    """Step 4: (out float32, power_after, scale)."""
    pa = power(v32)
    scale = 1.0 if pa == 0.0 or len(v32) == 0 else math.sqrt(power_before / pa)
    return (np.asarray(v32, F32).astype(F64) * scale).astype(F32), pa, scale


def overlap_save_f32(x, h):
    """The whole of x * h (n + L - 1 values) by partitioned overlap-save in
    float32: numpy.fft on complex64 (N = 2048, 1,024 new samples a block),
    products and sums in complex64.  An independent float32 formulation:
    another factorisation, natural bin order, numpy's own twiddles."""
    x = np.asarray(x, F32)
    h = np.asarray(h, F32)
    n, L = len(x), len(h)
    P, NB = (L + 1023) // 1024, (n + 1023) // 1024
    hp = np.zeros((P, 2048), F32)
    for p in range(P):
        seg = h[1024 * p:1024 * p + 1024]
        hp[p, :len(seg)] = seg
    G = np.fft.fft(hp.astype(np.complex64), axis=1)
    assert G.dtype == np.complex64
    xp = np.zeros(1024 * (NB + 2), F32)
    xp[1024:1024 + n] = x  # block m - 1 and m of x at xp[1024 m : 1024 m + 2048]
    X = np.stack([np.fft.fft(xp[1024 * m:1024 * m + 2048].astype(np.complex64)) for m in range(NB + 1)])
    K = (n + L - 2) // 1024 + 1
    full = np.zeros(1024 * K, F32)
    for k in range(K):
        acc = np.zeros(2048, np.complex64)
        for p in range(max(0, k - NB), min(P - 1, k) + 1):
            acc = acc + X[k - p] * G[p]
        full[1024 * k:1024 * k + 1024] = np.fft.ifft(acc)[1024:].real.astype(F32)
    return full[:n + L - 1]


U32 = 2.0 ** -24


def block_error_bounds(x, h, fs):
    """A bound on the error of every float32 sample of x * h and x * h_e that
    include/mp3g.h's pipeline produces, per block of 1,024 of the full timeline:
    B[k] holds for t in [1024 k, 1024 k + 1024).  DESIGN.md 9k has the steps.
    Higham's Theorem 24.2 (Accuracy and Stability of Numerical Algorithms, 2nd
    ed.): a radix-2 transform y = F a of N = 2^t points computed with twiddles in
    error by at most mu errs by ||dy||_2 <= eps_F ||y||_2, eps_F = t eta / (1 - t eta),
    eta = mu + gamma_4 (sqrt 2 + mu), gamma_4 = 4 u / (1 - 4 u) -- a bound of the
    2-norm, not of a single bin.  Here t = 11, u = mu = 2^-24, and a radix-4 pass is
    taken as two radix-2 levels of which one has exact twiddles.  With X = F x^(m)
    (x^(m) the 2,048 input samples of a block), G = F g_p, ||F a||_2 = sqrt N ||a||_2
    and ||F^-1 A||_2 = ||A||_2 / sqrt N, to first order and per partition:
      dX o G:   ||.||_2 <= eps_F ||X||_2 max|G|             -> eps_F ||x||_2 max|G|
      X o dG:   ||.||_2 <= max|X| ||dG||_2 <= ||x||_1 eps_F sqrt N ||g||_2
                                                             -> eps_F ||x||_1 ||g||_2
      product (two roundings a part) and the P - 1 additions:  (P + 2) u ||x||_2 max|G|
      inverse:  eps_F ||z||_2, ||z||_2 <= sum_p ||x||_2 max|G|
    so |dz_j| <= ||dz||_2 <= sum_p ((2 eps_F + (P + 2) u) ||x^(k-p)||_2 max|G_p|
                                   + eps_F ||x^(k-p)||_1 ||g_p||_2),
    with 1 % added for the second-order terms.  A worst-case bound of a 2-norm:
    two to four orders above the errors seen."""
    x = np.asarray(x, F64)
    h = np.asarray(h, F64)
    n, L = len(x), len(h)
    peak, es, ee, P = rir_info(h, fs)
    g = h.astype(np.complex128)
    g.imag[es:ee] = h[es:ee]
    NB = (n + 1023) // 1024
    xp = np.zeros(1024 * (NB + 2))
    xp[1024:1024 + n] = x
    x2 = [float(np.linalg.norm(xp[1024 * m:1024 * m + 2048])) for m in range(NB + 1)]
    x1 = [float(np.abs(xp[1024 * m:1024 * m + 2048]).sum()) for m in range(NB + 1)]
    ginf, g2 = [], []
    for p in range(P):
        gp = np.zeros(2048, np.complex128)
        seg = g[1024 * p:1024 * p + 1024]
        gp[:len(seg)] = seg
        ginf.append(float(np.abs(np.fft.fft(gp)).max()))
        g2.append(float(np.linalg.norm(gp)))
    t, eta = 11, U32 + 4 * U32 / (1 - 4 * U32) * (math.sqrt(2.0) + U32)
    eps_f = t * eta / (1 - t * eta)
    c = 2 * eps_f + (P + 2) * U32
    K = (n + L - 2) // 1024 + 1
    return np.array([1.01 * sum(c * x2[k - p] * ginf[p] + eps_f * x1[k - p] * g2[p]
                                for p in range(max(0, k - NB), min(P - 1, k) + 1)) for k in range(K)])
