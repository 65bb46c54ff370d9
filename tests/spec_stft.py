"""An independent float64 statement of the STFT features (include/mp3g.h "STFT
and mel spectrograms of decoded rows"): framing with
reflection, the periodic Hann window of win_length centred in the frame, the DFT
by np.fft.rfft, the mel filter bank from its formulas (Slaney's or HTK's scale,
with or without the area normalisation), the logarithms with their floor, and
the derived error bounds the host reference is held to.  Nothing here calls the
library."""
import numpy as np

import spec_logmel

SIZES = (256, 512, 1024, 2048, 4096)
U = 2.0 ** -24  # float32's unit roundoff

n_frames = spec_logmel.n_frames
signals = spec_logmel.signals


def window64(n_fft, win_length=None):
    """[n_fft]: torch.stft's window -- hann_window(win_length, periodic=True)
    (one sample: 1) with zeros around it, left offset (n_fft - win_length) // 2."""
    L = n_fft if win_length is None else win_length
    w = np.zeros(n_fft)
    left = (n_fft - L) // 2
    for j in range(L):
        w[left + j] = 1.0 if L == 1 else 0.5 - 0.5 * np.cos(2.0 * np.pi * j / L)
    return w


def twiddles64(n_fft):
    """[n_fft, 2]: (cos, -sin)(2 pi k / n_fft), exact at the multiples of n_fft / 4."""
    k = np.arange(n_fft)
    t = np.stack([np.cos(2.0 * np.pi * k / n_fft), -np.sin(2.0 * np.pi * k / n_fft)], axis=1)
    t[::n_fft // 4] = [[1, 0], [0, -1], [-1, 0], [0, 1]]
    return t


def frames64(x, n_fft, hop, center=True, count=None):
    """[count, n_fft] float64 by integer indexing: frame f is xr[f hop - pad + n]."""
    x = np.asarray(x, np.float64)
    T, pad = len(x), n_fft // 2 if center else 0
    F = n_frames(T, n_fft, hop, center) if count is None else count
    out = np.zeros((F, n_fft))
    for f in range(F):
        for n in range(n_fft):
            j = f * hop - pad + n
            if j < 0:
                j = -j
            if j > T - 1:
                j = 2 * (T - 1) - j
            out[f, n] = x[j]
    return out


def frames64_fast(x, n_fft, hop, center=True, count=None):
    """frames64 by array indexing (the same index arithmetic)."""
    x = np.asarray(x, np.float64)
    T, pad = len(x), n_fft // 2 if center else 0
    F = n_frames(T, n_fft, hop, center) if count is None else count
    j = np.arange(F, dtype=np.int64)[:, None] * hop - pad + np.arange(n_fft, dtype=np.int64)[None, :]
    j = np.abs(j)
    j = np.where(j > T - 1, 2 * (T - 1) - j, j)
    return x[j]


def stft64(x, n_fft, hop, win_length=None, center=True, count=None, slow=False):
    """[K, F] complex128: rfft(frame * window), torch.stft's sign."""
    fr = (frames64 if slow else frames64_fast)(x, n_fft, hop, center, count)
    return np.fft.rfft(fr * window64(n_fft, win_length)[None, :], axis=1).T


def hz_to_mel(f, htk=False):
    if htk:
        return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)
    return spec_logmel.hz_to_mel(f)


def mel_to_hz(m, htk=False):
    if htk:
        return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)
    return spec_logmel.mel_to_hz(m)


def mel_filters64(rate, n_fft, n_mels, fmin=0.0, fmax=0.0, htk=False, norm=True):
    """[n_mels, K]: librosa.filters.mel(htk=htk, norm="slaney" if norm else None) =
    torchaudio.functional.melscale_fbanks(.., norm=.., mel_scale=..).T"""
    fmax = fmax or rate / 2.0
    fft_f = np.arange(n_fft // 2 + 1) * (rate / n_fft)
    pts = mel_to_hz(np.linspace(hz_to_mel(fmin, htk), hz_to_mel(fmax, htk), n_mels + 2), htk)
    fdiff = np.diff(pts)
    ramps = pts[:, None] - fft_f[None, :]
    w = np.maximum(0.0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
    return w * (2.0 / (pts[2:n_mels + 2] - pts[:n_mels]))[:, None] if norm else w


def features64(x, rate, n_fft, hop, win_length=None, output="power", n_mels=0, fmin=0.0, fmax=0.0, htk=False,
               norm=True, log=None, floor=None, center=True, count=None):
    """[bins, F]: complex128 for "complex", else float64."""
    X = stft64(x, n_fft, hop, win_length, center, count)
    if output == "complex":
        return X
    s = X.real ** 2 + X.imag ** 2
    if output == "magnitude":
        s = np.sqrt(s)
    if n_mels:
        s = mel_filters64(rate, n_fft, n_mels, fmin, fmax, htk, norm) @ s
    if log:
        s = (np.log if log == "ln" else np.log10)(np.maximum(s, float(np.float32(floor))))
    return s


# ---- the derived bounds --------------------------------------------------------
def gamma(n):
    return n * U / (1.0 - n * U)


def spectrum_bound(x, n_fft, hop, win_length=None, center=True, count=None):
    """[F]: a bound on |X_host[k] - X_64[k]| for every bin of frame f, relative to
    nothing: absolute.  v = fl(w x) carries U |w x| per sample (and U |x| from the
    rounded window), which the transform maps to at most sqrt(P) U ||wx||_2.  The
    network itself is Higham's (Accuracy and Stability, Thm 24.2) FFT bound: with
    twiddles in error by mu = U and butterflies costing gamma_4 per stage
    (two additions, and a product of one multiply and one fused step), the
    computed transform errs by at most stages (mu + gamma_4) (1 + ..) ||z||_2
    sqrt(len) in the 2-norm, hence in every bin.  The half-length route has
    log2(P / 2) radix-2-equivalent stages and the split step, which is one more
    stage of the same kind: log2 P stages over ||v||_2 sqrt(P)."""
    fr = np.abs(frames64_fast(x, n_fft, hop, center, count) * window64(n_fft, win_length)[None, :])
    norm2 = np.sqrt((fr ** 2).sum(axis=1))
    stages = int(np.log2(n_fft))
    eta = stages * (U + gamma(4)) * (1.0 + U + gamma(4)) ** stages
    tiny = 2.0 ** -149 * n_fft * stages  # each operation may also round in the subnormal range
    return np.sqrt(n_fft) * norm2 * (2.0 * U + eta) * (1 + 2 * U) + tiny


def feature_bound(want_X, dX, rate, n_fft, output, n_mels, fmin, fmax, htk, norm, log, floor):
    """A bound on |host - features64| per feature ([bins, F]) from the per-frame
    spectrum bound dX [F]: p = fmaf(re, re, im im) is (|X| + dX)^2 - |X|^2 off
    plus gamma_2 of its value; sqrtf adds half an ulp; the mel chain over a
    support of n bins is gamma_n (weights rounded once: one more U) of the sum of
    |w| (s + ds); the faithful logarithms add one ulp of the result to the
    propagated relative error, which the floor caps (log(max(.)) is 1-Lipschitz
    in log space above the floor)."""
    a = np.abs(want_X)
    d = dX[None, :]
    if output == "complex":
        return d + 0.0 * a
    s = a ** 2
    ds = (2.0 * a * d + d ** 2) * (1 + gamma(2)) + gamma(2) * s + 2.0 ** -149
    if output == "magnitude":
        # |sqrt(s + ds) - sqrt(s)| <= sqrt(ds) and <= ds / sqrt(s); then half an ulp
        root = np.sqrt(s)
        ds = np.minimum(np.sqrt(ds), ds / np.maximum(root, 1e-300)) + U * (root + np.sqrt(ds)) + 2.0 ** -149
        s = root
    if n_mels:
        W = mel_filters64(rate, n_fft, n_mels, fmin, fmax, htk, norm)
        n = int((W > 0).sum(axis=1).max()) + 1
        ds = W @ ds * (1 + gamma(n + 1)) + gamma(n + 1) * (W @ s) + 2.0 ** -149 * n
        s = W @ s
    if log:
        fl = float(np.float32(floor))
        lo = np.maximum(s - ds, fl)
        hi = np.maximum(s + ds, fl)
        dl = np.log(hi / lo) / (1.0 if log == "ln" else np.log(10.0))
        val = np.abs((np.log if log == "ln" else np.log10)(np.maximum(s, fl)))
        ds = dl + 2.0 * U * (val + dl) + 2.0 ** -126
    return ds
