"""An independent float64 statement of Kaldi's MFCC features (include/mp3g.h
"Kaldi MFCC features of decoded rows") on top of the
filter-bank spec (spec_fbank): Kaldi's DCT matrix, the cepstral lifter, the raw
and the windowed log energy, the energy floor and the replacement of c0, and
the per-row mean / variance normalisation.  Framing is spec_fbank's
Python-integer framing.  Nothing here calls the library."""
import numpy as np

import spec_fbank as fb

# (n_mels, n_ceps)
TABLES = [(23, 13), (40, 40), (80, 20), (128, 128), (4, 4)]
EPS = fb.EPS


def dct_matrix(M, n_ceps):
    """[n_ceps, M]: Kaldi's ComputeDctMatrix, its first n_ceps rows."""
    D = np.empty((n_ceps, M))
    D[0, :] = np.sqrt(1.0 / M)
    for i in range(1, n_ceps):
        D[i, :] = np.sqrt(2.0 / M) * np.cos(np.pi / M * (np.arange(M) + 0.5) * i)
    return D


def lifter(Q, n_ceps):
    if Q == 0:
        return np.ones(n_ceps)
    return 1.0 + 0.5 * Q * np.sin(np.pi * np.arange(n_ceps) / Q)


def centred64(x, N, hop, snip=True, count=None, scale=32768.0, remove_dc=True):
    """[F, N] float64: the scaled frames after DC removal (d of the contract)."""
    x = np.asarray(x, np.float64)
    idx = np.array(fb.frame_indices(len(x), N, hop, snip, count), dtype=np.int64).reshape(-1, N)
    s = scale * x[idx]
    return s - s.sum(axis=1, keepdims=True) / N if remove_dc else s


def energy64(x, N, hop, raw=True, kind="povey", snip=True, count=None, scale=32768.0, remove_dc=True, preemph=0.97):
    """[F] float64: sum d^2 (raw) or sum (w e)^2."""
    if raw:
        v = centred64(x, N, hop, snip, count, scale, remove_dc)
    else:
        v = fb.frames64(x, N, hop, snip, count, scale, remove_dc, preemph) * fb.window(kind, N)[None, :]
    return (v * v).sum(axis=1)


def mfcc64(x, rate, N, hop, n_mels, n_ceps, Q=22.0, use_energy=True, raw=True, energy_floor=0.0, kind="povey",
           low=20.0, high=0.0, snip=True, count=None, scale=32768.0, remove_dc=True, preemph=0.97):
    """[F, n_ceps] float64."""
    kw = dict(snip=snip, count=count, scale=scale, remove_dc=remove_dc, preemph=preemph)
    L = fb.fbank64(x, rate, N, hop, n_mels, kind, low, high, **kw)
    y = (L @ dct_matrix(n_mels, n_ceps).T) * lifter(Q, n_ceps)[None, :]
    if use_energy:
        le = np.log(np.maximum(energy64(x, N, hop, raw, kind, **kw), EPS))
        if energy_floor > 0.0:
            le = np.maximum(le, np.log(energy_floor))
        y[:, 0] = le
    return y


def cmvn64(x, lengths, norm_vars=False, n_cols=None):
    """A float64 normalised copy of x [B, (C,) F, S]: per row over its first
    min(lengths[b], F) frames, columns below n_cols."""
    y = np.array(x, dtype=np.float64)
    cols = y.shape[-1] if n_cols is None else n_cols
    for b in range(y.shape[0]):
        n = min(int(lengths[b]), y.shape[-2])
        if n == 0:
            continue
        part = y[b, ..., :n, :cols]
        mean = part.mean(axis=-2, keepdims=True)
        out = part - mean
        if norm_vars:
            var = (part * part).mean(axis=-2, keepdims=True) - mean * mean
            out = out / np.sqrt(np.maximum(var, 1e-20))
        y[b, ..., :n, :cols] = out
    return y
