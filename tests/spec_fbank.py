"""An independent float64 statement of Kaldi's filter-bank features
(include/mp3g.h "Kaldi filter-bank features of decoded rows", DESIGN.md section
9e), written from the formulas with Python-integer indices: framing in both
modes, DC removal, pre-emphasis with the replicated first sample, the four
windows, the power of the zero-padded P-point rfft, Kaldi's mel bank and
log(max(., eps)).  Nothing here calls the library."""
import numpy as np

# (rate, N, hop, n_mels)
CONFIGS = [(16000, 400, 160, 80), (16000, 400, 160, 128), (8000, 200, 80, 23), (22050, 551, 220, 80),
           (16000, 16, 4, 4)]
WINDOWS = ("povey", "hamming", "hanning", "rectangular")
EPS = 2.0 ** -23


def padded(N):
    P = 16
    while P < N:
        P *= 2
    return P


def n_frames(T, N, hop, snip=True):
    if T < N:
        return 0
    return 1 + (T - N) // hop if snip else (T + hop // 2) // hop


def frame_indices(T, N, hop, snip=True, count=None):
    """[F][N] Python integers: the sample every frame element reads."""
    F = n_frames(T, N, hop, snip) if count is None else count
    rows = []
    for f in range(F):
        start = f * hop if snip else f * hop + hop // 2 - N // 2
        row = []
        for n in range(N):
            j = start + n
            if j < 0:
                j = -j - 1
            if j >= T:
                j = 2 * T - 1 - j
            assert 0 <= j < T
            row.append(j)
        rows.append(row)
    return rows


def window(kind, N):
    a = 2.0 * np.pi * np.arange(N) / (N - 1)
    if kind == "povey":
        return (0.5 - 0.5 * np.cos(a)) ** 0.85
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if kind == "hanning":
        return 0.5 - 0.5 * np.cos(a)
    assert kind == "rectangular"
    return np.ones(N)


def frames64(x, N, hop, snip=True, count=None, scale=32768.0, remove_dc=True, preemph=0.97):
    """[F, N] float64: the scaled frames after DC removal and pre-emphasis, before the window."""
    x = np.asarray(x, np.float64)
    idx = np.array(frame_indices(len(x), N, hop, snip, count), dtype=np.int64).reshape(-1, N)
    s = scale * x[idx]
    if remove_dc:
        s = s - s.sum(axis=1, keepdims=True) / N
    prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)  # the first sample refers to itself
    return s - preemph * prev


def dft_tables64(N, kind="povey"):
    """Cw, Sw [K, N]: the window folded into the rows of the P-point DFT, (k n) mod P in integers."""
    P = padded(N)
    k = np.arange(P // 2, dtype=np.int64)[:, None]
    n = np.arange(N, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((k * n) % P).astype(np.float64) / P
    w = window(kind, N)[None, :]
    return w * np.cos(a), -w * np.sin(a)


def power64(x, N, hop, kind="povey", **kw):
    """[F, K]: |rfft(frame * window, P)|^2 without the Nyquist bin."""
    sp = np.fft.rfft(frames64(x, N, hop, **kw) * window(kind, N)[None, :], n=padded(N), axis=1)[:, :-1]
    return sp.real ** 2 + sp.imag ** 2


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_filters64(rate, N, n_mels, low=20.0, high=0.0):
    """[n_mels, K]: Kaldi's get_mel_banks without VTLN, no normalisation."""
    P = padded(N)
    if high <= 0.0:
        high += rate / 2.0
    delta = (mel(high) - mel(low)) / (n_mels + 1)
    mk = mel(np.arange(P // 2) * (rate / P))[None, :]
    left = mel(low) + np.arange(n_mels)[:, None] * delta
    right = left + 2.0 * delta
    return np.maximum(0.0, np.minimum((mk - left) / delta, (right - mk) / delta))


def fbank64(x, rate, N, hop, n_mels, kind="povey", low=20.0, high=0.0, **kw):
    """[F, n_mels] float64."""
    m = power64(x, N, hop, kind, **kw) @ mel_filters64(rate, N, n_mels, low, high).T
    return np.log(np.maximum(m, EPS))


def signals(T, rng):
    """The input kinds of the tests: (name, float32 [T], scale).  Noise at int16
    scale, a constant (with DC removal all floor), a large DC offset plus small
    noise (the cancellation in d), the impulses of the edges, zeros, and noise
    scaled by 2^-120 with scale 1 (the power underflows to the floor)."""
    noise = rng.uniform(-1.0, 1.0, T).astype(np.float32)
    yield "noise", noise, 32768.0
    yield "constant", np.full(T, 0.75, np.float32), 32768.0
    yield "dc+noise", (np.float32(0.9) + noise * np.float32(2.0 ** -10)).astype(np.float32), 32768.0
    for p in (0, 1, T - 2, T - 1):
        x = np.zeros(T, np.float32)
        x[p] = 1.0
        yield f"impulse@{p}", x, 32768.0
    yield "zeros", np.zeros(T, np.float32), 32768.0
    yield "tiny", (noise * np.float32(2.0 ** -120)).astype(np.float32), 1.0
