"""An independent float64 statement of the log-mel features (include/mp3g.h
"log-mel features of decoded rows"): framing with
reflection, the periodic Hann window, the DFT by np.fft.rfft, Slaney's mel
filter bank from its formulas, np.log10 and Whisper's clamp.  Nothing here
calls the library."""
import numpy as np

# (n_fft, hop, n_mels, rate)
CONFIGS = [(400, 160, 80, 16000), (400, 160, 128, 16000), (1024, 256, 128, 44100), (16, 4, 4, 16000)]
FLOOR = 1e-10


def n_frames(T, n_fft, hop, center=True):
    if center:
        return T // hop + 1 if T > n_fft // 2 else 0
    return (T - n_fft) // hop + 1 if T >= n_fft else 0


def frames64(x, n_fft, hop, center=True, count=None):
    """[count, n_fft] float64: frame f is xr[f hop - pad + n], xr the reflected signal."""
    x = np.asarray(x, np.float64)
    if center:
        x = np.pad(x, n_fft // 2, mode="reflect")
    F = (len(x) - n_fft) // hop + 1 if count is None else count
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    return x[idx]


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def dft_tables64(n_fft):
    """Cw, Sw [K, n_fft]: the window folded into the DFT rows, (k n) mod n_fft in integers."""
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
    n = np.arange(n_fft, dtype=np.int64)[None, :]
    a = 2.0 * np.pi * ((k * n) % n_fft).astype(np.float64) / n_fft
    w = hann(n_fft)[None, :]
    return w * np.cos(a), -w * np.sin(a)


def power64(x, n_fft, hop, center=True, count=None):
    """[F, K]: |rfft(frame * hann)|^2."""
    spec = np.fft.rfft(frames64(x, n_fft, hop, center, count) * hann(n_fft)[None, :], axis=1)
    return spec.real ** 2 + spec.imag ** 2


def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filters64(rate, n_fft, n_mels, fmin=0.0, fmax=0.0):
    """[n_mels, K]: librosa.filters.mel(htk=False, norm="slaney")."""
    fmax = fmax or rate / 2.0
    fft_f = np.arange(n_fft // 2 + 1) * (rate / n_fft)
    pts = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(pts)
    ramps = pts[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (pts[2:n_mels + 2] - pts[:n_mels]))[:, None]


def clamp(y):
    """Whisper's normalisation of one row's features (any float dtype, kept)."""
    mx = y.max()
    return (np.maximum(y, mx - y.dtype.type(8.0)) + y.dtype.type(4.0)) * y.dtype.type(0.25)


def logmel64(x, rate, n_fft, hop, n_mels, center=True, do_clamp=False, count=None, fmin=0.0, fmax=0.0):
    """[n_mels, F] float64."""
    mel = mel_filters64(rate, n_fft, n_mels, fmin, fmax) @ power64(x, n_fft, hop, center, count).T
    y = np.log10(np.maximum(mel, FLOOR))
    return clamp(y) if do_clamp else y


def signals(T, rng):
    """The input kinds of the tests: (name, float32 [T])."""
    noise = rng.uniform(-1.0, 1.0, T).astype(np.float32)
    yield "noise", noise
    yield "constant", np.full(T, 0.75, np.float32)
    for p in (0, 1, T - 2, T - 1):  # the reflection
        x = np.zeros(T, np.float32)
        x[p] = 1.0
        yield f"impulse@{p}", x
    yield "zeros", np.zeros(T, np.float32)
    yield "tiny", (noise * np.float32(2.0 ** -120)).astype(np.float32)  # the power underflows to the floor
