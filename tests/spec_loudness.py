"""An independent float64 statement of ITU-R BS.1770-4 integrated loudness
(include/mp3g.h "Integrated loudness of decoded rows"): the K-weighting designed
from its analog prototypes, scipy.signal.lfilter run SEQUENTIALLY over the whole
row (no segment decomposition), numpy block sums and gates, np.log10.  Shares no
code with the library."""
import numpy as np
from scipy.signal import lfilter

ABS_GATE = 10.0 ** -6.9309  # -70 LUFS as a mean-square energy

# the standard's table 1 and 2 (48 kHz), as printed
BS1770_48K = {"shelf_b": [1.53512485958697, -2.69169618940638, 1.19839281085285],
              "shelf_a": [1.0, -1.69065929318241, 0.73248077421585],
              "highpass_b": [1.0, -2.0, 1.0],
              "highpass_a": [1.0, -1.99004745483398, 0.99007225036621]}


def k_weighting(rate):
    """((b, a) of the shelf, (b, a) of the high-pass) in float64."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = (np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]),
             np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / rate)
    a0 = 1.0 + K / Q + K * K
    highpass = (np.array([1.0, -2.0, 1.0]), np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]))
    return shelf, highpass


def segment(rate):
    """Samples in 100 ms, as libebur128 counts them."""
    return (rate + 5) // 10


def block_energies(x, rate, length=None):
    """z_i of the row x [C, T] (or [T]) over its first `length` samples."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = x.shape[-1] if length is None else min(int(length), x.shape[-1])
    H = segment(rate)
    nseg = n // H
    nb = nseg - 3 if nseg >= 4 else 0
    if nb == 0:
        return np.zeros(0)
    shelf, highpass = k_weighting(rate)
    z = np.zeros(nb)
    for ch in x:
        w = lfilter(highpass[0], highpass[1], lfilter(shelf[0], shelf[1], ch[:nseg * H]))
        e = (w * w).reshape(nseg, H).sum(axis=1)
        z += (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * H)
    return z


def gate_margin(z):
    """The smallest relative distance of a block energy to either gate."""
    if len(z) == 0:
        return np.inf
    m = np.abs(z / ABS_GATE - 1.0).min()
    a = z[z >= ABS_GATE]
    if len(a):
        rel = 0.1 * a.mean()
        m = min(m, np.abs(a / rel - 1.0).min())
    return m


def integrated(x, rate, length=None):
    """dict(energy, lufs, peak, n_blocks, n_abs, n_gated) of one row."""
    xx = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n = xx.shape[-1] if length is None else min(int(length), xx.shape[-1])
    z = block_energies(xx, rate, n)
    a = z[z >= ABS_GATE]
    g = a[a >= 0.1 * a.mean()] if len(a) else a
    energy = float(g.mean()) if len(g) else 0.0
    return {"energy": energy, "lufs": -0.691 + 10.0 * np.log10(energy) if energy > 0 else -np.inf,
            "peak": float(np.abs(xx[:, :n]).max()) if n else 0.0,
            "n_blocks": len(z), "n_abs": len(a), "n_gated": len(g)}
