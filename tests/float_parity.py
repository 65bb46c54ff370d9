"""Float-domain parity against the float64 decode of tests/spec_dsp.py: the one
metric, the case list and the caps (a plain module, shared by
tests/test_spec_reference.py and tests/test_gpu_float_parity.py).

Units.  Everything is in int16 LSBs: the spec's `val` (unclamped), the oracle's
t = sum * 32767.0f (oracle.dsp_streams_float) and a product float sample times
32768.  The truth is v = clip(val, -32767, 32767); a candidate x is
clip(t) for the oracle and f * 32768 for the product.  The reference float
sample (include/mp3g.h, "Output formats") is f_ref = float32(clip(t)) * 2^-15,
an exact scaling, so f_ref * 32768 = clip(t).

Metric, over one case (stream_metrics):
  e            = x - v
  scale[k, ch] = max(max|val[k, :, ch]|, max|val[k - 1, :, ch]|) within a stream
                 (the previous granule's V history enters the first 15 slots of
                 this one); at a stream start the granule's own peak
  scale == 0  -> e must be 0 on that granule-channel; it is left out
  rel_rms      = sqrt(mean e^2) / sqrt(mean val^2)
  max_rel      = max |e| / scale
Both ratios are invariant under a common scaling of x and val: they see the
same thing at -120 dB as at full scale.  store_metrics is the same pair for the
exported overlap store, per stream and channel relative to max|store|.

Why the magnitudes come from the unclamped val.  Wherever a sample does not
clip, |val| = |v| and this is the metric on v itself.  A float32 rounding error
is proportional to the terms summed, though, not to what the clamp leaves of
them: the hot-granule cases (global_gain 230) overdrive the output by up to
10^3, most samples clamp to +-32767 with e = 0, and the few that land inside
the range carry the rounding error of sums 10^3 times as large.  Against the
clamped peak the oracle itself shows max_rel = 5.9e-3 there (8.7e-4 on the
scattered-hot case), three orders above every other case, and one cap over
the case list would be blind to the 1e-5 constant error this check exists to
catch; against |val| the same cases show 2.0e-7 and 1.0e-6, as every other.
"""
import functools

import numpy as np

import oracle
import spec_dsp
from mp3g import synth
from test_gpu_parity import SYNTH_CASES

CLIP = 32767.0
N_STREAMS, N_FRAMES = 2, 24  # every case; the float64 spec takes ~0.1 s per stream

# ---- caps: 2.5 x the worst value the oracle shows over CASES (the table below) ----------------
#
# Oracle (gcc -O2 -ffp-contract=off, glibc) against the float64 spec, measured on
# the CPU over the two streams of every case (tests/test_spec_reference.py
# prints the same figures):
#
#   case               rel_rms    max_rel   store rel_rms  store max_rel
#   dual                2.68e-07   1.06e-06    3.39e-07      5.16e-07
#   joint_all_is        3.99e-07   1.01e-06    1.71e-07      3.79e-07
#   joint_mixed         4.48e-07   1.03e-06    3.71e-07      4.57e-07
#   joint_ms_is         3.48e-07   1.12e-06    1.96e-07      2.73e-07
#   mono                5.12e-07   1.06e-06    3.05e-07      3.70e-07
#   mpeg1_32k           4.00e-07   9.78e-07    3.03e-07      3.79e-07
#   mpeg1_48k           2.57e-07   1.04e-06    2.49e-07      3.79e-07
#   mpeg2_16k           5.26e-07   1.15e-06    3.41e-07      4.77e-07
#   mpeg2_24k           5.27e-07   1.07e-06    3.41e-07      4.77e-07
#   mpeg2_joint         3.94e-07   8.11e-07    3.78e-07      3.89e-07
#   mpeg2_mono          4.64e-07   8.50e-07    2.24e-07      2.04e-07
#   stereo              3.35e-07   1.02e-06    5.37e-07      5.59e-07
#   all_short_joint     8.54e-08   5.04e-07    9.31e-08      1.50e-07
#   all_short_mono      7.54e-08   5.58e-07    9.34e-08      2.12e-07
#   gain_m40            4.98e-07   1.02e-06    2.39e-07      3.24e-07
#   gain_m80            4.98e-07   1.02e-06    2.39e-07      3.24e-07
#   gain_m120           4.98e-07   1.02e-06    2.39e-07      3.24e-07
#   requant_table_edge  3.28e-07   1.20e-06    8.55e-08      6.28e-07
#   sparse_linbits      1.86e-07   6.33e-07    1.94e-07      4.44e-07
#   scattered_hot       1.25e-09   9.95e-07    3.80e-07      4.73e-07
#   all_hot             4.28e-09   2.04e-07    3.69e-07      5.22e-07
#   worst               5.27e-07   1.20e-06    5.37e-07      6.28e-07
#
# (On the two hot cases rel_rms is diluted by the overdriven samples' own
# magnitude; max_rel is per granule-channel and is not.)
SAMPLE_WORST_RMS, SAMPLE_WORST_MAX = 5.27e-7, 1.20e-6
STORE_WORST_RMS, STORE_WORST_MAX = 5.37e-7, 6.28e-7
CAP_RMS, CAP_MAX = 2.5 * SAMPLE_WORST_RMS, 2.5 * SAMPLE_WORST_MAX
STORE_CAP_RMS, STORE_CAP_MAX = 2.5 * STORE_WORST_RMS, 2.5 * STORE_WORST_MAX


# ---- the metric -------------------------------------------------------------------------------

def clip(val):
    return np.clip(np.asarray(val, np.float64), -CLIP, CLIP)


def f_ref(t):
    """The float32 sample the product must write for the oracle's product t."""
    return (np.clip(np.asarray(t, np.float32), np.float32(-CLIP), np.float32(CLIP)) *
            np.float32(2.0 ** -15)).astype(np.float32)


def downmix_f32(f):
    """MP3G_OUT_F32_MONO's rule on [..., 2] float32 samples, in float32."""
    f = np.asarray(f, np.float32)
    return ((f[..., 0] + f[..., 1]) * np.float32(0.5)).astype(np.float32)


def mono_truth(val):
    """The float64 truth of the mono downmix: (vL + vR) / 2 of the clamped samples."""
    v = clip(val)
    return (v[..., 0] + v[..., 1]) * 0.5


def magnitude(val):
    """|val| of the unclamped truth [n, 576, 2]: what scale and the RMS denominator
    are taken from (|v| wherever the sample does not clip)."""
    return np.abs(np.asarray(val, np.float64))


def mono_magnitude(val):
    """The same for the mono downmix: |(vL + vR) / 2| where neither channel clips,
    the larger |val| of the two channels where one does."""
    a = np.abs(np.asarray(val, np.float64))
    return np.where((a > CLIP).any(axis=-1), a.max(axis=-1), np.abs(mono_truth(val)))


def granule_scale(mag, streams):
    """scale[k, ch] of the magnitudes [n, 576, C] (see the module docstring)."""
    peak = mag.max(axis=1)
    scale = peak.copy()
    for s in streams:
        lo, n = int(s["first_granule"]), int(s["n_granules"])
        if n > 1:
            scale[lo + 1:lo + n] = np.maximum(peak[lo + 1:lo + n], peak[lo:lo + n - 1])
    return scale


def stream_metrics(x, v, streams, mag=None):
    """(rel_rms, max_rel, per [n, C] array of max|e| / scale) of the candidate x
    against the clamped truth v, both [n, 576] or [n, 576, C] in LSBs; mag is
    magnitude(val) / mono_magnitude(val) of the unclamped truth (default |v|:
    nothing clips).  Raises AssertionError where a silent granule-channel is
    not silent in x."""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    mag = np.abs(v) if mag is None else np.asarray(mag, np.float64)
    if x.ndim == 2:
        x, v, mag = x[..., None], v[..., None], mag[..., None]
    assert x.shape == v.shape == mag.shape, (x.shape, v.shape, mag.shape)
    e = x - v
    scale = granule_scale(mag, streams)
    emax = np.abs(e).max(axis=1)
    silent = scale == 0
    assert not emax[silent].any(), f"non-zero samples on {int((emax[silent] > 0).sum())} silent granule-channels"
    per = np.zeros_like(scale)
    per[~silent] = emax[~silent] / scale[~silent]
    sv = float((mag ** 2).sum())
    rel_rms = float(np.sqrt((e ** 2).sum() / sv)) if sv else 0.0
    return rel_rms, float(per.max(initial=0.0)), per


def store_metrics(x, v):
    """The same pair for overlap stores [n_streams, 2, 32, 18]: the error relative
    to max|store| of the stream's channel."""
    x, v = np.asarray(x, np.float64), np.asarray(v, np.float64)
    assert x.shape == v.shape, (x.shape, v.shape)
    e = x - v
    scale = np.abs(v).max(axis=(2, 3))
    emax = np.abs(e).max(axis=(2, 3))
    silent = scale == 0
    assert not emax[silent].any(), "non-zero store of a silent channel"
    per = np.zeros_like(scale)
    per[~silent] = emax[~silent] / scale[~silent]
    sv = float((v ** 2).sum())
    rel_rms = float(np.sqrt((e ** 2).sum() / sv)) if sv else 0.0
    return rel_rms, float(per.max(initial=0.0))


# ---- the case list ----------------------------------------------------------------------------

def _batch(seed, **kw):
    g, c, s = synth.synth_batch(N_STREAMS, N_FRAMES, seed=seed, **kw)
    s["flags"] = 2  # MP3G_STREAM_STATE_OUT
    return g, c, s


def _synth_case(name):
    return lambda: _batch(100 + len(name), **SYNTH_CASES[name])


def _all_short(mode):
    """tests/test_gpu_fast.py, test_all_short_blocks."""
    g, c, s = _batch(21, mode=mode, p_is=0.5)
    ch = g["ch"]
    ch["win_switch_flag"] = 1
    ch["block_type"] = 2
    ch["mixed_block_flag"] = 0
    return g, c, s


def _gain_shift(shift):
    """A mixed / intensity-stereo / short-block stream with every global_gain
    moved by `shift` quarter-octaves: -40 is 2^-10 in amplitude (a few LSBs
    left), -80 and -120 leave an s16 PCM of zeros."""
    g, c, s = _batch(33, p_mixed=0.5, p_is=0.6, p_event=0.1)
    gg = g["ch"]["global_gain"].astype(np.int32) + shift
    assert gg.min() >= 0
    g["ch"]["global_gain"] = gg.astype(np.uint8)
    return g, c, s


def _requant_table_edge():
    """tests/test_gpu_fast.py, test_fast_requant_table_edge."""
    g, c, s = _batch(9, p_event=0.0)
    ch = g["ch"]
    assert not (ch["block_type"] == 2).any()
    ch["count1"] = 576
    ch["global_gain"] = 134
    rng = np.random.default_rng(4)
    inside = np.array([-128, -127, -126, -2, -1, 1, 2, 126, 127], np.int16)
    outside = np.array([-8206, -300, -129, 128, 129, 255, 256, 8206], np.int16)
    c[:] = 0
    for i in range(len(g)):
        m = rng.random(c[i].shape) < 0.05
        c[i][m] = rng.choice(inside, size=int(m.sum()))
        if i % 2:
            m = rng.random(c[i].shape) < 0.004
            c[i][m] = rng.choice(outside, size=int(m.sum()))
    return g, c, s


def _sparse_linbits():
    """tests/test_gpu_fast.py, test_fast_sparse_linbits_spikes."""
    rng = np.random.default_rng(21)
    g, c, s = _batch(57)
    for gi in range(len(g)):
        for ch in range(2):
            n1 = int(g["ch"]["count1"][gi, ch])
            pos = rng.choice(np.arange(n1) if n1 > 3 else np.arange(3), size=3, replace=False)
            c[gi, ch, pos] = rng.choice([-8206, -3000, 3000, 8206], size=3)
            g["ch"]["count1"][gi, ch] = max(n1, int(pos.max()) + 1)
    g["ch"]["global_gain"] = 150
    return g, c, s


def _scattered_hot():
    """tests/test_gpu_fast.py, test_fast_hot_granules (rand15 at global_gain 230),
    on 2 x 48 granules: isolated, in a run, at stream starts and ends."""
    rng = np.random.default_rng(230 + 6)
    g, c, s = _batch(55, p_mixed=0.3, p_event=0.1, p_is=0.3)
    idx = np.array([0, 5, 17, 18, 19, 40, 47, 48, 49, 70, 95])
    for ch in range(2):
        C = g["ch"][:, ch]
        C["global_gain"][idx] = 230
        C["count1"][idx] = 576
    c[idx] = rng.integers(-15, 16, size=(len(idx), 2, 576))
    return g, c, s


def _all_hot():
    """tests/test_gpu_fast.py, test_fast_all_hot_is_reference_order."""
    rng = np.random.default_rng(8)
    g, c, s = _batch(66, p_event=0.1)
    g["ch"]["global_gain"] = 230
    g["ch"]["count1"] = 576
    c[:] = rng.integers(-15, 16, size=c.shape)
    return g, c, s


CASES = {name: _synth_case(name) for name in sorted(SYNTH_CASES)}
CASES.update({
    "all_short_joint": lambda: _all_short(synth.MODE_JOINT),
    "all_short_mono": lambda: _all_short(synth.MODE_MONO),
    "gain_m40": lambda: _gain_shift(-40),
    "gain_m80": lambda: _gain_shift(-80),
    "gain_m120": lambda: _gain_shift(-120),
    "requant_table_edge": _requant_table_edge,
    "sparse_linbits": _sparse_linbits,
    "scattered_hot": _scattered_hot,
    "all_hot": _all_hot,
})
QUIET_CASES = ("gain_m80", "gain_m120")  # the s16 PCM is all zeros


def spec_streams(g, c, s, synth_d):
    """spec_dsp.spec_decode_float stream by stream: (val [n, 576, 2], store [n_streams, 2, 32, 18])."""
    val = np.zeros((len(g), 576, 2))
    store = np.zeros((len(s), 2, 32, 18))
    for k, st in enumerate(s):
        lo, n = int(st["first_granule"]), int(st["n_granules"])
        val[lo:lo + n], store[k] = spec_dsp.spec_decode_float(g[lo:lo + n], c[lo:lo + n], synth_d)
    return val, store


class Case:
    """One case's input, its float64 truth and the oracle's own figures, computed
    once per process and never written to."""

    def __init__(self, name):
        self.name = name
        self.g, self.c, self.s = CASES[name]()
        self.val, self.store = spec_streams(self.g, self.c, self.s, oracle.tables()["synth_d"].astype(np.float64))
        self.v = clip(self.val)
        self.t, self.state = oracle.dsp_streams_float(self.g, self.c, self.s)
        self.f_ref = f_ref(self.t)
        self.mono = ((self.g["header"] >> 6) & 3) == 3
        # the oracle's own error: stereo samples, the float32 downmix, the store
        x = self.f_ref.astype(np.float64) * 32768.0
        self.mag = magnitude(self.val)
        self.ref_rms, self.ref_max, self.ref_per = stream_metrics(x, self.v, self.s, self.mag)
        self.mono_ref = downmix_f32(self.f_ref)
        self.mono_ref[self.mono] = self.f_ref[self.mono][..., 0]
        self.mono_v, self.mono_mag = mono_truth(self.val), mono_magnitude(self.val)
        self.ref_mono_rms, self.ref_mono_max, _ = stream_metrics(self.mono_ref.astype(np.float64) * 32768.0,
                                                                 self.mono_v, self.s, self.mono_mag)
        self.ref_store_rms, self.ref_store_max = store_metrics(self.state["store"], self.store)
        for a in (self.val, self.v, self.t, self.f_ref, self.mono_ref, self.mono_v,
                  self.mag, self.mono_mag, self.store, self.state):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
