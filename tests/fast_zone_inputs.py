"""Inputs for the hot-zone list at its edges (CPU only: numpy, the oracle and
tests/zone_model.py): zones of more than 64 pieces, chunks that record a
ninth zone, pieces that start inside a mono run, and a loud batch whose
counters the model gives exactly.  tests/test_zone_model_cpu.py checks the
conditions of every case here without a GPU; tests/test_gpu_fast_zones.py runs
them.

Content.  "Ordinary" granules are synth.synth_stream's (global_gain 142..177:
no granule near the hot bound).  "Loud" granules carry the alternating-sign
pattern of fast_edge_inputs._coefficients("alt") at amplitude 8 on all 576
lines and a global_gain of 200..204: hot by a wide margin, yet a good share of
their PCM stays inside +-32767 -- the suite's usual hot content (random +-15
at gain 230) clips 99.97 % of its samples, and a clipped sample cannot tell
the fast transforms from the reference's order.
"""
import numpy as np

import mp3g
import oracle
import zone_model
from fast_edge_inputs import _coefficients
from mp3g import synth

LOUD_AMP = 8
LOUD_GAINS = (200, 204)  # inclusive
# An isolated loud granule makes the granule after it hot as well, through the
# IMDCT overlap it leaves: at gain 200 that granule's ratio is ~0.95, inside
# the band the model refuses (at 202 with MS stereo off), from 204 on it is over 1.3.
ISOLATED_GAINS = (204, 206)


def make_loud(g, c, idx, rng, gains=LOUD_GAINS):
    """Granules idx of (g, c) made loud in place (module docstring), gains
    drawn from `gains` (inclusive); channel 1 of a mono granule stays empty."""
    idx = np.asarray(idx)
    pat = (_coefficients("alt", rng, len(idx), 1) * LOUD_AMP).astype(np.int16)
    mono = zone_model.nch_of(g[idx]) == 1
    pat[mono, 1] = 0
    c[idx] = pat
    gain = rng.integers(gains[0], gains[1] + 1, len(idx))
    for ch in range(2):
        C = g["ch"][:, ch]
        C["global_gain"][idx] = gain
        C["count1"][idx] = np.where(mono & (ch == 1), 0, 576)
        # flat band gains: uneven ones undo the pattern's cancellation (more
        # clipping) and pull single granules down to the hot bound
        for f in ("scalefac_l", "scalefac_s", "subblock_gain", "scalefac_scale", "preflag"):
            C[f][idx] = 0


def long_zone(n_loud, seed=1, quiet=40):
    """Three streams -- quiet, loud, quiet -- the loud one n_loud granules of
    nothing but loud content: one unbroken zone when it is one chunk."""
    rng = np.random.default_rng([seed, n_loud])
    parts = [synth.synth_stream(700 + seed, quiet // 2),
             synth.synth_stream(710 + seed, (n_loud + 1) // 2, p_event=0.05),
             synth.synth_stream(720 + seed, quiet // 2)]
    parts[1] = (parts[1][0][:n_loud], parts[1][1][:n_loud])
    g = np.concatenate([p[0] for p in parts])
    c = np.concatenate([p[1] for p in parts])
    make_loud(g, c, np.arange(quiet, quiet + n_loud), rng)
    return g, c, mp3g.streams_for([quiet, n_loud, quiet], mp3g.STATE_OUT)


def saturated_tail(n=2200, first=10, count=10, step=6, seed=2):
    """One stream of n ordinary granules with `count` isolated loud granules
    `step` apart from `first`: in one chunk, eight zones and the eighth running
    to the chunk end."""
    rng = np.random.default_rng([seed, n])
    g, c = synth.synth_stream(730 + seed, n // 2, p_event=0.05)
    make_loud(g, c, first + step * np.arange(count), rng, ISOLATED_GAINS)
    return g, c, mp3g.streams_for([n], mp3g.STATE_OUT)


def exact_saturation(lsf, per_chunk=(12, 8, 9, 0), chunk=128, first=10, step=6, seed=3):
    """One stream of len(per_chunk) * chunk granules, chunk i holding
    per_chunk[i] isolated loud granules: 12 (far past saturation), 8 (the last
    count that fits), 9 (the first that does not) and none."""
    rng = np.random.default_rng([seed, int(lsf)])
    n = chunk * len(per_chunk)
    g, c = synth.synth_stream(740 + seed, n if lsf else n // 2, lsf=lsf, p_event=0.05)
    idx = np.concatenate([i * chunk + first + step * np.arange(k) for i, k in enumerate(per_chunk)]).astype(np.int64)
    make_loud(g, c, idx, rng, ISOLATED_GAINS)
    return g, c, mp3g.streams_for([n], mp3g.STATE_OUT)


def lsf_channel_switch_stream(pattern, seed):
    """tests/test_gpu_fast.py _lsf_channel_switch_stream: an MPEG-2 LSF stream
    (one granule per frame) whose channel count follows `pattern` ('M' / 'S'
    per frame)."""
    n = len(pattern)
    mono_g, mono_c = synth.synth_stream(seed, n, mode=synth.MODE_MONO, lsf=True, p_event=0.1)
    st_g, st_c = synth.synth_stream(seed + 1, n, mode=synth.MODE_JOINT, lsf=True, p_event=0.1, p_is=0.3)
    sel = np.array([ch == "S" for ch in pattern])
    return np.where(sel, st_g, mono_g), np.where(sel[:, None, None], st_c, mono_c), sel


def mono_run(loud_in_run, lead=10, run=40, tail=39, seed=4):
    """`lead` stereo granules, a loud stereo granule, `run` mono granules, then
    stereo: the loud granule's channel-1 V waits for the first stereo granule
    after the run, so its zone spans the run (run + 2 granules) and is cut
    into pieces that start inside it.  loud_in_run: a loud mono granule in the
    middle of the run as well."""
    rng = np.random.default_rng([seed, int(loud_in_run)])
    g, c, sel = lsf_channel_switch_stream("S" * (lead + 1) + "M" * run + "S" * tail, 750 + seed)
    g, c = g.copy(), c.copy()
    make_loud(g, c, [lead] + ([lead + 1 + run // 2] if loud_in_run else []), rng, ISOLATED_GAINS)
    return g, c, mp3g.streams_for([len(g)], mp3g.STATE_OUT)


LOUD_BATCH_SEEDS = range(40, 56)
# synth.loud_granules' seed.  The only one of 1..1499 whose batch has no
# governing ratio in zone_model.BAND in the serial decode (the granule after a
# boosted one takes whatever the overlap leaves it); the replays of most
# chunkings have none either (test_zone_model_cpu.py lists the chunk counts
# that do, the cost model's on an MI355X, 86 per stream, not among them).
LOUD_BATCH_LOUD_SEED = 103


def loud_batch(loud_seed=LOUD_BATCH_LOUD_SEED):
    """tests/test_gpu_fast.py's loud batch: 16 encoded streams of 256 granules,
    6 % of the granules boosted by synth.loud_granules."""
    _, g, c, s = synth.encode_batch(LOUD_BATCH_SEEDS, 128, n_threads=4)
    g, _ = synth.loud_granules(g, 0.06, seed=loud_seed)
    s = s.copy()
    s["flags"] = mp3g.STATE_OUT
    return g, c, s


def quiet_like(g, c, seed=9):
    """A quiet input of the same shape and channel layout (the second launch of
    a plan, assertion (g)): ordinary gains, sparse small coefficients."""
    rng = np.random.default_rng(seed)
    g2 = g.copy()
    c2 = np.zeros_like(c)
    m = rng.random(c.shape) < 0.1
    c2[m] = rng.integers(-3, 4, int(m.sum()))
    c2[zone_model.nch_of(g) == 1, 1] = 0
    for ch in range(2):
        C = g2["ch"][:, ch]
        C["global_gain"] = rng.integers(150, 170, len(g))
        C["count1"] = np.where((zone_model.nch_of(g) == 1) & (ch == 1), 0, 576)
    return g2, c2


# name -> (builder, the plans' granules_per_chunk values the model covers)
CASES = {
    "long1024": (lambda: long_zone(1024), (2048,)),
    "long1025": (lambda: long_zone(1025), (2048,)),
    "long1100": (lambda: long_zone(1100), (2048,)),
    "tail2200": (lambda: saturated_tail(), (2200,)),
    "sat128_mpeg1": (lambda: exact_saturation(False), (128,)),
    "sat128_lsf": (lambda: exact_saturation(True), (128,)),
    "monorun": (lambda: mono_run(False), (90, 64, 8)),
    "monorun_loud": (lambda: mono_run(True), (90, 64, 8)),
    "loud_batch": (loud_batch, (64,)),
}
_cache = {}


def case(name):
    """(g, c, s, {granules_per_chunk: zone_model.model(...)}, info) of CASES[name],
    built once per process (read-only).  info: "pcm" / "state" the oracle's
    output, "unclipped" {granules_per_chunk: the share of oracle samples inside
    +-32767 over the rewritten granules}."""
    if name not in _cache:
        build, chunks = CASES[name]
        g, c, s = build()
        pcm, state = oracle.dsp_streams(g, c, s)
        models = {k: zone_model.model(g, c, s, k) for k in chunks}
        inside = np.abs(pcm.astype(np.int32)) < 32767
        # (channel 1 of a mono granule repeats channel 0: count it once)
        inside_g = np.where(zone_model.nch_of(g) == 1, inside[:, :, 0].mean(axis=1), inside.mean(axis=(1, 2)))
        unclipped = {k: float(inside_g[m["mask"]].mean()) if m["mask"].any() else 0.0 for k, m in models.items()}
        _cache[name] = (g, c, s, models, dict(pcm=pcm, state=state, unclipped=unclipped))
    return _cache[name]
