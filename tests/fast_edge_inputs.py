"""Inputs at the fast mode's hot-granule thresholds (CPU only: the oracle and
numpy, nothing of the GPU library but its constants and dtypes).

The fast kernel keeps a granule on its reassociated transforms unless
max |S| > kHotS AND some time slot's sum of |S| over the 32 subbands exceeds
kHotL1 (granule_fast.hip; S = the hybrid output the matrixing reads).  Its
+-1 LSB promise is a measurement below that bound, so the inputs that matter
are the ones just under it.  edge_batch() builds them: per stream it picks the
coefficient amplitude a and the global_gain that put the stream's governing
quantity

    r_A = max |S| / kHotS          (first level: fast because no line
                                    exceeds kHotS)
    r_B = max slot sum / kHotL1    (second level: lines above kHotS, but no
                                    slot's sum above kHotL1)

-- per granule the smaller of the two (the test that keeps it fast), per
stream the largest of that over its granules (the granule nearest to hot) --

as close under 1 - MARGIN as the grid a^(4/3) 2^(gg/4) allows, from the
oracle's own S at gain 210 scaled by 2^((gg - 210) / 4), and verifies the
choice with a second oracle pass at the final gain.  side="over" is the same batch one gain step
(2^(1/4)) higher: then some granule of every stream is over both bounds.

tools/adversarial_tolerance.py (the large search) and the tests
(tests/test_fast_edge_inputs_cpu.py, tests/test_gpu_fast_threshold.py) build
their inputs here.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import mp3g
import oracle
from mp3g import synth

MARGIN = 1e-3  # relative distance kept from a bound (and the width of the hot-flag bands)
BASE_GAIN = 210  # global_gain with a unit requantize scale (2^((gg - 210) / 4))
SIGN_KINDS = ("rand", "alt", "altsb", "low")  # +-a on every (rand, alt, altsb) or the low 72 lines
SPIKE_KINDS = ("spike", "spike_zero", "spike_rand")  # spike: even streams over zeros, odd over random -2..2
KINDS = SIGN_KINDS + ("p43edge",) + SPIKE_KINDS
VARIANTS = ("long", "short", "mixed", "ms", "mono", "bandgain", "bandgain_short")
SPIKES = np.array([3000, 5000, 8206])
DRAWS = 4  # candidate draws per stream of the kinds without an amplitude (p43edge, spikes)


def _descriptors(variant, n_streams, frames, rng):
    """Granule descriptors of `variant` with global_gain = BASE_GAIN, count1 = 576."""
    mono = variant == "mono"
    n = n_streams * 2 * frames
    g = np.zeros(n, mp3g.GRANULE_DTYPE)  # MPEG-1: two granules per frame
    g["gr"] = np.tile(np.arange(2), n // 2)
    if variant == "ms":
        g["header"] = synth.header(synth.MODE_JOINT, ms=True)
    else:
        g["header"] = synth.header(synth.MODE_MONO if mono else synth.MODE_STEREO)
    for ch in range(1 if mono else 2):
        C = g["ch"][:, ch]
        C["global_gain"] = BASE_GAIN
        C["count1"] = 576
        C["scalefac_l"] = 0
        C["scalefac_s"] = 0
        C["scalefac_scale"] = 0
        C["preflag"] = 0
        C["subblock_gain"] = 0
        if variant in ("short", "mixed", "bandgain_short"):
            C["win_switch_flag"] = 1
            C["block_type"] = 2
            C["mixed_block_flag"] = 1 if variant == "mixed" else 0
        else:
            C["win_switch_flag"] = 0
            C["block_type"] = 0
            C["mixed_block_flag"] = 0
        if variant in ("bandgain", "bandgain_short"):
            # scale factors over the whole range their slen allows (scalefac_compress
            # picks (slen1, slen2), maindata.go), a quarter of them at its maximum
            sc = rng.integers(0, 16, n)
            lim1 = (1 << synth.SLEN_MPEG1[sc, 0]) - 1
            lim2 = (1 << synth.SLEN_MPEG1[sc, 1]) - 1
            C["scalefac_scale"] = rng.integers(0, 2, n)
            if variant == "bandgain":
                lim = np.where(np.arange(22)[None, :] < 11, lim1[:, None], lim2[:, None])
                sf = rng.integers(0, lim + 1)
                sf = np.where(rng.random(sf.shape) < 0.25, lim, sf)
                sf[:, 21] = 0
                C["scalefac_l"] = sf
                C["preflag"] = rng.integers(0, 2, n)
            else:
                lim = np.where(np.arange(13)[None, :, None] < 6, lim1[:, None, None], lim2[:, None, None])
                lim = np.broadcast_to(lim, (n, 13, 3))
                sf = rng.integers(0, lim + 1)
                sf = np.where(rng.random(sf.shape) < 0.25, lim, sf)
                sf[:, 12, :] = 0
                C["scalefac_s"] = sf
                C["subblock_gain"] = rng.integers(0, 8, (n, 3))
    return g


def _coefficients(kind, rng, n, per):
    """One draw of the pattern, int64 [n, 2, 576]: the sign kinds as signs
    (times the amplitude a later), the others as values."""
    i = np.arange(576)
    ones = np.ones((n, 2, 1), np.int64)
    if kind == "rand":
        return rng.choice([-1, 1], size=(n, 2, 576))
    if kind == "alt":
        return np.where(i % 2 == 0, 1, -1) * ones
    if kind == "altsb":
        return np.where((i // 18) % 2 == 0, 1, -1) * ones
    if kind == "low":
        c = np.zeros((n, 2, 576), np.int64)
        c[:, :, :72] = rng.choice([-1, 1], size=(n, 2, 72))
        return c
    odd = ((np.arange(n) // per) % 2 == 1)[:, None, None]  # odd streams
    if kind == "p43edge":  # around the edge of the fast kernel's x^(4/3) table (|x| <= 127 / -128)
        mag = np.where(odd, rng.integers(128, 136, size=(n, 2, 576)), rng.integers(120, 128, size=(n, 2, 576)))
        return mag * rng.choice([-1, 1], size=(n, 2, 576))
    bg = rng.integers(-2, 3, size=(n, 2, 576))
    c = {"spike": np.where(odd, bg, 0), "spike_zero": np.zeros_like(bg), "spike_rand": bg}[kind].copy()
    pos = np.argsort(rng.random((n, 2, 576)), axis=2)[:, :, :3]
    val = rng.choice(SPIKES, size=(n, 2, 3)) * rng.choice([-1, 1], size=(n, 2, 3))
    np.put_along_axis(c, pos, val, axis=2)
    return c


def _by_stream(fn, g, c, s, threads=16):
    """fn(granules, coeffs, streams) -> tuple of arrays (per granule first,
    per stream after), large batches split by stream over host threads (ctypes
    drops the GIL; the streams are independent and lie in order)."""
    if len(s) < 4 * threads:
        return fn(g, c, s)

    def one(idx):
        ss = s[idx].copy()
        lo = int(ss["first_granule"][0])
        hi = int(ss["first_granule"][-1] + ss["n_granules"][-1])
        ss["first_granule"] -= lo
        return fn(g[lo:hi], c[lo:hi], ss)

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, np.array_split(np.arange(len(s)), threads)))
    return tuple(np.concatenate(p) for p in zip(*parts))


def stream_ratios(g, c, s, hot_s=None, hot_l1=None):
    """The oracle's S of the batch against the bounds: per granule
    (r_A, r_B) = (max |S| / kHotS, max slot sum / kHotL1) over the channels the
    granule has, and their per-stream maxima."""
    hot_s = mp3g.FAST_HOT_S if hot_s is None else hot_s
    hot_l1 = mp3g.FAST_HOT_L1 if hot_l1 is None else hot_l1
    n = len(g)
    S = np.abs(_by_stream(lambda *a: (oracle.hybrid_streams(*a),), g, c, s)[0]).reshape(n, 2, 32, 18)
    S[((g["header"] >> 6) & 3) == 3, 1] = 0  # a mono granule has no channel 1
    ra = S.max(axis=(1, 2, 3)).astype(np.float64) / hot_s
    rb = S.sum(axis=2, dtype=np.float64).max(axis=(1, 2)) / hot_l1
    first = s["first_granule"].astype(np.int64)
    return ra, rb, np.maximum.reduceat(ra, first), np.maximum.reduceat(rb, first)


def _set_gain(g, gg, per):
    for ch in range(2):
        g["ch"]["global_gain"][:, ch] = np.repeat(gg, per)


def edge_batch(kind, variant, side, n_streams=64, frames=2, seed=1, amps=None, hot_s=None, hot_l1=None):
    """(granules, coeffs int16 [n, 2, 576], streams, info): n_streams streams of
    2 * frames granules of `kind` x `variant` at the thresholds (module
    docstring).  Deterministic in its arguments.  amps: the amplitudes the
    sign kinds search (default 1..15); hot_s / hot_l1: the bounds, by default
    the library's (mp3g.FAST_HOT_S / FAST_HOT_L1).

    info: "ratio" [n_streams] the governing quantity over its bound, "level"
    [n_streams] 0 = first level (max |S|) / 1 = second (slot sums), "a" (the
    amplitude; the draw taken for p43edge and the spikes) and "gain" the choice, "r_a" / "r_b" per granule, "hot" / "hot_hi" / "hot_lo"
    per granule: over both bounds strictly / by more than 1 + MARGIN / by more
    than 1 - MARGIN, "pcm" and "state" the oracle's output, "unclipped" the
    share of its samples inside +-32767."""
    assert kind in KINDS and variant in VARIANTS and side in ("under", "over"), (kind, variant, side)
    assert kind != "p43edge" or variant in ("long", "ms", "mono", "bandgain"), "p43edge: long blocks only"
    hot_s = mp3g.FAST_HOT_S if hot_s is None else hot_s
    hot_l1 = mp3g.FAST_HOT_L1 if hot_l1 is None else hot_l1
    rng = np.random.default_rng([seed, KINDS.index(kind), VARIANTS.index(variant)])
    per = 2 * frames
    g = _descriptors(variant, n_streams, frames, rng)
    n = len(g)
    s = mp3g.streams_for([per] * n_streams, mp3g.STATE_OUT)
    amps = np.arange(1, 16) if amps is None else np.asarray(amps)
    if kind in SIGN_KINDS:
        unit = _coefficients(kind, rng, n, per)
        cands = [(unit * a).astype(np.int16) for a in amps]
    else:
        # no amplitude to search: DRAWS independent draws of the pattern per
        # stream instead (the gain step alone leaves the ratio anywhere in
        # 2^(-1/4) .. 1, and a stream just above 2^(-1/4) has no "over" side)
        amps = np.arange(DRAWS)
        cands = [_coefficients(kind, rng, n, per).astype(np.int16) for _ in amps]
    if variant == "mono":
        for cand in cands:
            cand[:, 1] = 0
    # S at BASE_GAIN per candidate; gain gg scales it by 2^((gg - 210) / 4)
    # (to float32 rounding: the second oracle pass below is what counts)
    base = [stream_ratios(g, cand, s, hot_s, hot_l1) for cand in cands]
    ra_g = np.stack([b[0] for b in base]).reshape(len(amps), n_streams, per)
    rb_g = np.stack([b[1] for b in base]).reshape(len(amps), n_streams, per)
    gains = np.arange(0, 255)  # "over" is one step higher and stays <= 255
    f = 2.0 ** ((gains - BASE_GAIN) / 4.0)
    lim = (1.0 - MARGIN) * (1.0 - 1e-5)
    # a granule is fast while min(r_A, r_B) <= 1: the stream's governing
    # quantity is the largest of that over its granules, [amps, streams, gains]
    gov = np.minimum(ra_g, rb_g)
    score = gov.max(axis=2)[..., None] * f
    # (<= lim: under the bound.  One gain step up that granule should be over
    # both bounds by more than the band, for side="over": choices that are not
    # -- ratios within 0.3 % of 2^(-1/4) -- rank below all that are, and are
    # taken only by a stream with nothing else, e.g. a single amplitude)
    score = np.where(score <= lim, np.where(score * 2.0 ** 0.25 > 1.0 + 2 * MARGIN, score, score - 2.0), -10.0)
    for _ in range(4):
        flat = score.transpose(1, 0, 2).reshape(n_streams, -1)
        best = flat.argmax(axis=1)
        assert (flat[np.arange(n_streams), best] > -5).all(), f"{kind}/{variant}: a stream has no valid (a, gain)"
        ai, gi = np.unravel_index(best, (len(amps), len(gains)))
        a, gg = amps[ai], gains[gi]
        pick = np.repeat(ai, per)
        c = np.zeros((n, 2, 576), np.int16)
        for k, cand in enumerate(cands):
            c[pick == k] = cand[pick == k]
        _set_gain(g, gg, per)
        ra, rb, _, _ = stream_ratios(g, c, s, hot_s, hot_l1)  # the second pass, at the final gain
        gov = np.minimum(ra, rb).reshape(n_streams, per)
        top = gov.argmax(axis=1) + per * np.arange(n_streams)  # the granule that governs its stream
        ratio = gov.max(axis=1)
        level = (rb[top] < ra[top]).astype(np.int8)
        bad = ratio > 1.0 - MARGIN
        if not bad.any():
            break
        score[ai[bad], np.nonzero(bad)[0], gi[bad]] = -10.0  # rounding put it over: the next best choice
    else:
        raise AssertionError(f"{kind}/{variant}: no choice verified under the bound")
    if side == "over":
        gg = gg + 1
        _set_gain(g, gg, per)
        ra, rb, _, _ = stream_ratios(g, c, s, hot_s, hot_l1)
        ratio = np.minimum(ra, rb).reshape(n_streams, per).max(axis=1)
    pcm, state = _by_stream(oracle.dsp_streams, g, c, s)
    info = {
        "ratio": ratio, "level": level, "a": a, "gain": gg, "r_a": ra, "r_b": rb,
        "hot": (ra > 1.0) & (rb > 1.0),
        "hot_hi": (ra > 1.0 + MARGIN) & (rb > 1.0 + MARGIN),
        "hot_lo": (ra > 1.0 - MARGIN) & (rb > 1.0 - MARGIN),
        "pcm": pcm, "state": state,
        "unclipped": float((np.abs(pcm.astype(np.int32)) < 32767).mean()),
    }
    return g, c, s, info


# The (kind, variant) grid of the tests: every kind on long blocks, every
# variant with a second-level (rand) and a first-level (altsb) pattern, and
# the table-edge / spike / low patterns on the variants that change their path.
CASES = [(k, "long") for k in ("rand", "alt", "altsb", "low", "p43edge", "spike")] + \
        [(k, v) for v in VARIANTS[1:] for k in ("rand", "altsb")] + \
        [("low", "mono"), ("low", "bandgain"), ("spike", "short"), ("spike", "bandgain_short"),
         ("p43edge", "ms"), ("p43edge", "bandgain")]
_cache = {}


def edge_case(kind, variant, side):
    """edge_batch(kind, variant, side) at the tests' size, built once per process
    (treat what it returns as read-only)."""
    key = (kind, variant, side)
    if key not in _cache:
        _cache[key] = edge_batch(kind, variant, side, seed=1 + CASES.index((kind, variant)))
    return _cache[key]
