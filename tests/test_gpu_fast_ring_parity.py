"""The fast kernel's X ring alternates between two layouts of its 34-slot
columns (granule_fast.hip, rphys): every stereo granule that leaves a history
flips the layout instead of moving the history, a mono granule keeps the layout
and moves channel 0's history inside it, and a chunk enters in layout E.  So the
layout a granule runs in depends on where its chunk starts.

Streams of 1..6 granules of every granule kind (K P K K P K cut to the length:
the kind lands on both parities and the chunk ends on both), mono granules
inside stereo streams, all-mono streams, and one loud stereo granule at an even
and at an odd position (its hot zone is recorded in each layout), decoded with
1, 2, 3 and 4 granules per chunk: chunk starts at both parities, halos of one
and two granules, the walk-back over mono granules.  With and without an entry
state, always exporting the state, in fast mode (s16, f32, f32 planar, s16
mono) and in exact mode (the untouched v4 kernel: a guard on the shared
helpers).  Every chunking is compared bit for bit with the one-chunk decode
(PCM and exported state) -- the same granule then runs in both layouts -- and
the one-chunk decode with the oracle: within 1 LSB in fast mode, 0 in exact.
"""
import numpy as np
import pytest

import oracle
from mp3g import synth
from test_gpu_fast_loop_entry import _pools, _worst, run
from test_gpu_outfmt import as_interleaved, q
from test_gpu_outfmt_mono import as_mono, dm16

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 4, 5, 6)
CHUNKS = (1, 2, 3, 4)
ONE_CHUNK = 8  # granules per chunk >= the longest stream: one chunk per stream
MONO_IN_STEREO = ("SM", "SMS", "SSMMS", "SMMSS", "MSS")
ALL_MONO = ("M", "MM", "MMMMM", "MMMMMM")
LOUD = ("PPLPPP", "PLPPPP")  # the loud granule in layout E / in layout O of a one-chunk decode


def _batch(mp3g):
    """41 streams: 5 kinds x 6 lengths, 5 with mono granules inside, 4 all
    mono, 2 with a loud granule."""
    (g, c), (gm, cm), idx = _pools()
    gs, cs, lengths, names = [], [], [], []

    def add(take, name):
        gs.append(np.array([t[0] for t in take], dtype=g.dtype))
        cs.append(np.stack([t[1] for t in take]))
        lengths.append(len(take))
        names.append(name)

    p = idx["plain"]
    assert len(p) >= 8, f"the generator produced {len(p)} 'plain' granules"
    for kind in ("plain", "all_short", "mixed", "intensity", "line128"):
        k = idx[kind]
        picks = [k[0], p[0], k[1], k[2], p[1], k[0]]
        for n in LENGTHS:
            add([(g[i], c[i]) for i in picks[:n]], f"{kind}-{n}")
    for pat in MONO_IN_STEREO + ALL_MONO:
        add([(gm[i], cm[i]) if t == "M" else (g[p[2 + i]], c[p[2 + i]]) for i, t in enumerate(pat)], pat)
    loud, mask = synth.loud_granules(g[p[:1]], 1.0)
    assert mask.all()
    for pat in LOUD:
        add([(loud[0], c[p[0]]) if t == "L" else (g[p[1 + i]], c[p[1 + i]]) for i, t in enumerate(pat)], pat)
    gb, cb = np.concatenate(gs), np.concatenate(cs)
    assert mp3g.validate(gb, cb)[0] == 0
    # an entry state: the oracle's after 20 granules of the (stereo) pool
    _, st = oracle.dsp_streams(g[:20], c[:20], mp3g.streams_for([20], mp3g.STATE_OUT))
    return gb, cb, lengths, names, np.repeat(st, len(lengths)), loud[0]


@pytest.fixture(scope="module")
def batch(gpu):
    gb, cb, lengths, names, st, loud = _batch(gpu)
    out = {"g": gb, "c": cb, "names": names, "loud": loud}
    for with_state in (False, True):
        s = gpu.streams_for(lengths, gpu.STATE_OUT | (gpu.STATE_IN if with_state else 0))
        sin = st if with_state else None
        want, so = oracle.dsp_streams(gb, cb, s, sin)
        out[with_state] = (s, sin, want, so)
    return out


def test_batch_covers_both_layouts(gpu, batch):
    """The mono patterns are what their names say, and the loud granule sits
    once at an even and once at an odd position."""
    names = batch["names"]
    assert len(names) == 41
    g, s = batch["g"], batch[False][0]
    mono = ((g["header"] >> 6) & 3) == 3
    for pat in MONO_IN_STEREO + ALL_MONO:
        x = s[names.index(pat)]
        lo = int(x["first_granule"])
        assert "".join("M" if m else "S" for m in mono[lo:lo + int(x["n_granules"])]) == pat
    for pat in LOUD:
        lo = int(s[names.index(pat)]["first_granule"])
        loud = [g[lo + i].tobytes() == batch["loud"].tobytes() for i in range(len(pat))]
        assert loud == [t == "L" for t in pat]
    assert {LOUD[0].index("L") & 1, LOUD[1].index("L") & 1} == {0, 1}


FORMATS = {"s16": "OUT_S16", "f32": "OUT_F32", "planar": "OUT_F32_PLANAR", "s16mono": "OUT_S16_MONO"}


@pytest.mark.parametrize("with_state", [False, True], ids=["zero_state", "state_in"])
@pytest.mark.parametrize("what", ["fast-s16", "fast-f32", "fast-planar", "fast-s16mono", "exact-s16"])
def test_ring_parity(gpu, batch, what, with_state):
    mode_name, fmt_name = what.split("-")
    mode = gpu.MODE_FAST if mode_name == "fast" else gpu.MODE_EXACT
    fmt = getattr(gpu, FORMATS[fmt_name])
    tol = 1 if mode_name == "fast" else 0
    g, c, names = batch["g"], batch["c"], batch["names"]
    s, sin, want, so_want = batch[with_state]
    ref, so_ref = run(gpu, g, c, s, sin, fmt, mode, ONE_CHUNK)
    # the one-chunk decode against the oracle
    if fmt == gpu.OUT_S16_MONO:
        # (L and R within 1 LSB each: their sum within 2, its half within 1)
        got, exp = as_mono(gpu, ref, fmt, len(g)), dm16(want)
    else:
        out = as_interleaved(gpu, ref, s, fmt, len(g))
        got, exp = (out if fmt == gpu.OUT_S16 else q(out)), want
    d = np.abs(got.astype(np.int32) - exp.astype(np.int32))
    print(f"{what} {'state_in' if with_state else 'zero state'}: max |dPCM| = {d.max()} LSB, "
          f"{(d > 0).mean():.4%} of samples differ")
    assert d.max() <= tol, f"{what}: max |dPCM| per stream {_worst(d, s, names)} (> {tol})"
    if mode_name == "exact":
        assert so_ref.tobytes() == so_want.tobytes(), "exact mode: the exported state differs from the oracle's"
    # every chunking against the one-chunk decode: bit-identical
    for chunk in CHUNKS:
        raw, so = run(gpu, g, c, s, sin, fmt, mode, chunk)
        if not np.array_equal(raw, ref):
            w = gpu.out_bytes_per_granule(fmt) // 4
            if fmt == gpu.OUT_F32_PLANAR:
                bad = "(planar)"
            else:
                rows = np.nonzero((raw != ref).reshape(len(g), w).any(axis=1))[0]
                first = np.asarray(s["first_granule"], np.int64)
                bad = sorted({names[int(np.searchsorted(first, r, side="right")) - 1] for r in rows})
            raise AssertionError(f"{what} chunk={chunk}: PCM differs from the one-chunk decode in {bad}")
        bad = [n for n, a, b in zip(names, so, so_ref) if a.tobytes() != b.tobytes()]
        assert not bad, f"{what} chunk={chunk}: exported state differs in {bad}"
