"""The hand-over from a chunk's prologue to its granule loop (granule_fast.hip,
granule_wexact.hip): the prologue loads the first granule's coefficients and
the first two descriptors and settles them before the loop, and the loop's
first pass consumes those registers -- on the all-long path, or on one of the
paths that read them first in another way (short-block staging, the descriptor
dropped into LDS for short blocks and intensity stereo, the arithmetic redo of
a line outside the p43 table, a mono granule's frozen channel).

Streams of 1, 2, 3 and 5 granules decoded with 1, 2 and 3 granules per chunk:
chunks whose loop runs once, chunks with and without a halo, and the last
granule's prefetch past the chunk (no records).  Every stream starts with the
granule kind it is named after (and repeats it at the later chunk starts), with
and without an entry state, in fast mode (s16 and both float formats) and in
exact mode.  Each decode is compared bit for bit with the same streams decoded
as one chunk each (PCM and exported state) and with the oracle: within 1 LSB
in fast mode (its contract, tests/test_gpu_fast.py), 0 in exact mode.
"""
import numpy as np
import pytest

import oracle
from mp3g import synth
from test_gpu_outfmt import as_interleaved, q

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 5)
CHUNKS = (1, 2, 3)
ONE_CHUNK = 8  # granules per chunk >= the longest stream: one chunk per stream


def _is_short(c):
    return (c["win_switch_flag"] == 1) & (c["block_type"] == 2)


def _pools():
    """Granules by kind, taken from synth's branch generators."""
    g, c = synth.synth_stream(71, 100, p_event=0.15, p_mixed=0.5, p_is=0.5)
    gm, cm = synth.synth_stream(72, 10, mode=synth.MODE_MONO)
    ch = g["ch"]
    short = _is_short(ch)                      # [n, 2]
    mixed = short & (ch["mixed_block_flag"] == 1)
    any_short = short.any(axis=1)
    isg = (g["header"] & 0x10) != 0            # joint stereo with intensity stereo on
    big = (np.abs(c.astype(np.int32)) >= 128).any(axis=(1, 2))
    kinds = {
        "plain": ~any_short & ~isg & ~big,
        "all_short": short.all(axis=1) & ~mixed.any(axis=1),
        "mixed": mixed.any(axis=1),
        "intensity": isg & ~any_short,
        "line128": big & ~any_short,
    }
    idx = {k: np.nonzero(v)[0] for k, v in kinds.items()}
    for k, v in idx.items():
        assert len(v) >= 3, f"the generator produced {len(v)} '{k}' granules"
    return (g, c), (gm, cm), idx


def _batch(mp3g):
    """24 streams: 6 kinds x 4 lengths.  Kind K (P = plain): K P K K P cut to
    the length; mono (S = stereo, M = mono): M / S M / S S M / S S M M S."""
    (g, c), (gm, cm), idx = _pools()
    gs, cs, lengths, names = [], [], [], []
    for kind in ("plain", "all_short", "mixed", "intensity", "line128"):
        k, p = idx[kind], idx["plain"]
        picks = [k[0], p[0], k[1], k[2], p[1]]
        for n in LENGTHS:
            gs.append(g[picks[:n]])
            cs.append(c[picks[:n]])
            lengths.append(n)
            names.append(f"{kind}-{n}")
    p = idx["plain"]
    mono = {1: "M", 2: "SM", 3: "SSM", 5: "SSMMS"}
    for n in LENGTHS:
        take = [(gm[i], cm[i]) if t == "M" else (g[p[2 + i]], c[p[2 + i]]) for i, t in enumerate(mono[n])]
        gs.append(np.array([t[0] for t in take], dtype=g.dtype))
        cs.append(np.stack([t[1] for t in take]))
        lengths.append(n)
        names.append(f"mono_after_stereo-{n}")
    gb, cb = np.concatenate(gs), np.concatenate(cs)
    assert mp3g.validate(gb, cb)[0] == 0
    # an entry state: the oracle's after 20 granules of the (stereo) pool
    _, st = oracle.dsp_streams(g[:20], c[:20], mp3g.streams_for([20], mp3g.STATE_OUT))
    return gb, cb, lengths, names, np.repeat(st, len(lengths))


@pytest.fixture(scope="module")
def batch(gpu):
    gb, cb, lengths, names, st = _batch(gpu)
    out = {"g": gb, "c": cb, "names": names}
    for with_state in (False, True):
        s = gpu.streams_for(lengths, gpu.STATE_OUT | (gpu.STATE_IN if with_state else 0))
        sin = st if with_state else None
        want, so = oracle.dsp_streams(gb, cb, s, sin)
        out[with_state] = (s, sin, want, so)
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run(mp3g, g, c, s, state_in, fmt, mode, chunk):
    """Plan.execute on torch buffers: (raw output words, exported state)."""
    import torch
    d_out = torch.zeros(len(g) * mp3g.out_bytes_per_granule(fmt) // 4, dtype=torch.int32, device="cuda")
    d_so = torch.zeros(len(s) * mp3g.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_si = _dev(state_in) if state_in is not None else None
    plan = mp3g.Plan(s, granules_per_chunk=chunk, mode=mode)
    plan.execute(_dev(g), _dev(c), d_out, d_si, d_so, stream=torch.cuda.current_stream().cuda_stream, out_format=fmt)
    torch.cuda.synchronize()
    plan.close()
    return d_out.cpu().numpy().view(np.uint32), d_so.cpu().numpy().view(mp3g.STATE_DTYPE)


def _worst(d, s, names):
    """max |d| per stream, for the failure message."""
    per = [int(d[int(x["first_granule"]):int(x["first_granule"]) + int(x["n_granules"])].max()) for x in s]
    return {n: v for n, v in zip(names, per) if v}


@pytest.mark.parametrize("with_state", [False, True], ids=["zero_state", "state_in"])
@pytest.mark.parametrize("what", ["fast-s16", "fast-f32", "fast-planar", "exact-s16"])
def test_loop_entry(gpu, batch, what, with_state):
    mode_name, fmt_name = what.split("-")
    mode = gpu.MODE_FAST if mode_name == "fast" else gpu.MODE_EXACT
    fmt = {"s16": gpu.OUT_S16, "f32": gpu.OUT_F32, "planar": gpu.OUT_F32_PLANAR}[fmt_name]
    tol = 1 if mode_name == "fast" else 0
    g, c, names = batch["g"], batch["c"], batch["names"]
    s, sin, want, so_want = batch[with_state]
    ref, so_ref = run(gpu, g, c, s, sin, fmt, mode, ONE_CHUNK)
    # the one-chunk decode against the oracle
    out = as_interleaved(gpu, ref, s, fmt, len(g))
    got = out if fmt == gpu.OUT_S16 else q(out)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
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
        assert so.tobytes() == so_ref.tobytes(), f"{what} chunk={chunk}: exported state differs"
