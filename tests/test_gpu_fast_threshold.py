"""The fused fast kernel AT its hot-granule thresholds.

Fast mode's +-1 LSB promise rests on a two-level test inside
granule_fast_kernel: a granule runs in the reference's operation order when
max |S| > kHotS and some slot's sum of |S| exceeds kHotL1; below that the
reassociated transforms are only *measured* to stay within 1 LSB.  The other
fast-mode tests sit far on either side of the bound; these put every stream
of 24 input shapes between 0.84 (0.95 for the sign patterns) and 0.999 of its
governing bound (tests/fast_edge_inputs.py; the conditions on the inputs are
checked in tests/test_fast_edge_inputs_cpu.py), where the front end's, the
IMDCT's and the matrixing's errors are largest while the fallback is still
off -- and one gain step higher, where the fallback must be on.

"under": the hot counters are all zero (the fast transforms made this PCM),
max |PCM - oracle| <= 1 over all samples, chunkings and both builds of the
kernel agree byte for byte, the exported state is within float noise of the
oracle's; on the long variants the float32 and mono formats follow their
value rules.  "over": the counters say the fallback ran for the granules
the oracle's S puts over both bounds, and the PCM stays within 1 LSB.

(That the builder's bounds are the kernel's is asserted on the CPU side:
tests/test_fast_edge_inputs_cpu.py::test_bounds_are_the_kernels.)

Each case prints its measured figures (pytest -s): they are the record in
DESIGN.md section 7.
"""
import numpy as np
import pytest

import fast_edge_inputs as fe
from test_gpu_outfmt import q

pytestmark = pytest.mark.gpu

IDS = [f"{k}-{v}" for k, v in fe.CASES]
ZERO_STATS = {"rewritten": 0, "zones": 0, "hot": 0, "in_wave": 0}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Batch:
    """One case's inputs on the device, decoded as the tests ask."""

    def __init__(self, mp3g, g, c, s):
        self.mp3g, self.s, self.n = mp3g, s, len(g)
        self.d_g, self.d_c = _dev(g), _dev(c)

    def run(self, chunk, mode, fmts=(0,)):
        """One plan, one launch per format: ([output per format], state_out, hot_stats)."""
        import torch
        m = self.mp3g
        plan = m.Plan(self.s, granules_per_chunk=chunk, mode=mode)
        outs = []
        try:
            for fmt in fmts:
                d_out = torch.zeros(self.n * m.out_bytes_per_granule(fmt), dtype=torch.uint8, device="cuda")
                d_so = torch.zeros(len(self.s) * m.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                plan.execute(self.d_g, self.d_c, d_out, None, d_so,
                             stream=torch.cuda.current_stream().cuda_stream, out_format=fmt)
                torch.cuda.synchronize()
                raw = d_out.cpu().numpy()
                if fmt in (m.OUT_S16, m.OUT_S16_MONO):
                    outs.append(raw.view(np.int16).reshape((self.n, 576, 2) if fmt == m.OUT_S16 else (self.n, 576)))
                else:
                    outs.append(raw.view(np.float32).reshape(self.n, 576, 2))
                so = d_so.cpu().numpy().view(m.STATE_DTYPE)
            hs = plan.hot_stats() if mode & m.FLAG_HOT_STATS else None
        finally:
            plan.close()
        return outs, so, hs


def measure(pcm, want):
    """(max |dPCM|, differing share among the unclipped samples, unclipped share)."""
    d = np.abs(pcm.astype(np.int32) - want.astype(np.int32))
    ok = np.abs(want.astype(np.int32)) < 32767
    return int(d.max()), float((d[ok] > 0).mean()), float(ok.mean())


def check_state(so, ref):
    """test_fast_hot_granules' bound on the exported state against the oracle's."""
    for key in ("store", "vvec"):
        for st in range(len(ref)):
            r, got = ref[key][st], so[key][st]
            if key == "vvec":
                r, got = r[:, :960], got[:, :960]
            np.testing.assert_allclose(got, r, rtol=0, atol=2e-5 * max(1.0, float(np.abs(r).max())))


def check_chunkings(b, mp3g, pcm0, so0, what):
    """The plain build at granules_per_chunk 1 (every granule behind a replayed
    halo) and 0 (the default): the bytes of the counting build's single chunk."""
    for chunk in (1, 0):
        (pcm,), so, _ = b.run(chunk, mp3g.MODE_FAST)
        assert np.array_equal(pcm, pcm0), f"{what}: chunk={chunk} differs from the one-chunk counting run"
        assert so.tobytes() == so0.tobytes(), f"{what}: chunk={chunk}: exported state differs"


@pytest.mark.parametrize("kind,variant", fe.CASES, ids=IDS)
def test_under(gpu, kind, variant):
    g, c, s, info = fe.edge_case(kind, variant, "under")
    want = info["pcm"]
    b = Batch(gpu, g, c, s)
    # one chunk per stream, the counting build: nothing was flagged, so the
    # fast transforms produced every sample below
    (pcm0,), so0, hs = b.run(4, gpu.MODE_FAST | gpu.FLAG_HOT_STATS)
    dmax, diff, uncl = measure(pcm0, want)
    print(f"under {kind}/{variant}: ratio {info['ratio'].min():.4f}..{info['ratio'].max():.4f}, "
          f"max|dPCM| {dmax}, differing {diff:.4%} of unclipped, unclipped {uncl:.3f}, hot_stats {hs}")
    assert hs == ZERO_STATS, f"{kind}/{variant}: granules under the bounds took the fallback: {hs}"
    assert dmax <= 1, f"{kind}/{variant}: max|dPCM| = {dmax} LSB just under the hot-granule bounds"
    check_chunkings(b, gpu, pcm0, so0, f"{kind}/{variant}")
    check_state(so0, info["state"])
    if variant != "long":
        return
    # the other formats of the same plan (include/mp3g.h's value rules)
    (s16, f32, m16), so, _ = b.run(4, gpu.MODE_FAST, (gpu.OUT_S16, gpu.OUT_F32, gpu.OUT_S16_MONO))
    assert np.array_equal(s16, pcm0) and so.tobytes() == so0.tobytes()
    assert np.array_equal(q(f32), s16), f"{kind}: q(float) differs from the fast s16 output"
    (exact,), _, _ = b.run(4, gpu.MODE_EXACT, (gpu.OUT_F32,))
    assert np.array_equal(q(exact), want)
    d = float(np.abs(f32.astype(np.float64) - exact.astype(np.float64)).max() * 32768.0)
    print(f"under {kind}/{variant}: fast vs exact float, max |d| * 32768 = {d:.6f}")
    assert d < 2.0, d
    mono = ((s16[..., 0].astype(np.int32) + s16[..., 1].astype(np.int32)) >> 1).astype(np.int16)
    assert np.array_equal(m16, mono), f"{kind}: S16_MONO differs from (L + R) >> 1 of the fast s16 output"


@pytest.mark.parametrize("kind,variant", fe.CASES, ids=IDS)
def test_over(gpu, kind, variant):
    """One gain step over the bounds.  hs["hot"] is what the fast pass flagged
    (record_hot's caller: every granule it decodes whose V feeds an output,
    halo replays included).  With one chunk per stream there is no halo, and
    the kernel's S differs from the oracle's only by the fast IMDCT's
    rounding (~1e-6 relative, far inside the 1e-3 bands), so both the lower
    and the upper count are exact here."""
    g, c, s, info = fe.edge_case(kind, variant, "over")
    want = info["pcm"]
    b = Batch(gpu, g, c, s)
    (pcm0,), so0, hs = b.run(4, gpu.MODE_FAST | gpu.FLAG_HOT_STATS)
    dmax, diff, uncl = measure(pcm0, want)
    lo, hi = int(info["hot_hi"].sum()), int(info["hot_lo"].sum())
    print(f"over {kind}/{variant}: hot by the oracle {lo}..{hi} of {len(g)}, max|dPCM| {dmax}, "
          f"differing {diff:.4%} of unclipped, unclipped {uncl:.3f}, hot_stats {hs}")
    assert lo >= len(s)  # (every stream has one: tests/test_fast_edge_inputs_cpu.py)
    assert lo <= hs["hot"] <= hi, (hs, lo, hi)
    assert hs["zones"] > 0 and hs["in_wave"] == 0, hs
    assert hs["rewritten"] >= hs["hot"], hs
    assert dmax <= 1, f"{kind}/{variant}: max|dPCM| = {dmax} LSB just over the hot-granule bounds"
    check_chunkings(b, gpu, pcm0, so0, f"{kind}/{variant}")
    check_state(so0, info["state"])
