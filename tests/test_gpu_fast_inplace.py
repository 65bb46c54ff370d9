"""The fast kernel's stages that compute no sample of their own
(granule_fast.hip, granule_out.hip): the antialias butterflies applied in
place under the lane mask instead of selected per line, the s16 pack whose
clamp is the integer pack's saturation, and the MS stage between the
requantize and the butterflies.  None of them changes the
arithmetic, so what is checked is what they decide: which lanes a butterfly
touches, which lines MS transforms, and what a sum outside +-32767 becomes.

Every stream is a few dozen granules, decoded at chunk lengths 1, 2, 5 and 12
(both ring layouts at every granule, as tests/test_gpu_fast_addr.py): the same
bytes at every chunking, within 1 LSB of the oracle.

  Clamp.  A stereo and a mono source whose global_gain is raised, by a boost
  chosen on the CPU with the oracle, just far enough that the oracle's PCM
  reaches +32767 and -32767 while no granule is hot (max |S| stays under kHotS:
  mp3g_plan_hot_stats reports no rewritten granule, so the clipped samples are
  this pack's and not the exact zones').  Where the oracle is at a rail the GPU
  equals it; no sample is -32768.
  Antialias.  Channel 0 loud in subbands 0 and 31 next to a silent channel 1
  (and the reverse): nothing crosses lanes 31 / 32; mixed blocks (butterflies
  between subbands 0 and 1 only); short non-mixed blocks (none); mono granules
  inside a stereo stream (channel 1's lanes frozen).
  MS.  Over every line; with intensity stereo; with short blocks and a small
  count1 (the partial branch: lines at and above max(count1) keep their values).
"""
import numpy as np
import pytest

import oracle
from fast_edge_inputs import stream_ratios
from mp3g import synth
from test_gpu_fast_addr import check_chunkings
from test_gpu_outfmt import _dev

pytestmark = pytest.mark.gpu

RAIL = 32767


def _is_short(ch):
    return (ch["win_switch_flag"] == 1) & (ch["block_type"] == 2)


def _stereo(g):
    return ((g["header"] >> 6) & 3) != 3


def _one_stream(gpu, g, c):
    assert gpu.validate(g, c)[0] == 0
    return g, c, gpu.streams_for([len(g)], gpu.STATE_OUT)


# ---- clamp --------------------------------------------------------------------

def clipping_stream(gpu, mode):
    """12 all-long granules with few, low lines (a handful of loud partials: the
    PCM swings far while every |S| stays small), and the smallest global_gain
    boost at which the oracle's PCM stands at either rail in eight samples or
    more.  Returns (g, c, s, oracle PCM)."""
    g, c = synth.synth_stream(61 + mode, 6, mode=mode, p_event=0.0, p_is=0.0)
    g, c = g[:12].copy(), c[:12].copy()
    nch = 1 if mode == synth.MODE_MONO else 2
    rng = np.random.default_rng(5 + mode)
    c[:] = 0
    for ch in range(nch):
        # three partials per granule in subbands 0..3, amplitude 20..40
        for gi in range(len(g)):
            lines = rng.choice(72, size=3, replace=False)
            c[gi, ch, lines] = rng.integers(20, 41, size=3) * rng.choice([-1, 1], size=3)
        g["ch"]["count1"][:, ch] = 72
        g["ch"]["global_gain"][:, ch] = 150
        g["ch"]["scalefac_l"][:, ch] = 0
        g["ch"]["scalefac_scale"][:, ch] = 0
        g["ch"]["preflag"][:, ch] = 0
    s = gpu.streams_for([len(g)], gpu.STATE_OUT)
    for boost in range(0, 80):
        g["ch"]["global_gain"][:, :nch] = 150 + boost
        want, _ = oracle.dsp_streams(g, c, s)
        w = want[:, :, :nch]
        if (w == RAIL).sum() >= 8 and (w == -RAIL).sum() >= 8:
            break
    else:
        raise AssertionError("no boost brings the oracle to both rails")
    assert gpu.validate(g, c)[0] == 0
    return g, c, s, want


@pytest.mark.parametrize("mode", [synth.MODE_JOINT, synth.MODE_MONO], ids=["stereo", "mono"])
def test_clamp_at_the_rails(gpu, mode):
    import torch
    g, c, s, want = clipping_stream(gpu, mode)
    # the oracle clips at both rails (the test cannot pass vacuously) ...
    hi, lo = want == RAIL, want == -RAIL
    print(f"global_gain {int(g['ch']['global_gain'][0, 0])}: {int(hi.sum())} samples at +{RAIL}, {int(lo.sum())} at -{RAIL}")
    assert hi.any() and lo.any()
    # ... and no granule is hot, by the oracle's S and by the plan's own count
    ra, rb, _, _ = stream_ratios(g, c, s)
    print(f"max |S| / kHotS = {ra.max():.3f}, max slot sum / kHotL1 = {rb.max():.3f}")
    assert np.minimum(ra, rb).max() < 0.99, "a granule is at the hot bound"
    plan = gpu.Plan(s, granules_per_chunk=5, mode=gpu.MODE_FAST | gpu.FLAG_HOT_STATS)
    d_p = torch.zeros(len(g) * 1152, dtype=torch.int16, device="cuda")
    d_so = torch.zeros(len(s) * gpu.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    plan.execute(_dev(g), _dev(c), d_p, None, d_so, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    stats = plan.hot_stats()
    plan.close()
    assert stats["hot"] == 0 and stats["rewritten"] == 0, stats
    ref = check_chunkings(gpu, g, c, s, f"clamp mode={mode}")
    assert np.array_equal(d_p.cpu().numpy().reshape(len(g), 576, 2), ref), "the counting build's PCM differs"
    rail = hi | lo
    bad = np.nonzero(ref[rail] != want[rail])[0]
    assert len(bad) == 0, f"{len(bad)} of {int(rail.sum())} rail samples differ: GPU {ref[rail][bad[:8]]}, oracle {want[rail][bad[:8]]}"
    assert (ref != -32768).all(), "a sample is -32768"


# ---- antialias edges ------------------------------------------------------------

def edge_subband_stream(gpu):
    """12 plain stereo all-long granules: one channel loud in subbands 0 and 31
    only, the other silent -- channel 0 loud in the first six, channel 1 in the
    last six."""
    g, c = synth.synth_stream(71, 6, mode=synth.MODE_STEREO, p_event=0.0, p_is=0.0)
    g, c = g[:12].copy(), c[:12].copy()
    rng = np.random.default_rng(72)
    c[:] = 0
    for gi in range(12):
        loud = 0 if gi < 6 else 1
        v = rng.integers(3, 16, size=36) * rng.choice([-1, 1], size=36)
        c[gi, loud, :18] = v[:18]
        c[gi, loud, 558:] = v[18:]
        g["ch"]["count1"][gi, loud] = 576
        g["ch"]["count1"][gi, 1 - loud] = 0
    g["ch"]["global_gain"][:] = 170
    return _one_stream(gpu, g, c)


def test_antialias_stays_inside_a_channel(gpu):
    g, c, s = edge_subband_stream(gpu)
    want, _ = oracle.dsp_streams(g, c, s)
    ref = check_chunkings(gpu, g, c, s, "subbands 0 and 31 next to a silent channel")
    assert np.abs(want[:6, :, 0].astype(np.int32)).max() > 1000 and np.abs(want[8:, :, 1].astype(np.int32)).max() > 1000
    # the silent channel is silent: nothing crossed lanes 31 / 32
    assert not want[:6, :, 1].any() and not ref[:6, :, 1].any(), "channel 1 hears channel 0"
    # (granules 6, 7 still carry channel 0's overlap and window history)
    assert not want[8:, :, 0].any() and not ref[8:, :, 0].any(), "channel 0 hears channel 1"


@pytest.mark.parametrize("p_mixed", [1.0, 0.0], ids=["mixed", "short"])
def test_antialias_short_and_mixed_blocks(gpu, p_mixed):
    """Mixed blocks: butterflies between subbands 0 and 1 only; short non-mixed
    blocks: none.  Loud lines in every subband, so a butterfly too many shows."""
    g, c = synth.synth_stream(81, 12, p_event=0.3, p_mixed=p_mixed, p_is=0.0)
    g, c = g[:24].copy(), c[:24].copy()
    short = _is_short(g["ch"])
    assert short.any(axis=1).sum() >= 4, "the generator produced too few short-block granules"
    mixed = g["ch"]["mixed_block_flag"] == 1
    assert mixed[short].all() if p_mixed else not mixed.any()
    g, c, s = _one_stream(gpu, g, c)
    check_chunkings(gpu, g, c, s, f"short blocks, p_mixed={p_mixed}")


def test_antialias_mono_inside_stereo(gpu):
    """Mono granules inside a stereo stream: channel 1's lanes keep their
    overlap and take no butterfly."""
    parts = [synth.synth_stream(91, 4, p_is=0.0), synth.synth_stream(92, 3, mode=synth.MODE_MONO),
             synth.synth_stream(93, 3, p_is=0.0), synth.synth_stream(94, 1, mode=synth.MODE_MONO),
             synth.synth_stream(95, 2, p_is=0.0)]
    g = np.concatenate([p[0] for p in parts])
    c = np.concatenate([p[1] for p in parts])
    assert len(g) == 26 and 0 < _stereo(g).sum() < len(g)
    g, c, s = _one_stream(gpu, g, c)
    check_chunkings(gpu, g, c, s, "mono granules inside a stereo stream")


# ---- MS -----------------------------------------------------------------------

def _ms(g):
    return _stereo(g) & (((g["header"] >> 6) & 3) == 1) & ((g["header"] & 0x20) != 0)


def test_ms_over_every_line(gpu):
    g, c = synth.synth_stream(101, 6, p_ms=1.0, p_is=0.0, p_event=0.0)
    g, c = g[:12].copy(), c[:12].copy()
    assert _ms(g).all() and not (g["header"] & 0x10).any() and not _is_short(g["ch"]).any()
    # channels of unlike count1: lines between the two are MS lines too
    assert (g["ch"]["count1"][:, 0] != g["ch"]["count1"][:, 1]).any()
    g, c, s = _one_stream(gpu, g, c)
    check_chunkings(gpu, g, c, s, "MS over every line")


def test_ms_with_intensity_stereo(gpu):
    g, c = synth.synth_stream(111, 6, p_ms=1.0, p_is=1.0, p_event=0.0)
    g, c = g[:12].copy(), c[:12].copy()
    assert _ms(g).all() and (g["header"] & 0x10).all()
    g, c, s = _one_stream(gpu, g, c)
    check_chunkings(gpu, g, c, s, "MS with intensity stereo")


def test_ms_partial_short_blocks_small_count1(gpu):
    """MS with short blocks and a small count1: the reorder moves values past
    max(count1), and MS must leave the lines at and above it alone."""
    g, c = synth.synth_stream(121, 12, p_ms=1.0, p_is=0.0, p_event=0.3)
    g, c = g[:24].copy(), c[:24].copy()
    short = _is_short(g["ch"]).any(axis=1)
    assert short.sum() >= 4 and _ms(g).all()
    for gi in np.nonzero(short)[0]:
        for ch, lim in ((0, 90), (1, 60)):
            c[gi, ch, lim:] = 0
            g["ch"]["count1"][gi, ch] = lim
    g, c, s = _one_stream(gpu, g, c)
    want, _ = oracle.dsp_streams(g, c, s)
    assert np.abs(want[short].astype(np.int32)).max() > 8, "the short-block granules are silent"
    check_chunkings(gpu, g, c, s, "MS, short blocks, small count1")
