"""The fast kernel's LDS addressing (granule_fast.hip): the window's operands,
the S rows and the matrixing columns read and written through per-granule
column pointers plus immediate offsets, in both ring layouts, and the
long-block requantize's table offsets with their out-of-table test (the OR of
a lane's offsets against a mask).  No arithmetic depends on how an address is
formed, so what is checked is what the addresses decide: which ring slot a tap
multiplies and which table entry (or the arithmetic redo) a line gets.

  1. 2 streams x 12 granules of the synthetic writer, fast plan, s16: chunk
     lengths 1, 2, 5 and 12 (both ring layouts at every granule, chunks with
     and without a halo) give the same bytes, within 1 LSB of the oracle.
  2. The same on the first 64 granules of the two sample files (mono runs,
     short and mixed blocks, intensity stereo).
  3. One stream whose all-long granules hold lines at and around the table's
     edge -- x = 127, 128, -128, -129 and 8206 (mp3g_validate's bound), with both
     halves of a coefficient dword outside the table and either half alone --
     placed below count1.  The granules are quiet enough (global_gain) not to be
     hot: the zone launch rewrites nothing, the PCM is the fast pass's own.
  4. float32 interleaved and planar and both mono formats on case 1, by their
     defined relations to the s16 output (tests/test_gpu_outfmt.py,
     tests/test_gpu_outfmt_mono.py): q(float) is the s16 sample, S16_MONO is
     (L + R) >> 1, F32_MONO the float32 mean of the F32 output.

The bound is fast mode's contract (tests/test_gpu_fast.py): 1 LSB of the
oracle; between chunkings 0.
"""
import numpy as np
import pytest

import oracle
from mp3g import synth
from test_gpu_outfmt import as_interleaved, q, run_out
from test_gpu_outfmt_mono import as_mono, dm16, dm32

pytestmark = pytest.mark.gpu

CHUNKS = (1, 2, 5, 12)
EDGE = (127, 128, -128, -129, 8206)


def fast_s16(gpu, g, c, s, chunk, mode=None):
    raw, so = run_out(gpu, g, c, s, gpu.OUT_S16, chunk=chunk, mode=gpu.MODE_FAST if mode is None else mode)
    return as_interleaved(gpu, raw, s, gpu.OUT_S16, len(g)).copy(), so


def check_chunkings(gpu, g, c, s, what, chunks=CHUNKS):
    """Every chunking's s16 PCM: the same bytes, within 1 LSB of the oracle."""
    want, _ = oracle.dsp_streams(g, c, s)
    ref, so_ref = fast_s16(gpu, g, c, s, chunks[-1])
    d = np.abs(ref.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: max |dPCM| = {d.max()} LSB against the oracle, {(d > 0).mean():.4%} of samples differ")
    assert d.max() <= 1, f"{what}: {d.max()} LSB from the oracle in granules {np.unique(np.nonzero(d > 1)[0])[:8]}"
    for chunk in chunks[:-1]:
        got, so = fast_s16(gpu, g, c, s, chunk)
        bad = np.nonzero((got != ref).any(axis=(1, 2)))[0]
        assert len(bad) == 0, f"{what} chunk={chunk}: PCM differs from chunk={chunks[-1]} in granules {bad[:8]}"
        assert so.tobytes() == so_ref.tobytes(), f"{what} chunk={chunk}: exported state differs"
    return ref


@pytest.fixture(scope="module")
def two_streams(gpu):
    g, c, s = synth.synth_batch(2, 6, seed=29)
    assert len(g) == 24 and [int(x["n_granules"]) for x in s] == [12, 12]
    s = gpu.streams_for([12, 12], gpu.STATE_OUT)
    assert gpu.validate(g, c)[0] == 0
    return g, c, s


@pytest.fixture(scope="module")
def two_streams_s16(gpu, two_streams):
    g, c, s = two_streams
    return {chunk: fast_s16(gpu, g, c, s, chunk) for chunk in CHUNKS}


def test_synthetic_chunkings(gpu, two_streams):
    check_chunkings(gpu, *two_streams, "synthetic 2 x 12")


@pytest.mark.parametrize("name", ["mpeg2.mp3", "classic_lame.mp3"])
def test_sample_file_chunkings(gpu, captured, name):
    g, c, _ = captured[name]
    n = min(64, len(g))
    g, c = g[:n].copy(), c[:n].copy()
    check_chunkings(gpu, g, c, gpu.streams_for([n], gpu.STATE_OUT), name)


def _is_short(ch):
    return (ch["win_switch_flag"] == 1) & (ch["block_type"] == 2)


def edge_stream(gpu):
    """12 granules of one synthetic stream; in its all-long stereo granules
    without intensity stereo, lines below count1 are overwritten with the
    values at the table's edge.  Per coefficient dword (lines 2q, 2q + 1 of a
    subband, low and high half): both halves outside the table, either half
    alone, and every EDGE value in either half."""
    g, c = synth.synth_stream(41, 6, p_event=0.0, p_is=0.0)
    g, c = g[:12].copy(), c[:12].copy()
    short = _is_short(g["ch"]).any(axis=1)
    stereo = ((g["header"] >> 6) & 3) != 3
    plain = np.nonzero(~short & stereo & ((g["header"] & 0x10) == 0))[0]
    assert len(plain) >= 6, "the generator produced too few all-long stereo granules"
    # (low half, high half) of one dword
    pairs = [(128, 128), (-129, 8206), (8206, -129),     # both outside
             (128, 127), (127, 128), (-129, -128), (-128, -129), (8206, 0), (0, 8206), (-8206, 5), (5, -8206),  # one
             (127, -128), (-128, 127), (127, 127), (-128, -128)]  # both inside, at the edge
    edited = []
    for n, gi in enumerate(plain[:6]):
        # quiet, so that no granule is hot and no sample clips: with the lines
        # at +-8206, 8206^(4/3) 2^((128 - 210) / 4) = 0.11; without them (odd n)
        # 129^(4/3) 2^((160 - 210) / 4) = 0.11
        for ch in range(2):
            g["ch"][gi, ch]["global_gain"] = 128 if n % 2 == 0 else 160
            g["ch"][gi, ch]["count1"] = max(int(g["ch"][gi, ch]["count1"]), 400)
        c[gi] = np.clip(c[gi], -15, 15)  # (the writer's own rare large lines: only the edits below)
        for m, (lo, hi) in enumerate(pairs):
            if n % 2 and max(abs(lo), abs(hi)) > 129:
                continue
            # dword q = (m + n) % 9 of subband 1 + m (below line 400), on one
            # channel or both: lanes with and without a line outside the table
            sb, dq = 1 + m, (m + n) % 9
            for ch in ((0, 1) if (m + n) % 3 == 0 else ((m + n) % 2,)):
                c[gi, ch, 18 * sb + 2 * dq] = lo
                c[gi, ch, 18 * sb + 2 * dq + 1] = hi
        edited.append(int(gi))
    assert gpu.validate(g, c)[0] == 0
    for v in EDGE:
        assert (c[edited] == v).any(), v
    return g, c, edited


def test_table_edge_lines(gpu):
    g, c, edited = edge_stream(gpu)
    s = gpu.streams_for([len(g)], gpu.STATE_OUT)
    ref = check_chunkings(gpu, g, c, s, "table-edge lines")
    assert np.abs(ref[edited].astype(np.int32)).max() > 8, "the edited granules are silent: nothing was checked"
    # the PCM compared is the fast pass's own: no granule was redone in the reference's order
    import torch
    from test_gpu_outfmt import _dev
    plan = gpu.Plan(s, granules_per_chunk=5, mode=gpu.MODE_FAST | gpu.FLAG_HOT_STATS)
    d_p = torch.zeros(len(g) * 1152, dtype=torch.int16, device="cuda")
    d_so = torch.zeros(len(s) * gpu.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    plan.execute(_dev(g), _dev(c), d_p, None, d_so, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    stats = plan.hot_stats()
    plan.close()
    assert stats["rewritten"] == 0, stats
    assert np.array_equal(d_p.cpu().numpy().reshape(len(g), 576, 2), ref), "the counting build's PCM differs"


@pytest.mark.parametrize("chunk", CHUNKS)
def test_formats(gpu, two_streams, two_streams_s16, chunk):
    g, c, s = two_streams
    n = len(g)
    s16, so16 = two_streams_s16[chunk]
    f32 = None
    for fmt in (gpu.OUT_F32, gpu.OUT_F32_PLANAR):
        raw, so = run_out(gpu, g, c, s, fmt, chunk=chunk, mode=gpu.MODE_FAST)
        out = as_interleaved(gpu, raw, s, fmt, n)
        assert np.array_equal(q(out), s16), f"fmt={fmt} chunk={chunk}: q(float) differs from the s16 output"
        assert so.tobytes() == so16.tobytes()
        if fmt == gpu.OUT_F32:
            f32 = out.copy()
    raw, so = run_out(gpu, g, c, s, gpu.OUT_S16_MONO, chunk=chunk, mode=gpu.MODE_FAST)
    assert np.array_equal(as_mono(gpu, raw, gpu.OUT_S16_MONO, n), dm16(s16)), f"chunk={chunk}: S16_MONO"
    assert so.tobytes() == so16.tobytes()
    raw, so = run_out(gpu, g, c, s, gpu.OUT_F32_MONO, chunk=chunk, mode=gpu.MODE_FAST)
    assert as_mono(gpu, raw, gpu.OUT_F32_MONO, n).tobytes() == dm32(f32).tobytes(), f"chunk={chunk}: F32_MONO"
    assert so.tobytes() == so16.tobytes()
