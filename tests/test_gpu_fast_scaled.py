"""The fast kernel's folded factors on the GPU (granule_fast.hip): the scaled
DCT-32 (sigma in the window taps, per lane and tap parity), the scaled
DCT-IV-18 (factors in the long IMDCT windows) and the MS 1/sqrt2 in the band
gains of all-long MS granules.  The scale never leaves a wave, so besides the
fast mode's +-1 LSB against the oracle every chunking must stay bit-identical
to the one-chunk decode, and the exported state stays in the V domain.

Inputs are 4 streams x 40 frames unless stated; each case asserts that its
input really takes the branch it is about."""
import numpy as np
import pytest

import oracle
from mp3g import synth
from test_gpu_fast import assert_close, fast_plan
from test_gpu_outfmt import as_interleaved, run_out

pytestmark = pytest.mark.gpu


def folded(g):
    """Granules on the folded-gain branch: joint stereo with MS and without
    intensity stereo, every channel a long block."""
    h = g["header"]
    joint = ((h >> 6) & 3) == 1
    return joint & ((h & 0x30) == 0x20) & (g["ch"]["block_type"] != 2).all(axis=1)


def check_case(gpu, g, c, s, what):
    """Within 1 LSB of the oracle; chunkings of 1, 3 and 7 granules
    bit-identical to the one-chunk decode (a stream per chunk)."""
    want, _ = oracle.dsp_streams(g, c, s)
    one, _ = fast_plan(gpu, g, c, s, chunk=int(s["n_granules"].max()))
    dmax, frac = assert_close(one, want, what)
    print(f"{what}: max|dPCM|={dmax} LSB, {frac:.5%} of samples differ")
    for chunk in (1, 3, 7):
        pcm, _ = fast_plan(gpu, g, c, s, chunk=chunk)
        assert np.array_equal(pcm, one), f"{what}: chunk={chunk} differs from the one-chunk decode"
    return want


def test_all_ms_long(gpu):
    """MS on every frame, no intensity stereo, no window events: the folded
    gains on every granule."""
    g, c, s = synth.synth_batch(4, 40, seed=41, p_ms=1.0, p_is=0.0, p_event=0.0)
    assert folded(g).all()
    want = check_case(gpu, g, c, s, "all MS, long")
    assert np.abs(want).max() > 1000


@pytest.fixture(scope="module")
def mixed_input():
    g, c, s = synth.synth_batch(4, 40, seed=42, p_ms=0.5, p_is=0.5, p_event=0.1, p_mixed=0.3)
    f = folded(g)
    # both branches, alternating: a good share of each and many changes
    assert 0.1 < f.mean() < 0.9 and np.count_nonzero(f[1:] != f[:-1]) > 20
    # MS with intensity stereo and MS on short blocks: the partial branch
    ms = (g["header"] & 0x20) != 0
    assert (ms & ~f).sum() > 20
    bt = g["ch"]["block_type"]
    assert all((bt == t).any() for t in range(4)) and g["ch"]["mixed_block_flag"].any()
    return g, c, s


def test_mixed_branches(gpu, mixed_input):
    """MS / IS per frame with window switching and mixed blocks: folded and
    unfolded gains from granule to granule, every long window shape."""
    g, c, s = mixed_input
    check_case(gpu, g, c, s, "MS/IS, window switching")


def test_mono_and_switching(gpu):
    """The frozen channel's history (X / sigma in the ring) in both layouts:
    mono streams, and one stream alternating mono and stereo runs."""
    g, c, s = synth.synth_batch(4, 40, seed=43, mode=synth.MODE_MONO, p_mixed=0.3)
    check_case(gpu, g, c, s, "mono")
    parts = [synth.synth_stream(51, 6, p_ms=1.0, p_is=0.0), synth.synth_stream(52, 5, mode=synth.MODE_MONO),
             synth.synth_stream(53, 7, p_ms=1.0, p_is=0.0), synth.synth_stream(54, 4, mode=synth.MODE_MONO),
             synth.synth_stream(55, 1), synth.synth_stream(56, 1, mode=synth.MODE_MONO),
             synth.synth_stream(57, 16, p_event=0.1, p_mixed=0.3)]
    g = np.concatenate([p[0] for p in parts])
    c = np.concatenate([p[1] for p in parts])
    assert len(g) == 80
    check_case(gpu, g, c, gpu.streams_for([len(g)], gpu.STATE_OUT), "mono / stereo runs")


def float_pcm_ref(g, c, s):
    """The reference's float PCM without the s16 truncation: the oracle's
    hybrid output (float32 lines, frame.go:140-486) through the polyphase
    synthesis of frame.go:630-669 in float64 with the reference's own float32
    tables, f = clamp(sum * 32767, +-32767) / 32768 (include/mp3g.h's value
    rule).  Stereo streams entering with zero state."""
    T = oracle.tables()
    nwin = T["synth_nwin"].astype(np.float64)
    D = T["synth_d"].astype(np.float64).reshape(16, 32)
    lines = oracle.hybrid_streams(g, c, s).astype(np.float64)  # [n, 2, 576], line = 18 sb + slot
    out = np.zeros((len(g), 576, 2))
    i = np.arange(32)
    for st in s:
        lo, n = int(st["first_granule"]), int(st["n_granules"])
        for ch in range(2):
            S = lines[lo:lo + n, ch].reshape(n, 32, 18).transpose(0, 2, 1).reshape(n * 18, 32)  # [time slot][sb]
            V = np.concatenate([np.zeros((15, 64)), S @ nwin.T])  # V[15 + T]
            acc = np.zeros((n * 18, 32))
            for j in range(16):
                Vj = V[15 - j:15 - j + n * 18]  # V of slot T - j
                acc += D[j] * (Vj[:, 32 + i] if j & 1 else Vj[:, i])
            out[lo:lo + n, :, ch] = acc.reshape(n, 576)
    return np.clip(out * 32767.0, -32767.0, 32767.0) / 32768.0


def test_f32_against_float_reference(gpu, mixed_input):
    """MP3G_OUT_F32 of the mixed input: floats within one LSB-equivalent of the
    reference's untruncated PCM -- no truncation to hide a factor that is
    slightly off."""
    g, c, s = mixed_input
    ref = float_pcm_ref(g, c, s)
    want, _ = oracle.dsp_streams(g, c, s)
    # the float64 reference against the reference's own float32 sums: the same
    # samples but where a sum sits within rounding of an integer
    d16 = np.abs(np.trunc(ref * 32768.0) - want)
    assert d16.max() <= 1 and (d16 > 0).mean() < 1e-3, (d16.max(), (d16 > 0).mean())
    assert np.abs(ref).max() > 0.03
    raw, _ = run_out(gpu, g, c, s, gpu.OUT_F32, mode=gpu.MODE_FAST)
    out = as_interleaved(gpu, raw, s, gpu.OUT_F32, len(g)).astype(np.float64)
    d = np.abs(out - ref)
    print(f"fast f32 vs float64 reference: max |d| * 32768 = {d.max() * 32768.0:.6f}")
    # one LSB-equivalent plus the float32 rounding of a value below 1
    assert d.max() <= 1.0 / 32768.0 + 2.0 ** -24, d.max() * 32768.0


def test_state_export_import(gpu):
    """One stream of 12 frames cut at an odd granule: the exported state is V
    and the overlap store themselves (the ring's scale undone on export), and
    the continuation multiplies it back in."""
    g, c, _ = synth.synth_batch(1, 12, seed=31, p_mixed=0.3, p_event=0.1)
    n, cut = len(g), 13
    want, _ = oracle.dsp_streams(g, c, gpu.streams_for([n], gpu.STATE_OUT))
    s1 = gpu.streams_for([cut], gpu.STATE_OUT)
    _, st_ref = oracle.dsp_streams(g[:cut], c[:cut], s1)
    p1, st1 = gpu.decode_host(g[:cut], c[:cut], s1, mode=gpu.MODE_FAST)
    rtol = atol = 1e-4  # test_gpu_fast.py::test_fast_state_continuation's, for `store`
    for key in ("store", "vvec"):
        ref, got = st_ref[key][0], st1[key][0]
        if key == "vvec":
            # (the 16th V block is never read again: not exported)
            ref, got = ref[:, :960].reshape(2, 15, 64), got[:, :960].reshape(2, 15, 64)
        # only entries the tolerance resolves: at or above atol in the oracle
        chk = np.abs(ref) >= atol
        if key == "vvec":
            # every V index but the zero row 16, so every X[m], in both channels
            cover = chk.any(axis=1)
            assert cover[:, np.arange(64) != 16].all(), "vvec: a V index without a checked entry"
            assert chk.mean() > 0.9
        else:
            assert chk.reshape(2, -1).sum(axis=1).min() >= 50, "store: too few entries above atol"
        np.testing.assert_allclose(got[chk], ref[chk], rtol=rtol, atol=atol, err_msg=key)
        assert np.abs(got[~chk]).max(initial=0) < 2 * atol, key
    s2 = gpu.streams_for([n - cut], gpu.STATE_IN | gpu.STATE_OUT)
    p2, _ = gpu.decode_host(g[cut:], c[cut:], s2, state_in=st1, mode=gpu.MODE_FAST)
    assert_close(np.concatenate([p1, p2]), want, "continuation")
    for chunk in (1, 3):
        p3, _ = fast_plan(gpu, g[cut:], c[cut:], s2, chunk=chunk, state_in=st1)
        assert np.array_equal(p3, p2), f"continuation chunk={chunk}"
    p4, _ = gpu.decode_host(g[cut:], c[cut:], s2, state_in=st_ref, mode=gpu.MODE_FAST)
    assert_close(p4, want[cut:], "oracle state -> fast")
