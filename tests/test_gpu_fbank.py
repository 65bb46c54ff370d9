"""The Kaldi filter-bank features on the GPU (include/mp3g.h "Kaldi filter-bank
features of decoded rows"): mp3g_fbank_execute against
mp3g_fbank_host bit for bit, nothing else written, and
decode_windows_fbank_tensor against the host reference applied to the rows of
decode_windows_resampled_tensor."""
import numpy as np
import pytest

import spec_fbank as spec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
GUARD = 1
FLOOR = np.float32(-23.0 * np.log(2.0))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(gpu, rate, N, hop, n_mels, **kw):
    fb = gpu.FBank(rate, (N + 0.5) * 1000.0 / rate, (hop + 0.5) * 1000.0 / rate, n_mels, device=0, **kw)
    assert (fb.N, fb.hop) == (N, hop) and fb.tile_frames in (8, 16, 32)
    return fb


def batch_of(T, rng, tiny=False):
    """[3, 2, T] float32: noise, a constant, the four impulses of the edges, an
    all-zero row, a large offset plus small noise, and noise at |x| <= 32, which
    scale = 32768 takes to the domain's edge 2^20.  tiny: every row noise scaled
    by 2^-120 (for scale = 1: subnormal products, kept)."""
    if tiny:
        return (rng.uniform(-1.0, 1.0, (3, 2, T)) * 2.0 ** -120).astype(np.float32)
    kinds = {k: v for k, v, _ in spec.signals(T, rng)}
    imp = sum(v for k, v in kinds.items() if k.startswith("impulse"))
    loud = (kinds["noise"][::-1] * np.float32(32.0)).astype(np.float32)
    rows = [kinds["noise"], kinds["constant"], np.minimum(imp, np.float32(1.0)), kinds["zeros"], kinds["dc+noise"], loud]
    return np.stack(rows).reshape(3, 2, T)


def reference(fb, src):
    """mp3g_fbank_host of every (row, plane), every frame: computed once per batch."""
    return [[fb.host(src[r, p]) for p in range(src.shape[1])] for r in range(src.shape[0])]


def check_launch(fb, src, ref, rows, planes, n_frames, stride):
    """One launch over src[:rows, :planes] into a sentinel-filled buffer with a
    guard row on both sides; every word against the host reference or the
    sentinel.  Returns the features compared."""
    import torch
    x = np.ascontiguousarray(src[:rows, :planes])
    buf = torch.full((rows + 2 * GUARD, planes, n_frames, stride), SENTINEL, dtype=torch.int32, device="cuda")
    fb.execute(torch.from_numpy(x).cuda(), buf[GUARD:GUARD + rows].view(torch.float32))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    want = np.full(got.shape, SENTINEL, np.uint32)
    for r in range(rows):
        for p in range(planes):
            want[GUARD + r, p, :, :fb.n_mels] = bits(ref[r][p][:n_frames])
    bad = np.argwhere(got != want)
    assert not len(bad), ((fb.N, fb.hop, fb.n_mels, fb.snip_edges), x.shape, n_frames, stride, len(bad),
                          bad[:6].tolist(), [(hex(got[tuple(b)]), hex(want[tuple(b)])) for b in bad[:6]])
    return rows * planes * fb.n_mels * n_frames


def length_for(fb, frames):
    """The shortest row with `frames` frames, plus some samples no frame of a snipped row reads."""
    if fb.snip_edges:
        return fb.N + (frames - 1) * fb.hop + min(37, fb.hop - 1)
    T = max(fb.N, frames * fb.hop - fb.hop // 2)
    assert fb.frames(T) == frames or T == fb.N
    return T


def sweep(fb, rng, tiny=False):
    """The frame counts 1, tile - 1, tile, tile + 1, 2 tile + 3 over rows 1 and
    3, planes 1 and 2, mel_stride = n_mels and n_mels + 3, on one row length with
    2 tile + 3 frames (a launch may ask for fewer frames than the row has)."""
    t = fb.tile_frames
    T = length_for(fb, 2 * t + 3)
    assert fb.frames(T) == 2 * t + 3 and fb.frames(fb.N - 1) == 0
    src = batch_of(T, rng, tiny)
    ref = reference(fb, src)
    n = 0
    for nf, rows, planes, pad in ((1, 1, 1, 3), (t - 1, 3, 2, 0), (t, 1, 2, 3), (t + 1, 3, 1, 0), (2 * t + 3, 3, 2, 3),
                                  (2 * t + 3, 1, 2, 0)):
        n += check_launch(fb, src, ref, rows, planes, nf, fb.n_mels + pad)
    return n


@pytest.mark.parametrize("snip", [True, False])
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, snip):
    """uint32 views: every (row, plane)'s n_frames x n_mels features are
    mp3g_fbank_host's bits; every other word of the output -- the stride's tail,
    the guard rows on both sides -- keeps its sentinel.  Without SNIP_EDGES both
    reflections are read, and T = N has frames that reflect at both ends."""
    fb = make(gpu, 16000, 400, 160, 80, snip_edges=snip)
    assert fb.tile_frames == 32
    rng = np.random.default_rng(400 + snip)
    n = sweep(fb, rng)
    for T in (400, 400 + 160 - 1):  # T = N and T = N + hop - 1
        src = batch_of(T, rng)
        F = fb.frames(T)
        assert F == spec.n_frames(T, 400, 160, snip) == (1 if snip else 3)
        n += check_launch(fb, src, reference(fb, src), 3, 2, F, 83)
    assert n > 1000  # (the comparison is not vacuous)
    fb.close()


def test_kernel_less_than_one_bin_tile(gpu):
    """(16, 4, 4): P = 16, K = 8 bins in a tile of 32."""
    for snip in (True, False):
        fb = make(gpu, 16000, 16, 4, 4, snip_edges=snip)
        assert (fb.P, fb.K) == (16, 8)
        assert sweep(fb, np.random.default_rng(16 + snip)) > 500
        fb.close()


def test_kernel_odd_window_two_bin_tiles_per_wave(gpu):
    """(551, 220, 80) at 22.05 kHz: N = 3 mod 4 (zero table rows up to 552), P =
    1024: 16 bin tiles on 8 waves and the LDS raised above 64 KB."""
    fb = make(gpu, 22050, 551, 220, 80)
    assert (fb.P, fb.K) == (1024, 512)
    assert sweep(fb, np.random.default_rng(551)) > 1000
    fb.close()
    fb = make(gpu, 22050, 551, 220, 80, snip_edges=False)
    t = fb.tile_frames
    src = batch_of(length_for(fb, t + 1), np.random.default_rng(552))
    check_launch(fb, src[:1], reference(fb, src[:1]), 1, 2, t + 1, 80)
    fb.close()


def test_kernel_short_tile_and_2d_tensors(gpu):
    """N = hop = 1024: the span of 32 frames does not fit the stage, the tile is 8
    frames and the MFMA's other rows repeat the last; [B, T] tensors are one
    plane per row."""
    import torch
    fb = make(gpu, 16000, 1024, 1024, 16)
    t = fb.tile_frames
    assert t == 8
    T = (2 * t + 3) * 1024 + 5
    x = np.random.default_rng(8).uniform(-1, 1, (2, T)).astype(np.float32)
    got = fb.execute(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (2, 2 * t + 3, 16)
    for r in range(2):
        assert np.array_equal(bits(got[r]), bits(fb.host(x[r])))
    out = torch.empty((2, 2 * t + 4, 16), dtype=torch.float32, device="cuda")
    with pytest.raises(gpu.Mp3gError):  # more frames than the rows have
        fb.execute(torch.from_numpy(x).cuda(), out)
    with pytest.raises(gpu.Mp3gError):  # a stride below n_mels
        fb.execute(torch.from_numpy(x).cuda(), out[:, :4, :15].contiguous())
    fb.close()


@pytest.mark.parametrize("n_mels,kw,tiny", [(128, {}, False), (80, dict(remove_dc=False), False),
                                            (80, dict(preemphasis=0.0), False), (80, dict(window="hamming"), False),
                                            (80, dict(scale=1.0), True), (80, dict(scale=1.0, remove_dc=False), True)])
def test_kernel_variants(gpu, n_mels, kw, tiny):
    """128 bands with the empty filter, REMOVE_DC off, preemph = 0, Hamming, and
    scale = 1 on 2^-120-scaled noise (subnormals kept), one full launch each;
    scale = 32768 on |x| <= 32 is a row of every batch."""
    fb = make(gpu, 16000, 400, 160, n_mels, **kw)
    if n_mels == 128:
        assert sum(1 for lo, hi in fb.support if lo > hi) == 1
    t = fb.tile_frames
    src = batch_of(length_for(fb, 2 * t + 3), np.random.default_rng(n_mels + len(kw)), tiny)
    ref = reference(fb, src)
    if tiny:  # subnormal operands reach the spectrum: not every feature is the floor
        assert (src != 0).all() and np.abs(src).max() < 2.0 ** -119
    else:
        assert np.ptp(ref[0][0]) > 1.0
    check_launch(fb, src, ref, 3, 2, 2 * t + 3, n_mels + 3)
    fb.close()


# ---- end to end -----------------------------------------------------------------------

T_E2E = 8000  # 0.5 s at 16 kHz
F_E2E = 1 + (T_E2E - 400) // 160


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, 40-frame synthetic streams at all six sample rates and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for lsf in (False, True):
        for sfreq in range(3):
            data.append(synth.encode_stream(300 + 3 * int(lsf) + sfreq, 40, lsf=lsf, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


def check_end_to_end(gpu, streams, starts, fmt, mode, snip=True):
    batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(streams, starts, T_E2E, 16000, mode=mode,
                                                                    out_format=fmt)
    feats, flen, st2, rates2 = gpu.decode_windows_fbank_tensor(streams, starts, T_E2E, mode=mode, out_format=fmt,
                                                               snip_edges=snip)
    B, F = len(streams), F_E2E if snip else (T_E2E + 80) // 160
    planes = 2 if fmt == gpu.OUT_F32_PLANAR else 1
    assert tuple(feats.shape) == ((B, 2, F, 80) if planes == 2 else (B, F, 80))
    assert rates2.tolist() == rates.tolist() and rates[-1] == 0 and st2.tolist() == st.tolist()
    if snip:
        assert flen.tolist() == [min(F, max(0, (int(n) - 400) // 160 + 1)) for n in lengths]
    else:
        assert flen.tolist() == [min(F, (int(n) + 80) // 160) for n in lengths]
    fb = gpu.FBank(snip_edges=snip)
    rows = batch.cpu().numpy().reshape(B, planes, T_E2E)
    got = feats.cpu().numpy().reshape(B, planes, F, 80)
    for k in range(B):
        for p in range(planes):
            want = fb.host(rows[k, p], F)
            assert np.array_equal(bits(got[k, p]), bits(want)), (k, p, np.argwhere(bits(got[k, p]) != bits(want))[:4])
    # the stream without a frame: an all-zero row, the floor
    assert (got[-1] == FLOOR).all() and flen[-1] == 0
    assert rows[:-1].any(axis=(1, 2)).all() and np.ptp(got[0]) > 1.0  # (not vacuous)
    fb.close()
    return lengths


def test_end_to_end_exact(gpu, streams):
    lengths = check_end_to_end(gpu, streams, [0] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_EXACT)
    assert lengths[:-1].tolist() == [T_E2E] * (len(streams) - 1) and lengths[-1] == 0
    # windows that run over each stream's end: fewer valid samples, fewer whole frames
    n_y = [gpu.Resampler(int(f), 16000).out_len(v.shape[-1]) if f else 0 for f, v in zip(
        gpu.stream_rates(streams), gpu.decode_streams_tensor(streams, out_format=gpu.OUT_F32_MONO)[1])]
    starts = [max(0, n - 3000 - 137 * k) for k, n in enumerate(n_y)]
    lengths = check_end_to_end(gpu, streams, starts, gpu.OUT_F32_MONO, gpu.MODE_EXACT, snip=False)
    assert 0 < lengths[:-1].max() < T_E2E


def test_end_to_end_planar(gpu, streams):
    check_end_to_end(gpu, streams, [100] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_EXACT)


def test_end_to_end_fast_mode(gpu, streams):
    """The host reference runs on the fast-mode samples: the features add nothing mode-dependent."""
    check_end_to_end(gpu, streams, [50] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_FAST)
    check_end_to_end(gpu, streams, [50] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_FAST)


def test_arguments(gpu, streams):
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_fbank_tensor(streams[:1], [0], T_E2E, out_format=gpu.OUT_S16)
    assert e.value.status == 8
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_fbank_tensor(streams[:1], [0], T_E2E, n_frames=F_E2E + 1)
    assert e.value.status == 1
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_fbank_tensor(streams[:1], [0], T_E2E, frame_length_ms=100.0)
    assert e.value.status == 8
    feats, flen, _, rates = gpu.decode_windows_fbank_tensor([], [], T_E2E)
    assert tuple(feats.shape) == (0, F_E2E, 80) and len(flen) == 0 and len(rates) == 0
    feats, flen, _, _ = gpu.decode_windows_fbank_tensor(streams[:1], [0], T_E2E, n_frames=7)
    assert tuple(feats.shape) == (1, 7, 80) and flen.tolist() == [7]
