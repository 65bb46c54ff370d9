"""The Kaldi MFCC features on the GPU (include/mp3g.h "Kaldi MFCC features of
decoded rows"): mp3g_mfcc_execute against mp3g_mfcc_host
bit for bit, nothing else written, and decode_windows_mfcc_tensor against the
host chain applied to the rows of decode_windows_resampled_tensor."""
import numpy as np
import pytest

import spec_fbank as fspec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
GUARD = 1
FLOOR_BITS = 0xC17F1402  # logf(2^-23)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(gpu, rate, N, hop, n_mels, n_ceps, **kw):
    mf = gpu.MFCC(rate, (N + 0.5) * 1000.0 / rate, (hop + 0.5) * 1000.0 / rate, n_mels, n_ceps, device=0, **kw)
    assert (mf.N, mf.hop) == (N, hop) and mf.tile_frames in (8, 16, 32)
    return mf


def batch_of(T, rng, tiny=False):
    """[3, 2, T] float32: noise, a constant, the four impulses of the edges, an
    all-zero row, a large offset plus small noise, and noise at |x| <= 32, which
    scale = 32768 takes to the domain's edge 2^20.  tiny: every row noise scaled
    by 2^-120 (for scale = 1: subnormal products, kept)."""
    if tiny:
        return (rng.uniform(-1.0, 1.0, (3, 2, T)) * 2.0 ** -120).astype(np.float32)
    kinds = {k: v for k, v, _ in fspec.signals(T, rng)}
    imp = sum(v for k, v in kinds.items() if k.startswith("impulse"))
    loud = (kinds["noise"][::-1] * np.float32(32.0)).astype(np.float32)
    rows = [kinds["noise"], kinds["constant"], np.minimum(imp, np.float32(1.0)), kinds["zeros"], kinds["dc+noise"], loud]
    return np.stack(rows).reshape(3, 2, T)


def reference(mf, src):
    """mp3g_mfcc_host of every (row, plane), every frame: computed once per batch."""
    return [[mf.host(src[r, p]) for p in range(src.shape[1])] for r in range(src.shape[0])]


def check_launch(mf, src, ref, rows, planes, n_frames, stride):
    """One launch over src[:rows, :planes] into a sentinel-filled buffer with a
    guard row on both sides; every word against the host reference or the
    sentinel.  Returns the features compared."""
    import torch
    x = np.ascontiguousarray(src[:rows, :planes])
    buf = torch.full((rows + 2 * GUARD, planes, n_frames, stride), SENTINEL, dtype=torch.int32, device="cuda")
    mf.execute(torch.from_numpy(x).cuda(), buf[GUARD:GUARD + rows].view(torch.float32))
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    want = np.full(got.shape, SENTINEL, np.uint32)
    for r in range(rows):
        for p in range(planes):
            want[GUARD + r, p, :, :mf.n_ceps] = bits(ref[r][p][:n_frames])
    bad = np.argwhere(got != want)
    assert not len(bad), ((mf.N, mf.hop, mf.n_mels, mf.n_ceps, mf.snip_edges), x.shape, n_frames, stride, len(bad),
                          bad[:6].tolist(), [(hex(got[tuple(b)]), hex(want[tuple(b)])) for b in bad[:6]])
    return rows * planes * mf.n_ceps * n_frames


def length_for(mf, frames):
    """The shortest row with `frames` frames, plus some samples no frame of a snipped row reads."""
    if mf.snip_edges:
        return mf.N + (frames - 1) * mf.hop + min(37, mf.hop - 1)
    T = max(mf.N, frames * mf.hop - mf.hop // 2)
    assert mf.frames(T) == frames or T == mf.N
    return T


def sweep(mf, rng, tiny=False):
    """The frame counts 1, tile - 1, tile, tile + 1, 2 tile + 3 over rows 1 and
    3, planes 1 and 2, cep_stride = n_ceps and n_ceps + 3, on one row length with
    2 tile + 3 frames (a launch may ask for fewer frames than the row has)."""
    t = mf.tile_frames
    T = length_for(mf, 2 * t + 3)
    assert mf.frames(T) == 2 * t + 3 and mf.frames(mf.N - 1) == 0
    src = batch_of(T, rng, tiny)
    ref = reference(mf, src)
    n = 0
    for nf, rows, planes, pad in ((1, 1, 1, 3), (t - 1, 3, 2, 0), (t, 1, 2, 3), (t + 1, 3, 1, 0), (2 * t + 3, 3, 2, 3),
                                  (2 * t + 3, 1, 2, 0)):
        n += check_launch(mf, src, ref, rows, planes, nf, mf.n_ceps + pad)
    return n


def full_launch(mf, rng, tiny=False):
    t = mf.tile_frames
    src = batch_of(length_for(mf, 2 * t + 3), rng, tiny)
    ref = reference(mf, src)
    check_launch(mf, src, ref, 3, 2, 2 * t + 3, mf.n_ceps + 3)
    return src, ref


@pytest.mark.parametrize("snip", [True, False])
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, snip):
    """uint32 views: every (row, plane)'s n_frames x n_ceps features are
    mp3g_mfcc_host's bits; every other word of the output -- the stride's tail,
    the guard rows on both sides -- keeps its sentinel.  Without SNIP_EDGES both
    reflections are read, and T = N has frames that reflect at both ends."""
    mf = make(gpu, 16000, 400, 160, 23, 13, snip_edges=snip)
    assert mf.tile_frames == 32 and mf.dct_in_lds
    rng = np.random.default_rng(1400 + snip)
    n = sweep(mf, rng)
    for T in (400, 400 + 160 - 1):  # T = N and T = N + hop - 1
        src = batch_of(T, rng)
        F = mf.frames(T)
        assert F == fspec.n_frames(T, 400, 160, snip) == (1 if snip else 3)
        n += check_launch(mf, src, reference(mf, src), 3, 2, F, 16)
    assert n > 1000  # (the comparison is not vacuous)
    mf.close()


def test_kernel_less_than_one_bin_tile(gpu):
    """(16, 4, 4, 4): P = 16, K = 8 bins in a tile of 32."""
    for snip in (True, False):
        mf = make(gpu, 16000, 16, 4, 4, 4, snip_edges=snip)
        assert (mf.P, mf.K) == (16, 8)
        assert sweep(mf, np.random.default_rng(16 + snip)) > 500
        mf.close()


def test_kernel_odd_window(gpu):
    """(551, 220, 80, 20) at 22.05 kHz: N = 3 mod 4, P = 1024: 16 bin tiles on 8
    waves; the energy chains' head, blocks and tail at an odd length."""
    for raw in (True, False):
        mf = make(gpu, 22050, 551, 220, 80, 20, raw_energy=raw)
        assert (mf.P, mf.K) == (1024, 512) and mf.dct_in_lds
        assert sweep(mf, np.random.default_rng(551 + raw)) > 1000
        mf.close()


def test_kernel_short_tile_largest_tables_and_2d_tensors(gpu):
    """N = hop = 1024 with 128 bins and 128 coefficients: the 8-frame tile, the
    largest L tile and the largest D, which is read from global memory; [B, T]
    tensors are one plane per row."""
    import torch
    mf = make(gpu, 16000, 1024, 1024, 128, 128)
    t = mf.tile_frames
    assert t == 8 and not mf.dct_in_lds
    T = (2 * t + 3) * 1024 + 5
    x = np.random.default_rng(8).uniform(-1, 1, (2, T)).astype(np.float32)
    got = mf.execute(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (2, 2 * t + 3, 128)
    for r in range(2):
        assert np.array_equal(bits(got[r]), bits(mf.host(x[r])))
    out = torch.empty((2, 2 * t + 4, 128), dtype=torch.float32, device="cuda")
    with pytest.raises(gpu.Mp3gError):  # more frames than the rows have
        mf.execute(torch.from_numpy(x).cuda(), out)
    with pytest.raises(gpu.Mp3gError):  # a stride below n_ceps
        mf.execute(torch.from_numpy(x).cuda(), out[:, :4, :127].contiguous())
    mf.close()
    mf = make(gpu, 16000, 1024, 1024, 128, 128, raw_energy=False, snip_edges=False)
    full_launch(mf, np.random.default_rng(9))
    mf.close()


@pytest.mark.parametrize("M,n_ceps,kw,tiny", [
    (40, 40, dict(high_freq=-400.0), False), (23, 1, {}, False), (23, 1, dict(use_energy=False), False),
    (23, 13, dict(use_energy=False), False), (23, 13, dict(raw_energy=False), False),
    (23, 13, dict(raw_energy=False, window="hamming"), False), (23, 13, dict(cepstral_lifter=0.0), False),
    (23, 13, dict(remove_dc=False), False), (23, 13, dict(remove_dc=False, raw_energy=False), False),
    (23, 13, dict(preemphasis=0.0), False), (23, 13, dict(preemphasis=0.0, raw_energy=False), False),
    (23, 13, dict(scale=1.0), True), (23, 13, dict(scale=1.0, raw_energy=False), True)])
def test_kernel_variants(gpu, M, n_ceps, kw, tiny):
    """(40, 40) with a band below Nyquist, n_ceps = 1, use_energy off, the
    windowed energy under the Povey and the Hamming window, Q = 0, REMOVE_DC off,
    preemph = 0, and scale = 1 on 2^-120-scaled noise, one full launch each."""
    mf = make(gpu, 16000, 400, 160, M, n_ceps, **kw)
    src, ref = full_launch(mf, np.random.default_rng(M + n_ceps + len(kw)), tiny)
    if tiny:
        assert (src != 0).all() and np.abs(src).max() < 2.0 ** -119
    else:
        assert np.ptp(ref[0][0]) > (1.0 if n_ceps > 1 else 0.01)
    mf.close()


def test_kernel_energy_floor(gpu):
    """energy_floor = 1.0 on a batch with an all-zero row: that row's c0 is +0."""
    mf = make(gpu, 16000, 400, 160, 23, 13, energy_floor=1.0)
    src, ref = full_launch(mf, np.random.default_rng(77))
    assert not src[1, 1].any() and (bits(ref[1][1][:, 0]) == 0).all() and (ref[0][0][:, 0] > 1.0).all()
    mf.close()
    mf = make(gpu, 16000, 400, 160, 23, 13)
    src, ref = full_launch(mf, np.random.default_rng(77))
    assert (bits(ref[1][1][:, 0]) == FLOOR_BITS).all()
    mf.close()


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
    B, F = len(streams), F_E2E if snip else (T_E2E + 80) // 160
    planes = 2 if fmt == gpu.OUT_F32_PLANAR else 1
    rows = batch.cpu().numpy().reshape(B, planes, T_E2E)
    mf = gpu.MFCC(snip_edges=snip)
    plain = np.stack([np.stack([mf.host(rows[k, p], F) for p in range(planes)]) for k in range(B)])
    mf.close()
    for cmvn in (None, "mean", "mean_var"):
        feats, flen, st2, rates2 = gpu.decode_windows_mfcc_tensor(streams, starts, T_E2E, mode=mode, out_format=fmt,
                                                                  snip_edges=snip, cmvn=cmvn)
        assert tuple(feats.shape) == ((B, 2, F, 13) if planes == 2 else (B, F, 13))
        assert rates2.tolist() == rates.tolist() and rates[-1] == 0 and st2.tolist() == st.tolist()
        if snip:
            assert flen.tolist() == [min(F, max(0, (int(n) - 400) // 160 + 1)) for n in lengths]
        else:
            assert flen.tolist() == [min(F, (int(n) + 80) // 160) for n in lengths]
        want = plain if cmvn is None else gpu.cmvn_host(plain, flen, norm_vars=cmvn == "mean_var")
        got = feats.cpu().numpy().reshape(B, planes, F, 13)
        assert np.array_equal(bits(got), bits(want)), (cmvn, np.argwhere(bits(got) != bits(want))[:4].tolist())
        # the stream without a frame: an all-zero row, untouched by the normalisation
        assert flen[-1] == 0 and (bits(got[-1, :, :, 0]) == FLOOR_BITS).all()
    assert rows[:-1].any(axis=(1, 2)).all() and np.ptp(plain[0]) > 1.0  # (not vacuous)
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
    """Argument errors raise before any launch."""
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_mfcc_tensor(streams[:1], [0], T_E2E, out_format=gpu.OUT_S16)
    assert e.value.status == 8
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_mfcc_tensor(streams[:1], [0], T_E2E, n_frames=F_E2E + 1)
    assert e.value.status == 1
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_mfcc_tensor(streams[:1], [0], T_E2E, frame_length_ms=100.0)
    assert e.value.status == 8
    for kw in (dict(n_ceps=24), dict(n_ceps=0), dict(cepstral_lifter=-1.0), dict(energy_floor=-1.0), dict(cmvn="var")):
        with pytest.raises(gpu.Mp3gError) as e:
            gpu.decode_windows_mfcc_tensor(streams[:1], [0], T_E2E, **kw)
        assert e.value.status == 1, kw
    feats, flen, _, rates = gpu.decode_windows_mfcc_tensor([], [], T_E2E, cmvn="mean")
    assert tuple(feats.shape) == (0, F_E2E, 13) and len(flen) == 0 and len(rates) == 0
    feats, flen, _, _ = gpu.decode_windows_mfcc_tensor(streams[:1], [0], T_E2E, n_frames=7, cmvn="mean_var")
    assert tuple(feats.shape) == (1, 7, 13) and flen.tolist() == [7]
