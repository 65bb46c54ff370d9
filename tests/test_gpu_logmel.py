"""The log-mel features on the GPU (include/mp3g.h "log-mel features of decoded
rows"): mp3g_logmel_execute against mp3g_logmel_host bit
for bit, nothing else written, and decode_windows_logmel_tensor against the
host reference applied to the rows of decode_windows_resampled_tensor."""
import numpy as np
import pytest

import spec_logmel as spec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
GUARD = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def batch_of(T, rng):
    """[3, 2, T] float32: noise, a constant, the four impulses of the reflection,
    an all-zero row, noise scaled by 2^-120 (the power underflows to the floor)
    and noise at the domain's edge, |x| <= 2^20."""
    kinds = dict(spec.signals(T, rng))
    imp = sum(v for k, v in kinds.items() if k.startswith("impulse"))
    loud = (kinds["noise"][::-1] * np.float32(2.0 ** 20)).astype(np.float32)
    rows = [kinds["noise"], kinds["constant"], np.minimum(imp, np.float32(1.0)), kinds["zeros"], kinds["tiny"], loud]
    return np.stack(rows).reshape(3, 2, T)


def check_launch(lm, src, rows, planes, n_frames, stride):
    """One launch over src[:rows, :planes] into a sentinel-filled buffer with a
    guard row on both sides; every word against the host reference or the
    sentinel.  Returns the features compared."""
    import torch
    x = np.ascontiguousarray(src[:rows, :planes])
    buf = torch.full((rows + 2 * GUARD, planes, lm.n_mels, stride), SENTINEL, dtype=torch.int32, device="cuda")
    lm.execute(torch.from_numpy(x).cuda(), buf[GUARD:GUARD + rows].view(torch.float32), n_frames)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    want = np.full(got.shape, SENTINEL, np.uint32)
    for r in range(rows):
        for p in range(planes):
            want[GUARD + r, p, :, :n_frames] = bits(lm.host(x[r, p], n_frames))
    bad = np.argwhere(got != want)
    assert not len(bad), ((lm.n_fft, lm.hop, lm.n_mels, lm.center, lm.clamp), x.shape, n_frames, stride, len(bad),
                          bad[:6].tolist(), [(hex(got[tuple(b)]), hex(want[tuple(b)])) for b in bad[:6]])
    return rows * planes * lm.n_mels * n_frames


def lengths_for(lm):
    """T: the shortest row with a frame, the smallest with tile + 1 frames, one
    that is no multiple of hop with 2 tile + 3 frames."""
    t, hop = lm.tile_frames, lm.hop
    if lm.center:
        return lm.pad + 1, t * hop, (2 * t + 2) * hop + min(37, hop - 1)
    return lm.n_fft, lm.n_fft + t * hop, lm.n_fft + (2 * t + 2) * hop + min(37, hop - 1)


@pytest.mark.parametrize("n_fft,hop,n_mels,center,clamp", [(400, 160, 80, True, True), (400, 160, 80, True, False),
                                                           (16, 4, 4, True, False), (16, 4, 4, True, True),
                                                           (400, 160, 80, False, True)])
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, n_fft, hop, n_mels, center, clamp):
    """uint32 views: every (row, plane)'s n_mels x n_frames features are
    mp3g_logmel_host's bits; every other word of the output -- the stride's
    tail, the guard rows on both sides -- keeps its sentinel."""
    lm = gpu.LogMel(16000, n_fft, hop, n_mels, center=center, clamp=clamp, device=0)
    t = lm.tile_frames
    assert t in (8, 16, 32)
    rng = np.random.default_rng(n_fft + n_mels + 2 * center + clamp)
    T0, T1, T2 = lengths_for(lm)
    assert lm.frames(T0 - 1) == 0 and lm.frames(T1) == t + 1 and lm.frames(T1 - 1) == t and lm.frames(T2) == 2 * t + 3
    assert T2 % hop
    n = 0
    src = batch_of(T0, rng)
    for nf in sorted({1, lm.frames(T0)}):
        n += check_launch(lm, src, 3, 2, nf, nf + 3)
    src = batch_of(T1, rng)
    n += check_launch(lm, src, 3, 2, t + 1, t + 4)
    n += check_launch(lm, src, 1, 1, t, t)
    src = batch_of(T2, rng)
    for nf, rows, planes in ((1, 1, 1), (t - 1, 3, 2), (t, 1, 2), (t + 1, 3, 1), (2 * t + 3, 3, 2)):
        n += check_launch(lm, src, rows, planes, nf, nf + 5)
    n += check_launch(lm, src, 1, 2, 2 * t + 3, 2 * t + 3)
    assert n > 1000  # (the comparison is not vacuous)
    lm.close()


def test_kernel_long_transform(gpu):
    """n_fft = 1024, 128 bands at 44.1 kHz: nine passes of bin-tile pairs over four waves, the largest LDS."""
    lm = gpu.LogMel(44100, 1024, 256, 128, device=0)
    t = lm.tile_frames
    T = lengths_for(lm)[2]
    check_launch(lm, batch_of(T, np.random.default_rng(1024)), 3, 2, 2 * t + 3, 2 * t + 4)
    lm.close()


def test_kernel_short_tile_and_2d_tensors(gpu):
    """hop = n_fft = 1024: the span of 32 frames does not fit the stage, the tile
    is 8 frames and the MFMA's other rows repeat the last; [B, T] tensors are one
    plane per row."""
    import torch
    lm = gpu.LogMel(16000, 1024, 1024, 16, clamp=False, device=0)
    t = lm.tile_frames
    assert t == 8
    T = (2 * t + 2) * 1024 + 5
    x = np.random.default_rng(8).uniform(-1, 1, (2, T)).astype(np.float32)
    got = lm.execute(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (2, 16, 2 * t + 3)
    for r in range(2):
        assert np.array_equal(bits(got[r]), bits(lm.host(x[r])))
    with pytest.raises(gpu.Mp3gError):
        lm.execute(torch.from_numpy(x).cuda(), n_frames=2 * t + 4)
    lm.close()


# ---- end to end -----------------------------------------------------------------------

T_E2E = 8000  # 0.5 s at 16 kHz


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, 40-frame synthetic streams at all six sample rates and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for lsf in (False, True):
        for sfreq in range(3):
            data.append(synth.encode_stream(300 + 3 * int(lsf) + sfreq, 40, lsf=lsf, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


def check_end_to_end(gpu, streams, starts, fmt, mode, clamp):
    batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(streams, starts, T_E2E, 16000, mode=mode,
                                                                    out_format=fmt)
    feats, flen, st2, rates2 = gpu.decode_windows_logmel_tensor(streams, starts, T_E2E, mode=mode, out_format=fmt,
                                                                clamp=clamp)
    B, F = len(streams), T_E2E // 160
    planes = 2 if fmt == gpu.OUT_F32_PLANAR else 1
    assert tuple(feats.shape) == ((B, 2, 80, F) if planes == 2 else (B, 80, F))
    assert rates2.tolist() == rates.tolist() and rates[-1] == 0 and st2.tolist() == st.tolist()
    assert flen.tolist() == [min(F, -(-int(n) // 160)) for n in lengths]
    lm = gpu.LogMel(clamp=clamp)
    rows = batch.cpu().numpy().reshape(B, planes, T_E2E)
    got = feats.cpu().numpy().reshape(B, planes, 80, F)
    for k in range(B):
        for p in range(planes):
            want = lm.host(rows[k, p], F)
            assert np.array_equal(bits(got[k, p]), bits(want)), (k, p, np.argwhere(bits(got[k, p]) != bits(want))[:4])
    # the stream without a frame: an all-zero row, the floor (clamped: (-10 + 4) / 4)
    assert (got[-1] == np.float32(-1.5 if clamp else -10.0)).all()
    assert rows[:-1].any(axis=(1, 2)).all() and np.ptp(got[0]) > 0.5  # (not vacuous)
    lm.close()
    return lengths


def test_end_to_end_exact(gpu, streams):
    lengths = check_end_to_end(gpu, streams, [0] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_EXACT, True)
    assert lengths[:-1].tolist() == [T_E2E] * (len(streams) - 1) and lengths[-1] == 0
    # windows that run over each stream's end: fewer valid samples, fewer whole frames
    n_y = [gpu.Resampler(int(f), 16000).out_len(v.shape[-1]) if f else 0 for f, v in zip(
        gpu.stream_rates(streams), gpu.decode_streams_tensor(streams, out_format=gpu.OUT_F32_MONO)[1])]
    starts = [max(0, n - 3000 - 137 * k) for k, n in enumerate(n_y)]
    lengths = check_end_to_end(gpu, streams, starts, gpu.OUT_F32_MONO, gpu.MODE_EXACT, False)
    assert 0 < lengths[:-1].max() < T_E2E


def test_end_to_end_planar(gpu, streams):
    check_end_to_end(gpu, streams, [100] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_EXACT, True)


def test_end_to_end_fast_mode(gpu, streams):
    """The host reference runs on the fast-mode samples: the features add nothing mode-dependent."""
    check_end_to_end(gpu, streams, [50] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_FAST, True)


def test_arguments(gpu, streams):
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_logmel_tensor(streams[:1], [0], T_E2E, out_format=gpu.OUT_S16)
    assert e.value.status == 8
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_logmel_tensor(streams[:1], [0], T_E2E, n_frames=T_E2E // 160 + 2)
    assert e.value.status == 1
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_logmel_tensor(streams[:1], [0], T_E2E, n_fft=402)
    assert e.value.status == 8
    feats, flen, _, rates = gpu.decode_windows_logmel_tensor([], [], T_E2E)
    assert tuple(feats.shape) == (0, 80, 50) and len(flen) == 0 and len(rates) == 0
