"""The STFT features on the GPU (include/mp3g.h "STFT and mel spectrograms of
decoded rows"): mp3g_stft_execute against mp3g_stft_host
bit for bit, nothing else written, and decode_windows_stft_tensor against the
host reference applied to the rows of decode_windows_resampled_tensor."""
import numpy as np
import pytest

import spec_stft as spec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
GUARD = 1
RATE = 44100


def bits(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.float32) if a.dtype == np.complex64 else a).view(np.uint32)


def batch_of(T, rng, scale=1.0):
    """[3, 2, T] float32: noise, a constant, the four impulses of the reflection,
    an all-zero row, noise scaled by 2^-120 and noise at the domain's edge, |x|
    <= 2^20; `scale` multiplies the first (noise) row."""
    kinds = dict(spec.signals(T, rng))
    imp = sum(v for k, v in kinds.items() if k.startswith("impulse"))
    loud = (kinds["noise"][::-1] * np.float32(2.0 ** 20)).astype(np.float32)
    first = (kinds["noise"] * np.float32(scale)).astype(np.float32)
    rows = [first, kinds["constant"], np.minimum(imp, np.float32(1.0)), kinds["zeros"], kinds["tiny"], loud]
    return np.stack(rows).reshape(3, 2, T)


def check_launch(st, src, rows, planes, n_frames, stride):
    """One launch over src[:rows, :planes] into a sentinel-filled buffer with a
    guard row on both sides; every word against the host reference or the
    sentinel.  Returns the words compared."""
    import torch
    x = np.ascontiguousarray(src[:rows, :planes])
    tail = (2,) if st.complex else ()
    buf = torch.full((rows + 2 * GUARD, planes, st.bins, stride) + tail, SENTINEL, dtype=torch.int32, device="cuda")
    st.execute(torch.from_numpy(x).cuda(), buf[GUARD:GUARD + rows].view(torch.float32), n_frames)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    want = np.full(got.shape, SENTINEL, np.uint32)
    for r in range(rows):
        for p in range(planes):
            w = bits(st.host(x[r, p], n_frames))
            want[GUARD + r, p, :, :n_frames] = w.reshape((st.bins, n_frames) + tail)
    bad = np.argwhere(got != want)
    assert not len(bad), ((st.n_fft, st.hop, st.win_length, st.output, st.n_mels, st.log, st.center), x.shape,
                          n_frames, stride, len(bad), bad[:6].tolist(),
                          [(hex(got[tuple(b)]), hex(want[tuple(b)])) for b in bad[:6]])
    return rows * planes * st.bins * n_frames * (2 if st.complex else 1)


def lengths_for(st):
    """T: the shortest row with a frame, the smallest with tile + 1 frames, one
    that is no multiple of hop (where hop > 1) with 2 tile + 3 frames."""
    t, hop = st.tile_frames, st.hop
    if st.center:
        return st.pad + 1, max(t * hop, st.pad + 1), (2 * t + 2) * hop + min(37, hop - 1)
    return st.n_fft, st.n_fft + t * hop, st.n_fft + (2 * t + 2) * hop + min(37, hop - 1)


def sweep(st, rng):
    """The frame counts 1, tile - 1, tile, tile + 1, 2 tile + 3 over rows 1 and 3,
    planes 1 and 2, frame_stride = n_frames and + 5, at the smallest rows that have them."""
    t = st.tile_frames
    T0, T1, T2 = lengths_for(st)
    assert st.frames(T0 - 1) == 0 and st.frames(T0) >= 1 and st.frames(T2) == 2 * t + 3
    n = 0
    src = batch_of(T0, rng)
    for nf in sorted({1, st.frames(T0)}):
        n += check_launch(st, src, 3, 2, nf, nf + 3)
    if st.frames(T1) == t + 1:
        n += check_launch(st, batch_of(T1, rng), 1, 2, t + 1, t + 1)
    src = batch_of(T2, rng)
    for nf, rows, planes in ((1, 1, 1), (t - 1, 3, 2), (t, 1, 2), (t + 1, 3, 1), (2 * t + 3, 3, 2)):
        n += check_launch(st, src, rows, planes, nf, nf + 5)
    n += check_launch(st, src, 1, 2, 2 * t + 3, 2 * t + 3)
    return n


@pytest.mark.parametrize("n_fft", spec.SIZES)
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, n_fft):
    """Every size has its own pass structure.  Power bins, centred, hop = P / 4:
    uint32 views, every (row, plane)'s K x n_frames values are mp3g_stft_host's
    bits; every other word of the output -- the stride's tail, the guard rows on
    both sides -- keeps its sentinel.  T = pad + 1 has both reflections in one frame."""
    st = gpu.STFT(RATE, n_fft, n_fft // 4, output="power", device=0)
    assert st.tile_frames in (8, 16)
    n = sweep(st, np.random.default_rng(n_fft))
    assert n > 50000  # (the comparison is not vacuous)
    st.close()


@pytest.mark.parametrize("n_fft,hop,win,center", [(256, 256, 256, True), (512, 441, 512 - 37, True),
                                                  (1024, 441, 1024, False), (2048, 2048, 2048 - 37, False),
                                                  (4096, 441, 4096 - 37, True), (4096, 4096, 4096, False)])
def test_complex_bins_hops_windows_and_framings(gpu, n_fft, hop, win, center):
    """Complex output as bits -- the +0 imaginary parts of bins 0 and P / 2 among
    them -- with hop = P, an odd hop, a short window, centred and not."""
    st = gpu.STFT(RATE, n_fft, hop, win_length=win, output="complex", center=center, device=0)
    n = sweep(st, np.random.default_rng(n_fft + hop))
    assert n > 100000  # (not vacuous)
    x = np.random.default_rng(5).uniform(-1, 1, lengths_for(st)[2]).astype(np.float32)
    import torch
    got = st.execute(torch.from_numpy(x[None]).cuda())
    assert got.dtype == torch.complex64 and tuple(got.shape) == (1, st.K, 2 * st.tile_frames + 3)
    im = bits(got.cpu().numpy().imag.astype(np.float32))
    assert not im[0, 0].any() and not im[0, -1].any()  # +0, not -0
    assert np.abs(got.cpu().numpy()).max() > 1.0
    st.close()


@pytest.mark.parametrize("n_fft", (256, 2048, 4096))
@pytest.mark.parametrize("scale", (2.0 ** -60, 1.0, 2.0 ** 20))
def test_magnitude_over_many_exponents(gpu, n_fft, scale):
    """sqrtf on the device against the host's, as bits, on noise at 2^-60, 1 and 2^20."""
    st = gpu.STFT(RATE, n_fft, n_fft // 4, output="magnitude", device=0)
    t = st.tile_frames
    src = batch_of(lengths_for(st)[2], np.random.default_rng(n_fft), scale)
    n = check_launch(st, src, 3, 2, t + 1, t + 6)
    assert n > 10000  # (not vacuous)
    st.close()


@pytest.mark.parametrize("n_fft,output,n_mels,htk,norm,log,floor",
                         [(2048, "power", 80, False, True, None, None), (2048, "magnitude", 128, True, False, None, None),
                          (1024, "power", 128, True, True, "log10", 1e-10), (4096, "magnitude", 80, False, False, "ln", 1e-5),
                          (256, "power", 128, False, True, "ln", 1e-3), (512, "power", 80, True, False, "log10", 1e-2)])
def test_mel_and_logarithms(gpu, n_fft, output, n_mels, htk, norm, log, floor):
    """Mel of power and of magnitude, 80 and 128 bands, both scales, both
    normalisations, both logarithms; at P = 256, 128 bands leave empty filters."""
    st = gpu.STFT(RATE, n_fft, n_fft // 4, output=output, n_mels=n_mels, htk=htk, norm=norm, log=log, floor=floor,
                  device=0)
    empty = int((st.support[:, 0] > st.support[:, 1]).sum())
    assert empty > 0 or n_fft != 256
    t = st.tile_frames
    src = batch_of(lengths_for(st)[2], np.random.default_rng(n_fft + n_mels))
    n = check_launch(st, src, 3, 2, 2 * t + 3, 2 * t + 8) + check_launch(st, src, 1, 1, t - 1, t - 1)
    assert n > 5000  # (not vacuous)
    if log:  # the floor is hit by some entries (the all-zero row: by all) and not by others
        noise, quiet = st.host(src[0, 0]), st.host(src[1, 1])
        assert (quiet == quiet[0, 0]).all() and (noise > quiet[0, 0]).any()
    st.close()


def test_log_of_bins_with_a_floor_some_entries_hit(gpu):
    """No mel bank: the logarithm of the power bins, floor = 1 -- noise lies on both sides of it."""
    for log in ("ln", "log10"):
        st = gpu.STFT(RATE, 512, 128, output="power", log=log, floor=1.0, device=0)
        src = batch_of(lengths_for(st)[2], np.random.default_rng(9))
        y = st.host(src[0, 0])
        assert (y == 0).any() and (y > 0).any()
        assert check_launch(st, src, 3, 2, st.tile_frames + 1, st.tile_frames + 6) > 10000
        st.close()


def test_2d_tensors_and_arguments(gpu):
    import torch
    st = gpu.STFT(RATE, 1024, 256, device=0)
    x = np.random.default_rng(8).uniform(-1, 1, (2, 5000)).astype(np.float32)
    got = st.execute(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (2, 513, 5000 // 256 + 1)
    for r in range(2):
        assert np.array_equal(bits(got[r]), bits(st.host(x[r])))
    with pytest.raises(gpu.Mp3gError):
        st.execute(torch.from_numpy(x).cuda(), n_frames=5000 // 256 + 2)
    st.close()


# ---- end to end -----------------------------------------------------------------------

T_E2E = 6000


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, 40-frame synthetic streams at all six sample rates and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for lsf in (False, True):
        for sfreq in range(3):
            data.append(synth.encode_stream(300 + 3 * int(lsf) + sfreq, 40, lsf=lsf, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


def check_end_to_end(gpu, streams, rate, starts, fmt, mode, **kw):
    batch, lengths, status, rates = gpu.decode_windows_resampled_tensor(streams, starts, T_E2E, rate, mode=mode,
                                                                        out_format=fmt)
    feats, flen, status2, rates2 = gpu.decode_windows_stft_tensor(streams, starts, T_E2E, rate, mode=mode,
                                                                  out_format=fmt, **kw)
    st = gpu.STFT(rate, **kw)
    B, F = len(streams), T_E2E // st.hop if st.center else st.frames(T_E2E)
    planes = 2 if fmt == gpu.OUT_F32_PLANAR else 1
    assert tuple(feats.shape) == ((B, 2, st.bins, F) if planes == 2 else (B, st.bins, F))
    assert rates2.tolist() == rates.tolist() and rates[-1] == 0 and status2.tolist() == status.tolist()
    assert flen.tolist() == [min(F, -(-int(n) // st.hop)) for n in lengths]
    rows = batch.cpu().numpy().reshape(B, planes, T_E2E)
    got = feats.cpu().numpy().reshape(B, planes, st.bins, F)
    for k in range(B):
        for p in range(planes):
            want = st.host(rows[k, p], F)
            assert np.array_equal(bits(got[k, p]), bits(want)), (k, p, np.argwhere(bits(got[k, p]) != bits(want))[:4])
    assert rows[:-1].any(axis=(1, 2)).all() and not rows[-1].any() and np.ptp(np.abs(got[0])) > 0  # (not vacuous)
    st.close()
    return rates


def test_end_to_end_native_rate_copied_rows(gpu, streams):
    """rate = 44,100: the streams already at it are copied, the others resampled; exact mode, mono, complex bins."""
    rates = check_end_to_end(gpu, streams, 44100, [0] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_EXACT, n_fft=2048,
                             hop=512, output="complex")
    assert (rates == 44100).any() and ((rates != 44100) & (rates != 0)).any()
    check_end_to_end(gpu, streams, 48000, [100] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_FAST, n_fft=4096, hop=1024,
                     output="magnitude")


def test_end_to_end_resampled_mel(gpu, streams):
    """rate = 22,050: librosa's mel defaults in dB-less form; fast mode planar, exact mode mono."""
    kw = dict(n_fft=1024, hop=256, output="power", n_mels=80, log="log10", floor=1e-10)
    check_end_to_end(gpu, streams, 22050, [50] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_FAST, **kw)
    check_end_to_end(gpu, streams, 22050, [0] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_EXACT, center=False, **kw)


def test_end_to_end_arguments(gpu, streams):
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_stft_tensor(streams[:1], [0], T_E2E, 44100, out_format=gpu.OUT_S16)
    assert e.value.status == 8
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_stft_tensor(streams[:1], [0], T_E2E, 44100, n_frames=T_E2E // 512 + 2)
    assert e.value.status == 1
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_stft_tensor(streams[:1], [0], T_E2E, 44100, n_fft=400)
    assert e.value.status == 8
    feats, flen, _, rates = gpu.decode_windows_stft_tensor([], [], T_E2E, 44100, n_fft=1024, hop=256)
    assert tuple(feats.shape) == (0, 513, T_E2E // 256) and len(flen) == 0 and len(rates) == 0
