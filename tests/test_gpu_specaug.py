"""SpecAugment on the GPU (include/mp3g.h "SpecAugment: time warp, frequency and
time masks"): mp3g_specaug_rows against mp3g_specaug_host
bit for bit -- both layouts, both fills, with the warp, without it and in place,
16-byte and scalar paths -- with nothing else written, and the spec_augment= and
cmvn= keywords of the decode_windows_*_tensor calls against the host chain."""
import numpy as np
import pytest

import spec_specaug as spec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
GUARD = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feats(rng, shape):
    x = rng.normal(-4.0, 3.0, shape).astype(np.float32)
    x.reshape(-1)[::7] = -0.0
    return x


def padded(x, freq_major, stride):
    """x [B, C, F, nb] (or [B, F, nb]) as the call reads it, the words past the live count SENTINEL."""
    src = np.swapaxes(x, -1, -2) if freq_major else x
    buf = np.full(src.shape[:-1] + (stride,), SENTINEL, np.uint32).view(np.float32)
    buf[..., :src.shape[-1]] = src
    return buf


def check(gpu, x, lengths, rows, fill=0.0, freq_major=False, warp=True, inplace=False, stride=None,
          device_lengths=False, device_rows=False):
    """The call into a sentinel-filled buffer with a guard row on both sides:
    every word is mp3g_specaug_host's or the sentinel.  Returns the host's output."""
    import torch
    live = x.shape[-2] if freq_major else x.shape[-1]
    buf = padded(x, freq_major, live if stride is None else stride)
    want = gpu.spec_augment_host(buf, lengths, rows, fill=fill, freq_major=freq_major, warp=warp, n_cols=live)
    want, want_fills = want if fill == "mean" else (want, None)
    d_in = torch.from_numpy(buf).cuda()
    obuf = torch.full((len(x) + 2 * GUARD,) + buf.shape[1:], SENTINEL, dtype=torch.int32, device="cuda")
    d_out = obuf[GUARD:GUARD + len(x)].view(torch.float32)
    if inplace:
        d_out.copy_(d_in)
        d_in = d_out
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda") if device_lengths else lengths
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).copy()).cuda() if device_rows else rows
    got = gpu.spec_augment(d_in, n, d_rows, fill=fill, freq_major=freq_major, warp=warp, out=d_out, n_cols=live)
    torch.cuda.synchronize()
    if fill == "mean":
        got, fills = got
        assert fills.dtype == torch.float32 and tuple(fills.shape) == x.shape[:-2]
        assert np.array_equal(bits(fills.cpu().numpy()), bits(want_fills)), (fills.cpu().numpy(), want_fills)
    assert got.data_ptr() == d_out.data_ptr()
    guard = np.full((GUARD,) + buf.shape[1:], SENTINEL, np.uint32)
    full = np.concatenate([guard, bits(want), guard])
    bad = np.argwhere(obuf.cpu().numpy().view(np.uint32) != full)
    assert not len(bad), (x.shape, fill, freq_major, warp, inplace, stride, len(bad), bad[:6].tolist())
    assert (bits(want[..., live:]) == SENTINEL).all()
    return want


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("n_bins,stride", [(1, 1), (13, 16), (65, 72), (80, 80)])
@pytest.mark.parametrize("F", [1, 4, 33, 65, 301])
def test_kernels_equal_the_host_reference_and_write_nothing_else(gpu, F, n_bins, stride, planes):
    """Rows of lengths 0, 1, 2, 3, 33, F and F + 9 whose descriptors walk the
    warp and mask edge cases of spec_specaug.py; both fills, both layouts, with
    the warp, without it and in place; lengths from the host and the device.  In
    the frequency-major layout the grid's padding goes after the live frames."""
    rng = np.random.default_rng(1000 * F + 10 * stride + planes)
    lengths = [0, 1, 2, 3, 33, F, F + 9]
    x = feats(rng, (len(lengths), planes, F, n_bins))
    if planes == 1 and F % 2:
        x = x[:, 0]  # a three-dimensional tensor
    k = 0
    changed = False
    for freq_major in (False, True):
        s = F + (stride - n_bins) if freq_major else stride
        for fill in (0.0, "mean", -1.5):
            for warp, inplace in ((True, False), (False, False), (False, True)):
                rows = spec.edge_rows(gpu.SPECAUG_ROW_DTYPE, lengths, F, n_bins, shift=k + F)
                want = check(gpu, x, lengths, rows, fill=fill, freq_major=freq_major, warp=warp, inplace=inplace,
                             stride=s, device_lengths=bool(k % 2))
                live = want[..., :F] if freq_major else want[..., :n_bins]
                changed = changed or not np.array_equal(bits(np.swapaxes(live, -1, -2) if freq_major else live),
                                                        bits(x))
                k += 1
    assert changed or F == 1


@pytest.mark.parametrize("freq_major", [False, True])
def test_many_short_rows_and_one_long_row(gpu, freq_major):
    """300 rows of 5 frames: more workgroups than the device runs at once; one row
    of 4,099 frames x 80: many workgroups of one plane, the fill's sums over many
    blocks of 32 frames."""
    rng = np.random.default_rng(77 + freq_major)
    lengths = [5, 4, 3, 5, 2, 5] * 50
    x = feats(rng, (300, 5, 80))
    rows = gpu.spec_augment_rows(rng, lengths, 80, time_warp=2, freq_mask_width=27, time_mask_width=2)
    rows["warp_center"][::3], rows["warp_to"][::3] = 1, 3
    check(gpu, x, lengths, rows, fill="mean", freq_major=freq_major, stride=8 if freq_major else 80)
    x = feats(rng, (1, 4099, 80))
    rows = gpu.spec_augment_rows(rng, [4099], 80, time_warp=80, time_mask_width=100, n_time_masks=10)
    assert rows["warp_center"][0] > 0
    check(gpu, x, [4099], rows, fill="mean", freq_major=freq_major, stride=4100 if freq_major else 80)
    check(gpu, x, [4000], rows, fill=0.0, freq_major=freq_major, warp=False, inplace=True,
          stride=4099 if freq_major else 80)


def test_descriptors_on_the_device(gpu):
    import torch
    rng = np.random.default_rng(5)
    lengths = [40, 33, 7, 0, 55]
    x = feats(rng, (5, 2, 40, 13))
    rows = spec.edge_rows(gpu.SPECAUG_ROW_DTYPE, lengths, 40, 13, shift=1)
    a = check(gpu, x, lengths, rows, fill="mean", stride=16)
    b = check(gpu, x, lengths, rows, fill="mean", stride=16, device_rows=True)
    assert np.array_equal(bits(a), bits(b))
    d_x = torch.from_numpy(x).cuda()
    d_rows = torch.from_numpy(rows.view(np.int32).copy()).cuda()  # int32 words
    got = gpu.spec_augment(d_x, lengths, d_rows)
    assert np.array_equal(bits(got.cpu().numpy()), bits(gpu.spec_augment_host(x, lengths, rows)))
    with pytest.raises(ValueError):
        gpu.spec_augment(d_x, lengths, d_rows[:-1])
    with pytest.raises(ValueError):
        gpu.spec_augment(d_x, lengths, rows, out=d_x)  # in place needs warp=False
    assert gpu.spec_augment(d_x, lengths, rows, warp=False, out=d_x) is d_x


# ---- end to end -----------------------------------------------------------------------

T_E2E = 8000  # 0.5 s at 16 kHz
POLICY = dict(time_warp=5, freq_mask_width=27, n_freq_masks=2, time_mask_width=10, n_time_masks=2,
              time_mask_ratio=1.0)


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, 40-frame synthetic streams at four sample rates and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for lsf in (False, True):
        for sfreq in range(2):
            data.append(synth.encode_stream(300 + 3 * int(lsf) + sfreq, 40, lsf=lsf, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


def test_fbank_cmvn_and_spec_augment_end_to_end(gpu, streams):
    starts = [0, 50, 3000, 0, 0, 0, 0]
    for fmt in (gpu.OUT_F32_MONO, gpu.OUT_F32_PLANAR):
        plain, flen, st, rates = gpu.decode_windows_fbank_tensor(streams, starts, T_E2E, out_format=fmt)
        rows = gpu.spec_augment_rows(np.random.default_rng(3), flen, 80, **POLICY)
        assert rows["warp_center"].any() and rows["time"][:, :, 1].any() and flen[-1] == 0
        got, flen2, st2, rates2 = gpu.decode_windows_fbank_tensor(streams, starts, T_E2E, out_format=fmt, cmvn="mean",
                                                                  spec_augment=rows)
        assert flen2.tolist() == flen.tolist() and st2.tolist() == st.tolist() and rates2.tolist() == rates.tolist()
        normed = gpu.cmvn_host(plain.cpu().numpy(), flen)
        want = gpu.spec_augment_host(normed, flen, rows)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want))
        assert not np.array_equal(bits(want), bits(normed))
        # cmvn= alone is the normalisation; the dict form draws the rows from the returned frame lengths
        only, _, _, _ = gpu.decode_windows_fbank_tensor(streams, starts, T_E2E, out_format=fmt, cmvn="mean")
        assert np.array_equal(bits(only.cpu().numpy()), bits(normed))
        drawn, _, _, _ = gpu.decode_windows_fbank_tensor(streams, starts, T_E2E, out_format=fmt, cmvn="mean",
                                                         spec_augment=dict(POLICY, rng=np.random.default_rng(3)))
        assert np.array_equal(bits(drawn.cpu().numpy()), bits(want))
    with pytest.raises(gpu.Mp3gError):
        gpu.decode_windows_fbank_tensor(streams[:1], [0], T_E2E, cmvn="sliding")
    with pytest.raises(gpu.Mp3gError):
        gpu.decode_windows_fbank_tensor(streams[:1], [0], T_E2E, spec_augment=dict(POLICY))  # no rng
    with pytest.raises(gpu.Mp3gError):
        gpu.decode_windows_fbank_tensor(streams[:2], [0, 0], T_E2E, spec_augment=rows[:1])


def test_logmel_and_stft_spec_augment_end_to_end(gpu, streams):
    starts = [0, 50, 3000, 0, 0, 0, 0]
    plain, flen, _, _ = gpu.decode_windows_logmel_tensor(streams, starts, T_E2E)
    got, flen2, _, _ = gpu.decode_windows_logmel_tensor(
        streams, starts, T_E2E, spec_augment=dict(POLICY, rng=np.random.default_rng(9), fill="mean"))
    rows = gpu.spec_augment_rows(np.random.default_rng(9), flen, 80, **POLICY)
    want, _ = gpu.spec_augment_host(plain.cpu().numpy(), flen, rows, fill="mean", freq_major=True)
    assert flen2.tolist() == flen.tolist() and rows["warp_center"].any()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and not np.array_equal(bits(want), bits(plain.cpu().numpy()))
    # explicit rows on the mel STFT, both planes
    kw = dict(n_fft=512, hop=160, n_mels=40, log="ln", floor=1e-10, out_format=gpu.OUT_F32_PLANAR)
    plain, flen, _, _ = gpu.decode_windows_stft_tensor(streams, starts, T_E2E, 16000, **kw)
    rows = gpu.spec_augment_rows(np.random.default_rng(10), flen, 40, **POLICY)
    got, _, _, _ = gpu.decode_windows_stft_tensor(streams, starts, T_E2E, 16000, spec_augment=rows, **kw)
    want = gpu.spec_augment_host(plain.cpu().numpy(), flen, rows, freq_major=True)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and not np.array_equal(bits(want), bits(plain.cpu().numpy()))
    with pytest.raises(gpu.Mp3gError):
        gpu.decode_windows_stft_tensor(streams[:1], [0], T_E2E, 16000, output="complex", spec_augment=rows[:1])
