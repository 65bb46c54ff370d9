"""The reverberation and noise mixing on the GPU (include/mp3g.h "Room
reverberation and noise at an SNR"): mp3g_augment_rows
against mp3g_augment_host bit for bit, samples and records, nothing else
written; mp3g_row_power_rows against its host call; the object's spectra on the
device against its host copy."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no sample has
SENTINEL64 = 0x7FF8DEADDEADDEAD
GUARD = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def bank(rng, L, n=3):
    """n responses of L taps, decaying noise below 0.3 with the peak (1.0) at 0,
    in the middle and at L - 1 in turn."""
    h = (0.3 * rng.uniform(-1, 1, (n, L)) * np.exp(-np.arange(L) / max(1.0, L / 5))).astype(np.float32)
    for i in range(n):
        h[i, (0, L // 2, L - 1)[i % 3]] = 1.0
    return h


def check(gpu, x, lengths, device_lengths=False, **kw):
    """x [B, (C,) T] augmented into a sentinel-filled buffer with a guard row on
    both sides, the records likewise: every word is mp3g_augment_host's or the
    sentinel, and the input is unchanged.  Returns (out, stats) of the device."""
    import torch
    B = len(x)
    d_x = torch.from_numpy(x).cuda()
    buf = torch.full((B + 2 * GUARD,) + x.shape[1:], SENTINEL, dtype=torch.int32, device="cuda")
    sshape = x.shape[:-1] + (4,)
    sbuf = torch.full((B + 2 * GUARD,) + sshape[1:], SENTINEL64, dtype=torch.int64, device="cuda")
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda") if device_lengths else lengths
    out, stats = gpu.augment(d_x, n, out=buf[GUARD:GUARD + B].view(torch.float32),
                             stats=sbuf[GUARD:GUARD + B].view(torch.float64), **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf[GUARD:].data_ptr() and stats.data_ptr() == sbuf[GUARD:].data_ptr()
    host_kw = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items()}
    want, want_stats = gpu.augment_host(x, lengths, **host_kw)
    got = buf.cpu().numpy().view(np.uint32)
    guard = np.full((GUARD,) + x.shape[1:], SENTINEL, np.uint32)
    bad = np.argwhere(got != np.concatenate([guard, bits(want), guard]))
    assert not len(bad), (x.shape, len(bad), bad[:6].tolist())
    got_stats = sbuf.cpu().numpy().view(np.uint64)
    guard = np.full((GUARD,) + sshape[1:], SENTINEL64, np.uint64)
    bad = np.argwhere(got_stats != np.concatenate([guard, bits64(want_stats), guard]))
    assert not len(bad), (x.shape, len(bad), bad[:6].tolist(), got_stats[GUARD:-GUARD].view(np.float64)[:2],
                          want_stats[:2])
    assert np.array_equal(bits(d_x.cpu().numpy()), bits(x))
    return got[GUARD:-GUARD].view(np.float32), got_stats[GUARD:-GUARD].view(np.float64)


@pytest.fixture(scope="module")
def noise(gpu):
    """(bank float32 [4, 900], lengths): a full row, a short one, a silent one, one sample."""
    rng = np.random.default_rng(77)
    nz = (0.1 * rng.standard_normal((4, 900))).astype(np.float32)
    nz[2] = 0.0
    return nz, [900, 333, 500, 1]


@pytest.mark.parametrize("L", [1, 1024, 1025, 2500])
@pytest.mark.parametrize("T", [1, 1023, 1025, 3100])
def test_kernels_equal_host_reference_and_write_nothing_else(gpu, noise, T, L):
    """Lengths 0, 1, T - 1, T and T + 9; three peak positions; rows with and
    without a response and rows sharing one; one and two planes; 8 and 44.1 kHz;
    the lengths from the host and as a device tensor; with and without a noise."""
    rng = np.random.default_rng(1000 * T + L)
    lengths = [0, 1, T - 1, T, T + 9]
    h = bank(rng, L)
    nz, nl = noise
    for k, (fs, planes) in enumerate(((8000, 1), (8000, 2), (44100, 1), (44100, 2))):
        rv = gpu.Reverb(h, None, fs, device=0)
        x = (0.25 * rng.standard_normal((5, planes, T))).astype(np.float32)
        ri = [[2, 1, -1, 1, 0], [0, 0, 1, 2, -1]][k % 2]
        shaped = x[:, 0] if planes == 1 and k % 4 else x
        add = None if k % 2 else dict(index=[[0], [1], [-1], [3], [1]], snr_db=[[5.0], [0.0], [1.0], [12.5], [-3.0]],
                                       start=[[0], [0], [0], [T // 2], [7]], offset=[[11], [300], [0], [0], [2]],
                                       wrap=[[1], [0], [1], [1], [1]])
        check(gpu, shaped, lengths, device_lengths=bool(k % 2), reverb=rv, rir_index=ri,
              noise=nz if add else None, noise_lengths=nl if add else None, additive=add)
        rv.close()


def test_many_rows(gpu, noise):
    """600 rows of T = 1025: more workgroups than the device has compute units."""
    rng = np.random.default_rng(6)
    rv = gpu.Reverb(bank(rng, 1500, 5), [1500, 1200, 1024, 7, 1500], 16000, device=0)
    x = (0.25 * rng.standard_normal((600, 1025))).astype(np.float32)
    nz, nl = noise
    add = dict(index=rng.integers(-1, 4, (600, 1)), snr_db=rng.uniform(0, 20, (600, 1)),
               start=rng.integers(0, 1100, (600, 1)), offset=np.zeros((600, 1), np.int64), wrap=rng.integers(0, 2, (600, 1)))
    check(gpu, x, rng.integers(0, 1040, 600).tolist(), device_lengths=True, reverb=rv,
          rir_index=rng.integers(-1, 5, 600), noise=nz, noise_lengths=nl, additive=add)
    rv.close()


def test_nine_partitions(gpu):
    """L = 9000: nine partitions, an early window across two of them."""
    rng = np.random.default_rng(9)
    h = (rng.standard_normal(9000) * np.exp(-np.arange(9000) / 1500)).astype(np.float32)
    h[1000] = 6.0
    rv = gpu.Reverb(h, None, 16000, device=0)
    assert rv.info()["P"].tolist() == [9] and rv.info()["es"][0] // 1024 != (rv.info()["ee"][0] - 1) // 1024
    check(gpu, (0.25 * rng.standard_normal((1, 3100))).astype(np.float32), [3100], reverb=rv, rir_index=[0])
    rv.close()


def test_lowest_rate(gpu):
    """20 Hz, the lowest rate the object takes: the early window is the peak alone;
    a row of one sample and one that ends a sample past a block."""
    rv = gpu.Reverb(np.array([1.0, 0.5], np.float32), None, 20, device=0)
    assert (rv.info()["es"][0], rv.info()["ee"][0]) == (0, 1)
    rng = np.random.default_rng(20)
    out, _ = check(gpu, (0.25 * rng.standard_normal((3, 1025))).astype(np.float32), [1, 1025, 1024], reverb=rv,
                   rir_index=[0, 0, 0])
    assert np.isfinite(out).all()
    rv.close()
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.Reverb(np.ones(2, np.float32), None, 19, device=0)
    assert e.value.status == 8


def test_noise_cases(gpu, noise):
    """The wrap, the clip at the row's end and at the noise's, a start at and
    past the length, a silent noise, none, eight slots in order and the same
    slots swapped (another chain, checked against the host all the same), with
    and without a response; normalize on and off."""
    rng = np.random.default_rng(12)
    nz, nl = noise
    T, B = 2100, 6
    x = (0.25 * rng.standard_normal((B, 2, T))).astype(np.float32)
    lengths = [T, T - 1, 1500, 1024, 2, T]
    rv = gpu.Reverb(bank(rng, 700), None, 16000, device=0)
    add = dict(index=[[0, 1, 2, 3, -1, 1, 0, 3]] * B, snr_db=[[10, 3, 0, 20, 0, -5, 15, 8]] * B,
               start=[[0, 100, 0, 5, 0, T - 50, 1500, T + 3]] * B, offset=[[899, 0, 0, 0, 0, 300, 450, 0]] * B,
               wrap=[[1, 0, 1, 1, 1, 0, 0, 1]] * B)
    swapped = {k: [row[::-1] for row in v] for k, v in add.items()}
    outs = []
    for a in (add, swapped):
        for normalize in (True, False):
            for ri in ([-1] * B, [0, 1, 2, 0, 1, -1]):
                out, st = check(gpu, x, lengths, reverb=rv, rir_index=ri, noise=nz, noise_lengths=nl, additive=a,
                                normalize=normalize)
                outs.append(out)
                if not normalize:
                    assert (st[..., 3] == 1.0).all()
    assert not np.array_equal(bits(outs[0]), bits(outs[4]))  # the order of the slots is part of the result
    plain, _ = check(gpu, x, lengths, reverb=rv, rir_index=[-1] * B, normalize=False)
    assert np.array_equal(bits(plain[0]), bits(x[0]))
    # noise_power given, as an array and as a device tensor, equals the bank's own
    import torch
    pn = gpu.row_power_host(nz, nl)
    one = dict(index=[[0]] * B, snr_db=[[6.0]] * B, wrap=[[1]] * B)
    a, _ = check(gpu, x, lengths, noise=nz, noise_lengths=nl, additive=one)
    b, _ = check(gpu, x, lengths, noise=torch.from_numpy(nz).cuda(), noise_lengths=nl, additive=one,
                 noise_power=torch.from_numpy(pn).cuda())
    assert np.array_equal(bits(a), bits(b))
    rv.close()


@pytest.mark.parametrize("T", [1, 1023, 1024, 1025, 4096, 4097, 9000])
def test_row_power(gpu, T):
    import torch
    rng = np.random.default_rng(T)
    x = rng.standard_normal((5, T)).astype(np.float32)
    lengths = [0, 1, T - 1, T, T + 9]
    for ln in (None, lengths, torch.tensor(lengths, dtype=torch.int32, device="cuda")):
        got = gpu.row_power(torch.from_numpy(x).cuda(), ln)
        torch.cuda.synchronize()
        want = gpu.row_power_host(x, lengths if ln is not None else None)
        assert np.array_equal(bits64(got.cpu().numpy()), bits64(want)), T
    assert want[0] == 0.0 and abs(want[3] - float(np.mean(x[3].astype(np.float64) ** 2))) <= 1e-12 * want[3]


def test_spectra_on_the_device(gpu):
    rng = np.random.default_rng(4)
    rv = gpu.Reverb(bank(rng, 2500, 4), [2500, 1, 1024, 1025], 44100, device=0)
    assert rv.n_spectra == 2048 * (3 + 1 + 1 + 2)
    assert np.array_equal(bits(rv.device_spectra()), bits(rv.spectra()))
    rv.close()


def test_arguments(gpu, noise):
    import torch
    nz, nl = noise
    x = torch.zeros((2, 2, 40), dtype=torch.float32, device="cuda")
    rv = gpu.Reverb(np.ones((2, 5), np.float32), None, 16000, device=0)
    one = dict(index=[[0], [0]])
    for kw in (dict(out=x), dict(reverb=rv, rir_index=[0, 2]), dict(rir_index=[0, -1]),
               dict(noise=nz, noise_lengths=nl, additive=dict(index=[[4], [0]])),
               dict(noise=nz, noise_lengths=nl, additive=dict(one, offset=[[900], [0]])),
               dict(noise=nz, noise_lengths=nl, additive=dict(index=[[1], [0]], offset=[[333], [0]])),
               dict(noise=nz, noise_lengths=nl, additive=dict(index=[[0] * 9] * 2)), dict(additive=one)):
        with pytest.raises(gpu.Mp3gError) as e:
            gpu.augment(x, [40, 40], **kw)
        assert e.value.status == 1, kw
    with pytest.raises(gpu.Mp3gError) as e:  # out overlapping x without being it
        flat = torch.zeros(2 * 2 * 40 + 8, dtype=torch.float32, device="cuda")
        gpu.augment(flat[:160].view(2, 2, 40), [40, 40], out=flat[8:168].view(2, 2, 40))
    assert e.value.status == 1
    for bad in (x.cpu(), x.double(), x[:, :, :3], x[0, 0]):
        with pytest.raises(ValueError):
            gpu.augment(bad, None)
    with pytest.raises(ValueError):
        gpu.augment(x, [4])
    with pytest.raises(ValueError):
        gpu.augment(x, None, out=x[:1])
    # a scratch smaller than the query's, and none, through the C call
    import ctypes as C
    a = gpu._AugmentArgs()
    y, st = torch.empty_like(x), torch.zeros((2, 2, 4), dtype=torch.float64, device="cuda")
    a.x, a.out, a.stats, a.n_rows, a.n_planes, a.T = x.data_ptr(), y.data_ptr(), st.data_ptr(), 2, 2, 40
    need = gpu.lib().mp3g_reverb_scratch_bytes(rv._h, 2, 2, 40)
    assert need == (4 * 2 + 4 * 1) * 8 + 4 * 2 * 2048 * 8
    scratch = torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    for ptr, size in ((None, need), (scratch.data_ptr(), need - 8)):
        assert gpu.lib().mp3g_augment_rows(rv._h, 0, C.byref(a), None, None, None, ptr, size, None) == 1
    assert gpu.lib().mp3g_augment_rows(rv._h, 0, C.byref(a), None, None, None, scratch.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    out, st = gpu.augment(x[:0], [])
    assert out.shape == (0, 2, 40) and st.shape == (0, 2, 4)
    out, st = gpu.augment(x, [40, 90], reverb=rv, rir_index=[1, 0])
    torch.cuda.synchronize()
    assert not out.any() and st.cpu().tolist() == [[[0.0, 0.0, 0.0, 1.0]] * 2] * 2
    rv.close()
