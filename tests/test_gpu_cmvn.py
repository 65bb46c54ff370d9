"""The per-row mean and variance normalisation on the GPU (include/mp3g.h
"Per-row mean and variance normalisation"): mp3g_cmvn_rows
against mp3g_cmvn_host bit for bit, nothing else written."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
GUARD = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(gpu, x, lengths, norm_vars, n_cols, device_lengths=False):
    """x [B, (C,) F, S] between two guard rows of sentinels, normalised in place
    on the device: every word is mp3g_cmvn_host's, and with it every word the
    call must leave alone (the stride's tail holds sentinels too)."""
    import torch
    x = x.copy()
    bits(x)[..., n_cols:] = SENTINEL
    guard = np.full((GUARD,) + x.shape[1:], SENTINEL, np.uint32)
    buf = torch.from_numpy(np.concatenate([guard, bits(x), guard]).view(np.int32)).cuda()
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda") if device_lengths else lengths
    out = gpu.cmvn(buf[GUARD:GUARD + len(x)].view(torch.float32), n, norm_vars=norm_vars, n_cols=n_cols)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf[GUARD:].data_ptr()
    got = buf.cpu().numpy().view(np.uint32)
    want = np.concatenate([guard, bits(gpu.cmvn_host(x, lengths, norm_vars, n_cols)), guard])
    bad = np.argwhere(got != want)
    assert not len(bad), (x.shape, norm_vars, n_cols, len(bad), bad[:6].tolist(),
                          [(hex(got[tuple(b)]), hex(want[tuple(b)])) for b in bad[:6]])
    assert (want[GUARD:-GUARD][..., n_cols:] == SENTINEL).all()
    return got[GUARD:-GUARD].view(np.float32)


@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("planes,stride", [(1, 13), (2, 13), (1, 16), (2, 16)])
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, planes, stride, norm_vars):
    """(rows 3, F = 7, 13 columns) with lengths 0, 1 and 7; a constant column."""
    rng = np.random.default_rng(13 * planes + stride + norm_vars)
    x = (rng.normal(0.0, 4.0, (3, planes, 7, stride)) + rng.uniform(-30, 30, stride)).astype(np.float32)
    x[:, :, :, 5] = np.float32(2.5)  # a constant column: exact zeros, a finite scale through the floor
    for shaped in (x, x[:, 0]) if planes == 1 else (x,):
        y = check(gpu, shaped, [0, 1, 7], norm_vars, 13)
        assert (bits(y[2][..., 5]) == 0).all() and (bits(y[0][..., :13]) == bits(shaped[0][..., :13])).all()
        assert not y[1][..., 0, :13].any() and np.isfinite(y[..., :13]).all()
    check(gpu, x, [9, 3, 12], norm_vars, 13, device_lengths=True)  # capped at F


@pytest.mark.parametrize("norm_vars", [False, True])
def test_kernel_long_rows_of_80_columns(gpu, norm_vars):
    """F = 300, 80 columns: more than one workgroup; log-mel-like values and the cancellation column."""
    rng = np.random.default_rng(300 + norm_vars)
    x = (rng.normal(0.0, 2.0, (3, 2, 300, 80)) - 12.0).astype(np.float32)
    x[:, :, :, 7] = (1e4 + 1e-2 * rng.normal(0.0, 1.0, (3, 2, 300))).astype(np.float32)
    y = check(gpu, x, [300, 151, 1000], norm_vars, 80)
    assert np.abs(y[0].astype(np.float64).mean(axis=-2)).max() < 1e-4


def test_arguments(gpu):
    import torch
    x = torch.zeros((2, 4, 6), dtype=torch.float32, device="cuda")
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.cmvn(x, [4, 4], n_cols=7)
    assert e.value.status == 1
    for bad in (x.cpu(), x.double(), x[:, :, :3], x[0]):
        with pytest.raises(ValueError):
            gpu.cmvn(bad, [4, 4])
    with pytest.raises(ValueError):
        gpu.cmvn(x, [4])
    assert gpu.cmvn(x[:0], []).shape == (0, 4, 6)
    assert not x.any()
