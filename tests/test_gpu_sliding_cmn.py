"""The sliding-window CMN on the GPU (include/mp3g.h "Sliding-window CMN, energy
VAD and voiced-frame selection"): mp3g_sliding_cmn_rows
against mp3g_sliding_cmn_host bit for bit, nothing else written."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
GUARD = 1
FLAGS = list(itertools.product([False, True], [False, True]))  # (center, norm_vars)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def features(rng, shape, n_cols):
    """[.., F, stride] float32, MFCC-like; with three columns or more, column 1
    is the cancellation column (mean 1e4, deviation 1e-2) and column 2 a constant."""
    x = (rng.normal(0.0, 3.0, shape) + rng.uniform(-20, 20, shape[-1])).astype(np.float32)
    if n_cols >= 3:
        x[..., 1] = (1e4 + 1e-2 * rng.normal(0.0, 1.0, shape[:-1])).astype(np.float32)
        x[..., 2] = np.float32(3.0)
    return x


def check(gpu, x, lengths, W, mw, center, norm_vars, n_cols, device_lengths=False):
    """x [B, (C,) F, S] with sentinels in the stride's tail, normalised into a
    sentinel-filled buffer with a guard row on both sides: every word of it is
    mp3g_sliding_cmn_host's or the sentinel, and the input is unchanged."""
    import torch
    x = x.copy()
    bits(x)[..., n_cols:] = SENTINEL
    d_x = torch.from_numpy(bits(x).view(np.int32)).cuda()
    buf = torch.full((len(x) + 2 * GUARD,) + x.shape[1:], SENTINEL, dtype=torch.int32, device="cuda")
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda") if device_lengths else lengths
    out = gpu.sliding_cmn(d_x.view(torch.float32), n, W, mw, center, norm_vars,
                          out=buf[GUARD:GUARD + len(x)].view(torch.float32), n_cols=n_cols)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf[GUARD:].data_ptr()
    got = buf.cpu().numpy().view(np.uint32)
    guard = np.full((GUARD,) + x.shape[1:], SENTINEL, np.uint32)
    want = np.concatenate([guard, bits(gpu.sliding_cmn_host(x, lengths, W, mw, center, norm_vars, n_cols)), guard])
    bad = np.argwhere(got != want)
    assert not len(bad), (x.shape, W, mw, center, norm_vars, n_cols, len(bad), bad[:6].tolist(),
                          [(hex(got[tuple(b)]), hex(want[tuple(b)])) for b in bad[:6]])
    assert (want[GUARD:-GUARD][..., n_cols:] == SENTINEL).all()
    assert np.array_equal(d_x.cpu().numpy().view(np.uint32), bits(x))
    return got[GUARD:-GUARD].view(np.float32)


@pytest.mark.parametrize("n_cols,stride", [(1, 1), (13, 16), (40, 40), (65, 72)])
@pytest.mark.parametrize("F", [1, 33, 65, 301])
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, F, n_cols, stride):
    """Rows of lengths 0, 1, 33, F and F + 9, one and two planes, W = 1, 3, 64,
    300 and 600, both flags on and off; the lengths from the host and as a
    device tensor; min_window 100, 1 and above the row in turn."""
    rng = np.random.default_rng(1000 * F + stride)
    lengths = [0, 1, 33, F, F + 9]
    for planes in (1, 2):
        x = features(rng, (5, planes, F, stride), n_cols)
        for k, (W, (center, norm_vars)) in enumerate(itertools.product([1, 3, 64, 300, 600], FLAGS)):
            mw = (100, 1, F + 5)[k % 3]
            shaped = x[:, 0] if planes == 1 and k % 2 else x
            y = check(gpu, shaped, lengths, W, mw, center, norm_vars, n_cols, device_lengths=bool(k % 2))
            if n_cols >= 3:
                assert (bits(y[3][..., 2]) == 0).all()  # the constant column: +0
            if norm_vars and center and W == 1:
                assert (bits(y[3][..., :n_cols]) == 0).all()
            assert (bits(y[0][..., :n_cols]) == bits(shaped[0][..., :n_cols])).all()  # no frames: a copy


@pytest.mark.parametrize("center,norm_vars", FLAGS)
def test_kernel_long_rows_of_80_columns(gpu, center, norm_vars):
    """F = 700, 80 columns: five workgroups per row, 22 blocks; lengths 700, 333 and above F."""
    rng = np.random.default_rng(700 + center + 2 * norm_vars)
    x = features(rng, (3, 2, 700, 80), 80)
    y = check(gpu, x, [700, 333, 1000], 300, 100, center, norm_vars, 80)
    if not norm_vars:
        assert np.abs(y[0][..., 300:400, 0]).max() < 30.0


def test_many_planes(gpu):
    """600 short rows: more workgroups than the device has compute units."""
    rng = np.random.default_rng(6)
    x = features(rng, (600, 40, 13), 13)
    check(gpu, x, rng.integers(0, 45, 600).tolist(), 30, 10, True, True, 13, device_lengths=True)


def test_arguments(gpu):
    import torch
    x = torch.zeros((2, 4, 6), dtype=torch.float32, device="cuda")
    for kw in (dict(n_cols=7), dict(cmn_window=0), dict(min_window=0), dict(out=x)):
        with pytest.raises(gpu.Mp3gError) as e:
            gpu.sliding_cmn(x, [4, 4], **kw)
        assert e.value.status == 1, kw
    for bad in (x.cpu(), x.double(), x[:, :, :3], x[0]):
        with pytest.raises(ValueError):
            gpu.sliding_cmn(bad, [4, 4])
    with pytest.raises(ValueError):
        gpu.sliding_cmn(x, [4])
    with pytest.raises(ValueError):
        gpu.sliding_cmn(x, [4, 4], out=x[:1])
    assert gpu.sliding_cmn(x[:0], []).shape == (0, 4, 6)
    y = gpu.sliding_cmn(x, [4, 9])
    torch.cuda.synchronize()
    assert y.data_ptr() != x.data_ptr() and not y.any() and not x.any()
