"""The per-row mean and variance normalisation's host side (include/mp3g.h
"Per-row mean and variance normalisation"):
mp3g_cmvn_host against float64 numpy within a derived tolerance, what it must
leave untouched as bits, and its refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import mp3g
import spec_mfcc as spec

U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tolerance(x, lengths, norm_vars, n_cols):
    """A bound on |y32 - y64| [like x], derived.  The sums are n-term float64
    recurrences: relative n 2^-53 on sum |x| and sum x^2, so |dmean| <= n 2^-53
    mean|x| (+ one rounding) and |dvar| <= 2 n 2^-53 (mean x^2 + mean^2) -- the
    cancellation case (mean 1e4, deviation 1e-2) pays that absolutely.  y = fl32(x -
    mean) is one float32 rounding of a float64 difference.  With NORM_VARS, vf is
    the float32 of var (relative u plus dvar / var), the square root and the
    division are correctly rounded (u each; the root halves the relative error of
    its argument) and the product is one more rounding."""
    x = np.asarray(x, np.float64)
    tol = np.zeros_like(x)
    for b in range(x.shape[0]):
        n = min(int(lengths[b]), x.shape[-2])
        if n == 0:
            continue
        part = x[b, ..., :n, :n_cols]
        e = (n + 2) * 2.0 ** -53
        amean = np.abs(part).mean(axis=-2, keepdims=True)
        mean = part.mean(axis=-2, keepdims=True)
        msq = (part * part).mean(axis=-2, keepdims=True)
        dmean = e * amean
        y = part - mean
        dy = dmean + 2.0 ** -53 * np.abs(y)
        if not norm_vars:
            tol[b, ..., :n, :n_cols] = U * (np.abs(y) + dy) + dy + 2.0 ** -149
            continue
        var = msq - mean * mean
        dvar = 2 * e * (msq + mean * mean) + 2 * np.abs(mean) * dmean
        vf = np.maximum(var, 1e-20)
        # below the floor by more than dvar the scale is the floor's exactly (to the roundings)
        rel = np.where(var + dvar < 1e-20, 0.0, dvar / np.maximum(var - dvar, 1e-20))
        scale = 1.0 / np.sqrt(vf)
        dscale = scale * (0.5 * rel + 0.5 * U + 2 * U) * 1.01
        t = (np.abs(y) + dy) * dscale + dy * scale
        tol[b, ..., :n, :n_cols] = t + 2 * U * (np.abs(y) * scale + t) + 2.0 ** -149
    return tol


def check(x, lengths, norm_vars, n_cols=None):
    cols = x.shape[-1] if n_cols is None else n_cols
    got = mp3g.cmvn_host(x, lengths, norm_vars, n_cols)
    assert got.dtype == np.float32 and got.shape == x.shape
    want = spec.cmvn64(x, lengths, norm_vars, cols)
    tol = tolerance(x, lengths, norm_vars, cols)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= tol).all(), (float((err / np.maximum(tol, 1e-300)).max()), np.argwhere(err > tol)[:4].tolist())
    # frames past the length and columns past n_cols: unchanged as bits
    keep = np.ones(x.shape, bool)
    for b in range(x.shape[0]):
        keep[b, ..., :min(int(lengths[b]), x.shape[-2]), :cols] = False
    assert np.array_equal(bits(got)[keep], bits(x)[keep])
    return got, float((err[~keep] / tol[~keep]).max()) if (~keep).any() else 0.0


@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("shape", [(5, 9, 13), (5, 2, 9, 16)])
def test_host_against_float64(shape, norm_vars):
    """Lengths 0, 1, 2, F and F + 5 (capped), all columns and fewer than the stride."""
    rng = np.random.default_rng(len(shape) + norm_vars)
    F = shape[-2]
    x = (rng.normal(0.0, 3.0, shape) + rng.uniform(-20, 20, shape[-1])).astype(np.float32)
    lengths = [0, 1, 2, F, F + 5]
    for n_cols in (None, shape[-1] - 3):
        got, worst = check(x, lengths, norm_vars, n_cols)
        print(f"{shape}, vars {norm_vars}, cols {n_cols}: worst err / tolerance = {worst:.4f}")
        cols = shape[-1] if n_cols is None else n_cols
        assert np.array_equal(bits(got[0]), bits(x[0]))            # length 0: nothing written
        assert not got[1, ..., 0, :cols].any()                      # length 1: x - x
        assert np.abs(got[3, ..., :cols].astype(np.float64).mean(axis=-2)).max() < 1e-5
        if norm_vars:
            assert np.abs(got[4, ..., :cols].astype(np.float64).std(axis=-2) - 1.0).max() < 1e-5
        assert np.array_equal(bits(got[3]), bits(mp3g.cmvn_host(x[3:4], [F + 5], norm_vars, n_cols)[0]))  # capped


def test_constant_column_and_cancellation():
    rng = np.random.default_rng(9)
    x = rng.normal(0.0, 1.0, (2, 50, 4)).astype(np.float32)
    x[:, :, 1] = np.float32(-3.25)                                   # a constant column
    x[:, :, 2] = (1e4 + 1e-2 * rng.normal(0.0, 1.0, (2, 50))).astype(np.float32)  # mean 1e4, deviation 1e-2
    for norm_vars in (False, True):
        got, worst = check(x, [50, 31], norm_vars)
        print(f"vars {norm_vars}: worst err / tolerance = {worst:.4f}")
        assert (bits(got[0, :, 1]) == 0).all() and (bits(got[1, :31, 1]) == 0).all()  # exact zeros, a finite scale
        assert np.isfinite(got).all()
    got = mp3g.cmvn_host(x, [50, 50], True)
    assert np.abs(got[:, :, 2].astype(np.float64).std(axis=1) - 1.0).max() < 0.05  # (float32 spacing at 1e4 is 1e-3)


def test_refusals():
    L = mp3g.lib()
    x = np.zeros((2, 1, 4, 6), np.float32)
    n = np.array([4, 4], np.uint32)
    px, pn = x.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p)
    assert L.mp3g_cmvn_host(px, 2, 1, 4, 6, 6, pn, 0) == 0 and L.mp3g_cmvn_host(px, 2, 1, 4, 6, 6, pn, 1) == 0
    assert L.mp3g_cmvn_host(px, 2, 1, 4, 6, 7, pn, 0) == 1    # stride < n_cols
    assert L.mp3g_cmvn_host(None, 2, 1, 4, 6, 6, pn, 0) == 1  # a null pointer with work to do
    assert L.mp3g_cmvn_host(px, 2, 1, 4, 6, 6, None, 0) == 1
    assert L.mp3g_cmvn_host(px, 2, 1, 4, 6, 6, pn, 2) == 1    # an unknown flag
    for empty in ((0, 1, 4, 6, 6), (2, 0, 4, 6, 6), (2, 1, 0, 6, 6), (2, 1, 4, 6, 0)):
        assert L.mp3g_cmvn_host(None, *empty, None, 0) == 0
    # the device call refuses the same before any device call
    assert L.mp3g_cmvn_rows(0, px, 2, 1, 4, 6, 7, pn, 0, None) == 1
    assert L.mp3g_cmvn_rows(0, None, 2, 1, 4, 6, 6, pn, 0, None) == 1
    assert L.mp3g_cmvn_rows(-1, px, 2, 1, 4, 6, 6, pn, 0, None) == 1
    assert L.mp3g_cmvn_rows(0, px, 2, 1, 4, 6, 6, pn, 4, None) == 1
    with pytest.raises(ValueError):
        mp3g.cmvn_host(x, [4])
    with pytest.raises(ValueError):
        mp3g.cmvn_host(x[0, 0], [4])
