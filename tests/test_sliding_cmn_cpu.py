"""The sliding-window CMN's host side (include/mp3g.h "Sliding-window CMN,
energy VAD and voiced-frame selection"): the window rule
over the whole grid, mp3g_sliding_cmn_host against the float64 spec within a
derived tolerance, the exact statements as bits, what it must leave untouched,
and its refusals.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mp3g
import spec_frameops as spec
from test_cmvn_cpu import tolerance as cmvn_tolerance

U = 2.0 ** -24
E = 2.0 ** -53
N_GRID = [1, 2, 31, 32, 33, 63, 64, 65, 299, 300, 301, 700]
W_GRID = [1, 2, 3, 64, 300, 600]
FLAGS = list(itertools.product([False, True], [False, True]))  # (center, norm_vars)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def min_windows(n):
    return [1, 100, n + 5]


def test_symbols_and_constants():
    L = mp3g.lib()
    for fn in ("sliding_cmn_rows", "sliding_cmn_host", "vad_energy_rows", "vad_energy_host", "select_frames_rows",
               "select_frames_host"):
        assert hasattr(L, "mp3g_" + fn)
    assert L.mp3g_abi_version() == 5
    assert (mp3g.SCMN_CENTER, mp3g.SCMN_NORM_VARS) == (1, 2)


def test_window_rule_over_the_grid():
    """0 <= s <= t < e <= n, and s and e never decrease in t and grow by at most
    one per frame (what the kernel's chains rely on), for every (n, W,
    min_window, center) of the grid."""
    for n, W, center in itertools.product(N_GRID, W_GRID, [False, True]):
        for mw in min_windows(n):
            se = np.array([spec.window(t, n, W, mw, center) for t in range(n)])
            t = np.arange(n)
            assert (0 <= se[:, 0]).all() and (se[:, 0] <= t).all() and (t < se[:, 1]).all() and (se[:, 1] <= n).all()
            d = np.diff(se, axis=0)
            assert ((d == 0) | (d == 1)).all(), (n, W, mw, center)
            if center and W >= 2 * n:
                assert (se == [0, n]).all()


def tolerance(x, lengths, W, mw, center, norm_vars, n_cols):
    """A bound on |y32 - y64| [like x], derived.  A prefix P[f] is a float64 sum
    of at most 32 + n / 32 additions in its longest chain, so its error is at
    most (n + 2) 2^-53 sum|x| over the row; the window's sum S = P[e] - P[s] pays
    that twice plus its own rounding, the mean dS / (e - s) plus the division's.
    The spec's mean is a correctly rounded sum divided once: 2 * 2^-53 |mean|.
    y = fl32(x - mean) is one float64 and one float32 rounding.  With
    NORM_VARS, var = S2 / len - mean^2 has the same prefix error on sum x^2, the
    error 2 |mean| dmean of the square and three roundings; vf = max(fl32(var),
    1e-10f) lies in [max(var - dvar, 1e-10), max(var + dvar, 1e-10)] (1 +- 2u) (the
    floor constant is a float32 too), so scale lies between the two inverse
    roots (a correctly rounded root and division: 1.5 u more; the spec's own
    root and division are float64), and the product is one more float32
    rounding.  Where the variance cancels (mean 1e4, deviation 1e-2) dvar is of
    var's order and the interval, not a linearisation, is what holds."""
    x = np.asarray(x, np.float64)
    tol = np.zeros_like(x)
    for (tp, n), (xp, _) in zip(spec.planes_of(tol, lengths), spec.planes_of(x, lengths)):
        if n == 0:
            continue
        part = xp[:n, :n_cols]
        eP = (n + 2) * E * np.abs(part).sum(axis=0)
        eP2 = (n + 2) * E * (part * part).sum(axis=0)
        for t in range(n):
            s, e = spec.window(t, n, W, mw, center)
            w = part[s:e]
            ln = e - s
            mean = w.mean(axis=0)
            dmean = (2 * eP + E * np.abs(w.sum(axis=0))) / ln + 3 * E * np.abs(mean)
            y = part[t] - mean
            dy = dmean + E * np.abs(y)
            if not norm_vars:
                tp[t, :n_cols] = U * (np.abs(y) + dy) + dy + 2.0 ** -149
                continue
            msq = (w * w).mean(axis=0)
            var = msq - mean * mean
            dvar = (2 * eP2 + E * (w * w).sum(axis=0)) / ln + 2 * np.abs(mean) * dmean + dmean ** 2 \
                + 4 * E * (msq + mean * mean)
            lo, hi = np.maximum(var - dvar, 1e-10) * (1 - 2 * U), np.maximum(var + dvar, 1e-10) * (1 + 2 * U)
            scale = 1.0 / np.sqrt(np.maximum(var, 1e-10))
            dscale = np.maximum(1.0 / np.sqrt(lo) - scale, scale - 1.0 / np.sqrt(hi)) + 1.5 * U / np.sqrt(lo)
            tt = (np.abs(y) + dy) * dscale + dy * scale
            tp[t, :n_cols] = tt + 2 * U * (np.abs(y) * scale + tt) + 2.0 ** -149
    return tol


def columns(rng, shape):
    """[.., F, 5] float32: two MFCC-like columns, the cancellation column (mean
    1e4, deviation 1e-2), a constant column, and a tail column nothing may write."""
    x = (rng.normal(0.0, 3.0, shape + (5,)) + rng.uniform(-20, 20, 5)).astype(np.float32)
    x[..., 2] = (1e4 + 1e-2 * rng.normal(0.0, 1.0, shape)).astype(np.float32)
    x[..., 3] = np.float32(3.0)
    return x


def check(x, lengths, W, mw, center, norm_vars, n_cols):
    got = mp3g.sliding_cmn_host(x, lengths, W, mw, center, norm_vars, n_cols)
    assert got.dtype == np.float32 and got.shape == x.shape
    want = spec.sliding_cmn64(x, lengths, W, mw, center, norm_vars, n_cols)
    tol = tolerance(x, lengths, W, mw, center, norm_vars, n_cols)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= tol).all(), (W, mw, center, norm_vars, float((err / np.maximum(tol, 1e-300)).max()),
                                np.argwhere(err > tol)[:4].tolist())
    keep = np.ones(x.shape, bool)
    for b in range(x.shape[0]):
        keep[b, ..., :min(int(lengths[b]), x.shape[-2]), :n_cols] = False
    assert np.array_equal(bits(got)[keep], bits(x)[keep])  # frames past the length, columns past n_cols: copies
    live = ~keep
    frac = float((err[live] / tol[live]).max()) if live.any() else 0.0
    ulp = np.spacing(np.abs(want[live]).astype(np.float32)).astype(np.float64)
    in_ulp = float((err[live] / ulp).max()) if live.any() else 0.0
    return got, frac, in_ulp


@pytest.mark.parametrize("n", N_GRID)
def test_host_against_float64_over_the_grid(n):
    """Every (W, min_window, flags) of the grid on a row of n frames in a tensor
    of n + 3: within the derived bound; the constant column is +0 as bits; with
    NORM_VARS a window of one frame (W = 1, centred) is +0."""
    rng = np.random.default_rng(n)
    x = columns(rng, (1, n + 3))
    worst = {}
    for W, (center, norm_vars) in itertools.product(W_GRID, FLAGS):
        for mw in min_windows(n):
            got, frac, in_ulp = check(x, [n], W, mw, center, norm_vars, 4)
            key = (center, norm_vars)
            worst[key] = max(worst.get(key, (0.0, 0.0)), (frac, in_ulp))
            assert (bits(got[0, :n, 3]) == 0).all(), (W, mw, center, norm_vars)  # the sums of 3.0 are exact
            if norm_vars and W == 1 and center:
                assert (bits(got[0, :n, :4]) == 0).all()
            if norm_vars:
                assert np.isfinite(got).all()
    for key, (frac, in_ulp) in sorted(worst.items()):
        print(f"n {n}, center {key[0]}, vars {key[1]}: worst err / tolerance = {frac:.4f}, err / ulp = {in_ulp:.4f}")


@pytest.mark.parametrize("center,norm_vars", FLAGS)
def test_lengths_and_planes(center, norm_vars):
    """Lengths 0, 1, below F, F and above F (capped) in one planar batch; rows of length 0 are copies."""
    rng = np.random.default_rng(7 + center + 2 * norm_vars)
    F = 70
    x = columns(rng, (5, 2, F))
    lengths = [0, 1, 41, F, F + 9]
    got, frac, _ = check(x, lengths, 64, 20, center, norm_vars, 4)
    print(f"center {center}, vars {norm_vars}: worst err / tolerance = {frac:.4f}")
    assert np.array_equal(bits(got[0]), bits(x[0]))
    assert not got[1, :, 0, :4].any()  # one frame: x - x
    capped = mp3g.sliding_cmn_host(x[4:5], [F], 64, 20, center, norm_vars, 4)
    assert np.array_equal(bits(got[4]), bits(capped[0]))
    mono = mp3g.sliding_cmn_host(x[:, 1], lengths, 64, 20, center, norm_vars, 4)
    assert np.array_equal(bits(mono), bits(got[:, 1]))


def test_whole_row_window_equals_per_utterance_cmvn():
    """Centred with W >= 2 n every window is the row, so the output is
    mp3g_cmvn_host's mean-only one -- summed in another order: within the two
    calls' derived bounds of each other, not bit for bit."""
    rng = np.random.default_rng(11)
    x = columns(rng, (3, 97))
    lengths = [97, 50, 1]
    a = mp3g.sliding_cmn_host(x, lengths, 600, 100, True, False, 4)
    b = mp3g.cmvn_host(x, lengths, False, 4)
    tol = tolerance(x, lengths, 600, 100, True, False, 4) + cmvn_tolerance(x, lengths, False, 4)
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert (err <= tol).all()
    print(f"differing words: {int((bits(a) != bits(b)).sum())} of {a.size}")


def test_refusals():
    L = mp3g.lib()
    x = np.zeros((2, 1, 4, 6), np.float32)
    y = np.zeros_like(x)
    n = np.array([4, 4], np.uint32)
    px, py, pn = (a.ctypes.data_as(C.c_void_p) for a in (x, y, n))
    host = L.mp3g_sliding_cmn_host
    assert host(px, py, 2, 1, 4, 6, 6, pn, 300, 100, 0) == 0 and host(px, py, 2, 1, 4, 6, 6, pn, 300, 100, 3) == 0
    assert host(px, py, 2, 1, 4, 6, 7, pn, 300, 100, 0) == 1    # stride < n_cols
    assert host(px, py, 2, 1, 4, 6, 6, pn, 300, 100, 4) == 1    # an unknown flag
    assert host(px, py, 2, 1, 4, 6, 6, pn, 0, 100, 0) == 1      # W = 0
    assert host(px, py, 2, 1, 4, 6, 6, pn, 300, 0, 0) == 1      # min_window = 0
    assert host(px, px, 2, 1, 4, 6, 6, pn, 300, 100, 0) == 1    # in place
    half = C.c_void_p(px.value + 4 * 24)
    assert host(px, half, 1, 1, 4, 6, 6, pn, 300, 100, 0) == 0  # row 1 from row 0: apart
    assert host(px, C.c_void_p(px.value + 4), 1, 1, 3, 6, 6, pn, 300, 100, 0) == 1  # overlapping
    for a, b, c in ((None, py, pn), (px, None, pn), (px, py, None)):  # a null pointer with work to do
        assert host(a, b, 2, 1, 4, 6, 6, c, 300, 100, 0) == 1
    for empty in ((0, 1, 4, 6, 6), (2, 0, 4, 6, 6), (2, 1, 0, 6, 6), (2, 1, 4, 6, 0)):
        assert host(None, None, *empty, None, 300, 100, 0) == 0
    # the device call refuses the same before any device call
    rows = L.mp3g_sliding_cmn_rows
    assert rows(0, px, py, 2, 1, 4, 6, 7, pn, 300, 100, 0, None) == 1
    assert rows(0, px, py, 2, 1, 4, 6, 6, pn, 300, 100, 4, None) == 1
    assert rows(0, px, py, 2, 1, 4, 6, 6, pn, 0, 100, 0, None) == 1
    assert rows(0, px, py, 2, 1, 4, 6, 6, pn, 300, 0, 0, None) == 1
    assert rows(0, px, px, 2, 1, 4, 6, 6, pn, 300, 100, 0, None) == 1
    assert rows(0, None, py, 2, 1, 4, 6, 6, pn, 300, 100, 0, None) == 1
    assert rows(-1, px, py, 2, 1, 4, 6, 6, pn, 300, 100, 0, None) == 1
    far = C.c_void_p(1 << 40), C.c_void_p(1 << 41)  # (never read: refused before any device call)
    assert rows(0, *far, 1, 1, 40960, 6, 6, pn, 300, 100, 0, None) == 8     # the row's block sums do not fit
    assert rows(0, *far, 1, 1, 20480, 6, 6, pn, 300, 100, 2, None) == 8
    assert rows(0, None, None, 0, 1, 4, 6, 6, None, 300, 100, 0, None) == 0
    with pytest.raises(ValueError):
        mp3g.sliding_cmn_host(x, [4])
    with pytest.raises(ValueError):
        mp3g.sliding_cmn_host(x[0, 0], [4])
