"""Delta features and frame context, host side (include/mp3g.h "Delta features and
frame context"): mp3g_delta_scales against the recurrence
in numpy float32 and in exact fractions, mp3g_add_deltas_host against the float64
statement within the bound spec_framectx.py derives, order 1 against torch's
conv1d, the bit copies, mp3g_stack_frames_host word for word against the index
statement and against FunASR's apply_lfr loop, per-plane lengths, the words that
must stay untouched, the refusals and the sanitizer build of the new host code.
No GPU.

Observed worst |y - y64| / bound of test_deltas_against_the_float64_statement, per
(order, window) over rows of 0, 1, 2, 3, 5, 33, 301 and 310 frames (a bound of 1
would be reached exactly): (1,2) 0.29, (2,2) 0.36, (2,3) 0.37, (3,1) 0.20,
(1,9) 0.14, (4,8) 0.14; (0,1) has no arithmetic.  The scales: delta_scales(2, 2)
is within 0.20 of its own bound, which is at most 8.0 ulp of the entry (at the
two entries of 1/100, whose sums carry the roundings of terms four times their
size)."""
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_framectx as spec
from conftest import REPO

SENTINEL = 0x7FC0DEAD
ROW_FRAMES = [1, 2, 3, 5, 33, 301]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feats(rng, shape):
    x = rng.normal(-4.0, 3.0, shape).astype(np.float32)
    x.reshape(-1)[::7] = -0.0
    return x


def ulp(v):
    return float(np.spacing(np.float32(abs(v))))


# ---- scales ---------------------------------------------------------------------------

def test_order_1_scales_are_j_times_a_tenth():
    s = mp3g.delta_scales(1, 2)
    assert [len(a) for a in s] == [1, 5] and s[0][0] == 1.0
    want = np.array([-2, -1, 0, 1, 2], np.float32) * np.float32(0.1)
    assert np.array_equal(bits(s[1]), bits(want))


def test_order_2_scales_are_the_integer_filter_within_the_derived_bound():
    s2 = mp3g.delta_scales(2, 2)[2]
    ints = [4, 4, 1, -4, -10, -4, 1, 4, 4]
    exact = spec.scales_exact(2, 2)[2]
    assert [e * 100 for e in exact] == ints
    E = spec.scale_bounds(2, 2)[2]
    worst = 0.0
    for k in range(9):
        err = abs(float(s2[k]) - float(exact[k]))
        assert err <= float(E[k]), (k, err, float(E[k]))
        worst = max(worst, err / float(E[k]))
        # symmetric up to the two entries' roundings; zero exactly where the integer filter is
        assert abs(float(s2[k]) - float(s2[8 - k])) <= float(E[k] + E[8 - k])
        assert (s2[k] == 0) == (ints[k] == 0)
    print("delta_scales(2, 2): worst error / bound = %.3f, bound / ulp <= %.2f"
          % (worst, max(float(E[k]) / ulp(float(exact[k])) for k in range(9))))
    s1 = mp3g.delta_scales(1, 2)[1]
    assert [v == 0 for v in s1] == [False, False, True, False, False]


@pytest.mark.parametrize("order,window", spec.DELTA_SETS + [(4, 1), (1, 32), (2, 16), (0, 40)])
def test_scales_equal_the_float32_recurrence_bit_for_bit(order, window):
    got, want = mp3g.delta_scales(order, window), spec.scales_f32(order, window)
    assert len(got) == order + 1
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(bits(g), bits(w))
    E, exact = spec.scale_bounds(order, window), spec.scales_exact(order, window)
    for i in range(order + 1):
        for k in range(len(exact[i])):
            assert abs(float(got[i][k]) - float(exact[i][k])) <= float(E[i][k]), (i, k)


def test_scales_refusals():
    for order, window, status in ((1, 0, 1), (5, 1, 8), (2, 17, 8), (4, 9, 8), (1, 33, 8)):
        with pytest.raises(mp3g.Mp3gError) as e:
            mp3g.delta_scales(order, window)
        assert e.value.status == status, (order, window)
    assert mp3g.lib().mp3g_delta_scales(1, 2, None) == 1


# ---- deltas ---------------------------------------------------------------------------

@pytest.mark.parametrize("order,window", spec.DELTA_SETS)
def test_deltas_against_the_float64_statement(order, window):
    """Rows of 0, 1, 2, 3, 5, 33, 301 and F + 9 frames in a batch of F = 301, 13
    live columns of a stride of 16: every word within the derived bound (no case
    excluded), block 0 and the zero padding bit for bit."""
    rng = np.random.default_rng(100 * order + window)
    lengths = [0] + ROW_FRAMES + [310]
    F, cols = 301, 13
    x = feats(rng, (len(lengths), F, 16))
    got = mp3g.add_deltas_host(x, lengths, order, window, n_cols=cols)
    assert got.shape == (len(lengths), F, (order + 1) * cols) and got.dtype == np.float32
    scales = mp3g.delta_scales(order, window)
    worst = 0.0
    for r, n in enumerate(lengths):
        n = min(n, F)
        y64, bound = spec.deltas_spec(x[r, :, :cols], n, order, window, scales)
        g = got[r].reshape(F, order + 1, cols)
        assert np.array_equal(bits(g[:n, 0]), bits(x[r, :n, :cols]))
        assert not bits(g[n:]).any(), "frames past the length are +0"
        if order and n:
            err = np.abs(g[:n, 1:].astype(np.float64) - y64[:n, 1:])
            assert (err <= bound[:n, 1:]).all(), (n, float((err / bound[:n, 1:]).max()))
            worst = max(worst, float((err / bound[:n, 1:]).max()))
    print("add_deltas_host (%d, %d): worst error / bound = %.3f" % (order, window, worst))
    assert worst < 1.0 and (worst > 0.0 or order == 0)


def test_order_2_is_not_order_1_applied_twice():
    """The same in a row's interior (up to the roundings), different within 2 W
    frames of its ends, where order 1 twice clamps on clamped deltas."""
    rng = np.random.default_rng(4)
    W, n = 2, 40
    x = rng.normal(0.0, 3.0, (1, n, 4)).astype(np.float32)
    d2 = mp3g.add_deltas_host(x, [n], 2, W)[0, :, 8:]
    d1 = mp3g.add_deltas_host(x, [n], 1, W)[:, :, 4:]
    twice = mp3g.add_deltas_host(d1, [n], 1, W)[0, :, 4:]
    diff = np.abs(d2 - twice).max(axis=1)
    assert diff[2 * W:n - 2 * W].max() < 1e-5
    assert diff[0] > 1e-2 and diff[n - 1] > 1e-2
    assert (diff[:W] > 1e-3).all() and (diff[n - W:] > 1e-3).all()


@pytest.mark.parametrize("window", [1, 2, 9])
def test_order_1_against_torch_conv1d(window):
    import torch
    rng = np.random.default_rng(window)
    s1 = mp3g.delta_scales(1, window)[1]
    for n in (1, 2, 5, 33, 301):
        x = rng.normal(-4.0, 3.0, (1, n, 6)).astype(np.float32)
        got = mp3g.add_deltas_host(x, [n], 1, window)[0, :, 6:]
        rows = torch.from_numpy(x[0].T.copy())[:, None, :]  # [cols, 1, n]
        padded = torch.nn.functional.pad(rows, (window, window), mode="replicate")
        want = torch.nn.functional.conv1d(padded, torch.from_numpy(s1.copy())[None, None, :])[:, 0, :].numpy().T
        assert (np.abs(got.astype(np.float64) - want) <= spec.conv_bound(x[0], n, window, s1)).all(), n


def test_block_0_is_a_bit_copy_and_a_zero_tap_keeps_inf_out():
    rng = np.random.default_rng(8)
    x = spec.special_values(feats(rng, (2, 2, 9, 5)))
    got = mp3g.add_deltas_host(x, [9, 4], 2, 2)
    assert np.array_equal(bits(got[0, :, :, :5]), bits(x[0]))
    assert np.array_equal(bits(got[1, :, :4, :5]), bits(x[1, :, :4])) and not bits(got[1, :, 4:]).any()
    # an Inf at frame t: the order-1 delta of frame t skips its own (zero) tap
    y = np.ones((1, 7, 1), np.float32)
    y[0, 3, 0] = np.inf
    d = mp3g.add_deltas_host(y, [7], 1, 2)[0, :, 1]
    assert np.isfinite(d[3]) and abs(d[3]) < 1e-6 and np.isinf(d[2]) and np.isinf(d[4])


# ---- frame context -----------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(spec.STACK_SETS))
def test_stack_against_the_index_statement(name):
    """n_out and every word, special values included, for rows of 0, 1, 2, 3, 5, 33,
    301 and F + 9 frames (first >= n and left > n among them) and n_frames_out
    below, equal to and above n_out(F)."""
    left, right, step, first = spec.STACK_SETS[name]
    rng = np.random.default_rng(len(name) + step)
    lengths = [0] + ROW_FRAMES + [310]
    F, cols = 301, 5
    live = feats(rng, (len(lengths), F, cols))
    for row in live:
        spec.special_values(row)
    x = np.zeros((len(lengths), F, 8), np.float32)
    bits(x)[..., :cols] = bits(live)
    full = spec.n_out(F, step, first)
    assert mp3g.stack_frames_count(F, step, first) == full
    for Fo in (None, full - 7, full, full + 5):
        got, m = mp3g.stack_frames_host(x, lengths, left, right, step, first, n_frames_out=Fo, n_cols=cols)
        Fo = full if Fo is None else Fo
        assert got.shape == (len(lengths), Fo, (left + right + 1) * cols) and m.dtype == np.int32
        for r, n in enumerate(lengths):
            want, wm = spec.stack_spec(x[r, :, :cols], n, left, right, step, first, Fo)
            assert m[r] == wm == min(spec.n_out(min(n, F), step, first), Fo)
            assert np.array_equal(bits(got[r]), want), (name, n, Fo)


def test_counts():
    for n in (0, 1, 2, 5, 6, 7, 301, 2 ** 32 - 1):
        for step in (1, 2, 3, 6, 2 ** 31):
            for first in (0, 1, 2, 5, 300, 2 ** 32 - 1):
                assert mp3g.stack_frames_count(n, step, first) == spec.n_out(n, step, first)
    assert mp3g.lfr_options() == dict(left=3, right=3, step=6, first=0)
    assert mp3g.lfr_options(5, 1) == dict(left=2, right=2, step=1, first=0)
    assert mp3g.lfr_options(4, 3) == dict(left=1, right=2, step=3, first=0)


@pytest.mark.parametrize("m,n", [(7, 6), (5, 1), (4, 3)])
def test_lfr_equals_funasr_apply_lfr(m, n):
    rng = np.random.default_rng(m)
    for T in (1, 2, 3, 5, 6, 7, 33, 301):
        x = feats(rng, (1, T, 80))
        got, count = mp3g.stack_frames_host(x, [T], **mp3g.lfr_options(m, n))
        want = spec.apply_lfr(x[0], m, n)
        assert count[0] == len(want) == -(-T // n)
        assert np.array_equal(bits(got[0]), bits(want.astype(np.float32))), T


def test_per_plane_lengths():
    rng = np.random.default_rng(12)
    x = feats(rng, (3, 2, 40, 4))
    per_plane = np.array([[40, 7], [0, 33], [12, 12]])
    d = mp3g.add_deltas_host(x, per_plane, 2, 2)
    s, m = mp3g.stack_frames_host(x, per_plane, 2, 2, 3, 1)
    assert m.tolist() == [[spec.n_out(int(n), 3, 1) for n in row] for row in per_plane]
    for r in range(3):
        for p in range(2):
            n = int(per_plane[r, p])
            alone = mp3g.add_deltas_host(x[r:r + 1, p], [n], 2, 2)
            assert np.array_equal(bits(d[r, p]), bits(alone[0]))
            alone, _ = mp3g.stack_frames_host(x[r:r + 1, p], [n], 2, 2, 3, 1)
            assert np.array_equal(bits(s[r, p]), bits(alone[0]))
    assert not np.array_equal(bits(d[0, 0]), bits(mp3g.add_deltas_host(x[:1, 0], [7], 2, 2)[0]))
    with pytest.raises(ValueError):
        mp3g.add_deltas_host(x, [[1, 2, 3]] * 3)
    with pytest.raises(ValueError):
        mp3g.stack_frames_host(x, [1, 2])


# ---- buffers and arguments ------------------------------------------------------------------

def test_nothing_else_is_written():
    """Sentinel-filled outputs with a guard row on both sides and strides above the
    live widths: only the live words of the rows change."""
    rng = np.random.default_rng(21)
    x = np.full((3, 2, 20, 8), SENTINEL, np.uint32).view(np.float32)
    x[..., :5] = feats(rng, (3, 2, 20, 5))
    lengths = [20, 0, 6]
    for call, width, frames in (
            (lambda o: mp3g.add_deltas_host(x, lengths, 2, 2, n_cols=5, out=o), 15, 20),
            (lambda o: mp3g.stack_frames_host(x, lengths, 1, 2, 3, 1, n_cols=5, out=o)[0], 20, 9)):
        buf = np.full((5, 2, frames, width + 3), SENTINEL, np.uint32)
        got = bits(call(buf[1:4].view(np.float32)))
        assert got.shape == buf[1:4].shape
        assert (got[..., width:] == SENTINEL).all() and (got[..., :width] != SENTINEL).all()
        lib, L = mp3g.lib(), np.asarray(lengths, np.uint32)
        y = buf.copy()
        if frames == 20:
            st = lib.mp3g_add_deltas_host(mp3g._ptr(x), mp3g._ptr(y[1:]), 3, 2, 20, 8, 5, width + 3, mp3g._ptr(L), 1,
                                          2, 2)
        else:
            m = np.zeros((3, 2), np.uint32)
            st = lib.mp3g_stack_frames_host(mp3g._ptr(x), 3, 2, 20, 8, 5, mp3g._ptr(L), 1, 1, 2, 3, 1, mp3g._ptr(y[1:]),
                                            frames, width + 3, mp3g._ptr(m))
        assert st == 0
        assert (y[0] == SENTINEL).all() and (y[4] == SENTINEL).all() and np.array_equal(y[1:4], got)


def test_refusals():
    lib = mp3g.lib()
    x, y = np.zeros(2 * 6 * 8 + 64, np.float32), np.zeros(2 * 6 * 64, np.float32)
    L, m = np.array([6, 3], np.uint32), np.zeros(2, np.uint32)
    px, py, pL, pm = mp3g._ptr(x), mp3g._ptr(y), mp3g._ptr(L), mp3g._ptr(m)
    off = lambda a, words: mp3g.C.c_void_p(a.ctypes.data + 4 * words)  # noqa: E731
    INV, UNS = 1, 8

    def deltas(want, inp=px, out=py, rows=2, planes=1, F=6, stride=8, cols=8, so=24, lengths=pL, lp=1, O=2, W=2):
        assert lib.mp3g_add_deltas_host(inp, out, rows, planes, F, stride, cols, so, lengths, lp, O, W) == want
        if want != 0 or not (rows and planes and F and cols):  # (an accepted call with work would reach the device)
            assert lib.mp3g_add_deltas_rows(0, inp, out, rows, planes, F, stride, cols, so, lengths, lp, O, W,
                                            None) == want
    deltas(0)
    deltas(INV, stride=7)
    deltas(INV, so=23)
    deltas(INV, W=0)
    deltas(INV, lp=2)
    deltas(INV, planes=2, lp=3)
    deltas(INV, out=px)
    deltas(INV, inp=None)
    deltas(INV, out=None)
    deltas(INV, lengths=None)
    deltas(INV, out=off(x, 8))
    deltas(INV, inp=off(x, 8), out=px)
    deltas(UNS, O=5, so=64)
    deltas(UNS, O=2, W=17)
    deltas(UNS, O=4, W=9, so=64)
    deltas(0, O=4, W=8, so=40)
    deltas(0, O=0, W=1000, so=8)
    for zero in ("rows", "planes", "F", "cols"):
        deltas(0, inp=None, out=None, lengths=None, **{zero: 0})
    assert lib.mp3g_add_deltas_rows(-1, px, py, 2, 1, 6, 8, 8, 24, pL, 1, 2, 2, None) == INV

    def stack(want, inp=px, rows=2, planes=1, F=6, stride=8, cols=8, lengths=pL, lp=1, left=1, right=1, step=1, first=0,
              out=py, Fo=6, so=24, lo=pm):
        assert lib.mp3g_stack_frames_host(inp, rows, planes, F, stride, cols, lengths, lp, left, right, step, first,
                                          out, Fo, so, lo) == want
        if want != 0 or not (rows and planes):
            assert lib.mp3g_stack_frames_rows(0, inp, rows, planes, F, stride, cols, lengths, lp, left, right, step,
                                              first, out, Fo, so, lo, None) == want
    stack(0)
    stack(INV, stride=7)
    stack(INV, so=23)
    stack(INV, step=0)
    stack(INV, lp=2)
    stack(INV, out=px)
    stack(INV, inp=None)
    stack(INV, out=None)
    stack(INV, lengths=None)
    stack(INV, lo=None)
    stack(INV, out=off(x, 8))
    stack(UNS, left=65, so=8 * 67, cols=1, stride=1)
    stack(UNS, right=65, so=8 * 67, cols=1, stride=1)
    stack(0, left=64, right=64, cols=1, stride=1, so=129, Fo=2)
    stack(0, inp=None, out=None, lengths=None, lo=None, rows=0)
    stack(0, inp=None, out=None, lengths=None, lo=None, planes=0)
    m[:] = 9
    stack(0, inp=None, out=None, cols=0)  # no word to write: the counts still are
    assert m.tolist() == [6, 3]
    stack(0, inp=None, out=None, Fo=0)
    assert m.tolist() == [0, 0]
    assert lib.mp3g_stack_frames_rows(-1, px, 2, 1, 6, 8, 8, pL, 1, 1, 1, 1, 0, py, 6, 24, pm, None) == INV
    # the Python layer
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.add_deltas_host(np.zeros((1, 4, 3), np.float32), [4], order=5)
    assert e.value.status == UNS
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.stack_frames_host(np.zeros((1, 4, 3), np.float32), [4], step=0, n_frames_out=4)
    assert e.value.status == INV
    with pytest.raises(ValueError):
        mp3g.add_deltas_host(np.zeros((4, 3), np.float32), [4])
    for call in (mp3g.decode_windows_fbank_tensor, mp3g.decode_windows_mfcc_tensor):
        for kw in (dict(deltas=dict(order=2, windows=2)), dict(stack=dict(left=1, stride=2)), dict(deltas=2),
                   dict(stack=[1, 1])):
            with pytest.raises(mp3g.Mp3gError) as e:  # (before any device call)
                call([b""], [0], 8000, **kw)
            assert e.value.status == 1


def test_sanitizer_build_of_the_host_code():
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-framectx"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "framectx_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "framectx_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
