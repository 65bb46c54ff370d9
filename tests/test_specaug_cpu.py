"""SpecAugment's host side (include/mp3g.h "SpecAugment: time warp, frequency and
time masks"): mp3g_specaug_host against the float64 spec --
copies and fills bit for bit, warped words within the bound spec_specaug.py
derives -- the warp against torch's bicubic interpolate, the mean fill, the
descriptor generator's limits, the refusals, the struct's size from C and the
sanitizer build of the new host code.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_specaug as spec
from conftest import REPO

SENTINEL = 0x7FC0DEAD
DT = mp3g.SPECAUG_ROW_DTYPE
WARP_N = [2, 3, 7, 33, 301]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feats(rng, shape):
    """Log-mel-like float32 values with a few -0.0 among them."""
    x = rng.normal(-4.0, 3.0, shape).astype(np.float32)
    x.reshape(-1)[::7] = -0.0
    return x


def padded(x, freq_major, stride):
    """x [B, C, F, nb] laid out as the call reads it, the words past the live count SENTINEL."""
    src = x.transpose(0, 1, 3, 2) if freq_major else x
    buf = np.full(src.shape[:-1] + (stride,), SENTINEL, np.uint32).view(np.float32)
    buf[..., :src.shape[-1]] = src
    return buf


def check(x, lengths, rows, fill=0.0, warp=True, freq_major=False, pad=0, stats=None):
    """mp3g_specaug_host on x [B, C, F, nb] against the spec; returns the output as [B, C, F, nb]."""
    live = x.shape[-2] if freq_major else x.shape[-1]
    buf = padded(x, freq_major, live + pad)
    got = mp3g.spec_augment_host(buf, lengths, rows, fill=fill, freq_major=freq_major, warp=warp, n_cols=live)
    fills = None
    if fill == "mean":
        got, fills = got
        assert fills.shape == x.shape[:2] and fills.dtype == np.float32
    assert got.shape == buf.shape and got.dtype == np.float32
    assert (bits(got[..., live:]) == SENTINEL).all()  # never written
    out = got[..., :live].transpose(0, 1, 3, 2) if freq_major else got[..., :live]
    kind, value, bound = spec.specaug64(x, lengths, rows, fill=fill if fills is None else 0.0, warp=warp, fills=fills)
    same = kind <= spec.COPY
    assert np.array_equal(bits(out)[same], bits(x)[same])
    fl = kind == spec.FILL
    assert np.array_equal(bits(out)[fl], bits(value.astype(np.float32))[fl])
    wp = kind == spec.WARP
    err = np.abs(out.astype(np.float64) - value)[wp]
    if stats is not None and wp.any():
        stats.append(float((err / np.maximum(bound[wp], 1e-300)).max()))
    assert (err <= bound[wp]).all(), float((err / np.maximum(bound[wp], 1e-300)).max())
    return out, fills


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("freq_major", [False, True])
@pytest.mark.parametrize("fill", [0.0, -0.0, 1.5])
def test_masks_against_the_spec(planes, freq_major, fill):
    rng = np.random.default_rng(11)
    F, nb = 40, 13
    lengths = [0, 1, 2, 3, 33, F, F + 9] * 5
    x = feats(rng, (len(lengths), planes, F, nb))
    for shift in (0, 1, 2):
        rows = spec.edge_rows(DT, lengths, F, nb, shift)
        out, _ = check(x, lengths, rows, fill=fill, warp=False, freq_major=freq_major, pad=3)
        assert (out != x).any()
    # a zero fill has the sign it was given
    rows = spec.edge_rows(DT, lengths, F, nb, 0)
    out, _ = check(x, lengths, rows, fill=fill, warp=False, freq_major=freq_major)
    changed = bits(out) != bits(x)
    assert (bits(out)[changed] == bits(np.float32(fill))).all()


def test_in_place_writes_only_the_masked_words():
    rng = np.random.default_rng(12)
    F, nb = 21, 8
    lengths = [F, 9, 0, F + 1]
    x = feats(rng, (4, 2, F, nb))
    rows = spec.edge_rows(DT, lengths, F, nb, 7)
    want, _ = check(x, lengths, rows, fill=2.0, warp=False)
    buf = x.copy()
    lens = np.asarray(lengths, np.uint32)
    desc = np.ascontiguousarray(rows)
    st = mp3g.lib().mp3g_specaug_host(buf.ctypes.data, buf.ctypes.data, 4, 2, F, nb, nb, lens.ctypes.data,
                                      desc.ctypes.data, 0, 2.0, None)
    assert st == 0 and np.array_equal(bits(buf), bits(want))


@pytest.mark.parametrize("n", WARP_N)
def test_warp_against_the_spec(n, record_property):
    rng = np.random.default_rng(n)
    cases = spec.warp_cases(n)
    x = feats(rng, (len(cases), 2, n + 2, 5))
    rows = np.zeros(len(cases), DT)
    for b, (c, w) in enumerate(cases):
        rows[b]["warp_center"], rows[b]["warp_to"] = c % 2 ** 32, w % 2 ** 32
    stats = []
    for fm in (False, True):
        out, _ = check(x, [n] * len(cases), rows, freq_major=fm, pad=1, stats=stats)
        for b, (c, w) in enumerate(cases):
            if not spec.warps(c, w, n):  # no warp, out of range: a copy, -0.0 and all
                assert np.array_equal(bits(out[b]), bits(x[b]))
            elif c == w:  # both segments keep their length: the input's values (-0 may become +0)
                assert np.array_equal(out[b], x[b])
    print("warp n=%d: worst error over bound %.3f" % (n, max(stats) if stats else 0.0))
    record_property("worst_over_bound", max(stats) if stats else 0.0)


@pytest.mark.parametrize("n", WARP_N)
def test_warp_against_torch(n):
    """torch.nn.functional.interpolate(mode="bicubic", align_corners=False) on the
    two segments, as ESPnet's time_warp calls it.  torch forms the source
    coordinate in float32: scale = fl(n_in / n_out), then fl(fl(scale (j + 0.5))
    - 0.5) -- three roundings of values up to n_in, so the coordinate is off by up
    to 3 U n_in.  The interpolant is C1 in the coordinate with |d/ds| <= sum
    |w_k'| max|x| <= (1.35 + 1.35 + 0.75 + 0.75) max|x| = 4.2 max|x|, a floor that
    falls on the other side included.  Add our own bound (<= 57.2 U max|x| from
    the weights, 5 U from the chain: spec_specaug.py) and as much again for
    torch's weights and sums: tol = (12.6 n_in + 125) U max|x|, growing with the
    segment."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(100 + n)
    cases = [cw for cw in spec.warp_cases(n) if spec.warps(*cw, n)]
    x = feats(rng, (len(cases), 1, n, 6))
    rows = np.zeros(len(cases), DT)
    for b, (c, w) in enumerate(cases):
        rows[b]["warp_center"], rows[b]["warp_to"] = c, w
    got = mp3g.spec_augment_host(x, [n] * len(cases), rows)
    worst = 0.0
    for b, (c, w) in enumerate(cases):
        t = torch.from_numpy(x[b][None])  # [1, 1, n, bins]
        for src, dst, lo in ((t[:, :, :c], w, 0), (t[:, :, c:], n - w, w)):
            want = torch.nn.functional.interpolate(src, size=(dst, x.shape[-1]), mode="bicubic",
                                                   align_corners=False)[0, 0].numpy()
            n_in = src.shape[2]
            tol = (12.6 * n_in + 125.0) * spec.U * float(np.abs(src.numpy()).max())
            err = float(np.abs(got[b, 0, lo:lo + dst].astype(np.float64) - want).max())
            worst = max(worst, err / tol)
            assert err <= tol, (n, c, w, err / tol)
    print("torch n=%d: worst difference over tolerance %.3f" % (n, worst))


@pytest.mark.parametrize("freq_major", [False, True])
def test_mean_fill(freq_major):
    rng = np.random.default_rng(13)
    F, nb = 70, 9
    lengths = [0, 1, 31, 32, 33, 64, F, F + 3]
    x = feats(rng, (len(lengths), 2, F, nb)) + np.float32(3.0)
    rows = spec.edge_rows(DT, lengths, F, nb, 4)
    _, fills = check(x, lengths, rows, fill="mean", freq_major=freq_major, pad=2)
    for b, length in enumerate(lengths):
        n = min(length, F)
        for p in range(2):
            mean, sum_abs = spec.mean_fill(x[b, p].astype(np.float64), n)
            if n == 0:
                assert bits(fills[b, p]) == 0  # +0.0
                continue
            # n nb float64 additions, the blocks' and the division: each rounding at most 2^-53 of a partial
            # sum <= sum |x| (the frames' and blocks' additions are far below that: they add few, large terms)
            e = (n * nb + 2) * 2.0 ** -53 * sum_abs / (n * nb)
            assert np.float32(mean - e) <= fills[b, p] <= np.float32(mean + e)


def test_both_layouts_agree_bit_for_bit():
    rng = np.random.default_rng(14)
    F, nb = 45, 12
    lengths = [F, 33, 2, 0, 17]
    x = feats(rng, (5, 2, F, nb))
    rows = spec.edge_rows(DT, lengths, F, nb, 3)
    a, fa = mp3g.spec_augment_host(x, lengths, rows, fill="mean")
    b, fb = mp3g.spec_augment_host(np.ascontiguousarray(x.transpose(0, 1, 3, 2)), lengths, rows, fill="mean",
                                   freq_major=True)
    assert np.array_equal(bits(a), bits(b.transpose(0, 1, 3, 2))) and np.array_equal(bits(fa), bits(fb))
    assert (bits(a) != bits(x)).any()


def test_three_dimensional_input_is_one_plane():
    rng = np.random.default_rng(15)
    x = feats(rng, (3, 20, 6))
    rows = spec.edge_rows(DT, [20, 11, 4], 20, 6, 2)
    a = mp3g.spec_augment_host(x, [20, 11, 4], rows, fill=1.0)
    b = mp3g.spec_augment_host(x[:, None], [20, 11, 4], rows, fill=1.0)
    assert a.shape == x.shape and np.array_equal(bits(a), bits(b[:, 0]))


def test_rows_are_within_their_limits():
    W, fw, tw, nb = 5, 27, 100, 80
    for seed in range(40):
        rng = np.random.default_rng(seed)
        lengths = [0, 1, 2 * W, 2 * W + 1, 11, 50, 300, 3000][seed % 3:]
        ratio = [None, 0.2, 1.0][seed % 3]
        rows = mp3g.spec_augment_rows(rng, lengths, nb, time_warp=W, n_freq_masks=seed % 5, freq_mask_width=fw,
                                      n_time_masks=seed % 17, time_mask_width=tw, time_mask_ratio=ratio)
        assert rows.dtype == DT and rows.shape == (len(lengths),)
        again = mp3g.spec_augment_rows(np.random.default_rng(seed), lengths, nb, time_warp=W, n_freq_masks=seed % 5,
                                       freq_mask_width=fw, n_time_masks=seed % 17, time_mask_width=tw,
                                       time_mask_ratio=ratio)
        assert rows.tobytes() == again.tobytes()  # the same generator state, the same rows
        for r, n in zip(rows, lengths):
            c, w = int(r["warp_center"]), int(r["warp_to"])
            if n - W <= W:
                assert (c, w) == (0, 0)  # no warp
            else:
                assert W <= c < n - W and c - W + 1 <= w <= c + W and spec.warps(c, w, n)
            assert r["n_freq"] == seed % 5 and r["n_time"] == seed % 17
            cap = min(tw, n) if ratio is None else min(tw, n, int(ratio * n))
            for k in range(16):
                s, wd = (int(v) for v in r["time"][k])
                assert (s, wd) == (0, 0) if k >= seed % 17 else (0 <= wd <= cap and 0 <= s <= n - wd)
            for k in range(4):
                s, wd = (int(v) for v in r["freq"][k])
                assert (s, wd) == (0, 0) if k >= seed % 5 else (0 <= wd <= min(fw, nb) and 0 <= s <= nb - wd)
    with pytest.raises(ValueError):
        mp3g.spec_augment_rows(np.random.default_rng(0), [10], nb, n_time_masks=17)
    with pytest.raises(ValueError):
        mp3g.spec_augment_rows(np.random.default_rng(0), [10], nb, n_freq_masks=5)
    # the widths do reach their maxima and the warp both directions
    rows = mp3g.spec_augment_rows(np.random.default_rng(1), [400] * 300, nb, time_warp=W, time_mask_ratio=0.05)
    assert rows["time"][:, :2, 1].max() == 20 and rows["freq"][:, :2, 1].max() == fw
    d = rows["warp_to"].astype(np.int64) - rows["warp_center"]
    assert d.min() == 1 - W and d.max() == W


def _call(inp, out, n_rows, planes, F, nb, stride, lens, desc, flags, fills):
    p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    return mp3g.lib().mp3g_specaug_host(p(inp), p(out), n_rows, planes, F, nb, stride, p(lens), p(desc), flags, 0.0,
                                        p(fills))


def test_refusals():
    INVALID, UNSUPPORTED = 1, 8
    assert mp3g.STATUS[INVALID] == "invalid argument" and mp3g.STATUS[UNSUPPORTED] == "unsupported"
    x = np.zeros((2, 1, 6, 8), np.float32)
    y = np.zeros_like(x)
    lens = np.array([6, 3], np.uint32)
    desc = np.zeros(2, DT)
    fills = np.zeros((2, 1), np.float32)
    W, FM, MEAN = mp3g.SPECAUG_WARP, mp3g.SPECAUG_FREQ_MAJOR, mp3g.SPECAUG_FILL_MEAN
    assert _call(x, y, 2, 1, 6, 8, 8, lens, desc, W, None) == 0
    assert _call(x, y, 2, 1, 6, 8, 8, lens, desc, 8, None) == INVALID  # unknown flag
    assert _call(x, y, 2, 1, 6, 8, 7, lens, desc, 0, None) == INVALID  # stride below the bins
    assert _call(x, y, 2, 1, 9, 6, 8, lens, desc, FM, None) == INVALID  # stride below the frames
    assert _call(x, y, 2, 1, 8, 6, 8, lens, desc, FM, None) == 0
    for missing in range(4):
        args = [x, y, lens, desc]
        args[missing] = None
        assert _call(args[0], args[1], 2, 1, 6, 8, 8, args[2], args[3], 0, None) == INVALID
    assert _call(x, y, 2, 1, 6, 8, 8, lens, desc, MEAN, None) == INVALID  # FILL_MEAN needs its buffer
    assert _call(x, y, 2, 1, 6, 8, 8, lens, desc, MEAN, fills) == 0
    assert _call(x, x, 2, 1, 6, 8, 8, lens, desc, W, None) == INVALID  # the warp is out of place
    assert _call(x, x, 2, 1, 6, 8, 8, lens, desc, 0, None) == 0  # masks only: in place
    flat = np.zeros(2 * 48 + 8, np.float32)
    assert _call(flat[:96], flat[8:], 2, 1, 6, 8, 8, lens, desc, 0, None) == INVALID  # partial overlap
    assert _call(None, None, 1, 1, 2 ** 22 + 1, 1, 1, lens, desc, W, None) == UNSUPPORTED
    assert _call(None, None, 1, 1, 2 ** 22 + 1, 1, 1, lens, desc, 0, None) == INVALID  # (null with work to do)
    for shape in ((0, 1, 6, 8), (2, 0, 6, 8), (2, 1, 0, 8), (2, 1, 6, 0)):  # empty: nothing done
        assert _call(None, None, *shape, 8, None, None, W, None) == 0
    # python: out=feats with the warp, a wrong descriptor count, an unknown fill
    with pytest.raises(ValueError):
        mp3g.spec_augment_host(x, [6, 3], desc[:1])
    with pytest.raises(ValueError):
        mp3g.spec_augment_host(x, [6, 3], desc, fill="median")


def test_struct_size_from_c(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mp3g.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d\\n", sizeof(mp3g_specaug_row), offsetof(mp3g_specaug_row, time),\n'
                   '         offsetof(mp3g_specaug_row, freq), MP3G_SPECAUG_MAX_TIME_MASKS, MP3G_SPECAUG_MAX_FREQ_MASKS);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)], text=True).split()
    assert got == [str(DT.itemsize), str(DT.fields["time"][1]), str(DT.fields["freq"][1]),
                   str(mp3g.SPECAUG_MAX_TIME_MASKS), str(mp3g.SPECAUG_MAX_FREQ_MASKS)]
    assert DT.itemsize == 176
    h = open(os.path.join(REPO, "include", "mp3g.h")).read()
    for name, value in (("FREQ_MAJOR", mp3g.SPECAUG_FREQ_MAJOR), ("WARP", mp3g.SPECAUG_WARP),
                        ("FILL_MEAN", mp3g.SPECAUG_FILL_MEAN)):
        assert "#define MP3G_SPECAUG_%s %du" % (name, value) in h


def test_sanitizer_build_of_the_host_code():
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-specaug"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "specaug_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "specaug_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
