"""The energy VAD's and the voiced-frame selection's host side (include/mp3g.h
"Sliding-window CMN, energy VAD and voiced-frame selection", DESIGN.md section
9j): mp3g_vad_energy_host against the float64 spec on inputs that keep a derived
margin from the threshold, the two float32 ties of the proportion test,
mp3g_select_frames_host against numpy boolean indexing, the refusals, and the
sanitizer build of the new host code.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_frameops as spec
from conftest import REPO

SENTINEL = 0x7FC0DEAD
VOXCELEB = dict(energy_threshold=5.5, energy_mean_scale=0.5, proportion_threshold=0.12, frames_context=2)
KALDI = dict(energy_threshold=5.0, energy_mean_scale=0.5, proportion_threshold=0.6, frames_context=0)
N_GRID = [0, 1, 31, 32, 33, 300]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def energies(rng, shape, col, n_cols):
    """[.., F, n_cols + 1] float32: log-energy-like values in `col`, MFCC-like ones elsewhere."""
    x = rng.normal(0.0, 4.0, shape + (n_cols + 1,)).astype(np.float32)
    x[..., col] = rng.normal(7.0, 3.0, shape).astype(np.float32)
    return x


def margin_ok(x, lengths, thr, mean_scale, col):
    """Whether no live x[t] lies within the derived margin of the spec's
    threshold: 2^-23 |thr| (the float32 rounding of thr, and the spec's own
    float64 roundings, far below it) plus the blocked sum's error (n + 2) 2^-53
    sum|x| carried to thr by mean_scale / n.  Beyond it the float32 comparison
    x > thr has one answer for the host's and the spec's threshold."""
    k = 0
    flat = thr.reshape(-1)
    for xp, n in spec.planes_of(np.asarray(x, np.float64), lengths):
        if n:
            e = xp[:n, col]
            m = 2.0 ** -23 * abs(flat[k]) + abs(mean_scale) * (n + 2) * 2.0 ** -53 * np.abs(e).sum() / n
            if not (np.abs(e - flat[k]) > m).all():
                return False
        k += 1
    return True


def check_vad(x, lengths, opts, col=0, n_cols=None):
    voiced, counts = mp3g.vad_energy_host(x, lengths, col=col, n_cols=n_cols, **opts)
    want, wcounts, thr = spec.vad64(x, lengths, col=col, **opts)
    assert margin_ok(x, lengths, thr, opts["energy_mean_scale"], col)  # the precondition the inputs meet
    assert voiced.dtype == np.uint8 and voiced.shape == x.shape[:-1] and counts.shape == x.shape[:-2]
    assert np.array_equal(voiced, want), np.argwhere(voiced != want)[:4].tolist()
    assert np.array_equal(counts, wcounts) and counts.dtype == np.int32
    return voiced, counts


@pytest.mark.parametrize("opts", [KALDI, VOXCELEB, dict(KALDI, frames_context=2),
                                  dict(VOXCELEB, frames_context=400), dict(VOXCELEB, energy_mean_scale=0.0)],
                         ids=["kaldi", "voxceleb", "context2", "context400", "no_mean"])
def test_vad_host_against_spec(opts):
    """n = 0, 1, 31, 32, 33, 300 (and above F), mono and planar, contexts 0, 2
    and above n; frames past the length are 0."""
    rng = np.random.default_rng(5)
    F = 300
    for shape in ((7, F), (7, 2, F)):
        x = energies(rng, shape, 0, 13)
        lengths = N_GRID + [F + 40]
        voiced, counts = check_vad(x, lengths, opts, n_cols=13)
        for b, n in enumerate(lengths):
            assert not voiced[b, ..., min(n, F):].any()
        assert counts[0].max() == 0 and 0 < counts[5].min() and counts[6].min() <= F  # (not vacuous)
        if opts["energy_mean_scale"] and opts["frames_context"] <= 2:
            assert counts[5].max() < F
    x = energies(rng, (3, 40), 5, 13)
    check_vad(x, [40, 17, 3], opts, col=5)


@pytest.mark.parametrize("context,den,num,t", [(2, 5, 3, 2), (5, 10, 6, 4)])
def test_float32_ties_are_voiced(context, den, num, t):
    """proportion_threshold = 0.6f: (float)den * 0.6f is exactly num (a tie
    rounded to even), so num frames above the threshold of den make frame t
    voiced, which is Kaldi's answer; the float64 product is above num and would
    say unvoiced.  Context 2 in a row's middle, context 5 clipped at its start."""
    p = np.float32(0.6)
    assert np.float32(den) * p == np.float32(num)               # the float32 product: a tie
    assert float(den) * float(p) > float(num)                   # what a double product would compare
    n = 12
    x = np.zeros((1, n, 2), np.float32)
    lo, hi = max(0, t - context), min(n - 1, t + context)
    assert hi - lo + 1 == den
    x[0, lo:lo + num, 0] = 9.0
    opts = dict(energy_threshold=5.0, energy_mean_scale=0.0, proportion_threshold=0.6, frames_context=context)
    voiced, _ = check_vad(x, [n], opts, n_cols=1)
    assert voiced[0, t] == 1
    x[0, lo + num - 1, 0] = 0.0                                 # one fewer: below the proportion
    voiced, _ = check_vad(x, [n], opts, n_cols=1)
    assert voiced[0, t] == 0


def test_vad_reads_only_its_column_and_its_frames():
    """energy_mean_scale = 0 with NaNs in another column and in the frames past the length: the same answer."""
    rng = np.random.default_rng(8)
    x = energies(rng, (2, 50), 0, 3)
    opts = dict(VOXCELEB, energy_mean_scale=0.0)
    a, ca = check_vad(x, [50, 20], opts, n_cols=3)
    y = x.copy()
    y[:, :, 1] = np.nan
    y[1, 20:, :] = np.nan
    b, cb = mp3g.vad_energy_host(y, [50, 20], n_cols=3, **opts)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    b, cb = mp3g.vad_energy_host(y, [50, 20], n_cols=3, **VOXCELEB)  # (the mean too reads nothing else)
    a, ca = mp3g.vad_energy_host(x, [50, 20], n_cols=3, **VOXCELEB)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)


def patterns(shape, rng):
    """uint8 [.., F] flag rows: none, all, alternating, random, then random again."""
    v = (rng.uniform(size=shape) < 0.4).astype(np.uint8)
    v[0] = 0
    v[1] = 1
    v[2, ..., ::2] = 0
    v[2, ..., 1::2] = 7  # (any non-zero byte is voiced)
    return v


@pytest.mark.parametrize("shape", [(5, 41), (5, 2, 41)])
def test_select_host_against_boolean_indexing(shape):
    rng = np.random.default_rng(len(shape))
    F = shape[-1]
    x = rng.normal(0.0, 3.0, shape + (6,)).astype(np.float32)
    x[x == 0] = 1.0
    v = patterns(shape, rng)
    lengths = [F, F, F - 1, 30, F + 5]
    for Fo in (0, 7, 20, F, F + 6):  # (the all-voiced row has F: below, equal and above the count)
        for n_cols, S_out in ((6, 6), (4, 7)):
            buf = np.full(shape[:-1] + (Fo, S_out), SENTINEL, np.uint32).view(np.float32)
            got, m = mp3g.select_frames_host(x, v, lengths, n_cols=n_cols, out=buf)
            want, wm = spec.select(x, v, lengths, Fo, n_cols)
            assert np.array_equal(m, wm) and m.dtype == np.int32
            assert np.array_equal(bits(got[..., :n_cols]), bits(want[..., :n_cols]))  # copies and +0, as bits
            assert (bits(got[..., n_cols:]) == SENTINEL).all()                        # the stride's tail
            assert m[0].max() == 0 and m[1].min() == min(F, Fo) and not got[0, ..., :n_cols].any()
    got, m = mp3g.select_frames_host(x, v, lengths)
    assert got.shape == x.shape and np.array_equal(m, spec.select(x, v, lengths, F)[1])


def test_refusals():
    L = mp3g.lib()
    x = np.zeros((2, 1, 4, 6), np.float32)
    y = np.zeros_like(x)
    n = np.array([4, 4], np.uint32)
    v = np.zeros((2, 1, 4), np.uint8)
    cnt = np.zeros(2, np.uint32)
    px, py, pn, pv, pc = (a.ctypes.data_as(C.c_void_p) for a in (x, y, n, v, cnt))
    vad = L.mp3g_vad_energy_host
    assert vad(px, 2, 1, 4, 6, 6, 5, pn, 5.0, 0.5, 0.6, 0, pv, pc) == 0
    assert vad(px, 2, 1, 4, 6, 6, 6, pn, 5.0, 0.5, 0.6, 0, pv, pc) == 1   # col >= n_cols
    assert vad(px, 2, 1, 4, 6, 7, 0, pn, 5.0, 0.5, 0.6, 0, pv, pc) == 1   # stride < n_cols
    for a in ((None, pn, pv, pc), (px, None, pv, pc), (px, pn, None, pc), (px, pn, pv, None)):
        assert vad(a[0], 2, 1, 4, 6, 6, 0, a[1], 5.0, 0.5, 0.6, 0, a[2], a[3]) == 1
    assert vad(None, 0, 1, 4, 6, 6, 0, None, 5.0, 0.5, 0.6, 0, None, None) == 0
    rows = L.mp3g_vad_energy_rows
    assert rows(0, px, 2, 1, 4, 6, 6, 6, pn, 5.0, 0.5, 0.6, 0, pv, pc, None) == 1
    assert rows(0, None, 2, 1, 4, 6, 6, 0, pn, 5.0, 0.5, 0.6, 0, pv, pc, None) == 1
    assert rows(-1, px, 2, 1, 4, 6, 6, 0, pn, 5.0, 0.5, 0.6, 0, pv, pc, None) == 1
    assert rows(0, None, 0, 1, 4, 6, 6, 0, None, 5.0, 0.5, 0.6, 0, None, None, None) == 0
    sel = L.mp3g_select_frames_host
    assert sel(px, 2, 1, 4, 6, 6, pv, pn, py, 4, 6, pc) == 0
    assert sel(px, 2, 1, 4, 6, 7, pv, pn, py, 4, 7, pc) == 1     # stride < n_cols
    assert sel(px, 2, 1, 4, 6, 6, pv, pn, py, 4, 5, pc) == 1     # stride_out < n_cols
    assert sel(px, 2, 1, 4, 6, 6, pv, pn, px, 4, 6, pc) == 1     # out is in
    for a in ((None, pv, pn, py, pc), (px, None, pn, py, pc), (px, pv, None, py, pc), (px, pv, pn, None, pc),
              (px, pv, pn, py, None)):
        assert sel(a[0], 2, 1, 4, 6, 6, a[1], a[2], a[3], 4, 6, a[4]) == 1
    assert sel(None, 0, 1, 4, 6, 6, None, None, None, 4, 6, None) == 0
    rows = L.mp3g_select_frames_rows
    assert rows(0, px, 2, 1, 4, 6, 6, pv, pn, px, 4, 6, pc, None) == 1
    assert rows(0, px, 2, 1, 4, 6, 6, pv, pn, py, 4, 5, pc, None) == 1
    assert rows(-1, px, 2, 1, 4, 6, 6, pv, pn, py, 4, 6, pc, None) == 1
    assert rows(0, None, 0, 1, 4, 6, 6, None, None, None, 4, 6, None, None) == 0
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.vad_energy_host(x, [4, 4], col=6)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        mp3g.vad_energy_host(x, [4])
    with pytest.raises(ValueError):
        mp3g.select_frames_host(x, v[:, :, :3], [4, 4])


def test_sanitizer_program_runs_clean():
    """The new host code (mp3g_sliding_cmn_host, mp3g_vad_energy_host,
    mp3g_select_frames_host, the refusals) under ASan + UBSan, as a stand-alone
    program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-frameops"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "frameops_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "frameops_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
