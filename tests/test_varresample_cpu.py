"""The variable-ratio resampler's host side (include/mp3g.h "variable-ratio
resampling of decoded rows"): the prototype table against
its formulae, mp3g_varresample_host against the analytic value within a bound
derived from the table step and the float32 roundings, speed perturbation of a
sine, crops, edges, refusals, and the sanitizer build of the new host code.
No GPU."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mp3g
import spec_varresample as spec
from conftest import REPO

U32 = np.uint32


def preset(name):
    return spec.FAST if name == "fast" else spec.BEST


@pytest.mark.parametrize("P", (7, 9))
@pytest.mark.parametrize("zeros", (4, 16, 64))
def test_table_against_formulae(zeros, P):
    """Every F and D is the float64 formula rounded once to float32 (half an
    ulp, 2^-24 relative) plus 1e-9 for the float64 evaluations' own differences."""
    rolloff, beta = (spec.FAST if zeros < 64 else spec.BEST)[1:]
    v = mp3g.VarResampler(zeros, rolloff, beta, precision=P)
    Z, R, _, _ = spec.params(zeros, rolloff, P, 1, 1)
    assert (v.P, v.Z, v.R) == (P, Z, R) and v.tile > 0 and v.stage > 0
    assert v.table.shape == (Z + 1, 2) and v.table.dtype == np.float32
    F, D = spec.table64(zeros, beta, P)
    for name, got, want in (("F", v.table[:, 0], F), ("D", v.table[:, 1], D)):
        err = np.abs(got.astype(np.float64) - want)
        bound = 2.0 ** -24 * np.abs(want) + 1e-9
        print(f"zeros {zeros} P {P} {name}: max err/bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
    assert v.table[0, 0] == 1.0 and not v.table[Z].any()


def test_cutoff_and_window_arithmetic():
    v = mp3g.VarResampler()
    assert (v.P, v.Z, v.R) == (9, 8192, 435)
    assert v.ratio(44100, 16000, 1) == (441, 160) and v.ratio(44100, 16000, (11, 10)) == (4851, 1600)
    assert v.ratio(44100, 16000, Fraction(9, 10)) == (3969, 1600) and v.ratio(16000, 16000, 1.1) == (11, 10)
    assert v.ratio(44100, 16000, 1.037) == (457317, 160000)
    for num, den in ((33, 10), (4851, 1600), (10, 11), (7, 7), (48, 1)):
        Z, R, I, Wr = spec.params(16, 0.85, 9, num, den)
        assert v.step(num, den) == I and (v.half_width(num, den) == Wr or num == den)
        # the quantised cutoff is at most 2^-P below rolloff min(1, den / num)
        assert 0 <= 0.85 * min(1.0, den / num) - I / 512.0 <= 2.0 ** -9
        assert v.out_len(1000, num, den) == spec.out_len(1000, num, den)
    assert v.src_window(200, 100, 33, 10) == (200 * 33 // 10 - v.half_width(33, 10) + 1,
                                              299 * 33 // 10 + v.half_width(33, 10) + 1)
    assert v.src_window(0, 10, 33, 10)[0] == 0 and v.src_window(5, 10, 3, 3) == (5, 15)


def signals(Wr, rng):
    """Uniform noise, a constant, an impulse at each of the first and last 2 Wr positions."""
    N = 6 * Wr + 37
    yield "noise", rng.uniform(-1.0, 1.0, N).astype(np.float32)
    yield "constant", np.full(N, 0.75, np.float32)
    for p in list(range(2 * Wr)) + list(range(N - 2 * Wr, N)):
        x = np.zeros(N, np.float32)
        x[p] = 1.0
        yield f"impulse@{p}", x


@pytest.mark.parametrize("num,den,quality", [(33, 10, "fast"), (4851, 1600, "fast"), (33, 10, "best"),
                                             (4851, 1600, "best"), (3969, 1600, "best"), (10, 11, "fast"),
                                             (10, 11, "best"), (30011, 12345, "fast")])
def test_host_reference_against_analytic_value(num, den, quality):
    """|host - analytic| <= c sum |x_j| (M2 / (8 4^P) + 3 2^-24) + gamma c sum
    |w_j x_j| (spec_varresample.bound): linear interpolation of f at step 2^-P
    -- M2 = max |f''| taken numerically from the analytic f -- the roundings of
    F, D and the weight, and the FMA chain.  Nothing in the bound comes from
    the code under test."""
    zeros, rolloff, beta = preset(quality)
    P = 9
    v = mp3g.VarResampler(zeros, rolloff, beta, precision=P)
    _, _, I, Wr = spec.params(zeros, rolloff, P, num, den)
    assert v.step(num, den) == I
    if num <= den:
        assert I == v.R  # upsampling: c = R / 2^P
    M2 = spec.max_f2(zeros, beta)
    assert abs(M2 - np.pi ** 2 / 3) < 0.2
    worst = worst_noise = 0.0
    for name, x in signals(Wr, np.random.default_rng(num + zeros)):
        n_y = v.out_len(len(x), num, den)
        support = None
        if name.startswith("impulse"):  # an impulse touches few outputs: those around it
            p = int(name.split("@")[1])
            lo = max(0, (p - Wr) * den // num - 2)
            n = min(n_y + 3, (p + Wr) * den // num + 3) - lo
            support = (p, p + 1)
        else:
            lo, n = 0, n_y + 3
        y = v.host(x, 0, lo, n, num, den)
        if support is None:
            want, sx, swx, taps = spec.analytic(x, 0, lo, n, num, den, zeros, rolloff, beta, P)
        else:  # every impulse position, 16 of the outputs it touches: both ends and an even spread between
            pick = np.unique(np.linspace(0, n - 1, 16).astype(int))
            parts = [spec.analytic(x, 0, lo + int(i), 1, num, den, zeros, rolloff, beta, P, support=support)
                     for i in pick]
            want, sx, swx, taps = (np.concatenate([q[j] for q in parts]) for j in range(4))
            y = y[pick]
        err = np.abs(y.astype(np.float64) - want)
        b = spec.bound(sx, swx, taps, I, P, M2) + 2.0 ** -150
        assert (err <= b).all(), (name, float((err / b).max()))
        nz = sx > 0
        worst = max(worst, float((err[nz] / b[nz]).max()))
        if name == "noise":
            worst_noise = float(err.max())
            bound_noise = float(b.max())
        if name == "constant":  # the DC gain in the row's interior
            mid = y[2 * Wr * den // num + 2:n_y - 2 * Wr * den // num - 2] / np.float32(0.75)
            dc = float(np.abs(mid - 1.0).max())
    print(f"{num}/{den} {quality}: worst err / bound = {worst:.4f}; noise: worst err {worst_noise:.3e} "
          f"(bound {bound_noise:.3e}); |DC gain - 1| <= {dc:.2e}")


@pytest.mark.parametrize("speed,f_out", [((11, 10), 1100.0), ((9, 10), 900.0)])
def test_speed_moves_a_sine(speed, f_out):
    rate, N = 16000, 16000
    x = np.sin(2 * np.pi * 1000.0 * np.arange(N) / rate).astype(np.float32)
    v = mp3g.VarResampler()
    num, den = v.ratio(rate, rate, speed)
    n_y = v.out_len(N, num, den)
    assert n_y == -(-N * speed[1] // speed[0])
    y = v.host(x, 0, 0, n_y, num, den)
    spectrum = np.abs(np.fft.rfft(y.astype(np.float64) * np.hanning(n_y)))
    peak = float(np.argmax(spectrum)) * rate / n_y
    assert abs(peak - f_out) <= rate / n_y, peak
    assert abs(float(np.abs(y[200:-200]).max()) - 1.0) < 1e-3


def test_crops_windows_and_origins():
    rng = np.random.default_rng(11)
    v = mp3g.VarResampler(4, 0.85, spec.FAST[2])
    N = 2000
    x = rng.uniform(-1, 1, N).astype(np.float32)
    for num, den in ((4851, 1600), (10, 11), (457317, 160000)):
        Wr = v.half_width(num, den)
        n_y = v.out_len(N, num, den)
        pad = 40
        full = v.host(x, 0, 0, n_y + pad, num, den)
        # a crop starting at s equals the same slice of the full output, over 0 and N, inside and past the end
        for s, n in ((0, 5), (1, 64), ((den - 1) % n_y, 3), (den % n_y, 3), (n_y - 10, 30), (n_y, 10), (n_y + 20, 20),
                     (300, 0)):
            w = v.host(x, 0, s, n, num, den)
            assert np.array_equal(w.view(U32), full[s:s + n].view(U32)), (num, den, s, n)
        assert not full[n_y + Wr * den // num + 2:].any()
        # zero extension: an explicitly padded source at a shifted origin
        xp = np.concatenate([np.zeros(50, np.float32), x, np.zeros(300, np.float32)])
        for s, n in ((0, 80), (n_y - 10, 60)):
            assert np.array_equal(v.host(xp, 0, s, n, num, den).view(U32), v.host(x, 50, s, n, num, den).view(U32))
        # a part of the source at its origin = the whole with the rest zeroed
        a, b = v.src_window(200, 100, num, den)
        assert a == 200 * num // den - Wr + 1 and b == 299 * num // den + Wr + 1
        part = v.host(x[a:b], a, 200, 100, num, den)
        assert np.array_equal(part.view(U32), full[200:300].view(U32))
        xz = np.zeros_like(x)
        xz[a + 5:b - 5] = x[a + 5:b - 5]
        assert np.array_equal(v.host(x[a + 5:b - 5], a + 5, 200, 100, num, den).view(U32),
                              v.host(xz, 0, 200, 100, num, den).view(U32))
        # out_start = 2^33 + 7 with a short source at the matching origin: within the bound of the analytic
        # value, and a crop of a longer window there bit for bit
        s = 2 ** 33 + 7
        a, b = v.src_window(s, 50, num, den)
        xs = rng.uniform(-1, 1, b - a).astype(np.float32)
        y = v.host(xs, a, s, 50, num, den)
        want, sx, swx, taps = spec.analytic(xs, a, s, 50, num, den, 4, 0.85, spec.FAST[2], 9)
        b9 = spec.bound(sx, swx, taps, v.step(num, den), 9, spec.max_f2(4, spec.FAST[2]))
        assert (sx > 0).all() and (np.abs(y - want) <= b9).all()
        a2, b2 = v.src_window(s - 9, 70, num, den)
        x2 = np.zeros(b2 - a2, np.float32)
        x2[a - a2:b - a2] = xs
        assert np.array_equal(v.host(x2, a2, s - 9, 70, num, den)[9:59].view(U32), y.view(U32))
        # subnormal products are kept
        tiny = (x * np.float32(2.0 ** -120)).astype(np.float32)
        yt = v.host(tiny, 0, 0, n_y, num, den)
        want, sx, swx, taps = spec.analytic(tiny, 0, 0, n_y, num, den, 4, 0.85, spec.FAST[2], 9)
        bt = spec.bound(sx, swx, taps, v.step(num, den), 9, spec.max_f2(4, spec.FAST[2]))
        assert yt.any() and (np.abs(yt - want) <= bt + 2.0 ** -149).all()


def test_gain_is_the_last_multiplication():
    """y = (c acc) gain: with c = R / 2^P when upsampling, gain 1 gives c acc,
    and any gain multiplies that float32 once more."""
    v = mp3g.VarResampler()
    x = np.random.default_rng(3).uniform(-1, 1, 700).astype(np.float32)
    for num, den in ((10, 11), (4851, 1600)):
        y1 = v.host(x, 0, 0, 200, num, den)
        for g in (0.5, -0.37, 3.0, 1e-30):
            yg = v.host(x, 0, 0, 200, num, den, gain=g)
            assert np.array_equal(yg.view(U32), (y1 * np.float32(g)).view(U32)), (num, den, g)


def test_equal_num_and_den_are_a_copy():
    v = mp3g.VarResampler()
    x = np.array([-0.0, 1.5, np.float32(2.0 ** -140), -3.0], np.float32)
    for num, den in ((1, 1), (7, 7), (2 ** 31 - 1, 2 ** 31 - 1)):
        y = v.host(x, 2, 0, 8, num, den)
        assert np.array_equal(y.view(U32), np.concatenate([[0, 0], x.view(U32), [0, 0]]))  # -0 stays -0
        y = v.host(x, 2, 0, 8, num, den, gain=2.0)
        assert np.array_equal(y.view(U32), (np.concatenate([[0, 0], x, [0, 0]]).astype(np.float32)
                                            * np.float32(2.0)).view(U32))
    assert v.src_window(5, 10, 7, 7) == (5, 15) and v.out_len(77, 7, 7) == 77 and v.half_width(3, 3) == 0


def test_refusals():
    fz, fb = spec.FAST[1:]
    for args, kw, status in (((0, fz, fb), {}, 8), ((65, fz, fb), {}, 8), ((16, fz, fb), {"precision": 4}, 8),
                             ((16, fz, fb), {"precision": 10}, 8), ((16, 0.0, fb), {}, 1), ((16, 1.5, fb), {}, 1),
                             ((16, float("nan"), fb), {}, 1), ((16, 0.01, fb), {"precision": 5}, 1),  # R == 0
                             ((16, fz, -1.0), {}, 1)):
        with pytest.raises(mp3g.Mp3gError) as e:
            mp3g.VarResampler(*args, **kw)
        assert e.value.status == status, (args, kw)
    assert mp3g.VarResampler(1, 1.0, 0.0, precision=5).R == 32   # the smallest table; rolloff 1 is accepted
    v = mp3g.VarResampler()
    x = np.ones(100, np.float32)
    for num, den in ((0, 1), (1, 0), (2 ** 31, 1), (1, 2 ** 31), (436, 1), (2 ** 31 - 1, 4000000)):  # the last two: I == 0
        with pytest.raises(mp3g.Mp3gError) as e:
            v.host(x, 0, 0, 4, num, den)
        assert e.value.status == 1, (num, den)
    assert v.host(x, 0, 0, 4, 435, 1).shape == (4,)  # I == 1: the narrowest cutoff the table resolves
    for args in ((x, 2 ** 62, 0, 1, 3, 2), (x, 0, 2 ** 62, 1, 3, 2)):
        with pytest.raises(mp3g.Mp3gError) as e:
            v.host(*args)
        assert e.value.status == 1
    with pytest.raises(mp3g.Mp3gError):
        v.ratio(44100, 16000, 0)
    with pytest.raises(mp3g.Mp3gError):
        v.half_width(436, 1)
    # the device call refuses a host-only object and a bad channel count before any device call
    L = mp3g.lib()
    assert L.mp3g_varresample_rows(v._h, None, 8, None, 8, 2, None, 1, None) == 1
    assert L.mp3g_varresample_rows(v._h, None, 8, None, 8, 3, None, 1, None) == 1
    assert L.mp3g_varresample_rows(None, None, 8, None, 8, 2, None, 1, None) == 1
    assert L.mp3g_varresampler_info(None, None, None, None, None, None, None) == 1


def test_sanitizer_program_runs_clean():
    """The new host code (the table, mp3g_varresample_host with the shared
    arithmetic, the refusals) under ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-varresample"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "varresample_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "varresample_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:],
                                                                         r.stderr[-4000:])
