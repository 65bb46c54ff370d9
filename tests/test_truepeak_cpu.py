"""The true peak on the CPU (include/mp3g.h "True peak of decoded rows",
DESIGN.md section 9i): the coefficients against their float64 formula,
mp3g_true_peak_host against the float64 convolution of spec_truepeak.py within
the bound derived there, the exact statements as bits, EBU Tech 3341 style
conformance, the refusals and the sanitizer program."""
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_truepeak as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 4000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the coefficients ------------------------------------------------------------------

def test_coefficients():
    c = mp3g.true_peak_coefs()
    assert c.shape == (3, 12) and c.dtype == np.float32
    ph = spec.phases()
    # phase 0 is the sample itself: one tap, 1, at delay 6
    assert ph[0][0].tolist() == [6] and abs(ph[0][1][0] - 1.0) < 1e-15
    sums = []
    for f in (1, 2, 3):
        delays, want = ph[f]
        assert delays.tolist() == list(range(12))  # exactly 12 taps past 1e-6, delays 0..11
        assert (np.abs(c[f - 1].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-9).all(), f
        sums.append(np.abs(want).sum())
    assert np.abs(np.array(sums) - [1.63118, 1.86418, 1.63118]).max() < 1e-5, sums
    assert np.array_equal(bits(c[0]), bits(c[2][::-1]))  # phases 1 and 3 mirror each other
    assert np.array_equal(bits(c[1]), bits(c[1][::-1]))
    assert mp3g.true_peak_tile() >= 12


def test_generated_table_is_the_generators():
    """truepeak_coefs.inc is what tools/gen_truepeak.py prints."""
    out = subprocess.run(["python3", os.path.join(REPO, "tools", "gen_truepeak.py")], capture_output=True, text=True,
                         check=True).stdout
    with open(os.path.join(REPO, "go-mp3_amd", "csrc", "truepeak_coefs.inc")) as fh:
        assert fh.read() == out


# ---- the host reference against the float64 convolution ---------------------------------

def signal(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        x = 0.3 * rng.standard_normal(n)
    elif kind == "sine997":
        x = 0.25 * np.sin(2 * np.pi * 997.0 * np.arange(n) / 8000.0)
    elif kind == "alternating":  # a burst of +-1 in silence: the interpolator's largest overshoot
        x = np.zeros(n)
        x[n // 3:n // 3 + 40] = np.where(np.arange(40) % 2, -1.0, 1.0)
    elif kind == "impulse":
        x = np.zeros(n)
        x[n // 2] = -0.75
    elif kind == "zeros":
        x = np.zeros(n)
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


KINDS = ("noise", "sine997", "alternating", "impulse", "zeros")
LENGTHS = (0, 1, 11, 12, 13, T)


def test_host_within_derived_bound_of_float64_convolution():
    worst = 0.0
    for planes in (1, 2):
        x = np.stack([np.stack([signal(k, T, 10 * i + p) for p in range(planes)]) for i, k in enumerate(KINDS)])
        ld = mp3g.Loudness(8000)
        for length in LENGTHS:
            got = mp3g.true_peak_host(x, [length] * len(KINDS))
            peak = ld.host(x, [length] * len(KINDS))["peak"]
            for r, kind in enumerate(KINDS):
                want, bound = spec.true_peak(x[r], length), spec.error_bound(x[r], length)
                err = abs(float(got[r]) - want)
                # (the result is one of the chains' float32 values or a sample: the bound holds its roundings)
                assert err <= bound, (kind, planes, length, got[r], want, bound)
                if bound:
                    worst = max(worst, err / bound)
                # exact statements on every row of every case
                assert got[r] >= peak[r], (kind, planes, length)
                assert got[r] <= np.float32(1.8642) * peak[r] * np.float32(1 + 2.0 ** -20), (kind, length, got[r],
                                                                                             peak[r])
                if kind == "zeros" or length == 0:
                    assert bits(got[r]) == 0
        ld.close()
    print(f"worst |host - float64| as a fraction of the derived bound: {worst:.3f}")
    assert worst > 0.0  # (the comparison is not vacuous: some case differs from float64)


def test_alternating_burst_overshoots():
    """The +-1 burst reaches past 1: what a sample peak misses."""
    x = signal("alternating", T, 0)[None]
    tp = mp3g.true_peak_host(x)[0]
    assert 1.0 < tp <= 1.8642 * (1 + 2.0 ** -20) and abs(tp - spec.true_peak(x)) <= spec.error_bound(x)
    assert spec.true_peak(x) > 1.1  # (the burst's edges, in float64: 1.169)


# ---- exact statements, as bits ------------------------------------------------------------

def test_exact_statements():
    # a single impulse at least 12 samples before the end: |a| exactly (every |c| < 1)
    for a, n0, n in ((0.5, 0, 12), (-0.3, 7, 19), (1.0, 100, 200), (np.float32(-1e-30), 3, 40)):
        x = np.zeros((1, 1, n), np.float32)
        x[0, 0, n0] = a
        assert bits(mp3g.true_peak_host(x))[0] == bits(np.abs(np.float32(a))), (a, n0, n)
    # lengths: capped at T, zero handled, and the same as a shorter tensor
    rng = np.random.default_rng(4)
    y = (0.2 * rng.standard_normal((4, 2, 300))).astype(np.float32)
    y[:, :, 290] = 5.0  # (past the lengths of rows 0 and 2)
    got = mp3g.true_peak_host(y, [0, 1000, 150, 300])
    assert bits(got)[0] == 0
    assert bits(got)[1] == bits(mp3g.true_peak_host(y[1:2]))[0] and got[1] >= 5.0
    assert bits(got)[3] == bits(mp3g.true_peak_host(y[3:4]))[0] and got[3] >= 5.0
    assert bits(got)[2] == bits(mp3g.true_peak_host(y[2:3, :, :150]))[0] and got[2] < 5.0
    # a plane's first outputs use zeros before it, not the plane or row that precedes it in memory
    z = np.zeros((2, 2, 64), np.float32)
    z[0] = 1e30
    z[1, 0, :] = 0.0
    z[1, 1, 5] = 0.25
    assert bits(mp3g.true_peak_host(z))[1] == bits(np.float32(0.25))
    # no tail flush: an impulse in the last sample contributes its own 12 outputs' first only
    w = np.zeros((1, 1, 50), np.float32)
    w[0, 0, 49] = 1.0
    c = mp3g.true_peak_coefs()
    assert mp3g.true_peak_host(w)[0] == 1.0 and np.abs(c[:, 0]).max() < 1.0
    # [B, T] is one plane
    assert np.array_equal(bits(mp3g.true_peak_host(y[:, 0])), bits(mp3g.true_peak_host(y[:, :1])))
    # the maximum over planes
    both = mp3g.true_peak_host(y)
    each = np.maximum(mp3g.true_peak_host(y[:, 0]), mp3g.true_peak_host(y[:, 1]))
    assert np.array_equal(bits(both), bits(each))


# ---- conformance, in the style of EBU Tech 3341 cases 15 to 19 ----------------------------------

@pytest.mark.parametrize("divisor,phase_deg,amp", [(4, 0.0, 0.5), (4, 45.0, 0.5), (6, 60.0, 0.5), (8, 67.5, 0.5),
                                                   (4, 45.0, 1.41)])
def test_conformance(divisor, phase_deg, amp):
    """A sine at fs / divisor, 48 kHz, with a 10 ms raised-cosine fade at both
    ends: 20 log10(amp) dBTP within Tech 3341's +0.2 / -0.4 dB."""
    n = 9600  # 0.2 s at 48 kHz
    t = np.arange(n)
    x = amp * np.sin(2 * np.pi * t / divisor + np.deg2rad(phase_deg))
    fade = 480  # 10 ms
    ramp = 0.5 * (1.0 - np.cos(np.pi * (np.arange(fade) + 0.5) / fade))
    x[:fade] *= ramp
    x[-fade:] *= ramp[::-1]
    x = x.astype(np.float32)
    dbtp = 20.0 * np.log10(float(mp3g.true_peak_host(np.stack([x, x])[None])[0]))
    want = 20.0 * np.log10(amp)
    print(f"fs/{divisor} {phase_deg} deg {amp}: {dbtp:.3f} dBTP (expected {want:.3f})")
    assert -0.4 <= dbtp - want <= 0.2, (dbtp, want)
    assert abs(dbtp - 20.0 * np.log10(spec.true_peak(x))) < 1e-5


# ---- refusals: *tp untouched --------------------------------------------------------------------

def test_refusals():
    L, p = mp3g.lib(), mp3g._ptr
    x = np.zeros(8, np.float32)
    tp = np.full(1, 7.0, np.float32)
    assert L.mp3g_true_peak_coefs(None) == 1
    assert L.mp3g_true_peak_host(p(x), 1, 3, 2, None, p(tp)) == 1
    assert L.mp3g_true_peak_host(p(x), 1, 0, 8, None, p(tp)) == 1
    assert L.mp3g_true_peak_host(None, 1, 1, 8, None, p(tp)) == 1
    assert L.mp3g_true_peak_host(p(x), 1, 1, 8, None, None) == 1
    assert L.mp3g_true_peak_host(p(x), 1, 1, 1 << 31, None, p(tp)) == 8
    assert L.mp3g_true_peak_host(None, 0, 1, 8, None, None) == 0
    assert tp[0] == 7.0
    assert L.mp3g_true_peak_host(None, 1, 1, 0, None, p(tp)) == 0 and bits(tp)[0] == 0  # (no sample: +0)
    tile = mp3g.true_peak_tile()
    assert L.mp3g_true_peak_scratch_bytes(1, 3, 8) == 0
    assert L.mp3g_true_peak_scratch_bytes(3, 2, tile + 1) in (0, 3 * 2 * 2 * 4)
    # the device call refuses bad arguments before any device call
    tp[0] = 7.0
    assert L.mp3g_true_peak_rows(-1, p(x), 1, 1, 8, None, None, 0, p(x), p(tp), None) == 1
    assert L.mp3g_true_peak_rows(0, p(x), 1, 3, 2, None, None, 0, p(x), p(tp), None) == 1
    assert L.mp3g_true_peak_rows(0, p(x), 1, 1, 8, None, p(x), 2, p(x), p(tp), None) == 1  # (more indices than rows)
    assert L.mp3g_true_peak_rows(0, p(x), 1, 1, 8, None, None, 0, p(x), None, None) == 1
    assert L.mp3g_true_peak_rows(0, None, 0, 1, 8, None, None, 0, None, None, None) == 0
    assert tp[0] == 7.0
    with pytest.raises(ValueError):
        mp3g.true_peak_host(np.zeros(8, np.float32))
    with pytest.raises(ValueError):
        mp3g.true_peak_host(np.zeros((2, 8), np.float32), [1])
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.true_peak_host(np.zeros((1, 3, 8), np.float32))
    assert e.value.status == 1


def test_sanitizer_program_runs_clean():
    """The new host code (mp3g_true_peak_host, mp3g_loudness_range_host,
    mp3g_gain_host_peak, the refusals) under ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-truepeak"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "truepeak_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "truepeak_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
