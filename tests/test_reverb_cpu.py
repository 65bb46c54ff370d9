"""The reverberation's host side (include/mp3g.h "Room reverberation and noise at
an SNR"): the object's peaks, early windows and
partitions against the words, mp3g_augment_host's convolution against the
float64 spec within a bound taken from an independent float32 formulation, the
powers and the scale within bounds that follow from it, the paths without a
response and with a delayed unit impulse, and the sanitizer build of the new
host code.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_reverb as spec
from conftest import REPO

U = 2.0 ** -53
NS = [1, 2, 1023, 1024, 1025, 2049, 3100]
LS = [1, 2, 1023, 1024, 1025, 2500]
RATES = [8000, 16000, 44100]
T = max(NS)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bank(rng, L):
    """Five responses of L taps: the peak at 0, in the middle and at L - 1, the
    maximum twice (the first wins), a negative spike larger in magnitude than
    the peak (not chosen).  Decaying noise below 0.3 around them."""
    h = (0.3 * rng.uniform(-1, 1, (5, L)) * np.exp(-np.arange(L) / max(1.0, L / 5))).astype(np.float32)
    want = [0, L // 2, L - 1, L // 3, (2 * L) // 3]
    for i in range(3):
        h[i, want[i]] = 1.0
    h[3, L // 3] = h[3, min(L - 1, L // 3 + 7)] = 1.0
    h[4, (2 * L) // 3] = 1.0
    if L > 1:
        h[4, L // 6] = -2.0
    return h, want


@pytest.fixture(scope="module")
def signal():
    rng = np.random.default_rng(9)
    return (0.25 * rng.standard_normal((len(NS), T))).astype(np.float32)


def bounds(x, h, fs):
    """From the derived bound B of the full timeline's samples
    (spec_reverb.block_error_bounds): the bound of each kept sample
    [n], and the relative bound of signal_power -- what B allows the m samples e
    of the early reverberation, (2 sqrt(sum e^2 sum B^2) + sum B^2) / sum e^2, plus
    (m + 2) 2^-53 for the sums."""
    n = len(x)
    peak, es, ee, _ = spec.rir_info(h, fs)
    B = spec.block_error_bounds(x, h, fs)
    early = np.convolve(np.asarray(x, np.float64), np.asarray(h, np.float64)[es:ee])
    sq, b_sq = float(np.sum(early * early)), float(np.sum(B[np.arange(es, n + ee - 1) // 1024] ** 2))
    return B[np.arange(peak, peak + n) // 1024], (2 * math.sqrt(sq * b_sq) + b_sq) / sq + (len(early) + 2) * U


def test_object_against_the_words():
    rng = np.random.default_rng(3)
    for fs in RATES:
        for L in LS:
            h, want = bank(rng, L)
            rv = mp3g.Reverb(h, None, fs, device=None)
            info = rv.info()
            assert rv.n_rirs == 5 and rv.max_taps == L
            for i in range(5):
                peak, es, ee, P = spec.rir_info(h[i], fs)
                assert peak == want[i], (L, i)
                assert (info["L"][i], info["peak"][i], info["es"][i], info["ee"][i], info["P"][i]) == \
                    (L, peak, es, ee, P), (fs, L, i)
                assert es == max(0, peak - int(0.001 * fs)) and ee == min(L, peak + int(0.05 * fs))
            assert rv.n_spectra == 5 * 2048 * ((L + 1023) // 1024)
            assert np.array_equal(info["offset"], np.arange(5) * 2048 * ((L + 1023) // 1024))
            rv.close()
    # the early window spans one to three partitions and clips at both ends
    spans = set()
    for fs in RATES:
        for h in bank(rng, 2500)[0]:
            peak, es, ee, _ = spec.rir_info(h, fs)
            spans.add((ee - 1) // 1024 - es // 1024 + 1)
    assert spans == {1, 2, 3}
    # rows longer than their responses: the tail is not read as taps
    h = np.zeros((2, 40), np.float32)
    h[0, 3] = h[1, 30] = 1.0
    h[0, 20] = 5.0
    rv = mp3g.Reverb(h, [10, 40], 16000, device=None)
    assert rv.info()["peak"].tolist() == [3, 30] and rv.info()["L"].tolist() == [10, 40]
    rv.close()
    # the twiddles: exp(-2 pi i k / 4096) from float64
    rv = mp3g.Reverb(np.ones(1, np.float32), None, 16000, device=None)
    k = np.arange(4096)
    tw = np.stack([np.cos(2 * np.pi * k / 4096), -np.sin(2 * np.pi * k / 4096)], axis=1)
    assert np.abs(rv.twiddles - tw).max() <= 2.0 ** -24
    assert rv.twiddles[1024].tolist() == [0.0, -1.0] and rv.twiddles[2048].tolist() == [-1.0, 0.0]
    # a unit impulse's spectrum is all ones: G = FFT(1 + i) in every slot
    assert (rv.spectra() == 1.0).all()
    rv.close()


def test_object_refusals():
    h = np.zeros((1, 65537), np.float32)
    for kw in (dict(rir_lengths=[0]), dict(rir_lengths=[65537]), dict(rate=0), dict(rate=-5)):
        with pytest.raises(mp3g.Mp3gError) as e:
            mp3g.Reverb(h, **dict(dict(rir_lengths=[9], rate=16000, device=None), **kw))
        assert e.value.status == 1, kw
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.Reverb(h[:, :8], [9], 16000, device=None)  # more taps than the row
    assert e.value.status == 1
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.Reverb(h[:0], [], 16000, device=None)
    assert e.value.status == 1
    for rate in (400000, 19, 10, 1):  # (below 20 Hz the early window would be empty)
        with pytest.raises(mp3g.Mp3gError) as e:
            mp3g.Reverb(h, [9], rate, device=None)
        assert e.value.status == 8, rate
    rv = mp3g.Reverb(np.array([1.0, 0.5], np.float32), None, 20, device=None)
    assert (rv.info()["es"][0], rv.info()["ee"][0]) == (0, 1)
    x = np.full((2, 1025), 0.25, np.float32)
    out, st = mp3g.augment_host(x, [1, 1025], reverb=rv, rir_index=[0, 0], normalize=False)
    assert abs(out[0, 0] - 0.25) < 1e-6 and abs(out[1, 0] - 0.25) < 1e-6  # every kept sample is written,
    assert np.abs(out[1, 1:] - 0.375).max() < 1e-6                        # the one past the first block too
    rv.close()
    with pytest.raises(ValueError):
        mp3g.Reverb(h, [9, 9], 16000, device=None)
    mp3g.Reverb(h, [65536], 16000, device=None).close()


@pytest.mark.parametrize("fs", RATES)
@pytest.mark.parametrize("L", LS)
def test_convolution_powers_and_scale_against_spec(signal, L, fs):
    """Every n of the grid as a row's length, every response of the bank.  The
    samples within the derived bound B (spec_reverb.block_error_bounds, DESIGN.md
    9k); power_before within (n + 2) 2^-53 (n - 1 additions and a division
    against fsum and a division); the early power within what B allows its m
    samples e, (2 sqrt(sum e^2 sum B^2) + sum B^2) / sum e^2, plus (m + 2) 2^-53;
    power_after within (n + 2) 2^-53 of the exact power of the samples it was
    formed from; the scale and the scaled samples exactly.  The derived bound
    is a worst case, orders above the errors seen, so beside it the rows of
    more than two samples are held to the measured rule: at most four times the
    error of an independent float32 formulation on the same input
    (spec_reverb.overlap_save_f32), at least 2^-23 max|y|.  That rule holds in 621
    of these 630 rows; it is missed by factors of 1.05 to 1.26 in 9, all of n = 2
    (there numpy's transform of two non-zero samples is nearly exact, the floor
    decides, and a 2,048-point float32 transform leaves 2.1 to 3.7 times 2^-24
    max|y| when the maximum is over two samples), where only the derived bound
    is asserted."""
    rng = np.random.default_rng(100 * L + fs)
    h, _ = bank(rng, L)
    rv = mp3g.Reverb(h, None, fs, device=None)
    worst = tight = 0.0
    for i in range(5):
        raw, st0 = mp3g.augment_host(signal, NS, reverb=rv, rir_index=[i] * len(NS), normalize=False)
        out, st = mp3g.augment_host(signal, NS, reverb=rv, rir_index=[i] * len(NS))
        peak, es, ee, _ = spec.rir_info(h[i], fs)
        for r, n in enumerate(NS):
            x = signal[r, :n]
            y, pb, sig = spec.reverberate(x, h[i], fs)
            err = np.abs(raw[r, :n].astype(np.float64) - y)
            bound, rel = bounds(x, h[i], fs)
            assert (err <= bound).all(), (L, fs, i, n, float(err.max()), float(bound.min()))
            tight = max(tight, float((err / bound).max()))
            ref32 = spec.overlap_save_f32(x, h[i])[peak:peak + n]
            floor = 2.0 ** -23 * float(np.abs(y).max())
            allowed = max(4.0 * float(np.abs(ref32 - y).max()), floor)
            worst = max(worst, float(err.max()) / allowed)
            if n > 2:  # (the nine rows that miss this rule all have n = 2: the docstring)
                assert float(err.max()) <= allowed, (L, fs, i, n, float(err.max()), allowed)
            assert (bits(raw[r, n:]) == 0).all() and (bits(out[r, n:]) == 0).all()
            assert abs(st[r, 0] - pb) <= (n + 2) * U * pb
            assert abs(st[r, 1] - sig) <= rel * sig, (L, fs, i, n, st[r, 1], sig, rel)
            assert np.array_equal(st[r, :2], st0[r, :2])
            pa = spec.power(raw[r, :n])
            assert abs(st[r, 2] - pa) <= (n + 2) * U * pa and st0[r, 2] == st[r, 2] and st0[r, 3] == 1.0
            assert st[r, 3] == math.sqrt(st[r, 0] / st[r, 2])
            assert np.array_equal(bits(out[r, :n]), bits((raw[r, :n].astype(np.float64) * st[r, 3]).astype(np.float32)))
    print(f"L = {L}, fs = {fs}: worst error / derived bound = {tight:.2e}; worst error / what the measured rule "
          f"allows (n = 2 included) = {worst:.3f}")
    rv.close()


def test_long_responses_many_partitions():
    """(n, L) = (5000, 3000) and (9000, 16000): 3 and 16 partitions."""
    rng = np.random.default_rng(5)
    for n, L in ((5000, 3000), (9000, 16000)):
        x = (0.25 * rng.standard_normal(n)).astype(np.float32)
        h = (rng.standard_normal(L) * np.exp(-np.arange(L) / (L / 6))).astype(np.float32)
        rv = mp3g.Reverb(h, None, 16000, device=None)
        raw, st = mp3g.augment_host(x[None], None, reverb=rv, rir_index=[0], normalize=False)
        y, pb, sig = spec.reverberate(x, h, 16000)
        peak = spec.rir_info(h, 16000)[0]
        ref32 = spec.overlap_save_f32(x, h)[peak:peak + n]
        err = np.abs(raw[0].astype(np.float64) - y)
        bound, rel = bounds(x, h, 16000)
        assert (err <= bound).all()
        print(f"n = {n}, L = {L}: host {err.max() / np.abs(y).max():.3e}, float32 formulation "
              f"{np.abs(ref32 - y).max() / np.abs(y).max():.3e} of max|y|; worst error / bound {(err / bound).max():.2e}")
        assert abs(st[0, 1] - sig) <= rel * sig
        rv.close()


def test_no_response_is_a_copy(signal):
    """Without a response y = x as bits, signal_power == power_before, and with
    nothing added the scale is 1.0 exactly -- through every way of saying 'none'."""
    x = signal.copy()
    bits(x)[0, 0] = 0x80000000  # -0 survives as bits
    rv = mp3g.Reverb(np.ones(4, np.float32), None, 16000, device=None)
    for kw in (dict(), dict(reverb=rv), dict(reverb=rv, rir_index=[-1] * len(NS)), dict(rir_index=[-7] * len(NS))):
        for normalize in (True, False):
            out, st = mp3g.augment_host(x, NS, normalize=normalize, **kw)
            for r, n in enumerate(NS):
                assert np.array_equal(bits(out[r, :n]), bits(x[r, :n])) and (bits(out[r, n:]) == 0).all()
                assert st[r, 1] == st[r, 0] == st[r, 2] and st[r, 3] == 1.0
                assert abs(st[r, 0] - spec.power(x[r, :n])) <= (n + 2) * U * st[r, 0]
    rv.close()


def test_delayed_unit_impulse_returns_the_signal(signal):
    """h = delta[d]: the peak is d and the shift removes it."""
    for L, d in ((1, 0), (7, 6), (1025, 1024), (2500, 1300)):
        h = np.zeros(L, np.float32)
        h[d] = 1.0
        rv = mp3g.Reverb(h, None, 16000, device=None)
        out, st = mp3g.augment_host(signal, NS, reverb=rv, rir_index=[0] * len(NS), normalize=False)
        for r, n in enumerate(NS):
            x = signal[r, :n].astype(np.float64)
            bound, rel = bounds(signal[r, :n], h, 16000)
            assert (np.abs(out[r, :n] - x) <= bound).all(), (L, d, n)
            m = n + min(L, d + 800) - max(0, d - 16) - 1  # the early window holds the whole response
            assert abs(st[r, 1] * m - st[r, 0] * n) <= (rel + (n + 2) * U) * st[r, 0] * n
        rv.close()


def test_shapes_planes_and_lengths(signal):
    """[B, T] and [B, C, T]; every plane gets the row's response; lengths 0, 1,
    below, at and above T; +0 past the length; stats of an empty row."""
    rng = np.random.default_rng(8)
    h, _ = bank(rng, 1025)
    rv = mp3g.Reverb(h, None, 16000, device=None)
    Tt = 1500
    x = signal[:5, :Tt]
    lengths = [0, 1, Tt - 1, Tt, Tt + 9]
    ri = [0, 1, -1, 3, 4]
    mono, st1 = mp3g.augment_host(x, lengths, reverb=rv, rir_index=ri)
    assert mono.shape == x.shape and st1.shape == (5, 4)
    two = np.stack([x, x[::-1]], axis=1)
    out, st2 = mp3g.augment_host(two, lengths, reverb=rv, rir_index=ri)
    assert out.shape == two.shape and st2.shape == (5, 2, 4)
    assert np.array_equal(bits(out[:, 0]), bits(mono)) and np.array_equal(st2[:, 0], st1)
    assert st1[0].tolist() == [0.0, 0.0, 0.0, 1.0] and (bits(mono[0]) == 0).all()
    assert (bits(mono[1, 1:]) == 0).all() and (bits(mono[2, Tt - 1:]) == 0).all()
    alone, _ = mp3g.augment_host(x[::-1][4:5], [Tt], reverb=rv, rir_index=[4])
    assert np.array_equal(bits(out[4, 1]), bits(alone[0]))  # a plane does not depend on its neighbours
    rv.close()


def test_sanitizer_program_runs_clean():
    """The new host code (the object, mp3g_row_power_host, mp3g_augment_host with
    the shared transforms, the refusals) under ASan + UBSan, as a stand-alone
    program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-reverb"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "reverb_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "reverb_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
