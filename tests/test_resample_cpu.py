"""The resampler's host side (include/mp3g.h "sample-rate conversion of
decoded rows"): the filter table against the formula,
mp3g_resample_host against a float64 dot product, its edges, and the
sanitizer build of the new host code.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_resample as spec
from conftest import REPO


@pytest.mark.parametrize("zeros", (4, 16, 64))
@pytest.mark.parametrize("fi,fo", spec.PAIRS)
def test_table_against_formula(fi, fo, zeros):
    """Every tap is the float64 formula rounded once to float32 (half an ulp,
    2^-24 relative) plus 1e-9 for the float64 evaluations' own differences."""
    rolloff, beta = (spec.FAST if zeros < 64 else spec.BEST)[1:]
    L, M, W, _ = spec.params(fi, fo, zeros, rolloff)
    r = mp3g.Resampler(fi, fo, zeros, rolloff, beta)
    assert (r.L, r.M, r.W) == (L, M, W) and r.tile > 0
    h64 = spec.taps64(fi, fo, zeros, rolloff, beta)
    assert r.taps.shape == h64.shape == (L, 2 * W) and r.taps.dtype == np.float32
    err = np.abs(r.taps.astype(np.float64) - h64)
    bound = 2.0 ** -24 * np.abs(h64) + 1e-9
    print(f"{fi}->{fo} zeros {zeros}: max err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def test_table_sizes_and_presets():
    assert mp3g.RESAMPLE_FAST == spec.FAST and mp3g.RESAMPLE_BEST == spec.BEST
    for (fi, fo, preset), (L, M, W) in {(44100, 16000, spec.FAST): (160, 441, 52),
                                        (44100, 16000, spec.BEST): (160, 441, 187),
                                        (32000, 44100, spec.BEST): (441, 320, 68)}.items():
        r = mp3g.Resampler(fi, fo, *preset)
        assert (r.L, r.M, r.W) == (L, M, W) and r.taps.size == L * 2 * W
    assert mp3g.Resampler(44100, 16000).W == 52  # the default preset is "fast"
    # the DC gain of every phase, with no per-phase normalisation: a property of
    # the formula (float64: 2.04e-5 from 1 at worst for "fast", 48 -> 44.1 kHz;
    # below 2e-8 for "best"), kept by the float32 table to its rounding (2W
    # taps of at most c <= 1, half an ulp each)
    for preset, tol in ((spec.FAST, 2.1e-5), (spec.BEST, 2e-8)):
        for fi, fo in spec.PAIRS:
            r = mp3g.Resampler(fi, fo, *preset)
            dc = spec.taps64(fi, fo, *preset).sum(axis=1)
            assert np.abs(dc - 1.0).max() < tol, (fi, fo)
            assert np.abs(r.taps.astype(np.float64).sum(axis=1) - dc).max() <= 2 * r.W * 2.0 ** -25, (fi, fo)


def test_refusals():
    for args, status in (((44100, 16001), 8),           # L * 2W > 2^18
                         ((44100, 16000, 65), 8), ((44100, 16000, 0), 8),
                         ((0, 16000), 1), ((44100, -5), 1), ((44100, 16000, 16, 0.0), 1),
                         ((44100, 16000, 16, 1.5), 1)):
        with pytest.raises(mp3g.Mp3gError) as e:
            mp3g.Resampler(*args)
        assert e.value.status == status, args
    # the device call refuses a host-only resampler and a bad channel count before any device call
    r = mp3g.Resampler(44100, 16000, 4)
    L = mp3g.lib()
    assert L.mp3g_resample_rows(r._h, None, 8, None, 8, 2, None, 1, None) == 1
    assert L.mp3g_resample_rows(r._h, None, 8, None, 8, 3, None, 1, None) == 1
    assert L.mp3g_resample_rows(None, None, 8, None, 8, 2, None, 1, None) == 1


def signals(W, rng):
    """Uniform noise, an impulse at each of the first and last 2W positions, a constant."""
    N = 6 * W + 37
    yield "noise", rng.uniform(-1.0, 1.0, N).astype(np.float32)
    yield "constant", np.full(N, 0.75, np.float32)
    for p in list(range(2 * W)) + list(range(N - 2 * W, N)):
        x = np.zeros(N, np.float32)
        x[p] = 1.0
        yield f"impulse@{p}", x


@pytest.mark.parametrize("fi,fo,zeros", [(44100, 16000, 16), (32000, 44100, 4), (48000, 16000, 4), (24000, 16000, 4),
                                         (22050, 16000, 4), (48000, 44100, 4), (44100, 16000, 64)])
def test_host_reference_against_float64(fi, fo, zeros):
    """|y32 - sum h32 x| <= gamma sum |h32 x|, gamma = 2W u / (1 - 2W u), u =
    2^-24: the bound of a length-2W FMA chain (one rounding per step).  The
    float64 sum uses the library's own float32 taps."""
    rolloff, beta = (spec.FAST if zeros < 64 else spec.BEST)[1:]
    r = mp3g.Resampler(fi, fo, zeros, rolloff, beta)
    u = 2.0 ** -24
    gamma = 2 * r.W * u / (1 - 2 * r.W * u)
    worst = 0.0
    sigs = list(signals(r.W, np.random.default_rng(fi + zeros)))
    if zeros == 64:  # (the long filter: the noise, the constant and a few impulses)
        sigs = sigs[:2] + sigs[2::97]
    for name, x in sigs:
        n_y = r.out_len(len(x))
        assert n_y == spec.out_len(len(x), r.L, r.M)
        # an impulse touches few outputs: check those around it, everything for the others
        if name.startswith("impulse"):
            p = int(name.split("@")[1])
            lo = max(0, (p - r.W) * r.L // r.M - 2)
            n = min(n_y + 3, (p + r.W) * r.L // r.M + 3) - lo
        else:
            lo, n = 0, n_y + 3
        y = r.host(x, 0, lo, n)
        y64, mag = spec.resample64(r.taps, r.L, r.M, x, 0, lo, n)
        err = np.abs(y.astype(np.float64) - y64)
        # float32 subnormal results round absolutely: half the smallest subnormal
        assert (err <= gamma * mag + 2.0 ** -150).all(), (name, float((err - gamma * mag).max()))
        nz = mag > 0
        if nz.any():
            worst = max(worst, float((err[nz] / (gamma * mag[nz])).max()))
        if name.startswith("impulse"):  # one tap per output: the tap itself
            assert np.array_equal(y.astype(np.float64), y64)
    print(f"{fi}->{fo} zeros {zeros}: worst err / bound = {worst:.4f}")


def test_edges():
    rng = np.random.default_rng(7)
    r = mp3g.Resampler(44100, 16000, 4)
    N = 2000
    x = rng.uniform(-1, 1, N).astype(np.float32)
    n_y = r.out_len(N)
    assert n_y == -(-N * 160 // 441)
    pad = 40
    full = r.host(x, 0, 0, n_y + pad)
    # zero extension: the same outputs from an explicitly padded source (origin -300 is origin 0 of the padded one
    # shifted: a shift by M source samples is a shift by L outputs)
    xp = np.concatenate([np.zeros(r.M, np.float32), x, np.zeros(300, np.float32)])
    assert np.array_equal(r.host(xp, 0, r.L, n_y + pad).view(np.uint32), full.view(np.uint32))
    # windows straddling 0 and N, inside, and past the end
    for s, n in ((0, 5), (1, 64), (r.L - 1, 3), (r.L, 3), (n_y - 10, 30), (n_y, 10), (n_y + 20, 20), (300, 0)):
        w = r.host(x, 0, s, n)
        assert np.array_equal(w.view(np.uint32), full[s:s + n].view(np.uint32)), (s, n)
    assert not full[n_y + r.W * r.L // r.M + 2:].any()
    # a part of the source at its origin = the whole with the rest zeroed
    a, b = r.src_window(200, 100)
    assert a == 200 * r.M // r.L - r.W + 1 and b == 299 * r.M // r.L + r.W + 1
    part = r.host(x[a:b], a, 200, 100)
    assert np.array_equal(part.view(np.uint32), full[200:300].view(np.uint32))
    # ... and a narrower part is the zero-extension of that part
    xz = np.zeros_like(x)
    xz[a + 5:b - 5] = x[a + 5:b - 5]
    assert np.array_equal(r.host(x[a + 5:b - 5], a + 5, 200, 100).view(np.uint32),
                          r.host(xz, 0, 200, 100).view(np.uint32))
    # out_start = 2^33 + 7 with a short source at the matching origin, against the float64 spec
    s = 2 ** 33 + 7
    a, b = r.src_window(s, 50)
    xs = rng.uniform(-1, 1, b - a).astype(np.float32)
    y = r.host(xs, a, s, 50)
    y64, mag = spec.resample64(r.taps, r.L, r.M, xs, a, s, 50)
    gamma = 2 * r.W * 2.0 ** -24 / (1 - 2 * r.W * 2.0 ** -24)
    assert (mag > 0).all() and (np.abs(y - y64) <= gamma * mag).all()
    # the same bits as the same phases near zero: shifting by a multiple of L moves q by a multiple of M
    k = s // r.L
    assert np.array_equal(y.view(np.uint32), r.host(xs, a - k * r.M, s - k * r.L, 50).view(np.uint32))
    # subnormal products are kept
    tiny = (x * np.float32(2.0 ** -120)).astype(np.float32)
    yt = r.host(tiny, 0, 0, n_y)
    y64, mag = spec.resample64(r.taps, r.L, r.M, tiny, 0, 0, n_y)
    assert yt.any() and (np.abs(yt - y64) <= gamma * mag + 2.0 ** -150).all()


def test_equal_rates_are_a_copy():
    r = mp3g.Resampler(16000, 16000)
    assert (r.L, r.M, r.W) == (1, 1, 0) and r.taps.shape == (1, 0)
    x = np.array([-0.0, 1.5, np.float32(2.0 ** -140), -3.0], np.float32)
    y = r.host(x, 2, 0, 8)
    assert np.array_equal(y.view(np.uint32), np.concatenate([[0, 0], x.view(np.uint32), [0, 0]]))
    assert r.src_window(5, 10) == (5, 15) and r.out_len(77) == 77


def test_stream_rates(sample_files):
    from mp3g import synth
    datas = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"], b"", b"\x00" * 500]
    want = [44100, 22050, 0, 0]
    for lsf in (False, True):
        for sfreq, f in enumerate((44100, 48000, 32000)):
            datas.append(synth.encode_stream(5 + sfreq, 3, lsf=lsf, sfreq=sfreq, mode=synth.MODE_MONO if sfreq == 1 else 1))
            want.append(f >> int(lsf))
    rates, nch = mp3g.stream_rates(datas, n_threads=2, channels=True)
    assert rates.tolist() == want
    first = [int(mp3g.parse_stream(d)[0]["header"][0]) for d in datas[:2]]  # the full parse's first frame
    assert nch.tolist() == [1 if (h >> 6) & 3 == 3 else 2 for h in first] + [0, 0, 2, 1, 2, 2, 1, 2]
    assert mp3g.stream_rates([]).tolist() == []


def test_sanitizer_program_runs_clean():
    """The new host code (filter design, mp3g_resample_host, the refusals) under
    ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-resample"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "resample_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "resample_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
