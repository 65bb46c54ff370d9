"""The log-mel features' host side (include/mp3g.h "log-mel features of decoded
rows"): the float64 spec against torch.stft, the tables
against the formulas, mp3g_log10f against float64 log10, mp3g_logmel_host
against a derived error bound, its edges and refusals, and the sanitizer build
of the new host code.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_logmel as spec
from conftest import REPO

U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_symbols_and_abi():
    L = mp3g.lib()
    for fn in ("create", "free", "info", "frames", "host", "execute", "log10f"):
        assert hasattr(L, "mp3g_logmel_" + fn)
    assert L.mp3g_abi_version() == 5
    assert (mp3g.LOGMEL_CENTER, mp3g.LOGMEL_CLAMP) == (1, 2)


@pytest.mark.parametrize("n_fft,hop", [(400, 160), (16, 4), (1024, 256)])
def test_spec_against_torch_stft(n_fft, hop):
    """The spec's framing, reflection and window are torch.stft(center=True,
    pad_mode="reflect", window=hann_window(periodic)) in float64: the powers
    agree within 1e-9 max(p) (a cap that catches a convention error; two float64
    sums differ by about 1e-13)."""
    import torch
    x = np.random.default_rng(n_fft).uniform(-1.0, 1.0, 5 * n_fft + 37)
    st = torch.stft(torch.from_numpy(x), n_fft, hop, window=torch.hann_window(n_fft, periodic=True, dtype=torch.float64),
                    center=True, pad_mode="reflect", return_complex=True)
    p_t = (st.real ** 2 + st.imag ** 2).numpy().T  # [F, K]
    p = spec.power64(x, n_fft, hop)
    assert p.shape == p_t.shape == (spec.n_frames(len(x), n_fft, hop), n_fft // 2 + 1)
    err = np.abs(p - p_t).max()
    print(f"n_fft {n_fft}: max |dp| / max p = {err / p.max():.3g}")
    assert err <= 1e-9 * p.max()
    # the folded tables state the same transform
    cw, sw = spec.dft_tables64(n_fft)
    fr = spec.frames64(x, n_fft, hop)
    assert np.abs((fr @ cw.T) ** 2 + (fr @ sw.T) ** 2 - p).max() <= 1e-9 * p.max()


@pytest.mark.parametrize("n_fft,hop,n_mels,rate", spec.CONFIGS)
def test_tables_against_formulas(n_fft, hop, n_mels, rate):
    """Every table entry is the float64 formula rounded once to float32 (2^-24
    relative) plus 1e-9 for the float64 evaluations' own differences."""
    lm = mp3g.LogMel(rate, n_fft, hop, n_mels)
    K = n_fft // 2 + 1
    assert lm.K == K and lm.tile_frames in (8, 16, 32)
    assert lm.cw.shape == lm.sw.shape == (K, n_fft) and lm.wm.shape == (n_mels, K) and lm.cw.dtype == np.float32
    cw, sw = spec.dft_tables64(n_fft)
    wm = spec.mel_filters64(rate, n_fft, n_mels)
    for name, got, want in (("Cw", lm.cw, cw), ("Sw", lm.sw, sw), ("Wm", lm.wm, wm)):
        err = np.abs(got.astype(np.float64) - want)
        bound = U * np.abs(want) + 1e-9
        print(f"{name} ({n_fft}, {n_mels}): max err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), name
    assert (lm.wm >= 0).all()
    centres = []
    for m in range(n_mels):
        lo, hi = (int(v) for v in lm.support[m])
        nz = np.flatnonzero(lm.wm[m])
        if len(nz) == 0:
            assert lo > hi
            continue
        assert (lo, hi) == (nz[0], nz[-1]) and len(nz) == hi - lo + 1  # contiguous
        centres.append(float((nz * lm.wm[m, nz]).sum() / lm.wm[m, nz].sum()))
    # (128 bands at 16 kHz are narrower than a bin at the low end: neighbours may hold the same single bin)
    assert all(a <= b for a, b in zip(centres, centres[1:])) and centres[0] < centres[-1]
    if n_fft == 400:
        assert len(centres) == n_mels  # no filter is empty
    lm.close()


def test_mel_filters_with_a_band():
    lm = mp3g.LogMel(16000, 400, 160, 40, fmin=80.0, fmax=7600.0)
    wm = spec.mel_filters64(16000, 400, 40, 80.0, 7600.0)
    assert (np.abs(lm.wm - wm) <= U * np.abs(wm) + 1e-9).all()
    assert not lm.wm[:, 0].any() and not lm.wm[:, 191:].any()


def test_log10f_against_float64():
    """|mp3g_log10f(x) - log10(x)| <= 2^-20 over all 2^23 mantissas of the binade
    [1, 2) and, for every exponent of [1e-10, 2^60], 4,097 mantissas evenly
    spread (the first and the last among them).

    Run over EVERY float32 of [1e-10, 2^60) instead (7.8e8 values, not part of
    the suite: a minute), the maximum is 0.50000003 * 2^-20 where |y| < 16 and
    2^-20 (1 + 7.5e-9) overall: from y >= 16 the bound is half an ulp and one
    input, 0x5D610FE9 (1.0135898e18, 3.7e-9 ulp from a tie), is rounded the
    other way, 7.1e-15 over the bound.  That input is asserted below as it is."""
    worst = 0.0
    mant = np.arange(1 << 23, dtype=np.uint32)
    x = (mant + np.uint32(127 << 23)).view(np.float32)
    err = np.abs(mp3g.log10f(x).astype(np.float64) - np.log10(x.astype(np.float64)))
    print(f"binade [1, 2): max |err| = {err.max():.4g} = {err.max() * 2 ** 20:.6f} * 2^-20")
    assert err.max() <= 2.0 ** -20
    some = np.concatenate([mant[::2048], mant[-1:]])
    lo = np.float32(1e-10)
    for e in range(-34, 60):
        x = (some + np.uint32((127 + e) << 23)).view(np.float32)
        x = x[x >= lo]
        assert len(x)
        err = np.abs(mp3g.log10f(x).astype(np.float64) - np.log10(x.astype(np.float64)))
        worst = max(worst, float(err.max()))
        assert err.max() <= 2.0 ** -20, (e, float(err.max()) * 2 ** 20)
    x = np.array([1e-10, 2.0 ** 60, 1.0, 10.0, 1e10], np.float32)
    assert mp3g.log10f(x).tolist() == [-10.0, float(np.float32(60 * np.log10(2.0))), 0.0, 1.0, 10.0]
    print(f"every exponent: max |err| = {worst * 2 ** 20:.6f} * 2^-20")
    # the one known float32 of the domain beyond the bound: by 7.1e-15, no more
    x = np.array([0x5D610FE9], np.uint32).view(np.float32)
    err = abs(float(mp3g.log10f(x)[0]) - float(np.log10(x.astype(np.float64))[0]))
    print(f"0x5D610FE9: |err| - 2^-20 = {err - 2.0 ** -20:.3g}")
    assert err <= 2.0 ** -20 + 1e-14


def gamma(n):
    return n * U / (1.0 - n * U)


def mel_bounds(lm, x, F):
    """(mel64, dmel, spread) [n_mels, F] in float64 from the library's own float32
    tables: |re32 - re| <= gamma S and |im32 - im| <= gamma T with gamma of an
    (n_fft)-step FMA chain, S = sum |Cw x|, T = sum |Sw x|; hence |dp| <= 3 gamma
    (S^2 + T^2) (2 gamma from the two squares' first-order terms, the rest covers
    gamma^2 and the two roundings of fmaf(re, re, im * im)); and |dmel| <= sum Wm
    |dp| + gamma_m sum Wm (p + |dp|), gamma_m of a chain as long as the support.
    spread = sum Wm (S^2 + T^2)."""
    fr = spec.frames64(x, lm.n_fft, lm.hop, lm.center, F)
    cw, sw, wm = (t.astype(np.float64) for t in (lm.cw, lm.sw, lm.wm))
    p = (fr @ cw.T) ** 2 + (fr @ sw.T) ** 2
    s2 = (np.abs(fr) @ np.abs(cw).T) ** 2 + (np.abs(fr) @ np.abs(sw).T) ** 2
    dp = 3.0 * gamma(lm.n_fft + 1) * s2
    length = np.maximum(0, lm.support[:, 1].astype(np.int64) - lm.support[:, 0].astype(np.int64) + 1)
    gm = gamma(length.astype(np.float64) + 1.0)[:, None]
    return (p @ wm.T).T, (dp @ wm.T).T + gm * ((p + dp) @ wm.T).T, (s2 @ wm.T).T


@pytest.mark.parametrize("n_fft,hop,n_mels,rate", spec.CONFIGS)
def test_host_reference_against_float64(n_fft, hop, n_mels, rate):
    """Where mel >= 1e-6: |y32 - log10 mel| <= 2^-20 + dmel / (mel ln 10), the
    derived bound of mel_bounds (nothing measured).  Against the independent
    spec the tables' own roundings add 4 u sum Wm (S^2 + T^2) to dmel."""
    lm = mp3g.LogMel(rate, n_fft, hop, n_mels, clamp=False)
    lmc = mp3g.LogMel(rate, n_fft, hop, n_mels, clamp=True)
    T = 3 * n_fft + 37
    F = lm.frames(T)
    assert F == spec.n_frames(T, n_fft, hop) == T // hop + 1
    worst, checked = 0.0, 0
    for name, x in spec.signals(T, np.random.default_rng(n_fft + n_mels)):
        y = lm.host(x)
        assert y.shape == (n_mels, F) and y.dtype == np.float32
        if name in ("zeros", "tiny"):  # the floor everywhere
            assert (y == np.float32(-10.0)).all(), name
            assert (lmc.host(x) == np.float32(-1.5)).all(), name
            continue
        mel, dmel, spread = mel_bounds(lm, x, F)
        ok = mel >= 1e-6
        assert ok.any(), name
        err = np.abs(y.astype(np.float64) - np.log10(np.maximum(mel, spec.FLOOR)))
        bound = 2.0 ** -20 + dmel / (np.maximum(mel, 1e-6) * np.log(10.0))
        assert (err[ok] <= bound[ok]).all(), (name, float((err[ok] / bound[ok]).max()))
        worst = max(worst, float((err[ok] / bound[ok]).max()))
        checked += int(ok.sum())
        y64 = spec.logmel64(x, rate, n_fft, hop, n_mels)
        err = np.abs(y.astype(np.float64) - y64)
        bound = 2.0 ** -20 + (dmel + 4 * U * spread) / (np.maximum(mel, 1e-6) * np.log(10.0))
        assert (err[ok] <= bound[ok]).all(), (name, "spec", float((err[ok] / bound[ok]).max()))
        # Whisper's clamp is the spec's formula on the unclamped features, in float32
        assert np.array_equal(bits(lmc.host(x)), bits(spec.clamp(y))), name
    print(f"({n_fft}, {hop}, {n_mels}): {checked} features, worst err / bound = {worst:.4f}")
    assert checked > 100
    lm.close()
    lmc.close()


def test_edges():
    rng = np.random.default_rng(5)
    for center in (True, False):
        lm = mp3g.LogMel(16000, 400, 160, 80, center=center, clamp=False)
        pad = 200 if center else 0
        assert lm.pad == pad
        # the shortest row with a frame, and one sample less
        T0 = pad + 1 if center else 400
        assert lm.frames(T0 - 1) == 0 and lm.frames(T0) == spec.n_frames(T0, 400, 160, center) >= 1
        x = rng.uniform(-1, 1, T0).astype(np.float32)
        y = lm.host(x)
        y64 = spec.logmel64(x, 16000, 400, 160, 80, center=center)
        assert y.shape == y64.shape and np.abs(y - y64).max() < 1e-3
        with pytest.raises(mp3g.Mp3gError) as e:
            lm.host(x[:-1], 1)
        assert e.value.status == 1
        # n_frames = 1 and the maximum; a wider stride writes nothing else
        T = 1637
        x = rng.uniform(-1, 1, T).astype(np.float32)
        F = lm.frames(T)
        assert F == spec.n_frames(T, 400, 160, center)
        full = lm.host(x)
        assert np.array_equal(bits(lm.host(x, 1)), bits(full[:, :1]))
        wide = lm.host(x, F - 2, F + 5)
        assert np.array_equal(bits(wide[:, :F - 2]), bits(full[:, :F - 2])) and not wide[:, F - 2:].any()
        # a frame depends on its own samples only: the signal cut after frame 1's last sample
        if not center:
            assert np.array_equal(bits(lm.host(x[:560])), bits(full[:, :2]))
        for bad in ((F + 1, F + 1), (2, 1)):
            with pytest.raises(mp3g.Mp3gError) as e:
                lm.host(x, *bad)
            assert e.value.status == 1
        assert lm.host(x, 0).shape == (80, 0)
        # the clamp's maximum is over the frames asked for
        lmc = mp3g.LogMel(16000, 400, 160, 80, center=center, clamp=True)
        for n in (1, 3, F):
            assert np.array_equal(bits(lmc.host(x, n)), bits(spec.clamp(full[:, :n])))
        lm.close()
        lmc.close()


def test_refusals():
    for args, status in (((0,), 1), ((16000, 0), 1), ((16000, -4), 1), ((16000, 400, 0), 1), ((16000, 400, 401), 1),
                         ((16000, 400, 160, 0), 1), ((16000, 400, 160, 80, -1.0), 1),
                         ((16000, 400, 160, 80, 0.0, 8001.0), 1), ((16000, 400, 160, 80, 5000.0, 5000.0), 1),
                         ((16000, 400, 160, 80, float("nan")), 1),
                         ((16000, 12, 4, 4), 8), ((16000, 402), 8), ((16000, 1028), 8), ((16000, 2048, 512), 8),
                         ((16000, 400, 160, 129), 8)):
        with pytest.raises(mp3g.Mp3gError) as e:
            mp3g.LogMel(*args)
        assert e.value.status == status, args
    L = mp3g.lib()
    h = C.c_void_p(1)  # a failed create leaves NULL
    assert L.mp3g_logmel_create(-1, 16000, 400, 160, 80, 0.0, 0.0, 4, C.byref(h)) == 1 and h.value is None
    h = C.c_void_p(1)
    assert L.mp3g_logmel_create(-1, 16000, 1028, 160, 80, 0.0, 0.0, 3, C.byref(h)) == 8 and h.value is None
    # the device call refuses a host-only object and a bad plane count before any device call
    lm = mp3g.LogMel()
    assert L.mp3g_logmel_execute(lm._h, None, 1, 1, 8000, None, 10, 10, None) == 1
    assert L.mp3g_logmel_execute(lm._h, None, 1, 3, 8000, None, 10, 10, None) == 1
    assert L.mp3g_logmel_execute(None, None, 1, 1, 8000, None, 10, 10, None) == 1
    assert L.mp3g_logmel_frames(None, 8000) == 0


def test_sanitizer_program_runs_clean():
    """The new host code (table design, mp3g_logmel_host, mp3g_log10f, the
    refusals) under ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-logmel"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "logmel_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "logmel_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
