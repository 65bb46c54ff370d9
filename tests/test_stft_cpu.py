"""The STFT features' host side (include/mp3g.h "STFT and mel spectrograms of
decoded rows"): the float64 spec against torch.stft, the
tables against the formulas, mp3g_stft_host against a derived error bound, its
shapes and refusals, the cross-check against LogMel at n_fft = 1024 and the
sanitizer build of the new host code.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_logmel
import spec_stft as spec
from conftest import REPO

U = spec.U
RATE = 44100


def bits(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.float32) if a.dtype == np.complex64 else a).view(np.uint32)


def test_symbols_and_abi():
    L = mp3g.lib()
    for fn in ("create", "free", "info", "frames", "host", "execute"):
        assert hasattr(L, "mp3g_stft_" + fn)
    assert L.mp3g_abi_version() == 5
    assert (mp3g.STFT_CENTER, mp3g.STFT_MEL_HTK, mp3g.STFT_MEL_NORM) == (1, 2, 4)
    assert mp3g.STFT_OUTPUTS == {"complex": 0, "power": 1, "magnitude": 2}
    assert mp3g.STFT_LOGS == {None: 0, "ln": 1, "log10": 2}


@pytest.mark.parametrize("n_fft,hop,win,center", [(256, 64, 256, True), (512, 441, 512, False), (1024, 256, 800, True),
                                                  (256, 100, 255, False), (2048, 512, 1, True)])
def test_spec_against_torch_stft(n_fft, hop, win, center):
    """The spec's framing, reflection, window placement and sign are torch.stft's
    in float64, to 1e-9 of the largest bin (a cap that catches a convention
    error; two float64 transforms differ by about 1e-13)."""
    import torch
    x = np.random.default_rng(n_fft + win).uniform(-1.0, 1.0, 3 * n_fft + 37)
    window = torch.hann_window(win, periodic=True, dtype=torch.float64)
    want = torch.stft(torch.from_numpy(x), n_fft, hop, win_length=win, window=window, center=center,
                      pad_mode="reflect", return_complex=True).numpy()
    got = spec.stft64(x, n_fft, hop, win, center, slow=True)
    assert got.shape == want.shape == (n_fft // 2 + 1, spec.n_frames(len(x), n_fft, hop, center))
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"({n_fft}, {hop}, {win}, {center}): max |dX| / max |X| = {err:.3g}")
    assert err <= 1e-9
    assert np.array_equal(got, spec.stft64(x, n_fft, hop, win, center))  # the array-indexed framing is the same


@pytest.mark.parametrize("n_fft", spec.SIZES)
def test_tables_against_formulas(n_fft):
    """Every entry of the window, the twiddles and Wm is the float64 formula
    rounded once (2^-24 relative) plus 1e-9 for the float64 evaluations' own
    differences; supports are contiguous; no bin lies in more than two filters."""
    for win in (n_fft, n_fft - 37, 1):
        st = mp3g.STFT(RATE, n_fft, n_fft // 4, win_length=win)
        assert st.K == n_fft // 2 + 1 and st.tile_frames in (8, 16) and st.wm is None and st.support is None
        for name, got, want in (("window", st.window, spec.window64(n_fft, win)),
                                ("twiddles", st.twiddles, spec.twiddles64(n_fft))):
            assert got.dtype == np.float32 and got.shape == want.shape
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= U * np.abs(want) + 1e-9).all(), name
        q = n_fft // 4
        assert st.twiddles[::q].tolist() == [[1, 0], [0, -1], [-1, 0], [0, 1]]
        st.close()
    for n_mels, htk, norm, fmin, fmax in ((80, False, True, 0.0, 0.0), (128, True, False, 0.0, 0.0),
                                          (128, False, False, 0.0, 0.0), (40, True, True, 80.0, 7600.0)):
        st = mp3g.STFT(RATE, n_fft, n_fft // 4, n_mels=n_mels, htk=htk, norm=norm, fmin=fmin, fmax=fmax)
        wm = spec.mel_filters64(RATE, n_fft, n_mels, fmin, fmax, htk, norm)
        assert st.wm.shape == wm.shape == (n_mels, st.K)
        err = np.abs(st.wm.astype(np.float64) - wm)
        bound = U * np.abs(wm) + 1e-9
        print(f"Wm ({n_fft}, {n_mels}, htk={htk}, norm={norm}): max err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all() and (st.wm >= 0).all()
        for m in range(n_mels):
            lo, hi = (int(v) for v in st.support[m])
            nz = np.flatnonzero(st.wm[m])
            if len(nz) == 0:
                assert lo > hi
            else:
                assert (lo, hi) == (nz[0], nz[-1]) and len(nz) == hi - lo + 1  # contiguous
        assert ((st.wm != 0).sum(axis=0) <= 2).all()
        if n_fft >= 2048 and n_mels == 80:
            assert (st.support[:, 0] <= st.support[:, 1]).all()  # no filter is empty
        st.close()


CONFIGS = [dict(output="complex"), dict(output="power"), dict(output="magnitude"),
           dict(output="power", n_mels=80, log="log10", floor=1e-10),
           dict(output="magnitude", n_mels=128, htk=True, norm=False, log="ln", floor=1e-5),
           dict(output="power", log="ln", floor=1e-3), dict(output="power", n_mels=40, win_length=-37, center=False)]

WORST = {}


@pytest.mark.parametrize("n_fft", spec.SIZES)
def test_host_reference_against_float64(n_fft):
    """|host - spec| <= spec.feature_bound, a bound derived from the formats and
    the network (nothing measured): the windowing rounding, Higham's FFT bound
    over log2 P stages relative to the frame's 2-norm, the power's rounding, the
    mel chain, half an ulp for sqrtf and one ulp for the faithful logarithms."""
    hop = n_fft // 4
    T = 3 * n_fft + 37
    worst_x, checked = 0.0, 0
    for cfg in CONFIGS:
        cfg = dict(cfg)
        if cfg.get("win_length"):
            cfg["win_length"] += n_fft
        st = mp3g.STFT(RATE, n_fft, hop, **cfg)
        kw = dict(win_length=cfg.get("win_length"), center=cfg.get("center", True))
        F = st.frames(T)
        assert F == spec.n_frames(T, n_fft, hop, kw["center"])
        for name, x in spec.signals(T, np.random.default_rng(n_fft)):
            for scale in (1.0, 2.0 ** 20) if name == "noise" else (1.0,):
                x = (x * np.float32(scale)).astype(np.float32)
                y = st.host(x)
                assert y.shape == (st.bins, F) and y.dtype == (np.complex64 if st.complex else np.float32)
                X = spec.stft64(x, n_fft, hop, kw["win_length"], kw["center"])
                dX = spec.spectrum_bound(x, n_fft, hop, kw["win_length"], kw["center"])
                fcfg = {k: v for k, v in cfg.items() if k not in ("win_length", "center")}
                want = spec.features64(x, RATE, n_fft, hop, **kw, **fcfg)
                bound = spec.feature_bound(X, dX, RATE, n_fft, st.output, st.n_mels, 0.0, 0.0, st.htk, st.norm,
                                           st.log, st.floor)
                err = np.abs(y.astype(want.dtype) - want)
                assert (err <= bound).all(), (cfg, name, scale, float((err / bound).max()))
                if st.complex and name == "noise":
                    worst_x = max(worst_x, float((err / bound).max()))
                    assert not bits(y)[0, 1::2].any() and not bits(y)[-1, 1::2].any()  # the imaginary parts: +0
                if name == "zeros" and not st.log:
                    assert not (y != 0).any()
                if name in ("zeros", "tiny") and st.log:  # the floor everywhere
                    assert (y == y[0, 0]).all() and abs(float(y[0, 0]) - float(want[0, 0])) < 1e-5
                checked += y.size
        st.close()
    WORST[n_fft] = worst_x
    print(f"n_fft {n_fft}: {checked} values, complex bins on noise: worst err / bound = {worst_x:.4f}")
    assert checked > 50000 and 0 < worst_x <= 1.0  # (not vacuous)


def test_shapes_and_edges():
    rng = np.random.default_rng(5)
    for n_fft in spec.SIZES:
        pad = n_fft // 2
        for kw in (dict(hop=1), dict(hop=n_fft), dict(hop=n_fft // 4, win_length=1),
                   dict(hop=n_fft // 4, win_length=n_fft - 1), dict(hop=n_fft // 4, win_length=n_fft)):
            for center in (True, False):
                st = mp3g.STFT(RATE, n_fft, output="complex", center=center, **kw)
                T = pad + 1 if center else n_fft  # the shortest row with a frame
                assert st.frames(T - 1) == 0 and st.frames(T) == (T // st.hop + 1 if center else 1)
                x = rng.uniform(-1, 1, T).astype(np.float32)
                n = min(st.frames(T), 5)
                y = st.host(x, n)
                want = spec.stft64(x, n_fft, st.hop, st.win_length, center, n)
                assert y.shape == (st.K, n)
                assert np.abs(y - want).max() <= spec.spectrum_bound(x, n_fft, st.hop, st.win_length, center, n).max()
                # fewer frames than available, a wider stride whose tail stays untouched
                wide = st.host(x, 1, 4)
                assert wide.shape == (st.K, 4) and np.array_equal(bits(wide[:, :1]), bits(y[:, :1]))
                assert not bits(wide[:, 1:]).any()
                with pytest.raises(mp3g.Mp3gError):
                    st.host(x, st.frames(T) + 1)
                with pytest.raises(mp3g.Mp3gError):
                    st.host(x, 2 if st.frames(T) >= 2 else 1, 0)
                with pytest.raises(mp3g.Mp3gError):
                    st.host(x[:-1], 1)
                st.close()
    # a frame's bits depend on its own samples only: not on its neighbours, not on n_frames
    st = mp3g.STFT(RATE, 2048, 512, output="complex", center=False)
    x = rng.uniform(-1, 1, 2048 + 7 * 512).astype(np.float32)
    y = st.host(x)
    for f in (0, 3, 7):
        assert np.array_equal(bits(st.host(x[f * 512:f * 512 + 2048])[:, 0]), bits(y[:, f]))
    assert np.array_equal(bits(st.host(x, 3)), bits(y[:, :3]))
    st.close()


def status_of(**kw):
    args = dict(rate=RATE, n_fft=2048, hop=512)
    args.update(kw)
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.STFT(**args)
    return e.value.status


def test_refusals():
    INV, UNS = 1, 8
    assert status_of(rate=0) == INV and status_of(rate=-1) == INV
    assert status_of(hop=0) == INV and status_of(hop=2049) == INV
    assert status_of(win_length=0) == INV and status_of(win_length=2049) == INV
    assert status_of(output="complex", n_mels=80) == INV
    assert status_of(output="complex", log="ln", floor=1e-5) == INV
    assert status_of(log="ln") == INV and status_of(log="log10", floor=0.0) == INV
    assert status_of(log="ln", floor=-1.0) == INV and status_of(log="ln", floor=1e-40) == INV
    assert status_of(log="ln", floor=float("inf")) == INV and status_of(log="ln", floor=float("nan")) == INV
    assert status_of(n_mels=80, fmin=-1.0) == INV and status_of(n_mels=80, fmax=RATE / 2 + 1) == INV
    assert status_of(n_mels=80, fmin=4000.0, fmax=4000.0) == INV
    assert status_of(output="phase") == INV and status_of(log="log2", floor=1.0) == INV
    assert status_of(device=-2) == INV
    for n_fft in (0, -256, 128, 400, 1000, 3072, 8192):
        assert status_of(n_fft=n_fft, hop=1, win_length=1) == UNS, n_fft
    assert status_of(n_mels=129) == UNS and status_of(n_mels=-1) == UNS
    h = mp3g.C.c_void_p(1)
    L = mp3g.lib()
    assert L.mp3g_stft_create(-1, RATE, 2048, 2048, 512, 1, 0, 0.0, 0.0, 0, 0.0, 8, mp3g.C.byref(h)) == INV  # a flag
    assert h.value is None  # *out = NULL
    mp3g.STFT(RATE, floor=-1.0).close()  # (ignored without a logarithm)


def logmel_bound(lm, x, F):
    """|LogMel.host - log10 mel| where mel >= 1e-6, as test_logmel_cpu derives it:
    FMA chains of n_fft steps over the float32 tables, the tables' own rounding,
    the mel chain, 2^-20 for mp3g_log10f."""
    def gamma(n):
        return n * U / (1.0 - n * U)
    fr = spec_logmel.frames64(x, lm.n_fft, lm.hop, lm.center, F)
    cw, sw, wm = (t.astype(np.float64) for t in (lm.cw, lm.sw, lm.wm))
    p = (fr @ cw.T) ** 2 + (fr @ sw.T) ** 2
    s2 = (np.abs(fr) @ np.abs(cw).T) ** 2 + (np.abs(fr) @ np.abs(sw).T) ** 2
    dp = 3.0 * gamma(lm.n_fft + 1) * s2
    length = np.maximum(0, lm.support[:, 1].astype(np.int64) - lm.support[:, 0].astype(np.int64) + 1)
    gm = gamma(length.astype(np.float64) + 1.0)[:, None]
    mel = (p @ wm.T).T
    dmel = (dp @ wm.T).T + gm * ((p + dp) @ wm.T).T + 4 * U * (s2 @ wm.T).T
    return mel, 2.0 ** -20 + dmel / (np.maximum(mel, 1e-6) * np.log(10.0))


def test_cross_check_against_logmel():
    """n_fft = 1024: the FFT route and LogMel's direct DFT are two roundings of
    the same mathematics and agree within the sum of their derived bounds."""
    st = mp3g.STFT(22050, 1024, 256, output="power", n_mels=80, log="log10", floor=1e-10)
    lm = mp3g.LogMel(22050, 1024, 256, 80, clamp=False)
    assert np.array_equal(bits(st.wm), bits(lm.wm))  # the same filter bank
    T = 5 * 1024 + 37
    worst, checked = 0.0, 0
    for name, x in spec.signals(T, np.random.default_rng(1024)):
        a, b = st.host(x), lm.host(x)
        assert a.shape == b.shape == (80, T // 256 + 1)
        if name in ("zeros", "tiny"):
            assert np.array_equal(bits(a), bits(b)) and (a == np.float32(-10.0)).all()
            continue
        mel, bound_lm = logmel_bound(lm, x, a.shape[1])
        X = spec.stft64(x, 1024, 256)
        bound_st = spec.feature_bound(X, spec.spectrum_bound(x, 1024, 256), 22050, 1024, "power", 80, 0.0, 0.0, False,
                                      True, "log10", 1e-10)
        ok = mel >= 1e-6
        err = np.abs(a.astype(np.float64) - b.astype(np.float64))
        assert ok.any() and (err[ok] <= (bound_lm + bound_st)[ok]).all(), name
        worst = max(worst, float((err[ok] / (bound_lm + bound_st)[ok]).max()))
        checked += int(ok.sum())
    print(f"STFT against LogMel at 1024: {checked} features, worst |d| / (sum of bounds) = {worst:.4f}")
    assert checked > 1000
    st.close()
    lm.close()


def test_sanitizer_program_runs_clean():
    """The new host code (table design, mp3g_stft_host with the shared transform,
    the refusals) under ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-stft"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "stft_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "stft_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
