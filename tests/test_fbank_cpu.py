"""The Kaldi filter-bank features' host side (include/mp3g.h "Kaldi filter-bank
features of decoded rows"): the float64 spec against
torch.fft.rfft, the tables against the formulas, mp3g_logf against float64 log,
mp3g_fbank_host against a derived error bound, its edges and refusals, and the
sanitizer build of the new host code.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_fbank as spec
from conftest import REPO

U = 2.0 ** -24
FLOOR = np.float32(-23.0 * np.log(2.0))  # ln(2^-23) rounded to nearest


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(rate, N, hop, n_mels, **kw):
    """An FBank from a window length and hop in samples (the constructor takes Kaldi's milliseconds)."""
    fb = mp3g.FBank(rate, (N + 0.5) * 1000.0 / rate, (hop + 0.5) * 1000.0 / rate, n_mels, **kw)
    assert (fb.N, fb.hop) == (N, hop)
    return fb


def test_symbols_and_abi():
    L = mp3g.lib()
    for fn in ("create", "free", "info", "frames", "host", "execute", "logf"):
        assert hasattr(L, "mp3g_fbank_" + fn)
    assert L.mp3g_abi_version() == 5
    assert (mp3g.FBANK_REMOVE_DC, mp3g.FBANK_SNIP_EDGES) == (1, 2)
    assert mp3g.FBANK_WINDOWS == {"povey": 0, "hamming": 1, "hanning": 2, "rectangular": 3}
    # Kaldi's conversion of milliseconds to samples
    fb = mp3g.FBank(22050)
    assert (fb.N, fb.hop, fb.P, fb.K) == (551, 220, 1024, 512)
    fb = mp3g.FBank()
    assert (fb.N, fb.hop, fb.P, fb.K, fb.n_mels, fb.scale) == (400, 160, 512, 256, 80, 32768.0)


@pytest.mark.parametrize("N,hop,kind", [(400, 160, "povey"), (551, 220, "hamming"), (16, 4, "hanning"),
                                        (1024, 1024, "rectangular")])
def test_spec_power_against_torch_rfft(N, hop, kind):
    """The spec's power spectrum against torch.fft.rfft (float64, n = P) of its
    own frames, and the folded tables against both: 1e-9 relative to max p."""
    import torch
    x = np.random.default_rng(N).uniform(-1.0, 1.0, 5 * N + 37)
    for snip in (True, False):
        fr = spec.frames64(x, N, hop, snip)
        assert fr.shape == (spec.n_frames(len(x), N, hop, snip), N)
        st = torch.fft.rfft(torch.from_numpy(fr * spec.window(kind, N)[None, :]), n=spec.padded(N), dim=1)[:, :-1]
        p_t = (st.real ** 2 + st.imag ** 2).numpy()
        p = spec.power64(x, N, hop, kind, snip=snip)
        assert p.shape == p_t.shape == (len(fr), spec.padded(N) // 2)
        err = np.abs(p - p_t).max()
        print(f"N {N} snip {snip}: max |dp| / max p = {err / p.max():.3g}")
        assert err <= 1e-9 * p.max()
        cw, sw = spec.dft_tables64(N, kind)
        assert np.abs((fr @ cw.T) ** 2 + (fr @ sw.T) ** 2 - p).max() <= 1e-9 * p.max()


def test_spec_framing():
    """Kaldi's counts and its reflection, which repeats the edge sample."""
    assert spec.n_frames(399, 400, 160) == spec.n_frames(399, 400, 160, False) == 0
    assert spec.n_frames(400, 400, 160) == 1 and spec.n_frames(559, 400, 160) == 1 and spec.n_frames(560, 400, 160) == 2
    assert spec.n_frames(400, 400, 160, False) == 3 and spec.n_frames(559, 400, 160, False) == 3
    idx = spec.frame_indices(400, 400, 160, False)
    assert idx[0][:122] == list(range(119, -1, -1)) + [0, 1]  # starts at 80 - 200 = -120: x[119] .. x[0], x[0], x[1]
    assert idx[2][-3:] == [202, 201, 200] and idx[2][199:202] == [399, 399, 398]
    x = np.arange(1.0, 21.0)
    e = spec.frames64(x, 16, 4, scale=1.0, remove_dc=False, preemph=0.5)
    assert e[0, 0] == 0.5 and e[0, 1] == 2.0 - 0.5 and e[1, 0] == 5.0 - 2.5  # the first sample refers to itself


@pytest.mark.parametrize("rate,N,hop,n_mels", spec.CONFIGS)
def test_tables_against_formulas(rate, N, hop, n_mels):
    """Every table entry is the float64 formula rounded once to float32 (2^-24
    relative) plus 1e-9 for the float64 evaluations' own differences."""
    for kind in spec.WINDOWS if n_mels == 80 and N == 400 else ("povey",):
        fb = make(rate, N, hop, n_mels, window=kind)
        P = spec.padded(N)
        K = P // 2
        assert (fb.P, fb.K) == (P, K) and fb.tile_frames in (8, 16, 32)
        assert fb.cw.shape == fb.sw.shape == (K, N) and fb.wm.shape == (n_mels, K) and fb.w.shape == (N,)
        assert fb.cw.dtype == fb.w.dtype == np.float32
        cw, sw = spec.dft_tables64(N, kind)
        wm = spec.mel_filters64(rate, N, n_mels)
        for name, got, want in (("w", fb.w, spec.window(kind, N)), ("Cw", fb.cw, cw), ("Sw", fb.sw, sw),
                                ("Wm", fb.wm, wm)):
            err = np.abs(got.astype(np.float64) - want)
            bound = U * np.abs(want) + 1e-9
            print(f"{name} ({N}, {n_mels}, {kind}): max err / bound = {float((err / bound).max()):.3f}")
            assert (err <= bound).all(), name
        assert (fb.wm >= 0).all() and (fb.wm <= 1).all() and not fb.wm[:, 0].any()
        empty = []
        for m in range(n_mels):
            lo, hi = (int(v) for v in fb.support[m])
            nz = np.flatnonzero(fb.wm[m])
            if len(nz) == 0:
                assert lo > hi
                empty.append(m)
                continue
            assert (lo, hi) == (nz[0], nz[-1]) and len(nz) == hi - lo + 1  # contiguous
        assert (np.count_nonzero(fb.wm, axis=0) <= 2).all()  # no bin lies in more than two filters
        if (N, n_mels) == (400, 128):
            assert len(empty) == 1  # narrower than a bin at the low end
        elif (N, n_mels) == (400, 80):
            assert not empty
        fb.close()


def test_mel_filters_with_a_band():
    fb = make(16000, 400, 160, 40, low_freq=80.0, high_freq=-400.0)
    wm = spec.mel_filters64(16000, 400, 40, 80.0, -400.0)
    assert (np.abs(fb.wm - wm) <= U * np.abs(wm) + 1e-9).all()
    assert not fb.wm[:, :3].any() and not fb.wm[:, 244:].any() and fb.wm[:, 3].any()  # 80 Hz .. 7600 Hz of 31.25 Hz bins


def test_logf_against_float64():
    """mp3g_logf is within one ulp of float64 log rounded to float32 (faithful)
    over all 2^23 mantissas of [1, 2) and, for every exponent of [2^-23, 2^60),
    4,097 mantissas evenly spread (the first and the last among them);
    logf(1) = +0 and logf(2^-23) = -23 ln 2 rounded to nearest.  Printed: the
    largest error in ulps of the result and how many results are not the
    nearest float32 (DESIGN.md 9e records them)."""
    def check(x):
        got = mp3g.logf(x)
        ref64 = np.log(x.astype(np.float64))
        ref = ref64.astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(ref), np.float32(2.0 ** -126))).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulp).all()
        return float((np.abs(got.astype(np.float64) - ref64) / ulp).max()), int((got != ref).sum())

    mant = np.arange(1 << 23, dtype=np.uint32)
    worst, misses = check((mant + np.uint32(127 << 23)).view(np.float32))
    print(f"binade [1, 2): max |err| = {worst:.7f} ulp, {misses} of 2^23 not the nearest float32")
    assert worst < 1.0
    some = np.concatenate([mant[::2048], mant[-1:]])
    worst_e, misses_e = 0.0, 0
    for e in range(-23, 60):
        w, n = check((some + np.uint32((127 + e) << 23)).view(np.float32))
        assert w < 1.0, e
        worst_e, misses_e = max(worst_e, w), misses_e + n
    print(f"every exponent: max |err| = {worst_e:.7f} ulp, {misses_e} of {83 * len(some)} not the nearest float32")
    y = mp3g.logf(np.array([1.0, 2.0 ** -23, 2.0, 2.0 ** 59], np.float32))
    assert bits(y).tolist() == bits(np.array([0.0, FLOOR, np.log(2.0), 59 * np.log(2.0)], np.float32)).tolist()


def gamma(n):
    return n * U / (1.0 - n * U)


def host_bounds(fb, x, scale, snip, F, kind="povey", low=20.0):
    """(mel, dmel) [F, n_mels] in float64: the spec's mel energies and a bound on
    |mel32 - mel| for mp3g_fbank_host's float32 chains, derived (u = 2^-24,
    gamma_n = n u / (1 - n u), every g below has n + 2 for the second-order terms):

    s = scale x is exact (scale is a power of two here).  The mean: an N-term
    chain and two roundings (rN, the product): |dmean| <= g(N) A, A = sum |s| / N.
    d32 = fl(s - mean32) = d - dmean + r with |r| <= u (|d| + |dmean|): the
    cancellation in d costs dmean absolutely, however small d is, but as ONE
    offset per frame.  e32 = fma(-pre32, d32[n-1], d32[n]), pre32 = pre (1 + <= u),
    carries that offset as c = dmean (1 - pre32), |c| <= |dmean| (1 - pre + u), and
    the rest as |de| <= (1 + u) (r[n] + pre (r[n-1] + u |d[n-1]|)) + u (|e| + |c|).
    re32 is an N-term chain over Cw32 = Cw (1 + <= u) + <= 1e-15 (the float64
    evaluation).  The offset passes through the window's own transform:
    |c| (|sum_n Cw| + u sum |Cw| + 1e-15 N); the rest: (1 + u) sum |Cw| de + (g(N) +
    u) S + 1e-15 E with S = sum |Cw| (|e| + |c| + de), E = sum (|e| + |c| + de); im alike.
    p32 = fl(re32^2 + fl(im32^2)): |dp| <= D + g(2) (p + D), D = 2 |re| dre + dre^2
    + 2 |im| dim + dim^2.  mel32, a chain of L = the support's length over Wm32:
    |dmel| <= sum Wm dp + (g(L) + u) sum Wm (p + dp) + 1e-15 sum (p + dp).
    Without DC removal dmean = r = c = 0."""
    N, hop, pre = fb.N, fb.hop, fb.preemphasis
    idx = np.array(spec.frame_indices(len(x), N, hop, snip, F), dtype=np.int64).reshape(-1, N)
    s = scale * np.asarray(x, np.float64)[idx]
    if fb.remove_dc:
        d = s - s.mean(axis=1, keepdims=True)
        dmean = (1 + U) * gamma(N + 2) * np.abs(s).mean(axis=1, keepdims=True)
        dd, c = U * (np.abs(d) + dmean), dmean * (1.0 - pre + U)
    else:
        d, dd, c = s, np.zeros_like(s), np.zeros((len(s), 1))

    def prev(a):
        return np.concatenate([a[:, :1], a[:, :-1]], axis=1)
    e = d - pre * prev(d)
    de = (1 + U) * (dd + pre * (prev(dd) + U * np.abs(prev(d)))) + U * (np.abs(e) + c)
    assert np.abs(e - spec.frames64(x, N, hop, snip, F, scale, fb.remove_dc, pre)).max() <= 1e-9 * max(1.0, np.abs(e).max())
    cw, sw = spec.dft_tables64(N, kind)
    mag = np.abs(e) + c + de
    E = mag.sum(axis=1, keepdims=True)

    def chain(tab):
        v = e @ tab.T
        dv = c * (np.abs(tab.sum(axis=1)) + U * np.abs(tab).sum(axis=1) + 1e-15 * N)[None, :]
        dv = dv + (1 + U) * (de @ np.abs(tab).T) + (gamma(N + 2) + U) * (mag @ np.abs(tab).T) + 1e-15 * E
        return v, dv
    re, dre = chain(cw)
    im, dim = chain(sw)
    p = re ** 2 + im ** 2
    D = 2 * np.abs(re) * dre + dre ** 2 + 2 * np.abs(im) * dim + dim ** 2
    dp = D + gamma(2 + 2) * (p + D)
    wm = spec.mel_filters64(fb.rate, N, fb.n_mels, low)
    L = np.maximum(0, fb.support[:, 1].astype(np.int64) - fb.support[:, 0].astype(np.int64) + 1).astype(np.float64)
    dmel = dp @ wm.T + (gamma(L + 2) + U)[None, :] * ((p + dp) @ wm.T) + 1e-15 * (p + dp).sum(axis=1, keepdims=True)
    return p @ wm.T, dmel


def check_against_spec(fb, x, scale, snip, kind="povey", n_frames=None):
    """Where mel >= 1 and dmel <= mel / 2: |y32 - ln mel| <= ulp(y32) + dmel /
    (mel - dmel) (mp3g_logf is faithful; |ln a - ln b| <= |a - b| / min(a, b)).
    Where mel + dmel < 2^-23 the float32 energy is below the floor too: y32 is
    ln(2^-23) exactly.  Returns (features checked, worst err / bound)."""
    y = fb.host(x, n_frames)
    F = len(y)
    assert y.shape == (F, fb.n_mels) and y.dtype == np.float32
    if F == 0:
        return 0, 0.0
    mel, dmel = host_bounds(fb, x, scale, snip, F, kind)
    floor = mel + dmel < spec.EPS
    assert (y[floor] == FLOOR).all()
    ok = (mel >= 1.0) & (dmel <= 0.5 * mel)
    if not ok.any():
        return 0, 0.0
    err = np.abs(y.astype(np.float64) - np.log(np.maximum(mel, spec.EPS)))
    bound = np.spacing(np.abs(y)).astype(np.float64) + dmel / np.maximum(mel - dmel, 0.5)
    assert (err[ok] <= bound[ok]).all(), float((err[ok] / bound[ok]).max())
    return int(ok.sum()), float((err[ok] / bound[ok]).max())


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("rate,N,hop,n_mels", spec.CONFIGS)
def test_host_reference_against_spec(rate, N, hop, n_mels, snip):
    """mp3g_fbank_host against the independent spec within the derived bound of
    host_bounds (nothing measured); the observed fraction of the bound is
    printed.  T = N + 6 hop: with SNIP_EDGES the last frame ends on the last
    sample, so the impulses at T - 2 and T - 1 are read."""
    T = N + 6 * hop
    worst, checked = 0.0, 0
    fbs = {s: make(rate, N, hop, n_mels, snip_edges=snip, scale=s) for s in (32768.0, 1.0)}
    assert fbs[1.0].frames(T) == spec.n_frames(T, N, hop, snip) == (7 if snip else (T + hop // 2) // hop)
    for name, x, scale in spec.signals(T, np.random.default_rng(N + n_mels)):
        n, w = check_against_spec(fbs[scale], x, scale, snip)
        if name in ("zeros", "tiny", "constant"):  # the floor everywhere (the constant: its mean is exact here)
            assert (fbs[scale].host(x) == FLOOR).all(), name
        elif name in ("noise", "dc+noise"):
            assert n > 0, name
        worst, checked = max(worst, w), checked + n
    print(f"({rate}, {N}, {hop}, {n_mels}, snip {snip}): {checked} features, worst err / bound = {worst:.4f}")
    assert checked >= 6 * n_mels // 2
    for fb in fbs.values():
        fb.close()


@pytest.mark.parametrize("kw", [dict(window="hamming"), dict(window="hanning"), dict(window="rectangular"),
                                dict(preemphasis=0.0), dict(preemphasis=1.0), dict(remove_dc=False), dict(scale=1.0)])
def test_host_reference_variants(kw):
    """The other windows, preemph 0 and 1, REMOVE_DC off and scale = 1 at (16 kHz, 400, 160, 80), same bound."""
    rng = np.random.default_rng(7)
    fb = make(16000, 400, 160, 80, **kw)
    x = rng.uniform(-1.0, 1.0, 400 + 6 * 160).astype(np.float32)
    if kw.get("scale") == 1.0:
        x = (x * np.float32(1000.0)).astype(np.float32)
    n, w = check_against_spec(fb, x, fb.scale, True, kw.get("window", "povey"))
    print(f"{kw}: {n} features, worst err / bound = {w:.4f}")
    assert n > 200
    fb.close()


def test_edges():
    rng = np.random.default_rng(5)
    N, hop = 400, 160
    for snip in (True, False):
        fb = make(16000, N, hop, 80, snip_edges=snip)
        # T = N - 1 has no frame in both modes; T = N and T = N + hop - 1
        assert fb.frames(N - 1) == 0 and fb.host(np.zeros(N - 1, np.float32)).shape == (0, 80)
        for T in (N, N + hop - 1):
            assert fb.frames(T) == spec.n_frames(T, N, hop, snip) == (1 if snip else (T + 80) // 160)
            x = rng.uniform(-1, 1, T).astype(np.float32)
            n, _ = check_against_spec(fb, x, 32768.0, snip)
            assert n > 40
        with pytest.raises(mp3g.Mp3gError) as e:
            fb.host(np.zeros(N - 1, np.float32), 1)
        assert e.value.status == 1
        # n_frames below the count; a wider stride leaves its tail untouched
        T = 1637
        x = rng.uniform(-1, 1, T).astype(np.float32)
        F = fb.frames(T)
        assert F == spec.n_frames(T, N, hop, snip) and F >= 8
        full = fb.host(x)
        assert np.array_equal(bits(fb.host(x, 1)), bits(full[:1]))
        assert np.array_equal(bits(fb.host(x, F - 2)), bits(full[:F - 2]))
        wide = fb.host(x, F - 2, 85)
        assert wide.shape == (F - 2, 85) and np.array_equal(bits(wide[:, :80]), bits(full[:F - 2])) and not wide[:, 80:].any()
        # a frame depends on its own samples only: the signal cut after frame 1's last sample
        if snip:
            assert np.array_equal(bits(fb.host(x[:560])), bits(full[:2]))
        for bad in ((F + 1, 80), (2, 79)):
            with pytest.raises(mp3g.Mp3gError) as e:
                fb.host(x, *bad)
            assert e.value.status == 1
        assert fb.host(x, 0).shape == (0, 80)
        fb.close()


def test_refusals():
    L = mp3g.lib()

    def create(rate=16000, N=400, hop=160, n_mels=80, low=20.0, high=0.0, pre=0.97, scale=32768.0, window=0, flags=3,
               device=-1):
        h = C.c_void_p(1)  # a failed create leaves NULL
        st = L.mp3g_fbank_create(device, rate, N, hop, n_mels, low, high, pre, scale, window, flags, C.byref(h))
        if st == 0:
            L.mp3g_fbank_free(h)
        else:
            assert h.value is None
        return st
    assert create() == 0 and create(flags=0) == 0 and create(window=3, pre=0.0, high=8000.0, low=0.0) == 0
    nan, inf = float("nan"), float("inf")
    for kw in (dict(rate=0), dict(N=0), dict(N=-4), dict(hop=0), dict(hop=401), dict(n_mels=0), dict(low=-1.0),
               dict(high=8000.5), dict(low=5000.0, high=5000.0), dict(high=-8000.0), dict(low=7000.0, high=-2000.0),
               dict(low=nan), dict(high=inf), dict(pre=-0.1), dict(pre=1.5), dict(pre=nan), dict(scale=0.0),
               dict(scale=-1.0), dict(scale=inf), dict(scale=nan), dict(scale=1e39), dict(window=4), dict(window=-1),
               dict(flags=4), dict(device=-2), dict(N=0, n_mels=200)):
        assert create(**kw) == 1, kw
    for kw in (dict(N=15, hop=4), dict(N=1025), dict(N=2048, hop=512), dict(n_mels=129)):
        assert create(**kw) == 8, kw
    assert L.mp3g_fbank_create(-1, 16000, 400, 160, 80, 20.0, 0.0, 0.97, 32768.0, 0, 3, None) == 1
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.FBank(window="blackman")
    assert e.value.status == 1
    # the device call refuses a host-only object, a bad plane count and a null object before any device call
    fb = mp3g.FBank()
    assert L.mp3g_fbank_execute(fb._h, None, 1, 1, 8000, None, 10, 80, None) == 1
    assert L.mp3g_fbank_execute(fb._h, None, 1, 3, 8000, None, 10, 80, None) == 1
    assert L.mp3g_fbank_execute(None, None, 1, 1, 8000, None, 10, 80, None) == 1
    assert L.mp3g_fbank_frames(None, 8000) == 0 and L.mp3g_fbank_frames(fb._h, 1 << 62) == 0
    assert L.mp3g_fbank_info(None, None, None, None, None, None, None, None, None) == 1


def test_sanitizer_program_runs_clean():
    """The new host code (table design, mp3g_fbank_host, mp3g_logf, the
    refusals) under ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-fbank"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "fbank_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "fbank_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
