"""The Kaldi MFCC features' host side (include/mp3g.h "Kaldi MFCC features of
decoded rows"): the DCT matrix and the lifter against
the formulas, mp3g_mfcc_host against the filter-bank features and against a
derived error bound, the exact statements as bits, its edges and refusals, and
the sanitizer build of the new host code.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_fbank as fspec
import spec_mfcc as spec
from conftest import REPO
from test_fbank_cpu import U, gamma, host_bounds

FLOOR_BITS = 0xC17F1402  # logf(2^-23)
TINY = 1e-30             # float32 underflow (absolute errors of 2^-149 the relative model does not see)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(rate, N, hop, n_mels, n_ceps, **kw):
    """An MFCC from a window length and hop in samples (the constructor takes Kaldi's milliseconds)."""
    mf = mp3g.MFCC(rate, (N + 0.5) * 1000.0 / rate, (hop + 0.5) * 1000.0 / rate, n_mels, n_ceps, **kw)
    assert (mf.N, mf.hop) == (N, hop)
    return mf


def test_symbols_abi_and_defaults():
    L = mp3g.lib()
    for fn in ("mfcc_create", "mfcc_free", "mfcc_info", "mfcc_frames", "mfcc_host", "mfcc_execute", "cmvn_rows",
               "cmvn_host"):
        assert hasattr(L, "mp3g_" + fn)
    assert L.mp3g_abi_version() == 5
    assert (mp3g.MFCC_USE_ENERGY, mp3g.MFCC_RAW_ENERGY, mp3g.CMVN_NORM_VARS) == (4, 8, 1)
    mf = mp3g.MFCC()
    assert (mf.N, mf.hop, mf.P, mf.K, mf.n_mels, mf.n_ceps, mf.scale) == (400, 160, 512, 256, 23, 13, 32768.0)
    assert (mf.use_energy, mf.raw_energy, mf.cepstral_lifter, mf.energy_floor) == (True, True, 22.0, 0.0)
    assert mf.flags == 15 and mf.dct.shape == (13, 23) and mf.lifter.shape == (13,)
    # the owned front end is FBank's, table for table
    fb = mp3g.FBank(n_mels=23)
    for name in ("cw", "sw", "wm", "support", "w"):
        assert np.array_equal(getattr(mf, name), getattr(fb, name)), name
    mf.close()
    assert mf.dct is None


@pytest.mark.parametrize("M,n_ceps", spec.TABLES)
def test_tables_against_formulas(M, n_ceps):
    """D and lift are the float64 formulas rounded once (2^-24 relative) plus
    1e-9; D D^T of the square cases is the identity to 1e-6; Q = 0 is all ones."""
    for Q in (22.0, 0.0, 7.5):
        mf = make(16000, 400, 160, M, n_ceps, cepstral_lifter=Q)
        for name, got, want in (("D", mf.dct, spec.dct_matrix(M, n_ceps)), ("lift", mf.lifter, spec.lifter(Q, n_ceps))):
            assert got.dtype == np.float32 and got.shape == want.shape
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= U * np.abs(want) + 1e-9).all(), (name, Q)
        if Q == 0.0:
            assert (bits(mf.lifter) == 0x3F800000).all()
        if M == n_ceps:
            D = mf.dct.astype(np.float64)
            assert np.abs(D @ D.T - np.eye(M)).max() <= 1e-6
        mf.close()


@pytest.mark.parametrize("rate,N,hop,M", [(16000, 400, 160, 23), (16000, 400, 160, 40), (16000, 16, 4, 4)])
def test_host_inverts_to_the_filter_bank_features(rate, N, hop, M):
    """use_energy off, Q = 0, n_ceps = M: y = D L in one float32 chain per
    coefficient, so with the exact orthogonal D,  D^T y = L + D^T ((D32 - D) L +
    delta), |D32 - D| <= u |D|, |delta_i| <= gamma(M) sum_m |D32[i][m]| |L[m]|:
    |D^T y - L|[m] <= sum_i |D[i][m]| (u + gamma(M + 1)) sum_m' |D[i][m']| |L[m']|
    + 1e-12 -- the DCT chain's bound alone, L being FBank.host's bits."""
    mf = make(rate, N, hop, M, M, use_energy=False, cepstral_lifter=0.0)
    fb = mp3g.FBank(rate, (N + 0.5) * 1000.0 / rate, (hop + 0.5) * 1000.0 / rate, M)
    x = np.random.default_rng(M).uniform(-1, 1, N + 9 * hop).astype(np.float32)
    y, L = mf.host(x).astype(np.float64), fb.host(x).astype(np.float64)
    assert y.shape == L.shape == (10, M)
    D = spec.dct_matrix(M, M)
    bound = ((U + gamma(M + 1)) * (np.abs(L) @ np.abs(D).T)) @ np.abs(D) + 1e-12
    err = np.abs(y @ D - L)
    print(f"({N}, {M}): worst err / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    mf.close()
    fb.close()


def mfcc_bounds(mf, x, scale, snip, F, kind="povey"):
    """(y, dy) [F, n_ceps] in float64: the spec's features and a bound on |y32 -
    y| for mp3g_mfcc_host, derived (u = 2^-24, gamma_n as test_fbank_cpu):

    L.  host_bounds gives mel and |mel32 - mel| <= dmel.  t -> ln(max(t, eps)) has
    slope at most 1 / max(t, eps) and mp3g_logf is faithful, so dL <= 2^-23 (|L| +
    dL') + dL', dL' = dmel / max(mel - dmel, eps): the floor caps the relative error.
    Cepstra.  c32 is an M-term chain over D32 = D (1 + <= u) + <= 1e-15: |dc| <=
    sum_m |D| dL + (gamma(M + 2) + u) sum |D| (|L| + dL) + 1e-15 sum (|L| + dL); the
    lifter is one rounded table entry and one rounded product: dy <= lift (1 + 3u)
    dc + 3u |c lift| + 1e-15.
    Energy.  s is exact (scale a power of two).  The mean's error is ONE offset per
    frame, |dmean| <= (1 + u) gamma(N + 2) mean|s|; d32 = d - dmean + r, |r| <= u
    (|d| + |dmean|).  Raw: v = d, dv = |dmean| + r.  Windowed: e32 carries the
    offset c = dmean (1 - pre + u) and the rest de as host_bounds states them, and
    v32 = fl(w32 e32) adds two roundings: dv = w (c + de) + 2u w (|e| + c + de).
    |sum (v + dv)^2 - sum v^2| <= sum (2 |v| dv + dv^2) -- for the offset alone this
    is 2 |c| sum |d| + N c^2 -- plus gamma(N + 2) on the chain over (|v| + dv)^2.
    le through the faithful logarithm like L; max(., lef) does not increase it."""
    N, hop, pre, M = mf.N, mf.hop, mf.preemphasis, mf.n_mels
    mel, dmel = host_bounds(mf, x, scale, snip, F, kind)
    L = np.log(np.maximum(mel, spec.EPS))
    dL = dmel / np.maximum(mel - dmel, spec.EPS) + TINY
    dL = dL + 2.0 ** -23 * (np.abs(L) + dL)
    D, lift = spec.dct_matrix(M, mf.n_ceps), spec.lifter(mf.cepstral_lifter, mf.n_ceps)
    c = L @ D.T
    mag = np.abs(L) + dL
    dc = dL @ np.abs(D).T + (gamma(M + 2) + U) * (mag @ np.abs(D).T) + 1e-15 * mag.sum(axis=1, keepdims=True)
    y = c * lift[None, :]
    dy = np.abs(lift)[None, :] * (1 + 3 * U) * dc + 3 * U * np.abs(y) + 1e-15
    if mf.use_energy:
        idx = np.array(fspec.frame_indices(len(x), N, hop, snip, F), dtype=np.int64).reshape(-1, N)
        s = scale * np.asarray(x, np.float64)[idx]
        if mf.remove_dc:
            d = s - s.mean(axis=1, keepdims=True)
            dmean = (1 + U) * gamma(N + 2) * np.abs(s).mean(axis=1, keepdims=True)
            dd = U * (np.abs(d) + dmean)
        else:
            d, dmean, dd = s, np.zeros((len(s), 1)), np.zeros_like(s)
        if mf.raw_energy:
            v, dv = d, dmean + dd
        else:
            def prev(a):
                return np.concatenate([a[:, :1], a[:, :-1]], axis=1)
            e = d - pre * prev(d)
            off = dmean * (1.0 - pre + U)
            de = (1 + U) * (dd + pre * (prev(dd) + U * np.abs(prev(d)))) + U * (np.abs(e) + off)
            w = fspec.window(kind, N)[None, :]
            v = w * e
            dv = w * (off + de) + 2 * U * w * (np.abs(e) + off + de) + 1e-15 * np.abs(e)
        dv = dv + 2.0 ** -149
        en = (v * v).sum(axis=1)
        den = (2 * np.abs(v) * dv + dv * dv).sum(axis=1) + gamma(N + 2) * ((np.abs(v) + dv) ** 2).sum(axis=1) + N * TINY
        assert np.abs(en - spec.energy64(x, N, hop, mf.raw_energy, kind, snip, F, scale, mf.remove_dc, pre)).max() \
            <= 1e-9 * max(1.0, en.max())
        le = np.log(np.maximum(en, spec.EPS))
        dle = den / np.maximum(en - den, spec.EPS) + TINY
        dle = dle + 2.0 ** -23 * (np.abs(le) + dle)
        if mf.energy_floor > 0.0:
            lef = np.log(mf.energy_floor)
            le, dle = np.maximum(le, lef), dle + 2.0 ** -23 * abs(lef)
        y[:, 0], dy[:, 0] = le, dle
    return y, dy


def check_against_spec(mf, x, scale, snip, kind="povey", n_frames=None):
    """Every feature of mp3g_mfcc_host within mfcc_bounds of the spec; returns
    (features, worst err / bound of the cepstra, of the energy column)."""
    got = mf.host(x, n_frames)
    F = len(got)
    assert got.shape == (F, mf.n_ceps) and got.dtype == np.float32
    if F == 0:
        return 0, 0.0, 0.0
    y, dy = mfcc_bounds(mf, x, scale, snip, F, kind)
    want = spec.mfcc64(x, mf.rate, mf.N, mf.hop, mf.n_mels, mf.n_ceps, mf.cepstral_lifter, mf.use_energy,
                       mf.raw_energy, mf.energy_floor, kind, snip=snip, count=F, scale=scale,
                       remove_dc=mf.remove_dc, preemph=mf.preemphasis)
    # the bound's centre is the spec: two float64 evaluations, apart by far less than the bound
    assert (np.abs(want - y) <= 1e-6 + 1e-3 * dy).all()
    frac = np.abs(got.astype(np.float64) - y) / dy
    assert (frac <= 1.0).all(), (float(frac.max()), np.argwhere(frac > 1.0)[:4].tolist())
    first = 1 if mf.use_energy else 0
    return got.size, float(frac[:, first:].max()) if mf.n_ceps > first else 0.0, float(frac[:, 0].max())


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("rate,N,hop,M,n_ceps", [(16000, 400, 160, 23, 13), (16000, 400, 160, 40, 40),
                                                 (22050, 551, 220, 80, 20), (16000, 16, 4, 4, 4)])
def test_host_reference_against_spec(rate, N, hop, M, n_ceps, snip, raw):
    """mp3g_mfcc_host against the independent spec within the derived bound
    (nothing measured) on spec_fbank's signals; the observed fractions of the
    bound are printed (DESIGN.md 9g records the worst)."""
    T = N + 6 * hop
    mfs = {s: make(rate, N, hop, M, n_ceps, snip_edges=snip, raw_energy=raw, scale=s) for s in (32768.0, 1.0)}
    worst_c = worst_e = 0.0
    for name, x, scale in fspec.signals(T, np.random.default_rng(N + M)):
        n, wc, we = check_against_spec(mfs[scale], x, scale, snip)
        assert n > 0
        worst_c, worst_e = max(worst_c, wc), max(worst_e, we)
        if name in ("zeros", "tiny", "constant"):  # the energy sits at the floor
            assert (bits(mfs[scale].host(x)[:, 0]) == FLOOR_BITS).all(), name
    print(f"({rate}, {N}, {hop}, {M}, {n_ceps}, snip {snip}, raw {raw}): worst err / bound: cepstra {worst_c:.4f}, "
          f"energy {worst_e:.4f}")
    for mf in mfs.values():
        mf.close()


@pytest.mark.parametrize("kw", [dict(window="hamming", raw_energy=False), dict(window="rectangular", raw_energy=False),
                                dict(preemphasis=0.0, raw_energy=False), dict(remove_dc=False),
                                dict(remove_dc=False, raw_energy=False), dict(use_energy=False),
                                dict(cepstral_lifter=0.0), dict(energy_floor=1e6)])
def test_host_reference_variants(kw):
    rng = np.random.default_rng(11)
    mf = make(16000, 400, 160, 23, 13, **kw)
    x = rng.uniform(-1.0, 1.0, 400 + 6 * 160).astype(np.float32)
    x[:700] *= np.float32(1e-3)  # (some frames below an energy floor of 1e6)
    n, wc, we = check_against_spec(mf, x, 32768.0, True, kw.get("window", "povey"))
    print(f"{kw}: {n} features, worst err / bound: cepstra {wc:.4f}, energy {we:.4f}")
    if "energy_floor" in kw:
        c0 = mf.host(x)[:, 0]
        assert (c0 == mp3g.logf(np.float32([1e6]))[0]).sum() >= 2 and (c0 > np.log(1e6)).sum() >= 2
    mf.close()


def test_exact_statements():
    """Compared as bits."""
    N, hop, T = 400, 160, 400 + 3 * 160
    rng = np.random.default_rng(3)
    noise = rng.uniform(-1, 1, T).astype(np.float32)
    # a frame that is a single impulse: the chain has one non-zero term, so it is exact
    x = np.zeros(T, np.float32)
    x[130] = np.float32(0.3)
    s = np.float32(32768.0) * x[130]
    mf = make(16000, N, hop, 23, 13, remove_dc=False)
    want = mp3g.logf(np.array([s * s], np.float32))
    assert bits(mf.host(x, 1)[0, :1]).tolist() == bits(want).tolist()
    mf.close()
    mf = make(16000, N, hop, 23, 13, remove_dc=False, raw_energy=False, preemphasis=0.0)
    v = mf.w[130] * s
    assert bits(mf.host(x, 1)[0, :1]).tolist() == bits(mp3g.logf(np.array([v * v], np.float32))).tolist()
    mf.close()
    # the floors on an all-zero row
    zeros = np.zeros(T, np.float32)
    for raw in (True, False):
        mf = make(16000, N, hop, 23, 13, energy_floor=1.0, raw_energy=raw)
        assert (bits(mf.host(zeros)[:, 0]) == 0).all()  # +0
        mf.close()
        mf = make(16000, N, hop, 23, 13, raw_energy=raw)
        assert (bits(mf.host(zeros)[:, 0]) == FLOOR_BITS).all() and mf.log_energy_floor == 0.0
        mf.close()
    # RAW_ENERGY without USE_ENERGY changes no bit; with USE_ENERGY coefficients 1.. are those without
    a = make(16000, N, hop, 23, 13, use_energy=False, raw_energy=True)
    b = make(16000, N, hop, 23, 13, use_energy=False, raw_energy=False)
    c = make(16000, N, hop, 23, 13)
    d = make(16000, N, hop, 23, 13, raw_energy=False)
    ya, yb, yc, yd = (m.host(noise) for m in (a, b, c, d))
    assert np.array_equal(bits(ya), bits(yb))
    assert np.array_equal(bits(yc[:, 1:]), bits(ya[:, 1:])) and np.array_equal(bits(yd[:, 1:]), bits(ya[:, 1:]))
    assert (yc[:, 0] != ya[:, 0]).all() and (yc[:, 0] != yd[:, 0]).all()
    for m in (a, b, c, d):
        m.close()


def test_shapes():
    rng = np.random.default_rng(5)
    N, hop = 400, 160
    for snip in (True, False):
        mf = make(16000, N, hop, 23, 13, snip_edges=snip)
        assert mf.frames(N - 1) == 0 and mf.host(np.zeros(N - 1, np.float32)).shape == (0, 13)
        for T in (N, N + hop - 1):
            assert mf.frames(T) == fspec.n_frames(T, N, hop, snip) == (1 if snip else (T + 80) // 160)
            n, _, _ = check_against_spec(mf, rng.uniform(-1, 1, T).astype(np.float32), 32768.0, snip)
            assert n == 13 * mf.frames(T)
        with pytest.raises(mp3g.Mp3gError) as e:
            mf.host(np.zeros(N - 1, np.float32), 1)
        assert e.value.status == 1
        T = 1637
        x = rng.uniform(-1, 1, T).astype(np.float32)
        F = mf.frames(T)
        assert F == fspec.n_frames(T, N, hop, snip) and F >= 8
        full = mf.host(x)
        assert np.array_equal(bits(mf.host(x, 1)), bits(full[:1]))
        assert np.array_equal(bits(mf.host(x, F - 2)), bits(full[:F - 2]))
        wide = mf.host(x, F - 2, 17)
        assert wide.shape == (F - 2, 17) and np.array_equal(bits(wide[:, :13]), bits(full[:F - 2])) and not wide[:, 13:].any()
        for bad in ((F + 1, 13), (2, 12)):
            with pytest.raises(mp3g.Mp3gError) as e:
                mf.host(x, *bad)
            assert e.value.status == 1
        assert mf.host(x, 0).shape == (0, 13)
        one = make(16000, N, hop, 23, 1, snip_edges=snip)  # n_ceps = 1: the energy alone
        assert np.array_equal(bits(one.host(x)), bits(full[:, :1]))
        one.close()
        one = make(16000, N, hop, 23, 1, snip_edges=snip, use_energy=False)
        y = one.host(x)
        assert y.shape == (F, 1) and (y[:, 0] != full[:, 0]).all()
        one.close()
        mf.close()


def test_refusals():
    L = mp3g.lib()

    def create(rate=16000, N=400, hop=160, n_mels=23, n_ceps=13, low=20.0, high=0.0, pre=0.97, scale=32768.0, Q=22.0,
               floor=0.0, window=0, flags=15, device=-1):
        h = C.c_void_p(1)  # a failed create leaves NULL
        st = L.mp3g_mfcc_create(device, rate, N, hop, n_mels, n_ceps, low, high, pre, scale, Q, floor, window, flags,
                                C.byref(h))
        if st == 0:
            L.mp3g_mfcc_free(h)
        else:
            assert h.value is None
        return st
    nan, inf = float("nan"), float("inf")
    assert create() == 0 and create(flags=0) == 0 and create(flags=8) == 0 and create(Q=0.0, floor=1.0) == 0
    assert create(n_ceps=23) == 0 and create(n_ceps=1) == 0 and create(floor=2.0 ** -126) == 0
    for kw in (dict(n_ceps=0), dict(n_ceps=-1), dict(n_ceps=24), dict(Q=-1.0), dict(Q=nan), dict(Q=inf),
               dict(floor=-1.0), dict(floor=1e-40), dict(floor=2.0 ** -127), dict(floor=nan), dict(floor=inf),
               dict(floor=1e39), dict(flags=16), dict(flags=1 << 31),
               # the front end's own
               dict(rate=0), dict(N=0), dict(hop=401), dict(n_mels=0), dict(low=-1.0), dict(high=8000.5), dict(pre=1.5),
               dict(scale=0.0), dict(scale=nan), dict(window=4), dict(device=-2)):
        assert create(**kw) == 1, kw
    for kw in (dict(N=15, hop=4), dict(N=1025), dict(n_mels=129, n_ceps=13)):
        assert create(**kw) == 8, kw
    assert L.mp3g_mfcc_create(-1, 16000, 400, 160, 23, 13, 20.0, 0.0, 0.97, 32768.0, 22.0, 0.0, 0, 15, None) == 1
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.MFCC(window="blackman")
    assert e.value.status == 1
    # the device call refuses a host-only object, a bad plane count and a null object before any device call
    mf = mp3g.MFCC()
    assert L.mp3g_mfcc_execute(mf._h, None, 1, 1, 8000, None, 10, 13, None) == 1
    assert L.mp3g_mfcc_execute(mf._h, None, 1, 3, 8000, None, 10, 13, None) == 1
    assert L.mp3g_mfcc_execute(None, None, 1, 1, 8000, None, 10, 13, None) == 1
    assert L.mp3g_mfcc_frames(None, 8000) == 0 and L.mp3g_mfcc_frames(mf._h, 1 << 62) == 0
    assert L.mp3g_mfcc_info(None, None, None, None, None, None, None) == 1
    mf.close()


def test_sanitizer_program_runs_clean():
    """The new host code (the tables, mp3g_mfcc_host, mp3g_cmvn_host, the
    refusals) under ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-mfcc"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "mfcc_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "mfcc_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
