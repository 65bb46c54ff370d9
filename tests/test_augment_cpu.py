"""The noise mixing's and the renormalisation's host side (include/mp3g.h "Room
reverberation and noise at an SNR"): mp3g_row_power_host
against the exact sum, the mix of mp3g_augment_host against the spec's float32
fmaf chain bit for bit given the gains -- the wrap, the clips, the skipped
slots, the order of the slots --, the achieved SNR, the lengths and every
refusal.  No GPU."""
import math

import numpy as np
import pytest

import mp3g
import spec_reverb as spec

U = 2.0 ** -53
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def noise():
    """(bank float32 [4, 900], lengths, powers): a full row, a short one, a silent one, one sample."""
    rng = np.random.default_rng(77)
    nz = (0.1 * rng.standard_normal((4, 900))).astype(np.float32)
    nz[2] = 0.0
    nl = [900, 333, 500, 1]
    return nz, nl, mp3g.row_power_host(nz, nl)


@pytest.fixture(scope="module")
def reverb():
    rng = np.random.default_rng(5)
    h = (0.3 * rng.uniform(-1, 1, (2, 700)) * np.exp(-np.arange(700) / 140.0)).astype(np.float32)
    h[0, 0] = h[1, 350] = 1.0
    rv = mp3g.Reverb(h, None, 16000, device=None)
    yield rv
    rv.close()


def test_row_power_against_the_exact_sum():
    """(n - 1) additions and a division against fsum and a division: (n + 2) 2^-53."""
    rng = np.random.default_rng(2)
    T = 5000
    x = rng.standard_normal((8, T)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 3, (8, 1)).astype(F32)
    lengths = [0, 1, 1023, 1024, 1025, 4096, T, T + 5]
    got = mp3g.row_power_host(x, lengths)
    for r, n in enumerate(np.minimum(lengths, T)):
        want = spec.power(x[r, :n])
        assert abs(got[r] - want) <= (n + 2) * U * want, (n, got[r], want)
    assert got[0] == 0.0 and got[1] == float(x[1, 0]) ** 2
    assert np.array_equal(mp3g.row_power_host(x), mp3g.row_power_host(x, [T] * 8))
    assert mp3g.row_power_host(np.zeros((0, 7), F32)).shape == (0,)
    assert mp3g.row_power_host(np.zeros((2, 0), F32)).tolist() == [0.0, 0.0]
    # the blocked order itself: blocks of 1,024 ascending, then the block sums
    n = 2500
    sums = []
    for b in range(0, n, 1024):
        s = 0.0
        for v in x[6, b:min(n, b + 1024)].astype(np.float64):
            s += v * v
        sums.append(s)
    total = 0.0
    for s in sums:
        total += s
    assert mp3g.row_power_host(x[6:7], [n])[0] == total / n
    with pytest.raises(ValueError):
        mp3g.row_power_host(x, [1, 2])
    with pytest.raises(ValueError):
        mp3g.row_power_host(x[0])


def gains(stats, slots, pn):
    """The float32 gains of slots [(noise index, snr_ratio), ...] from the host's
    own signal_power: float64 product, division and square root as
    include/mp3g.h orders them, rounded once."""
    return [F32(math.sqrt(float(ratio) * stats[1] / pn[i])) for i, ratio in slots]


CASES = {
    # name: [(noise index, snr_db, start, offset, wrap), ...]
    "wrap from the last sample": [(0, 10.0, 0, 899, 1)],
    "wrap of a short noise": [(1, 3.0, 7, 300, 1)],
    "one sample, repeated": [(3, 20.0, 5, 0, 1)],
    "clip at the noise's end": [(1, 0.0, 100, 0, 0)],
    "clip at the row's end": [(0, 6.0, 1400, 0, 0)],
    "start at the length": [(0, 6.0, 1500, 0, 1)],
    "start past the length": [(0, 6.0, 4000, 0, 0)],
    "a silent noise is skipped": [(2, 6.0, 0, 0, 1)],
    "none": [(-1, 6.0, 0, 0, 1)],
    "two slots in order": [(0, 10.0, 0, 0, 1), (1, 2.0, 3, 5, 1)],
    "the same two, swapped": [(1, 2.0, 3, 5, 1), (0, 10.0, 0, 0, 1)],
    "eight slots": [(0, 10.0, 0, 899, 1), (1, 3.0, 100, 0, 0), (2, 0.0, 0, 0, 1), (3, 20.0, 5, 0, 1),
                    (-1, 0.0, 0, 0, 1), (1, -5.0, 1450, 300, 0), (0, 15.0, 1000, 450, 0), (3, 8.0, 1503, 0, 1)],
}


@pytest.mark.parametrize("with_response", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_mix_against_the_fmaf_chain(noise, reverb, name, with_response):
    """n = 1500 of T = 1600, two planes.  Given y (the call without slots) and the
    gains (from the call's own signal_power), the mix is the spec's float32 fmaf
    chain bit for bit; then power_after within (n + 2) 2^-53 of the exact power
    of those samples, and the scale and the scaled samples exactly."""
    nz, nl, pn = noise
    rng = np.random.default_rng(len(name))
    n, T = 1500, 1600
    x = (0.25 * rng.standard_normal((1, 2, T))).astype(np.float32)
    kw = dict(reverb=reverb, rir_index=[1]) if with_response else {}
    y, st_y = mp3g.augment_host(x, [n], normalize=False, **kw)
    slots = CASES[name]
    add = {k: [[s[j] for s in slots]] for j, k in enumerate(("index", "snr_db", "start", "offset", "wrap"))}
    raw, st0 = mp3g.augment_host(x, [n], noise=nz, noise_lengths=nl, additive=add, normalize=False, **kw)
    out, st = mp3g.augment_host(x, [n], noise=nz, noise_lengths=nl, noise_power=pn, additive=add, **kw)
    ratios = mp3g._augment_slots(add, 1)["snr_ratio"][0]  # 10^(-snr_db / 10), as the wrapper hands it over
    assert np.allclose(ratios, [10.0 ** (-s[1] / 10.0) for s in slots], rtol=1e-15)
    for p in range(2):
        live = [s + (ratios[j],) for j, s in enumerate(slots) if s[0] >= 0 and pn[s[0]] != 0.0]
        g = gains(st_y[0, p], [(s[0], s[5]) for s in live], pn)
        want = spec.mix(y[0, p, :n], [(g[j], nz[s[0], :nl[s[0]]], s[2], s[3], s[4]) for j, s in enumerate(live)])
        assert np.array_equal(bits(raw[0, p, :n]), bits(want)), (name, p, np.argwhere(bits(raw[0, p, :n]) != bits(want))[:4])
        assert (bits(raw[0, p, n:]) == 0).all() and (bits(out[0, p, n:]) == 0).all()
        assert np.array_equal(st[0, p, :2], st_y[0, p, :2]) and np.array_equal(st0[0, p, :3], st[0, p, :3])
        pa = spec.power(want)
        assert abs(st[0, p, 2] - pa) <= (n + 2) * U * pa
        assert st0[0, p, 3] == 1.0 and st[0, p, 3] == math.sqrt(st[0, p, 0] / st[0, p, 2])
        assert np.array_equal(bits(out[0, p, :n]), bits((want.astype(np.float64) * st[0, p, 3]).astype(F32)))
        if not live or all(s[2] >= n for s in live):
            assert np.array_equal(bits(raw[0, p]), bits(y[0, p]))
    if name == "the same two, swapped":  # the order is part of the result
        first = {k: [v[0][::-1]] for k, v in add.items()}
        other, _ = mp3g.augment_host(x, [n], noise=nz, noise_lengths=nl, additive=first, normalize=False, **kw)
        assert not np.array_equal(bits(other), bits(raw))


def test_fmaf32_is_a_fused_multiply_add():
    """The spec's float32 fma against exact rational arithmetic, ties included."""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    g = rng.standard_normal(4000).astype(F32)
    a = rng.standard_normal(4000).astype(F32)
    v = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(F32)
    # ties of the float64 sum: v = 1, g a = 2^-24 + a little
    g[:4] = F32(2.0 ** -12)
    a[:4] = [F32(2.0 ** -12), F32(2.0 ** -12 + 2.0 ** -35), F32(-2.0 ** -12), F32(-2.0 ** -12 - 2.0 ** -35)]
    v[:4] = [1.0, 1.0, 1.0, 1.0]
    # the float64 sum rounds ONTO a tie whose even neighbour is the wrong one
    g[4], a[4], v[4] = F32(2.0 ** -12 * (1 + 2.0 ** -23)), F32(2.0 ** -12 * (1 - 2.0 ** -23)), F32(1 + 2.0 ** -23)
    got = spec.fmaf32(g, a, v)
    for j in range(len(g)):
        exact = Fraction(float(g[j])) * Fraction(float(a[j])) + Fraction(float(v[j]))
        r = got[j]
        lo, hi = np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))
        d = abs(Fraction(float(r)) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), j
    assert got[0] == 1.0 and got[1] > 1.0 and got[2] == F32(1 - 2.0 ** -24) and got[4] == F32(1 + 2.0 ** -23)


def test_achieved_snr(noise, reverb):
    """10 log10(signal_power / (g^2 Pn)) is snr_dB within the float32 rounding of
    g: g^2 is off by at most 2^-23 relatively, 10 / ln 10 * 2^-23 dB."""
    nz, nl, pn = noise
    rng = np.random.default_rng(3)
    x = (0.25 * rng.standard_normal((2, 1, 2000))).astype(np.float32)
    for snr in (-5.0, 0.0, 3.0, 12.5, 20.0):
        for ri in (-1, 0):
            kw = dict(reverb=reverb, rir_index=[ri, ri])
            y, st = mp3g.augment_host(x, None, normalize=False, **kw)
            v, _ = mp3g.augment_host(x, None, noise=nz, noise_lengths=nl, normalize=False,
                                     additive=dict(index=[[0], [0]], snr_db=[[snr], [snr]], wrap=[[1], [1]]), **kw)
            d = v[0, 0, :900].astype(np.float64) - y[0, 0, :900].astype(np.float64)
            ratio = mp3g._augment_slots(dict(index=[[0]], snr_db=[[snr]]), 1)["snr_ratio"][0, 0]
            g = gains(st[0, 0], [(0, ratio)], pn)[0]
            # v = fmaf(g, noise, y), one rounding: within half an ulp of v of y + g noise
            assert np.abs(d - float(g) * nz[0].astype(np.float64)).max() <= 2.0 ** -24 * np.abs(v[0, 0, :900]).max()
            achieved = 10.0 * math.log10(st[0, 0, 1] / (float(g) ** 2 * pn[0]))
            assert abs(achieved - snr) <= 10.0 / math.log(10.0) * 2.0 ** -23 * 1.01 + 1e-12, (snr, achieved)


def test_lengths_and_zero_rows(noise):
    nz, nl, pn = noise
    rng = np.random.default_rng(4)
    T = 1100
    x = (0.25 * rng.standard_normal((5, T))).astype(np.float32)
    lengths = [0, 1, T - 1, T, T + 9]
    add = dict(index=[[0]] * 5, snr_db=[[3.0]] * 5, wrap=[[1]] * 5)
    out, st = mp3g.augment_host(x, lengths, noise=nz, noise_lengths=nl, additive=add)
    for r, n in enumerate(np.minimum(lengths, T)):
        assert (bits(out[r, n:]) == 0).all()
        if n:
            assert (n == 1 or (out[r, :n] != x[r, :n]).any()) and abs(spec.power(out[r, :n]) / st[r, 0] - 1) <= 2.0 ** -22
    assert st[0].tolist() == [0.0, 0.0, 0.0, 1.0]
    full, _ = mp3g.augment_host(x, None, noise=nz, noise_lengths=nl, additive=add)
    assert np.array_equal(bits(full[3]), bits(out[3])) and np.array_equal(bits(full[4]), bits(out[4]))
    z, stz = mp3g.augment_host(np.zeros((2, T), F32), None, noise=nz, noise_lengths=nl,
                               additive={k: v[:2] for k, v in add.items()})
    assert not z.any() and stz.tolist() == [[0.0, 0.0, 0.0, 1.0]] * 2  # no signal power: a gain of 0
    e, ste = mp3g.augment_host(np.zeros((0, 2, T), F32), [])
    assert e.shape == (0, 2, T) and ste.shape == (0, 2, 4)
    e, ste = mp3g.augment_host(np.zeros((2, 0), F32), None)
    assert e.shape == (2, 0) and ste.shape == (2, 4)


def test_refusals(noise, reverb):
    nz, nl, pn = noise
    x = np.zeros((2, 2, 40), F32)
    one = dict(index=[[0], [0]])
    for kw in (dict(reverb=reverb, rir_index=[0, 2]), dict(rir_index=[0, -1]),
               dict(noise=nz, noise_lengths=nl, additive=dict(index=[[4], [0]])),
               dict(noise=nz, noise_lengths=nl, additive=dict(one, offset=[[900], [0]])),
               dict(noise=nz, noise_lengths=nl, additive=dict(index=[[1], [0]], offset=[[333], [0]])),
               dict(noise=nz, noise_lengths=[900, 0, 500, 1], additive=dict(index=[[1], [0]])),
               dict(noise=nz, noise_lengths=nl, additive=dict(index=[[0] * 9] * 2)), dict(additive=one)):
        with pytest.raises(mp3g.Mp3gError) as e:
            mp3g.augment_host(x, [40, 40], **kw)
        assert e.value.status == 1, kw
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.augment_host(np.zeros((2, 3, 40), F32))
    assert e.value.status == 1
    for bad in (dict(additive=dict(snr_db=[[1.0]] * 2)), dict(additive=dict(index=[[0]] * 3)),
                dict(additive=dict(one, start=[[-1], [0]])), dict(additive=dict(one, gain=[[1], [0]])),
                dict(rir_index=[0]), dict(noise=nz[0]), dict(noise=nz, noise_lengths=[1, 2]),
                dict(noise=nz, noise_power=[1.0])):
        with pytest.raises(ValueError):
            mp3g.augment_host(x, [40, 40], **bad)
    with pytest.raises(ValueError):
        mp3g.augment_host(x, [40])
    with pytest.raises(ValueError):
        mp3g.augment_host(x[0, 0])
    # the C calls: out of place, the scratch and a host-only object (before any device call)
    import ctypes as C
    a = mp3g._AugmentArgs()
    y, st = np.zeros_like(x), np.zeros((2, 2, 4))
    a.x, a.stats, a.n_rows, a.n_planes, a.T = x.ctypes.data, st.ctypes.data, 2, 2, 40
    lib = mp3g.lib()
    for out in (x.ctypes.data, x.ctypes.data + 4 * 79, None):
        a.out = out
        assert lib.mp3g_augment_host(None, C.byref(a)) == 1
        assert lib.mp3g_augment_rows(None, 0, C.byref(a), None, None, None, None, 0, None) == 1
    a.out = y.ctypes.data
    assert lib.mp3g_augment_host(None, C.byref(a)) == 0
    a.flags = 2
    assert lib.mp3g_augment_host(None, C.byref(a)) == 1
    a.flags = 1
    assert lib.mp3g_augment_rows(None, -1, C.byref(a), None, None, None, None, 0, None) == 1
    assert lib.mp3g_augment_rows(reverb._h, 0, C.byref(a), None, None, None, None, 0, None) == 1  # a host-only object
    assert lib.mp3g_reverb_scratch_bytes(None, 2, 2, 40) == 2 * 4 * 8
    assert lib.mp3g_reverb_scratch_bytes(reverb._h, 2, 2, 40) == (2 * 4 + 4) * 8 + 4 * 2 * 2048 * 8
    assert lib.mp3g_reverb_scratch_bytes(None, 2, 3, 40) == 0 and lib.mp3g_row_power_scratch_bytes(3, 1025) == 48
