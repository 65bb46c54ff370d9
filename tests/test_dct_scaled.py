"""The fast kernel's scaled transforms (go-mp3_amd/csrc/dct32.h
dct2_32_scaled_to, dct4_18.h dct4_18_pk_scaled): each output short of its
post-twiddle's factor, which the kernel folds into the tables the output is
multiplied by next (the synthesis window's taps, the IMDCT windows).  Built
for the CPU (tests/native/dct_scaled_host.hip) and checked against float64:
the transforms times their scale tables, the tables themselves, and one
synthesis slot end to end with the taps scaled by the kernel's rule, so a
factor attached to the wrong value or the wrong tap parity fails here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("native") / "libdct_scaled_host.so"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=fast", "--offload-arch=gfx950",
                           "-o", str(out), os.path.join(REPO, "tests", "native", "dct_scaled_host.hip")])
    L = C.CDLL(str(out))
    L.dct32_scaled_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.dct32_scales.argtypes = [C.c_void_p, C.c_void_p]
    L.dct4_18_scaled_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.dct4_18_scales.argtypes = [C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def scales(lib):
    s, inv = np.zeros(32, np.float32), np.zeros(32, np.float32)
    lib.dct32_scales(s.ctypes.data, inv.ctypes.data)
    return s, inv


@pytest.fixture(scope="module")
def scales18(lib):
    s9, sx = np.zeros((9, 2), np.float32), np.zeros(18, np.float32)
    lib.dct4_18_scales(s9.ctypes.data, sx.ctypes.data)
    return s9, sx


def run32(lib, S):
    S = np.ascontiguousarray(S, dtype=np.float32)
    X = np.empty_like(S)
    lib.dct32_scaled_host(S.ctypes.data, X.ctypes.data, len(S))
    return X


def ref64(S):
    k = np.arange(32)
    M = np.cos(np.pi * np.outer(np.arange(32), 2 * k + 1) / 64)  # [m][k]
    return S.astype(np.float64) @ M.T


def test_scale_tables(scales, scales18):
    s, inv = scales
    # every |sigma| in [1/sqrt2, 1] (float32 of cos(pi/4) at the low end)
    lo = float(np.float32(0.7071067812))
    assert np.all(np.abs(s) >= lo) and np.all(np.abs(s) <= 1.0), s
    # kScale * kInvScale = 1 to 1 ulp
    prod = s.astype(np.float64) * inv.astype(np.float64)
    assert np.abs(prod - 1.0).max() <= 2.0 ** -23, prod
    # the sign changes are the identity twiddles' second values: X[31], X[30]
    assert sorted(np.nonzero(s < 0)[0]) == [30, 31]
    s9, sx = scales18
    assert np.all(np.abs(s9) >= lo) and np.all(np.abs(s9) <= 1.0), s9
    assert [(k, h) for k in range(9) for h in range(2) if s9[k, h] < 0] == [(0, 1)]
    # by X index: pair k = (X[2k], X[17-2k])
    for k in range(9):
        assert sx[2 * k] == s9[k, 0] and sx[17 - 2 * k] == s9[k, 1]


@pytest.mark.parametrize("scale", [1e-6, 1.0, 3e3])
def test_dct32_scaled_vs_float64(lib, scales, scale):
    """The inputs, scales and bound of test_dct32.py::test_dct32_vs_float64."""
    rng = np.random.default_rng(5)
    S = (rng.standard_normal((2000, 32)) * scale).astype(np.float32)
    X = run32(lib, S).astype(np.float64) * scales[0].astype(np.float64)
    want = ref64(S)
    err = np.abs(X - want).max(axis=1) / np.abs(S.astype(np.float64)).sum(axis=1)
    assert err.max() < 4e-7, err.max()


def test_dct32_scaled_basis(lib, scales):
    """Unit impulses give the cosine columns (every twiddle and pair index)."""
    X = run32(lib, np.eye(32, dtype=np.float32)).astype(np.float64) * scales[0]
    assert np.abs(X - ref64(np.eye(32))).max() < 1e-6


@pytest.mark.parametrize("scale", [1e-6, 1.0, 3e3])
def test_dct4_18_scaled(lib, scales18, scale):
    """The scaled packed DCT-IV-18 times kScaleX against float64 and against
    the scalar dct4_18, within the bound of test_dct32.py::test_dct4_18_packed."""
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((2000, 18)) * scale).astype(np.float32)
    Xs = np.empty_like(x)
    X = np.empty_like(x)
    lib.dct4_18_scaled_host(x.ctypes.data, Xs.ctypes.data, X.ctypes.data, len(x))
    got = Xs.astype(np.float64) * scales18[1].astype(np.float64)
    m = np.arange(18)
    want = x.astype(np.float64) @ np.cos(np.pi / 72 * np.outer(2 * m + 1, 2 * m + 1)).T
    l1 = np.abs(x.astype(np.float64)).sum(axis=1)
    assert (np.abs(got - want).max(axis=1) / l1).max() < 4e-7
    # two float32 evaluations of one sum: twice the bound apart at the most
    assert (np.abs(got - X).max(axis=1) / l1).max() < 8e-7


def test_synthesis_slot_end_to_end(lib, scales):
    """One output slot of the polyphase synthesis, all 32 outputs: the scaled
    DCT-32 of the 16 slots the window reads, then the window's taps times
    sigma by the kernel's rule (even taps read X[a_i], odd taps X[b_i]:
    granule_fast.hip shared_init, dsp_tables.h FastTables::dwin), against the
    float64 V = synthNWin * S and window sum of frame.go:642-669."""
    import oracle
    T = oracle.tables()
    nwin = T["synth_nwin"].astype(np.float64)  # [64][32]
    D = T["synth_d"].astype(np.float64)  # [512]
    rng = np.random.default_rng(11)
    n = 200
    S = rng.standard_normal((n, 16, 32)).astype(np.float32)  # [case][j slots back][subband]
    V = S.astype(np.float64) @ nwin.T  # [case][j][64]
    i = np.arange(32)
    want = np.zeros((n, 32))
    for j in range(16):
        want += D[32 * j + i] * (V[:, j, 32 + i] if j & 1 else V[:, j, i])
    # the kernel's side, in float32 values: X / sigma, and taps dwin * sigma
    Xs = run32(lib, S.reshape(-1, 32)).reshape(n, 16, 32)
    sig = scales[0]
    ma = np.where(i < 16, 16 + i, np.where(i == 16, 0, 48 - i))
    mb = np.where(i < 16, 16 - i, i - 16)
    got = np.zeros((n, 32))
    for j in range(16):
        d = T["synth_d"][32 * j + i].astype(np.float32)
        if j & 1:
            tap, m = -d, mb  # V[32+i] = -X[b_i]
        else:
            tap, m = np.where(i < 16, d, np.where(i == 16, np.float32(0), -d)), ma  # V[i] = X[a_i] | 0 | -X[a_i]
        tap = (tap * sig[m]).astype(np.float32)
        got += tap.astype(np.float64) * Xs[:, j, m].astype(np.float64)
    # bound: the transform's 4e-7 of each slot's l1 norm (test_dct32_vs_float64)
    # plus two float32 roundings of the tap (the product with sigma, sigma
    # itself: 2 * 2^-24 = 1.2e-7), weighted by |D|; V[16]'s ~1e-16 residue is
    # far below it.  A wrong sigma is off by 2 % or more.
    l1 = np.abs(S.astype(np.float64)).sum(axis=2)  # [case][j]
    bound = np.zeros((n, 32))
    for j in range(16):
        bound += np.abs(D[32 * j + i]) * l1[:, j, None]
    rel = np.abs(got - want) / bound
    assert rel.max() < 5.2e-7, rel.max()
