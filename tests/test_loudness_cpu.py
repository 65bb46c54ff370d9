"""BS.1770 integrated loudness and the gain stage on the CPU (include/mp3g.h
"Integrated loudness of decoded rows"): the K-weighting
design, mp3g_loudness_host -- the segment decomposition -- against the
sequential float64 statement of spec_loudness.py, EBU Tech 3341 style
conformance, the exact statements as bits, mp3g_gain_host, the refusals and the
sanitizer program.

Observed on the 50 spec cases (x86-64): the gated energy's worst relative
difference to the sequential filter is 2.3e-10 (the DC offset under -60 dB
noise); test_host_equals_sequential_spec prints it, DESIGN.md 9h records it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mp3g
import spec_loudness as spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 16000, 44100, 48000)
KINDS = ("noise", "sine997", "dc+noise", "gated", "sine30")
NEG_INF_BITS = 0xFF800000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def signal(kind, rate, T, seed):
    """One float32 plane of T samples."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / rate
    if kind == "noise":
        x = 0.1 * rng.standard_normal(T)
    elif kind == "sine997":
        x = 0.25 * np.sin(2 * np.pi * 997.0 * t)
    elif kind == "dc+noise":
        x = 0.9 + 1e-3 * rng.standard_normal(T)
    elif kind == "gated":  # on and off at 0.7 Hz: silent blocks, loud blocks and the edges between
        x = 0.1 * rng.standard_normal(T) * (np.sin(2 * np.pi * 0.7 * t) > 0)
    elif kind == "sine30":
        x = 0.5 * np.sin(2 * np.pi * 30.0 * t)
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def rows_of(kind, rate, planes):
    T = 3 * rate + 123
    seed = 1000 * KINDS.index(kind) + RATES.index(rate)
    return np.stack([signal(kind, rate, T, seed + 100 * p) * np.float32(1.0 - 0.25 * p) for p in range(planes)])


def lufs_tolerance(want):
    """2 float32 ulps of the value plus mp3g_log10f's stated bound (half an ulp
    of the logarithm + 2^-45), times the 10 it is multiplied by."""
    lg = (want + 0.691) / 10.0
    return (2.0 * float(np.spacing(np.float32(abs(want)))) +
            10.0 * (0.5 * float(np.spacing(np.float32(abs(lg)))) + 2.0 ** -45))


# ---- the design ---------------------------------------------------------------------

def test_coefficients_are_the_standards_table_at_48k():
    ld = mp3g.Loudness(48000)
    want_s = spec.BS1770_48K["shelf_b"] + spec.BS1770_48K["shelf_a"][1:]
    want_h = spec.BS1770_48K["highpass_b"] + spec.BS1770_48K["highpass_a"][1:]
    # (the standard prints 14 decimals; the high-pass's are float32 values)
    assert np.abs(ld.shelf - want_s).max() < 1e-12, np.abs(ld.shelf - want_s).max()
    assert np.abs(ld.highpass[:3] - want_h[:3]).max() == 0.0
    assert np.abs(ld.highpass[3:] - want_h[3:]).max() < 1e-12, np.abs(ld.highpass - want_h).max()
    ld.close()


@pytest.mark.parametrize("rate,H", [(8000, 800), (11025, 1103), (22050, 2205), (44100, 4410), (48000, 4800),
                                    (96000, 9600)])
def test_segment_length_and_tables(rate, H):
    ld = mp3g.Loudness(rate)
    assert ld.H == H == spec.segment(rate)
    assert ld.blocks(4 * H - 1) == 0 and ld.blocks(4 * H) == 1 and ld.blocks(10 * H + 7) == 7
    (sb, sa), (hb, ha) = spec.k_weighting(rate)
    assert np.abs(ld.shelf - np.concatenate([sb, sa[1:]])).max() < 1e-15
    assert np.abs(ld.highpass - np.concatenate([hb, ha[1:]])).max() < 1e-15
    # V, AH and G describe the zero-input response: G = V^T V, and V against scipy
    assert ld.V.shape == (H, 4)
    assert np.allclose(ld.G, ld.V.T @ ld.V, rtol=1e-12, atol=0)
    from scipy.signal import lfilter
    # a unit shelf state s[0] is the response to zi = [1, 0] of the cascade with zero input
    y, _ = lfilter(sb, sa, np.zeros(H), zi=[1.0, 0.0])
    w = lfilter(hb, ha, y)
    assert np.abs(ld.V[:, 0] - w).max() < 1e-12
    ld.close()


# ---- the decomposition against the sequential filter ------------------------------------

def test_host_equals_sequential_spec():
    worst = 0.0
    for rate in RATES:
        ld = mp3g.Loudness(rate)
        for kind in KINDS:
            for planes in (1, 2):
                x = rows_of(kind, rate, planes)
                z = spec.block_energies(x, rate)
                margin = spec.gate_margin(z)
                assert margin > 1e-6, ("a block on a gate: pick another seed", rate, kind, planes, margin)
                want = spec.integrated(x, rate)
                got = ld.host(x[None])[0]
                case = (rate, kind, planes)
                assert (got["n_blocks"], got["n_abs"], got["n_gated"]) == (
                    want["n_blocks"], want["n_abs"], want["n_gated"]), (case, got, want)
                assert want["n_blocks"] == 27 and got["zero"] == 0
                assert want["n_gated"] > 0, case
                rel = abs(got["energy"] / want["energy"] - 1.0)
                worst = max(worst, rel)
                assert rel <= 1e-8, (case, rel)
                assert abs(float(got["lufs"]) - want["lufs"]) <= lufs_tolerance(want["lufs"]), (case, got, want)
                assert got["peak"] == np.float32(want["peak"])
                if kind == "gated":
                    assert want["n_abs"] < want["n_blocks"], case  # (the absolute gate acted)
        ld.close()
    print(f"worst relative energy difference to the sequential filter: {worst:.3e}")
    assert worst <= 1e-8


# ---- conformance, in the style of EBU Tech 3341 -----------------------------------------

def sine(rate, seconds, dbfs):
    t = np.arange(int(rate * seconds)) / rate
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * 997.0 * t)).astype(np.float32)


@pytest.mark.parametrize("rate", [48000, 44100])
def test_conformance(rate):
    ld = mp3g.Loudness(rate)

    def lufs(x):
        return float(ld.host(x[None])[0]["lufs"])
    s23, s33 = sine(rate, 20, -23.0), sine(rate, 20, -33.0)
    assert abs(lufs(np.stack([s23, s23])) + 23.0) <= 0.1
    assert abs(lufs(np.stack([s33, s33])) + 33.0) <= 0.1
    # 10 s at -36, 60 s at -23, 10 s at -36: the relative gate drops the quiet ends
    seq = np.concatenate([sine(rate, 10, -36.0), sine(rate, 60, -23.0), sine(rate, 10, -36.0)])
    st = ld.host(np.stack([seq, seq])[None])[0]
    assert abs(float(st["lufs"]) + 23.0) <= 0.1 and st["n_gated"] < st["n_abs"] == st["n_blocks"]
    # full scale in one channel of two
    full = sine(rate, 20, 0.0)
    assert abs(lufs(np.stack([full, np.zeros_like(full)])) + 3.01) <= 0.1
    ld.close()


# ---- exact statements, as bits -------------------------------------------------------------

def test_exact_statements():
    ld = mp3g.Loudness(8000)
    H = ld.H
    rng = np.random.default_rng(5)
    # a zero row
    st = ld.host(np.zeros((1, 2, 5 * H), np.float32))[0]
    assert st["energy"] == 0.0 and bits(st["lufs"]) == NEG_INF_BITS and st["n_abs"] == 0 and st["n_gated"] == 0
    assert st["n_blocks"] == 2 and st["peak"] == 0.0
    # 4H - 1 samples: no block, the peak still taken; 4H: one block
    x = (0.1 * rng.standard_normal((1, 1, 4 * H))).astype(np.float32)
    st = ld.host(x[:, :, :4 * H - 1])[0]
    assert st["n_blocks"] == 0 and bits(st["lufs"]) == NEG_INF_BITS and st["energy"] == 0.0
    assert st["peak"] == np.abs(x[0, 0, :4 * H - 1]).max()
    assert ld.host(x)[0]["n_blocks"] == 1 and ld.host(x)[0]["n_gated"] == 1
    # lengths: capped at T, zero handled, and the same as a shorter tensor
    T = 5 * H + 17
    y = (0.1 * rng.standard_normal((4, 2, T))).astype(np.float32)
    y[:, :, T - 3] = 3.0  # (in the ragged tail)
    lengths = [0, T + 1000, 4 * H + 5, T]
    st = ld.host(y, lengths)
    assert st[0].tobytes() == ld.host(np.zeros((1, 2, 0), np.float32))[0].tobytes()
    assert st[0]["n_blocks"] == 0 and st[0]["peak"] == 0.0 and bits(st[0]["lufs"]) == NEG_INF_BITS
    assert st[1].tobytes() == ld.host(y[1:2])[0].tobytes() == ld.host(y[1:2], [T])[0].tobytes()
    assert st[2].tobytes() == ld.host(y[2:3, :, :4 * H + 5])[0].tobytes() and st[2]["n_blocks"] == 1
    # the ragged tail reaches the peak only
    assert st[3]["peak"] == 3.0 and st[2]["peak"] < 3.0
    z = y[3:4].copy()
    z[:, :, 5 * H:] = 0.0
    a, b = ld.host(z)[0], st[3]
    assert a["energy"] == b["energy"] and bits(a["lufs"]) == bits(b["lufs"]) and a["peak"] < 3.0
    # a mono row is one channel: half the energy of the same signal in two planes
    m = ld.host(y[1:2, 0])[0]
    d = ld.host(np.repeat(y[1:2, :1], 2, axis=1))[0]
    assert d["energy"] == 2.0 * m["energy"]
    ld.close()


# ---- the gain stage ---------------------------------------------------------------------------

def test_gain_host():
    rate = 16000
    ld = mp3g.Loudness(rate)
    H = ld.H
    T = 12 * H + 5
    rng = np.random.default_rng(9)
    x = (0.05 * rng.standard_normal((4, 2, T))).astype(np.float32)
    x[1] *= 8.0  # loud
    x[2] = 0.0  # silent: not touched
    x[3, :, 100] = 0.9  # a peak for the ceiling
    lengths = np.array([T, T - 7, T, 11 * H + 3])
    st = ld.host(x, lengths)
    target = -23.0
    te = mp3g.loudness_target_energy(target)
    assert te == 10.0 ** ((target + 0.691) / 10.0)
    y, g = mp3g.loudness_gain_host(x, st, target, lengths=lengths)
    for r in range(4):
        if r == 2:
            assert g[r] == 1.0 and st[r]["energy"] == 0.0
            continue
        want = np.sqrt(te / st[r]["energy"])
        assert abs(float(g[r]) - want) <= 0.5 * float(np.spacing(np.float32(want))), (r, g[r], want)
    n = lengths[:, None, None] > np.arange(T)[None, None, :]
    n = np.broadcast_to(n, x.shape)
    assert np.array_equal(bits(y)[n], bits(x * g[:, None, None])[n])
    assert np.array_equal(bits(y)[~n], bits(x)[~n])  # words at n >= len: untouched
    assert np.array_equal(bits(y[2]), bits(x[2]))
    # re-measured, the rows read the target
    again = ld.host(y, lengths)
    for r in (0, 1, 3):
        assert abs(float(again[r]["lufs"]) - target) <= 1e-3, (r, again[r])
    # the ceiling: g = min(g, ceiling / peak), a float32 division
    ceiling = 0.5
    y2, g2 = mp3g.loudness_gain_host(x, st, target, peak_ceiling=ceiling, lengths=lengths)
    for r in (0, 1, 3):
        cap = np.float32(ceiling) / np.float32(st[r]["peak"])
        assert g2[r] == min(g[r], cap)
    assert g2[3] < g[3] and np.abs(y2[3, :, :lengths[3]]).max() <= ceiling * (1 + 2.0 ** -23)
    assert g2[2] == 1.0 and np.array_equal(bits(y2[2]), bits(x[2]))
    ld.close()


# ---- refusals ------------------------------------------------------------------------------------

def test_refusals():
    L = mp3g.lib()
    for rate, status in ((0, 1), (-8000, 1), (7999, 8), (192001, 8), (1 << 30, 8)):
        h = C.c_void_p(1)
        assert L.mp3g_loudness_create(-1, rate, C.byref(h)) == status and not h.value, rate
    assert L.mp3g_loudness_create(-1, 48000, None) == 1
    h = C.c_void_p(1)
    assert L.mp3g_loudness_create(-2, 48000, C.byref(h)) == 1 and not h.value
    for rate in (8000, 192000):
        ld = mp3g.Loudness(rate)
        assert ld.H == (rate + 5) // 10
        ld.close()
    ld = mp3g.Loudness(8000)
    x = np.zeros(8, np.float32)
    st = np.zeros(1, mp3g.LOUDNESS_STATS_DTYPE)
    p = mp3g._ptr
    assert L.mp3g_loudness_host(None, p(x), 1, 1, 8, None, p(st)) == 1
    assert L.mp3g_loudness_host(ld._h, p(x), 1, 3, 2, None, p(st)) == 1
    assert L.mp3g_loudness_host(ld._h, p(x), 1, 0, 8, None, p(st)) == 1
    assert L.mp3g_loudness_host(ld._h, None, 1, 1, 8, None, p(st)) == 1
    assert L.mp3g_loudness_host(ld._h, p(x), 1, 1, 8, None, None) == 1
    assert L.mp3g_loudness_host(ld._h, p(x), 1, 1, 1 << 31, None, p(st)) == 8
    assert L.mp3g_loudness_host(ld._h, None, 0, 1, 8, None, None) == 0
    assert L.mp3g_loudness_scratch_bytes(None, 1, 1, 8) == 0 and L.mp3g_loudness_scratch_bytes(ld._h, 1, 3, 8) == 0
    assert L.mp3g_loudness_scratch_bytes(ld._h, 3, 2, 1700) == 3 * 2 * 3 * 76
    assert L.mp3g_loudness_blocks(None, 100000) == 0
    assert L.mp3g_loudness_info(None, None, None, None, None, None, None) == 1
    # the device calls refuse a host-only object and bad arguments before any device call
    assert L.mp3g_loudness_rows(ld._h, p(x), 1, 1, 8, None, None, 0, p(x), p(st), None) == 1
    assert L.mp3g_loudness_rows(None, p(x), 1, 1, 8, None, None, 0, p(x), p(st), None) == 1
    assert L.mp3g_gain_host(p(x), 1, 3, 8, None, p(st), 1e-3, 0.0, None) == 1
    assert L.mp3g_gain_host(p(x), 1, 1, 8, None, p(st), 0.0, 0.0, None) == 1
    assert L.mp3g_gain_host(p(x), 1, 1, 8, None, p(st), float("nan"), 0.0, None) == 1
    assert L.mp3g_gain_host(p(x), 1, 1, 8, None, p(st), 1e-3, -1.0, None) == 1
    assert L.mp3g_gain_host(p(x), 1, 1, 8, None, None, 1e-3, 0.0, None) == 1
    assert L.mp3g_gain_host(None, 1, 1, 8, None, p(st), 1e-3, 0.0, None) == 1
    assert L.mp3g_gain_host(None, 0, 1, 8, None, None, 1e-3, 0.0, None) == 0
    assert L.mp3g_gain_rows(-1, p(x), 1, 1, 8, None, p(st), 1e-3, 0.0, None, None) == 1
    assert L.mp3g_gain_rows(0, p(x), 1, 3, 8, None, p(st), 1e-3, 0.0, None, None) == 1
    assert L.mp3g_gain_rows(0, p(x), 1, 1, 8, None, p(st), -1.0, 0.0, None, None) == 1
    ld.close()
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.Loudness(4000)
    assert e.value.status == 8


def test_sanitizer_program_runs_clean():
    """The new host code (the design, the tables, mp3g_loudness_host,
    mp3g_gain_host, the refusals) under ASan + UBSan, as a stand-alone program."""
    csrc = os.path.join(REPO, "go-mp3_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "asan-loudness"], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build", "asan", "loudness_sanitize")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "loudness_sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
