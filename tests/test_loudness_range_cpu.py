"""The momentary and short-term maxima, the loudness range and the gain against
a supplied peak on the CPU (include/mp3g.h "Momentary and short-term maxima,
loudness range"): mp3g_loudness_range_host against the
sequential float64 statement of spec_loudness_range.py, EBU Tech 3342 style
level steps, a steady sine, the edges as bits, the refusals, and
mp3g_gain_host_peak.

The record is float32 throughout, so the selected energies themselves cannot be
read from it: their float64 values are compared with the sequential filter's
within 1e-8 where they can be seen, in the device's scratch
(tests/test_gpu_loudness_range.py, whose records equal this host's byte for
byte); here the four LUFS values and lra are held to float32 resolution."""

import numpy as np
import pytest

import mp3g
import spec_loudness_range as spec

RATES = (8000, 16000, 44100, 48000)
KINDS = ("noise", "sine997", "dc+noise", "gated", "sine30")
NEG_INF_BITS = 0xFF800000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def signal(kind, rate, T, seed):
    """One float32 plane of T samples (test_loudness_cpu.py's five signals)."""
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
    """31 to 60 segments, a different count per case."""
    case = 4 * KINDS.index(kind) + RATES.index(rate)
    nseg = 31 + (case * 7 + 13 * (planes - 1)) % 30
    T = nseg * ((rate + 5) // 10) + 123
    seed = 1000 * KINDS.index(kind) + RATES.index(rate)
    return np.stack([signal(kind, rate, T, seed + 100 * p) * np.float32(1.0 - 0.25 * p) for p in range(planes)])


def lufs_tolerance(want):
    """2 float32 ulps of the value plus mp3g_log10f's stated bound (half an ulp
    of the logarithm + 2^-45), times the 10 it is multiplied by -- as
    test_loudness_cpu.py holds lufs."""
    lg = (want + 0.691) / 10.0
    return (2.0 * float(np.spacing(np.float32(abs(want)))) +
            10.0 * (0.5 * float(np.spacing(np.float32(abs(lg)))) + 2.0 ** -45))


# ---- the host reference against the sequential filter ----------------------------------

def test_host_equals_sequential_spec():
    worst = 0.0  # of the float32 LUFS values, as a fraction of their tolerance
    for rate in RATES:
        ld = mp3g.Loudness(rate)
        for kind in KINDS:
            for planes in (1, 2):
                x = rows_of(kind, rate, planes)
                want = spec.loudness_range(x, rate)
                case = (rate, kind, planes)
                assert 31 <= x.shape[-1] // ld.H <= 60 and want["n_short"] == x.shape[-1] // ld.H - 29, case
                assert want["margin"] > 1e-6, ("a short-term block on a gate: pick another seed", case, want["margin"])
                # neighbours of a selected rank: apart by more than 1e-6 on the seeded signals.  The
                # periodic ones cannot meet that -- a sine's short-term energies are all but equal, and the
                # gated noise's silent segments (1e-20) make windows that differ by one of them equal --
                # and need not: with equal counts an order statistic moves by no more than the largest
                # difference of any value, so a tie cannot cost more than the 1e-8 of the energies.  Theirs
                # must be ties outright (under 1e-9), not gaps a rounding could turn into a visible step.
                if kind in ("noise", "dc+noise"):
                    assert want["rank_gap"] > 1e-6, ("a tie at a rank: pick another seed", case, want["rank_gap"])
                else:
                    assert want["rank_gap"] > 1e-6 or want["rank_gap"] < 1e-9, (case, want["rank_gap"])
                got = ld.range_host(x[None])[0]
                assert (got["n_short"], got["n_range"], got["zero"]) == (want["n_short"], want["n_range"], 0), (
                    case, got, want["n_range"])
                assert want["n_range"] > 0, case
                for name in ("momentary_max", "shortterm_max", "range_lo", "range_hi"):
                    worst = max(worst, abs(float(got[name]) - want[name]) / lufs_tolerance(want[name]))
                    assert abs(float(got[name]) - want[name]) <= lufs_tolerance(want[name]), (case, name, got, want)
                assert abs(float(got["lra"]) - want["lra"]) <= (lufs_tolerance(want["range_lo"]) +
                                                                 lufs_tolerance(want["range_hi"]) +
                                                                 float(np.spacing(np.float32(abs(want["lra"]))))), (
                    case, got, want["lra"])
        ld.close()
    # (3 s blocks over rows of 3 to 6 s smooth these signals: no gate drops a block here; test_gates_act's do)
    print(f"worst LUFS difference to the sequential filter: {worst:.3f} of the tolerance")


# ---- EBU Tech 3342 style level steps ---------------------------------------------------------

def sine(rate, seconds, dbfs):
    t = np.arange(int(rate * seconds)) / rate
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)


@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("levels,lra,n_range", [((-20, -30), 10, 371), ((-20, -15), 5, 371), ((-40, -20), 20, 371),
                                                ((-50, -35, -20, -35, -50), 15, 627)])
def test_level_steps(rate, levels, lra, n_range):
    """A 1 kHz stereo sine, 20 s per level: the LRA within Tech 3342's 1 LU."""
    ld = mp3g.Loudness(rate)
    x = np.concatenate([sine(rate, 20, lv) for lv in levels])
    got = ld.range_host(np.stack([x, x])[None])[0]
    print(rate, levels, got)
    assert got["n_short"] == 200 * len(levels) - 29 and got["n_range"] == n_range, got
    assert abs(float(got["lra"]) - lra) <= 1.0, got
    assert got["lra"] == got["range_hi"] - got["range_lo"]
    ld.close()


@pytest.mark.parametrize("rate", [48000, 44100])
def test_steady_sine(rate):
    ld = mp3g.Loudness(rate)
    x = sine(rate, 10, -23.0)
    x = np.stack([x, x])[None]
    got, st = ld.range_host(x)[0], ld.host(x)[0]
    assert abs(float(got["momentary_max"]) - float(st["lufs"])) <= 0.01, (got, st)
    assert abs(float(got["shortterm_max"]) - float(st["lufs"])) <= 0.01, (got, st)
    assert 0.0 <= got["lra"] < 0.01 and got["n_range"] == got["n_short"] == 71
    ld.close()


# ---- the edges, as bits ------------------------------------------------------------------------

def test_edges():
    ld = mp3g.Loudness(8000)
    H = ld.H
    rng = np.random.default_rng(11)
    x = (0.1 * rng.standard_normal((1, 2, 31 * H))).astype(np.float32)
    for nseg, n_short, has_block in ((3, 0, False), (4, 0, True), (29, 0, True), (30, 1, True), (31, 2, True)):
        for T in (nseg * H, nseg * H + H - 1):
            got = ld.range_host(x[:, :, :T])[0]
            assert got["n_short"] == n_short and got["n_range"] == n_short and got["zero"] == 0, (nseg, got)
            assert (bits(got["momentary_max"]) != NEG_INF_BITS) == has_block, (nseg, got)
            assert got.tobytes() == ld.range_host(x, [T])[0].tobytes()  # (a length is a shorter tensor)
            if n_short == 0:
                assert bits(got["shortterm_max"]) == bits(got["range_lo"]) == bits(got["range_hi"]) == NEG_INF_BITS
                assert bits(got["lra"]) == 0
            else:
                assert np.isfinite(got["shortterm_max"]) and got["range_lo"] <= got["range_hi"] <= got["shortterm_max"]
    # n_range = 1: both percentiles are the one value, lra = +0
    one = ld.range_host(x[:, :, :30 * H])[0]
    assert one["n_range"] == 1 and bits(one["lra"]) == 0
    assert bits(one["range_lo"]) == bits(one["range_hi"]) == bits(one["shortterm_max"])
    # n_range = 2: ranks (1 * 10 + 50) / 100 = 0 and (1 * 95 + 50) / 100 = 1: the smaller and the larger
    two = ld.range_host(x)[0]
    assert two["n_range"] == 2 and two["range_lo"] < two["range_hi"] == two["shortterm_max"]
    assert two["lra"] == two["range_hi"] - two["range_lo"]
    # the momentary maximum is at or above the integrated loudness, the short-term at or below the momentary
    st = ld.host(x)[0]
    assert two["momentary_max"] >= st["lufs"] and two["shortterm_max"] <= two["momentary_max"]
    # a zero row: -inf, 0 and counts 0 past the gates
    zero = ld.range_host(np.zeros((1, 2, 40 * H), np.float32))[0]
    assert [bits(zero[k]) for k in ("momentary_max", "shortterm_max", "range_lo", "range_hi")] == [NEG_INF_BITS] * 4
    assert bits(zero["lra"]) == 0 and zero["n_short"] == 11 and zero["n_range"] == 0
    # lengths: zero, capped at T, several rows
    T = 33 * H + 5
    y = (0.1 * rng.standard_normal((3, 1, T))).astype(np.float32)
    got = ld.range_host(y, [0, T + 99, 30 * H])
    assert got[0].tobytes() == ld.range_host(np.zeros((1, 1, 0), np.float32))[0].tobytes() and got[0]["n_short"] == 0
    assert got[1].tobytes() == ld.range_host(y[1:2])[0].tobytes() and got[1]["n_short"] == 4
    assert got[2].tobytes() == ld.range_host(y[2:3, :, :30 * H])[0].tobytes() and got[2]["n_short"] == 1
    ld.close()


def test_gates_act():
    """Ten seconds at -60 dB around five loud ones: the relative gate drops the quiet short-term blocks;
    digital silence around them: the absolute gate does."""
    rate = 8000
    ld = mp3g.Loudness(rate)
    rng = np.random.default_rng(3)
    loud = 0.1 * rng.standard_normal(5 * rate)
    for quiet, name in ((1e-4, "relative"), (0.0, "absolute")):
        x = np.concatenate([quiet * rng.standard_normal(10 * rate), loud, quiet * rng.standard_normal(10 * rate)])
        x = x.astype(np.float32)[None, None]
        got, want = ld.range_host(x)[0], spec.loudness_range(x[0], rate)
        assert want["margin"] > 1e-6
        assert got["n_short"] == want["n_short"] == 221, (name, got)
        assert got["n_range"] == want["n_range"], (name, got, want["n_range"])
        assert 0 < got["n_range"] < got["n_short"], (name, got)
        for k in ("range_lo", "range_hi", "shortterm_max", "momentary_max"):
            assert abs(float(got[k]) - want[k]) <= lufs_tolerance(want[k]), (name, k, got, want[k])
    ld.close()


# ---- refusals: *out untouched -------------------------------------------------------------------

def test_refusals():
    L = mp3g.lib()
    ld = mp3g.Loudness(8000)
    x = np.zeros(8, np.float32)
    out = np.zeros(1, mp3g.LOUDNESS_RANGE_DTYPE)
    out.view(np.uint8)[:] = 0x5A
    before = out.tobytes()
    p = mp3g._ptr
    assert L.mp3g_loudness_range_host(None, p(x), 1, 1, 8, None, p(out)) == 1
    assert L.mp3g_loudness_range_host(ld._h, p(x), 1, 3, 2, None, p(out)) == 1
    assert L.mp3g_loudness_range_host(ld._h, p(x), 1, 0, 8, None, p(out)) == 1
    assert L.mp3g_loudness_range_host(ld._h, None, 1, 1, 8, None, p(out)) == 1
    assert L.mp3g_loudness_range_host(ld._h, p(x), 1, 1, 8, None, None) == 1
    assert L.mp3g_loudness_range_host(ld._h, p(x), 1, 1, 1 << 31, None, p(out)) == 8
    assert L.mp3g_loudness_range_host(ld._h, None, 0, 1, 8, None, None) == 0
    assert out.tobytes() == before
    assert L.mp3g_loudness_range_scratch_bytes(None, 1, 1, 8) == 0
    assert L.mp3g_loudness_range_scratch_bytes(ld._h, 1, 3, 8) == 0
    assert L.mp3g_loudness_range_scratch_bytes(ld._h, 3, 2, 1700) == 3 * 3 * 8
    # the device call refuses a host-only object and bad arguments before any device call
    assert L.mp3g_loudness_range_rows(ld._h, 1, 1, 8, None, None, 0, p(x), p(x), p(out), None) == 1
    assert L.mp3g_loudness_range_rows(None, 1, 1, 8, None, None, 0, p(x), p(x), p(out), None) == 1
    assert out.tobytes() == before
    with pytest.raises(ValueError):
        ld.range_host(np.zeros(8, np.float32))
    with pytest.raises(ValueError):
        ld.range_host(np.zeros((2, 8), np.float32), [1])
    ld.close()


# ---- the gain against a supplied peak --------------------------------------------------------

def loud_gain(energy, peak, target_energy, ceiling):
    """loud_gain of loudness_filter.h in numpy float64 / float32."""
    if not energy > 0.0:
        return np.float32(1.0)
    g = np.float32(np.sqrt(np.float64(target_energy) / np.float64(energy)))
    if ceiling > 0 and peak > 0:
        c = np.float32(ceiling) / np.float32(peak)
        g = min(c, g)
    return np.float32(g)


def test_gain_host_peak():
    rate = 16000
    ld = mp3g.Loudness(rate)
    T = 12 * ld.H + 5
    rng = np.random.default_rng(9)
    x = (0.05 * rng.standard_normal((4, 2, T))).astype(np.float32)
    x[1] *= 8.0
    x[2] = 0.0  # silent: not touched
    lengths = np.array([T, T - 7, T, 11 * ld.H + 3])
    st = ld.host(x, lengths)
    tp = mp3g.true_peak_host(x, lengths)
    te = mp3g.loudness_target_energy(-14.0)
    # without peaks: mp3g_gain_host's bits, through the new entry point
    L, p = mp3g.lib(), mp3g._ptr
    for ceiling in (0.0, 0.3):
        y0, g0 = mp3g.loudness_gain_host(x, st, -14.0, peak_ceiling=ceiling, lengths=lengths)
        y1, g1 = x.copy(), np.zeros(4, np.float32)
        ln = lengths.astype(np.uint32)
        assert L.mp3g_gain_host_peak(p(y1), 4, 2, T, p(ln), p(st), te, ceiling, p(g1), None) == 0
        assert np.array_equal(bits(y0), bits(y1)) and np.array_equal(bits(g0), bits(g1))
    # with peaks: loud_gain evaluated here
    ceiling = 0.3
    y, g = mp3g.loudness_gain_host(x, st, -14.0, peak_ceiling=ceiling, lengths=lengths, peaks=tp)
    want = np.array([loud_gain(st[r]["energy"], tp[r], te, ceiling) for r in range(4)], np.float32)
    assert np.array_equal(bits(g), bits(want)), (g, want)
    assert g[2] == 1.0 and np.array_equal(bits(y[2]), bits(x[2]))
    n = np.broadcast_to(lengths[:, None, None] > np.arange(T)[None, None, :], x.shape)
    assert np.array_equal(bits(y)[n], bits(x * g[:, None, None])[n]) and np.array_equal(bits(y)[~n], bits(x)[~n])
    # the true peak is at or above the sample peak, so its cap is at or below the sample peak's
    ys, gs = mp3g.loudness_gain_host(x, st, -14.0, peak_ceiling=ceiling, lengths=lengths)
    assert (tp >= st["peak"]).all() and (g <= gs).all() and (g[[0, 1, 3]] < gs[[0, 1, 3]]).any()
    assert (mp3g.true_peak_host(y, lengths)[[0, 1, 3]] <= ceiling * (1 + 2.0 ** -22)).all()
    # refusals, as mp3g_gain_host's
    assert L.mp3g_gain_host_peak(p(y1), 1, 3, 8, None, p(st), te, 0.0, None, p(tp)) == 1
    assert L.mp3g_gain_host_peak(p(y1), 1, 1, 8, None, p(st), 0.0, 0.0, None, p(tp)) == 1
    assert L.mp3g_gain_host_peak(p(y1), 1, 1, 8, None, None, te, 0.0, None, p(tp)) == 1
    assert L.mp3g_gain_host_peak(None, 0, 1, 8, None, None, te, 0.0, None, None) == 0
    assert L.mp3g_gain_rows_peak(-1, p(y1), 1, 1, 8, None, p(st), te, 0.0, None, None, p(tp)) == 1
    assert L.mp3g_gain_rows_peak(0, p(y1), 1, 3, 8, None, p(st), te, 0.0, None, None, p(tp)) == 1
    with pytest.raises(ValueError):
        mp3g.loudness_gain_host(x, st, -14.0, peaks=tp[:2])
    ld.close()
