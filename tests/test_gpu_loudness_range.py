"""The momentary and short-term maxima and the loudness range on the GPU
(include/mp3g.h "Momentary and short-term maxima, loudness range", DESIGN.md
section 9i): mp3g_loudness_range_rows against mp3g_loudness_range_host byte for
byte, nothing else written, the loudness records unchanged by it, and the
device's float64 short-term energies against the sequential float64 statement
of spec_loudness_range.py."""
import faulthandler

import numpy as np
import pytest

import spec_loudness_range as spec

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no sample and no record has
GUARD = 1
NEG_INF_BITS = 0xFF800000
H = 800  # 8000 Hz: the smallest shapes that can go wrong
STEP_LIMIT_S = 120  # every test's GPU work: the process is ended if it takes longer


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def signal(kind, T, rng):
    t = np.arange(T) / 8000.0
    if kind == "noise":
        x = 0.1 * rng.standard_normal(T)
    elif kind == "sine":
        x = 0.25 * np.sin(2 * np.pi * 997.0 * t)
    elif kind == "swell":  # noise whose level rises by 30 dB over the row: a range to measure
        x = 0.3 * rng.standard_normal(T) * 10.0 ** (-1.5 * (1.0 - np.arange(T) / max(T, 1)))
    elif kind == "gated":  # 3 s of silence, 1.5 s at -60 dB, then loud: the short-term blocks meet both gates
        level = np.where(np.arange(T) < 30 * H, 0.0, np.where(np.arange(T) < 45 * H, 1e-3, 0.3))
        x = level * rng.standard_normal(T)
    elif kind == "zeros":
        x = np.zeros(T)
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def batch_of(kinds, planes, T, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([signal(k, T, rng) for _ in range(planes)]) for k in kinds])


def check(gpu, ld, x, lengths=None, rows=None):
    """Loudness.execute with d_range on the batch x [B, C, T], in sentinel-filled
    buffers with a guard row on both sides and the sentinel in [len_r, T) of
    every row: every byte of both record arrays against the host references or
    the sentinel, the loudness records against a run without d_range, the source
    unchanged.  Returns the host's range records."""
    import torch
    B, planes, T = x.shape
    src = np.full((B + 2 * GUARD, planes, T), SENTINEL, np.uint32)
    src[GUARD:GUARD + B] = bits(x)
    ln = np.full(B, T) if lengths is None else np.minimum(np.asarray(lengths), T)
    for r in range(B):
        src[GUARD + r, :, ln[r]:] = SENTINEL
    inner = src[GUARD:GUARD + B].view(np.float32)
    want_stats, want = ld.host(inner, lengths), ld.range_host(inner, lengths)
    d_src = torch.from_numpy(src.view(np.int32)).cuda()
    d_x = d_src[GUARD:GUARD + B].view(torch.float32)
    measured = list(range(B)) if rows is None else list(rows)
    exp_s = np.full((B + 2 * GUARD, 8), SENTINEL, np.uint32)
    exp_r = exp_s.copy()
    for r in measured:
        exp_s[GUARD + r] = want_stats[r:r + 1].view(np.uint32)
        exp_r[GUARD + r] = want[r:r + 1].view(np.uint32)
    # without d_range: what the loudness records are today
    d_plain = torch.full((B + 2 * GUARD, 8), SENTINEL, dtype=torch.int32, device="cuda")
    ld.execute(d_x, lengths=lengths, rows=rows, d_stats=d_plain[GUARD:GUARD + B].view(torch.uint8))
    torch.cuda.synchronize()
    plain = d_plain.cpu().numpy().view(np.uint32)
    assert np.array_equal(plain, exp_s), np.argwhere(plain != exp_s)[:6].tolist()
    # with it
    d_all_s = torch.full((B + 2 * GUARD, 8), SENTINEL, dtype=torch.int32, device="cuda")
    d_all_r = torch.full((B + 2 * GUARD, 8), SENTINEL, dtype=torch.int32, device="cuda")
    d_range = d_all_r[GUARD:GUARD + B].view(torch.uint8)
    ld.execute(d_x, lengths=lengths, rows=rows, d_stats=d_all_s[GUARD:GUARD + B].view(torch.uint8), d_range=d_range)
    torch.cuda.synchronize()
    got_s, got_r = d_all_s.cpu().numpy().view(np.uint32), d_all_r.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_s, plain)  # (the range launch changes no loudness record)
    assert np.array_equal(got_r, exp_r), (np.argwhere(got_r != exp_r)[:6].tolist(),
                                          gpu.Loudness.range_stats(d_range)[measured], want[measured])
    assert gpu.Loudness.range_stats(d_range)[measured].tobytes() == want[measured].tobytes()
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src)  # (no sample is written)
    return want


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("T", [30 * H - 1, 30 * H, 31 * H + 17])
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, planes, T):
    """Rows of lengths 0, 4H, 29H, 30H and T in one batch, a zero row among them."""
    ld = gpu.Loudness(8000, device=0)
    assert ld.H == H
    x = batch_of(["noise", "sine", "swell", "noise", "swell", "zeros"], planes, T, seed=T + planes)
    want = check(gpu, ld, x, lengths=[0, 4 * H, 29 * H, 30 * H, T, T])
    n_short = T // H - 29 if T >= 30 * H else 0
    assert want["n_short"].tolist() == [0, 0, 0, 1 if T >= 30 * H else 0, n_short, n_short]
    assert bits(want["momentary_max"])[0] == NEG_INF_BITS and np.isfinite(want["momentary_max"][1:5]).all()
    assert bits(want["shortterm_max"])[5] == NEG_INF_BITS and want["n_range"][5] == 0 and bits(want["lra"])[5] == 0
    assert want["n_range"][4] == n_short
    check(gpu, ld, x)  # without lengths
    ld.close()


def test_seventy_segments_and_both_gates(gpu):
    """More short-term blocks than a wave has lanes; silence, -60 dB and loud
    stretches: the absolute and the relative gate both drop blocks."""
    ld = gpu.Loudness(8000, device=0)
    T = 70 * H + 3
    x = batch_of(["gated", "swell"], 2, T, seed=70)
    want = check(gpu, ld, x)
    assert want["n_short"].tolist() == [41, 41]
    assert 0 < want[0]["n_range"] < want[0]["n_short"], want[0]
    assert want[0]["lra"] > 0 and want[1]["lra"] > 5.0, want
    # both gates, on the sequential statement's numbers: a block under -70 LUFS and one under the relative gate
    s = spec.loudness_range(x[0], 8000)
    assert (s["S"] < spec.ABS_GATE).any() and want[0]["n_range"] == s["n_range"] < (s["S"] >= spec.ABS_GATE).sum()
    ld.close()


def test_many_rows_and_row_index(gpu):
    """67 rows of 31 segments, then rows= lists that skip rows: their records stay untouched."""
    ld = gpu.Loudness(8000, device=0)
    T = 31 * H + 17
    kinds = ["noise", "swell", "sine", "zeros"]
    x = batch_of([kinds[r % 4] for r in range(67)], 1, T, seed=67)
    lengths = [T - 13 * (r % 7) - (H if r % 5 == 0 else 0) for r in range(67)]
    want = check(gpu, ld, x, lengths=lengths)
    assert set(want["n_short"].tolist()) == {0, 1, 2}
    check(gpu, ld, x, lengths=lengths, rows=[1, 2, 5, 40, 66])
    check(gpu, ld, x[:9].repeat(2, axis=1), rows=[8, 0, 3])
    ld.close()


def test_short_term_energies_against_the_sequential_filter(gpu):
    """The float64 short-term energies the kernel leaves in its scratch -- the
    values the percentiles are selected from, which the float32 record cannot
    show -- within the 1e-8 that the segment energies are held to, and the
    selected ones among them."""
    import torch
    ld = gpu.Loudness(8000, device=0)
    T = 45 * H + 5
    x = batch_of(["noise", "swell", "sine"], 2, T, seed=45)
    d_range = torch.zeros((3, 32), dtype=torch.uint8, device="cuda")
    ld.execute(torch.from_numpy(x).cuda(), d_range=d_range)
    torch.cuda.synchronize()
    S1 = T // H + 1
    S = ld._range_scratch.cpu().numpy()[:3 * S1].reshape(3, S1)[:, :16]
    got = gpu.Loudness.range_stats(d_range)
    worst = 0.0
    for r in range(3):
        want = spec.loudness_range(x[r], 8000)
        assert want["n_short"] == 16 == got[r]["n_short"] and want["n_range"] == got[r]["n_range"] == 16
        assert want["margin"] > 1e-6
        worst = max(worst, np.abs(S[r] / want["S"] - 1.0).max())
        # the order statistics of the device's values against the statement's
        lo, hi = (15 * 10 + 50) // 100, (15 * 95 + 50) // 100
        for rank, v in ((lo, want["v_lo"]), (hi, want["v_hi"])):
            assert abs(np.sort(S[r])[rank] / v - 1.0) <= 1e-8
    print(f"worst relative difference of a short-term energy to the sequential filter: {worst:.3e}")
    assert worst <= 1e-8
    ld.close()


def test_arguments(gpu):
    import torch
    ld = gpu.Loudness(8000, device=0)
    x = torch.zeros((2, 2, 4000), device="cuda")
    with pytest.raises(ValueError):
        ld.execute(x, d_range=torch.zeros((2, 16), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ld.execute(x, d_range=torch.zeros((2, 32), dtype=torch.float32, device="cuda"))
    d_range = torch.full((2, 32), 0x5A, dtype=torch.uint8, device="cuda")
    ld.execute(x, rows=[], d_range=d_range)
    assert (d_range == 0x5A).all()
    ld.close()
