"""The true peak and the gain against a supplied peak on the GPU (include/mp3g.h
"True peak of decoded rows"): mp3g_true_peak_rows against
mp3g_true_peak_host bit for bit with large finite values wherever the kernel
must not read, mp3g_gain_rows_peak against mp3g_gain_host_peak, and
decode_windows_normalized_tensor(peak="true", extended=True) against the host
chain applied to the un-normalised decode."""
import faulthandler

import numpy as np
import pytest

from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no result has
BIG = np.float32(1e30)  # a stray read of it shows in the maximum (a NaN would be dropped by v > tp)
GUARD = 1
NEG_INF_BITS = 0xFF800000
STEP_LIMIT_S = 120  # every test's GPU work: the process is ended if it takes longer


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def signal(kind, T, rng):
    if kind == "noise":
        x = 0.3 * rng.standard_normal(T)
    elif kind == "sine":
        x = 0.25 * np.sin(2 * np.pi * 997.0 * np.arange(T) / 8000.0)
    elif kind == "alternating":
        x = np.where(np.arange(T) % 2, -0.9, 0.9)
    elif kind == "quiet":
        x = 1e-3 * rng.standard_normal(T)
    elif kind == "zeros":
        x = np.zeros(T)
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def batch_of(kinds, planes, T, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([signal(k, T, rng) for _ in range(planes)]) for k in kinds])


def check(gpu, x, lengths=None, rows=None):
    """The true peak of the batch x [B, C, T] on the device, with a guard row of
    BIG on both sides and BIG in [len_r, T) of every row; every result against
    the host reference as uint32, the sentinel where no row was measured, the
    source unchanged.  Returns the host's values."""
    import torch
    B, planes, T = x.shape
    src = np.full((B + 2 * GUARD, planes, T), BIG, np.float32)
    src[GUARD:GUARD + B] = x
    ln = np.full(B, T) if lengths is None else np.minimum(np.asarray(lengths), T)
    for r in range(B):
        src[GUARD + r, :, ln[r]:] = BIG
    inner = src[GUARD:GUARD + B]
    want = gpu.true_peak_host(inner, lengths)
    d_src = torch.from_numpy(src).cuda()
    d_x = d_src[GUARD:GUARD + B]
    d_all = torch.full((B + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    d_out = d_all[GUARD:GUARD + B].view(torch.float32)
    out = gpu.true_peak(d_x, lengths=lengths, rows=rows, d_out=d_out)
    torch.cuda.synchronize()
    assert out.data_ptr() == d_out.data_ptr()
    got = d_all.cpu().numpy().view(np.uint32)
    exp = np.full(got.shape, SENTINEL, np.uint32)
    measured = range(B) if rows is None else rows
    for r in measured:
        exp[GUARD + r] = bits(want)[r]
    assert np.array_equal(got, exp), (np.argwhere(got != exp)[:6].tolist(), got.view(np.float32), exp.view(np.float32))
    assert np.array_equal(bits(d_src.cpu().numpy()), bits(src))  # (the measurement writes no sample)
    return want


# ---- every size at which the kernel takes another path ---------------------------------------

def sizes(gpu):
    tile = gpu.true_peak_tile()
    return [1, 3, 11, 12, 13, tile - 1, tile, tile + 1, 2 * tile + 17]


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("which", range(9))
def test_kernel_equals_host_reference_and_reads_nothing_else(gpu, planes, which):
    """Rows of lengths 0, 1, 11, 12 and T in one batch (T odd and one plane: the
    rows are not 16-byte aligned; the last row's last words end at the tensor's end)."""
    T = sizes(gpu)[which]
    x = batch_of(["noise", "sine", "alternating", "noise", "noise"], planes, T, seed=100 * which + planes)
    want = check(gpu, x, lengths=[0, 1, 11, 12, T])
    assert bits(want)[0] == 0 and want[1] == abs(x[1, :, 0]).max()
    assert (want[1:] < 10.0).all()  # (nothing of the guards' 1e30 in the reference either)
    check(gpu, x)  # without lengths
    check(gpu, x[:1])  # one row: the tensor's end is this row's


def test_tensor_smaller_than_one_load(gpu):
    x = np.array([[[0.5, -0.75, 0.25]]], np.float32)
    want = check(gpu, x)
    assert want[0] >= 0.75
    check(gpu, x[:, :, :1])
    check(gpu, np.zeros((2, 1, 0), np.float32))  # no sample at all: +0
    check(gpu, np.array([[[0.5]], [[-0.25]]], np.float32))


def test_row_index(gpu):
    """rows= lists that skip rows: the unlisted entries keep the sentinel."""
    tile = gpu.true_peak_tile()
    T = tile + 17
    kinds = ["noise", "sine", "alternating", "quiet", "zeros"]
    x = batch_of([kinds[r % 5] for r in range(23)], 1, T, seed=23)
    lengths = [T - 13 * (r % 7) for r in range(23)]
    check(gpu, x, lengths=lengths)
    check(gpu, x, lengths=lengths, rows=[1, 2, 5, 20, 22])
    check(gpu, x[:9].repeat(2, axis=1), rows=[8, 0, 3])


def test_halo_stops_at_the_row_and_the_plane(gpu):
    """The 11 samples before a plane's first are zeros, not what lies before
    it in memory: a row that ends in 1e30 before a quiet row, and a plane loud
    only in its last 11 samples before a quiet plane."""
    tile = gpu.true_peak_tile()
    for T in (64, tile + 5):
        rng = np.random.default_rng(T)
        x = (1e-3 * rng.standard_normal((3, 2, T))).astype(np.float32)
        x[0, :, T - 11:] = BIG  # row 0 ends loud (in both planes); row 1 is quiet
        x[2, 0, T - 11:] = 0.9  # row 2: plane 0 loud only in its last 11 samples, plane 1 quiet
        want = check(gpu, x)
        assert want[0] >= BIG and want[1] < 0.01  # (row 1 sees nothing of row 0)
        one = check(gpu, x[2:3, :1])  # plane 0 alone: the row's true peak is its own
        assert bits(want)[2] == bits(one)[0] and 0.9 <= want[2] < 1.8
        assert check(gpu, x[2:3, 1:])[0] < 0.01  # plane 1 alone, behind the guard row's 1e30
        # the same with the loud tails outside the rows' lengths: 1e30 right before plane 1 and the next row
        short = check(gpu, x, lengths=[T - 11] * 3)
        assert (short < 0.01).all(), short


def test_arguments(gpu):
    import torch
    x = torch.zeros((2, 2, 400), device="cuda")
    with pytest.raises(ValueError):
        gpu.true_peak(x.double())
    with pytest.raises(ValueError):
        gpu.true_peak(x, rows=[2])
    with pytest.raises(ValueError):
        gpu.true_peak(x, lengths=[1, 2, 3])
    with pytest.raises(ValueError):
        gpu.true_peak(x, d_out=torch.zeros(3, device="cuda"))
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.true_peak(torch.zeros((2, 3, 400), device="cuda"))
    assert e.value.status == 1
    assert not gpu.true_peak(x, rows=[]).any()


# ---- the gain against the true peak ---------------------------------------------------------

def test_gain_with_true_peak(gpu):
    """Bits equal the host's, nothing else written; on the first row the true-peak
    ceiling binds where the sample-peak ceiling does not."""
    import torch
    ld = gpu.Loudness(8000, device=0)
    T = 6 * 800 + 13
    n = np.arange(T)
    x = batch_of(["noise", "sine", "zeros", "noise"], 2, T, seed=5)
    x[0] = (0.5 * np.sin(np.pi * n / 2 + np.pi / 4)).astype(np.float32)  # fs/4 at 45 degrees: samples at 0.354
    lengths = [T, T - 7, T, 5 * 800]
    st = ld.host(x, lengths)
    tp = gpu.true_peak_host(x, lengths)
    target = -20.0
    te = gpu.loudness_target_energy(target)
    g_loud = np.sqrt(te / st[0]["energy"])
    ceiling = float(g_loud * np.sqrt(float(st[0]["peak"]) * float(tp[0])))
    y_s, g_s = gpu.loudness_gain_host(x, st, target, peak_ceiling=ceiling, lengths=lengths)
    y_t, g_t = gpu.loudness_gain_host(x, st, target, peak_ceiling=ceiling, lengths=lengths, peaks=tp)
    assert tp[0] > 1.3 * st[0]["peak"]
    # (the ceiling binds only against the true peak)
    assert g_s[0] == np.float32(g_loud) and g_t[0] == np.float32(ceiling) / tp[0] < g_s[0]
    assert gpu.true_peak_host(y_s, lengths)[0] > ceiling * 1.1 >= gpu.true_peak_host(y_t, lengths)[0]
    for peaks, y, g in ((None, y_s, g_s), (tp, y_t, g_t)):
        src = np.full((4 + 2 * GUARD, 2, T), SENTINEL, np.uint32)
        src[GUARD:GUARD + 4] = bits(x)
        for r in range(4):
            src[GUARD + r, :, lengths[r]:] = SENTINEL
        d_src = torch.from_numpy(src.view(np.int32)).cuda()
        d_x = d_src[GUARD:GUARD + 4].view(torch.float32)
        d_stats = torch.from_numpy(st.view(np.uint8).reshape(4, 32).copy()).cuda()
        d_peak = None if peaks is None else gpu.true_peak(d_x, lengths=lengths)
        if peaks is not None:
            assert np.array_equal(bits(d_peak.cpu().numpy()), bits(tp))
        d_g = gpu.loudness_gain(d_x, d_stats, target, peak_ceiling=ceiling, lengths=lengths, d_peak=d_peak)
        torch.cuda.synchronize()
        exp = src.copy()
        for r in range(4):
            exp[GUARD + r, :, :lengths[r]] = bits(y)[r, :, :lengths[r]]
        got = d_src.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, exp), np.argwhere(got != exp)[:6].tolist()
        assert np.array_equal(bits(d_g.cpu().numpy()), bits(g))
        assert d_stats.cpu().numpy().tobytes() == st.tobytes()
    with pytest.raises(ValueError):
        gpu.loudness_gain(d_x, d_stats, target, d_peak=torch.zeros(3, device="cuda"))
    ld.close()


# ---- end to end --------------------------------------------------------------------------------

T_NATIVE = 20000  # at least four segments at every MP3 rate (4 H = 19200 at 48 kHz)
T_16K = 8000


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, 40-frame synthetic streams at all six sample rates and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for lsf in (False, True):
        for sfreq in range(3):
            data.append(synth.encode_stream(700 + 3 * int(lsf) + sfreq, 40, lsf=lsf, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


def check_end_to_end(gpu, streams, fmt, mode, rate):
    B = len(streams)
    # (the first sample file opens with a second of silence: its window starts behind it)
    starts = [60000 if rate is None else 22000] + [100] * (B - 1)
    T = T_NATIVE if rate is None else T_16K
    kw = dict(rate=rate, mode=mode, out_format=fmt)
    if rate is None:
        plain = gpu.decode_windows_tensor(streams, starts, T, mode=mode, out_format=fmt)
        rates = gpu.stream_rates(streams)
    else:
        plain = gpu.decode_windows_resampled_tensor(streams, starts, T, rate, mode=mode, out_format=fmt)
        rates = np.where(plain[3] > 0, rate, 0)
    rows, lengths = plain[0].cpu().numpy(), plain[1]
    assert rows[:-1].reshape(B - 1, -1).any(axis=1).all() and lengths[-1] == 0 and rates[-1] == 0
    # the host chain on the un-normalised batch
    want = np.zeros(B, gpu.LOUDNESS_STATS_DTYPE)
    want["lufs"] = -np.inf
    want_range = np.zeros(B, gpu.LOUDNESS_RANGE_DTYPE)
    for name in ("momentary_max", "shortterm_max", "range_lo", "range_hi"):
        want_range[name] = -np.inf
    for f in sorted(set(rates.tolist()) - {0}):
        ld = gpu.Loudness(int(f))
        ks = np.nonzero(rates == f)[0]
        want[ks] = ld.host(rows[ks], lengths[ks])
        want_range[ks] = ld.range_host(rows[ks], lengths[ks])
        ld.close()
    want_tp = gpu.true_peak_host(rows, lengths)
    assert (want["n_gated"][:-1] > 0).all() and (want_tp[:-1] > 0).all(), want  # (not vacuous)
    assert np.isfinite(want_range["momentary_max"][:-1]).all() and want_tp[-1] == 0
    assert (want_tp >= want["peak"]).all() and (want_tp[:-1] > want["peak"][:-1]).any()
    # the default call: what it returned before these arguments existed
    for target, ceiling in ((None, None), (-14.0, 0.5)):
        old = gpu.decode_windows_normalized_tensor(streams, starts, T, target_lufs=target, peak_ceiling=ceiling, **kw)
        new = gpu.decode_windows_normalized_tensor(streams, starts, T, target_lufs=target, peak_ceiling=ceiling,
                                                   peak="sample", extended=False, **kw)
        assert len(old) == len(new) == len(plain) + 2
        assert np.array_equal(bits(old[0].cpu().numpy()), bits(new[0].cpu().numpy()))
        for a, b in zip(old[1:], new[1:]):
            assert a.tobytes() == b.tobytes()
        y, g = gpu.loudness_gain_host(rows, want, -23.0 if target is None else target, peak_ceiling=ceiling,
                                      lengths=lengths)
        if target is not None:
            assert np.array_equal(bits(old[0].cpu().numpy()), bits(y)) and np.array_equal(bits(old[-1]), bits(g))
    # measuring only
    measured = gpu.decode_windows_normalized_tensor(streams, starts, T, target_lufs=None, peak="true", extended=True,
                                                    **kw)
    assert len(measured) == len(plain) + 4
    for a, b in zip(measured[1:-4], plain[1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(bits(measured[0].cpu().numpy()), bits(rows))  # measuring leaves the batch as decoded
    assert measured[-4].tobytes() == want.tobytes() and (measured[-3] == 1.0).all()
    assert measured[-2].tobytes() == want_range.tobytes(), (measured[-2], want_range)
    assert np.array_equal(bits(measured[-1]), bits(want_tp)) and measured[-1].dtype == np.float32
    # normalised against the true peak
    for target, ceiling in ((-23.0, None), (-14.0, 0.1)):
        norm = gpu.decode_windows_normalized_tensor(streams, starts, T, target_lufs=target, peak_ceiling=ceiling,
                                                    peak="true", extended=True, **kw)
        stats, gains, rng_stats, tps = norm[-4:]
        assert stats.tobytes() == want.tobytes() and rng_stats.tobytes() == want_range.tobytes()
        assert np.array_equal(bits(tps), bits(want_tp))
        y, g = gpu.loudness_gain_host(rows, want, target, peak_ceiling=ceiling, lengths=lengths, peaks=want_tp)
        assert np.array_equal(bits(gains), bits(g)) and gains.dtype == np.float32
        got = norm[0].cpu().numpy()
        assert np.array_equal(bits(got), bits(y))
        # the stream without a frame: an all-zero row, -inf, lra 0, counts 0, true peak 0, gain 1
        assert bits(stats["lufs"])[-1] == NEG_INF_BITS and gains[-1] == 1.0 and not got[-1].any()
        assert bits(rng_stats["momentary_max"])[-1] == NEG_INF_BITS and bits(rng_stats["lra"])[-1] == 0
        assert rng_stats["n_short"][-1] == 0 and rng_stats["n_range"][-1] == 0 and bits(tps)[-1] == 0
        if ceiling is not None:
            after = gpu.true_peak_host(got, lengths)
            assert (after[want_tp > 0] <= ceiling * (1 + 2.0 ** -22)).all(), after
            y_s, g_s = gpu.loudness_gain_host(rows, want, target, peak_ceiling=ceiling, lengths=lengths)
            assert (g <= g_s).all() and (g < g_s).any()  # (the true-peak ceiling is the stricter one somewhere)


@pytest.mark.parametrize("rate", [None, 16000])
def test_end_to_end_exact_planar(gpu, streams, rate):
    check_end_to_end(gpu, streams, gpu.OUT_F32_PLANAR, gpu.MODE_EXACT, rate)


@pytest.mark.parametrize("rate", [None, 16000])
def test_end_to_end_exact_mono(gpu, streams, rate):
    check_end_to_end(gpu, streams, gpu.OUT_F32_MONO, gpu.MODE_EXACT, rate)


@pytest.mark.parametrize("rate", [None, 16000])
def test_end_to_end_fast_mode(gpu, streams, rate):
    check_end_to_end(gpu, streams, gpu.OUT_F32_PLANAR, gpu.MODE_FAST, rate)
    check_end_to_end(gpu, streams, gpu.OUT_F32_MONO, gpu.MODE_FAST, rate)
