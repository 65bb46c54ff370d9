"""BS.1770 integrated loudness and the gain stage on the GPU (include/mp3g.h
"Integrated loudness of decoded rows"): mp3g_loudness_rows
against mp3g_loudness_host byte for byte, mp3g_gain_rows against mp3g_gain_host
bit for bit, nothing else written, and decode_windows_normalized_tensor against
the host chain applied to the un-normalised decode."""
import faulthandler

import numpy as np
import pytest

from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no sample and no record has
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


def signal(kind, rate, T, rng):
    t = np.arange(T) / rate
    if kind == "noise":
        x = 0.1 * rng.standard_normal(T)
    elif kind == "sine":
        x = 0.25 * np.sin(2 * np.pi * 997.0 * t)
    elif kind == "dc+noise":
        x = 0.9 + 1e-3 * rng.standard_normal(T)
    elif kind == "gated":  # silent, quiet and loud stretches of 0.2 s steps: both gates act on a long enough row
        level = np.array([0.0, 0.0, 0.0, 0.003, 0.003, 0.3, 0.3, 0.3])[(np.arange(T) * 5 // rate) % 8]
        x = level * rng.standard_normal(T)
    elif kind == "zeros":
        x = np.zeros(T)
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


def batch_of(kinds, rate, planes, T, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([signal(k, rate, T, rng) for _ in range(planes)]) for k in kinds])


def check(gpu, ld, x, lengths=None, rows=None, target=-23.0, ceiling=None):
    """The measurement and the gain of the batch x [B, C, T] on the device, in
    sentinel-filled buffers with a guard row on both sides and the sentinel in
    [len_r, T) of every row; every byte against the host reference or the
    sentinel.  Returns the host records."""
    import torch
    B, planes, T = x.shape
    src = np.full((B + 2 * GUARD, planes, T), SENTINEL, np.uint32)
    src[GUARD:GUARD + B] = bits(x)
    ln = np.full(B, T) if lengths is None else np.minimum(np.asarray(lengths), T)
    for r in range(B):
        src[GUARD + r, :, ln[r]:] = SENTINEL
    inner = src[GUARD:GUARD + B].view(np.float32)
    want = ld.host(inner, lengths)
    d_src = torch.from_numpy(src.view(np.int32)).cuda()
    d_x = d_src[GUARD:GUARD + B].view(torch.float32)
    d_all = torch.full((B + 2 * GUARD, 8), SENTINEL, dtype=torch.int32, device="cuda")
    d_stats = d_all[GUARD:GUARD + B].view(torch.uint8)
    out = ld.execute(d_x, lengths=lengths, rows=rows, d_stats=d_stats)
    torch.cuda.synchronize()
    assert out.data_ptr() == d_stats.data_ptr()
    got = d_all.cpu().numpy().view(np.uint32)
    exp = np.full(got.shape, SENTINEL, np.uint32)
    measured = range(B) if rows is None else rows
    for r in measured:
        exp[GUARD + r] = want[r:r + 1].view(np.uint32)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:6].tolist()
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src)  # (the measurement writes no sample)
    assert gpu.Loudness.stats(d_stats)[list(measured)].tobytes() == want[list(measured)].tobytes()
    if rows is not None:
        return want
    # the gain, in place
    y, g = gpu.loudness_gain_host(inner, want, target, peak_ceiling=ceiling, lengths=lengths)
    d_g = gpu.loudness_gain(d_x, d_stats, target, peak_ceiling=ceiling, lengths=lengths)
    torch.cuda.synchronize()
    exp_src = src.copy()
    exp_src[GUARD:GUARD + B] = bits(y)
    got_src = d_src.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_src, exp_src), np.argwhere(got_src != exp_src)[:6].tolist()
    for r in range(B):
        assert (got_src[GUARD + r, :, ln[r]:] == SENTINEL).all()
    assert np.array_equal(bits(d_g.cpu().numpy()), bits(g))
    assert np.array_equal(d_all.cpu().numpy().view(np.uint32), exp)  # (the gain writes no record)
    return want


# ---- 8000 Hz, H = 800: the smallest shapes that can go wrong --------------------------------

@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("T", [4 * 800 - 1, 4 * 800, 5 * 800 + 17])
def test_kernels_equal_host_reference_and_write_nothing_else(gpu, planes, T):
    """Rows of lengths 0, 1, 4H and T in one batch (T odd and one plane: the rows
    are not 16-byte aligned), a zero row, and the ceiling active."""
    ld = gpu.Loudness(8000, device=0)
    assert ld.H == 800
    x = batch_of(["noise", "sine", "dc+noise", "noise", "zeros"], 8000, planes, T, seed=T + planes)
    want = check(gpu, ld, x, lengths=[0, 1, 4 * 800, T, T], ceiling=0.25)
    assert want["n_blocks"].tolist() == [0, 0, 1 if T >= 3200 else 0, ld.blocks(T), ld.blocks(T)]
    assert want[1]["peak"] == abs(x[1, :, 0]).max() and bits(want["lufs"])[4] == NEG_INF_BITS
    check(gpu, ld, x)  # without lengths, without a ceiling
    ld.close()


def test_seventy_segments_in_one_row(gpu):
    """More segments than a wave has lanes; the DC offset and the stepped noise: both gates act."""
    ld = gpu.Loudness(8000, device=0)
    T = 70 * 800 + 3
    x = batch_of(["gated", "dc+noise"], 8000, 2, T, seed=70)
    want = check(gpu, ld, x)
    assert want["n_blocks"].tolist() == [67, 67]
    assert 0 < want[0]["n_gated"] < want[0]["n_abs"] < want[0]["n_blocks"], want[0]
    ld.close()


def test_many_short_rows_and_row_index(gpu):
    """67 rows of 5 segments (6 items each: rows share waves and straddle a
    workgroup), then a rows= list that skips rows: their records stay untouched."""
    ld = gpu.Loudness(8000, device=0)
    T = 5 * 800 + 17
    kinds = ["noise", "gated", "dc+noise", "sine", "zeros"]
    x = batch_of([kinds[r % 5] for r in range(67)], 8000, 1, T, seed=67)
    lengths = [T - 13 * (r % 7) for r in range(67)]
    check(gpu, ld, x, lengths=lengths)
    check(gpu, ld, x, lengths=lengths, rows=[1, 2, 5, 40, 66])
    check(gpu, ld, x[:9].repeat(2, axis=1), rows=[8, 0, 3])
    ld.close()


def test_tensor_smaller_than_one_load(gpu):
    ld = gpu.Loudness(8000, device=0)
    x = np.array([[[0.5, -0.75, 0.25]]], np.float32)
    want = check(gpu, ld, x)
    assert want[0]["peak"] == 0.75 and want[0]["n_blocks"] == 0
    ld.close()


@pytest.mark.parametrize("rate,H", [(11025, 1103), (44100, 4410), (48000, 4800)])
def test_other_rates(gpu, rate, H):
    """About 1 s: an odd H, H mod 32 = 26 and H mod 32 = 0."""
    ld = gpu.Loudness(rate, device=0)
    assert ld.H == H
    T = rate + 37
    x = batch_of(["noise", "gated", "dc+noise"], rate, 2, T, seed=rate)
    want = check(gpu, ld, x, lengths=[T, T - 5, 9 * H + 1], ceiling=0.5)
    assert want["n_blocks"].tolist() == [7, 7, 6]
    ld.close()


def test_arguments(gpu):
    import torch
    ld = gpu.Loudness(8000, device=0)
    x = torch.zeros((2, 2, 4000), device="cuda")
    with pytest.raises(ValueError):
        ld.execute(x.double())
    with pytest.raises(ValueError):
        ld.execute(x, rows=[2])
    with pytest.raises(ValueError):
        ld.execute(x, lengths=[1, 2, 3])
    with pytest.raises(gpu.Mp3gError) as e:
        ld.execute(torch.zeros((2, 3, 4000), device="cuda"))
    assert e.value.status == 1
    st = ld.execute(x, rows=[])
    assert not st.any()
    with pytest.raises(ValueError):
        gpu.loudness_gain(x, st[:1], -23.0)
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.loudness_gain(x, st, float("nan"))
    assert e.value.status == 1
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
    for f in sorted(set(rates.tolist()) - {0}):
        ld = gpu.Loudness(int(f))
        ks = np.nonzero(rates == f)[0]
        want[ks] = ld.host(rows[ks], lengths[ks])
        ld.close()
    assert (want["n_gated"][:-1] > 0).all(), want  # (not vacuous: every real stream is measured)
    measured = gpu.decode_windows_normalized_tensor(streams, starts, T, target_lufs=None, rate=rate, mode=mode,
                                                    out_format=fmt)
    assert len(measured) == len(plain) + 2
    for a, b in zip(measured[1:-2], plain[1:]):
        assert np.array_equal(a, b)
    assert np.array_equal(bits(measured[0].cpu().numpy()), bits(rows))  # measuring leaves the batch as decoded
    assert measured[-2].tobytes() == want.tobytes() and (measured[-1] == 1.0).all()
    for target, ceiling in ((-23.0, None), (-14.0, 0.5)):
        norm = gpu.decode_windows_normalized_tensor(streams, starts, T, target_lufs=target, peak_ceiling=ceiling,
                                                    rate=rate, mode=mode, out_format=fmt)
        stats, gains = norm[-2], norm[-1]
        assert stats.tobytes() == want.tobytes()
        y, g = gpu.loudness_gain_host(rows, want, target, peak_ceiling=ceiling, lengths=lengths)
        assert np.array_equal(bits(gains), bits(g)) and gains.dtype == np.float32
        shape = (B,) + (1,) * (rows.ndim - 1)
        got = norm[0].cpu().numpy()
        assert np.array_equal(bits(got), bits(rows * gains.reshape(shape)))
        assert np.array_equal(bits(got), bits(y))
        # the stream without a frame: an all-zero row, -inf, gain 1
        assert bits(stats["lufs"])[-1] == NEG_INF_BITS and gains[-1] == 1.0 and not got[-1].any()
        if ceiling is not None:
            assert np.abs(got).max() <= ceiling * (1 + 2.0 ** -23)


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
