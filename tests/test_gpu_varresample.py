"""The variable-ratio resampler on the GPU (include/mp3g.h "variable-ratio
resampling of decoded rows"): mp3g_varresample_rows
against mp3g_varresample_host bit for bit -- mixed ratios and gains in ONE
launch, nothing else written, degenerate rows -- and the speed and gain
keywords of the windowed calls against the host reference applied to the full
decode."""
import numpy as np
import pytest

import spec_resample as rspec
import spec_varresample as spec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no resample produces
GUARD = 1
# downsampling at MP3 rates with and without a speed factor, upsampling, a 5-digit denominator, a span no stage holds
RATIOS = [(33, 10), (4851, 1600), (3969, 1600), (10, 11), (30011, 12345), (48, 1)]
GAINS = [1.0, -0.37, 2.5, 1.0]
KINDS = ("zero", "inside", "across_end", "past_end", "far")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def launch_rows(mp3g, v, kind, C, rng, shift):
    """Ten rows for one launch: every n_out of the list with the ratios dealt
    round-robin (from `shift`), a copy row and a speed-1 row; one kind of
    out_start; source and output rows permuted.  Returns (rows, src [10, C, S],
    out_stride)."""
    tile = v.tile
    n_outs = [1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5, tile + 1, 65]
    B = len(n_outs)
    rows = np.zeros(B, mp3g.VARRESAMPLE_ROW_DTYPE)
    for i, n in enumerate(n_outs):
        num, den = RATIOS[(i + shift) % len(RATIOS)] if i < 8 else ((7, 7), (441, 160))[i - 8]
        Wr = v.half_width(num, den)
        if kind == "zero":  # the first taps fall before sample 0
            s = (0, 1, 2, den - 1, den)[i % 5] % 4000
            a, b = v.src_window(s, n, num, den)
            origin, n_src = 0, max(1, b - 7 * i)  # (i > 0: the window also runs over the source's end)
        elif kind == "inside":  # a part of the source at its origin
            s = 1000 + 17 * i
            a, b = v.src_window(s, n, num, den)
            origin, n_src = a, b - a
        elif kind == "across_end":
            origin, n_src = 0, 700 + 37 * i
            s = max(0, v.out_len(n_src, num, den) - n // 2 - 1)
        elif kind == "past_end":  # n_out = 0, or zeros
            origin, n_src = 0, 300 + i
            s = v.out_len(n_src, num, den) + 2 * (Wr * den // num + 1) + 5 + i
            n = 0 if i % 2 == 0 else n
        else:  # far out, a short source at the matching origin
            s = 2 ** 33 + 7
            a, b = v.src_window(s, n, num, den)
            origin, n_src = a + 2 * i, max(1, b - a - 5 * i)
        rows[i] = (s, origin, (3 * i + 1) % B, (7 * i + 2) % B, n_src, n, num, den, GAINS[(i + shift) % 4], 0)
    S = int(rows["n_src"].max()) + 3
    src = rng.uniform(-1.0, 1.0, (B, C, S)).astype(np.float32)
    src[3] *= np.float32(2.0 ** -120)  # subnormal products
    src[5, :, ::9] = -0.0
    return rows, src, max(n_outs) + 11


def check_launch(v, rows, src, T, C, d_rows=None, free=()):
    """One launch into a sentinel-filled buffer with guard rows; every row's
    n_out samples per plane are the host reference's bits (rows in `free` may
    hold anything there), every other word keeps its sentinel."""
    import torch
    B = src.shape[0]
    d_src = torch.from_numpy(src).cuda()
    buf = torch.full((B + 2 * GUARD, C, T), SENTINEL, dtype=torch.int32, device="cuda")
    v.rows(d_src, buf[GUARD:GUARD + B].view(torch.float32), rows if d_rows is None else d_rows)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    want = np.full(got.shape, SENTINEL, np.uint32)
    for i, row in enumerate(rows):
        n = min(int(row["n_out"]), T)
        for ch in range(C):
            x = src[row["src_row"], ch, :row["n_src"]]
            if i in free:
                want[GUARD + row["out_row"], ch, :n] = got[GUARD + row["out_row"], ch, :n]
            elif row["den"] == 0 or row["num"] == 0 or v.step(int(row["num"]), int(row["den"])) == 0:
                want[GUARD + row["out_row"], ch, :n] = 0
            else:
                want[GUARD + row["out_row"], ch, :n] = bits(v.host(x, int(row["src_origin"]), int(row["out_start"]), n,
                                                                   int(row["num"]), int(row["den"]),
                                                                   float(row["gain"])))
    bad = np.argwhere(got != want)
    assert not len(bad), (C, bad[:4].tolist(), rows)
    return want


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("zeros,quality,P", [(16, "fast", 9), (64, "best", 9), (4, "fast", 7)])
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, zeros, quality, P, C):
    """uint32 views.  `best` keeps its table in global memory whatever the
    object's choice for `fast`; 48/1 is a span no stage holds."""
    rolloff, beta = (spec.FAST if quality == "fast" else spec.BEST)[1:]
    v = gpu.VarResampler(zeros, rolloff, beta, precision=P, device=0)
    assert v.tile >= 64 and v.stage >= 1024
    # the list reaches both sides of the stage threshold
    spans = [(v.tile - 1) * num // den + 2 * v.half_width(num, den) for num, den in RATIOS]
    assert min(spans) <= v.stage // 2 and max(spans) > v.stage
    rng = np.random.default_rng(zeros + P + C)
    for k, kind in enumerate(KINDS):
        rows, src, T = launch_rows(gpu, v, kind, C, rng, k)
        want = check_launch(v, rows, src, T, C)
        # (the rows are not all zero: the comparison is not vacuous)
        assert kind == "past_end" or ((want != SENTINEL) & (want != 0)).sum() > 1000
    v.close()


def test_degenerate_rows_write_zero_and_stay_in_bounds(gpu):
    """Device rows are taken as they are: den = 0, num = 0 and I = 0 write +0 to
    their n_out samples; a descriptor of garbage positions writes only its own
    samples; the rows around them are right.  The same rows as a numpy array are
    refused."""
    import torch
    v = gpu.VarResampler(device=0)
    rng = np.random.default_rng(5)
    B, C, S, T = 8, 2, 900, 700
    src = rng.uniform(-1, 1, (B, C, S)).astype(np.float32)
    rows = np.zeros(B, gpu.VARRESAMPLE_ROW_DTYPE)
    for i in range(B):
        rows[i] = (5 * i, 0, i, (i + 3) % B, S - i, 200 + 60 * i, 441, 160, 1.0 + i, 0)
    rows["num"][1], rows["den"][1] = 441, 0
    rows["num"][3], rows["den"][3] = 0, 160
    rows["num"][4], rows["den"][4] = 436 * 3, 3           # I = floor(435 * 3 / 1308) = 0
    rows["num"][6], rows["den"][6] = 2 ** 32 - 1, 2 ** 32 - 2  # beyond 2^31, I = 434
    rows["out_start"][6], rows["src_origin"][6] = 2 ** 64 - 5, 2 ** 63 + 11
    assert v.step(436 * 3, 3) == 0
    d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    check_launch(v, rows, src, T, C, d_rows=d_rows, free=(6,))
    for bad in (1, 3, 4, 6):
        with pytest.raises(gpu.Mp3gError) as e:
            v.rows(torch.from_numpy(src).cuda(), torch.zeros((B, C, T), device="cuda"), rows[[0, bad]])
        assert e.value.status == 1
    rows2 = rows[[0, 2]].copy()
    rows2["n_out"][1] = T + 1  # a row longer than the output's rows is refused by the binding
    with pytest.raises(ValueError):
        v.rows(torch.from_numpy(src).cuda(), torch.zeros((B, C, T), device="cuda"), rows2)
    v.close()


def test_single_channel_2d_tensors_and_many_rows(gpu):
    """[*, S] tensors are one plane per row; 70,000 rows of 1,024 distinct ratios in one launch."""
    import torch
    v = gpu.VarResampler(4, 0.85, spec.FAST[2], device=0)
    rng = np.random.default_rng(3)
    n_rows, S, T = 70000, 40, 6
    src = rng.uniform(-1, 1, (n_rows, S)).astype(np.float32)
    rows = np.zeros(n_rows, gpu.VARRESAMPLE_ROW_DTYPE)
    i = np.arange(n_rows)
    rows["out_start"], rows["src_row"], rows["out_row"] = i % 11, i, n_rows - 1 - i
    rows["n_src"], rows["n_out"] = S - i % 5, 1 + (i * 7) % T
    rows["num"], rows["den"], rows["gain"] = 900 + i % 1024, 1000, 1.0 + (i % 3)
    out = torch.full((n_rows, T), SENTINEL, dtype=torch.int32, device="cuda")
    v.rows(torch.from_numpy(src).cuda(), out.view(torch.float32), rows)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    for row in rows[::37]:
        n = int(row["n_out"])
        assert np.array_equal(got[row["out_row"], :n],
                              bits(v.host(src[row["src_row"], :row["n_src"]], 0, int(row["out_start"]), n,
                                          int(row["num"]), int(row["den"]), float(row["gain"]))))
    tail = np.arange(T)[None, :] >= rows["n_out"][::-1, None]  # (out_row = n_rows - 1 - i)
    assert (got[tail] == SENTINEL).all() and (got[~tail] != SENTINEL).all()
    v.close()


# ---- end to end -----------------------------------------------------------------------

T_E2E = 1500
SPEEDS = [(9, 10), 1, (11, 10), 1.037]


@pytest.fixture(scope="module")
def streams(gpu, sample_files):
    """The two sample files, 40-frame synthetic streams at all six sample rates
    and a stream without a frame; per format their full exact decodes as numpy;
    a speed and a gain per stream."""
    class S:
        def __init__(self):
            self.data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
            self.rates = [44100, 22050]
            for lsf in (False, True):
                for sfreq, f in enumerate((44100, 48000, 32000)):
                    self.data.append(synth.encode_stream(300 + 3 * int(lsf) + sfreq, 40, lsf=lsf, sfreq=sfreq))
                    self.rates.append(f >> int(lsf))
            self.data.append(b"\x00" * 700)
            self.rates.append(0)
            self.speed = [SPEEDS[k % 4] for k in range(len(self.data))]
            self.gain = [(1.0, 0.5, -1.25, 1.0, 2.0)[k % 5] for k in range(len(self.data))]
            self.cache = {}

        def full(self, fmt):
            if fmt not in self.cache:
                _, views, _, _ = gpu.decode_streams_tensor(self.data, mode=gpu.MODE_EXACT, out_format=fmt)
                vs = [v.cpu().numpy().copy() for v in views]
                for v in vs:
                    v.setflags(write=False)
                self.cache[fmt] = vs
            return self.cache[fmt]
    return S()


def expected_rows(mp3g, views, rates, rate, starts, T, speed, gain, quality=spec.FAST):
    """(rows [B, planes, T], lengths) from VarResampler.host on each stream's
    full view; lengths by the formula clamp(ceil(N den / num) - start, 0, T)."""
    planes = views[0].shape[0] if views[0].ndim == 2 else 1
    want = np.zeros((len(views), planes, T), np.float32)
    lengths = np.zeros(len(views), np.int64)
    v = mp3g.VarResampler(*quality)
    for k, (view, f) in enumerate(zip(views, rates)):
        view = view.reshape(planes, -1)
        if not f:
            continue
        num, den = v.ratio(f, rate, speed[k])
        n = max(0, min(T, -(-view.shape[1] * den // num) - starts[k]))
        lengths[k] = n
        for ch in range(planes):
            want[k, ch, :n] = v.host(view[ch], 0, starts[k], n, num, den, gain[k])
    return want, lengths


def start_sets(mp3g, views, rates, rate, T, speed):
    """Three starts per stream, in perturbed samples: 0, mid-stream, running past the stream's end."""
    sets = [[], [], []]
    for k, (v, f) in enumerate(zip(views, rates)):
        n_y = mp3g.VarResampler.out_len(v.shape[-1], *mp3g.VarResampler.ratio(f, rate, speed[k])) if f else 0
        for s, val in zip(sets, (0, n_y // 2 + 13, max(0, n_y - T // 2))):
            s.append(val)
    return sets


@pytest.mark.parametrize("fmt", ["planar", "mono"])
def test_end_to_end_exact(gpu, streams, fmt):
    fmt = {"planar": gpu.OUT_F32_PLANAR, "mono": gpu.OUT_F32_MONO}[fmt]
    views = streams.full(fmt)
    T, rate = T_E2E, 16000
    assert gpu.VarResampler.ratio(44100, rate, 1.037) == (457317, 160000)
    for i, starts in enumerate(start_sets(gpu, views, streams.rates, rate, T, streams.speed)):
        batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(
            streams.data, starts, T, rate, out_format=fmt, n_threads=4, speed=streams.speed, gain=streams.gain)
        assert rates.tolist() == streams.rates
        want, want_len = expected_rows(gpu, views, streams.rates, rate, starts, T, streams.speed, streams.gain)
        assert lengths.tolist() == want_len.tolist(), starts
        got = batch.cpu().numpy().reshape(want.shape)
        assert np.array_equal(bits(got), bits(want)), (starts, np.argwhere(bits(got) != bits(want))[:4].tolist())
        assert lengths.max() == (T, T, T // 2)[i] and want.any() and not got[-1].any()
    # one of the two keywords alone: the other is 1 for every stream
    starts = [0] * len(streams.data)
    ones = [1] * len(streams.data)
    for kw, sp, gn in ((dict(speed=streams.speed), streams.speed, ones), (dict(gain=streams.gain), ones, streams.gain)):
        batch, lengths, _, _ = gpu.decode_windows_resampled_tensor(streams.data, starts, T, rate, out_format=fmt, **kw)
        want, want_len = expected_rows(gpu, views, streams.rates, rate, starts, T, sp, gn)
        assert lengths.tolist() == want_len.tolist()
        assert np.array_equal(bits(batch.cpu().numpy().reshape(want.shape)), bits(want))


def test_end_to_end_best_quality(gpu, streams):
    views = streams.full(gpu.OUT_F32_PLANAR)
    starts = start_sets(gpu, views, streams.rates, 16000, T_E2E, streams.speed)[2]
    batch, lengths, _, _ = gpu.decode_windows_resampled_tensor(streams.data, starts, T_E2E, 16000, quality="best",
                                                               speed=streams.speed, gain=streams.gain)
    want, want_len = expected_rows(gpu, views, streams.rates, 16000, starts, T_E2E, streams.speed, streams.gain,
                                   spec.BEST)
    assert lengths.tolist() == want_len.tolist()
    assert np.array_equal(bits(batch.cpu().numpy()), bits(want))


def test_without_the_keywords_the_polyphase_path_runs(gpu, streams):
    """speed=None, gain=None: the bits of Resampler.host on the full decode, as before."""
    views = streams.full(gpu.OUT_F32_PLANAR)
    starts = [13] * len(streams.data)
    batch, lengths, _, _ = gpu.decode_windows_resampled_tensor(streams.data, starts, T_E2E, 16000, speed=None,
                                                               gain=None)
    want = np.zeros((len(views), 2, T_E2E), np.float32)
    for k, (v, f) in enumerate(zip(views, streams.rates)):
        if f:
            r = gpu.Resampler(f, 16000, *rspec.FAST)
            n = max(0, min(T_E2E, r.out_len(v.shape[1]) - starts[k]))
            assert lengths[k] == n
            for ch in range(2):
                want[k, ch, :n] = r.host(v[ch], 0, starts[k], n)
    assert np.array_equal(bits(batch.cpu().numpy()), bits(want))
    # the variable-ratio path at speed 1 is another filter (its cutoff is quantised): not these bits
    b1, l1, _, _ = gpu.decode_windows_resampled_tensor(streams.data, starts, T_E2E, 16000, speed=[1] * len(starts))
    assert l1.tolist() == lengths.tolist() and not np.array_equal(bits(b1.cpu().numpy()), bits(want))


def test_gapless(gpu, streams, sample_files):
    data = sample_files["classic_lame.mp3"]
    full = streams.full(gpu.OUT_F32_PLANAR)[0]
    info, _ = gpu.lame_parse_reader(data[data.index(b"\xff\xfb"):])
    first, count = info.trim(full.shape[1], 1152)
    assert first > 0 and count < full.shape[1]
    trimmed = full[:, first:first + count]
    speed, gain = [(11, 10), (9, 10), (11, 10)], [1.0, 0.5, 1.0]
    n_y = gpu.VarResampler.out_len(count, *gpu.VarResampler.ratio(44100, 16000, (9, 10)))
    starts = [0, n_y - 400, 0]
    batch, lengths, st, _ = gpu.decode_windows_resampled_tensor([data] * 3, starts, T_E2E, 16000,
                                                                gapless=[True, True, False], speed=speed, gain=gain)
    want_t, len_t = expected_rows(gpu, [trimmed, trimmed], [44100] * 2, 16000, starts[:2], T_E2E, speed[:2], gain[:2])
    want_f, len_f = expected_rows(gpu, [full], [44100], 16000, [0], T_E2E, speed[2:], gain[2:])
    assert lengths.tolist() == [T_E2E, 400, T_E2E] == len_t.tolist() + len_f.tolist()
    got = batch.cpu().numpy()
    assert np.array_equal(bits(got[:2]), bits(want_t)) and np.array_equal(bits(got[2:]), bits(want_f))
    assert not np.array_equal(bits(got[0]), bits(got[2]))


def test_mfcc_of_the_perturbed_batch(gpu, streams):
    """decode_windows_mfcc_tensor(..., speed=, gain=) = MFCC.execute on the perturbed batch."""
    import torch
    T = 4000
    starts = [100] * len(streams.data)
    batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(
        streams.data, starts, T, 16000, out_format=gpu.OUT_F32_MONO, speed=streams.speed, gain=streams.gain)
    mf = gpu.MFCC(16000, device=0)
    want = mf.execute(batch)
    torch.cuda.synchronize()
    feats, flen, st2, rates2 = gpu.decode_windows_mfcc_tensor(streams.data, starts, T, speed=streams.speed,
                                                              gain=streams.gain)
    assert tuple(feats.shape) == (len(starts), mf.frames(T), 13) and rates2.tolist() == rates.tolist()
    assert flen.tolist() == [min(mf.frames(T), max(0, (int(n) - 400) // 160 + 1)) for n in lengths]
    assert np.array_equal(bits(feats.cpu().numpy()), bits(want.cpu().numpy()[:, :mf.frames(T), :13]))
    plain, _, _, _ = gpu.decode_windows_mfcc_tensor(streams.data, starts, T)
    assert not np.array_equal(bits(plain.cpu().numpy()), bits(feats.cpu().numpy()))
    mf.close()


def test_augmented_perturbed_batch(gpu, streams):
    """decode_windows_augmented_tensor(..., speed=, gain=): speed and gain first,
    then reverberation and noise -- augment_host of the perturbed batch."""
    import torch
    rng = np.random.default_rng(31)
    B, T = len(streams.data), 4000
    h = (rng.standard_normal((2, 600)) * np.exp(-np.arange(600) / 100.0)).astype(np.float32)
    h[0, 10] = h[1, 0] = 8.0
    rv = gpu.Reverb(h, [600, 300], 16000, device=0)
    noise = (0.05 * rng.standard_normal((2, 5000))).astype(np.float32)
    starts = [50] * B
    kw = dict(reverb=rv, rir_index=[k % 3 - 1 for k in range(B)], noise_lengths=[5000, 3000],
              additive=dict(index=rng.integers(-1, 2, (B, 1)), snr_db=rng.uniform(0, 15, (B, 1)),
                            start=rng.integers(0, 1000, (B, 1)), offset=rng.integers(0, 2000, (B, 1)),
                            wrap=[[1]] * B))
    batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(streams.data, starts, T, 16000,
                                                                    speed=streams.speed, gain=streams.gain)
    same = gpu.decode_windows_augmented_tensor(streams.data, starts, T, 16000, speed=streams.speed, gain=streams.gain)
    assert len(same) == 4 and np.array_equal(bits(same[0].cpu().numpy()), bits(batch.cpu().numpy()))
    out, lengths2, _, _, stats = gpu.decode_windows_augmented_tensor(
        streams.data, starts, T, 16000, speed=streams.speed, gain=streams.gain,
        noise=torch.from_numpy(noise).cuda(), **kw)
    torch.cuda.synchronize()
    want, want_stats = gpu.augment_host(batch.cpu().numpy(), lengths, noise=noise, **kw)
    assert lengths2.tolist() == lengths.tolist()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), want_stats.view(np.uint64))
    rv.close()


def test_arguments(gpu, streams):
    with pytest.raises(ValueError):
        gpu.decode_windows_resampled_tensor(streams.data[:2], [0, 0], 100, 16000, speed=[1])
    with pytest.raises(gpu.Mp3gError):
        gpu.decode_windows_resampled_tensor(streams.data[:1], [0], 100, 16000, speed=[0])
    with pytest.raises(gpu.Mp3gError) as e:  # 44.1 kHz to 8 Hz: beyond the table's resolution
        gpu.decode_windows_resampled_tensor(streams.data[:1], [0], 100, 8, speed=[1])
    assert e.value.status == 1
    with pytest.raises(gpu.Mp3gError):
        gpu.decode_windows_normalized_tensor(streams.data[:1], [0], 100, speed=[1])
    batch, lengths, _, rates = gpu.decode_windows_resampled_tensor([], [], 100, 16000, speed=[], gain=[])
    assert batch.shape == (0, 2, 100) and len(lengths) == 0 and len(rates) == 0
