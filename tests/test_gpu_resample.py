"""The resampler on the GPU (include/mp3g.h "sample-rate conversion of decoded
rows"): mp3g_resample_rows against mp3g_resample_host
bit for bit, nothing else written, and decode_windows_resampled_tensor against
the host reference applied to the full decode."""
import numpy as np
import pytest

import spec_resample as spec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no resample produces
GUARD = 1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def launch_rows(r, kind, C, rng):
    """Eight rows for one launch: every n_out of the list, one kind of out_start.
    Returns (rows, src [8, C, S] float32, out_stride)."""
    tile, L, M, W = r.tile, r.L, r.M, r.W
    n_outs = [1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5]
    span = max(W * L // M, 1)  # outputs the filter's half width covers
    rows = np.zeros(8, r_dtype())
    for i, n in enumerate(n_outs):
        if kind in (0, 1, 2, 3, 4):  # 0, 1, L - 1, L, 2: the first taps fall before sample 0
            s = (0, 1, L - 1, L, 2)[kind]
            a, b = r.src_window(s, n)
            origin, n_src = 0, max(1, b - 7 * i)  # (i > 0: the window also runs over the source's end)
        elif kind == 5:  # the window runs over the source's end
            origin, n_src = 0, 700 + 37 * i
            s = max(0, r.out_len(n_src) - n // 2 - 1)
        elif kind == 6:  # past the source's end: n_out = 0, or zeros
            origin, n_src = 0, 300 + i
            s = r.out_len(n_src) + 2 * span + 5 + i
            n = 0 if i % 2 == 0 else n
        else:  # far out, a short source at the matching origin
            s = 2 ** 33 + 7
            a, b = r.src_window(s, n)
            origin, n_src = a + 2 * i, max(1, b - a - 5 * i)
        rows[i] = (s, origin, (3 * i + 1) % 8, (5 * i + 2) % 8, n_src, n)
    S = int(rows["n_src"].max()) + 3
    src = rng.uniform(-1.0, 1.0, (8, C, S)).astype(np.float32)
    src[3] *= np.float32(2.0 ** -120)  # subnormal products
    return rows, src, max(n_outs) + 11


def r_dtype():
    import mp3g
    return mp3g.RESAMPLE_ROW_DTYPE


# The MP3 pairs run the phase-grouped kernel.  The others reach the generic kernel's four builds: (48000, 8000) a
# staged span and a table in LDS, (44100, 70000) L = 700 > 512 and a table in global memory, (48000, 1000) and
# (48000, 1002) spans beyond the LDS stage, the table in LDS / in global memory.
CASES = [(fi, fo, 4) for fi, fo in spec.PAIRS] + [(44100, 44100, 4), (44100, 16000, 16), (44100, 16000, 64),
                                                  (48000, 8000, 4), (44100, 70000, 4), (48000, 1000, 4),
                                                  (48000, 1002, 4)]


@pytest.mark.parametrize("fi,fo,zeros", CASES)
def test_kernel_equals_host_reference_and_writes_nothing_else(gpu, fi, fo, zeros):
    """uint32 views: every row's n_out samples per plane are mp3g_resample_host's
    bits; every other word of the output -- row tails, untouched rows, the
    guard rows on both sides -- keeps its sentinel."""
    import torch
    rolloff, beta = (spec.FAST if zeros < 64 else spec.BEST)[1:]
    r = gpu.Resampler(fi, fo, zeros, rolloff, beta, device=0)
    assert r.tile >= 64
    rng = np.random.default_rng(fi + fo + zeros)
    kinds = range(8) if zeros == 4 else (0, 5, 7)
    for C in (1, 2):
        for kind in kinds:
            rows, src, T = launch_rows(r, kind, C, rng)
            d_src = torch.from_numpy(src).cuda()
            buf = torch.full((8 + 2 * GUARD, C, T), SENTINEL, dtype=torch.int32, device="cuda")
            r.rows(d_src, buf[GUARD:GUARD + 8].view(torch.float32), rows)
            torch.cuda.synchronize()
            got = buf.cpu().numpy().view(np.uint32)
            want = np.full(got.shape, SENTINEL, np.uint32)
            for row in rows:
                n = int(row["n_out"])
                for ch in range(C):
                    x = src[row["src_row"], ch, :row["n_src"]]
                    want[GUARD + row["out_row"], ch, :n] = bits(r.host(x, int(row["src_origin"]), int(row["out_start"]), n))
            bad = np.argwhere(got != want)
            assert not len(bad), (fi, fo, zeros, C, kind, bad[:4].tolist(), rows)
            # (the rows are not all zero: the comparison is not vacuous)
            assert kind == 6 or (want != SENTINEL).sum() > 1000
    r.close()


def test_single_channel_2d_tensors_and_many_rows(gpu):
    """[*, S] tensors are one plane per row; more rows (32,768 + 9) than one launch takes."""
    import torch
    r = gpu.Resampler(24000, 16000, 4, device=0)
    rng = np.random.default_rng(3)
    n_rows, S, T = 32768 + 9, 24, 6
    src = rng.uniform(-1, 1, (n_rows, S)).astype(np.float32)
    rows = np.zeros(n_rows, gpu.RESAMPLE_ROW_DTYPE)
    i = np.arange(n_rows)
    rows["out_start"], rows["src_row"], rows["out_row"] = i % 11, i, n_rows - 1 - i
    rows["n_src"], rows["n_out"] = S - i % 5, 1 + (i * 7) % T
    out = torch.full((n_rows, T), SENTINEL, dtype=torch.int32, device="cuda")
    r.rows(torch.from_numpy(src).cuda(), out.view(torch.float32), rows)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    for row in rows:
        n = int(row["n_out"])
        assert np.array_equal(got[row["out_row"], :n], bits(r.host(src[row["src_row"], :row["n_src"]], 0,
                                                                   int(row["out_start"]), n)))
        assert (got[row["out_row"], n:] == SENTINEL).all()
    rows["n_out"][0] = T + 1  # a row longer than the output's rows is refused by the binding
    with pytest.raises(ValueError):
        r.rows(torch.from_numpy(src).cuda(), out.view(torch.float32), rows)


# ---- end to end -----------------------------------------------------------------------

T_E2E = 1500


@pytest.fixture(scope="module")
def streams(gpu, sample_files):
    """The two sample files, 40-frame synthetic streams at all six sample rates
    and a stream without a frame; per (mode, format) their full decodes as numpy."""
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
            self.cache = {}

        def full(self, mode, fmt):
            if (mode, fmt) not in self.cache:
                _, views, _, _ = gpu.decode_streams_tensor(self.data, mode=mode, out_format=fmt)
                vs = [v.cpu().numpy().copy() for v in views]
                for v in vs:
                    v.setflags(write=False)
                self.cache[(mode, fmt)] = vs
            return self.cache[(mode, fmt)]
    return S()


def expected_rows(mp3g, views, rates, rate, starts, T, quality=spec.FAST):
    """(rows [B, planes, T], lengths) from Resampler.host on each stream's full view."""
    planes = views[0].shape[0] if views[0].ndim == 2 else 1
    want = np.zeros((len(views), planes, T), np.float32)
    lengths = np.zeros(len(views), np.int64)
    for k, (v, f) in enumerate(zip(views, rates)):
        v = v.reshape(planes, -1)
        if not f:
            continue
        r = mp3g.Resampler(f, rate, *quality)
        n = max(0, min(T, r.out_len(v.shape[1]) - starts[k]))
        lengths[k] = n
        for ch in range(planes):
            want[k, ch, :n] = r.host(v[ch], 0, starts[k], n)
    return want, lengths


def start_sets(mp3g, views, rates, rate, T):
    """Five starts per stream, at the target rate: 0, mid-stream, ending exactly
    at the stream's end, running past it, starting past it."""
    sets = [[], [], [], [], []]
    for v, f in zip(views, rates):
        n_y = mp3g.Resampler(f, rate, 4).out_len(v.shape[-1]) if f else 0
        for s, val in zip(sets, (0, n_y // 2 + 13, max(0, n_y - T), max(0, n_y - T // 2), n_y + 5)):
            s.append(val)
    return sets


@pytest.mark.parametrize("fmt", ["planar", "mono"])
@pytest.mark.parametrize("rate", [16000, 44100])
def test_end_to_end_exact(gpu, streams, rate, fmt):
    fmt = {"planar": gpu.OUT_F32_PLANAR, "mono": gpu.OUT_F32_MONO}[fmt]
    views = streams.full(gpu.MODE_EXACT, fmt)
    T = T_E2E
    for i, starts in enumerate(start_sets(gpu, views, streams.rates, rate, T)):
        batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(streams.data, starts, T, rate, out_format=fmt,
                                                                        n_threads=4)
        assert rates.tolist() == streams.rates
        want, want_len = expected_rows(gpu, views, streams.rates, rate, starts, T)
        assert lengths.tolist() == want_len.tolist(), (rate, starts)
        got = batch.cpu().numpy().reshape(want.shape)
        assert np.array_equal(bits(got), bits(want)), (rate, starts, np.argwhere(bits(got) != bits(want))[:4].tolist())
        # (not vacuous: sets 0-2 fill their rows, set 3 runs past the end, set 4 starts past it)
        assert lengths.max() == (T, T, T, T // 2, 0)[i] and bool(want.any()) == (i < 4), (i, lengths)


def test_end_to_end_best_quality(gpu, streams):
    views = streams.full(gpu.MODE_EXACT, gpu.OUT_F32_PLANAR)
    starts = start_sets(gpu, views, streams.rates, 16000, T_E2E)[3]
    batch, lengths, _, _ = gpu.decode_windows_resampled_tensor(streams.data, starts, T_E2E, 16000, quality="best")
    want, want_len = expected_rows(gpu, views, streams.rates, 16000, starts, T_E2E, spec.BEST)
    assert lengths.tolist() == want_len.tolist()
    assert np.array_equal(bits(batch.cpu().numpy()), bits(want))


def test_streams_already_at_the_rate_equal_the_windowed_decode(gpu, streams):
    idx = [k for k, f in enumerate(streams.rates) if f == 44100]
    assert len(idx) >= 2
    datas = [streams.data[k] for k in idx]
    N = [streams.full(gpu.MODE_EXACT, gpu.OUT_F32_PLANAR)[k].shape[1] for k in idx]
    for starts in ([0] * len(idx), [n - 700 for n in N], [n + 3 for n in N]):
        for fmt in (gpu.OUT_F32_PLANAR, gpu.OUT_F32_MONO):
            a, la, sa, rates = gpu.decode_windows_resampled_tensor(datas, starts, T_E2E, 44100, out_format=fmt)
            b, lb, sb = gpu.decode_windows_tensor(datas, starts, T_E2E, out_format=fmt)
            assert a.shape == b.shape and np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy()))
            assert la.tolist() == lb.tolist() and sa.tolist() == sb.tolist() and set(rates.tolist()) == {44100}


def test_gapless(gpu, streams, sample_files):
    data = sample_files["classic_lame.mp3"]
    full = streams.full(gpu.MODE_EXACT, gpu.OUT_F32_PLANAR)[0]
    info, _ = gpu.lame_parse_reader(data[data.index(b"\xff\xfb"):])
    first, count = info.trim(full.shape[1], 1152)
    assert first > 0 and count < full.shape[1]
    trimmed = full[:, first:first + count]
    r = gpu.Resampler(44100, 16000)
    n_y = r.out_len(count)
    starts = [0, n_y - 400, 0]
    batch, lengths, st, _ = gpu.decode_windows_resampled_tensor([data] * 3, starts, T_E2E, 16000,
                                                                gapless=[True, True, False])
    want_t, len_t = expected_rows(gpu, [trimmed, trimmed], [44100] * 2, 16000, starts[:2], T_E2E)
    want_f, len_f = expected_rows(gpu, [full], [44100], 16000, [0], T_E2E)
    assert lengths.tolist() == [T_E2E, 400, T_E2E] == len_t.tolist() + len_f.tolist()
    got = batch.cpu().numpy()
    assert np.array_equal(bits(got[:2]), bits(want_t)) and np.array_equal(bits(got[2:]), bits(want_f))
    assert not np.array_equal(bits(got[0]), bits(got[2]))


def test_fast_mode(gpu, streams):
    """The same identity against the fast-mode full decode: the resampler adds nothing mode-dependent."""
    views = streams.full(gpu.MODE_FAST, gpu.OUT_F32_PLANAR)
    starts = start_sets(gpu, views, streams.rates, 16000, T_E2E)[1]
    batch, lengths, _, _ = gpu.decode_windows_resampled_tensor(streams.data, starts, T_E2E, 16000, mode=gpu.MODE_FAST)
    want, want_len = expected_rows(gpu, views, streams.rates, 16000, starts, T_E2E)
    assert lengths.tolist() == want_len.tolist()
    assert np.array_equal(bits(batch.cpu().numpy()), bits(want))


def test_formats_and_arguments(gpu, streams):
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_resampled_tensor(streams.data[:1], [0], 100, 16000, out_format=gpu.OUT_S16)
    assert e.value.status == 8
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_resampled_tensor(streams.data[:1], [0], 100, 16000, out_format=77)
    assert e.value.status == 1
    with pytest.raises(gpu.Mp3gError):
        gpu.decode_windows_resampled_tensor(streams.data[:1], [0], 100, 0)
    batch, lengths, _, rates = gpu.decode_windows_resampled_tensor([], [], 100, 16000)
    assert batch.shape == (0, 2, 100) and len(lengths) == 0 and len(rates) == 0
