"""Sample-windowed decode into dense rows on the GPU (include/mp3g.h
"sample-windowed decode").

The reference of every test is the full decode of the same stream in the same
mode and format (mp3g.decode_streams_tensor, or a plain plan over the full
scan): a window's samples are the same bits, and nothing else is written.
"""
import numpy as np
import pytest

from mp3g import synth
from test_gpu_outfmt import q
from windows_ref import layout, switching_lsf_stream, switching_stream

pytestmark = pytest.mark.gpu

SKIPS = (0, 1, 31, 32, 33, 63, 64, 575)  # the planar store's 32-sample runs, the mono layout's 64-sample stores
T_VALUES = (1, 575, 576, 577, 1153, 3000)
SENTINEL = 0x7FC0DEAD  # a NaN payload no decode produces

STREAMS = {
    "joint": lambda sf: synth.encode_stream(101, 50),
    "mixed+is": lambda sf: synth.encode_stream(102, 50, p_mixed=0.3, p_event=0.1, p_is=0.5),
    "mono": lambda sf: synth.encode_stream(103, 50, mode=synth.MODE_MONO),
    "mpeg2": lambda sf: synth.encode_stream(104, 60, lsf=True, p_event=0.1),
    "mpeg2-mono": lambda sf: synth.encode_stream(105, 60, lsf=True, mode=synth.MODE_MONO),
    "reservoir-full": lambda sf: synth.encode_stream(1, 50, fill=1.3),
    "switching": lambda sf: switching_stream(),
    "switching-lsf": lambda sf: switching_lsf_stream(),
    "classic_lame.mp3": lambda sf: sf["classic_lame.mp3"],
    "mpeg2.mp3": lambda sf: sf["mpeg2.mp3"],
}


@pytest.fixture(scope="module")
def refs(gpu, sample_files):
    """Per stream: its bytes and, on demand, the full decode per (mode, format) as numpy -- computed once."""
    class Refs:
        def __init__(self):
            self.data = {k: f(sample_files) for k, f in STREAMS.items()}
            self.cache = {}

        def full(self, name, mode=0, fmt=2):
            key = (name, mode, fmt)
            if key not in self.cache:
                _, views, streams, st = gpu.decode_streams_tensor([self.data[name]], mode=mode, out_format=fmt)
                assert st[0] == 7 and streams[0]["n_granules"] > 0
                a = views[0].cpu().numpy().copy()
                a.setflags(write=False)
                self.cache[key] = a
            return self.cache[key]
    return Refs()


def window_starts(N, T):
    """<= 16 starts: every skip of SKIPS, lead 0 / 1 / 2, the stream's end met exactly, overrun and missed."""
    los = (0, 0, 1, 1, 2, 3, 5, 9)
    starts = [576 * lo + sk for lo, sk in zip(los, SKIPS)] + [575, 576, N // 2 + 64, max(N - T, 0),
                                                               max(N - T // 2 - 1, 0), N, N + 5]
    assert {s % 576 for s in starts} >= set(SKIPS) and {min(s // 576, 2) for s in starts} == {0, 1, 2}
    return starts


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_rows(batch, lengths, full, starts, T, what):
    """Every row: its valid samples are the full decode's bits, the rest is zero."""
    N = full.shape[-1]
    batch = batch.cpu().numpy()
    for k, start in enumerate(starts):
        n = max(0, min(T, N - start))
        assert int(lengths[k]) == n, (what, start, T, lengths[k], n)
        row = batch[k]
        assert np.array_equal(bits(row[..., :n]), bits(full[..., start:start + n])), (what, start, T)
        assert not bits(row[..., n:]).any(), (what, start, T)


# ---- 1. exact mode, bit for bit ---------------------------------------------------

@pytest.mark.parametrize("name", sorted(STREAMS))
def test_exact_bit_for_bit(gpu, refs, name):
    full = refs.full(name)
    N = full.shape[1]
    for T in T_VALUES:
        starts = window_starts(N, T)
        batch, lengths, st = gpu.decode_windows_tensor([refs.data[name]] * len(starts), starts, T)
        assert batch.shape == (len(starts), 2, T)
        check_rows(batch, lengths, full, starts, T, name)
        for k, start in enumerate(starts):
            assert st[k] == (7 if start + T > N else 0), (name, start, T, st[k])


def test_batch_of_different_streams(gpu, refs):
    """One call, a different stream and start per row."""
    names = sorted(STREAMS)
    T = 3000
    starts = [(577 * (3 + 5 * i)) % (refs.full(n).shape[1] - 1000) for i, n in enumerate(names)]
    batch, lengths, st = gpu.decode_windows_tensor([refs.data[n] for n in names], starts, T, n_threads=3)
    for k, n in enumerate(names):
        check_rows(batch[k:k + 1], lengths[k:k + 1], refs.full(n), starts[k:k + 1], T, n)


# ---- plan-level runs ----------------------------------------------------------------

class Windows:
    """A windowed scan on the device (main data decoded), to run plans over."""

    def __init__(self, mp3g, datas, starts, T, patch=None):
        import torch
        self.m, self.T, self.B = mp3g, T, len(datas)
        s = mp3g.scan_windows(datas, starts, T)
        self.rows, self.streams = s["rows"], s["streams"]
        n = len(s["granules"])
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
        self.d_g, d_j, d_m = dev(s["granules"]), dev(s["jobs"]), dev(s["main_data"])
        self.d_c = torch.empty(n * 1152, dtype=torch.int16, device="cuda")
        mp3g.huffman_execute(d_j, n, d_m, self.d_g, self.d_c, stream=torch.cuda.current_stream().cuda_stream,
                             flags=mp3g.HUFF_ROWS_COUNT1)
        torch.cuda.synchronize()
        if patch is not None:  # descriptors changed on the host after the main-data kernel completed them
            g = self.d_g.cpu().numpy().view(mp3g.GRANULE_DTYPE).copy()
            patch(g, self.streams, self.rows)
            self.d_g = dev(g)

    def run(self, fmt, mode=0, chunk=0, guard_rows=1):
        """(words uint32 [guard + B + guard, planes, T], hot_stats) with the sentinel wherever nothing was written."""
        import torch
        m = self.m
        planes = 2 if fmt == m.OUT_F32_PLANAR else 1
        buf = torch.full(((self.B + 2 * guard_rows) * planes * self.T,), SENTINEL, dtype=torch.int32, device="cuda")
        plan = m.WindowPlan(self.streams, self.rows, self.T, granules_per_chunk=chunk, mode=mode)
        try:
            info = plan.info()
            assert info["halo_granules"] >= int(self.rows["lead"][self.streams["n_granules"] > 0].sum())
            plan.execute(self.d_g, self.d_c, buf[guard_rows * planes * self.T:],
                         stream=torch.cuda.current_stream().cuda_stream, out_format=fmt)
            torch.cuda.synchronize()
            hs = plan.hot_stats() if mode & m.FLAG_HOT_STATS else None
        finally:
            plan.close()
        return buf.cpu().numpy().view(np.uint32).reshape(self.B + 2 * guard_rows, planes, self.T), hs


def full_plan_run(mp3g, data, fmt, mode, patch=None):
    """The full decode of one stream through a plain plan, with the same descriptor patch: [planes, N] float32."""
    import torch
    s = mp3g.scan_streams([data])
    n = len(s["granules"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    d_g, d_j, d_m = dev(s["granules"]), dev(s["jobs"]), dev(s["main_data"])
    d_c = torch.empty(n * 1152, dtype=torch.int16, device="cuda")
    mp3g.huffman_execute(d_j, n, d_m, d_g, d_c, stream=torch.cuda.current_stream().cuda_stream,
                         flags=mp3g.HUFF_ROWS_COUNT1)
    torch.cuda.synchronize()
    if patch is not None:
        g = d_g.cpu().numpy().view(mp3g.GRANULE_DTYPE).copy()
        patch(g)
        d_g = dev(g)
    planes = 2 if fmt == mp3g.OUT_F32_PLANAR else 1
    out = torch.zeros(n * 576 * planes, dtype=torch.float32, device="cuda")
    plan = mp3g.Plan(s["streams"], mode=mode)
    try:
        plan.execute(d_g, d_c, out, stream=torch.cuda.current_stream().cuda_stream, out_format=fmt)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return out.cpu().numpy().reshape(planes, n * 576)


def check_words(words, rows, full, starts, what, guard_rows=1):
    """The valid samples are the full decode's bits; every other word -- the tail
    of plane 0, the head of plane 1, the neighbouring rows, the guard rows --
    still holds the sentinel."""
    B = len(starts)
    assert (words[:guard_rows] == SENTINEL).all() and (words[guard_rows + B:] == SENTINEL).all(), what
    N = full.shape[-1]
    for k, start in enumerate(starts):
        n = int(rows["n_valid"][k])
        assert n == max(0, min(words.shape[2], N - start)), (what, k)
        row = words[guard_rows + k]
        assert np.array_equal(row[:, :n], np.ascontiguousarray(full[:, start:start + n]).view(np.uint32)), (what, k, start)
        assert (row[:, n:] == SENTINEL).all(), (what, k, start)


# ---- 2. nothing else is written -----------------------------------------------------

@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("fmt", ["planar", "mono"])
@pytest.mark.parametrize("name", ["joint", "switching", "mpeg2-mono"])
def test_nothing_else_is_written(gpu, refs, name, fmt, mode):
    fmt = {"planar": gpu.OUT_F32_PLANAR, "mono": gpu.OUT_F32_MONO}[fmt]
    m = gpu.MODE_FAST if mode == "fast" else gpu.MODE_EXACT
    full = refs.full(name, m, fmt).reshape(-1, refs.full(name, m, fmt).shape[-1])
    N = full.shape[1]
    for T in (1, 577, 1153):
        starts = window_starts(N, T)
        w = Windows(gpu, [refs.data[name]] * len(starts), starts, T)
        words, _ = w.run(fmt, m)
        check_words(words, w.rows, full, starts, (name, T))


# ---- 3. chunkings -------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_chunkings(gpu, refs, mode):
    m = gpu.MODE_FAST if mode == "fast" else gpu.MODE_EXACT
    for name in ("mixed+is", "switching"):
        full = refs.full(name, m)
        N = full.shape[1]
        T = 3000
        starts = window_starts(N, T)
        w = Windows(gpu, [refs.data[name]] * len(starts), starts, T)
        first = None
        for chunk in (1, 2, 3, 7, 0):
            words, _ = w.run(gpu.OUT_F32_PLANAR, m, chunk=chunk)
            if first is None:
                first = words
                check_words(words, w.rows, full, starts, (name, chunk))
            assert np.array_equal(words, first), (name, chunk)


# ---- 4. mono downmix ----------------------------------------------------------------

@pytest.mark.parametrize("name", ["joint", "switching", "switching-lsf", "mono", "classic_lame.mp3"])
def test_mono(gpu, refs, name):
    full = refs.full(name, 0, gpu.OUT_F32_MONO)
    N = full.shape[0]
    for T in (1, 576, 577, 3000):
        starts = window_starts(N, T)
        batch, lengths, _ = gpu.decode_windows_tensor([refs.data[name]] * len(starts), starts, T,
                                                      out_format=gpu.OUT_F32_MONO)
        assert batch.shape == (len(starts), T)
        check_rows(batch, lengths, full, starts, T, name)


# ---- 5. fast mode -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["joint", "mixed+is", "switching", "mpeg2", "reservoir-full"])
def test_fast_ordinary(gpu, refs, name):
    full = refs.full(name, gpu.MODE_FAST)
    exact = refs.full(name)
    assert np.abs(q(full).astype(np.int32) - q(exact).astype(np.int32)).max() <= 1
    N = full.shape[1]
    for T in (577, 3000):
        starts = window_starts(N, T)
        for mode in (gpu.MODE_FAST, gpu.MODE_FAST | gpu.FLAG_HOT_STATS):
            batch, lengths, _ = gpu.decode_windows_tensor([refs.data[name]] * len(starts), starts, T, mode=mode)
            check_rows(batch, lengths, full, starts, T, name)


def _boost(g, idx, boost=56):
    """synth.loud_granules' boost on the granules `idx`."""
    gg = g["ch"]["global_gain"].astype(np.int32)
    gg[idx] = np.minimum(gg[idx] + boost, 255)
    g["ch"]["global_gain"] = gg.astype(np.uint8)


@pytest.mark.parametrize("name", ["joint", "switching"])
def test_fast_loud_granules(gpu, refs, name):
    """Loud granules (boost 56: far over the hot bounds) in the lead-in, at
    the window's first granule and at its last: the zone reaches the output
    range from a hot granule in the halo too."""
    data = refs.data[name]
    G = len(gpu.scan_streams([data])["granules"])
    N = 576 * G
    T = 3000
    los = [4, 9, 14, 20, 27, 33]
    starts = [576 * lo + sk for lo, sk in zip(los, (0, 1, 33, 64, 575, 300))]
    hot = set()
    for i, start in enumerate(starts):
        lo, hi = start // 576, -(-(start + T) // 576)
        hot.add((lo - 1, lo - 2, lo, hi - 1, lo - 1, hi - 1)[i])
    hot = sorted(hot)
    hdr = gpu.scan_streams([data])["granules"]["header"]

    def patch_full(g):
        _boost(g, hot)

    def patch_win(g, streams, rows):
        for k, start in enumerate(starts):
            h, n, *_ = layout(hdr, start, T)
            f = int(streams[k]["first_granule"])
            _boost(g, [f + x - h for x in hot if h <= x < h + n])

    full = full_plan_run(gpu, data, gpu.OUT_F32_PLANAR, gpu.MODE_FAST, patch_full)
    exact = full_plan_run(gpu, data, gpu.OUT_F32_PLANAR, gpu.MODE_EXACT, patch_full)
    d = np.abs(q(full).astype(np.int32) - q(exact).astype(np.int32)).max()
    print(f"{name}: fast vs exact full decode with loud granules, max |dPCM| = {d}")
    assert d <= 1
    w = Windows(gpu, [data] * len(starts), starts, T, patch=patch_win)
    for mode in (gpu.MODE_FAST, gpu.MODE_FAST | gpu.FLAG_HOT_STATS):
        for chunk in (0, 2):
            words, hs = w.run(gpu.OUT_F32_PLANAR, mode, chunk=chunk)
            check_words(words, w.rows, full, starts, (name, mode, chunk))
            if hs is not None:
                print(f"{name}: chunk {chunk}: hot_stats {hs}")
                assert hs["zones"] >= len(starts) and hs["rewritten"] >= len(starts), hs
    # the exact windowed decode of the same descriptors: within 1 LSB after the s16 quantisation
    xw, _ = w.run(gpu.OUT_F32_PLANAR, gpu.MODE_EXACT)
    check_words(xw, w.rows, exact, starts, (name, "exact"))
    mono_full = full_plan_run(gpu, data, gpu.OUT_F32_MONO, gpu.MODE_FAST, patch_full)
    words, _ = w.run(gpu.OUT_F32_MONO, gpu.MODE_FAST)
    check_words(words, w.rows, mono_full, starts, (name, "mono"))


# ---- 6. gapless, end to end ---------------------------------------------------------

def test_gapless_end_to_end(gpu, refs, sample_files):
    data = sample_files["classic_lame.mp3"]
    full = refs.full("classic_lame.mp3")
    info, _ = gpu.lame_parse_reader(data[data.index(b"\xff\xfb"):])
    first, count = info.trim(full.shape[1], 1152)
    T = 4000
    batch, lengths, st = gpu.decode_windows_tensor([data, data, data], [0, count - 1000, 0], T,
                                                   gapless=[True, True, False])
    b = batch.cpu().numpy()
    assert list(lengths) == [T, 1000, T] and list(st) == [0, 7, 0]
    assert np.array_equal(bits(b[0]), bits(full[:, first:first + T]))
    assert np.array_equal(bits(b[1][:, :1000]), bits(full[:, first + count - 1000:first + count]))
    assert not bits(b[1][:, 1000:]).any()
    assert np.array_equal(bits(b[2]), bits(full[:, :T]))
