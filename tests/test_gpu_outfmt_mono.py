"""Mono downmix output of the one-wave kernels (fast v3, exact v4) on the GPU --
MP3G_OUT_S16_MONO and MP3G_OUT_F32_MONO -- and the format-aware pipelined call
(mp3g_decode_streams_into_out).

The value rules (include/mp3g.h):
  S16_MONO: m = (L + R) >> 1 on the s16 samples MP3G_OUT_S16 of the same plan
            writes (arithmetic shift of the 32-bit sum: floor);
  F32_MONO: m = (fL + fR) * 0.5f on the float samples MP3G_OUT_F32 writes (one
            float32 add rounded to nearest, then the exact halving);
  a mono granule gives channel 0 as it is.
Every check is bit for bit, except the two fast-against-exact bounds that
follow from fast mode's +-1 LSB guarantee: the floors of two sums that differ
by at most 2 differ by at most 1, and |m_fast - m_exact| * 32768 < 2 + 2^-8
(2 per channel, hence for the mean; the two float adds contribute at most
2 * 2^-24 * 32768 ~ 0.004).

Measured on an MI355X (hot-zone batches, every chunking, both counter builds):
max |m_fast - m_exact| * 32768 = 0.0117, max |S16_MONO fast - exact| = 1 (the
test prints both).

The shapes, cases and helpers are those of tests/test_gpu_outfmt.py.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from mp3g import synth
from test_gpu_outfmt import (SENTINEL, SYNTH_CASES, _dev, as_interleaved, is_mono, run_out,  # noqa: F401
                             bitstreams, hot_batch, mono_cases, sixty, switching)

pytestmark = pytest.mark.gpu


def dm16(x):
    """S16_MONO's rule on [..., 2] s16 samples."""
    x = np.asarray(x)
    return ((x[..., 0].astype(np.int32) + x[..., 1].astype(np.int32)) >> 1).astype(np.int16)


def dm32(f):
    """F32_MONO's rule on [..., 2] float32 samples, in float32."""
    f = np.asarray(f, np.float32)
    return ((f[..., 0] + f[..., 1]) * np.float32(0.5)).astype(np.float32)


def as_mono(mp3g, raw, fmt, n):
    """[n, 576] samples of a mono format's raw output."""
    dt = np.int16 if fmt == mp3g.OUT_S16_MONO else np.float32
    return raw.view(dt)[:n * 576].reshape(n, 576)


def downmix_of(mp3g, fmt):
    """(the stereo format a mono format is defined on, its downmix rule)"""
    return (mp3g.OUT_S16, dm16) if fmt == mp3g.OUT_S16_MONO else (mp3g.OUT_F32, dm32)


# ---- 1. exact mode against the oracle -------------------------------------------

def check_exact_mono(gpu, g, c, s, want, what):
    """Both mono formats through decode_host: s16 mono against the oracle's PCM,
    float mono against the downmix of the same plan's OUT_F32 output."""
    m16, _ = gpu.decode_host(g, c, s, out_format=gpu.OUT_S16_MONO)
    assert m16.dtype == np.int16 and m16.shape == (len(g), 576)
    assert np.array_equal(m16, dm16(want)), f"{what}: S16_MONO differs from (L + R) >> 1 of the oracle PCM"
    t = want[..., 0].astype(np.int32) + want[..., 1]
    stereo = ~is_mono(g)
    if stereo.any():
        # a truncating divide (or a rounding one) would show on these
        assert np.any((t < 0) & (t & 1 == 1)), f"{what}: no sample with L + R odd and negative"
    else:
        # (L = R on every mono granule, frame.go:671-678: the sum is even, whatever the seed)
        assert not np.any(t & 1)
        assert np.array_equal(m16, want[..., 0])
    f32, _ = gpu.decode_host(g, c, s, out_format=gpu.OUT_F32)
    m32, _ = gpu.decode_host(g, c, s, out_format=gpu.OUT_F32_MONO)
    assert m32.dtype == np.float32 and m32.shape == (len(g), 576)
    assert m32.tobytes() == dm32(f32).tobytes(), f"{what}: F32_MONO differs from (fL + fR) * 0.5f of OUT_F32"
    assert np.abs(m32).max() <= np.float32(32767.0 / 32768.0)


@pytest.mark.parametrize("name", ["classic_lame.mp3", "mpeg2.mp3"])
def test_exact_mono_sample_files(gpu, captured, name):
    g, c, want = captured[name]
    check_exact_mono(gpu, g, c, None, want, name)


@pytest.mark.parametrize("case", sorted(SYNTH_CASES))
def test_exact_mono_synthetic_branches(gpu, case):
    g, c, s = synth.synth_batch(3, 40, seed=100 + len(case), **SYNTH_CASES[case])
    want, _ = oracle.dsp_streams(g, c, s)
    check_exact_mono(gpu, g, c, s, want, case)


# ---- 2. chunking and state -------------------------------------------------------

@pytest.fixture(scope="module")
def three_streams_mono(gpu):
    """80 granules cut into streams of 7, 40 and 33, at the automatic chunking:
    the two mono outputs, and the state the s16 run exports."""
    g, c, _ = synth.synth_batch(1, 40, seed=31, p_mixed=0.3, p_event=0.1, p_is=0.3)
    s = gpu.streams_for([7, 40, 33], gpu.STATE_OUT)
    raw16, so16 = run_out(gpu, g, c, s, gpu.OUT_S16)
    want, _ = oracle.dsp_streams(g, c, s)
    assert np.array_equal(as_interleaved(gpu, raw16, s, gpu.OUT_S16, len(g)), want)
    ref = {}
    for fmt in (gpu.OUT_S16_MONO, gpu.OUT_F32_MONO):
        raw, so = run_out(gpu, g, c, s, fmt)
        assert so.tobytes() == so16.tobytes()
        ref[fmt] = as_mono(gpu, raw, fmt, len(g)).copy()
    assert np.array_equal(ref[gpu.OUT_S16_MONO], dm16(want))
    return g, c, s, ref, so16


@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 0])
@pytest.mark.parametrize("fmt", ["s16_mono", "f32_mono"])
def test_exact_mono_chunking_and_state(gpu, three_streams_mono, fmt, chunk):
    fmt = {"s16_mono": gpu.OUT_S16_MONO, "f32_mono": gpu.OUT_F32_MONO}[fmt]
    g, c, s, ref, so16 = three_streams_mono
    raw, so = run_out(gpu, g, c, s, fmt, chunk=chunk)
    assert as_mono(gpu, raw, fmt, len(g)).tobytes() == ref[fmt].tobytes(), f"chunk={chunk} differs from chunk=0"
    assert so.tobytes() == so16.tobytes(), f"chunk={chunk}: the exported state depends on the format"


# ---- 3. mono, and mono / stereo switching -----------------------------------------

@pytest.mark.parametrize("chunk", [1, 2, 5, 7, 0])
@pytest.mark.parametrize("fmt", ["s16_mono", "f32_mono"])
@pytest.mark.parametrize("name", ["mono", "switch"])
def test_mono_and_switching(gpu, mono_cases, name, fmt, chunk):
    fmt = {"s16_mono": gpu.OUT_S16_MONO, "f32_mono": gpu.OUT_F32_MONO}[fmt]
    stereo_fmt, dm = downmix_of(gpu, fmt)
    g, c, s, want = mono_cases[name]
    n = len(g)
    raw2, _ = run_out(gpu, g, c, s, stereo_fmt, chunk=chunk)
    two = as_interleaved(gpu, raw2, s, stereo_fmt, n)
    if stereo_fmt == gpu.OUT_S16:
        assert np.array_equal(two, want)
    raw, _ = run_out(gpu, g, c, s, fmt, chunk=chunk)
    out = as_mono(gpu, raw, fmt, n)
    m = is_mono(g)
    assert m.any()
    assert out[m].tobytes() == np.ascontiguousarray(two[m][:, :, 0]).tobytes(), \
        f"{name} chunk={chunk}: mono granules differ from channel 0"
    if name == "switch":
        assert (~m).any()
        assert out[~m].tobytes() == dm(two[~m]).tobytes(), f"{name} chunk={chunk}: stereo granules differ from the downmix"
        assert not np.array_equal(two[~m][:, :, 0], two[~m][:, :, 1])


# ---- 4. fast mode, hot zones included ----------------------------------------------

@pytest.fixture(scope="module")
def hot_mono_exact(gpu, hot_batch):
    """Exact mode's two mono outputs of the hot-granule batch."""
    g, c, s, _ = hot_batch
    out = {}
    for fmt in (gpu.OUT_S16_MONO, gpu.OUT_F32_MONO):
        raw, _ = run_out(gpu, g, c, s, fmt)
        out[fmt] = as_mono(gpu, raw, fmt, len(g)).copy()
    return out


@pytest.mark.parametrize("chunk", [80, 1, 3, 7, 0])
def test_fast_mono(gpu, hot_batch, hot_mono_exact, chunk):
    import torch
    g, c, s, _ = hot_batch
    n = len(g)
    mode = gpu.MODE_FAST | gpu.FLAG_HOT_STATS
    plan_probe = gpu.Plan(s, granules_per_chunk=chunk, mode=mode)
    d_g, d_c = _dev(g), _dev(c)
    d_p = torch.zeros(n * 576, dtype=torch.int16, device="cuda")
    d_so = torch.zeros(len(s) * gpu.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    plan_probe.execute(d_g, d_c, d_p, None, d_so, stream=torch.cuda.current_stream().cuda_stream,
                       out_format=gpu.OUT_S16_MONO)
    torch.cuda.synchronize()
    assert plan_probe.hot_stats()["rewritten"] > 0, "no hot zone: the zone launch wrote nothing"
    plan_probe.close()
    probe = d_p.cpu().numpy().reshape(n, 576)
    raw16, so16 = run_out(gpu, g, c, s, gpu.OUT_S16, chunk=chunk, mode=gpu.MODE_FAST)
    s16 = as_interleaved(gpu, raw16, s, gpu.OUT_S16, n)
    raw32, _ = run_out(gpu, g, c, s, gpu.OUT_F32, chunk=chunk, mode=gpu.MODE_FAST)
    f32 = as_interleaved(gpu, raw32, s, gpu.OUT_F32, n)
    assert np.array_equal(probe, dm16(s16))
    # (both builds of the fast kernel: plain and with the hot counters)
    for md in (gpu.MODE_FAST, mode):
        raw, so = run_out(gpu, g, c, s, gpu.OUT_S16_MONO, chunk=chunk, mode=md)
        m16 = as_mono(gpu, raw, gpu.OUT_S16_MONO, n)
        assert np.array_equal(m16, dm16(s16)), f"chunk={chunk}: S16_MONO differs from (L + R) >> 1 of the fast s16 output"
        assert so.tobytes() == so16.tobytes()
        d16 = int(np.abs(m16.astype(np.int32) - hot_mono_exact[gpu.OUT_S16_MONO]).max())
        assert d16 <= 1, d16
        raw, so = run_out(gpu, g, c, s, gpu.OUT_F32_MONO, chunk=chunk, mode=md)
        m32 = as_mono(gpu, raw, gpu.OUT_F32_MONO, n)
        assert m32.tobytes() == dm32(f32).tobytes(), f"chunk={chunk}: F32_MONO differs from the downmix of the fast F32 output"
        assert so.tobytes() == so16.tobytes()
        d = np.abs((m32.astype(np.float64) - hot_mono_exact[gpu.OUT_F32_MONO].astype(np.float64)) * 32768.0).max()
        print(f"fast vs exact mono, chunk={chunk} mode={md:#x}: max |dm16| = {d16}, max |dm32| * 32768 = {d:.6f}")
        assert d < 2.0 + 2.0 ** -8, d


# ---- 5. no stray writes ------------------------------------------------------------

@pytest.mark.parametrize("chunk", [3, 0])
@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("fmt", [3, 4])
def test_no_stray_writes(gpu, sixty, fmt, mode, chunk):
    """One stream = granules [10, 50) of a 60-slot buffer holding a sentinel,
    compared in 16-bit words (a stray half-dword store must show): nothing
    outside the stream's range changes, nor a guard behind the buffer."""
    g, c = sixty
    s = np.zeros(1, gpu.STREAM_DTYPE)
    s["first_granule"], s["n_granules"], s["flags"] = 10, 40, gpu.STATE_OUT
    guard = 4
    md = gpu.MODE_FAST if mode == "fast" else gpu.MODE_EXACT
    raw, _ = run_out(gpu, g, c, s, fmt, chunk=chunk, mode=md, guard=guard, fill=SENTINEL)
    h = raw.view(np.uint16)
    w = gpu.out_bytes_per_granule(fmt) // 2  # 16-bit words per slot
    assert len(h) == (60 + guard) * w
    before = np.full(len(raw), SENTINEL, np.uint32).view(np.uint16)
    assert np.array_equal(h[:10 * w], before[:10 * w]), "wrote below the stream"
    assert np.array_equal(h[50 * w:60 * w], before[50 * w:60 * w]), "wrote above the stream"
    assert np.array_equal(h[60 * w:], before[60 * w:]), "wrote behind the buffer"
    if fmt == gpu.OUT_F32_MONO:
        inside = raw[10 * w // 2:50 * w // 2]
        assert not np.any(inside == SENTINEL), "a float of the stream's range was not written"
        assert np.all(np.isfinite(inside.view(np.float32)))
    else:
        # every sample of the range is the downmix of the s16 run: all were written
        raw16, _ = run_out(gpu, g, c, s, gpu.OUT_S16, chunk=chunk, mode=md, n_slots=60)
        s16 = raw16.view(np.int16)[:60 * 1152].reshape(60, 576, 2)[10:50]
        assert np.array_equal(h[10 * w:50 * w].view(np.int16).reshape(40, 576), dm16(s16))


# ---- 6. format gating ----------------------------------------------------------------

def test_format_gating(gpu):
    import torch
    g, c, s = synth.synth_batch(1, 4, seed=3)
    for fmt in (gpu.OUT_S16_MONO, gpu.OUT_F32_MONO):
        d_out = torch.zeros(len(g) * 1152, dtype=torch.float32, device="cuda")
        plan = gpu.Plan(s, mode=gpu.FLAG_KERNEL_V2)
        try:
            with pytest.raises(gpu.Mp3gError) as e:
                plan.execute(_dev(g), _dev(c), d_out, stream=torch.cuda.current_stream().cuda_stream, out_format=fmt)
        finally:
            torch.cuda.synchronize()
            plan.close()
        assert e.value.status == 8, fmt
        assert not d_out.cpu().numpy().any()
        with pytest.raises(gpu.Mp3gError) as e:
            gpu.decode_host(g, c, s, mode=gpu.FLAG_KERNEL_V2, out_format=fmt)
        assert e.value.status == 8, fmt


# ---- 7. decode_streams_tensor ---------------------------------------------------------

@pytest.mark.parametrize("fmt", ["s16_mono", "f32_mono"])
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_decode_streams_tensor_mono(gpu, bitstreams, mode, fmt):
    import torch
    datas, refs = bitstreams
    fmt = {"s16_mono": gpu.OUT_S16_MONO, "f32_mono": gpu.OUT_F32_MONO}[fmt]
    m = gpu.MODE_FAST if mode == "fast" else gpu.MODE_EXACT
    want16, wstreams, wst = gpu.decode_streams(datas, mode=m)
    out, views, streams, st = gpu.decode_streams_tensor(datas, mode=m, out_format=fmt)
    dt = torch.int16 if fmt == gpu.OUT_S16_MONO else torch.float32
    assert out.is_cuda and out.dtype == dt and out.dim() == 1
    assert out.numel() == 576 * len(want16)
    assert streams.tobytes() == wstreams.tobytes()
    assert list(st) == list(wst)
    if fmt == gpu.OUT_F32_MONO:
        _, views2, _, _ = gpu.decode_streams_tensor(datas, mode=m, out_format=gpu.OUT_F32)
    for k, v in enumerate(views):
        lo, n = int(streams[k]["first_granule"]), int(streams[k]["n_granules"])
        assert tuple(v.shape) == (n * 576,) and v.is_cuda and v.is_contiguous()
        assert v.data_ptr() == out.data_ptr() + lo * 576 * out.element_size()  # a slice of out
        got = v.cpu().numpy()
        if fmt == gpu.OUT_S16_MONO:
            if mode == "exact":
                assert np.array_equal(got, dm16(refs[k])), f"stream {k}: differs from the oracle's downmix"
            assert np.array_equal(got, dm16(want16[lo:lo + n].reshape(n * 576, 2))), f"stream {k} vs decode_streams"
        else:
            assert got.tobytes() == dm32(views2[k].cpu().numpy()).tobytes(), f"stream {k} vs the OUT_F32 tensor"


# ---- 8. decode_streams_into with a format ----------------------------------------------

@pytest.fixture(scope="module")
def into_case(gpu, bitstreams, sample_files):
    """The six bitstreams, a seventh truncated mid-file, and an eighth whose
    side info ends it early (its range keeps an unused tail: the pre-pass
    counts headers); per format, what decode_streams_tensor gives each stream."""
    from test_scan_cpu import _mpeg2_mixed_block
    datas = list(bitstreams[0])
    cut = sample_files["classic_lame.mp3"]
    datas.append(cut[:len(cut) // 2 + 100])
    datas.append(_mpeg2_mixed_block(sample_files["mpeg2.mp3"]))
    ref = {}
    for fmt in range(5):
        _, views, streams, st = gpu.decode_streams_tensor(datas, mode=gpu.MODE_EXACT, out_format=fmt)
        ref[fmt] = ([v.cpu().numpy().reshape(-1) for v in views], streams, list(st))
    return datas, ref


def _np_dtype(gpu, fmt):
    return np.int16 if fmt in (gpu.OUT_S16, gpu.OUT_S16_MONO) else np.float32


def _into_buffer(gpu, kind, fmt, slots, fill):
    import torch
    dt = _np_dtype(gpu, fmt)
    per = gpu.out_bytes_per_granule(fmt) // np.dtype(dt).itemsize
    if kind == "numpy":
        buf = np.full(slots * per, fill, dt)
        return buf, buf
    t = torch.full((slots * per,), fill, dtype=torch.int16 if dt == np.int16 else torch.float32).pin_memory()
    return t, t.numpy()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("n_groups", [0, 3])
@pytest.mark.parametrize("kind", ["numpy", "pinned"])
def test_decode_streams_into_formats(gpu, into_case, kind, n_groups, fmt):
    datas, ref = into_case
    want, wstreams, wst = ref[fmt]
    per = gpu.out_bytes_per_granule(fmt) // np.dtype(_np_dtype(gpu, fmt)).itemsize  # samples per granule slot
    # the capacity: one slot too few returns 1 with the need and writes nothing
    need = C.c_uint64()
    bufs, ptrs, lens = gpu._stream_args(datas)
    streams = np.zeros(len(datas), gpu.STREAM_DTYPE)
    status = np.zeros(len(datas), np.int32)
    probe, probe_np = _into_buffer(gpu, kind, fmt, 8, 77)
    rc = gpu.lib().mp3g_decode_streams_into_out(0, len(datas), ptrs, lens, 0, gpu.MODE_EXACT, n_groups,
                                                C.c_void_p(probe_np.ctypes.data), fmt, 8, C.byref(need),
                                                streams.ctypes.data, status.ctypes.data)
    total = need.value
    assert rc == 1 and total > sum(int(x) for x in wstreams["n_granules"])  # (the eighth stream's unused tail)
    assert np.all(probe_np == 77), "a too-small buffer was written"
    guard = 2
    out, out_np = _into_buffer(gpu, kind, fmt, total + guard, 77)
    n, s, st = gpu.decode_streams_into(datas, out[:total * per], mode=gpu.MODE_EXACT, n_groups=n_groups, out_format=fmt)
    assert n == total and st.tolist() == wst
    assert s["n_granules"].tolist() == wstreams["n_granules"].tolist()
    assert np.all(out_np[total * per:] == 77), "wrote behind the buffer"
    tails = 0
    for k in range(len(datas)):
        lo, m = int(s[k]["first_granule"]), int(s[k]["n_granules"])
        hi = int(s[k + 1]["first_granule"]) if k + 1 < len(datas) else total
        assert out_np[lo * per:(lo + m) * per].tobytes() == want[k].tobytes(), f"stream {k} vs decode_streams_tensor"
        assert not out_np[(lo + m) * per:hi * per].any(), f"stream {k}: the rest of its range is not zero"
        tails += hi - lo - m
    assert tails > 0
    if fmt == gpu.OUT_S16:  # byte-identical to the old entry point
        old, old_np = _into_buffer(gpu, kind, fmt, total + guard, 77)
        n2 = C.c_uint64()
        rc = gpu.lib().mp3g_decode_streams_into(0, len(datas), ptrs, lens, 0, gpu.MODE_EXACT, n_groups,
                                                C.c_void_p(old_np.ctypes.data), total, C.byref(n2),
                                                streams.ctypes.data, status.ctypes.data)
        assert rc == 0 and n2.value == total
        assert old_np.tobytes() == out_np.tobytes()
        assert streams.tobytes() == s.tobytes()
