"""Float32 PCM output of the one-wave kernels (fast v3, exact v4) on the GPU:
MP3G_OUT_F32 (interleaved) and MP3G_OUT_F32_PLANAR against the s16 output of
the same plan and the oracle.

The value rule (include/mp3g.h): f = clamp(sum * 32767, +-32767) * 2^-15, the
s16 sample's clamp without its truncation, so q(f) = trunc(f * 32768) IS the
s16 sample -- every check below is bit for bit, except the one bound that
follows from it: fast mode is within 1 LSB of exact mode in s16 (the existing
guarantee), hence |f_fast - f_exact| * 32768 < 2 in float.
"""
import numpy as np
import pytest

import oracle
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7fc0dead  # a NaN payload no kernel arithmetic produces


def q(f):
    """The s16 sample of a float sample (frame.go:663-669's truncation)."""
    return np.trunc(np.asarray(f, np.float32) * np.float32(32768)).astype(np.int16)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def run_out(mp3g, g, c, streams, fmt, chunk=0, mode=0, n_slots=None, guard=0, fill=None):
    """Plan.execute(out_format=fmt) on torch buffers: (raw output as uint32 /
    int16 words incl. guard, state_out).  n_slots: granule slots of the output
    buffer (default: len(g)); guard: extra slots behind it; fill: a 32-bit
    pattern the whole buffer holds before the launch."""
    import torch
    n = len(g) if n_slots is None else n_slots
    bpg = mp3g.out_bytes_per_granule(fmt)
    d_g, d_c = _dev(g), _dev(c)
    words = (n + guard) * bpg // 4
    d_out = torch.from_numpy(np.full(words, 0 if fill is None else fill, np.uint32).view(np.int32)).cuda()
    d_so = torch.zeros(len(streams) * mp3g.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    plan = mp3g.Plan(streams, granules_per_chunk=chunk, mode=mode)
    plan.execute(d_g, d_c, d_out, None, d_so, stream=torch.cuda.current_stream().cuda_stream, out_format=fmt)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy().view(np.uint32)
    so = d_so.cpu().numpy().view(mp3g.STATE_DTYPE)
    plan.close()
    return raw, so


def as_interleaved(mp3g, raw, streams, fmt, n):
    """[n, 576, 2] samples (int16 or float32) of any format's raw output."""
    if fmt == mp3g.OUT_S16:
        return raw.view(np.int16)[:n * 1152].reshape(n, 576, 2)
    f = raw.view(np.float32)[:n * 1152]
    if fmt == mp3g.OUT_F32:
        return f.reshape(n, 576, 2)
    out = np.zeros((n, 576, 2), np.float32)
    for s, v in zip(streams, mp3g.planar_views(f, streams)):
        lo, k = int(s["first_granule"]), int(s["n_granules"])
        out[lo:lo + k] = v.T.reshape(k, 576, 2)
    return out


def is_mono(g):
    return ((g["header"] >> 6) & 3) == 3


# ---- 1. exact mode, F32 -------------------------------------------------------

def check_f32_against_oracle(out, want, what):
    assert out.dtype == np.float32 and out.shape == want.shape
    assert np.array_equal(q(out), want), f"{what}: q(float) differs from the oracle PCM"
    assert np.abs(out).max() <= np.float32(32767.0 / 32768.0)
    scaled = out.astype(np.float64) * 32768.0
    assert np.any(scaled != np.trunc(scaled)), f"{what}: every float is an integer / 32768 (truncated?)"


@pytest.mark.parametrize("name", ["classic_lame.mp3", "mpeg2.mp3"])
def test_exact_f32_sample_files(gpu, captured, name):
    g, c, want = captured[name]
    out, _ = gpu.decode_host(g, c, out_format=gpu.OUT_F32)
    check_f32_against_oracle(out, want, name)


# (the branches of tests/test_gpu_parity.py's SYNTH_CASES)
SYNTH_CASES = {
    "joint_ms_is": dict(),
    "joint_mixed": dict(p_mixed=0.5, p_event=0.08),
    "joint_all_is": dict(p_is=1.0, p_ms=0.5),
    "stereo": dict(mode=synth.MODE_STEREO),
    "dual": dict(mode=synth.MODE_DUAL),
    "mono": dict(mode=synth.MODE_MONO, p_mixed=0.3),
    "mpeg2_joint": dict(lsf=True, p_is=0.5),
    "mpeg2_mono": dict(lsf=True, mode=synth.MODE_MONO),
    "mpeg1_48k": dict(sfreq=1, p_mixed=0.3),
    "mpeg1_32k": dict(sfreq=2, p_mixed=0.3, p_is=0.5),
    "mpeg2_24k": dict(lsf=True, sfreq=1, p_is=0.3),
    "mpeg2_16k": dict(lsf=True, sfreq=2),
}


@pytest.mark.parametrize("case", sorted(SYNTH_CASES))
def test_exact_f32_synthetic_branches(gpu, case):
    g, c, s = synth.synth_batch(3, 40, seed=100 + len(case), **SYNTH_CASES[case])
    want, _ = oracle.dsp_streams(g, c, s)
    out, _ = gpu.decode_host(g, c, s, out_format=gpu.OUT_F32)
    check_f32_against_oracle(out, want, case)


# ---- 2. exact mode, planar ----------------------------------------------------

@pytest.fixture(scope="module")
def three_streams(gpu):
    """80 granules cut into streams of 7, 40 and 33: a wrong plane stride shows."""
    g, c, _ = synth.synth_batch(1, 40, seed=31, p_mixed=0.3, p_event=0.1, p_is=0.3)
    s = gpu.streams_for([7, 40, 33], gpu.STATE_OUT)
    raw, so = run_out(gpu, g, c, s, gpu.OUT_F32)
    f32 = as_interleaved(gpu, raw, s, gpu.OUT_F32, len(g)).copy()
    _, so16 = run_out(gpu, g, c, s, gpu.OUT_S16)
    assert so.tobytes() == so16.tobytes()
    return g, c, s, f32, so16


@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 0])
def test_exact_planar(gpu, three_streams, chunk):
    g, c, s, f32, so16 = three_streams
    raw, so = run_out(gpu, g, c, s, gpu.OUT_F32_PLANAR, chunk=chunk)
    flat = raw.view(np.float32)
    views = gpu.planar_views(flat, s)
    for k, v in enumerate(views):
        lo, n = int(s[k]["first_granule"]), int(s[k]["n_granules"])
        assert v.shape == (2, n * 576)
        want = f32[lo:lo + n].reshape(n * 576, 2).T
        assert np.array_equal(v, want), f"stream {k} chunk={chunk}: planes differ from the de-interleaved F32"
    assert so.tobytes() == so16.tobytes(), f"chunk={chunk}: the exported state depends on the format"


# ---- 3. mono, and mono / stereo switching ------------------------------------

@pytest.fixture(scope="module")
def switching():
    parts = [synth.synth_stream(11, 6), synth.synth_stream(12, 20, mode=synth.MODE_MONO),
             synth.synth_stream(13, 8), synth.synth_stream(14, 3, mode=synth.MODE_MONO),
             synth.synth_stream(15, 5)]
    g = np.concatenate([p[0] for p in parts])
    c = np.concatenate([p[1] for p in parts])
    return g, c


@pytest.fixture(scope="module")
def mono_cases(gpu, switching):
    out = {}
    g, c = synth.synth_stream(21, 30, mode=synth.MODE_MONO, p_mixed=0.3)
    for name, (gg, cc) in (("mono", (g, c)), ("switch", switching)):
        s = gpu.streams_for([len(gg)], gpu.STATE_OUT)
        want, _ = oracle.dsp_streams(gg, cc, s)
        out[name] = (gg, cc, s, want)
    return out


@pytest.mark.parametrize("chunk", [1, 2, 5, 7, 0])
@pytest.mark.parametrize("fmt", ["f32", "planar"])
@pytest.mark.parametrize("name", ["mono", "switch"])
def test_mono_and_switching(gpu, mono_cases, name, fmt, chunk):
    fmt = {"f32": gpu.OUT_F32, "planar": gpu.OUT_F32_PLANAR}[fmt]
    g, c, s, want = mono_cases[name]
    raw, _ = run_out(gpu, g, c, s, fmt, chunk=chunk)
    out = as_interleaved(gpu, raw, s, fmt, len(g))
    assert np.array_equal(q(out), want), f"{name} chunk={chunk}"
    m = is_mono(g)
    assert m.any()
    assert np.array_equal(out[m][:, :, 0], out[m][:, :, 1]), "mono granules: the channels differ"
    if name == "switch":
        assert not np.array_equal(out[~m][:, :, 0], out[~m][:, :, 1])


# ---- 4. fast mode, hot zones included ----------------------------------------

def hot_coeffs(rng, kind, n):
    i = np.arange(576)
    ones = np.ones((n, 2, 1), np.int64)
    if kind == "rand15":
        return rng.integers(-15, 16, size=(n, 2, 576))
    return np.where((i // 18) % 2 == 0, 15, -15) * ones  # altsb15


@pytest.fixture(scope="module", params=[("rand15", 230), ("altsb15", 255)], ids=lambda p: f"{p[0]}-{p[1]}")
def hot_batch(gpu, request):
    """tests/test_gpu_fast.py's hot-granule construction on 3 x 80 granules,
    with the exact-mode floats of the same batch."""
    kind, gg = request.param
    rng = np.random.default_rng(gg + len(kind))
    g, c, _ = synth.synth_batch(3, 40, seed=55, p_mixed=0.3, p_event=0.1, p_is=0.3)
    s = gpu.streams_for([80, 80, 80], gpu.STATE_OUT)
    idx = np.array([0, 5, 17, 18, 19, 40, 79, 80, 81, 150, 200, 238, 239])
    for ch in range(2):
        ch_view = g["ch"][:, ch]
        ch_view["global_gain"][idx] = gg
        ch_view["count1"][idx] = 576
    c[idx] = hot_coeffs(rng, kind, len(idx))
    assert gpu.validate(g, c)[0] == 0
    raw, _ = run_out(gpu, g, c, s, gpu.OUT_F32)
    exact = as_interleaved(gpu, raw, s, gpu.OUT_F32, len(g)).astype(np.float64) * 32768.0
    return g, c, s, exact


@pytest.mark.parametrize("chunk", [80, 1, 3, 7, 0])
def test_fast_formats(gpu, hot_batch, chunk):
    g, c, s, exact = hot_batch
    n = len(g)
    mode = gpu.MODE_FAST | gpu.FLAG_HOT_STATS
    plan_probe = gpu.Plan(s, granules_per_chunk=chunk, mode=mode)
    d_g, d_c = _dev(g), _dev(c)
    import torch
    d_p = torch.zeros(n * 1152, dtype=torch.int16, device="cuda")
    d_so = torch.zeros(len(s) * gpu.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    plan_probe.execute(d_g, d_c, d_p, None, d_so, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert plan_probe.hot_stats()["rewritten"] > 0, "no hot zone: the zone launch wrote nothing"
    plan_probe.close()
    raw16, so16 = run_out(gpu, g, c, s, gpu.OUT_S16, chunk=chunk, mode=gpu.MODE_FAST)
    s16 = as_interleaved(gpu, raw16, s, gpu.OUT_S16, n)
    assert np.array_equal(s16, d_p.cpu().numpy().reshape(n, 576, 2))
    # (both builds of the fast kernel: plain and with the hot counters)
    for fmt in (gpu.OUT_F32, gpu.OUT_F32_PLANAR):
        for md in (gpu.MODE_FAST, mode):
            raw, so = run_out(gpu, g, c, s, fmt, chunk=chunk, mode=md)
            out = as_interleaved(gpu, raw, s, fmt, n)
            assert np.array_equal(q(out), s16), f"fmt={fmt} chunk={chunk}: q(float) differs from the fast s16 output"
            assert so.tobytes() == so16.tobytes()
            d = np.abs(out.astype(np.float64) * 32768.0 - exact).max()
            print(f"fast vs exact float, fmt={fmt} chunk={chunk}: max |d| * 32768 = {d:.6f}")
            assert d < 2.0, d


# ---- 5. no stray writes ---------------------------------------------------------

@pytest.fixture(scope="module")
def sixty():
    return synth.synth_stream(41, 30, p_mixed=0.2, p_event=0.1)  # 60 granules


@pytest.mark.parametrize("chunk", [3, 0])
@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_no_stray_writes(gpu, sixty, fmt, mode, chunk):
    """One stream = granules [10, 50) of a 60-slot buffer holding a sentinel:
    nothing outside the stream's range changes, nor a guard behind the buffer."""
    g, c = sixty
    s = np.zeros(1, gpu.STREAM_DTYPE)
    s["first_granule"], s["n_granules"], s["flags"] = 10, 40, gpu.STATE_OUT
    guard = 4
    raw, _ = run_out(gpu, g, c, s, fmt, chunk=chunk, mode=gpu.MODE_FAST if mode == "fast" else gpu.MODE_EXACT,
                     guard=guard, fill=SENTINEL)
    w = gpu.out_bytes_per_granule(fmt) // 4  # 32-bit words per slot
    assert len(raw) == (60 + guard) * w
    assert np.all(raw[:10 * w] == SENTINEL), "wrote below the stream"
    assert np.all(raw[50 * w:60 * w] == SENTINEL), "wrote above the stream"
    assert np.all(raw[60 * w:] == SENTINEL), "wrote behind the buffer"
    inside = raw[10 * w:50 * w]
    if fmt != gpu.OUT_S16:
        assert not np.any(inside == SENTINEL), "a float of the stream's range was not written"
        assert np.all(np.isfinite(inside.view(np.float32)))
    else:
        assert np.any(inside != SENTINEL)


# ---- 6. format gating -------------------------------------------------------------

def test_format_gating(gpu):
    g, c, s = synth.synth_batch(1, 4, seed=3)
    for mode, fmt, status in ((gpu.FLAG_KERNEL_V2, gpu.OUT_F32, 8), (gpu.FLAG_KERNEL_V2, gpu.OUT_F32_PLANAR, 8),
                              (gpu.MODE_EXACT, 7, 1), (gpu.MODE_FAST, 7, 1)):
        with pytest.raises(gpu.Mp3gError) as e:
            _execute_raw(gpu, g, c, s, fmt, mode)
        assert e.value.status == status, (mode, fmt)
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_host(g, c, s, mode=gpu.FLAG_KERNEL_V2, out_format=gpu.OUT_F32)
    assert e.value.status == 8
    # the cross-check kernel still writes s16
    raw, _ = run_out(gpu, g, c, s, gpu.OUT_S16, mode=gpu.FLAG_KERNEL_V2)
    want, _ = oracle.dsp_streams(g, c, s)
    assert np.array_equal(as_interleaved(gpu, raw, s, gpu.OUT_S16, len(g)), want)


def _execute_raw(mp3g, g, c, s, fmt, mode):
    import torch
    d_out = torch.zeros(len(g) * 1152, dtype=torch.float32, device="cuda")
    plan = mp3g.Plan(s, mode=mode)
    try:
        plan.execute(_dev(g), _dev(c), d_out, stream=torch.cuda.current_stream().cuda_stream, out_format=fmt)
    finally:
        torch.cuda.synchronize()
        plan.close()


# ---- 7. decode_streams_tensor -------------------------------------------------------

@pytest.fixture(scope="module")
def bitstreams(gpu, sample_files):
    datas = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"],
             synth.encode_stream(61, 40, p_mixed=0.2, p_event=0.1, p_is=0.4),
             synth.encode_stream(62, 33, mode=synth.MODE_MONO),
             synth.encode_stream(63, 50, lsf=True, p_event=0.1),
             synth.encode_stream(64, 7)]
    refs = []
    for d in datas:
        ost, opcm = oracle.decode_all(d)
        assert ost == oracle.ORC_OK
        refs.append(np.frombuffer(opcm, np.int16).reshape(-1, 2))
    return datas, refs


@pytest.mark.parametrize("fmt", ["planar", "f32"])
@pytest.mark.parametrize("mode", ["exact", "fast"])
def test_decode_streams_tensor(gpu, bitstreams, mode, fmt):
    import torch
    datas, refs = bitstreams
    fmt = {"f32": gpu.OUT_F32, "planar": gpu.OUT_F32_PLANAR}[fmt]
    m = gpu.MODE_FAST if mode == "fast" else gpu.MODE_EXACT
    want16, wstreams, wst = gpu.decode_streams(datas, mode=m)
    out, views, streams, st = gpu.decode_streams_tensor(datas, mode=m, out_format=fmt)
    assert out.is_cuda and out.dtype == torch.float32 and all(v.is_cuda for v in views)
    assert out.numel() == 1152 * len(want16)
    assert streams.tobytes() == wstreams.tobytes()
    assert list(st) == list(wst)
    for k, v in enumerate(views):
        lo, n = int(streams[k]["first_granule"]), int(streams[k]["n_granules"])
        assert v.shape == ((2, n * 576) if fmt == gpu.OUT_F32_PLANAR else (n * 576, 2))
        assert v.data_ptr() >= out.data_ptr() and v.data_ptr() < out.data_ptr() + out.numel() * 4  # a view
        got = v.cpu().numpy()
        got = got.T if fmt == gpu.OUT_F32_PLANAR else got
        if mode == "exact":
            assert np.array_equal(q(got), refs[k]), f"stream {k}: q(view) differs from the oracle"
        assert np.array_equal(q(got), want16[lo:lo + n].reshape(n * 576, 2)), f"stream {k} vs decode_streams"
