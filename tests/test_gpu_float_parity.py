"""Float32 PCM of the decode kernels against a float64 decode (tests/float_parity.py:
the metric, the case list, the reference's own figures).

Exact mode: the float the kernel writes IS the reference's sample before its
truncation, f_ref = float32(clamp(t)) * 2^-15 with t = sum * 32767.0f
(oracle.dsp_streams_float) -- bit for bit, in every float format, through the
host call and through a chunked plan.  (tests/test_gpu_outfmt.py pins only
trunc(f * 32768), the integer part.)

Fast mode: no bits to compare, so its error against the float64 decode is held
to the reference's own error against the same decode, on the same input:
rel_rms_fast <= 2 rel_rms_ref and max_rel_fast <= 3 max_rel_ref.  The fast
transforms and FMA contraction do as many float32 roundings as the reference's
order or fewer, so any equivalent rounding passes and a constant wrong by a
few 1e-6 does not; both ratios are relative, so the cases whose s16 PCM is all
zeros are held exactly as tightly as the loud ones.  The exported overlap
store is held the same way, and one consumer (windowed rows, BS.1770 loudness)
is checked on a bitstream 150 dB down.

The ratios measured on an MI355X are in DESIGN.md section 7.
"""
import faulthandler

import numpy as np
import pytest

import float_parity as fp
from mp3g import synth
from test_gpu_outfmt import as_interleaved, run_out

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 120  # every test's GPU work: the process is ended if it takes longer
RMS_FACTOR, MAX_FACTOR = 2.0, 3.0
CHUNK = 3


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} floats differ, first at {np.argwhere(bad)[:4].tolist()}"


def decode(gpu, k, fmt, mode, via):
    """(samples [n, 576, 2] or [n, 576], state_out) of case k in one float format,
    via the host call ("host") or a plan of `via` granules per chunk."""
    n = len(k.g)
    if via == "host":
        out, so = gpu.decode_host(k.g, k.c, k.s, mode=mode, out_format=fmt)
    else:
        out, so = run_out(gpu, k.g, k.c, k.s, fmt, chunk=via, mode=mode)
    if fmt in (gpu.OUT_S16_MONO, gpu.OUT_F32_MONO):
        dt = np.int16 if fmt == gpu.OUT_S16_MONO else np.float32
        return out.reshape(-1).view(dt)[:n * 576].reshape(n, 576), so
    return as_interleaved(gpu, out.reshape(-1).view(np.uint32), k.s, fmt, n), so


# ---- exact mode: bits ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(fp.CASES))
def test_exact_floats_are_the_reference_bits(gpu, name):
    k = fp.case(name)
    for via in ("host", CHUNK):
        f32, _ = decode(gpu, k, gpu.OUT_F32, gpu.MODE_EXACT, via)
        assert_bits(f32, k.f_ref, f"{name} F32 via {via}")
        planar, _ = decode(gpu, k, gpu.OUT_F32_PLANAR, gpu.MODE_EXACT, via)
        assert_bits(planar, k.f_ref, f"{name} F32_PLANAR via {via}")
        mono, _ = decode(gpu, k, gpu.OUT_F32_MONO, gpu.MODE_EXACT, via)
        assert_bits(mono, k.mono_ref, f"{name} F32_MONO via {via}")
    if name in fp.QUIET_CASES:
        assert not decode(gpu, k, gpu.OUT_S16, gpu.MODE_EXACT, "host")[0].any()
        assert (f32 != 0).mean() > 0.9


# ---- fast mode: accuracy against float64 --------------------------------------------------------

def check_factors(what, rms, mx, ref_rms, ref_max):
    print(f"{what}: rel_rms {rms:.3e} = {rms / ref_rms:.2f} x ref {ref_rms:.3e}, "
          f"max_rel {mx:.3e} = {mx / ref_max:.2f} x ref {ref_max:.3e}")
    assert rms <= RMS_FACTOR * ref_rms, f"{what}: rel_rms {rms:.3e} > {RMS_FACTOR} x {ref_rms:.3e}"
    assert mx <= MAX_FACTOR * ref_max, f"{what}: max_rel {mx:.3e} > {MAX_FACTOR} x {ref_max:.3e}"


@pytest.mark.parametrize("name", list(fp.CASES))
def test_fast_floats_against_float64(gpu, name):
    k = fp.case(name)
    fails = []
    for via in (0, CHUNK):
        for fmt, v, mag, ref in ((gpu.OUT_F32, k.v, k.mag, (k.ref_rms, k.ref_max)),
                                 (gpu.OUT_F32_MONO, k.mono_v, k.mono_mag, (k.ref_mono_rms, k.ref_mono_max))):
            out, _ = decode(gpu, k, fmt, gpu.MODE_FAST, via)
            assert out.dtype == np.float32 and np.isfinite(out).all()
            rms, mx, _ = fp.stream_metrics(out.astype(np.float64) * 32768.0, v, k.s, mag)
            try:
                check_factors(f"{name} fmt={fmt} chunk={via}", rms, mx, *ref)
            except AssertionError as e:  # (every figure is printed before the test fails)
                fails.append(str(e))
            if name in fp.QUIET_CASES:
                assert (out != 0).mean() > 0.9, "fast floats of a quiet case are zeros"
    assert not fails, fails
    if name in fp.QUIET_CASES:
        for mode in (gpu.MODE_EXACT, gpu.MODE_FAST):
            assert not decode(gpu, k, gpu.OUT_S16, mode, 0)[0].any(), "the s16 PCM of a quiet case is not all zeros"


@pytest.mark.parametrize("name", list(fp.CASES))
def test_fast_store_against_float64(gpu, name):
    k = fp.case(name)
    for via in ("host", CHUNK):
        _, so = decode(gpu, k, gpu.OUT_F32, gpu.MODE_FAST, via)
        rms, mx = fp.store_metrics(so["store"], k.store)
        check_factors(f"{name} store via {via}", rms, mx, k.ref_store_rms, k.ref_store_max)


# ---- one consumer: windowed rows and loudness of a quiet bitstream -------------------------------

QUIET_BOOST = -100  # global_gain steps: 2^-25 in amplitude, 150 dB down
QUIET_GAIN = 2.0 ** 25  # brings the rows back up; a power of two, so exact in float32


def test_quiet_bitstream_rows_and_loudness(gpu):
    """Three bitstreams 150 dB down (joint stereo 44.1 kHz with mixed blocks and
    intensity stereo, MPEG-2 22.05 kHz, mono 48 kHz): the s16 PCM of both modes
    is zeros; the float rows of fast and exact mode differ by
    rel_rms <= (1 + 2) cap_rms (each is within its factor of the reference's
    cap); and brought up by the exact gain 2^25 they measure the same
    integrated loudness to 1e-4 LU (a 1e-6 relative sample error is 2e-6 in
    power, 1e-5 dB: a tenfold margin)."""
    import torch
    datas = [synth.encode_stream(801, 40, p_mixed=0.3, p_event=0.1, p_is=0.4, gain_boost=QUIET_BOOST),
             synth.encode_stream(802, 40, lsf=True, p_event=0.1, gain_boost=QUIET_BOOST),
             synth.encode_stream(803, 40, mode=synth.MODE_MONO, sfreq=1, gain_boost=QUIET_BOOST)]
    T = 23040  # the MPEG-2 stream's 40 granules; more than four 100 ms steps at every rate here
    rows = {}
    for key, mode in (("exact", gpu.MODE_EXACT), ("fast", gpu.MODE_FAST)):
        assert not gpu.decode_streams(datas, mode=mode)[0].any(), f"{key}: the s16 PCM is not all zeros"
        batch, lengths, _ = gpu.decode_windows_tensor(datas, [0] * len(datas), T, mode=mode,
                                                      out_format=gpu.OUT_F32_PLANAR)
        assert lengths.tolist() == [T] * len(datas)
        rows[key] = batch
    ex, fa = (rows[key].cpu().numpy().astype(np.float64) for key in ("exact", "fast"))
    assert 0 < np.abs(ex).max() < 2.0 ** -16  # (under one s16 step)
    for r in range(len(datas)):
        rel = float(np.sqrt(((fa[r] - ex[r]) ** 2).sum() / (ex[r] ** 2).sum()))
        print(f"row {r}: fast against exact rel_rms = {rel:.3e} (bound {3 * fp.CAP_RMS:.2e})")
        assert 0 < rel <= (1 + RMS_FACTOR) * fp.CAP_RMS, (r, rel)
    rates = gpu.stream_rates(datas)
    assert rates.tolist() == [44100, 22050, 48000]
    for r, rate in enumerate(rates.tolist()):
        ld = gpu.Loudness(rate, device=0)
        lufs = []
        for key in ("exact", "fast"):
            loud = (rows[key][r:r + 1] * QUIET_GAIN).contiguous()
            lufs.append(float(gpu.Loudness.stats(ld.execute(loud))["lufs"][0]))
        torch.cuda.synchronize()
        ld.close()
        print(f"row {r}: lufs exact {lufs[0]:.6f}, fast {lufs[1]:.6f}, difference {abs(lufs[0] - lufs[1]):.2e} LU")
        assert np.isfinite(lufs).all() and lufs[0] > -70.0, lufs
        assert abs(lufs[0] - lufs[1]) < 1e-4, lufs
