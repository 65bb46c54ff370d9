"""Oracle PCM vs an independent float64 ISO 11172-3 synthesis (tests/spec_dsp.py).

The reference's conformance test compares against mpg123 with the ISO/IEC
11172-4 bars (compliance_test.go:28-45): limited = RMS < 4.62 LSB and
max <= 32; full = RMS < 0.289 and max <= 2.  mpg123 is absent here, so the
independent float64 synthesis stands in for it; the oracle must meet the
FULL bar on the reference's sample streams and on synthetic streams that
exercise mixed blocks and intensity stereo.

That bar is in int16 LSBs.  The second half compares in the float domain
(tests/float_parity.py): the oracle's sample before truncation and its
exported overlap store against the float64 decode, relative to the signal, on
every branch and down to content whose s16 PCM is all zeros -- the yardstick the
product's float output is held to (tests/test_gpu_float_parity.py).
"""
import numpy as np
import pytest

import float_parity as fp
import oracle
import spec_dsp
from mp3g import synth

FULL_RMS, FULL_MAX = 0.289, 2


def _check(got, want):
    d = (got.astype(np.int64) - want.astype(np.int64)).astype(np.float64)
    rms, mx = float(np.sqrt((d ** 2).mean())), float(np.abs(d).max())
    assert rms < FULL_RMS and mx <= FULL_MAX, (rms, mx)


@pytest.mark.parametrize("name", ["classic_lame.mp3", "mpeg2.mp3"])
def test_oracle_full_compliance_vs_float64(captured, name):
    g, c, want = captured[name]
    got = spec_dsp.spec_decode(g, c, oracle.tables()["synth_d"].astype(np.float64))
    _check(got, want)


@pytest.mark.parametrize("kw", [dict(p_mixed=0.5, p_is=0.6, p_event=0.1),
                                dict(lsf=True, p_is=0.5, p_event=0.1),
                                dict(mode=synth.MODE_MONO, p_mixed=0.5, p_event=0.1)])
def test_oracle_full_compliance_synthetic(kw):
    g, c, s = synth.synth_batch(1, 50, seed=21, **kw)
    want, _ = oracle.dsp_streams(g, c, s)
    got = spec_dsp.spec_decode(g, c, oracle.tables()["synth_d"].astype(np.float64))
    _check(got, want)


# ---- the float domain (tests/float_parity.py: metric, cases, caps) ---------------------------

def trunc_clamp(t):
    """pcm_sample's truncation and clamp of the product t."""
    return np.clip(np.trunc(np.asarray(t, np.float64)), -32767, 32767).astype(np.int16)


@pytest.mark.parametrize("name", list(fp.CASES))
def test_float_entry_point_is_the_pcm_before_truncation(name):
    """oracle.dsp_streams' PCM is trunc + clamp of dsp_streams_float's t, sample
    for sample, with the same exported state; a mono granule's t is in both
    channels."""
    k = fp.case(name)
    pcm, state = oracle.dsp_streams(k.g, k.c, k.s)
    assert k.t.dtype == np.float32 and k.t.shape == pcm.shape
    assert np.array_equal(trunc_clamp(k.t), pcm)
    assert state.tobytes() == k.state.tobytes()
    assert np.array_equal(k.t[k.mono][..., 0], k.t[k.mono][..., 1])
    if name in fp.QUIET_CASES:
        assert not pcm.any(), "the s16 PCM of a quiet case is not all zeros"
        assert (k.t != 0).mean() > 0.9, "the floats of a quiet case are zeros too"


@pytest.mark.parametrize("name", list(fp.CASES))
def test_oracle_float_against_float64(name):
    k = fp.case(name)
    print(f"{name}: rel_rms = {k.ref_rms:.3e} (cap {fp.CAP_RMS:.2e}), max_rel = {k.ref_max:.3e} "
          f"(cap {fp.CAP_MAX:.2e})")
    assert 0 < k.ref_rms < fp.CAP_RMS and 0 < k.ref_max < fp.CAP_MAX, (k.ref_rms, k.ref_max)
    # where nothing clips, the magnitudes are those of the clamped truth itself
    if not (k.mag > fp.CLIP).any():
        assert fp.stream_metrics(k.f_ref.astype(np.float64) * 32768.0, k.v, k.s)[:2] == (k.ref_rms, k.ref_max)


@pytest.mark.parametrize("name", list(fp.CASES))
def test_oracle_store_against_float64(name):
    k = fp.case(name)
    print(f"{name}: store rel_rms = {k.ref_store_rms:.3e} (cap {fp.STORE_CAP_RMS:.2e}), "
          f"max_rel = {k.ref_store_max:.3e} (cap {fp.STORE_CAP_MAX:.2e})")
    assert 0 < k.ref_store_rms < fp.STORE_CAP_RMS and 0 < k.ref_store_max < fp.STORE_CAP_MAX
    assert np.abs(k.store[:, 0]).max(axis=(1, 2)).min() > 0  # (every stream ends with a store to compare)


def test_caps_are_the_table():
    """The caps are 2.5 x the worst figures of the table in float_parity.py, and
    those are what the oracle shows over the case list (within the same 2.5,
    either way: a table gone stale shows here before a cap goes slack)."""
    ks = [fp.case(n) for n in fp.CASES]
    worst = [max(getattr(k, a) for k in ks) for a in ("ref_rms", "ref_max", "ref_store_rms", "ref_store_max")]
    table = [fp.SAMPLE_WORST_RMS, fp.SAMPLE_WORST_MAX, fp.STORE_WORST_RMS, fp.STORE_WORST_MAX]
    assert [fp.CAP_RMS, fp.CAP_MAX, fp.STORE_CAP_RMS, fp.STORE_CAP_MAX] == [2.5 * x for x in table]
    for got, want in zip(worst, table):
        assert want / 2.5 <= got <= 2.5 * want, (worst, table)


@pytest.mark.parametrize("name", ["joint_mixed", "mpeg2_24k", "gain_m120"])
def test_sensitivity_to_one_window_coefficient(name):
    """The largest synthesis-window coefficient times 1 + 1e-5 in the spec's input:
    the int16 ISO bar still passes, the float check does not."""
    k = fp.case(name)
    d = oracle.tables()["synth_d"].astype(np.float64)
    d[np.argmax(np.abs(d))] *= 1 + 1e-5
    val, _ = fp.spec_streams(k.g, k.c, k.s, d)
    pcm, _ = oracle.dsp_streams(k.g, k.c, k.s)
    _check(trunc_clamp(val), pcm)  # blind
    rms, mx, _ = fp.stream_metrics(k.f_ref.astype(np.float64) * 32768.0, fp.clip(val), k.s, fp.magnitude(val))
    print(f"{name}: perturbed rel_rms = {rms:.3e} (was {k.ref_rms:.3e}), max_rel = {mx:.3e} (was {k.ref_max:.3e})")
    assert mx > fp.CAP_MAX, (mx, fp.CAP_MAX)
