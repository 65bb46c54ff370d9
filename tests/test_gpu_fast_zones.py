"""The fast mode's hot-zone list at its edges, on the GPU (granule_fast.hip,
DESIGN.md section 7): zones of more than 64 pieces (over 1,024 granules: the
piece write used to stop at one piece per lane), a chunk that records a ninth
zone with a long tail, the boundary 8 / 9 zones at ordinary chunk sizes,
pieces that start inside a mono run, and the hot counters of a loud batch
against tests/zone_model.py instead of a band.

The inputs are tests/fast_zone_inputs.py's; tests/test_zone_model_cpu.py checks
their conditions (zone shapes, no governing ratio within 10 % of the hot
bound, at least 10 % of the rewritten samples unclipped) without a GPU.

Every case is held to (check_case):
  (a) fast PCM within 1 LSB of the oracle everywhere;
  (b) on the model's rewritten granules, fast PCM equal to exact-mode PCM
      (MODE_EXACT, the v4 kernel, same input and format) byte for byte: the
      zone launch IS the v4 kernel from an exact entry state;
  (c) with FLAG_HOT_STATS, rewritten / zones / hot equal to the model's, and
      in_wave == 0;
  (d) the plain build (no stats flag) gives the same bytes;
  (e) the exported state of a stream whose last zone reaches its end equal to
      exact mode's byte for byte, of the others within 2e-5 max |ref|
      (tests/test_gpu_fast.py's bar);
  (f) sentinel guards of one stream's size on both sides of the output
      untouched;
  (g) a second execute of the same plan on a quiet input equals that input's
      own fast decode and counts nothing: the list was emptied, no stale piece
      ran.
What detects a zone whose tail pieces are missing is (b): there the fast
transforms' output of hot granules stays, which differs from the reference's
order on unclipped samples.
"""
import numpy as np
import pytest

import fast_zone_inputs as Z
import zone_model
from test_gpu_outfmt import SENTINEL, _dev, as_interleaved, q
from test_gpu_outfmt_mono import as_mono, dm16

pytestmark = pytest.mark.gpu

ZERO_STATS = {"rewritten": 0, "zones": 0, "hot": 0, "in_wave": 0}


def run_guarded(gpu, g, c, s, chunk, mode, fmt=0, second=None):
    """One plan, executed into the middle of a sentinel-filled buffer with a
    guard of the longest stream's size on both sides (f).  Returns a dict: out
    (the raw 32-bit words of the n granule slots), state, stats (hot_stats after
    the launch), chunks (the plan's chunk count) and, with second = (g2, c2),
    out2 / state2 / stats2 of a second execute of the same plan on that input
    (counters reset in between)."""
    import torch
    n = len(g)
    bpg = gpu.out_bytes_per_granule(fmt)
    w = bpg // 4
    guard = int(s["n_granules"].max())
    st = torch.cuda.current_stream().cuda_stream
    plan = gpu.Plan(s, granules_per_chunk=chunk, mode=mode)
    res = {"chunks": plan.info()["chunks"]}

    def once(gg, cc, tag):
        d_g, d_c = _dev(gg), _dev(cc)
        buf = torch.from_numpy(np.full((n + 2 * guard) * w, SENTINEL, np.uint32).view(np.int32)).cuda()
        d_so = torch.zeros(len(s) * gpu.STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        plan.execute(d_g, d_c, buf.data_ptr() + guard * bpg, None, d_so, stream=st, out_format=fmt)
        torch.cuda.synchronize()
        raw = buf.cpu().numpy().view(np.uint32)
        assert np.all(raw[:guard * w] == SENTINEL), f"{tag}: wrote in front of the buffer"
        assert np.all(raw[(guard + n) * w:] == SENTINEL), f"{tag}: wrote behind the buffer"
        return raw[guard * w:(guard + n) * w].copy(), d_so.cpu().numpy().view(gpu.STATE_DTYPE).copy()

    res["out"], res["state"] = once(g, c, "first launch")
    res["stats"] = plan.hot_stats(reset=True)
    if second is not None:
        res["out2"], res["state2"] = once(second[0], second[1], "second launch")
        res["stats2"] = plan.hot_stats()
    plan.close()
    return res


def samples(gpu, raw, s, fmt, n):
    """[n, 576, 2] (or [n, 576] for a mono format) samples of a raw output."""
    if fmt in (gpu.OUT_S16_MONO, gpu.OUT_F32_MONO):
        return as_mono(gpu, raw, fmt, n)
    return as_interleaved(gpu, raw, s, fmt, n)


_exact = {}


def exact_run(gpu, name, fmt):
    """Exact mode's output and state of case `name` in format fmt (once); the
    s16 output checked against the oracle."""
    if (name, fmt) not in _exact:
        g, c, s, _, info = Z.case(name)
        r = run_guarded(gpu, g, c, s, 0, gpu.MODE_EXACT, fmt)
        if fmt == gpu.OUT_S16:
            assert np.array_equal(samples(gpu, r["out"], s, fmt, len(g)), info["pcm"]), f"{name}: exact mode != oracle"
            assert r["state"].tobytes() == info["state"].tobytes(), f"{name}: exact-mode state != oracle"
        _exact[(name, fmt)] = (r["out"], r["state"])
    return _exact[(name, fmt)]


def check_state(gpu, s, model, so, so_exact, what):
    """(e)"""
    for st in range(len(s)):
        if model["state_exact"][st]:
            assert so[st].tobytes() == so_exact[st].tobytes(), f"{what}: stream {st}: state differs from exact mode's"
            continue
        for key in ("store", "vvec"):
            ref, got = so_exact[key][st], so[key][st]
            if key == "vvec":
                ref, got = ref[:, :960], got[:, :960]
            np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5 * max(1.0, float(np.abs(ref).max())),
                                       err_msg=f"{what}: stream {st} {key}")


def check_case(gpu, name, chunk, model=None, fmt=0):
    """(a) .. (g) of the module docstring for one plan of case `name`; model:
    tests/zone_model.py's result for that plan (default: the case's own for
    `chunk`).  Returns the stats run's (out, state)."""
    g, c, s, models, info = Z.case(name)
    model = models[chunk] if model is None else model
    n, what = len(g), f"{name} chunk={chunk} fmt={fmt}"
    quiet = Z.quiet_like(g, c)
    r = run_guarded(gpu, g, c, s, chunk, gpu.MODE_FAST | gpu.FLAG_HOT_STATS, fmt, second=quiet)
    got = samples(gpu, r["out"], s, fmt, n)
    ex_out, ex_state = exact_run(gpu, name, fmt)
    ex = samples(gpu, ex_out, s, fmt, n)
    mask = model["mask"]
    print(f"{what}: {r['chunks']} chunks, stats {r['stats']}, model rewritten={model['rewritten']} "
          f"zones={model['zones_total']} hot={model['hot']}; samples differing from exact mode: "
          f"{int((got != ex).sum())} in all, {int((got[mask] != ex[mask]).sum())} on the rewritten granules")
    # (a)
    if fmt == gpu.OUT_S16:
        d = np.abs(got.astype(np.int32) - info["pcm"].astype(np.int32))
        assert d.max() <= 1, f"{what}: max |dPCM| = {d.max()} LSB at granule {int(np.argwhere(d > 1)[0][0])}"
    # (b)
    bad = np.nonzero((got[mask] != ex[mask]).reshape(int(mask.sum()), -1).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rewritten granules differ from exact mode, first at granule " \
                          f"{int(np.nonzero(mask)[0][bad[0]])}"
    # (c)
    assert r["stats"] == {"rewritten": model["rewritten"], "zones": model["zones_total"], "hot": model["hot"],
                          "in_wave": 0}, (what, r["stats"])
    # (d)
    p = run_guarded(gpu, g, c, s, chunk, gpu.MODE_FAST, fmt)
    assert p["stats"] == ZERO_STATS
    assert p["out"].tobytes() == r["out"].tobytes(), f"{what}: the plain build's output differs"
    assert p["state"].tobytes() == r["state"].tobytes(), f"{what}: the plain build's state differs"
    # (e)
    check_state(gpu, s, model, r["state"], ex_state, what)
    # (g)
    own = run_guarded(gpu, quiet[0], quiet[1], s, chunk, gpu.MODE_FAST, fmt)
    assert r["out2"].tobytes() == own["out"].tobytes(), f"{what}: second launch differs from the quiet input's decode"
    assert r["state2"].tobytes() == own["state"].tobytes(), f"{what}: second launch's state differs"
    assert r["stats2"] == ZERO_STATS, (what, r["stats2"])
    return r["out"], r["state"]


# ---- zones of more than 64 pieces ------------------------------------------------

@pytest.mark.parametrize("name", ["long1024", "long1025", "long1100"])
def test_long_zone(gpu, name):
    """Quiet, loud, quiet: the loud stream one chunk and one zone of 1,024
    (64 pieces, the last length the one-piece-per-lane write covered), 1,025
    and 1,100 granules (65 / 69 pieces).  s16, float32 planar (whose pieces
    carry stream_n) and the s16 mono downmix, by the value rules of
    tests/test_gpu_outfmt*.py on the same plan's s16 output; the cost model's
    chunking gives the same bytes."""
    g, c, s, models, _ = Z.case(name)
    n = len(g)
    out16, so16 = check_case(gpu, name, 2048)
    s16 = samples(gpu, out16, s, gpu.OUT_S16, n)
    auto = run_guarded(gpu, g, c, s, 0, gpu.MODE_FAST)
    assert auto["out"].tobytes() == out16.tobytes(), f"{name}: the cost model's chunking gives other PCM"
    assert auto["state"].tobytes() == so16.tobytes(), f"{name}: the cost model's chunking gives another state"
    for fmt in (gpu.OUT_F32_PLANAR, gpu.OUT_S16_MONO):
        out, so = check_case(gpu, name, 2048, fmt=fmt)
        v = samples(gpu, out, s, fmt, n)
        if fmt == gpu.OUT_F32_PLANAR:
            assert np.array_equal(q(v), s16), f"{name}: q(planar float) differs from the s16 output"
        else:
            assert np.array_equal(v, dm16(s16)), f"{name}: S16_MONO differs from (L + R) >> 1 of the s16 output"
        assert so.tobytes() == so16.tobytes(), f"{name} fmt={fmt}: the state depends on the format"
        auto = run_guarded(gpu, g, c, s, 0, gpu.MODE_FAST, fmt)
        assert auto["out"].tobytes() == out.tobytes(), f"{name} fmt={fmt}: the cost model's chunking gives other PCM"


# ---- saturation --------------------------------------------------------------------

def test_saturated_chunk_long_tail(gpu):
    """Ten isolated loud granules near the start of a 2,200-granule chunk: the
    ninth zone turns the eighth into "to the chunk end" -- 2,148 granules, 135
    pieces, nearly all of them ordinary granules that (b) holds to exact
    mode's bytes as well."""
    check_case(gpu, "tail2200", 2200)


@pytest.mark.parametrize("name", ["sat128_mpeg1", "sat128_lsf"])
def test_exact_saturation(gpu, name):
    """128-granule chunks with 12, 8, 9 and no isolated loud granules: 8 zones
    fit, the ninth runs the eighth to the chunk end; counters exact."""
    check_case(gpu, name, 128)


# ---- pieces that start inside a mono run ---------------------------------------------

@pytest.mark.parametrize("chunk", [90, 64, 8])
@pytest.mark.parametrize("name", ["monorun", "monorun_loud"])
def test_pieces_inside_mono_run(gpu, name, chunk):
    """A loud stereo granule, 40 mono granules, then stereo (monorun_loud: a
    loud mono granule inside the run as well): as one chunk, one zone of 42
    whose second and third piece start inside the run and take channel 1's
    state from the last two stereo granules before it; with the chunk
    boundary inside the run (chunks of 64 and 8) the zones the model gives for
    that plan."""
    check_case(gpu, name, chunk)


@pytest.mark.parametrize("name", ["monorun", "monorun_loud"])
def test_mono_run_chunking_is_bit_identical(gpu, name):
    """The bit-identical-chunking assertion of
    test_fast_hot_zones_across_channel_switches on the long mono run: every
    chunking gives the serial decode's PCM and state.

    A chunk that lies inside the run and holds no stereo granule used to
    replay two granules only, never met the loud granule in front of the run
    and kept the fast transforms' output where the serial decode -- whose zone
    spans the run -- has the reference's order: 2 to 4 samples of 1 LSB in
    mono granules of the run at chunks of 1, 2, 3, 4, 7, 8, 16 and the cost
    model's (chunks of 64 agreed).  The fast pass now replays such a chunk from
    the stereo granules in front of the run as well (prologue, ch1_always)."""
    g, c, s, _, info = Z.case(name)
    n = len(g)
    serial = run_guarded(gpu, g, c, s, n, gpu.MODE_FAST)
    ref = samples(gpu, serial["out"], s, gpu.OUT_S16, n).astype(np.int32)
    bad = []
    for chunk in (64, 8, 1, 2, 3, 4, 7, 16, 0):
        r = run_guarded(gpu, g, c, s, chunk, gpu.MODE_FAST)
        d = np.abs(samples(gpu, r["out"], s, gpu.OUT_S16, n).astype(np.int32) - ref)
        gr = np.nonzero(d.reshape(n, -1).any(axis=1))[0]
        same_state = r["state"].tobytes() == serial["state"].tobytes()
        vs_oracle = int(np.abs(samples(gpu, r["out"], s, gpu.OUT_S16, n).astype(np.int32) - info["pcm"]).max())
        print(f"{name} chunk={chunk}: {int((d > 0).sum())} samples differ from the serial run (max {int(d.max())} LSB) "
              f"in granules {gr.tolist()}; state {'equal' if same_state else 'differs'}; max |dPCM| against the "
              f"oracle {vs_oracle}")
        if d.any() or not same_state:
            bad.append(chunk)
    assert not bad, f"{name}: chunkings {bad} differ from the serial run"


# ---- the loud batch's counters, exactly ------------------------------------------------

def test_loud_batch_counters_exact(gpu):
    """tests/test_gpu_fast.py's loud batch (6 % of the granules boosted; the
    seed is one whose batch has no governing ratio within 10 % of the bound)
    at 64-granule chunks and at the cost model's chunking: the counters equal
    the model's, where test_fast_loud_batch_and_hot_counters accepts 0.8x to
    3x of the oracle's hot count."""
    g, c, s, models, _ = Z.case("loud_batch")
    check_case(gpu, "loud_batch", 64)
    plan = gpu.Plan(s, granules_per_chunk=0, mode=gpu.MODE_FAST)
    total = plan.info()["chunks"]
    plan.close()
    # (equal streams get equal chunk counts from the cost model and from the
    # whole-rounds spread alike: mp3g_abi.cpp auto_chunks / spread_chunks)
    assert total % len(s) == 0, total
    model = zone_model.model(g, c, s, counts=[total // len(s)] * len(s))
    check_case(gpu, "loud_batch", 0, model=model)
