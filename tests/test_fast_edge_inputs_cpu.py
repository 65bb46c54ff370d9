"""The threshold inputs of tests/test_gpu_fast_threshold.py, checked on the
oracle alone (no GPU): tests/fast_edge_inputs.py must really put every stream
just under the fast kernel's hot-granule bounds ("under") and just over them
("over"), with enough unclipped PCM left to show an error.  These are
conditions on the inputs, not measurements of the kernel: a case that misses
one is changed (amplitudes, draws, seed), never the condition.
"""
import os
import re

import numpy as np
import pytest

import mp3g
import fast_edge_inputs as fe

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LO_SIGN = 0.95           # the (a, gain) grid is dense: worst gap ~0.054 octave
LO_GAIN_ONLY = 2 ** -0.25  # what the gain step alone guarantees (0.84)
HI = 1.0 - fe.MARGIN
MIN_UNCLIPPED = 0.10     # a clipped sample cannot show an error

IDS = [f"{k}-{v}" for k, v in fe.CASES]


def test_bounds_are_the_kernels():
    """The builder takes its bounds from mp3g.FAST_HOT_S / FAST_HOT_L1, and those
    are the defaults granule_fast.hip is built with (the values
    tests/test_abi_cpu.py ties to the library): after a changed bound the
    inputs move with it or this fails -- builder and kernel cannot disagree
    silently."""
    src = open(os.path.join(REPO, "go-mp3_amd", "csrc", "granule_fast.hip")).read()
    hot_s = float(re.search(r"#define MP3G_HOT_S ([0-9.]+)f", src).group(1))
    hot_l1 = float(re.search(r"#define MP3G_HOT_L1 ([0-9.]+)f", src).group(1))
    assert (hot_s, hot_l1) == (mp3g.FAST_HOT_S, mp3g.FAST_HOT_L1)
    _, _, _, info = fe.edge_case("rand", "long", "under")
    _, _, _, same = fe.edge_batch("rand", "long", "under", seed=1 + fe.CASES.index(("rand", "long")),
                                  hot_s=hot_s, hot_l1=hot_l1)
    assert np.array_equal(info["gain"], same["gain"]) and np.array_equal(info["ratio"], same["ratio"])


def test_grid_covers_what_the_gpu_test_promises():
    kinds = {k for k, _ in fe.CASES}
    assert kinds == {"rand", "alt", "altsb", "low", "p43edge", "spike"}
    assert {k for k, v in fe.CASES if v == "long"} == kinds
    for k in ("rand", "altsb"):
        assert {v for kk, v in fe.CASES if kk == k} == set(fe.VARIANTS)
    assert len(set(fe.CASES)) == len(fe.CASES)


@pytest.mark.parametrize("kind,variant", fe.CASES, ids=IDS)
def test_under(kind, variant):
    g, c, s, info = fe.edge_case(kind, variant, "under")
    assert len(s) == 64 and len(g) == 256 and (s["n_granules"] == 4).all()
    assert mp3g.validate(g, c)[0] == 0
    gain = g["ch"]["global_gain"]
    assert gain.max() <= 254  # ("over" is one step higher)
    assert not info["hot"].any(), "a granule is hot by the oracle's S"
    assert not info["hot_lo"].any(), "a granule is within the band of both bounds"
    lo = LO_SIGN if kind in fe.SIGN_KINDS else LO_GAIN_ONLY
    r = info["ratio"]
    assert r.min() >= lo and r.max() <= HI, (r.min(), r.max())
    # the ratio is what the flags are made of: the governing granule's smaller quantity
    gov = np.minimum(info["r_a"], info["r_b"]).reshape(64, 4).max(axis=1)
    assert np.array_equal(gov, r)
    if kind == "spike":  # truly second-level: lines far above kHotS, kept fast by the slot sums
        assert (info["r_a"].reshape(64, 4).max(axis=1) > 2.0).all()
        assert (info["level"] == 1).all()
    if kind == "p43edge":  # both sides of the x^(4/3) table's edge are in play
        m = np.abs(c.astype(np.int32))
        assert m[:4].max() <= 127 and m[4:8].min() >= 128 and m.max() <= 135 and m.min() >= 120
    assert info["unclipped"] >= MIN_UNCLIPPED, info["unclipped"]


@pytest.mark.parametrize("kind,variant", fe.CASES, ids=IDS)
def test_over(kind, variant):
    g, c, s, info = fe.edge_case(kind, variant, "over")
    gu, cu, _, _ = fe.edge_case(kind, variant, "under")
    assert np.array_equal(c, cu)
    assert np.array_equal(g["ch"]["global_gain"][:, 0].astype(int), gu["ch"]["global_gain"][:, 0].astype(int) + 1)
    h = g.copy()
    h["ch"]["global_gain"] = gu["ch"]["global_gain"]
    assert h.tobytes() == gu.tobytes(), "the sides differ in more than the gain"
    assert mp3g.validate(g, c)[0] == 0
    assert info["hot_hi"].reshape(64, 4).any(axis=1).all(), "a stream has no granule over both bounds"
    assert info["unclipped"] >= MIN_UNCLIPPED, info["unclipped"]


def test_both_levels_govern():
    levels = np.concatenate([fe.edge_case(k, v, "under")[3]["level"] for k, v in fe.CASES])
    assert (levels == 0).sum() >= 64 and (levels == 1).sum() >= 64
    # the sign patterns land where the kernel's comments put them
    for k, v, lvl in (("alt", "long", 0), ("altsb", "long", 0), ("rand", "long", 1), ("low", "long", 1)):
        info = fe.edge_case(k, v, "under")[3]
        assert (info["level"] == lvl).all(), (k, v)
        if lvl == 0:
            assert info["r_a"].max() <= HI and info["r_b"].reshape(64, 4).max(axis=1).min() > 1.5
        else:
            assert info["r_b"].max() <= HI and info["r_a"].reshape(64, 4).max(axis=1).min() > 1.0


def test_deterministic_and_bounds_from_the_package():
    a = fe.edge_batch("rand", "bandgain_short", "under", n_streams=6, seed=3)
    b = fe.edge_batch("rand", "bandgain_short", "under", n_streams=6, seed=3)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(a[3]["pcm"], b[3]["pcm"])
    # another bound moves the inputs with it (nothing hard-coded)
    c = fe.edge_batch("rand", "long", "under", n_streams=6, seed=3, hot_s=8.0, hot_l1=128.0)
    d = fe.edge_batch("rand", "long", "under", n_streams=6, seed=3)
    assert np.array_equal(c[0]["ch"]["global_gain"].astype(int), d[0]["ch"]["global_gain"].astype(int) + 4)
