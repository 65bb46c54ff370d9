"""tests/zone_model.py and the inputs of tests/test_gpu_fast_zones.py, without a
GPU:

  * the capacity claim of kernels.h zone_list_capacity as a property: over
    random and adversarial hot patterns and chunk lengths 1..4,100 the pieces
    of a chunk number at most kZoneListPerChunk + ceil(n_out / kZonePiece), so
    a plan's pieces fit the capacity its list is given (floor of 64 included);
    pieces tile their zones, zones are disjoint, ordered and inside the chunk;
  * the input conditions of every GPU case: the zone and piece shape the case
    is built for, no governing ratio within 10 % of the hot bound (the model
    asserts it; the least distance is printed), and at least 10 % of the
    oracle's samples inside +-32767 on the rewritten granules -- a clipped
    sample cannot tell the fast transforms from the reference's order.
"""
import numpy as np
import pytest

import fast_zone_inputs as Z
import mp3g
import zone_model as M

MIN_UNCLIPPED = 0.10


def check_chunk(nch, cd, hot_abs):
    """The properties of one chunk's zones and pieces; returns (zones, pieces)."""
    zones, flagged = M.zones_from_flags(nch, cd, hot_abs)
    pieces = M.zone_pieces(cd, zones)
    first, end = cd["out_first"], cd["out_first"] + cd["n_out"]
    assert len(zones) <= M.K_ZONES
    prev = first - 1
    for zs, ze in zones:
        assert first <= zs < ze <= end, (zones, first, end)
        assert zs > prev, f"zones overlap or touch out of order: {zones}"
        prev = ze
    # the pieces tile the zones exactly, in order
    it = iter(pieces)
    for zs, ze in zones:
        at = zs
        while at < ze:
            ps, pn, fl = next(it)
            assert ps == at and 1 <= pn <= M.K_PIECE and (pn == M.K_PIECE or ps + pn == ze), (zones, pieces)
            assert bool(fl & M.STATE_OUT) == bool((cd["flags"] & M.STATE_OUT) and ps + pn == end)
            at += pn
        assert at == ze
    assert next(it, None) is None
    assert len(pieces) <= M.K_ZONES + (cd["n_out"] + M.K_PIECE - 1) // M.K_PIECE, (len(pieces), cd["n_out"])
    assert flagged <= int(hot_abs.sum())
    return zones, pieces


def chunk_at(lead, n, n_stream=None):
    return dict(out_first=lead, n_out=n, stream=0, stream_first=0, stream_n=n_stream or lead + n, flags=M.STATE_OUT)


# every length for the sparse pattern; the dense ones (python time per hot
# granule) on all short lengths, the lengths around the piece size's
# multiples and 64 pieces, and a stride over the rest
ALL_LENGTHS = range(1, 4101)
DENSE_LENGTHS = sorted(set(range(1, 200)) | {k * 16 + d for k in (16, 63, 64, 65, 128, 256) for d in (-1, 0, 1)}
                       | set(range(200, 4101, 97)) | {4095, 4096, 4097, 4100})


def test_capacity_eight_zones_then_a_ninth():
    """Eight one-granule hot spots three apart and a ninth: the worst case of
    the bound (eight zones that each start a piece of their own, the eighth
    running to the chunk end), at every chunk length 1..4,100 and with the
    chunk behind a two-granule replay."""
    worst = 0
    for n in ALL_LENGTHS:
        for lead in (0, 5):
            nch = np.full(lead + n, 2)
            hot = np.zeros(lead + n, bool)
            hot[lead + 3 * np.arange(9)[3 * np.arange(9) < n]] = True
            cd = chunk_at(lead, n)
            zones, pieces = check_chunk(nch, cd, hot)
            worst = max(worst, len(pieces) - (n + M.K_PIECE - 1) // M.K_PIECE)
            if n > 3 * 8:
                assert len(zones) == M.K_ZONES and zones[-1][1] == lead + n, (n, zones)
    print(f"pieces beyond ceil(n_out / {M.K_PIECE}): at most {worst} (bound {M.K_ZONES})")
    assert worst <= M.K_ZONES


@pytest.mark.parametrize("pattern", ["all", "third", "random", "mono_runs"])
def test_capacity_dense_patterns(pattern):
    rng = np.random.default_rng(len(pattern))
    for n in DENSE_LENGTHS:
        lead = int(rng.integers(0, 6))
        tot = lead + n
        nch = np.full(tot, 2)
        if pattern == "all":
            hot = np.ones(tot, bool)
        elif pattern == "third":
            hot = np.arange(tot) % 3 == 0
        elif pattern == "random":
            hot = rng.random(tot) < rng.choice([0.01, 0.05, 0.3])
        else:
            # mono runs of 1..60 granules between stereo stretches, hot granules sparse
            i = 0
            while i < tot:
                i += int(rng.integers(1, 8))
                r = int(rng.integers(1, 61))
                nch[i:i + r] = 1
                i += r
            hot = rng.random(tot) < 0.04
        zones, pieces = check_chunk(nch, chunk_at(lead, n), hot)
        if pattern == "all":
            assert zones == [(lead, lead + n)] and len(pieces) == (n + M.K_PIECE - 1) // M.K_PIECE


def test_plan_total_fits_capacity():
    """A plan's pieces against zone_list_capacity of its chunk table, its floor
    of 64 included, over several stream tables and chunk lengths."""
    rng = np.random.default_rng(5)
    assert M.zone_list_capacity([1]) == 64 and M.zone_list_capacity([1] * 8) == 72
    assert M.zone_list_capacity([1024, 1025]) == 8 + 64 + 8 + 65
    for lengths in ([1], [3, 1, 2], [40, 1100, 40], [2200], [512], [256] * 16, [1, 4100, 17, 64]):
        s = mp3g.streams_for(lengths, mp3g.STATE_OUT)
        tot = int(sum(lengths))
        nch = np.where(rng.random(tot) < 0.2, 1, 2)
        for k in (1, 2, 7, 16, 17, 64, 128, 1024, 1025, 2048, 5000):
            chunks = M.plan_chunks(s, k)
            assert sum(cd["n_out"] for cd in chunks) == tot
            for hot in (np.ones(tot, bool), rng.random(tot) < 0.1, np.arange(tot) % 3 == 0):
                pieces = sum(len(check_chunk(nch, cd, hot)[1]) for cd in chunks)
                assert pieces <= M.zone_list_capacity([cd["n_out"] for cd in chunks])


def test_plan_chunks_and_replay_start():
    s = mp3g.streams_for([10, 7], mp3g.STATE_OUT)
    ch = M.plan_chunks(s, 4)  # 3 chunks of [0, 3), [3, 6), [6, 10); 2 of [10, 13), [13, 17)
    assert [(c["out_first"], c["n_out"], c["flags"]) for c in ch] == \
        [(0, 3, 0), (3, 3, 0), (6, 4, 2), (10, 3, 0), (13, 4, 2)]
    assert [c["out_first"] for c in M.plan_chunks(s, counts=[1, 7])] == [0, 10, 11, 12, 13, 14, 15, 16]
    # S S S M M M S S: a chunk behind a mono granule goes to the second-last stereo
    # granule before it -- also one inside the run that holds no stereo granule and
    # exports no state (it needs the hot flag of granule 2, whose zone spans the run)
    nch = np.array([2, 2, 2, 1, 1, 1, 2, 2])
    cd = dict(out_first=4, n_out=2, stream=0, stream_first=0, stream_n=8, flags=0)
    assert M.replay_start(nch, cd) == (1, (False, False))
    cd = dict(out_first=5, n_out=3, stream=0, stream_first=0, stream_n=8, flags=0)
    assert M.replay_start(nch, cd) == (1, (False, False))
    cd = dict(out_first=5, n_out=1, stream=0, stream_first=0, stream_n=8, flags=M.STATE_OUT)
    assert M.replay_start(nch, cd)[0] == 1
    # (one of the two granules before it mono: channel 1 from the stereo granules 2 and 6)
    cd = dict(out_first=7, n_out=1, stream=0, stream_first=0, stream_n=8, flags=M.STATE_IN)
    assert M.replay_start(nch, cd) == (2, (False, False))
    cd = dict(out_first=1, n_out=2, stream=0, stream_first=0, stream_n=8, flags=M.STATE_IN)
    assert M.replay_start(nch, cd) == (0, (True, True))
    # M M S: channel 1 has no stereo granule before the chunk -- it keeps the entry state
    cd = dict(out_first=2, n_out=1, stream=0, stream_first=0, stream_n=3, flags=M.STATE_IN)
    assert M.replay_start(np.array([1, 1, 2]), cd) == (0, (True, True))
    cd = dict(out_first=3, n_out=1, stream=0, stream_first=0, stream_n=4, flags=M.STATE_IN)
    assert M.replay_start(np.array([1, 1, 1, 2]), cd) == (1, (False, True))
    # zone_end: across a mono run to the first stereo granule after it, plus one
    assert M.zone_end(nch, 2, 8) == 7 and M.zone_end(nch, 2, 5) == 5 and M.zone_end(nch, 3, 8) == 5
    assert M.zone_end(nch, 6, 8) == 8 and M.zone_end(nch, 0, 8) == 2


def test_replayed_hot_granule_counts_but_records_nothing():
    """S(hot) M S | chunk: the replay starts at the second-last stereo granule;
    its V reaches the last stereo granule before the chunk only, so it records
    no zone and is still counted; a hot replayed granule whose V nothing reads
    (followed by as many channels, not the last replayed) is not flagged."""
    hot = np.array([True, False, False, False, False])
    nch = np.array([2, 1, 2, 1, 2])
    cd = dict(out_first=4, n_out=1, stream=0, stream_first=0, stream_n=5, flags=0)
    assert M.replay_start(nch, cd)[0] == 0
    assert M.zones_from_flags(nch, cd, hot) == ([], 1)
    nch = np.array([2, 2, 1, 2, 1, 2])
    hot = np.array([True, False, False, False, False, False])
    cd = dict(out_first=5, n_out=1, stream=0, stream_first=0, stream_n=6, flags=0)
    assert M.replay_start(nch, cd)[0] == 1 and M.zones_from_flags(nch, cd, hot) == ([], 0)


EXPECT = {
    # name: {granules_per_chunk: (zones per chunk with zones, pieces per chunk with zones)}
    "long1024": {2048: ([[(40, 1064)]], [64])},
    "long1025": {2048: ([[(40, 1065)]], [65])},
    "long1100": {2048: ([[(40, 1140)]], [69])},
    "monorun": {90: ([[(10, 52)]], [3]), 64: ([[(10, 45)], [(45, 52)]], [3, 1]), 8: ([[(10, 15)], [(15, 22)], [(22, 30)], [(30, 37)], [(37, 45)], [(45, 52)]], [1] * 6)},
    "monorun_loud": {90: ([[(10, 52)]], [3]), 64: ([[(10, 45)], [(45, 52)]], [3, 1]),
                     8: ([[(10, 15)], [(15, 22)], [(22, 30)], [(30, 37)], [(37, 45)], [(45, 52)]], [1] * 6)},
}


@pytest.mark.parametrize("name", sorted(Z.CASES))
def test_gpu_case_conditions(name):
    g, c, s, models, info = Z.case(name)
    assert mp3g.validate(g, c)[0] == 0
    nch = M.nch_of(g)
    for k, m in models.items():
        zones = [z for z in m["zones"] if z]
        pieces = [len(p) for p in m["pieces"] if p]
        lens = [[ze - zs for zs, ze in z] for z in zones]
        print(f"{name} chunk={k}: {m['zones_total']} zones in {len(zones)} chunks, longest {max(map(max, lens))} "
              f"granules, pieces per chunk up to {max(pieces)} ({sum(pieces)} in all, capacity "
              f"{M.zone_list_capacity([cd['n_out'] for cd in m['chunks']])}); rewritten {m['rewritten']}, "
              f"hot {m['hot']}; least |ratio - 1| = {m['min_dist']:.3f}; unclipped share of the rewritten "
              f"granules {info['unclipped'][k]:.3f}")
        assert m["min_dist"] >= 0.1
        assert info["unclipped"][k] >= MIN_UNCLIPPED, info["unclipped"][k]
        assert sum(pieces) <= M.zone_list_capacity([cd["n_out"] for cd in m["chunks"]])
        for cd, z in zip(m["chunks"], m["zones"]):
            assert all(cd["out_first"] <= zs < ze <= cd["out_first"] + cd["n_out"] for zs, ze in z)
        if name in EXPECT:
            assert (zones, pieces) == EXPECT[name][k], (zones, pieces)
        # the second launch's input (assertion (g)) is quiet: nothing hot, nothing near
        q = M.model(*Z.quiet_like(g, c), s, k)
        assert q["hot"] == 0 and q["zones_total"] == 0 and q["min_dist"] >= 0.1
    if name.startswith("long"):
        m = models[2048]
        assert m["hot"] == m["rewritten"] == int(s["n_granules"][1]) and m["state_exact"].tolist() == [False, True, False]
    if name == "tail2200":
        (z,), (p,) = [z for z in models[2200]["zones"] if z], [p for p in models[2200]["pieces"] if p]
        assert len(z) == 8 and [zs for zs, _ in z] == [10 + 6 * i for i in range(8)] and z[-1] == (52, 2200)
        assert all(ze - zs == 3 for zs, ze in z[:7]) and len(p) == 7 + (2148 + 15) // 16 == 142
        assert models[2200]["hot"] == 20 and models[2200]["state_exact"].all()
    if name.startswith("sat128"):
        m = models[128]
        assert [len(z) for z in m["zones"]] == [8, 8, 8, 0], m["zones"]
        assert m["zones"][0][-1] == (52, 128) and m["zones"][1][-1] == (128 + 52, 128 + 55)
        assert m["zones"][2][-1] == (256 + 52, 384)
        assert m["hot"] == 2 * (12 + 8 + 9) and not m["state_exact"].any()
    if name.startswith("monorun"):
        # the second and third piece of the serial plan's zone start inside the mono run
        starts = [ps for ps, _, _ in models[90]["pieces"][0]]
        assert starts == [10, 26, 42] and nch[26] == 1 and nch[42] == 1 and nch[10] == 2 and nch[51] == 2
        if name == "monorun_loud":
            assert nch[31] == 1 and g["ch"]["global_gain"][31, 0] >= Z.ISOLATED_GAINS[0]
    if name == "loud_batch":
        m = models[64]
        assert m["zones_total"] > 64 and m["hot"] > 200 and max(len(z) for z in m["zones"]) < 8


def test_loud_batch_chunk_counts():
    """The loud batch at a sample of chunk counts per stream (of all 256, the
    model refuses 123: 26, 29, 49, 52, ... and most above 140, where a replay
    starts right at a granule that is hot only through the overlap it no
    longer gets).  The GPU test's cost-model plan must not land on one -- the
    model would refuse it there; on an MI355X it takes 86 chunks per stream."""
    g, c, s, _, _ = Z.case("loud_batch")
    bad = []
    for cs in (1, 2, 3, 4, 8, 16, 32, 52, 64, 85, 86, 87):
        try:
            M.model(g, c, s, counts=[cs] * len(s))
        except AssertionError:
            bad.append(cs)
    print(f"chunk counts per stream the model refuses: {bad}")
    assert bad == [52, 87]
