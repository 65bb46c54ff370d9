"""Directed main-data inputs (tests/directed_stream.py) through the three
decoders that run without a GPU: the oracle (a bit-serial tree walk), the
host parse (a two-level table with a tree-walk fallback) and the device job
decoder built for the CPU (tests/native/hjob_host.hip: the multi-level table
of huffman_job.h, read directly and staged at 64 / 960 / 8192 words).  On
every set the three give byte-identical descriptors and coefficients; on A,
B, D and the plain cases of E they also equal what the writer meant, values
that none of them produced.  The GPU run is tests/test_gpu_huffman_directed.py.

The sets, as measured (directed_stream.py describes them):
  A  every codeword: 1,410 of 1,410 codewords, all 81 signed quads of both
     count1 tables, every escape extreme, max |line| 8206; seeds 1 / 2 / 3:
     22 / 22 / 27 frames, 22,968 / 22,968 / 28,188 bytes; long (the three
     together): 71 frames, 74,124 bytes
  B  22 symbol classes at all 64 phases of the reader's window: 704 frames,
     109,824 bytes (at 320 kbps, B320: 734,976 bytes)
  C  the classes cut by the end of the buffer or of their part at every
     bit: 2,816 frames of 104 bytes, 292,864 bytes
  D  every big_values 0..288, quads to the i <= 572 limit: 146 frames,
     152,424 bytes
  E  MPEG-1 scale factors: 176 frames, 55,088 bytes; MPEG-2: 2,049 frames,
     159,822 bytes

The conditions that keep these tests from being vacuous are asserted from
the writer's log and the scan's jobs, never from a decoder's output.
"""
import numpy as np
import pytest

import directed_stream as ds
import mp3g
import oracle
from test_scan_cpu import build_hjob_host, hjob_host  # noqa: F401  (fixture)

# granules whose arrays the writer vouches for: all of A, B and D; of E1 all
# but the 32 frames whose scfsi copies from a short or mixed granule 0
NOT_PLAIN = {"A1": 0, "A2": 0, "A3": 0, "A_long": 0, "B": 0, "B320": 0, "C": None, "D": 0, "E1": 32, "E2": 0}
SIZES = {"A1": (22, 22968), "A2": (22, 22968), "A3": (27, 28188), "A_long": (71, 74124), "B": (704, 109824),
         "B320": (704, 734976),
         "C": (2816, 292864), "D": (146, 152424), "E1": (176, 55088), "E2": (2049, 159822)}


def decode_jobs(L, s, stage_words):
    """The scan's jobs through the host build of the device job decoder."""
    n = len(s["granules"])
    g = s["granules"].copy()
    c = np.full((n, 2, 576), 0x5A5A, np.int16)  # poison: every line must be written
    args = (s["jobs"].ctypes.data, n, s["main_data"].ctypes.data, g.ctypes.data, c.ctypes.data)
    rc = L.hjob_decode_host(*args) if stage_words is None else L.hjob_decode_host_staged(*args, stage_words)
    assert rc == 0
    return g, c


def same(g, c, g2, c2, what):
    assert len(g) == len(g2), what
    bad = np.nonzero((g.view(np.uint8).reshape(len(g), -1) != g2.view(np.uint8).reshape(len(g2), -1)).any(1))[0]
    assert len(bad) == 0, f"{what}: descriptors differ at granules {bad[:10]}"
    badc = np.nonzero((c != c2).any(axis=(1, 2)))[0]
    assert len(badc) == 0, f"{what}: coefficients differ at granules {badc[:10]}"


def check_all_decoders(L, name):
    st, _ = ds.directed_set(name)
    ost, _, g, c = oracle.decode_all_capture(st["data"])
    assert ost == oracle.ORC_OK and len(g) == len(st["granules"]), name
    g2, c2, end = mp3g.parse_stream(st["data"])
    assert end == 7
    same(g2, c2, g, c, f"{name}: host parse vs oracle")
    s = mp3g.scan_streams([st["data"]], n_threads=1)
    assert list(s["end_status"]) == [7]
    for stage_words in (None, 64, 960, 8192):
        g3, c3 = decode_jobs(L, s, stage_words)
        same(g3, c3, g, c, f"{name}: job decoder (stage {stage_words}) vs oracle")
    p = st["plain"]
    if NOT_PLAIN[name] is not None:  # (set C: the writer has no expectation, the bar is the oracle)
        assert int((~p).sum()) == NOT_PLAIN[name]
        same(g[p], c[p], st["granules"][p], st["coeffs"][p], f"{name}: oracle vs the writer")
    return st


def test_code_lists_agree():
    """The product's and the oracle's codeword lists hold the same 1,410 entries."""
    a, b = ds.parse_codes(ds.CODES_INC), ds.parse_codes(ds.ORACLE_CODES_INC)
    assert len(a[2]) == 1410 and a == b
    for t in range(34):  # a complete prefix code per tree (Kraft sum 1)
        lens = [n for tree, _, n, _, _ in a[2] if tree == t]
        assert not lens or sum(2.0 ** -n for n in lens) == 1.0, t


@pytest.mark.parametrize("name", ds.SET_NAMES)
def test_decoders_agree(hjob_host, name):
    st = check_all_decoders(hjob_host, name)
    assert (st["n_frames"], len(st["data"])) == SIZES[name]


def escapes_of(lg, t):
    """The (value, sign) sets the log shows for table t's escapes: x alone, y alone, both."""
    e = lg[lg["table"] == t]
    ex, ey = e["lin"][:, 0] >= 0, e["lin"][:, 1] >= 0
    neg = e["v"][:, :2] < 0
    xs = {(int(a), bool(s)) for a, s in zip(e["lin"][ex & ~ey, 0], neg[ex & ~ey, 0])}
    ys = {(int(a), bool(s)) for a, s in zip(e["lin"][ey & ~ex, 1], neg[ey & ~ex, 1])}
    both = {(int(a), int(b), bool(s), bool(u)) for (a, b), (s, u) in zip(e["lin"][ex & ey], neg[ex & ey])}
    return xs, ys, both


@pytest.mark.parametrize("name", ["A1", "A2", "A3", "A_long"])
def test_set_a_covers_every_codeword(name):
    st, _ = ds.directed_set(name)
    lg = st["log"]
    assert set(lg["code"].tolist()) == set(range(1410))
    for t in (32, 33):
        assert len({tuple(v) for v in lg["v"][lg["table"] == t].tolist()}) == 81, t
    assert set(lg["table"].tolist()) == set(ds.PAIR_TABLES) | {32, 33}
    for t in ds.LINBITS_TABLES:
        w = ds.LINBITS[t]
        esc = {0, 1, (1 << w) - 2, (1 << w) - 1}
        xs, ys, both = escapes_of(lg, t)
        want = {(a, s) for a in esc for s in (False, True)}
        assert xs >= want and ys >= want, t
        assert both >= {(a, b, s, u) for a in esc for b in esc for s in (False, True) for u in (False, True)}, t
    assert int(np.abs(lg["v"].astype(np.int32)).max()) == 8206 == int(np.abs(st["coeffs"].astype(np.int32)).max())
    # granule-channels of at most 288 pairs and 4,095 bits, the largest of them over 3,000 bits
    s = mp3g.scan_streams([st["data"]], n_threads=1)
    assert s["jobs"]["big_values"].max() <= 288 and 3000 < s["jobs"]["part2_3_length"].max() <= 4095
    if name == "A_long":
        assert st["n_frames"] >= 64


@pytest.mark.parametrize("name", ["B", "B320"])
def test_set_b_covers_every_phase(name):
    st, cls = ds.directed_set(name)
    jobs = mp3g.scan_streams([st["data"]], n_threads=1)["jobs"]
    lg = st["log"]
    classes = ds.symbol_classes()
    assert len(classes) == 22
    for ci, (cname, t, vals, nbits) in enumerate(classes):
        v4 = np.array(tuple(vals) + (0,) * (4 - len(vals)))
        e = lg[(cls[lg["g"]] == ci) & (lg["ch"] == 1) & (lg["table"] == t) & (lg["v"] == v4).all(1)]
        assert (e["nbits"] == nbits).all() and len(e) == 3 * 64, cname
        phase = (jobs["part2_start"][2 * e["g"] + 1].astype(np.int64) + e["off"]) % 64
        assert set(phase.tolist()) == set(range(64)), cname
        # all of them far enough from the end of their buffer for the one-peek path
        assert (jobs["part2_start"][2 * e["g"] + 1] + e["off"].astype(np.uint64) + np.uint64(47)
                <= jobs["bit_end"][2 * e["g"] + 1]).all(), cname
    assert max(c[3] for c in classes) == 36  # the longest symbol there is


def test_set_c_cuts_every_bit():
    st, meta = ds.directed_set("C")
    jobs = mp3g.scan_streams([st["data"]], n_threads=1)["jobs"]
    lg = st["log"]
    classes = ds.symbol_classes()
    assert st["md_bits"] == 544 and len(st["data"]) == 104 * st["n_frames"]
    j = 2 * (2 * np.arange(st["n_frames"]) + 1) + 1  # the frame's last granule-channel
    span = (jobs["bit_end"][j] - jobs["part2_start"][j]).astype(np.int64)  # bits to the end of the buffer
    p23 = jobs["part2_3_length"][j].astype(np.int64)
    kind = meta[:, 1]
    assert (p23[kind != 3] > span[kind != 3]).all() and (p23[kind == 3] + 47 < span[kind == 3]).all()
    assert (jobs["big_values"][j][kind == 1] == 288).all()
    # where each frame's part ends: the buffer (kinds 1, 2) or part2_3_length (kind 3)
    end = np.where(kind == 3, p23, span)
    e = lg[(lg["g"] % 2 == 1) & (lg["ch"] == 1)]
    fr = e["g"] // 2
    is_cls = e["table"] == np.array([c[1] for c in classes])[meta[fr, 0]]
    cut = is_cls & (e["off"] < end[fr]) & (e["off"] + e["nbits"] > end[fr])
    before = end[fr] - e["off"]
    for ci, (cname, t, vals, nbits) in enumerate(classes):
        for k in ((1, 3) if t < 32 else (2, 3)):
            m = cut & (meta[fr, 0] == ci) & (meta[fr, 1] == k)
            assert set(before[m].tolist()) == set(range(1, nbits)), (cname, k)


def unstaged_blocks(jobs, stage_words):
    """Per 256-job block of the kernel: True where its span does not fit the stage (tools/huff_time.py's rule)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(ds.REPO, "tools"))
    from huff_time import staged_blocks
    return np.array([staged_blocks(jobs[b:b + 256], 256, stage_words) == 0.0 for b in range(0, len(jobs), 256)])


def test_spread_cuts(hjob_host):
    """The cut symbols in a batch whose 256-job blocks do not fit the default
    and the mid stage (the kernel reads them from global memory there): the
    pieces decode to what the same frames decode to inside set C."""
    st, _ = ds.directed_set("C")
    datas, is_piece, frames = ds.spread_cuts()
    assert len(frames) == 640 and len(datas) == 160 and sum(len(d) for d in datas) == 2572160
    g, c, _ = mp3g.parse_stream(st["data"])
    g2, c2, streams, end = mp3g.parse_streams(datas, n_threads=4)
    assert (end == 7).all()
    own = np.concatenate([np.arange(int(s["first_granule"]), int(s["first_granule"] + s["n_granules"]))
                          for s in streams[is_piece]])
    src = (2 * frames[:, None] + np.arange(2)).reshape(-1)
    same(g2[own], c2[own], g[src], c[src], "pieces vs the frames in set C")
    s = mp3g.scan_streams(datas, n_threads=4)
    for stage_words in (None, 960):
        g3, c3 = decode_jobs(hjob_host, s, stage_words)
        same(g3, c3, g2, c2, f"spread cuts: job decoder (stage {stage_words}) vs host parse")
    # every block but the last, partial one is out of reach of the two smaller stages
    assert unstaged_blocks(s["jobs"], 3584)[:-1].all() and unstaged_blocks(s["jobs"], 5376)[:-1].all()
    assert not unstaged_blocks(s["jobs"], 8704).any()
    is_own = np.zeros(len(g2), bool)
    is_own[own] = True
    full = len(g2) // 128 * 128  # the granules of the whole blocks: all pieces but at most the last
    assert is_own[:full].sum() >= len(own) - 16


def test_set_d_covers_the_row_geometry():
    st, cases = ds.directed_set("D")
    jobs = mp3g.scan_streams([st["data"]], n_threads=1)["jobs"]
    g, ch, bv, nq = cases.T
    assert np.array_equal(jobs["big_values"][2 * g + ch], bv) and set(bv.tolist()) == set(range(289))
    count1 = st["granules"]["ch"]["count1"][g, ch]
    assert np.array_equal(count1, 2 * bv + 4 * nq) and {572, 574, 576} <= set(count1.tolist())
    assert set(ch.tolist()) == {0, 1}
    for parity in (0, 1):
        for sel in (0, 1):
            m = (bv % 2 == parity) & (jobs["count1_table"][2 * g + ch] == sel)
            # a quad run that crosses a 16-line block boundary, ...
            assert ((2 * bv[m]) // 16 != (2 * bv[m] + 4 * nq[m] - 1) // 16).any(), (parity, sel)
            if parity:  # ... and, on the odd phase, a quad that straddles it (lines 14, 15 | 16, 17)
                first = 2 * bv[m] + (14 - 2 * bv[m]) % 16
                assert (first + 4 <= 2 * bv[m] + 4 * nq[m]).any(), sel
    # the count1 region runs to the limit in four cases of five, and stops after a few quads in the others
    full = np.where(2 * bv <= 572, (572 - 2 * bv) // 4 + 1, 0)
    assert 0.15 < np.mean(nq < full) < 0.25
    # line values distinct by position: no 16-line block of big values equals the next
    c = st["coeffs"][g, ch]
    for k in range(len(cases)):
        blocks = c[k][:2 * bv[k] // 16 * 16].reshape(-1, 16)
        assert (blocks[1:] != blocks[:-1]).any(1).all(), k


def test_set_e_covers_the_scale_factor_layouts():
    st, combos = ds.directed_set("E1")
    s = mp3g.scan_streams([st["data"]], n_threads=1)
    jobs = s["jobs"].reshape(-1, 2)
    n_sweep = 2 * 64 * 2  # granules of the two value passes
    for gr in (0, 1):
        for ch in (0, 1):
            for p in (0, 1):
                sl = slice(128 * p + gr, 128 * (p + 1), 2)
                D = st["granules"]["ch"][sl, ch]
                seen = {(int(a), int(b), int(w), int(t), int(m)) for (a, b), w, t, m in
                        zip(jobs["slen"][sl, ch, :2], D["win_switch_flag"], D["block_type"], D["mixed_block_flag"])}
                assert len(seen) == 64 and set(combos[sl, ch].tolist()) == set(range(64)), (gr, ch, p)
    # the "max" pass reaches 15 = 2^4 - 1 in long and short factors; the "pos" pass has granule-channels
    # whose long factors take at least 8 different values (slen 3 or 4: distinct by position)
    sweep = st["granules"]["ch"][:n_sweep]
    assert sweep["scalefac_l"][:128].max() == 15 and sweep["scalefac_s"][:128].max() == 15
    assert max(len(set(r.tolist())) for r in sweep["scalefac_l"][128:].reshape(-1, 22)) >= 8
    # scfsi: all 16 masks per channel on top of a long, a short and a mixed granule 0
    g1 = jobs[n_sweep + 1::2]
    D0 = st["granules"]["ch"][n_sweep::2]  # (the writer's granule 0 of these frames)
    kind0 = D0["block_type"].astype(int) + D0["mixed_block_flag"]  # 0 long, 2 short, 3 mixed
    for ch in (0, 1):
        assert set(kind0[:, ch].tolist()) == {0, 2, 3}
        for k0 in (0, 2, 3):
            assert set(g1["scfsi"][kind0[:, ch] == k0, ch].tolist()) == set(range(16)), (ch, k0)
        assert (g1["sf_kind"][:, ch] == g1["sf_kind"][0, 0]).all()  # granule 1 is long throughout
    assert int((~st["plain"]).sum()) == 32

    st2, _ = ds.directed_set("E2")
    s2 = mp3g.scan_streams([st2["data"]], n_threads=1)
    j2 = s2["jobs"].reshape(-1, 2)[:2048]
    for ch in (0, 1):
        for p in (0, 1):
            q = j2[1024 * p:1024 * (p + 1), ch]
            for kind in set(q["sf_kind"].tolist()):
                lay = {tuple(a) + tuple(b) for a, b in zip(q["slen"][q["sf_kind"] == kind].tolist(),
                                                           q["nsf"][q["sf_kind"] == kind].tolist())}
                assert len(lay) == 512, (ch, p, kind)
            assert len(set(q["sf_kind"].tolist())) == 2
    assert int(st2["granules"]["ch"]["preflag"][:2048].sum()) == 2 * 2 * 2 * 12  # scalefac_compress >= 500
    h = int(st2["granules"]["header"][-1])
    assert (h >> 6) & 3 == 1 and (h >> 4) & 3 == 1  # the intensity-stereo frame


def test_root_bits_11(tmp_path):
    """The device table at the other documented end of MP3G_HUFF_ROOT_BITS:
    build_huff_lut succeeds and set A decodes to the same bytes."""
    L = build_hjob_host(tmp_path / "libhjob_host_root11.so", ["-DMP3G_HUFF_ROOT_BITS=11"])
    for name in ("A1", "A2", "A3"):
        check_all_decoders(L, name)
