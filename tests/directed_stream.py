"""A directed Layer III bitstream writer and the directed main-data input sets.

Test tooling in plain Python / numpy, independent of libmp3gsynth.so and of
every decoder: the caller gives an explicit list of granule-channel specs
(gc()) grouped into frames (frame()), and write_stream() returns the bytes,
the descriptors (GRANULE_DTYPE) and [n, 2, 576] coefficients a decoder must
recover, and a log of every Huffman symbol written (LOG_DTYPE: table, values,
escape values, bit offset inside its part, length).  The code lists are
parsed from go-mp3_amd/csrc/huffman_codes.inc; every other table here (scale
factor bands, slen pairs, the MPEG-2 nr_of_sfb "normal" rows, bitrates) is
the standard's numbers (ISO/IEC 11172-3, 13818-3).

Framing: MPEG-1 at 44.1 kHz or MPEG-2 (LSF) at 22.05 kHz, two channels, no
CRC, no padding, one bitrate per stream, main_data_begin = 0 in every frame
-- each frame's main data is its own buffer, so the writer controls where
that buffer ends.  The part2_3_length and big_values fields can be
overridden (the side info can lie); a granule-channel always starts where
the fields before it say, and what it writes past the end of the frame's
main data is dropped.

The shift tool: shift(k) is a granule-channel of k pairs (0, 0) in table 1,
one bit per pair; in front of another granule-channel it moves that one by
k bits (reader phases, cut positions).

The sets (all seeded, generated when asked for; sizes as measured):

  A  set_a(seed)      every codeword: each (x, y) of tables 1..31 (not 4,
                      14), every escape at linbits values {0, 1, 2^w - 2,
                      2^w - 1} in x alone, y alone and both with both signs,
                      all 81 signed quads of both count1 tables.  1,410 of
                      1,410 codewords, max |line| 8206.  320 kbps; seed 1 is
                      22 frames, 22,968 bytes; the long version (set_a_long,
                      seeds 1, 2, 3) 71 frames, 74,124 bytes.
  B  set_b()          phases: the widest symbol of each linbits table, the
                      longest plain codeword of trees 13, 15, 16, 24 and the
                      longest quad of each count1 table (22 classes), each at
                      all 64 phases of the reader's window.  48 kbps,
                      704 frames, 109,824 bytes; set_b(14), the same at
                      320 kbps for the reader of global memory: 704 frames,
                      734,976 bytes.
  C  set_c()          cuts: the classes of B as the last granule-channel of
                      104-byte frames (32 kbps, 544 bits of main data),
                      shifted by 0..63 bits, cut by the end of the buffer
                      (pairs: kind 1, quads: kind 2) or by part2_3_length
                      (kind 3).  2,816 frames, 292,864 bytes.  spread_cuts():
                      640 of them in a batch whose 256-job blocks exceed the
                      kernel's two smaller LDS stages, 2,572,160 bytes.
  D  set_d()          row geometry: every big_values 0..288 with the count1
                      region run to the i <= 572 limit (a fifth stop after a
                      few quads).  320 kbps, 146 frames, 152,424 bytes.
  E  set_e_mpeg1()    scale factors, MPEG-1: 16 scalefac_compress x {long,
                      start, short, mixed} in every channel and granule, two
                      value passes, 16 scfsi masks x granule 0 long / short /
                      mixed.  96 kbps, 176 frames, 55,088 bytes.
     set_e_mpeg2()    MPEG-2: scalefac_compress 0..511 x {long, short} on
                      both channels, two value passes, one intensity-stereo
                      frame.  24 kbps, 2,049 frames, 159,822 bytes.
"""
import os
import re

import numpy as np

import mp3g

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES_INC = os.path.join(REPO, "go-mp3_amd", "csrc", "huffman_codes.inc")
ORACLE_CODES_INC = os.path.join(REPO, "oracle", "huffman_codes.inc")

LONG, START, SHORT, STOP, MIXED = "long", "start", "short", "stop", "mixed"
_BLOCK_TYPE = {LONG: 0, START: 1, SHORT: 2, STOP: 3, MIXED: 2}

LOG_DTYPE = np.dtype([("g", "<i4"), ("ch", "i1"), ("table", "i1"), ("code", "<i2"), ("v", "<i2", (4,)),
                      ("lin", "<i2", (2,)), ("off", "<i4"), ("nbits", "<i2")])

# ISO/IEC 11172-3 Table B.8 (44.1 kHz) and 13818-3 (22.05 kHz): long-block scale factor bands
SFB_LONG = {False: [0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 90, 110, 134, 162, 196, 238, 288, 342, 418, 576],
            True: [0, 6, 12, 18, 24, 30, 36, 44, 54, 66, 80, 96, 116, 140, 168, 200, 238, 284, 336, 396, 464, 522,
                   576]}
# 11172-3 2.4.2.7: slen1, slen2 of scalefac_compress
SLEN_MPEG1 = [(0, 0), (0, 1), (0, 2), (0, 3), (3, 0), (1, 1), (1, 2), (1, 3),
              (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3), (4, 2), (4, 3)]
# 13818-3 Table 6, the rows used without intensity stereo: [row][long, short][part]
NSFB_MPEG2 = [[(6, 5, 5, 5), (9, 9, 9, 9)], [(6, 5, 7, 3), (9, 9, 12, 6)], [(11, 10, 0, 0), (18, 18, 0, 0)]]
# Layer III bitrates in kbps [lsf][index]
BITRATE = {False: [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320],
           True: [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]}


def parse_codes(path=CODES_INC):
    """(tree[34], linbits[34], codes[(tree, code, len, x, y)]) of a huffman_codes.inc."""
    text = open(path).read()
    ints = lambda name: [int(v) for v in re.search(name + r"\[34\] = \{([^}]*)\}", text).group(1).split(",")]
    codes = [(int(t), int(c, 16), int(n), int(x), int(y)) for t, c, n, x, y in
             re.findall(r"\{\s*(\d+), 0x([0-9a-fA-F]+),\s*(\d+),\s*(\d+),\s*(\d+)\}", text)]
    return ints("HUFF_TABLE_TREE"), ints("HUFF_TABLE_LINBITS"), codes


TREE, LINBITS, CODES = parse_codes()
assert len(CODES) == 1410
CODE_OF = {(t, x, y): k for k, (t, c, n, x, y) in enumerate(CODES)}
PAIR_TABLES = [t for t in range(1, 32) if TREE[t] >= 0]
LINBITS_TABLES = [t for t in PAIR_TABLES if LINBITS[t]]


def mpeg2_slen(sfc):
    """13818-3 2.4.3.2 without intensity stereo: (slen[4], nr_of_sfb row, preflag)."""
    if sfc < 400:
        return ((sfc >> 4) // 5, (sfc >> 4) % 5, (sfc & 15) >> 2, sfc & 3), 0, 0
    if sfc < 500:
        s = sfc - 400
        return ((s >> 2) // 5, (s >> 2) % 5, s & 3, 0), 1, 0
    s = sfc - 500
    return (s // 3, s % 3, 0, 0), 2, 1


def gc(pairs=(), quads=(), tables=(1, 1, 1), r0=0, r1=0, block=LONG, sfc=0, sf=None, c1sel=0, gain=120,
       p23=None, bv=None, sbg=(0, 0, 0), sfscale=0, preflag=0):
    """One granule-channel.  pairs: signed (x, y); quads: signed (v, w, x, y);
    sf: the scale factors in stream order (None: zeros; "max": every field at
    2^slen - 1; "pos": distinct by position); p23 / bv: overrides of the
    part2_3_length and big_values fields."""
    return dict(pairs=list(pairs), quads=list(quads), tables=tuple(tables), r0=r0, r1=r1, block=block, sfc=sfc,
                sf=sf, c1sel=c1sel, gain=gain, p23=p23, bv=bv, sbg=tuple(sbg), sfscale=sfscale, preflag=preflag)


def shift(k):
    """k bits: k pairs (0, 0) in table 1."""
    return gc(pairs=[(0, 0)] * k)


def frame(granules, scfsi=((0, 0, 0, 0), (0, 0, 0, 0)), mode_ext=None):
    """granules: [[ch0, ch1], [ch0, ch1]] (MPEG-2: one granule)."""
    return dict(gr=granules, scfsi=scfsi, mode_ext=mode_ext)


def region_starts(spec, lsf):
    """The first lines of regions 1 and 2 (11172-3 2.4.2.7 region0/1_count)."""
    if spec["block"] in (SHORT, MIXED):
        return 36, 576
    l = SFB_LONG[lsf]
    r0, r1 = (7, 13) if spec["block"] != LONG else (spec["r0"], spec["r1"])
    return l[r0 + 1], l[min(r0 + r1 + 2, 22)]


def sf_fields(spec, lsf, gr, scfsi):
    """The scale factor fields the stream carries, in order: (bits, dest),
    dest = ("l", sfb) or ("s", sfb, window)."""
    blk = spec["block"]
    if lsf:
        slen, row, _ = mpeg2_slen(spec["sfc"])
        assert blk != MIXED
        short = blk == SHORT
        out, k = [], 0
        for part in range(4):
            for _ in range(NSFB_MPEG2[row][short][part]):
                out.append((slen[part], ("s", k // 3, k % 3) if short else ("l", k)))
                k += 1
        return out
    s1, s2 = SLEN_MPEG1[spec["sfc"]]
    if blk == SHORT:
        return [(s1 if sfb < 6 else s2, ("s", sfb, w)) for sfb in range(12) for w in range(3)]
    if blk == MIXED:
        return [(s1, ("l", sfb)) for sfb in range(8)] + \
               [(s1 if sfb < 6 else s2, ("s", sfb, w)) for sfb in range(3, 12) for w in range(3)]
    out = []
    for part, (lo, hi) in enumerate(((0, 6), (6, 11), (11, 16), (16, 21))):
        if gr == 0 or not scfsi[part]:
            out += [(s1 if part < 2 else s2, ("l", sfb)) for sfb in range(lo, hi)]
    return out


def main_data_bits(lsf, bitrate_index):
    """The main-data bits of a frame: its size less the header and the side info."""
    size = (144 * BITRATE[lsf][bitrate_index] * 1000 // (22050 if lsf else 44100)) >> int(lsf)
    return 8 * (size - 4 - (17 if lsf else 32))


class _Bits:
    __slots__ = ("v", "n")

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, nbits):
        assert 0 <= val < (1 << nbits) or (nbits == 0 and val == 0), (val, nbits)
        self.v = (self.v << nbits) | val
        self.n += nbits


def _put_symbol(b, table, vals, log, g, ch):
    """One pair (table 1..31) or quad (32, 33) with its escapes and signs;
    logged with its bit offset from the start of the granule-channel's part 2."""
    start = b.n
    lb = LINBITS[table]
    lin = [-1, -1]
    if table < 32:
        mag = [abs(v) for v in vals]
        cx = [min(m, 15) if lb else m for m in mag]
        k = CODE_OF[(TREE[table], cx[0], cx[1])]
        b.put(CODES[k][1], CODES[k][2])
        for i in range(2):
            if lb and cx[i] == 15:
                lin[i] = mag[i] - 15
                b.put(lin[i], lb)
            if mag[i]:
                b.put(int(vals[i] < 0), 1)
        v4 = (vals[0], vals[1], 0, 0)
    else:
        assert all(abs(v) <= 1 for v in vals)
        k = CODE_OF[(TREE[table], 0, sum(abs(v) << (3 - i) for i, v in enumerate(vals)))]
        b.put(CODES[k][1], CODES[k][2])
        for v in vals:
            if v:
                b.put(int(v < 0), 1)
        v4 = tuple(vals)
    log.append((g, ch, table, k, v4, tuple(lin), start, b.n - start))


def write_stream(frames, lsf=False, bitrate_index=14, mode=0, mode_ext=0):
    """frames (frame()) -> dict(data, granules, coeffs, log, plain, md_bits).

    plain[n]: the writer's arrays are what a decoder must recover for granule
    n (no field override, no scfsi copy from a granule 0 that is not long)."""
    n_gr = 1 if lsf else 2
    si_bytes = 17 if lsf else 32
    md_bits = main_data_bits(lsf, bitrate_index)
    size = md_bits // 8 + 4 + si_bytes
    n = len(frames) * n_gr
    G = np.zeros(n, mp3g.GRANULE_DTYPE)
    coef = np.zeros((n, 2, 576), np.int16)
    plain = np.ones(n, bool)
    log, out = [], bytearray()
    for fi, fr in enumerate(frames):
        mx = mode_ext if fr["mode_ext"] is None else fr["mode_ext"]
        header = 0xFFE00000 | ((2 if lsf else 3) << 19) | (1 << 17) | (1 << 16) | (bitrate_index << 12) | \
            (mode << 6) | (mx << 4)
        si = _Bits()
        si.put(0, 8 if lsf else 9)  # main_data_begin
        si.put(0, 2 if lsf else 3)  # private bits
        if not lsf:
            for ch in range(2):
                for k in range(4):
                    si.put(fr["scfsi"][ch][k], 1)
        md, cursor, fits = 0, 0, True
        assert len(fr["gr"]) == n_gr
        for gr in range(n_gr):
            g = fi * n_gr + gr
            G[g]["header"], G[g]["gr"] = header, gr
            for ch in range(2):
                spec = fr["gr"][gr][ch]
                D = G[g]["ch"][ch]
                scfsi = fr["scfsi"][ch] if (not lsf and gr == 1 and spec["block"] in (LONG, START, STOP)) else (0,) * 4
                # ---- part 2 ----
                b = _Bits()
                fields = sf_fields(spec, lsf, gr, scfsi)
                sf = spec["sf"]
                if sf is None:
                    sf = [0] * len(fields)
                elif isinstance(sf, str):
                    sf = [((1 << w) - 1) if sf == "max" else ((k + 1) & ((1 << w) - 1)) for k, (w, _) in
                          enumerate(fields)]
                assert len(sf) == len(fields)
                for v, (w, dest) in zip(sf, fields):
                    b.put(v, w)
                    if dest[0] == "l":
                        D["scalefac_l"][dest[1]] = v
                    else:
                        D["scalefac_s"][dest[1]][dest[2]] = v
                if any(scfsi):
                    g0 = fr["gr"][0][ch]
                    if g0["block"] in (SHORT, MIXED):
                        plain[g] = False  # the reference's quirk: the oracle is the bar
                    for part, (lo, hi) in enumerate(((0, 6), (6, 11), (11, 16), (16, 21))):
                        if scfsi[part]:
                            D["scalefac_l"][lo:hi] = G[g - 1]["ch"][ch]["scalefac_l"][lo:hi]
                part2_len = b.n
                # ---- part 3 ----
                pairs, quads = spec["pairs"], spec["quads"]
                assert len(pairs) <= 288 and 2 * len(pairs) + 4 * len(quads) <= 576
                r1s, r2s = region_starts(spec, lsf)
                for k, p in enumerate(pairs):
                    t = spec["tables"][0 if 2 * k < r1s else 1 if 2 * k < r2s else 2]
                    _put_symbol(b, t, p, log, g, ch)
                    coef[g, ch, 2 * k], coef[g, ch, 2 * k + 1] = p
                for k, q in enumerate(quads):
                    _put_symbol(b, 32 + spec["c1sel"], q, log, g, ch)
                    coef[g, ch, 2 * len(pairs) + 4 * k:][:4] = q
                p23 = b.n if spec["p23"] is None else spec["p23"]
                bv = len(pairs) if spec["bv"] is None else spec["bv"]
                assert p23 < 4096 and bv < 512
                if spec["p23"] is not None or spec["bv"] is not None:
                    plain[g] = False
                D["count1"] = 2 * len(pairs) + 4 * len(quads) if p23 else 0
                ws = spec["block"] != LONG
                D["global_gain"], D["scalefac_scale"] = spec["gain"], spec["sfscale"]
                D["preflag"] = mpeg2_slen(spec["sfc"])[2] if lsf else spec["preflag"]
                D["win_switch_flag"], D["block_type"] = int(ws), _BLOCK_TYPE[spec["block"]]
                D["mixed_block_flag"] = int(spec["block"] == MIXED)
                if ws:
                    D["subblock_gain"] = spec["sbg"]
                # ---- side info ----
                si.put(p23, 12)
                si.put(bv, 9)
                si.put(spec["gain"], 8)
                si.put(spec["sfc"], 9 if lsf else 4)
                si.put(int(ws), 1)
                if ws:
                    si.put(_BLOCK_TYPE[spec["block"]], 2)
                    si.put(int(spec["block"] == MIXED), 1)
                    for t in spec["tables"][:2]:
                        si.put(t, 5)
                    for s in spec["sbg"]:
                        si.put(s, 3)
                else:
                    for t in spec["tables"]:
                        si.put(t, 5)
                    si.put(spec["r0"], 4)
                    si.put(spec["r1"], 3)
                if not lsf:
                    si.put(spec["preflag"], 1)
                si.put(spec["sfscale"], 1)
                si.put(spec["c1sel"], 1)
                # ---- into the frame's main data, clipped at its end ----
                room = md_bits - cursor
                if room > 0 and b.n:
                    keep = min(b.n, room)
                    md &= ~(((1 << keep) - 1) << (room - keep))  # a shortened part before it may reach in here
                    md |= (b.v >> (b.n - keep)) << (room - keep)
                if cursor + max(b.n, p23) > md_bits:
                    fits = False
                cursor += p23
        assert si.n == 8 * si_bytes, si.n
        if not fits:
            assert not plain[fi * n_gr:(fi + 1) * n_gr].all(), f"frame {fi} does not fit its main data"
            plain[fi * n_gr:(fi + 1) * n_gr] = False
        out += header.to_bytes(4, "big") + si.v.to_bytes(si_bytes, "big") + md.to_bytes(md_bits // 8, "big")
        assert len(out) == (fi + 1) * size
    return dict(data=bytes(out), granules=G, coeffs=coef, log=np.array(log, LOG_DTYPE), plain=plain,
                md_bits=md_bits, n_frames=len(frames))


# ---------------------------------------------------------------------------
# the symbol classes of sets B and C
# ---------------------------------------------------------------------------
def _longest(tree, plain):
    best = None
    for k, (t, c, n, x, y) in enumerate(CODES):
        if t == tree and (not plain or (x < 15 and y < 15)) and (best is None or n > CODES[best][2]):
            best = k
    return best


def symbol_classes():
    """[(name, table, values, bits)]: the widest symbol of every linbits
    table, the longest plain codeword of trees 13, 15, 16, 24 (in tables 13,
    15, 16, 24) and the longest quad of each count1 table."""
    out = []
    for t in LINBITS_TABLES:
        m = 15 + (1 << LINBITS[t]) - 1
        n = CODES[CODE_OF[(TREE[t], 15, 15)]][2] + 2 * LINBITS[t] + 2
        out.append((f"wide{t}", t, (-m, -m), n))
    # (wide23 is the longest symbol there is: 36 bits = 8 + 2 * 13 + 2.  The (15, 15) codewords are short, so
    # the 19 + 2 * 14 = 47 bits that decode_sym's one-peek path is sized for are a bound no symbol attains.)
    assert max(_pair_bits(t, (x, y)) for t in LINBITS_TABLES for x in list(range(15)) + [15 + (1 << LINBITS[t]) - 1]
               for y in list(range(15)) + [15 + (1 << LINBITS[t]) - 1]) == 36
    for t in (13, 15, 16, 24):
        _, _, n, x, y = CODES[_longest(TREE[t], LINBITS[t] > 0)]
        out.append((f"long{t}", t, (-x, y), n + (x > 0) + (y > 0)))
    for t in (32, 33):
        n = max(c[2] + bin(c[4]).count("1") for c in CODES if c[0] == t)
        q = [c for c in CODES if c[0] == t and c[2] + bin(c[4]).count("1") == n][0][4]
        out.append((f"quad{t}", t, tuple((-1) ** i * ((q >> (3 - i)) & 1) for i in range(4)), n))
    return out


def _class_gc(cls, n, gain=120, **kw):
    name, t, vals, _ = cls
    if t >= 32:
        return gc(quads=[vals] * n, c1sel=t - 32, gain=gain, **kw)
    return gc(pairs=[vals] * n, tables=(t, t, t), r0=15, r1=7, gain=gain, **kw)


# ---------------------------------------------------------------------------
# set A: every codeword
# ---------------------------------------------------------------------------
def _all_pairs(rng):
    """{table: [(x, y)]}: every leaf, every escape extreme, shuffled."""
    out = {}
    sgn = lambda: int(rng.integers(0, 2)) * 2 - 1
    for t in PAIR_TABLES:
        lb = LINBITS[t]
        side = 1 + max(c[3] for c in CODES if c[0] == TREE[t])
        esc = sorted({0, 1, (1 << lb) - 2, (1 << lb) - 1}) if lb else []
        ps = []
        for x in range(side):
            for y in range(side):
                ex, ey = lb and x == 15, lb and y == 15
                if not ex and not ey:
                    ps.append((x * sgn(), y * sgn()))
                elif ex and ey:
                    ps += [(sx * (15 + a), sy * (15 + b)) for a in esc for b in esc for sx in (1, -1) for sy in (1, -1)]
                elif ex:
                    ps += [(sx * (15 + a), y * sgn()) for a in esc for sx in (1, -1)]
                else:
                    ps += [(x * sgn(), sy * (15 + b)) for b in esc for sy in (1, -1)]
        rng.shuffle(ps)
        out[t] = ps
    return out


def _pair_bits(t, p):
    lb = LINBITS[t]
    cx = [min(abs(v), 15) if lb else abs(v) for v in p]
    return CODES[CODE_OF[(TREE[t], cx[0], cx[1])]][2] + sum(lb * (c == 15 and lb > 0) + (v != 0) for c, v in zip(cx, p))


def set_a_frames(seed):
    rng = np.random.default_rng(seed)
    full = _all_pairs(rng)
    queue = {t: list(ps) for t, ps in full.items()}
    quads = {s: [tuple(int(v) for v in q) for q in
                 np.array(np.meshgrid(*[[-1, 0, 1]] * 4)).reshape(4, -1).T[rng.permutation(81)]] for s in (0, 1)}
    gcs = []
    while any(queue.values()) or any(quads.values()):
        budget = int(rng.integers(500, 3500)) if len(gcs) % 2 == 0 else 4000 - gcs[-1][1]
        block = [LONG, LONG, LONG, START, STOP, SHORT, MIXED][int(rng.integers(0, 7))]
        sfc = int(rng.integers(0, 16))
        live = [t for t in PAIR_TABLES if queue[t]]
        rng.shuffle(live)
        tables = tuple((live + [1, 1, 1])[:3])
        spec = gc(tables=tables, r0=int(rng.integers(0, 16)), r1=int(rng.integers(0, 8)), block=block, sfc=sfc,
                  c1sel=len(gcs) // 2 % 2, gain=int(rng.integers(90, 121)), sfscale=int(rng.integers(0, 2)),
                  sbg=tuple(int(v) for v in rng.integers(0, 8, 3)) if block != LONG else (0, 0, 0))
        fields = sf_fields(spec, False, 0, (0,) * 4)  # (no scfsi in set A: every granule carries its own)
        spec["sf"] = [int(rng.integers(0, 1 << w)) for w, _ in fields]
        bits = sum(w for w, _ in fields)
        take = quads[spec["c1sel"]][:12]
        bits += sum(6 + 4 for _ in take)  # an upper bound of the quads' bits
        r1s, r2s = region_starts(spec, False)
        while len(spec["pairs"]) < 288 - 2 * len(take):
            k = 2 * len(spec["pairs"])
            t = tables[0 if k < r1s else 1 if k < r2s else 2]
            if queue[t]:
                p = queue[t][-1]
            elif any(queue[u] for u in tables[(0 if k < r1s else 1 if k < r2s else 2) + 1:]):
                p = full[t][int(rng.integers(0, len(full[t])))]  # fill the region up to the next table's
            else:
                break
            if bits + _pair_bits(t, p) > budget:
                break
            bits += _pair_bits(t, p)
            if queue[t]:
                queue[t].pop()
            spec["pairs"].append(p)
        spec["quads"] = take
        del quads[spec["c1sel"]][:12]
        gcs.append((spec, bits))
    if len(gcs) % 2:
        gcs.append((gc(), 0))
    if len(gcs) % 4:
        gcs += [(gc(), 0), (gc(), 0)]
    specs = [s for s, _ in gcs]
    return [frame([[specs[i], specs[i + 1]], [specs[i + 2], specs[i + 3]]]) for i in range(0, len(specs), 4)]


def set_a(seed=1):
    return write_stream(set_a_frames(seed), bitrate_index=14)


def set_a_long(seeds=(1, 2, 3)):
    return write_stream([f for s in seeds for f in set_a_frames(s)], bitrate_index=14)


# ---------------------------------------------------------------------------
# set B: every phase of the reader's window
# ---------------------------------------------------------------------------
def set_b(bitrate_index=3):
    """-> (stream, cls[n]: the class index of granule n's channel 1).  Channel
    0 is the shift that puts channel 1's first symbol on phase k.  At 48 kbps
    a 256-job block of the kernel spans 960 words and is staged in LDS; at
    320 kbps (bitrate_index 14) it spans 8,064 and only the wide stage holds it."""
    md_bits = main_data_bits(False, bitrate_index)
    grans, cls, pos = [], [], 0
    for ci, c in enumerate(symbol_classes()):
        for k in range(64):
            if len(grans) % 2 == 0:
                pos = len(grans) // 2 * md_bits  # a new frame
            s = (k - pos) % 64
            grans.append([shift(s), _class_gc(c, 3)])
            cls.append(ci)
            pos += s + 3 * c[3]
    frames = [frame([grans[i], grans[i + 1]]) for i in range(0, len(grans), 2)]
    return write_stream(frames, bitrate_index=bitrate_index), np.array(cls)


# ---------------------------------------------------------------------------
# set C: symbols cut by the end of the buffer or of their part
# ---------------------------------------------------------------------------
def set_c():
    """-> (stream, meta[frame] = (class index, kind, bits of the cut symbol
    before the end)); the class is the frame's last granule-channel."""
    frames, meta = [], []
    md_bits = 544
    empty = lambda: [gc(), gc()]
    lead = [(1, -1), (0, 1)]  # the "few pairs" in front of a quad class, table 1
    lead_bits = sum(_pair_bits(1, p) for p in lead)
    for ci, c in enumerate(symbol_classes()):
        name, t, vals, L = c
        for k in range(64):
            # kinds 1 and 2: the symbols run into the end of the buffer
            if t < 32:
                start = k
                spec = _class_gc(c, (md_bits - start) // L + 1, bv=288, p23=4095)
            else:
                start = k + lead_bits
                spec = _class_gc(c, (md_bits - start) // L + 1, p23=4095)
                spec["pairs"] = list(lead)
            frames.append(frame([empty(), [shift(k), spec]]))
            meta.append((ci, 1 if t < 32 else 2, (md_bits - start) % L))
            # kind 3: part2_3_length ends inside the last symbol, the data goes on
            cut = 1 + k % (L - 1)
            spec = _class_gc(c, 3, p23=(lead_bits if t >= 32 else 0) + 2 * L + cut)
            if t >= 32:
                spec["pairs"] = list(lead)
            frames.append(frame([empty(), [shift(k), spec]]))
            meta.append((ci, 3, cut))
    return write_stream(frames, bitrate_index=1), np.array(meta)


# ---------------------------------------------------------------------------
# set D: row geometry
# ---------------------------------------------------------------------------
def set_d():
    """-> (stream, cases[(granule, channel, big_values, quads)])."""
    grans, cases = [], []
    # (the two extra cases end their quads at line 572 for want of bits, where the limit would allow one more)
    for n, bv in enumerate(list(range(289)) + [284, 283]):
        ch = n & 1
        pairs = [((-1) ** (k // 3) * (1 + k % 7), (-1) ** (k // 2) * (1 + k % 5)) for k in range(bv)]
        nq = (572 - 2 * bv) // 4 + 1 if 2 * bv <= 572 else 0
        if bv % 5 == 4:
            nq = min(nq, 1 + bv % 7)
        if n >= 289:
            nq -= 1
        quads = [tuple((1 - 2 * ((k >> (i + 1)) & 1)) * (((k % 15 + 1) >> (3 - i)) & 1) for i in range(4))
                 for k in range(nq)]
        case = gc(pairs=pairs, quads=quads, tables=(13, 15, 24), r0=7 + bv % 5, r1=bv % 8, c1sel=(bv >> 1) & 1,
                  gain=150, sfc=bv % 16, sf="pos")
        filler = gc(pairs=[(1, -2), (0, 3)], tables=(7, 7, 7), gain=150)
        cases.append((len(grans), ch, bv, nq))
        grans.append([filler, case] if ch else [case, filler])
    grans.append([gc(), gc()])
    frames = [frame([grans[i], grans[i + 1]]) for i in range(0, len(grans), 2)]
    return write_stream(frames, bitrate_index=14), np.array(cases)


# ---------------------------------------------------------------------------
# set E: scale factors
# ---------------------------------------------------------------------------
_FEW = dict(pairs=[(1, -2), (3, 0), (-4, 5)], tables=(7, 7, 7), gain=170)


def set_e_mpeg1():
    """-> (stream, combos[granule][ch] = 4 * scalefac_compress + kind, or -1)."""
    kinds = [LONG, START, SHORT, MIXED]
    frames, combos = [], []
    for sf in ("max", "pos"):
        for i in range(64):
            gr = []
            for pos in range(4):  # every combination in every (granule, channel)
                c = (i + 17 * pos) % 64
                gr.append(gc(block=kinds[c & 3], sfc=c >> 2, sf=sf, sbg=(pos, 1, 2) if c & 3 else (0, 0, 0),
                             preflag=i & 1, sfscale=(i >> 1) & 1, **_FEW))
                combos.append(c)
            frames.append(frame([gr[:2], gr[2:]]))
    for g0 in (LONG, SHORT, MIXED):
        for m in range(16):
            bits = lambda v: tuple((v >> k) & 1 for k in range(4))
            frames.append(frame([[gc(block=g0, sfc=13, sf="pos", **_FEW), gc(block=g0, sfc=15, sf="max", **_FEW)],
                                 [gc(sfc=15, sf="max", **_FEW), gc(sfc=10, sf="pos", **_FEW)]],
                                scfsi=(bits(m), bits(15 - m))))
            combos += [-1] * 4
    return write_stream(frames, bitrate_index=7), np.array(combos).reshape(-1, 2)


def set_e_mpeg2():
    frames = []
    for sf in ("max", "pos"):
        for i in range(512):
            for kind, other in ((LONG, SHORT), (SHORT, LONG)):
                frames.append(frame([[gc(block=kind, sfc=i, sf=sf, **_FEW),
                                      gc(block=other, sfc=511 - i, sf=sf, **_FEW)]]))
    st = write_stream(frames, lsf=True, bitrate_index=3)
    # one intensity-stereo frame (joint stereo, mode extension 1): the same layout
    is_frame = write_stream([frame([[gc(sfc=273, sf="pos", **_FEW), gc(sfc=499, sf="pos", **_FEW)]])], lsf=True,
                            bitrate_index=3, mode=1, mode_ext=1)
    for key in ("granules", "coeffs", "plain"):
        st[key] = np.concatenate([st[key], is_frame[key]])
    lg = is_frame["log"].copy()
    lg["g"] += len(st["granules"]) - 1
    st["log"] = np.concatenate([st["log"], lg])
    st["data"] += is_frame["data"]
    st["n_frames"] += 1
    return st


def spread(st, frames, piece=8, filler=30):
    """A batch that keeps small frames out of the kernel's smaller LDS stages.
    Every frame has main_data_begin = 0, so any run of whole frames is a
    stream of its own: the chosen frames of `st` in pieces of `piece`, each
    followed by a stream of `filler` empty 320 kbps frames (1,008 bytes of
    main data each, no bits used).  Any 256 consecutive jobs then span more
    than 5,376 words of main data.  -> (datas, is_piece[stream])"""
    size = len(st["data"]) // st["n_frames"]
    empty = write_stream([frame([[gc(), gc()], [gc(), gc()]])] * filler, bitrate_index=14)["data"]
    datas, is_piece = [], []
    for i in range(0, len(frames), piece):
        datas.append(b"".join(st["data"][f * size:(f + 1) * size] for f in frames[i:i + piece]))
        datas.append(empty)
        is_piece += [True, False]
    return datas, np.array(is_piece)


def spread_cuts():
    """The frames of set C that hold the widest symbols (tables 23 and 31), the
    longest plain codeword (tree 13) and the two quad classes, spread():
    640 frames in 80 pieces, 160 streams, 2,572,160 bytes."""
    st, meta = directed_set("C")
    names = [c[0] for c in symbol_classes()]
    keep = [names.index(n) for n in ("wide23", "wide31", "long13", "quad32", "quad33")]
    frames = np.nonzero(np.isin(meta[:, 0], keep))[0]
    return spread(st, frames.tolist()) + (frames,)


_SETS = {}


def directed_set(name):
    """The sets by name, generated once per process and shared (read-only) by
    the tests: A1, A2, A3 (one seed each), A_long, B, B320, C, D, E1, E2 ->
    (stream, the set's own table or None)."""
    if name not in _SETS:
        make = {"A1": lambda: (set_a(1), None), "A2": lambda: (set_a(2), None), "A3": lambda: (set_a(3), None),
                "A_long": lambda: (set_a_long((1, 2, 3)), None), "B": set_b, "B320": lambda: set_b(14), "C": set_c,
                "D": set_d,
                "E1": set_e_mpeg1, "E2": lambda: (set_e_mpeg2(), None)}[name]
        st, extra = make()
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SETS[name] = (st, extra)
    return _SETS[name]


SET_NAMES = ("A1", "A2", "A3", "A_long", "B", "B320", "C", "D", "E1", "E2")
