"""A plain model of the fast mode's hot-zone recording (numpy and the oracle;
nothing of the GPU library but its constants and dtypes).

The fast kernel (granule_fast.hip) flags the hot granules of each chunk,
records the zones of granules whose PCM depends on them, cuts the zones into
pieces of kZonePiece granules and appends the pieces to the plan's zone list;
a second launch of the exact kernel decodes the list.
This module restates, per chunk, what that must produce -- zones, pieces and
the three counters of mp3g_plan_hot_stats -- from the granule headers, the
stream table, granules_per_chunk and the oracle's hybrid output:

  * plan_chunks: the chunk table (mp3g_abi.cpp plan_chunks: chunk i of cs
    covers [i n / cs, (i + 1) n / cs) of its stream);
  * replay_start: where a chunk's decode starts (granule_fast.hip prologue);
  * chunk_hot: the hot flags of a chunk's replay.  The kernel sees the S of
    the REPLAY -- the chunk's own decode from its replay start, from zero
    state or the stream's -- not of the serial decode: the first replayed
    granule has no overlap from the granule before it;
  * chunk_zones: record_hot / zone_end restated;
  * zone_pieces: the list entries of a chunk's zones.

The kernel takes its flags from the fast transforms' S and the model from the
oracle's, so the model refuses (by assertion) an input with any granule whose
governing ratio min(r_A, r_B) (tests/fast_edge_inputs.py) lies in BAND: the
two then agree on every flag and the counters are exact, not banded.
"""
import numpy as np

import mp3g
import oracle

K_ZONES = 8  # kernels.h kZoneListPerChunk: the zones a chunk records
K_PIECE = 16  # kernels.h kZonePiece
K_LIST_FLOOR = 64  # kernels.h zone_list_capacity: its smallest value
BAND = (0.9, 1.1)  # governing ratios the model refuses
STATE_IN, STATE_OUT = 1, 2  # kernels.h kChunkStateIn / kChunkStateOut


def nch_of(g):
    """Channels per granule (granule_hdr.h hdr_nch: mode 3 = mono)."""
    return np.where(((np.asarray(g["header"]) >> 6) & 3) == 3, 1, 2)


def chunks_per_stream(n, k):
    return (int(n) + int(k) - 1) // int(k)


def plan_chunks(streams, granules_per_chunk=None, counts=None):
    """The chunk table of mp3g_abi.cpp plan_chunks (:250-268) as a list of
    dicts (out_first, n_out, stream, stream_first, stream_n, flags): stream s
    in cs = ceil(n / granules_per_chunk) chunks (or counts[s] of them), chunk
    i covering [i n / cs, (i + 1) n / cs).  The cost model's chunking
    (granules_per_chunk = 0) depends on the device: pass the counts a plan
    reports instead.  (An empty stream's state pass-through chunk records
    nothing and is left out.)"""
    out = []
    for si, S in enumerate(streams):
        n, first, fl = int(S["n_granules"]), int(S["first_granule"]), int(S["flags"])
        cs = int(counts[si]) if counts is not None else chunks_per_stream(n, granules_per_chunk)
        off = 0
        for i in range(cs):
            if off >= n:
                break
            nxt = (i + 1) * n // cs
            flags = STATE_IN if fl & mp3g.STATE_IN else 0
            if (fl & mp3g.STATE_OUT) and nxt == n:
                flags |= STATE_OUT
            out.append(dict(out_first=first + off, n_out=nxt - off, stream=si, stream_first=first, stream_n=n,
                            flags=flags))
            off = nxt
    return out


def replay_start(nch, cd):
    """granule_fast.hip prologue, as the fast pass calls it (ch1_always):
    (w, from_in[2]) -- the first granule the chunk decodes and whether channel
    c starts from the stream's state_in (else from zero).

    A chunk at its stream's first granule starts there, from state_in if the
    stream has one.  Otherwise two granules back (clipped to the stream); and
    when one of those two is mono -- channel 1 was frozen across it (a mono
    granule leaves channel 1's state alone) -- back to the second-last stereo
    granule before the chunk, to the stream's start if there is only one, and
    with none channel 1 keeps the stream's entry state.  The fast pass does
    that whether or not the chunk has a stereo granule or exports state: what
    it needs is the hot flag of the stereo granule in front of the run, whose
    zone spans the run."""
    c0, s0, have_in = cd["out_first"], cd["stream_first"], bool(cd["flags"] & STATE_IN)
    if c0 == s0:
        return c0, (have_in, have_in)
    start0 = c0 - 2 if (c0 >= 2 and c0 - 2 > s0) else s0
    st1 = nch[c0 - 1] == 2
    st2 = nch[c0 - 2] == 2 if (c0 >= 2 and c0 - 2 >= s0) else False
    if st1 and st2:
        return start0, ((start0 == s0) and have_in,) * 2
    start1, ch1_from_in = c0, False
    stereo = np.nonzero(nch[s0:c0] == 2)[0] + s0
    if len(stereo) >= 2:
        start1 = int(stereo[-2])
    elif len(stereo) == 1:
        start1 = s0
    else:
        ch1_from_in = True
    w = min(start0, start1)
    in0 = (w == s0) and have_in
    return w, (in0, have_in if ch1_from_in else in0)


def zone_end(nch, g, end):
    """granule_fast.hip zone_end (:1053-1061): the end (exclusive, clipped to
    the chunk) of the granules whose PCM reads hot granule g's V: g + 2, or,
    g stereo and a mono run behind it, the first stereo granule after the run
    plus 1 (channel 1's V waits there)."""
    e = g + 2
    if nch[g] == 2:
        n = g + 1
        while n < end and nch[n] == 1:
            n += 1
        e = max(e, n + 1)
    return min(e, end)


def hot_ratios(g, c, first, n, state_in=None, hot_s=None, hot_l1=None):
    """(r_A, r_B) per granule of [first, first + n) decoded as a stream of its
    own (fast_edge_inputs.stream_ratios' quantities: max |S| / kHotS and the
    largest slot sum / kHotL1, channel 1 of a mono granule zeroed)."""
    hot_s = mp3g.FAST_HOT_S if hot_s is None else hot_s
    hot_l1 = mp3g.FAST_HOT_L1 if hot_l1 is None else hot_l1
    gg, cc = g[first:first + n], c[first:first + n]
    S = np.abs(oracle.hybrid_streams(gg, cc, mp3g.streams_for([n]), state_in)).reshape(n, 2, 32, 18)
    S[nch_of(gg) == 1, 1] = 0
    ra = S.max(axis=(1, 2, 3)).astype(np.float64) / hot_s
    rb = S.sum(axis=2, dtype=np.float64).max(axis=(1, 2)) / hot_l1
    return ra, rb


def chunk_hot(g, c, nch, cd, state_in=None):
    """(w, hot flags of [w, end), governing ratios of [w, end)): the chunk's
    replay run through the oracle's hybrid stages as a stream of its own."""
    w, from_in = replay_start(nch, cd)
    end = cd["out_first"] + cd["n_out"]
    st = None
    if state_in is not None and any(from_in):
        st = np.zeros(1, mp3g.STATE_DTYPE)
        for ch in range(2):
            if from_in[ch]:
                st["store"][0, ch] = state_in["store"][cd["stream"], ch]
                st["vvec"][0, ch] = state_in["vvec"][cd["stream"], ch]
    ra, rb = hot_ratios(g, c, w, end - w, st)
    gov = np.minimum(ra, rb)
    return w, gov > 1.0, gov


def chunk_zones(nch, cd, w, hot):
    """record_hot (granule_fast.hip :1070-1089) over the chunk's replay: the
    zones [zs, ze) and the number of flagged granules.

    A hot granule g whose V something reads (an output granule, the last
    replayed one, or a replayed one followed by a granule with fewer
    channels: the kernel's need_v, :1365-1366) is flagged and counted.  Its
    zone is [max(g, out_first), zone_end(g)); an empty one (a replayed granule
    whose V no output reads) records nothing.  A zone that starts at or before
    the last zone's end extends it; a ninth zone turns the eighth into "to the
    chunk end"."""
    out_first, end = cd["out_first"], cd["out_first"] + cd["n_out"]
    zones, flagged = [], 0
    for g in (np.nonzero(hot)[0] + w).tolist():
        if g + 1 < out_first and not nch[g + 1] < nch[g]:
            continue  # need_v false: its V feeds nothing, the kernel does not test it further
        flagged += 1
        zs, ze = max(g, out_first), zone_end(nch, g, end)
        if zs >= ze:
            continue
        if zones and zs <= zones[-1][1]:
            zones[-1][1] = max(ze, zones[-1][1])
        elif len(zones) < K_ZONES:
            zones.append([zs, ze])
        else:
            zones[-1][1] = end
    return [tuple(z) for z in zones], flagged


def zone_pieces(cd, zones):
    """The list entries of a chunk's zones (granule_fast.hip, after the
    granule loop): each zone in steps of K_PIECE, as (first, n, flags); the
    piece that ends a state-exporting chunk carries the state-out flag."""
    end = cd["out_first"] + cd["n_out"]
    out = []
    for zs, ze in zones:
        for ps in range(zs, ze, K_PIECE):
            pe = min(ps + K_PIECE, ze)
            out.append((ps, pe - ps, (cd["flags"] & STATE_IN) | ((cd["flags"] & STATE_OUT) if pe == end else 0)))
    return out


def zone_list_capacity(n_outs):
    """kernels.h zone_list_capacity, restated."""
    cap = sum(K_ZONES + (int(n) + K_PIECE - 1) // K_PIECE for n in n_outs)
    return max(cap, K_LIST_FLOOR)


def model(g, c, streams, granules_per_chunk=None, counts=None, state_in=None):
    """What the fast kernel must record for the plan of (streams,
    granules_per_chunk or counts).  Returns a dict:
      chunks     the chunk table (plan_chunks)
      zones      per chunk the zones [(zs, ze)]
      pieces     per chunk the pieces [(first, n, flags)]
      mask       bool [n granules]: PCM rewritten by the zone launch
      rewritten, zones_total, hot   the counters of mp3g_plan_hot_stats
                 (kernels.h kHotCounters [0], [1], [2])
      state_exact bool [n streams]: the stream's last zone reaches its end in
                 a state-exporting chunk (the zone launch rewrites the state)
      min_dist   the least |ratio - 1| over every granule of every replay
    Asserts that no governing ratio lies in BAND."""
    nch = nch_of(g)
    chunks = plan_chunks(streams, granules_per_chunk, counts)
    mask = np.zeros(len(g), bool)
    res = dict(chunks=chunks, zones=[], pieces=[], mask=mask, rewritten=0, zones_total=0, hot=0,
               state_exact=np.zeros(len(streams), bool), min_dist=np.inf)
    for cd in chunks:
        w, hot, gov = chunk_hot(g, c, nch, cd, state_in)
        bad = (gov > BAND[0]) & (gov < BAND[1])
        assert not bad.any(), f"chunk at {cd['out_first']}: governing ratio {gov[bad][0]:.4f} of granule " \
                              f"{w + int(np.nonzero(bad)[0][0])} inside the refused band"
        res["min_dist"] = min(res["min_dist"], float(np.abs(gov - 1.0).min()))
        zones, flagged = chunk_zones(nch, cd, w, hot)
        res["zones"].append(zones)
        res["pieces"].append(zone_pieces(cd, zones))
        res["hot"] += flagged
        res["zones_total"] += len(zones)
        for zs, ze in zones:
            mask[zs:ze] = True
            res["rewritten"] += ze - zs
        end = cd["out_first"] + cd["n_out"]
        if (cd["flags"] & STATE_OUT) and zones and zones[-1][1] == end:
            res["state_exact"][cd["stream"]] = True
    return res


def zones_from_flags(nch, cd, hot_abs):
    """chunk_zones for hot flags given per absolute granule index (the
    capacity tests draw flags instead of content)."""
    w, _ = replay_start(nch, cd)
    end = cd["out_first"] + cd["n_out"]
    return chunk_zones(nch, cd, w, hot_abs[w:end])
