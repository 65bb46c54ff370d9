"""Sample-windowed decode, host side (include/mp3g.h "sample-windowed
decode"), checked on the CPU.

* The layout (lead, skip, n_valid) and the decoded run of a window equal the
  rule written out in numpy (tests/windows_ref.py) on the full scan's headers.
* The windowed scan's jobs and main data, decoded by the host build of the
  device job decoder (tests/native/hjob_host.hip), give the coefficient rows
  and descriptors of the host parse byte for byte -- for a window at every
  frame of streams that use the bit reservoir up to its 511-byte limit: the
  scanner restarted behind a 511-byte pre-roll sees the full scan's bit
  buffers.
* The scan is windowed: its main data is the window frames' own plus the
  pre-roll, not the file.
* Early ends, the fuzz corpus, gapless starts and the argument checks of the
  windowed plan calls (no device needed).
"""
import ctypes as C
import os

import numpy as np
import pytest

import mp3g
from mp3g import synth
from test_oracle_kats import GOLDEN
from test_parse_cpu import mutations
from test_scan_cpu import hjob_host  # noqa: F401  (fixture)
from windows_ref import layout, starts_for, switching_lsf_stream, switching_stream

T_VALUES = (1, 576, 577, 3000)


def _layout_streams(sample_files):
    return {
        "mpeg1": synth.encode_stream(11, 40),
        "mpeg2": synth.encode_stream(12, 40, lsf=True),
        "mono": synth.encode_stream(13, 40, mode=synth.MODE_MONO),
        "switching": switching_stream(),
        "switching-lsf": switching_lsf_stream(),
        "classic_lame.mp3": sample_files["classic_lame.mp3"],
        "mpeg2.mp3": sample_files["mpeg2.mp3"],
    }


def _check_layout(data, full, start, T, w, k=0, what=""):
    """Row k of the windowed scan `w` against the rule on the full scan `full` of a clean stream."""
    hdr = full["granules"]["header"]
    h, n, lead, skip, n_valid = layout(hdr, start, T)
    row, st = w["rows"][k], w["streams"][k]
    assert (int(row["lead"]), int(row["skip"]), int(row["n_valid"])) == (lead, skip, n_valid), (what, start, T, row)
    assert int(st["n_granules"]) == n, (what, start, T)
    f = int(st["first_granule"])
    assert np.array_equal(w["granules"]["header"][f:f + n], hdr[h:h + n]), (what, start, T)
    want = int(full["end_status"][0]) if start + T > 576 * len(hdr) else 0
    assert int(w["end_status"][k]) == want, (what, start, T, w["end_status"][k])
    return h, n


def test_layout(sample_files):
    for name, data in _layout_streams(sample_files).items():
        full = mp3g.scan_streams([data])
        N = 576 * len(full["granules"])
        assert N > 0 and full["end_status"][0] == 7, name
        starts = starts_for(N)
        if name.startswith("switching"):
            starts += list(range(0, N, 576 * 3 + 100))  # windows in every run of the stream
        for T in T_VALUES:
            w = mp3g.scan_windows([data] * len(starts), starts, T, n_threads=2)
            for k, start in enumerate(starts):
                _check_layout(data, full, start, T, w, k, name)
            if name == "mono":
                assert int(w["rows"]["lead"].max()) <= 2  # no stereo granule: never the whole prefix


WINDOW_CASES = {
    "reservoir-full": dict(fill=1.3),
    "mixed+is": dict(p_mixed=0.3, p_event=0.1, p_is=0.5),
    "mpeg2": dict(lsf=True, p_event=0.1),
    "mono+linbits": dict(mode=synth.MODE_MONO, p_big=0.02),
}


def _frame_table(full):
    """Per frame of a single-stream full scan: (first granule, main-data bytes)."""
    gr = full["granules"]["gr"]
    first = np.nonzero(gr == 0)[0]
    end = full["jobs"]["bit_end"][0::2][first].astype(np.int64) // 8  # cumulative main data after the frame
    return first, np.diff(np.concatenate([[0], end]))


def _windows_equal_parse(hjob, data, starts, T, what):
    """The windowed scans (one per start) decode to the host parse's rows; returns the scan."""
    g2, c2, end = mp3g.parse_stream(data)
    full = mp3g.scan_streams([data])
    w = mp3g.scan_windows([data] * len(starts), starts, T, n_threads=4)
    n = len(w["granules"])
    want_g, want_c = [], []
    for k, start in enumerate(starts):
        h, cnt = _check_layout(data, full, start, T, w, k, what)
        want_g.append(g2[h:h + cnt])
        want_c.append(c2[h:h + cnt])
    want_g, want_c = np.concatenate(want_g), np.concatenate(want_c)
    assert len(want_g) == n
    for stage_words in (None, 960, 64):
        g = w["granules"].copy()
        c = np.full((n, 2, 576), 0x5A5A, np.int16)
        args = (w["jobs"].ctypes.data, n, w["main_data"].ctypes.data, g.ctypes.data, c.ctypes.data)
        rc = hjob.hjob_decode_host(*args) if stage_words is None else hjob.hjob_decode_host_staged(*args, stage_words)
        assert rc == 0
        assert g.tobytes() == want_g.tobytes(), f"{what} (stage {stage_words}): descriptors differ"
        assert np.array_equal(c, want_c), f"{what} (stage {stage_words}): coefficients differ"
    return full


def _check_windowed_size(data, full, starts, T, what):
    """Main data of each single-stream windowed scan <= its window frames' own + 511 + 1,500 + 16."""
    first, mdb = _frame_table(full)
    hdr = full["granules"]["header"]
    for start in starts:
        h, n, *_ = layout(hdr, start, T)
        if n == 0:
            continue
        fa = np.searchsorted(first, h, side="right") - 1
        fb = np.searchsorted(first, h + n - 1, side="right") - 1
        own = int(mdb[fa:fb + 1].sum())
        w = mp3g.scan_windows([data], [start], T)
        assert len(w["main_data"]) <= own + 511 + 1500 + 16, (what, start, len(w["main_data"]), own)
        assert len(w["main_data"]) >= own


@pytest.mark.parametrize("case", sorted(WINDOW_CASES))
def test_windowed_scan_equals_full_parse(hjob_host, case):  # noqa: F811
    # (seed 1: its reservoir-full stream reaches main_data_begin = 498 of the 511 possible)
    data = synth.encode_stream(1 if case == "reservoir-full" else 3, 120, **WINDOW_CASES[case])
    full = mp3g.scan_streams([data])
    first, _ = _frame_table(full)
    if case == "reservoir-full":  # the case the pre-roll rule exists for
        mdb = np.frombuffer(data, np.uint8)
        assert max((int(mdb[o + 4]) << 1) | (int(mdb[o + 5]) >> 7) for o in _frame_offsets(data)) > 480
    starts = [576 * int(g) for g in first]  # a window at every frame
    assert len(starts) == 120
    _windows_equal_parse(hjob_host, data, starts, 3 * 576, case)
    _check_windowed_size(data, full, starts, 3 * 576, case)


def _frame_offsets(data):
    """Byte offsets of the frames of a synthetic MPEG-1 128 kbps CBR stream."""
    off, out = 0, []
    while off + 4 <= len(data):
        h = int.from_bytes(data[off:off + 4], "big")
        assert h >> 21 == 0x7FF
        out.append(off)
        off += 144 * 128000 // 44100 + ((h >> 9) & 1)
    return out


@pytest.mark.parametrize("name", ["classic_lame.mp3", "mpeg2.mp3"])
def test_windowed_scan_sample_files(hjob_host, sample_files, name):  # noqa: F811
    data = sample_files[name]
    full = mp3g.scan_streams([data])
    first, _ = _frame_table(full)
    starts = [576 * int(g) for g in first[::7]]
    _windows_equal_parse(hjob_host, data, starts, 3 * 576, name)
    _check_windowed_size(data, full, starts, 3 * 576, name)


def test_unaligned_windows_equal_parse(hjob_host):  # noqa: F811
    """Windows that start and end inside granules and inside MPEG-1 frames (a
    run may begin with a frame's second granule), and the switching streams."""
    for what, data in (("joint", synth.encode_stream(21, 60, fill=1.3)), ("switching", switching_stream()),
                       ("switching-lsf", switching_lsf_stream())):
        N = 576 * len(mp3g.scan_streams([data])["granules"])
        starts = list(range(0, N, 576 + 97))
        for T in (1, 577, 1153):
            _windows_equal_parse(hjob_host, data, starts, T, what)


def _expect_like_full(data, start, T, what):
    """A window whose decoded range holds the stream's end: lengths and status as the full scan's."""
    full = mp3g.scan_streams([data])
    w = mp3g.scan_windows([data], [start], T)
    h, n, lead, skip, n_valid = layout(full["granules"]["header"], start, T)
    row = w["rows"][0]
    assert (int(row["lead"]), int(row["skip"]), int(row["n_valid"])) == (lead, skip, n_valid), (what, row)
    assert int(w["streams"][0]["n_granules"]) == n, what
    assert int(w["end_status"][0]) == int(full["end_status"][0]), (what, w["end_status"], full["end_status"])
    return full, w


def test_early_ends():
    data = synth.encode_stream(31, 40, fill=1.3)
    offs = _frame_offsets(data)
    # the file cut inside a window frame's main data
    cut = data[:offs[20] + 150]
    full, w = _expect_like_full(cut, 576 * 36, 8 * 576, "cut")
    assert len(full["granules"]) == 40 and int(w["rows"][0]["n_valid"]) == 4 * 576
    # a corrupted header inside the window: both scans resynchronise (or end) alike
    bad = bytearray(data)
    bad[offs[20]] = 0x00
    bad[offs[20] + 1] = 0x00
    full, w = _expect_like_full(bytes(bad), 576 * 36, 60 * 576, "header")
    # side info the reference rejects inside the window (big_values > 288): the stream ends there
    bad = bytearray(data)
    # (main_data_begin 9 bits, private 3, scfsi 8, part2_3_length 12: big_values is bits 32..40)
    bad[offs[20] + 4 + 3] |= 0x01  # part2_3_length != 0
    bad[offs[20] + 4 + 4] = 0xFF
    bad[offs[20] + 4 + 5] |= 0x80
    full, w = _expect_like_full(bytes(bad), 576 * 36, 8 * 576, "side info")
    assert len(full["granules"]) == 40 and int(full["end_status"][0]) == 6  # frames 0..19, then the error
    # starts beyond the end: nothing, and the stream's end status
    N = 576 * 80
    for start in (N, N + 1, N + 10 ** 9, 2 ** 63):
        w = mp3g.scan_windows([data], [start], 3000)
        assert int(w["rows"][0]["n_valid"]) == 0 and int(w["streams"][0]["n_granules"]) == 0
        assert int(w["end_status"][0]) == 7 and len(w["granules"]) == 0


def _check_consistent(datas, what):
    """Hostile input: the scan returns, every row is self-consistent, and a
    window the full scan covers is the full scan's."""
    fulls = [mp3g.scan_streams([d]) for d in datas]
    for frame in (0, 1, 5):
        for T in (1153, 3000):
            starts = [576 * frame * (1 if len(f["granules"]) and (f["granules"]["header"][0] >> 19) & 1 == 0 else 2)
                      for f in fulls]
            w = mp3g.scan_windows(datas, starts, T, n_threads=4)
            for k, (d, f) in enumerate(zip(datas, fulls)):
                row, st, end = w["rows"][k], w["streams"][k], int(w["end_status"][k])
                n, lead, skip, nv = int(st["n_granules"]), int(row["lead"]), int(row["skip"]), int(row["n_valid"])
                assert end in (0, 6, 7, 8), (what, k, end)
                assert lead <= n and skip < 576 and nv <= T and (n - lead) * 576 - skip >= nv, (what, k, row, n)
                assert (nv == 0) == (n == 0), (what, k)
                G = len(f["granules"])
                if frame == 0 or 576 * G >= starts[k] + T:
                    # no frame in front of the scanned range, or none the full scan rejects
                    h, n2, lead2, skip2, nv2 = layout(f["granules"]["header"], starts[k], T)
                    assert (n, lead, skip, nv) == (n2, lead2, skip2, nv2), (what, k, frame, T)
                    assert end == (int(f["end_status"][0]) if starts[k] + T > 576 * G else 0), (what, k, frame, T)


def test_fuzz_corpus_and_mutations(sample_files):
    d = os.path.join(GOLDEN, "fuzz")
    _check_consistent([open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))], "fuzz")
    for name in ("classic_lame.mp3", "mpeg2.mp3"):
        rng = np.random.default_rng(77 + len(name))
        _check_consistent(mutations(sample_files[name][:60000], rng, 60), name)


def test_gapless(sample_files):
    data = sample_files["classic_lame.mp3"]
    full = mp3g.scan_streams([data])
    G = len(full["granules"])
    info, _ = mp3g.lame_parse_reader(data[data.index(b"\xff\xfb"):])
    assert info.encoder_delay == 576
    first, count = info.trim(576 * G, 1152)
    assert first == 1152 + 576 + 529 and 0 < count < 576 * G - first
    for start, T in ((0, 3000), (1, 576), (count - 100, 3000), (count, 10), (count + 5, 10)):
        w = mp3g.scan_windows([data], [start], T, gapless=True)
        s2 = first + min(start, count)
        want_valid = max(0, min(T, first + count - s2))
        row = w["rows"][0]
        if want_valid == 0:
            assert int(row["n_valid"]) == 0 and int(w["streams"][0]["n_granules"]) == 0
            continue
        h, n, lead, skip, _ = layout(full["granules"]["header"], s2, want_valid)
        assert (int(row["lead"]), int(row["skip"]), int(row["n_valid"])) == (lead, skip, want_valid), (start, T, row)
        assert int(w["streams"][0]["n_granules"]) == n
        assert np.array_equal(w["granules"]["header"], full["granules"]["header"][h:h + n])
    # an untagged stream: as if the flag were off
    plain = synth.encode_stream(5, 40)
    a = mp3g.scan_windows([plain], [1000], 3000, gapless=True)
    b = mp3g.scan_windows([plain], [1000], 3000)
    for key in ("rows", "streams", "end_status", "granules", "jobs", "main_data"):
        assert a[key].tobytes() == b[key].tobytes(), key
    # per-stream flags in one call
    w = mp3g.scan_windows([data, data], [0, 0], 3000, gapless=[True, False])
    assert int(w["rows"][0]["skip"]) == first % 576 and int(w["rows"][1]["skip"]) == 0


def test_argument_checks_need_no_device():
    L = mp3g.lib()
    plan = C.c_void_p()
    streams = mp3g.streams_for([4])
    rows = np.zeros(1, mp3g.WINDOW_ROW_DTYPE)
    rows["n_valid"] = 576
    # MP3G_FLAG_KERNEL_V2 plans: unsupported, before any device call
    for mode in (mp3g.MODE_EXACT | mp3g.FLAG_KERNEL_V2,):
        st = L.mp3g_plan_create_windows(0, streams.ctypes.data, rows.ctypes.data, 1, 576, 0, mode, C.byref(plan))
        assert st == 8 and not plan.value
    # the execute call checks the format before it looks at the plan
    for fmt in (mp3g.OUT_S16, mp3g.OUT_F32, mp3g.OUT_S16_MONO):
        assert L.mp3g_plan_execute_windows(None, None, None, None, fmt, None) == 8, fmt
    for fmt in (5, 6, 7, 16, 17, 99):
        assert L.mp3g_plan_execute_windows(None, None, None, None, fmt, None) == 1, fmt
    # (the two windowed formats get as far as the null plan)
    for fmt in (mp3g.OUT_F32_PLANAR, mp3g.OUT_F32_MONO):
        assert L.mp3g_plan_execute_windows(None, None, None, None, fmt, None) == 1, fmt
    # a row that would write outside [0, T), or past its decoded granules
    for field, value in (("n_valid", 577), ("skip", 576), ("lead", 5)):
        bad = rows.copy()
        bad[field] = value
        st = L.mp3g_plan_create_windows(0, streams.ctypes.data, bad.ctypes.data, 1, 576, 0, mp3g.MODE_EXACT,
                                        C.byref(plan))
        assert st == 1 and not plan.value, field
    bad = rows.copy()
    bad["lead"], bad["n_valid"] = 3, 577  # one granule behind the lead
    assert L.mp3g_plan_create_windows(0, streams.ctypes.data, bad.ctypes.data, 1, 1000, 0, mp3g.MODE_EXACT,
                                      C.byref(plan)) == 1
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.decode_windows_tensor([b""], [0], 10, out_format=mp3g.OUT_S16)
    assert e.value.status == 8
    with pytest.raises(mp3g.Mp3gError) as e:
        mp3g.decode_windows_tensor([b""], [0], 10, out_format=9)
    assert e.value.status == 1
    # the format table is unchanged: no output format 5, 6 or 7
    assert [mp3g.out_bytes_per_granule(f) for f in (5, 6, 7, 16, 17)] == [0] * 5
