"""Mono downmix output formats (MP3G_OUT_S16_MONO / MP3G_OUT_F32_MONO) and the
format-aware pipelined call (mp3g_decode_streams_into_out), the part that
needs no GPU: the export under ABI 5, the sizes, and the format checks that
come before any device call."""
import ctypes as C
import re
import subprocess

import numpy as np

import mp3g


def test_symbol_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", mp3g.lib_path()], text=True)
    exported = set(re.findall(r" T (mp3g_\w+)", out))
    assert "mp3g_decode_streams_into_out" in exported
    assert "mp3g_decode_streams_into" in exported  # (the old entry point stays)


def test_abi_version_unchanged():
    assert hasattr(mp3g.lib(), "mp3g_decode_streams_into_out")
    assert mp3g.lib().mp3g_abi_version() == 5


def test_out_bytes_per_granule():
    assert (mp3g.OUT_S16_MONO, mp3g.OUT_F32_MONO) == (3, 4)
    assert [mp3g.out_bytes_per_granule(f) for f in (3, 4)] == [1152, 2304]
    assert mp3g.out_bytes_per_granule(7) == 0


def _into_out(datas, out_ptr, fmt, cap):
    bufs, ptrs, lens = mp3g._stream_args(datas)
    streams = np.zeros(len(datas), mp3g.STREAM_DTYPE)
    status = np.zeros(len(datas), np.int32)
    n = C.c_uint64(12345)
    rc = mp3g.lib().mp3g_decode_streams_into_out(0, len(datas), ptrs, lens, 1, mp3g.MODE_EXACT, 0, out_ptr, fmt, cap,
                                                 C.byref(n), streams.ctypes.data, status.ctypes.data)
    return rc, n.value


def test_streams_into_out_refuses_unknown_format_without_a_device(sample_files):
    """Format 7 is MP3G_ERR_INVALID_ARGUMENT before anything touches a device
    (this test runs where there is none), whatever the buffer holds."""
    datas = [sample_files["classic_lame.mp3"]]
    out = np.zeros(1000 * 2304, np.uint8)
    rc, _ = _into_out(datas, out.ctypes.data, 7, 1000)
    assert rc == 1  # MP3G_ERR_INVALID_ARGUMENT
    assert b"format" in mp3g.lib().mp3g_last_error()
    assert not out.any()
    # the binding refuses it too
    try:
        mp3g.decode_streams_into(datas, np.zeros(1152, np.int16), out_format=7)
    except mp3g.Mp3gError as e:
        assert e.status == 1
    else:
        raise AssertionError("format 7 was accepted")


def test_streams_into_out_capacity_check_in_mono_slots(sample_files):
    """The capacity is counted in granule slots of the format: too few slots
    give MP3G_ERR_INVALID_ARGUMENT with the need, before any device call."""
    datas = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for fmt in (mp3g.OUT_S16, mp3g.OUT_S16_MONO, mp3g.OUT_F32_MONO):
        rc, need = _into_out(datas, None, fmt, 0)
        assert rc == 1 and need == 770 + 2872, fmt
        assert b"format" not in mp3g.lib().mp3g_last_error()


def test_decode_host_out_accepts_mono_format_past_the_format_check():
    """mp3g_decode_host_out with MP3G_OUT_S16_MONO gets past the format check:
    where there is no device it fails later, with a device status."""
    g = np.zeros(2, mp3g.GRANULE_DTYPE)
    c = np.zeros((2, 2, 576), np.int16)
    s = mp3g.streams_for([2])
    out = np.zeros((2, 576), np.int16)
    L = mp3g.lib()
    st = L.mp3g_decode_host_out(0, g.ctypes.data, c.ctypes.data, 2, s.ctypes.data, 1, None, None,
                                out.ctypes.data, mp3g.OUT_S16_MONO, mp3g.MODE_EXACT)
    if st != 0:  # (no device here; on a GPU machine the call simply succeeds)
        assert st in (3, 4, 5), st  # MP3G_ERR_NO_DEVICE / _DEVICE / _OUT_OF_MEMORY
        assert b"format" not in L.mp3g_last_error()


def test_host_buffer_dtype_follows_the_format():
    """decode_streams_into checks the dtype the format implies (the library
    writes through a raw pointer)."""
    import pytest
    with pytest.raises(ValueError, match="int16"):
        mp3g.decode_streams_into([b"\xff\xfb"], np.zeros(1152, np.float32), out_format=mp3g.OUT_S16_MONO)
    for fmt in (mp3g.OUT_F32, mp3g.OUT_F32_PLANAR, mp3g.OUT_F32_MONO):
        with pytest.raises(ValueError, match="float32"):
            mp3g.decode_streams_into([b"\xff\xfb"], np.zeros(2304, np.int16), out_format=fmt)
