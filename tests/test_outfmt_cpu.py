"""Output formats (MP3G_OUT_S16 / MP3G_OUT_F32 / MP3G_OUT_F32_PLANAR), the part
that needs no GPU: the C-ABI additions are exported under ABI 5, the sizes,
the format check that comes before any device call, and the planar layout
helper of the binding."""
import ctypes as C
import re
import subprocess

import numpy as np

import mp3g


def test_symbols_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", mp3g.lib_path()], text=True)
    exported = set(re.findall(r" T (mp3g_\w+)", out))
    assert {"mp3g_out_bytes_per_granule", "mp3g_plan_execute_out", "mp3g_decode_host_out"} <= exported


def test_abi_version_unchanged():
    assert mp3g.lib().mp3g_abi_version() == 5


def test_out_bytes_per_granule():
    assert (mp3g.OUT_S16, mp3g.OUT_F32, mp3g.OUT_F32_PLANAR) == (0, 1, 2)
    assert [mp3g.out_bytes_per_granule(f) for f in (mp3g.OUT_S16, mp3g.OUT_F32, mp3g.OUT_F32_PLANAR)] == \
        [2304, 4608, 4608]
    assert mp3g.out_bytes_per_granule(7) == 0


def test_unknown_format_is_refused_without_a_device():
    """Format 7 is MP3G_ERR_INVALID_ARGUMENT before anything touches a device
    (this test runs where there is none)."""
    g = np.zeros(2, mp3g.GRANULE_DTYPE)
    c = np.zeros((2, 2, 576), np.int16)
    s = mp3g.streams_for([2])
    out = np.zeros(2 * 1152, np.float32)
    L = mp3g.lib()
    st = L.mp3g_decode_host_out(0, g.ctypes.data, c.ctypes.data, 2, s.ctypes.data, 1, None, None,
                                out.ctypes.data, 7, mp3g.MODE_EXACT)
    assert st == 1  # MP3G_ERR_INVALID_ARGUMENT
    assert b"format" in L.mp3g_last_error()
    # the plan entry checks the format first too (no plan needed to see it)
    assert L.mp3g_plan_execute_out(None, None, None, None, None, None, 7, None) == 1
    assert b"format" in L.mp3g_last_error()


def test_planar_views_offsets():
    lengths = [7, 40, 33]
    s = mp3g.streams_for(lengths)
    n = sum(lengths)
    out = np.arange(n * 1152, dtype=np.float32)  # every float holds its own index
    views = mp3g.planar_views(out, s)
    assert len(views) == 3
    first = 0
    for v, k in zip(views, lengths):
        assert v.shape == (2, k * 576)
        assert v[0, 0] == first * 1152 and v[0, -1] == first * 1152 + k * 576 - 1
        assert v[1, 0] == first * 1152 + k * 576 and v[1, -1] == (first + k) * 1152 - 1
        assert np.shares_memory(v, out)
        first += k
