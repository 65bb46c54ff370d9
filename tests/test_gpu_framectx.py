"""Delta features and frame context on the GPU (include/mp3g.h "Delta features and
frame context"): mp3g_add_deltas_rows and
mp3g_stack_frames_rows against their host references bit for bit, between guard
rows of sentinel-filled buffers -- 16-byte and single-word paths, strides above
the live widths, views one float into an allocation, lengths per row and per
plane from the host and the device -- and the deltas= and stack= keywords of the
fbank and MFCC tensor calls against the host chain on the rows of
decode_windows_resampled_tensor."""
import numpy as np
import pytest

import spec_framectx as spec
from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
FRAMES = [1, 2, 5, 33, 65, 301]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feats(rng, shape):
    x = rng.normal(-4.0, 3.0, shape).astype(np.float32)
    x.reshape(-1)[::7] = -0.0
    return x


def padded(x, stride):
    """x [B, (C,) F, cols] in a buffer of `stride` columns, the words past cols SENTINEL."""
    buf = np.full(x.shape[:-1] + (stride,), SENTINEL, np.uint32)
    buf[..., :x.shape[-1]] = bits(x)
    return buf.view(np.float32)


def on_device(torch, host, offset):
    """host (float32) on the device as a contiguous tensor `offset` floats into its allocation."""
    flat = torch.empty(host.size + offset, dtype=torch.int32, device="cuda")
    view = flat[offset:].view(host.shape)
    view.copy_(torch.from_numpy(bits(host).view(np.int32)))
    return view.view(torch.float32)


def run(gpu, call, host_call, buf, lengths, out_shape, out_offset=0, device_lengths=False):
    """call(d_in, lengths, d_out) into a sentinel-filled allocation with a guard row
    on both sides of the rows: every word is host_call(out)'s or the sentinel.
    Returns what the device call returned."""
    import torch
    B = out_shape[0]
    row = int(np.prod(out_shape[1:]))
    obuf = torch.full(((B + 2) * row + out_offset,), SENTINEL, dtype=torch.int32, device="cuda")
    d_out = obuf[out_offset + row:out_offset + (B + 1) * row].view(out_shape).view(torch.float32)
    want = host_call(np.full(out_shape, SENTINEL, np.uint32).view(np.float32))
    n = torch.tensor(np.asarray(lengths), dtype=torch.int32, device="cuda") if device_lengths else lengths
    got = call(buf, n, d_out)
    torch.cuda.synchronize()
    full = np.full(obuf.shape, SENTINEL, np.uint32)
    first = want[0] if isinstance(want, tuple) else want
    full[out_offset + row:out_offset + (B + 1) * row] = bits(first).reshape(-1)
    bad = np.argwhere(obuf.cpu().numpy().view(np.uint32) != full)
    assert not len(bad), (out_shape, out_offset, len(bad), bad[:6].reshape(-1).tolist())
    return got, want


def check_deltas(gpu, x, lengths, order, window, stride, so_pad=0, in_offset=0, out_offset=0, device_lengths=False):
    import torch
    cols = x.shape[-1]
    buf = padded(x, stride)
    out_shape = x.shape[:-1] + ((order + 1) * cols + so_pad,)
    d_in = on_device(torch, buf, in_offset)
    got, want = run(gpu, lambda i, n, o: gpu.add_deltas(i, n, order, window, out=o, n_cols=cols),
                    lambda o: gpu.add_deltas_host(buf, lengths, order, window, n_cols=cols, out=o),
                    d_in, lengths, out_shape, out_offset, device_lengths)
    assert tuple(got.shape) == out_shape
    return want


def check_stack(gpu, x, lengths, params, stride, n_frames_out=None, so_pad=0, in_offset=0, out_offset=0,
                device_lengths=False):
    import torch
    left, right, step, first = params
    cols, F = x.shape[-1], x.shape[-2]
    buf = padded(x, stride)
    Fo = spec.n_out(F, step, first) if n_frames_out is None else n_frames_out
    out_shape = x.shape[:-2] + (Fo, (left + right + 1) * cols + so_pad)
    d_in = on_device(torch, buf, in_offset)
    (got, m), (want, want_m) = run(
        gpu, lambda i, n, o: gpu.stack_frames(i, n, left, right, step, first, n_cols=cols, out=o),
        lambda o: gpu.stack_frames_host(buf, lengths, left, right, step, first, n_cols=cols, out=o),
        d_in, lengths, out_shape, out_offset, device_lengths)
    assert m.dtype == torch.int32 and tuple(m.shape) == x.shape[:-2] and np.array_equal(m.cpu().numpy(), want_m)
    return want, want_m


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("n_cols,stride", [(1, 1), (13, 16), (40, 40), (65, 72), (80, 80)])
@pytest.mark.parametrize("F", FRAMES)
def test_kernels_equal_the_host_references_and_write_nothing_else(gpu, F, n_cols, stride, planes):
    """Rows of 0, 1, 2, 33, F and F + 9 frames (shorter than the halo, across the
    tile edge at 64), every (order, window) and stack set of the CPU tests.  Over
    the sets the output stride is the live width, four more and three more, one
    input and one output are views one float into their allocation, and the
    lengths are per row or per plane, from the host or the device; the rotation
    moves with F, so every set meets every path."""
    rng = np.random.default_rng(1000 * F + 10 * stride + planes)
    per_row = [0, 1, 2, 33, F, F + 9]
    per_plane = np.stack([per_row, per_row[::-1]], 1)[:, :planes]
    x = feats(rng, (len(per_row), planes, F, n_cols))
    if planes == 1 and F % 2:
        x = x[:, 0]  # a three-dimensional tensor
    k = FRAMES.index(F)
    for order, window in spec.DELTA_SETS:
        lengths = per_plane if k % 2 and x.ndim == 4 else per_row
        want = check_deltas(gpu, x, lengths, order, window, stride, so_pad=(0, 4, 3)[k % 3],
                            in_offset=int(k % 5 == 3), out_offset=int(k % 5 == 4), device_lengths=bool(k % 4 >= 2))
        assert order == 0 or F == 1 or want[..., n_cols:(order + 1) * n_cols].any()
        k += 1
    special = x.copy()
    for row in special.reshape((-1,) + special.shape[-2:]):  # (views of the copy: -0, Inf, NaN payloads, a subnormal)
        spec.special_values(row)
    for name in sorted(spec.STACK_SETS):
        params = spec.STACK_SETS[name]
        lengths = per_plane if k % 2 and x.ndim == 4 else per_row
        full = spec.n_out(F, params[2], params[3])
        Fo = (None, full + 3, max(full - 1, 0))[k % 3]
        check_stack(gpu, special, lengths, params, stride, n_frames_out=Fo, so_pad=(0, 4, 3)[(k // 2) % 3],
                    in_offset=int(k % 5 == 3), out_offset=int(k % 5 == 4), device_lengths=bool(k % 4 >= 2))
        k += 1


def test_many_short_rows_and_one_long_row(gpu):
    """300 rows of 5 frames: more workgroups than the device runs at once; one row
    of 4,099 frames: many tiles of one plane, the halo across every tile edge."""
    rng = np.random.default_rng(77)
    lengths = [5, 4, 3, 5, 2, 5] * 50
    x = feats(rng, (300, 5, 80))
    check_deltas(gpu, x, lengths, 2, 2, 80)
    check_deltas(gpu, x, lengths, 4, 8, 80, so_pad=3)
    check_stack(gpu, x, lengths, spec.STACK_SETS["splice_3_3"], 80)
    check_stack(gpu, x, lengths, spec.STACK_SETS["lfr_7_6"], 80, n_frames_out=3)
    x = feats(rng, (1, 4099, 80))
    check_deltas(gpu, x, [4099], 2, 2, 80)
    check_deltas(gpu, x, [4000], 4, 8, 80, device_lengths=True)
    check_deltas(gpu, x[..., :13], [4099], 2, 3, 16)
    check_stack(gpu, x, [4099], spec.STACK_SETS["splice_3_3"], 80)
    check_stack(gpu, x, [4000], spec.STACK_SETS["lfr_7_6"], 80, device_lengths=True)
    check_stack(gpu, x[..., :13], [4099], spec.STACK_SETS["subsample_3_2"], 16)


def test_wide_rows_and_the_python_layer(gpu):
    """More columns than one delta workgroup takes (two column groups, the second
    partial), and the tensors the calls make themselves."""
    import torch
    rng = np.random.default_rng(5)
    x = feats(rng, (3, 2, 70, 200))
    lengths = [[70, 3], [0, 69], [64, 65]]
    check_deltas(gpu, x, lengths, 2, 2, 200)
    check_deltas(gpu, x[..., :197], lengths, 3, 1, 200)
    check_stack(gpu, x, lengths, (1, 0, 2, 1), 200)
    d_x = torch.from_numpy(x).cuda()
    got = gpu.add_deltas(d_x, lengths)
    assert tuple(got.shape) == (3, 2, 70, 600)
    assert np.array_equal(bits(got.cpu().numpy()), bits(gpu.add_deltas_host(x, lengths)))
    got, m = gpu.stack_frames(d_x, lengths, **gpu.lfr_options(7, 6))
    want, want_m = gpu.stack_frames_host(x, lengths, **gpu.lfr_options(7, 6))
    assert tuple(got.shape) == (3, 2, 12, 1400) and np.array_equal(m.cpu().numpy(), want_m)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    empty, m = gpu.stack_frames(d_x[:0], [], 1, 1)
    assert tuple(empty.shape) == (0, 2, 70, 600) and tuple(m.shape) == (0, 2)
    assert tuple(gpu.add_deltas(d_x[:0], []).shape) == (0, 2, 70, 600)
    for bad in (d_x.cpu(), d_x.double(), d_x[..., :3], d_x[0, 0]):
        with pytest.raises(ValueError):
            gpu.add_deltas(bad, [1, 1, 1])
        with pytest.raises(ValueError):
            gpu.stack_frames(bad, [1, 1, 1])
    with pytest.raises(ValueError):
        gpu.add_deltas(d_x, [1, 2])
    with pytest.raises(gpu.Mp3gError):
        gpu.add_deltas(d_x, lengths, out=d_x)
    with pytest.raises(gpu.Mp3gError):
        gpu.add_deltas(d_x, lengths, order=2, window=17)


# ---- end to end -----------------------------------------------------------------------

T_E2E = 32000  # 2 s at 16 kHz
F_E2E = 1 + (T_E2E - 400) // 160
VOXCELEB = dict(energy_threshold=5.5, energy_mean_scale=0.5, proportion_threshold=0.12, frames_context=2)


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, a synthetic stream per MPEG-1 sample rate and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for sfreq in range(3):
        data.append(synth.encode_stream(300 + sfreq, 100, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


@pytest.fixture(scope="module")
def rows_of(gpu, streams):
    """(rows [B, planes, T], frame lengths [B]) of decode_windows_resampled_tensor, per output format."""
    def make(fmt, start):
        batch, lengths, _, _ = gpu.decode_windows_resampled_tensor(streams, [start] * len(streams), T_E2E, 16000,
                                                                   out_format=fmt)
        planes = 2 if fmt == gpu.OUT_F32_PLANAR else 1
        flen = np.array([min(F_E2E, max(0, (int(n) - 400) // 160 + 1)) for n in lengths])
        return batch.cpu().numpy().reshape(len(streams), planes, T_E2E), flen
    return make


def host_features(ob, rows):
    return np.stack([np.stack([ob.host(rows[k, p], F_E2E) for p in range(rows.shape[1])]) for k in range(len(rows))])


def test_mfcc_cmvn_and_deltas_end_to_end(gpu, streams, rows_of):
    """The GMM recipes' apply-cmvn | add-deltas."""
    rows, flen = rows_of(gpu.OUT_F32_MONO, 0)
    mf = gpu.MFCC()
    plain = host_features(mf, rows)[:, 0]
    mf.close()
    got, flen2, _, _ = gpu.decode_windows_mfcc_tensor(streams, [0] * len(streams), T_E2E, cmvn="mean",
                                                      deltas=dict(order=2, window=2))
    want = gpu.add_deltas_host(gpu.cmvn_host(plain, flen), flen, 2, 2)
    assert tuple(got.shape) == (len(streams), F_E2E, 39) and flen2.tolist() == flen.tolist() and flen[-1] == 0
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and want[:-1, :, 13:].any()
    # without the keywords: what the call returned before them
    base, _, _, _ = gpu.decode_windows_mfcc_tensor(streams, [0] * len(streams), T_E2E, cmvn="mean")
    assert np.array_equal(bits(base.cpu().numpy()), bits(gpu.cmvn_host(plain, flen)))


def test_fbank_lfr_end_to_end(gpu, streams, rows_of):
    """The Paraformer front end: 7 filter-bank frames stacked at a stride of 6."""
    rows, flen = rows_of(gpu.OUT_F32_MONO, 50)
    fb = gpu.FBank()
    plain = host_features(fb, rows)[:, 0]
    fb.close()
    got, slen, _, _ = gpu.decode_windows_fbank_tensor(streams, [50] * len(streams), T_E2E, stack=gpu.lfr_options(7, 6))
    want, want_len = gpu.stack_frames_host(plain, flen, **gpu.lfr_options(7, 6))
    assert tuple(got.shape) == (len(streams), -(-F_E2E // 6), 560)
    assert slen.dtype == np.int64 and slen.tolist() == want_len.tolist() == [-(-int(n) // 6) for n in flen]
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and slen[-1] == 0 and not got[-1].any()
    # deltas, then the stack
    got, slen, _, _ = gpu.decode_windows_fbank_tensor(streams, [50] * len(streams), T_E2E, cmvn="mean",
                                                      deltas=dict(order=1, window=3), stack=dict(step=3, first=1))
    want, want_len = gpu.stack_frames_host(gpu.add_deltas_host(gpu.cmvn_host(plain, flen), flen, 1, 3), flen, step=3,
                                           first=1)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and slen.tolist() == want_len.tolist()


def test_mfcc_vad_and_splice_end_to_end_per_plane(gpu, streams, rows_of):
    """The voxceleb VAD leaves a count per plane; the splice takes them as they are."""
    rows, flen = rows_of(gpu.OUT_F32_PLANAR, 100)
    kw = dict(n_ceps=30, n_mels=30)
    mf = gpu.MFCC(**kw)
    plain = host_features(mf, rows)
    mf.close()
    got, slen, _, _ = gpu.decode_windows_mfcc_tensor(streams, [100] * len(streams), T_E2E, vad=VOXCELEB,
                                                     out_format=gpu.OUT_F32_PLANAR, stack=dict(left=2, right=2), **kw)
    voiced, counts = gpu.vad_energy_host(plain, flen, **VOXCELEB)
    selected, vlen = gpu.select_frames_host(plain, voiced, flen)
    want, want_len = gpu.stack_frames_host(selected, vlen, left=2, right=2)
    assert tuple(got.shape) == (len(streams), 2, F_E2E, 150) and slen.shape == (len(streams), 2)
    assert np.array_equal(slen, want_len) and np.array_equal(want_len, counts)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
