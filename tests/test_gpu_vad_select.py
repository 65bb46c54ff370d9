"""The energy VAD and the voiced-frame selection on the GPU (include/mp3g.h
"Sliding-window CMN, energy VAD and voiced-frame selection", DESIGN.md section
9j): mp3g_vad_energy_rows and mp3g_select_frames_rows against their host
references bit for bit, nothing else written, and decode_windows_mfcc_tensor's
speaker front end against the host chain on the rows of
decode_windows_resampled_tensor."""
import numpy as np
import pytest

from mp3g import synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a NaN payload no feature has
BYTE = 0xA5            # what a flag never is
GUARD = 1
VOXCELEB = dict(energy_threshold=5.5, energy_mean_scale=0.5, proportion_threshold=0.12, frames_context=2)
KALDI = dict(energy_threshold=5.0, energy_mean_scale=0.5, proportion_threshold=0.6, frames_context=0)
FLOOR_BITS = 0xC17F1402  # logf(2^-23)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def features(rng, shape, col):
    x = rng.normal(0.0, 4.0, shape).astype(np.float32)
    x[..., col] = rng.normal(7.0, 3.0, shape[:-1]).astype(np.float32)
    return x


def check_vad(gpu, x, lengths, opts, col, n_cols, device_lengths=False):
    """The flags into a buffer with a guard row on both sides, the counts
    between two guard words: every byte and word is mp3g_vad_energy_host's."""
    import torch
    d_x = torch.from_numpy(x).cuda()
    vbuf = torch.full((len(x) + 2 * GUARD,) + x.shape[1:-1], BYTE, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((len(x) + 2 * GUARD,) + x.shape[1:-2], -7, dtype=torch.int32, device="cuda")
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda") if device_lengths else lengths
    voiced, counts = gpu.vad_energy(d_x, n, col=col, n_cols=n_cols, out=(vbuf[GUARD:-GUARD], cbuf[GUARD:-GUARD]),
                                    **opts)
    torch.cuda.synchronize()
    want_v, want_c = gpu.vad_energy_host(x, lengths, col=col, n_cols=n_cols, **opts)
    got_v, got_c = vbuf.cpu().numpy(), cbuf.cpu().numpy()
    assert (got_v[:GUARD] == BYTE).all() and (got_v[-GUARD:] == BYTE).all()
    assert (got_c[:GUARD] == -7).all() and (got_c[-GUARD:] == -7).all()
    bad = np.argwhere(got_v[GUARD:-GUARD] != want_v)
    assert not len(bad), (x.shape, opts, len(bad), bad[:6].tolist())
    assert np.array_equal(got_c[GUARD:-GUARD], want_c)
    return d_x, voiced, want_v, want_c


def check_select(gpu, d_x, x, d_voiced, voiced, lengths, n_frames_out, n_cols, stride_out):
    """The selection into a sentinel-filled buffer with a guard row on both
    sides: every word is mp3g_select_frames_host's (copies, +0 padding) or the
    sentinel; lengths_out equal."""
    import torch
    shape = x.shape[:-2] + (n_frames_out, stride_out)
    buf = torch.full((len(x) + 2 * GUARD,) + shape[1:], SENTINEL, dtype=torch.int32, device="cuda")
    out, m = gpu.select_frames(d_x, d_voiced, lengths, n_cols=n_cols, out=buf[GUARD:GUARD + len(x)].view(torch.float32))
    torch.cuda.synchronize()
    host_buf = np.full(shape, SENTINEL, np.uint32).view(np.float32)
    want, want_m = gpu.select_frames_host(x, voiced, lengths, n_cols=n_cols, out=host_buf)
    guard = np.full((GUARD,) + shape[1:], SENTINEL, np.uint32)
    got = buf.cpu().numpy().view(np.uint32)
    full = np.concatenate([guard, bits(want), guard])
    bad = np.argwhere(got != full)
    assert not len(bad), (x.shape, n_frames_out, n_cols, len(bad), bad[:6].tolist())
    assert np.array_equal(m.cpu().numpy(), want_m) and m.dtype == torch.int32
    return want_m


@pytest.mark.parametrize("n_cols,stride", [(1, 1), (13, 16), (40, 40), (65, 72)])
@pytest.mark.parametrize("F", [1, 33, 65, 301])
def test_kernels_equal_host_references_and_write_nothing_else(gpu, F, n_cols, stride):
    """Rows of lengths 0, 1, 33, F and F + 9, one and two planes; Kaldi's and
    the voxceleb options, a context above the row and a fixed threshold; then
    the selection of what the VAD found into fewer, as many and more frames."""
    rng = np.random.default_rng(1000 * F + stride)
    lengths = [0, 1, 33, F, F + 9]
    col = min(n_cols - 1, 3)
    for planes in (1, 2):
        x = features(rng, (5, planes, F, stride), col)
        for k, opts in enumerate((KALDI, VOXCELEB, dict(VOXCELEB, frames_context=F + 2),
                                  dict(KALDI, energy_mean_scale=0.0, frames_context=1))):
            shaped = x[:, 0] if planes == 1 and k % 2 else x
            d_x, d_v, v, counts = check_vad(gpu, shaped, lengths, opts, col, n_cols, device_lengths=bool(k % 2))
            assert counts[0].max() == 0
            for Fo, so in ((F, stride), (max(1, F // 3), n_cols), (F + 3, n_cols + 2)):
                m = check_select(gpu, d_x, shaped, d_v, v, lengths, Fo, n_cols, so)
                assert (m <= np.minimum(counts, Fo)).all()


@pytest.mark.parametrize("context,den,num,t", [(2, 5, 3, 2), (5, 10, 6, 4)])
def test_float32_ties_are_voiced(gpu, context, den, num, t):
    """The two ties of the float32 proportion test at 0.6f (tests/test_vad_select_cpu.py): voiced, as in Kaldi."""
    n = 12
    x = np.zeros((1, n, 2), np.float32)
    lo = max(0, t - context)
    x[0, lo:lo + num, 0] = 9.0
    opts = dict(energy_threshold=5.0, energy_mean_scale=0.0, proportion_threshold=0.6, frames_context=context)
    _, _, v, _ = check_vad(gpu, x, [n], opts, 0, 1)
    assert v[0, t] == 1
    x[0, lo + num - 1, 0] = 0.0
    _, _, v, _ = check_vad(gpu, x, [n], opts, 0, 1)
    assert v[0, t] == 0


def test_rows_longer_than_a_chunk(gpu):
    """F = 2,500: ten chunks of 256 frames, the count carried from chunk to
    chunk; more voiced frames than n_frames_out; all, none and alternating flags."""
    import torch
    rng = np.random.default_rng(2500)
    F = 2500
    x = features(rng, (4, 2, F, 30), 0)
    lengths = [F, 2301, 257, F]
    d_x, d_v, v, counts = check_vad(gpu, x, lengths, VOXCELEB, 0, 30)
    assert counts[0].min() > 600 and counts[2].max() <= 257
    for Fo in (600, F):  # (600 < every long row's count)
        m = check_select(gpu, d_x, x, d_v, v, lengths, Fo, 30, 30)
        assert m[0].max() == min(Fo, counts[0].max())
    flags = np.zeros((4, 2, F), np.uint8)
    flags[0] = 1
    flags[1, :, ::2] = 3
    flags[3, :, 255:258] = 1
    m = check_select(gpu, d_x, x, torch.from_numpy(flags).cuda(), flags, lengths, F, 30, 32)
    assert m.tolist() == [[F, F], [1151, 1151], [0, 0], [3, 3]]


def test_arguments(gpu):
    import torch
    x = torch.zeros((2, 4, 6), dtype=torch.float32, device="cuda")
    v = torch.zeros((2, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.vad_energy(x, [4, 4], col=6)
    assert e.value.status == 1
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.select_frames(x, v, [4, 4], out=x)
    assert e.value.status == 1
    for bad in (x.cpu(), x.double(), x[:, :, :3], x[0]):
        with pytest.raises(ValueError):
            gpu.vad_energy(bad, [4, 4])
    with pytest.raises(ValueError):
        gpu.select_frames(x, v[:, :3], [4, 4])
    with pytest.raises(ValueError):
        gpu.select_frames(x, v.to(torch.int32), [4, 4])
    voiced, counts = gpu.vad_energy(x[:0], [])
    assert voiced.shape == (0, 4) and counts.shape == (0,)
    out, m = gpu.select_frames(x, v, [4, 4], n_frames_out=9)
    torch.cuda.synchronize()
    assert out.shape == (2, 9, 6) and not out.any() and m.tolist() == [0, 0]


# ---- end to end -----------------------------------------------------------------------

T_E2E = 32000  # 2 s at 16 kHz
F_E2E = 1 + (T_E2E - 400) // 160


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, a synthetic stream per MP3 sample rate and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for lsf in (False, True):
        for sfreq in range(3):
            data.append(synth.encode_stream(300 + 3 * int(lsf) + sfreq, 100, lsf=lsf, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


def check_end_to_end(gpu, streams, starts, fmt, mode):
    kw = dict(mode=mode, out_format=fmt, n_ceps=30, n_mels=30)
    batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(streams, starts, T_E2E, 16000, mode=mode,
                                                                    out_format=fmt)
    B, F = len(streams), F_E2E
    planes = 2 if fmt == gpu.OUT_F32_PLANAR else 1
    rows = batch.cpu().numpy().reshape(B, planes, T_E2E)
    mf = gpu.MFCC(n_mels=30, n_ceps=30)
    plain = np.stack([np.stack([mf.host(rows[k, p], F) for p in range(planes)]) for k in range(B)])
    mf.close()
    flen = np.array([min(F, max(0, (int(n) - 400) // 160 + 1)) for n in lengths])
    # the speaker recipes' front end: the VAD on the raw features, the sliding mean over all frames, the selection
    feats, vlen, st2, rates2 = gpu.decode_windows_mfcc_tensor(streams, starts, T_E2E, cmvn="sliding", cmn_window=30,
                                                              vad=VOXCELEB, **kw)
    assert tuple(feats.shape) == ((B, 2, F, 30) if planes == 2 else (B, F, 30))
    assert rates2.tolist() == rates.tolist() and rates[-1] == 0 and st2.tolist() == st.tolist()
    norm = gpu.sliding_cmn_host(plain, flen, 30, 100, True, False)
    voiced, counts = gpu.vad_energy_host(plain, flen, **VOXCELEB)
    want, want_len = gpu.select_frames_host(norm, voiced, flen)
    got = feats.cpu().numpy().reshape(B, planes, F, 30)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:4].tolist()
    assert vlen.dtype == np.int64 and vlen.shape == ((B, 2) if planes == 2 else (B,))
    assert np.array_equal(vlen.reshape(B, planes), want_len) and np.array_equal(want_len, counts)
    assert vlen[-1].max() == 0 and not got[-1].any()           # the stream without a frame: length 0, a zero row
    assert 0 < vlen[:-1].min() and vlen[:-1].max() <= F and (vlen.reshape(B, planes) < flen[:, None])[:-1].any()
    # the other normalisations with the VAD, and the sliding one without it
    for cmvn in ("sliding_var", "mean", None):
        feats, vlen, _, _ = gpu.decode_windows_mfcc_tensor(streams, starts, T_E2E, cmvn=cmvn, cmn_window=30,
                                                           min_cmn_window=10, center=False, vad=VOXCELEB, **kw)
        norm = (plain if cmvn is None else gpu.cmvn_host(plain, flen) if cmvn == "mean"
                else gpu.sliding_cmn_host(plain, flen, 30, 10, False, True))
        want, want_len = gpu.select_frames_host(norm, voiced, flen)
        got = feats.cpu().numpy().reshape(B, planes, F, 30)
        assert np.array_equal(bits(got), bits(want)), cmvn
        assert np.array_equal(vlen.reshape(B, planes), want_len)
    feats, flen2, _, _ = gpu.decode_windows_mfcc_tensor(streams, starts, T_E2E, cmvn="sliding", **kw)
    assert np.array_equal(bits(feats.cpu().numpy().reshape(B, planes, F, 30)),
                          bits(gpu.sliding_cmn_host(plain, flen, 300, 100, True, False)))
    assert flen2.tolist() == flen.tolist()
    # without the new keywords: what the call returned before them
    for cmvn in (None, "mean"):
        feats, flen2, _, _ = gpu.decode_windows_mfcc_tensor(streams, starts, T_E2E, cmvn=cmvn, **kw)
        want = plain if cmvn is None else gpu.cmvn_host(plain, flen)
        assert np.array_equal(bits(feats.cpu().numpy().reshape(B, planes, F, 30)), bits(want)), cmvn
        assert flen2.tolist() == flen.tolist() and flen2.shape == (B,)


def test_end_to_end_exact(gpu, streams):
    check_end_to_end(gpu, streams, [0] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_EXACT)


def test_end_to_end_planar(gpu, streams):
    check_end_to_end(gpu, streams, [100] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_EXACT)


def test_end_to_end_fast_mode(gpu, streams):
    check_end_to_end(gpu, streams, [50] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_FAST)
    check_end_to_end(gpu, streams, [50] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_FAST)


def test_end_to_end_arguments(gpu, streams):
    for kw in (dict(vad=VOXCELEB, use_energy=False), dict(vad=dict(threshold=5.0)), dict(vad=5.5),
               dict(cmvn="sliding", cmn_window=0), dict(cmvn="slide")):
        with pytest.raises(gpu.Mp3gError) as e:
            gpu.decode_windows_mfcc_tensor(streams[:1], [0], T_E2E, **kw)
        assert e.value.status == 1, kw
    feats, flen, _, _ = gpu.decode_windows_mfcc_tensor([], [], T_E2E, cmvn="sliding", vad=VOXCELEB)
    assert tuple(feats.shape) == (0, F_E2E, 13) and flen.shape == (0,)
