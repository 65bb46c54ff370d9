"""The augmented training batch end to end on the GPU (include/mp3g.h "Room
reverberation and noise at an SNR"):
decode_windows_augmented_tensor -- MP3 bytes, the windowed decode, the resampler,
the reverberation and the noises, with no copy to the host -- against
augment_host of the resampled tensor bit for bit, and without augment keywords
against decode_windows_resampled_tensor."""
import numpy as np
import pytest

from mp3g import synth

pytestmark = pytest.mark.gpu

T_E2E = 16000  # 1 s at 16 kHz


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def streams(sample_files):
    """The two sample files, a synthetic stream per MP3 sample rate and a stream without a frame."""
    data = [sample_files["classic_lame.mp3"], sample_files["mpeg2.mp3"]]
    for lsf in (False, True):
        for sfreq in range(3):
            data.append(synth.encode_stream(500 + 3 * int(lsf) + sfreq, 60, lsf=lsf, sfreq=sfreq))
    data.append(b"\x00" * 700)
    return data


@pytest.fixture(scope="module")
def banks(gpu):
    """(reverb of three responses at 16 kHz, noise bank [3, 20000], its lengths)."""
    rng = np.random.default_rng(31)
    L = 4000
    h = (rng.standard_normal((3, L)) * np.exp(-np.arange(L) / 600.0)).astype(np.float32)
    h[0, 40] = h[1, 0] = h[2, 1500] = 8.0
    rv = gpu.Reverb(h, [4000, 1024, 2500], 16000, device=0)
    noise = (0.05 * rng.standard_normal((3, 20000))).astype(np.float32)
    yield rv, noise, [20000, 7000, 12345]
    rv.close()


def check_end_to_end(gpu, streams, banks, starts, fmt, mode):
    import torch
    rv, noise, nl = banks
    B = len(streams)
    rng = np.random.default_rng(B + fmt + mode)
    batch, lengths, st, rates = gpu.decode_windows_resampled_tensor(streams, starts, T_E2E, 16000, mode=mode,
                                                                    out_format=fmt)
    same = gpu.decode_windows_augmented_tensor(streams, starts, T_E2E, 16000, mode=mode, out_format=fmt)
    assert len(same) == 4 and np.array_equal(bits(same[0].cpu().numpy()), bits(batch.cpu().numpy()))
    assert same[1].tolist() == lengths.tolist() and same[2].tolist() == st.tolist() and same[3].tolist() == rates.tolist()
    kw = dict(reverb=rv, rir_index=[k % 4 - 1 for k in range(B)], noise_lengths=nl,
              additive=dict(index=rng.integers(-1, 3, (B, 2)), snr_db=rng.uniform(0, 15, (B, 2)),
                            start=rng.integers(0, 4000, (B, 2)), offset=rng.integers(0, 7000, (B, 2)),
                            wrap=[[1, 0]] * B))
    for normalize in (True, False):
        out, lengths2, st2, rates2, stats = gpu.decode_windows_augmented_tensor(
            streams, starts, T_E2E, 16000, mode=mode, out_format=fmt, noise=torch.from_numpy(noise).cuda(),
            normalize=normalize, **kw)
        torch.cuda.synchronize()
        assert lengths2.tolist() == lengths.tolist() and st2.tolist() == st.tolist() and rates2.tolist() == rates.tolist()
        want, want_stats = gpu.augment_host(batch.cpu().numpy(), lengths, noise=noise, normalize=normalize, **kw)
        assert tuple(out.shape) == tuple(batch.shape)
        got = out.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:4].tolist()
        assert np.array_equal(stats.cpu().numpy().view(np.uint64), want_stats.view(np.uint64))
        assert rates[-1] == 0 and not got[-1].any()  # the stream without a frame: a zero row
        if normalize:  # the rows come back at the power they had
            s = want_stats.reshape(B, -1, 4)
            live = s[..., 0] > 0
            assert live.any() and np.allclose(s[..., 2][live] * s[..., 3][live] ** 2, s[..., 0][live], rtol=1e-12)
    assert not np.array_equal(bits(got), bits(batch.cpu().numpy()))


def test_end_to_end_exact_mono(gpu, streams, banks):
    check_end_to_end(gpu, streams, banks, [0] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_EXACT)


def test_end_to_end_exact_planar(gpu, streams, banks):
    check_end_to_end(gpu, streams, banks, [100] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_EXACT)


def test_end_to_end_fast_mode(gpu, streams, banks):
    check_end_to_end(gpu, streams, banks, [50] * len(streams), gpu.OUT_F32_MONO, gpu.MODE_FAST)
    check_end_to_end(gpu, streams, banks, [50] * len(streams), gpu.OUT_F32_PLANAR, gpu.MODE_FAST)


def test_end_to_end_arguments(gpu, streams, banks):
    rv, noise, nl = banks
    with pytest.raises(TypeError):
        gpu.decode_windows_augmented_tensor(streams[:1], [0], T_E2E, 16000, reverbs=rv)
    with pytest.raises(gpu.Mp3gError) as e:
        gpu.decode_windows_augmented_tensor(streams[:1], [0], T_E2E, 16000, reverb=rv, rir_index=[3])
    assert e.value.status == 1
    out, lengths, _, _, stats = gpu.decode_windows_augmented_tensor([], [], T_E2E, 16000, normalize=True)
    assert tuple(out.shape) == (0, 2, T_E2E) and lengths.shape == (0,) and tuple(stats.shape) == (0, 2, 4)
