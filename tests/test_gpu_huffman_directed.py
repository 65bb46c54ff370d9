"""The directed main-data inputs (tests/directed_stream.py) on the GPU.

test_gpu_huffman.py runs the main-data kernel (huffman_dev.hip) on random
streams, which never write 40 of the 1,410 codewords (the leaves behind the
second- and third-level links of the device table), never select table 31,
never write a 13-bit escape near its maximum and put a long symbol on a
given phase of the reader's 64-bit window, or on the end of its buffer, only
by chance.  Here the kernel decodes

  A  every codeword and escape extreme (1,410 / 1,410 codewords, 81 / 81
     signed quads per count1 table, max |line| 8206): 22 frames, 22,968
     bytes; long version 71 frames, 74,124 bytes (more than one 256-job
     block, the first of them read from global memory by the two smaller
     stages)
  B  22 symbol classes on all 64 phases: 704 frames, 109,824 bytes; again at
     320 kbps (734,976 bytes), where the two smaller stages read global memory
  C  the classes cut at every bit by the end of the buffer or of their
     part: 2,816 frames, 292,864 bytes; 640 of them again in a batch spread
     so that the two smaller stages read global memory (2,572,160 bytes)
  D  every big_values 0..288, quads to the i <= 572 limit: 146 frames,
     152,424 bytes
  E  every scale factor layout, MPEG-1 (176 frames, 55,088 bytes) and MPEG-2
     (2,049 frames, 159,822 bytes)

with each of its three stages.  The bar is byte equality with the host
parse, which test_directed_stream_cpu.py holds to the oracle and to the
writer's own arrays (where the coverage of each set is asserted too); A and
D are compared with the writer's arrays directly as well.
"""
import os
import re
import sys

import numpy as np
import pytest

import directed_stream as ds
import oracle
from conftest import REPO
from test_gpu_huffman import assert_same_as_host, gpu_parse

pytestmark = pytest.mark.gpu

SETS = ("A1", "A_long", "B", "B320", "C", "D", "E1", "E2")
STAGES = {"default": 0, "mid": "HUFF_STAGE_MID", "wide": "HUFF_STAGE_WIDE"}


def stage_flags(gpu, stage):
    return getattr(gpu, STAGES[stage]) if STAGES[stage] else 0


@pytest.mark.parametrize("stage", sorted(STAGES))
@pytest.mark.parametrize("name", SETS)
def test_stages(gpu, name, stage):
    st, _ = ds.directed_set(name)
    g, c = assert_same_as_host(gpu, [st["data"]], f"set {name}, {stage} stage", stage_flags(gpu, stage))
    assert len(g) == len(st["granules"])
    if name[0] in "AD":
        assert st["plain"].all()
        assert g.tobytes() == st["granules"].tobytes(), name
        assert np.array_equal(c, st["coeffs"]), name


def test_stage_model(gpu):
    """Which of the kernel's paths the A sets take, by its own rule (blocks of
    256 jobs, staged when their span in 64-bit words fits the stage): long A
    is read from global memory in at least one block by the default and the
    mid stage and staged by the wide one; short A is staged by the default."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from huff_time import staged_blocks
    text = open(os.path.join(REPO, "go-mp3_amd", "csrc", "kernels.h")).read()
    words = {k: int(re.search(r"constexpr int kHuffStageWords%s = (\d+);" % k, text).group(1))
             for k in ("", "Mid", "Wide")}
    assert words == {"": 3584, "Mid": 5376, "Wide": 8704}
    assert "#define MP3G_HUFF_THREADS 256" in open(os.path.join(REPO, "go-mp3_amd", "csrc", "huffman_dev.hip")).read()
    long_jobs = gpu.scan_streams([ds.directed_set("A_long")[0]["data"]], n_threads=1)["jobs"]
    short_jobs = gpu.scan_streams([ds.directed_set("A1")[0]["data"]], n_threads=1)["jobs"]
    assert len(long_jobs) > 256
    assert staged_blocks(long_jobs, 256, words[""]) < 1.0
    assert staged_blocks(long_jobs, 256, words["Mid"]) < 1.0
    assert staged_blocks(long_jobs, 256, words["Wide"]) == 1.0
    assert staged_blocks(short_jobs, 256, words[""]) == 1.0
    b320 = gpu.scan_streams([ds.directed_set("B320")[0]["data"]], n_threads=1)["jobs"]
    assert len(b320) % 256 == 0  # whole blocks of 64 frames, 8,064 words each
    assert staged_blocks(b320, 256, words["Mid"]) == 0.0 and staged_blocks(b320, 256, words["Wide"]) == 1.0


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_cuts_from_global_memory(gpu, stage):
    """Set C's widest symbols, longest codeword and quads, cut at every bit, in
    a batch whose blocks only the wide stage holds (directed_stream.spread;
    the model of that is asserted in test_directed_stream_cpu.py): the
    default and the mid stage read them with the reader of global memory."""
    datas, _, _ = ds.spread_cuts()
    assert_same_as_host(gpu, datas, f"spread cuts, {stage} stage", stage_flags(gpu, stage))


@pytest.mark.parametrize("name", ["A1", "A_long", "D"])
def test_rows_to_count1(gpu, name):
    """MP3G_HUFF_ROWS_COUNT1: lines below min(count1 + 6, 576) equal the full-row decode, descriptors equal."""
    st, _ = ds.directed_set(name)
    g0, c0, _, _ = gpu_parse(gpu, [st["data"]], 0)
    g1, c1, _, _ = gpu_parse(gpu, [st["data"]], gpu.HUFF_ROWS_COUNT1)
    assert g0.tobytes() == g1.tobytes() == st["granules"].tobytes()
    lim = np.minimum(g0["ch"]["count1"].astype(np.int64) + 6, 576)
    inside = np.arange(576)[None, None, :] < lim[:, :, None]
    assert np.array_equal(c1[inside], c0[inside]) and np.array_equal(c0, st["coeffs"])
    assert (c1 == 0x5A5A).any(), "the tails should be left unwritten"


@pytest.mark.parametrize("name", ["A1", "A_long", "D", "E1", "E2"])
def test_pcm_vs_oracle(gpu, name):
    """scan + device Huffman + device DSP of the valid sets: exact mode is
    the oracle's PCM byte for byte, fast mode within its 1 LSB."""
    st, _ = ds.directed_set(name)
    ost, opcm = oracle.decode_all(st["data"])
    assert ost == oracle.ORC_OK
    pcm, streams, end = gpu.decode_streams([st["data"]], mode=gpu.MODE_EXACT)
    assert list(end) == [7] and int(streams[0]["n_granules"]) == len(st["granules"])
    assert pcm.tobytes() == opcm
    pcm_f, _, _ = gpu.decode_streams([st["data"]], mode=gpu.MODE_FAST)
    assert np.abs(pcm_f.astype(np.int32) - pcm).max() <= 1
