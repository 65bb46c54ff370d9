"""Timing of the pipelined batch drop-in (mp3g_decode_streams_into) at c3
(VERDICT r04 item 3), beside what bounds it: the host scan alone and the PCIe
rates of the same bytes (pinned, one direction at a time and both at once).
GPU box:  python tools/pipe_time.py [repeats] [n_groups ...] [--formats s16,s16_mono,f32_mono] [--out FILE.json]
--formats: the output formats of mp3g_decode_streams_into_out to time, one
after the other in this process (s16, f32, f32_planar, s16_mono, f32_mono;
default s16), each with the PCIe time of its own output bytes beside it;
--out: the numbers as one JSON line.
(under rocprofv3 --kernel-trace --memory-copy-trace for the timeline;
MP3G_PIPE_TRACE=1 prints the library's per-group host timestamps)."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "go-mp3_amd"))
import torch  # noqa: E402
import mp3g  # noqa: E402
from mp3g import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("repeats", nargs="?", type=int, default=3)
    ap.add_argument("n_groups", nargs="*", type=int)
    ap.add_argument("--formats", default="s16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps, groups = a.repeats, a.n_groups or [0]
    known = {"s16": mp3g.OUT_S16, "f32": mp3g.OUT_F32, "f32_planar": mp3g.OUT_F32_PLANAR,
             "s16_mono": mp3g.OUT_S16_MONO, "f32_mono": mp3g.OUT_F32_MONO}
    fmts = [(f, known[f]) for f in a.formats.split(",")]
    n_streams, n_frames = 1024, 1024
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        datas = list(ex.map(lambda k: synth.encode_stream(1 + k, n_frames), range(n_streams)))
    print(f"writer {time.perf_counter() - t:.2f} s", flush=True)
    s = mp3g.scan_streams(datas, n_threads=16)
    n = len(s["granules"])
    print(f"host scan alone: {s['scan_s'] * 1e3:.1f} ms ({n} granules)", flush=True)
    hp = torch.empty(n * 1152, dtype=torch.int16).pin_memory()
    dev = torch.device("cuda:0")
    d_p = torch.empty(n * 1152, dtype=torch.int16, device=dev)
    inb = s["granules"].nbytes + s["jobs"].nbytes + s["main_data"].nbytes
    hin = torch.empty(inb, dtype=torch.uint8).pin_memory()
    d_in = torch.empty(inb, dtype=torch.uint8, device=dev)
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        hp.copy_(d_p, non_blocking=True)
        torch.cuda.synchronize()
        d2h = time.perf_counter() - t
        t = time.perf_counter()
        d_in.copy_(hin, non_blocking=True)
        torch.cuda.synchronize()
        h2d = time.perf_counter() - t
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        t = time.perf_counter()
        with torch.cuda.stream(s1):
            hp.copy_(d_p, non_blocking=True)
        with torch.cuda.stream(s2):
            d_in.copy_(hin, non_blocking=True)
        torch.cuda.synchronize()
        both = time.perf_counter() - t
    print(f"PCIe: D2H {hp.numel() * 2 / 1e9:.2f} GB {d2h * 1e3:.1f} ms = {hp.numel() * 2 / d2h / 1e9:.1f} GB/s; "
          f"H2D {inb / 1e9:.2f} GB {h2d * 1e3:.1f} ms = {inb / h2d / 1e9:.1f} GB/s; both at once {both * 1e3:.1f} ms",
          flush=True)
    res = {"tool": "tools/pipe_time.py", "workload": f"c3: {n_streams} streams x {n_frames} frames", "granules": n,
           "repeats": reps, "mode": "fast", "host_scan_ms": round(s["scan_s"] * 1e3, 1),
           "pcie_s16": {"d2h_ms": round(d2h * 1e3, 1), "h2d_ms": round(h2d * 1e3, 1), "both_ms": round(both * 1e3, 1)},
           "formats": {}}
    del hp, d_p
    for name, fmt in fmts:
        bpg = mp3g.out_bytes_per_granule(fmt)
        dt = torch.int16 if fmt in (mp3g.OUT_S16, mp3g.OUT_S16_MONO) else torch.float32
        hp = torch.empty(n * bpg // (2 if dt == torch.int16 else 4), dtype=dt).pin_memory()
        # the PCIe time of this format's output bytes alone
        d_p = torch.empty_like(hp, device=dev)
        for _ in range(2):
            torch.cuda.synchronize()
            t = time.perf_counter()
            hp.copy_(d_p, non_blocking=True)
            torch.cuda.synchronize()
            d2h = time.perf_counter() - t
        del d_p
        print(f"{name}: {n * bpg / 1e9:.2f} GB of output, D2H alone {d2h * 1e3:.1f} ms", flush=True)
        res["formats"][name] = {"out_gb": round(n * bpg / 1e9, 3), "d2h_alone_ms": round(d2h * 1e3, 1), "ms": {}}
        ref = None
        for G in groups:
            times = []
            for _ in range(reps):
                t = time.perf_counter()
                n_p, _, st = mp3g.decode_streams_into(datas, hp, mode=mp3g.MODE_FAST, n_threads=16, n_groups=G,
                                                      out_format=fmt)
                times.append(time.perf_counter() - t)
                assert n_p == n and all(x == 7 for x in st)
            same = None
            h = hp[::4099].clone()
            if ref is None:
                ref = h
            else:
                same = bool(torch.equal(h, ref))
            res["formats"][name]["ms"][str(G)] = [round(x * 1e3, 1) for x in times]
            print(f"decode_streams_into {name} n_groups={G}: " + " ".join(f"{x * 1e3:.1f}" for x in times) +
                  f" ms  ({n // 2 / min(times[1:] or times):.3e} frames/s best after the first; PCM same as first: {same})",
                  flush=True)
        del hp
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
