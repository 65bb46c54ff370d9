#!/usr/bin/env python3
"""Plan.execute time per output format (s16, float32 interleaved, float32
planar, s16 mono downmix, float32 mono downmix) on the c3 workload, fast and
exact mode, in one process.

The batch is bench.py's c3 (1,024 independently seeded streams x 1,024 frames,
synth.encode_batch seeds 1..1024).  The formats alternate inside every round
(s16, f32, planar, s16 mono, f32 mono, s16, ...), each window of --steps launches bracketed by a
device synchronise and timed with HIP events on the launch stream; a format's
time is the median of its windows.  Writes one JSON line to
profiles/outfmt_c3.json (and prints it): ms per mode and format, the bytes a
granule moves in each format (the s16 kernel's 4,768 B plus the output
difference) and the implied TB/s.

  python tools/outfmt_time.py [--steps 10] [--warmup 6] [--rounds 5] [--streams 1024] [--frames 1024]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-mp3_amd"))

S16_BYTES_PER_GRANULE = 4768  # what the s16 plan kernel reads + writes per granule


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "outfmt_c3.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("outfmt_time: no gfx950 device")
    dev = torch.device("cuda:0")
    _, g, c, s = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    n = len(g)
    d_g = torch.from_numpy(g.view(np.uint8)).to(dev)
    d_c = torch.from_numpy(c.view(np.uint8).reshape(-1)).to(dev)
    fmts = (("s16", mp3g.OUT_S16), ("f32", mp3g.OUT_F32), ("f32_planar", mp3g.OUT_F32_PLANAR),
            ("s16_mono", mp3g.OUT_S16_MONO), ("f32_mono", mp3g.OUT_F32_MONO))
    d_out = {name: torch.empty(n * mp3g.out_bytes_per_granule(f), dtype=torch.uint8, device=dev) for name, f in fmts}
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    res = {"tool": "tools/outfmt_time.py", "workload": f"c3: {a.streams} streams x {a.frames} frames",
           "granules": n, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(dev), "lib": os.path.basename(mp3g.lib_path()),
           "bytes_per_granule": {name: S16_BYTES_PER_GRANULE + mp3g.out_bytes_per_granule(f) - 2304
                                 for name, f in fmts},
           "ms": {}, "ms_windows": {}, "tb_per_s": {}, "ratio_to_s16": {}}
    for mode_name, mode in (("fast", mp3g.MODE_FAST), ("exact", mp3g.MODE_EXACT)):
        plan = mp3g.Plan(s, mode=mode)
        for name, f in fmts:
            for _ in range(a.warmup):
                plan.execute(d_g, d_c, d_out[name], stream=h, out_format=f)
        torch.cuda.synchronize(dev)
        win = {name: [] for name, _ in fmts}
        for _ in range(a.rounds):
            for name, f in fmts:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record(st)
                for _ in range(a.steps):
                    plan.execute(d_g, d_c, d_out[name], stream=h, out_format=f)
                e1.record(st)
                torch.cuda.synchronize(dev)
                win[name].append(e0.elapsed_time(e1) / a.steps)
        plan.close()
        ms = {name: statistics.median(v) for name, v in win.items()}
        res["ms"][mode_name] = {k: round(v, 4) for k, v in ms.items()}
        res["ms_windows"][mode_name] = {k: [round(x, 4) for x in v] for k, v in win.items()}
        res["tb_per_s"][mode_name] = {k: round(n * res["bytes_per_granule"][k] / (v * 1e-3) / 1e12, 3)
                                      for k, v in ms.items()}
        res["ratio_to_s16"][mode_name] = {k: round(v / ms["s16"], 4) for k, v in ms.items()}
    # the formats must agree before a number is worth keeping: trunc(f * 32768) is the s16 sample
    f32 = d_out["f32"].view(torch.float32)
    q = torch.trunc(f32 * 32768.0).to(torch.int16)
    res["f32_matches_s16"] = bool(torch.equal(q, d_out["s16"].view(torch.int16)))
    # and the mono formats are the downmix of the stereo ones: (L + R) >> 1, (fL + fR) * 0.5f
    lr = d_out["s16"].view(torch.int16).view(-1, 2).to(torch.int32)
    res["s16_mono_matches_s16"] = bool(torch.equal(((lr[:, 0] + lr[:, 1]) >> 1).to(torch.int16),
                                                   d_out["s16_mono"].view(torch.int16)))
    del lr, q
    f2 = f32.view(-1, 2)
    res["f32_mono_matches_f32"] = bool(torch.equal((f2[:, 0] + f2[:, 1]) * 0.5, d_out["f32_mono"].view(torch.float32)))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    if not res["f32_matches_s16"]:
        raise SystemExit("outfmt_time: float output does not quantise to the s16 output")
    if not (res["s16_mono_matches_s16"] and res["f32_mono_matches_f32"]):
        raise SystemExit("outfmt_time: a mono output is not the downmix of its stereo format")


if __name__ == "__main__":
    main()
