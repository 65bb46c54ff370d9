#!/usr/bin/env python3
"""The log-mel features (LogMel.execute) on the c3 workload, in one process.

The batch is bench.py's c3 (independently seeded 44.1 kHz streams x 1,024
frames, synth.encode_batch seeds 1..): every one of --streams streams gives one
window of --seconds at 16 kHz, and the first --long-streams give one
--long-seconds window (the streams are 26.7 s long: its tail is the dense
batch's zero padding, as Whisper pads).  Both come from
decode_windows_resampled_tensor (fast mode, mono).  The two legs alternate
inside every round on the same device tensor; a leg's time is the median of its
windows (HIP events on the launch stream):

  logmel_execute   LogMel.execute: Whisper's 80-band features, clamp included
  torch_baseline   torch.stft + power + mel matmul + log10 + clamp

with the kernel's FMA rate (2 flop per sample, bin and cos/sin of every frame)
against the 157.3 TF/s FP32 peak and the largest difference between the two.

Writes one JSON line per batch to profiles/logmel_c3.json (and prints them).

  python tools/logmel_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
                              [--frames 1024] [--out FILE]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-mp3_amd"))

PEAK_FP32_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--long-streams", type=int, default=128)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--long-seconds", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "logmel_c3.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("logmel_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    rate, n_fft, hop, n_mels = 16000, 400, 160, 80
    datas, _, _, _ = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    n_y = mp3g.Resampler(44100, rate).out_len(1152 * a.frames)
    lm = mp3g.LogMel(rate, n_fft, hop, n_mels, device=0)
    window = torch.hann_window(n_fft, periodic=True, device=dev)
    filters = torch.from_numpy(lm.wm.copy()).to(dev)
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for x in lines:
                fh.write(json.dumps(x) + "\n")

    def baseline(x):
        s = torch.stft(x, n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True)[..., :-1]
        y = torch.clamp(filters @ (s.real ** 2 + s.imag ** 2), min=1e-10).log10()
        y = torch.maximum(y, y.amax(dim=(1, 2), keepdim=True) - 8.0)
        return (y + 4.0) * 0.25

    rng = np.random.default_rng(2025)
    for name, B, seconds in (("short", a.streams, a.seconds), ("long", min(a.long_streams, a.streams), a.long_seconds)):
        T = int(round(seconds * rate))
        F = T // hop
        starts = rng.integers(0, max(1, n_y - T), B) if T < n_y else np.zeros(B, np.int64)
        x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], starts, T, rate, mode=mp3g.MODE_FAST,
                                                                out_format=mp3g.OUT_F32_MONO, n_threads=16)
        out = torch.empty((B, n_mels, F), dtype=torch.float32, device=dev)
        legs = {"logmel_execute": lambda: lm.execute(x, out, F, stream=st.cuda_stream), "torch_baseline": lambda: baseline(x)}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize(dev)
        win = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record(st)
                for _ in range(a.steps):
                    fn()
                e1.record(st)
                torch.cuda.synchronize(dev)
                win[k].append(e0.elapsed_time(e1) / a.steps)
        ms = {k: round(statistics.median(v), 4) for k, v in win.items()}
        lm.execute(x, out, F, stream=st.cuda_stream)
        ref = baseline(x)
        torch.cuda.synchronize(dev)
        diff = float((out - ref).abs().max())
        # the numbers are only worth keeping if the features are the host reference's
        got, rows = out.cpu().numpy(), x.cpu().numpy()
        ks = range(0, B, max(1, B // 4))
        ok = all(np.array_equal(got[k].view(np.uint32), lm.host(rows[k], F).view(np.uint32)) for k in ks)
        flop = 2.0 * B * F * n_fft * 2 * lm.K  # the DFT's useful multiply-adds: every frame, sample, bin, cos and sin
        tiles = -(-F // lm.tile_frames)
        issued = 2.0 * B * tiles * 32 * n_fft * 2 * 32 * (-(-lm.K // 32))  # what the 32 x 32 MFMA tiles execute, padding included
        t = ms["logmel_execute"] * 1e-3
        emit({"tool": "tools/logmel_time.py", "batch": name,
              "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {rate} Hz, mono",
              "config": {"n_fft": n_fft, "hop": hop, "n_mels": n_mels, "clamp": True, "tile_frames": lm.tile_frames},
              "window_samples": T, "frames": F, "valid_samples_median": int(np.median(lengths)),
              "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
              "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
              "speedup_over_torch_baseline": round(ms["torch_baseline"] / ms["logmel_execute"], 3),
              "useful_fma_tflops": round(flop / t / 1e12, 2),
              "useful_share_of_fp32_peak": round(flop / t / 1e12 / PEAK_FP32_TFLOPS, 4),
              "issued_mfma_tflops": round(issued / t / 1e12, 2),
              "issued_share_of_fp32_peak": round(issued / t / 1e12 / PEAK_FP32_TFLOPS, 4),
              "max_abs_difference_from_torch_baseline": diff, "features_match_host_reference": bool(ok),
              "device": torch.cuda.get_device_name(dev)})
        del x, out, ref
        torch.cuda.empty_cache()
        if not ok:
            raise SystemExit("logmel_time: a feature row differs from the host reference")


if __name__ == "__main__":
    main()
