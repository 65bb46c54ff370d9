#!/usr/bin/env python3
"""The Kaldi filter-bank features (FBank.execute) on the c3 workload, in one process.

The batch is bench.py's c3 (independently seeded 44.1 kHz streams x 1,024
frames, synth.encode_batch seeds 1..): every one of --streams streams gives one
window of --seconds at 16 kHz, and the first --long-streams give one
--long-seconds window (the streams are 26.7 s long: its tail is the dense
batch's zero padding).  Both come from decode_windows_resampled_tensor (fast
mode, mono).  The three legs alternate inside every round on the same device
tensor; a leg's time is the median of its windows (HIP events on the launch
stream):

  fbank_execute    FBank.execute: Kaldi's defaults, 25 ms / 10 ms, 80 bands
  logmel_execute   LogMel.execute(400, 160, 80) without the clamp: the yardstick
                   kernel (7 bin tiles of 32 where the filter bank has 8)
  torch_baseline   unfold, mean, pre-emphasis, window, torch.fft.rfft(n=512),
                   power, mel matmul, log

with the kernel's FMA rate (2 flop per sample, bin and cos/sin of every frame)
against the 157.3 TF/s FP32 peak and the largest difference from the baseline.

Writes one JSON line per batch to profiles/fbank_c3.json (and prints them).

  python tools/fbank_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
                             [--frames 1024] [--out FILE] [--label TEXT] [--no-remove-dc]

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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fbank_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    ap.add_argument("--no-remove-dc", action="store_true", help="without the per-frame mean (what the mean's chain costs)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("fbank_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    rate, n_mels = 16000, 80
    datas, _, _, _ = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    n_y = mp3g.Resampler(44100, rate).out_len(1152 * a.frames)
    fb = mp3g.FBank(rate, n_mels=n_mels, remove_dc=not a.no_remove_dc, device=0)
    lm = mp3g.LogMel(rate, fb.N, fb.hop, n_mels, center=False, clamp=False, device=0)
    N, hop, P = fb.N, fb.hop, fb.P
    window = torch.from_numpy(fb.w.copy()).to(dev)
    filters = torch.from_numpy(fb.wm.copy()).to(dev)
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for x in lines:
                fh.write(json.dumps(x) + "\n")

    def baseline(x):
        s = x.unfold(-1, N, hop) * fb.scale
        if fb.remove_dc:
            s = s - s.mean(dim=-1, keepdim=True)
        e = s - fb.preemphasis * torch.cat([s[..., :1], s[..., :-1]], dim=-1)
        sp = torch.fft.rfft(e * window, n=P)[..., :-1]
        return torch.clamp((sp.real ** 2 + sp.imag ** 2) @ filters.T, min=2.0 ** -23).log()

    rng = np.random.default_rng(2025)
    for name, B, seconds in (("short", a.streams, a.seconds), ("long", min(a.long_streams, a.streams), a.long_seconds)):
        T = int(round(seconds * rate))
        F = fb.frames(T)
        assert F == lm.frames(T)
        starts = rng.integers(0, max(1, n_y - T), B) if T < n_y else np.zeros(B, np.int64)
        x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], starts, T, rate, mode=mp3g.MODE_FAST,
                                                                out_format=mp3g.OUT_F32_MONO, n_threads=16)
        out = torch.empty((B, F, n_mels), dtype=torch.float32, device=dev)
        out_lm = torch.empty((B, n_mels, F), dtype=torch.float32, device=dev)
        legs = {"fbank_execute": lambda: fb.execute(x, out, stream=st.cuda_stream),
                "logmel_execute": lambda: lm.execute(x, out_lm, F, stream=st.cuda_stream),
                "torch_baseline": lambda: baseline(x)}
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
        fb.execute(x, out, stream=st.cuda_stream)
        ref = baseline(x)
        torch.cuda.synchronize(dev)
        diff = float((out - ref).abs().max())
        # the numbers are only worth keeping if the features are the host reference's
        got, rows = out.cpu().numpy(), x.cpu().numpy()
        ks = range(0, B, max(1, B // 4))
        ok = all(np.array_equal(got[k].view(np.uint32), fb.host(rows[k], F).view(np.uint32)) for k in ks)
        flop = 2.0 * B * F * N * 2 * fb.K  # the DFT's useful multiply-adds: every frame, sample, bin, cos and sin
        tiles = -(-F // fb.tile_frames)
        issued = 2.0 * B * tiles * 32 * (-(-N // 4) * 4) * 2 * 32 * (-(-fb.K // 32))  # what the MFMA tiles execute
        t = ms["fbank_execute"] * 1e-3
        emit({"tool": "tools/fbank_time.py", "batch": name, "label": a.label,
              "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {rate} Hz, mono",
              "config": {"N": N, "hop": hop, "P": P, "K": fb.K, "n_mels": n_mels, "remove_dc": fb.remove_dc,
                         "tile_frames": fb.tile_frames},
              "window_samples": T, "frames": F, "valid_samples_median": int(np.median(lengths)),
              "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
              "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
              "fbank_over_logmel": round(ms["fbank_execute"] / ms["logmel_execute"], 3),
              "mfma_work_over_logmel": round(8 / 7, 3),
              "speedup_over_torch_baseline": round(ms["torch_baseline"] / ms["fbank_execute"], 3),
              "useful_fma_tflops": round(flop / t / 1e12, 2),
              "useful_share_of_fp32_peak": round(flop / t / 1e12 / PEAK_FP32_TFLOPS, 4),
              "issued_mfma_tflops": round(issued / t / 1e12, 2),
              "issued_share_of_fp32_peak": round(issued / t / 1e12 / PEAK_FP32_TFLOPS, 4),
              "max_abs_difference_from_torch_baseline": diff, "features_match_host_reference": bool(ok),
              "device": torch.cuda.get_device_name(dev)})
        del x, out, out_lm, ref
        torch.cuda.empty_cache()
        if not ok:
            raise SystemExit("fbank_time: a feature row differs from the host reference")


if __name__ == "__main__":
    main()
