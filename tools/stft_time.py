#!/usr/bin/env python3
"""The STFT features (STFT.execute) on the c3 workload, in one process.

The batch is bench.py's c3 (independently seeded 44.1 kHz streams x 1,024
frames, synth.encode_batch seeds 1..): every one of --streams streams gives one
window of --seconds at its native 44.1 kHz (the copied path), and the first
--long-streams give one --long-seconds window (the streams are 26.7 s long: its
tail is the dense batch's zero padding).  Both come from
decode_windows_resampled_tensor (fast mode, mono).  The legs alternate inside
every round on the same device tensor; a leg's time is the median of its
windows (HIP events on the launch stream):

  stft_power_2048      STFT.execute(2048, 512, power): librosa's defaults
  torch_power_2048     torch.stft(..).abs() ** 2
  stft_mel_2048        STFT.execute(2048, 512, power, 128 mels, ln, floor 1e-5)
  torch_mel_2048       torch.stft, abs() ** 2, a matmul with the same filters, clamp, log
  stft_complex_4096    STFT.execute(4096, 1024, complex): a source-separation front end
  torch_complex_4096   torch.stft(4096, 1024)
  stft_mel_1024        STFT.execute(1024, 256, power, 80 mels, log10, floor 1e-10)
  logmel_1024          LogMel.execute(1024, 256, 80) without the clamp: the direct DFT
                       on the f32 MFMA at the same size -- would an FFT pay there too?

with the kernel's useful flop rate (2.5 P log2 P per frame, the real transform's
count), the LDS bytes a frame moves, and the shader clock from
mp3g_debug_clock_probe while the first leg's launches run.

Writes one JSON line per batch to profiles/stft_c3.json (and prints them).

  python tools/stft_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
                            [--frames 1024] [--out FILE] [--label TEXT]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-mp3_amd"))

RATE = 44100


def lds_bytes_per_frame(st):
    """What stft.hip moves through LDS for one frame: the windowed values in, every
    pass and the split step read and written in place, the epilogue's reads."""
    n = st.n_fft // 2
    # round trips of the passes: three from n_fft = 2048 (two double passes and what is left), else one per pass
    passes = 3 if st.n_fft >= 2048 else (int(math.log2(n)) + 1) // 2
    read_out = st.K * (8 if st.complex else 4) if not st.n_mels else 2 * st.K * 4  # (a bin lies in <= 2 filters)
    return n * 8 * (1 + 2 * passes + 2) + read_out


def clock_during(mp3g, torch, dev, fn, launches=12):
    """bench.py's clock_leg around `launches` calls of fn."""
    import numpy as np
    if not hasattr(mp3g.lib(), "mp3g_debug_clock_probe"):
        return None
    main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.zeros(8 * 5, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    mp3g.clock_probe(flag, out, 8, 5000, stream=side.cuda_stream, device=0)
    for _ in range(launches):
        fn()
    flag.fill_(1)  # (on the main stream, after the launches)
    torch.cuda.synchronize(dev)
    rows = out.view(8, 5).cpu().numpy().astype(np.float64)
    dt, dr = rows[:, 1] - rows[:, 0], rows[:, 3] - rows[:, 2]
    ok = (rows[:, 4] != 0) & (dr > 0)
    if not ok.any():
        return {"clock_ghz": None, "note": "no probe saw the flag"}
    clk = dt[ok] / dr[ok] * 0.1  # GHz: memrealtime ticks at 100 MHz
    return {"clock_ghz": round(float(np.median(clk)), 4), "min_ghz": round(float(clk.min()), 4),
            "max_ghz": round(float(clk.max()), 4), "window_ms": round(float(np.median(dr[ok])) / 1e5, 2),
            "probes": int(ok.sum())}


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stft_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("stft_time: no gfx950 device")
    dev = torch.device("cuda:0")
    cur = torch.cuda.current_stream(dev)
    datas, _, _, _ = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    n_y = 1152 * a.frames
    objs = {"power_2048": mp3g.STFT(RATE, 2048, 512, output="power", device=0),
            "mel_2048": mp3g.STFT(RATE, 2048, 512, output="power", n_mels=128, log="ln", floor=1e-5, device=0),
            "complex_4096": mp3g.STFT(RATE, 4096, 1024, output="complex", device=0),
            "mel_1024": mp3g.STFT(RATE, 1024, 256, output="power", n_mels=80, log="log10", floor=1e-10, device=0)}
    lm = mp3g.LogMel(RATE, 1024, 256, 80, clamp=False, device=0)
    hann = {p: torch.hann_window(p, periodic=True, dtype=torch.float32, device=dev) for p in (2048, 4096)}
    filters = torch.from_numpy(objs["mel_2048"].wm.copy()).to(dev)
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for x in lines:
                fh.write(json.dumps(x) + "\n")

    def t_stft(x, p, hop):
        return torch.stft(x, p, hop, window=hann[p], center=True, pad_mode="reflect", return_complex=True)

    rng = np.random.default_rng(2025)
    for name, B, seconds in (("short", a.streams, a.seconds), ("long", min(a.long_streams, a.streams), a.long_seconds)):
        T = int(round(seconds * RATE))
        starts = rng.integers(0, max(1, n_y - T), B) if T < n_y else np.zeros(B, np.int64)
        x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], starts, T, RATE, mode=mp3g.MODE_FAST,
                                                                out_format=mp3g.OUT_F32_MONO, n_threads=16)
        F = {k: st.frames(T) for k, st in objs.items()}
        outs = {k: torch.empty((B, st.bins, F[k]) + ((2,) if st.complex else ()), dtype=torch.float32, device=dev)
                for k, st in objs.items()}
        out_lm = torch.empty((B, 80, lm.frames(T)), dtype=torch.float32, device=dev)
        legs = {}
        for k, st in objs.items():
            legs["stft_" + k] = (lambda st=st, k=k: st.execute(x, outs[k], F[k], stream=cur.cuda_stream))
        legs["torch_power_2048"] = lambda: t_stft(x, 2048, 512).abs() ** 2
        legs["torch_mel_2048"] = lambda: torch.clamp(filters @ (t_stft(x, 2048, 512).abs() ** 2), min=1e-5).log()
        legs["torch_complex_4096"] = lambda: t_stft(x, 4096, 1024)
        legs["logmel_1024"] = lambda: lm.execute(x, out_lm, out_lm.shape[-1], stream=cur.cuda_stream)
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize(dev)
        win = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record(cur)
                for _ in range(a.steps):
                    fn()
                e1.record(cur)
                torch.cuda.synchronize(dev)
                win[k].append(e0.elapsed_time(e1) / a.steps)
        ms = {k: round(statistics.median(v), 4) for k, v in win.items()}
        clock = clock_during(mp3g, torch, dev, legs["stft_power_2048"])
        # the numbers are only worth keeping if the features are the host reference's
        rows = x.cpu().numpy()
        ks = range(0, B, max(1, B // 3))
        diffs, ok = {}, True
        for k, st in objs.items():
            legs["stft_" + k]()
            torch.cuda.synchronize(dev)
            nf = min(F[k], 64)  # (the first frames of a few rows)
            for r in ks:
                got = outs[k][r, :, :nf].contiguous().cpu().numpy()
                want = st.host(rows[r], nf)
                want = want.view(np.float32).reshape(got.shape) if st.complex else want
                ok = ok and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        ref = t_stft(x[:4], 2048, 512).abs() ** 2
        diffs["power_2048_rel"] = float(((outs["power_2048"][:4] - ref).abs().max() / ref.abs().max()).cpu())
        ref = t_stft(x[:4], 4096, 1024)
        diffs["complex_4096_rel"] = float(((torch.view_as_complex(outs["complex_4096"][:4]) - ref).abs().max()
                                           / ref.abs().max()).cpu())
        per = {}
        for k, st in objs.items():
            flop = 2.5 * st.n_fft * math.log2(st.n_fft) * B * F[k]
            t = ms["stft_" + k] * 1e-3
            per[k] = {"n_fft": st.n_fft, "hop": st.hop, "frames": F[k], "tile_frames": st.tile_frames,
                      "useful_tflops": round(flop / t / 1e12, 3), "frames_per_us": round(B * F[k] / t / 1e6, 3),
                      "lds_bytes_per_frame": lds_bytes_per_frame(st),
                      "lds_tb_per_s": round(lds_bytes_per_frame(st) * B * F[k] / t / 1e12, 3),
                      "output_gb_per_s": round(outs[k].numel() * 4 / t / 1e9, 1)}
        emit({"tool": "tools/stft_time.py", "batch": name, "label": a.label,
              "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {RATE} Hz, mono",
              "window_samples": T, "valid_samples_median": int(np.median(lengths)),
              "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
              "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()}, "kernel": per,
              "speedup_over_torch": {k: round(ms["torch_" + k] / ms["stft_" + k], 3)
                                     for k in ("power_2048", "mel_2048", "complex_4096")},
              "stft_over_logmel_1024": round(ms["stft_mel_1024"] / ms["logmel_1024"], 3),
              "clock_probe_during_stft_power_2048": clock,
              "max_rel_difference_from_torch": diffs, "features_match_host_reference": bool(ok),
              "device": torch.cuda.get_device_name(dev)})
        del x, outs, out_lm, ref
        torch.cuda.empty_cache()
        if not ok:
            raise SystemExit("stft_time: a feature row differs from the host reference")


if __name__ == "__main__":
    main()
