#!/usr/bin/env python3
"""The BS.1770 loudness measure (Loudness.execute) and the gain stage
(mp3g.loudness_gain) on the c3 workload, in one process.

The batch is bench.py's c3 (independently seeded 44.1 kHz streams x 1,024
frames, synth.encode_batch seeds 1..): every one of --streams streams gives one
stereo window of --seconds at its own 44.1 kHz (decode_windows_tensor), and the
first --long-streams give one stereo --long-seconds window at 16 kHz
(decode_windows_resampled_tensor; the streams are 26.7 s long: its tail is the
dense batch's zero padding).  Fast mode, planar.  The legs alternate inside
every round on the same device tensor; a leg's time is the median of its
windows (HIP events on the launch stream; one untimed launch of the leg before
each window):

  loudness          Loudness.execute: the segment kernel, then the row kernel
  loudness_no_rows  the same with every length 0: the segment kernel runs its
                    whole loop (its trip count depends on no length), the row
                    kernel has nothing to scan -- the segment kernel's share
  fbank_execute     FBank.execute on the 16 kHz batch: the yardstick
  gain              mp3g.loudness_gain in place (target = what the batch already
                    has, so the samples stay in range over the run)
  torch_mul         torch's in-place multiply by a broadcast [B, 1, 1] tensor

and the shader clock (mp3g.clock_probe) while 12 launches of the first leg run.

read_once_ms is the time to read the batch once at 8 TB/s: arithmetic, not a
measurement.  Writes one JSON line per batch to profiles/loudness_c3.json (and
prints them).

  python tools/loudness_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
                                [--frames 1024] [--out FILE] [--label TEXT]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-mp3_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from stft_time import clock_during  # noqa: E402  (bench.py's clock_leg around a call)

NOT_MEASURED = ["hardware counters (LDS bank conflicts, VALU busy, memory traffic)",
                "rates other than 44,100 and 16,000 Hz", "one plane",
                "the two kernels apart (loudness_no_rows is an estimate of the segment kernel's share)"]


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loudness_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("loudness_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    datas, _, _, _ = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    n_src = 1152 * a.frames
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for x in lines:
                fh.write(json.dumps(x) + "\n")

    rng = np.random.default_rng(2025)
    for name, B, seconds, rate in (("short", a.streams, a.seconds, 44100),
                                   ("long", min(a.long_streams, a.streams), a.long_seconds, 16000)):
        T = int(round(seconds * rate))
        if rate == 44100:
            starts = rng.integers(0, max(1, n_src - T), B)
            x, lengths, _ = mp3g.decode_windows_tensor(datas[:B], starts, T, mode=mp3g.MODE_FAST, n_threads=16)
        else:
            x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], np.zeros(B, np.int64), T, rate,
                                                                    mode=mp3g.MODE_FAST, n_threads=16)
        ld = mp3g.Loudness(rate, device=0)
        d_len = torch.from_numpy(lengths.astype(np.int32)).to(dev)
        d_zero = torch.zeros_like(d_len)
        d_stats = ld.execute(x, lengths=d_len).clone()
        scratch = torch.zeros_like(d_stats)
        stats = mp3g.Loudness.stats(d_stats)
        # the gain that leaves the batch as loud as it is: sqrt(energy / energy) = 1 on most rows
        target = float(np.median(stats["lufs"][np.isfinite(stats["lufs"])]))
        ones = torch.full((B, 1, 1), 1.0, dtype=torch.float32, device=dev)
        legs = {"loudness": lambda: ld.execute(x, lengths=d_len, d_stats=scratch, stream=st.cuda_stream),
                "loudness_no_rows": lambda: ld.execute(x, lengths=d_zero, d_stats=scratch, stream=st.cuda_stream)}
        work = x.clone()
        same = torch.from_numpy(np.ascontiguousarray(
            np.broadcast_to(np.array([(mp3g.loudness_target_energy(target), target, 1.0, 0, 0, 0, 0)],
                                     mp3g.LOUDNESS_STATS_DTYPE), (B,))).view(np.uint8).reshape(B, 32).copy()).to(dev)
        legs["gain"] = lambda: mp3g.loudness_gain(work, same, target, lengths=d_len, stream=st.cuda_stream)
        legs["torch_mul"] = lambda: work.mul_(ones)
        fb = None
        if rate == 16000:
            fb = mp3g.FBank(rate, device=0)
            out_fb = torch.empty((B, 2, fb.frames(T), fb.n_mels), dtype=torch.float32, device=dev)
            legs["fbank_execute"] = lambda: fb.execute(x, out_fb, stream=st.cuda_stream)
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize(dev)
        win = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                fn()  # (untimed: a window does not start on what the leg before it left behind)
                torch.cuda.synchronize(dev)
                e0.record(st)
                for _ in range(a.steps):
                    fn()
                e1.record(st)
                torch.cuda.synchronize(dev)
                win[k].append(e0.elapsed_time(e1) / a.steps)
        ms = {k: round(statistics.median(v), 4) for k, v in win.items()}
        # the shader clock while the same call runs (tools/stft_time.py's probe)
        probe = clock_during(mp3g, torch, dev, legs["loudness"], launches=12)
        # the numbers are only worth keeping if the records are the host reference's
        rows = x.cpu().numpy()
        ks = list(range(0, B, max(1, B // 4)))
        got = mp3g.Loudness.stats(ld.execute(x, lengths=d_len, d_stats=scratch, stream=st.cuda_stream))
        ok = got[ks].tobytes() == ld.host(rows[ks], lengths[ks]).tobytes()
        unchanged = bool(torch.equal(work, x))  # (gain 1 and the multiply by one: the batch as decoded)
        emit({"tool": "tools/loudness_time.py", "batch": name, "label": a.label,
              "workload": f"c3: {B} streams x {a.frames} frames, one stereo {seconds:g} s window each at {rate} Hz",
              "config": {"rate": rate, "H": ld.H, "segments_per_plane": T // ld.H, "planes": 2},
              "window_samples": T, "valid_samples_median": int(np.median(lengths)),
              "lufs_median": target, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
              "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
              "read_once_ms_at_8TBps": round(B * 2 * T * 4 / 8e12 * 1e3, 4),
              "segment_kernel_ms_estimate": ms["loudness_no_rows"],
              "row_kernel_ms_estimate": round(ms["loudness"] - ms["loudness_no_rows"], 4),
              "gain_over_torch_mul": round(ms["gain"] / ms["torch_mul"], 3),
              "clock_probe_during_loudness": probe, "records_match_host_reference": bool(ok), "gain_of_one_left_batch": unchanged,
              "not_measured": NOT_MEASURED, "device": torch.cuda.get_device_name(dev)})
        ld.close()
        if fb is not None:
            fb.close()
        del x, work
        torch.cuda.empty_cache()
        if not ok:
            raise SystemExit("loudness_time: a record differs from the host reference")


if __name__ == "__main__":
    main()
