#!/usr/bin/env python3
"""The resampler (Resampler.rows / decode_windows_resampled_tensor) on the c3
workload, in one process.

The batch is bench.py's c3 (1,024 independently seeded 44.1 kHz streams x 1,024
frames, synth.encode_batch seeds 1..1024); every stream gives one window of
--seconds at --rate (16 kHz), at seeded random starts.  The legs of a
comparison alternate inside every round; a leg's time is the median of its
windows (HIP events on the launch stream for the launches, host wall time end
to end).

  (a) launch: the rows launch alone, "fast" and "best" quality, against the
      windowed decode launch (fast mode) that fills the intermediate tensor it
      reads -- the share of the device time the new stage takes -- with the
      kernel's FMA rate (2 flop per tap and output) against the 157.3 TF/s
      FP32 peak, and its LDS traffic per output.
  (b) end to end: decode_windows_resampled_tensor against what a user does
      without it: decode_windows_tensor at the source rate over hand-computed
      source windows, then a polyphase resampler from torch.nn.functional.conv1d
      with the same taps (L output channels, stride M, the phase offsets folded
      into the weights) and a gather of each row's outputs.

Writes one JSON line per part to profiles/resample_c3.json (and prints them).

  python tools/resample_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--frames 1024]
                                [--rate 16000] [--parts ab] [--out FILE]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-mp3_amd"))

PEAK_FP32_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_c3.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("resample_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    fi, B = 44100, a.streams
    datas, _, _, _ = synth.encode_batch(range(1, 1 + B), a.frames, n_threads=16)
    N = 1152 * a.frames  # samples per stream
    T = int(round(a.seconds * a.rate))
    rs = {q: mp3g.Resampler(fi, a.rate, *mp3g.RESAMPLE_QUALITY[q], device=0) for q in ("fast", "best")}
    L, M = rs["fast"].L, rs["fast"].M
    n_y = rs["fast"].out_len(N)
    rng = np.random.default_rng(2024)
    starts = rng.integers(L, n_y - T, B)  # (>= L: the conv1d leg's source window starts at a sample >= 0)
    base = {"tool": "tools/resample_time.py", "workload": f"c3: {B} streams x {a.frames} frames, {fi} -> {a.rate} Hz",
            "window_samples": T, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
            "device": torch.cuda.get_device_name(dev), "lib": os.path.basename(mp3g.lib_path())}
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for x in lines:
                fh.write(json.dumps(x) + "\n")

    def alternate(legs):
        """legs: {name: fn}; ({name: median ms per call}, {name: windows})."""
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
        return ({k: round(statistics.median(v), 4) for k, v in win.items()},
                {k: [round(x, 4) for x in v] for k, v in win.items()})

    # ---- (a) the rows launch against the windowed decode launch that feeds it ----
    if "a" in a.parts:
        # one intermediate for both qualities: the "best" filter's source windows hold the "fast" filter's
        win = np.zeros(B, mp3g.WINDOW_DTYPE)
        for k in range(B):
            lo, hi = rs["best"].src_window(int(starts[k]), T)
            win["start"][k], win["n_samples"][k] = lo, hi - lo
        T_src = int(win["n_samples"].max())
        s = mp3g._scan_windows(datas, win["start"], win["n_samples"], False, 16)
        n = len(s["granules"])
        d_g = torch.from_numpy(s["granules"].view(np.uint8)).to(dev)
        d_j = torch.from_numpy(s["jobs"].view(np.uint8)).to(dev)
        d_m = torch.from_numpy(s["main_data"]).to(dev)
        d_c = torch.empty(n * 1152, dtype=torch.int16, device=dev)
        mp3g.huffman_execute(d_j, n, d_m, d_g, d_c, stream=h,
                             flags=mp3g.HUFF_ROWS_COUNT1 | mp3g.huffman_stage_flags(s["jobs"], n))
        inter = torch.zeros((B, 2, T_src), dtype=torch.float32, device=dev)
        batch = torch.zeros((B, 2, T), dtype=torch.float32, device=dev)
        wplan = mp3g.WindowPlan(s["streams"], s["rows"], T_src, mode=mp3g.MODE_FAST)
        rows = np.zeros(B, mp3g.RESAMPLE_ROW_DTYPE)
        rows["out_start"], rows["src_origin"] = starts, win["start"]
        rows["src_row"] = rows["out_row"] = np.arange(B)
        rows["n_src"], rows["n_out"] = s["rows"]["n_valid"], T
        d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
        wplan.execute(d_g, d_c, inter, stream=h, out_format=mp3g.OUT_F32_PLANAR)
        ms, wins = alternate({
            "windowed_decode_fast_mode": lambda: wplan.execute(d_g, d_c, inter, stream=h, out_format=mp3g.OUT_F32_PLANAR),
            "rows_fast": lambda: rs["fast"].rows(inter, batch, d_rows, stream=h),
            "rows_best": lambda: rs["best"].rows(inter, batch, d_rows, stream=h)})
        # the numbers are only worth keeping if the rows are the host reference's
        x = inter[:, :, :].cpu().numpy()
        ok = True
        for q in ("fast", "best"):
            rs[q].rows(inter, batch, d_rows, stream=h)
            torch.cuda.synchronize(dev)
            got = batch.cpu().numpy()
            for k in range(0, B, 97):
                want = rs[q].host(x[k, 1, :int(rows["n_src"][k])], int(rows["src_origin"][k]), int(starts[k]), T)
                ok = ok and np.array_equal(got[k, 1].view(np.uint32), want.view(np.uint32))
        outs = B * 2 * T
        kern = {}
        for q in ("fast", "best"):
            W = rs[q].W
            kern[q] = {"taps_per_output": 2 * W,
                       "fma_tflops": round(2.0 * outs * 2 * W / (ms["rows_" + q] * 1e-3) / 1e12, 2),
                       "share_of_fp32_peak": round(2.0 * outs * 2 * W / (ms["rows_" + q] * 1e-3) / 1e12 / PEAK_FP32_TFLOPS, 4),
                       "ns_per_output": round(ms["rows_" + q] * 1e6 / outs, 4),
                       "lds_bytes_read_per_output": 4 * 2 * W,
                       "lds_bytes_written_per_output": round(4 * (M / L + 2 * W / rs[q].tile), 2),
                       "share_of_decode_plus_rows": round(ms["rows_" + q] / (ms["rows_" + q] + ms["windowed_decode_fast_mode"]), 4)}
        emit(dict(base, part="a_launch", ms=ms, ms_windows=wins, source_row_samples=T_src, granules_decoded=n,
                  L=L, M=M, tile=rs["fast"].tile, kernel=kern, rows_match_host_reference=bool(ok)))
        wplan.close()
        del inter, batch, d_g, d_j, d_m, d_c
        torch.cuda.empty_cache()
        if not ok:
            raise SystemExit("resample_time: a resampled row differs from the host reference")

    # ---- (b) end to end against decode_windows_tensor + a conv1d polyphase resampler ----
    def conv1d_leg(q):
        import torch.nn.functional as F
        r = rs[q]
        W = r.W
        # block-aligned: output n = m L + j reads taps h[(j M) mod L] from source m M + (j M) // L - W + 1
        m0 = starts // L
        lo = m0 * M - (W - 1)
        nb = (T + L - 1) // L + 1
        S = (nb - 1) * M + 2 * W + M
        x, lengths, _ = mp3g.decode_windows_tensor(datas, lo, S, mode=mp3g.MODE_FAST, n_threads=16)
        wt = np.zeros((L, 1, 2 * W + M), np.float32)
        for j in range(L):
            off = (j * M) // L
            wt[j, 0, off:off + 2 * W] = r.taps[(j * M) % L]
        y = F.conv1d(x.view(B * 2, 1, S), torch.from_numpy(wt).to(dev), stride=M)  # [B * 2, L, nb]
        y = y.transpose(1, 2).reshape(B, 2, -1)
        idx = torch.from_numpy((starts - m0 * L)[:, None] + np.arange(T)[None, :]).to(dev)
        return torch.gather(y, 2, idx[:, None, :].expand(B, 2, T))

    for q in ("fast", "best") if "b" in a.parts else ():
        e2e = {"resampled_call": [], "windows_then_conv1d": []}
        err, max_diff = None, None
        for rnd in range(a.e2e_rounds + 1):  # (round 0 warms both legs up: library loads, kernel caches)
            t0 = time.perf_counter()
            batch, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas, starts, T, a.rate, mode=mp3g.MODE_FAST,
                                                                        quality=q, n_threads=16)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            try:
                ref = conv1d_leg(q)
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                max_diff = float((ref - batch).abs().max())
                del ref
            except Exception as e:  # (recorded: the comparison leg is another package's kernel)
                err, t2 = repr(e)[:300], None
            if rnd:
                e2e["resampled_call"].append(t1 - t0)
                if t2 is not None:
                    e2e["windows_then_conv1d"].append(t2 - t1)
            del batch
            torch.cuda.empty_cache()
        med = {k: round(statistics.median(v), 4) for k, v in e2e.items() if v}
        emit(dict(base, part="b_end_to_end", mode="fast", quality=q, host_threads=16,
                  seconds={k: [round(x, 4) for x in v] for k, v in e2e.items()}, median_seconds=med,
                  speedup=round(med["windows_then_conv1d"] / med["resampled_call"], 2) if len(med) == 2 else None,
                  conv1d_max_abs_difference=max_diff, conv1d_error=err))


if __name__ == "__main__":
    main()
