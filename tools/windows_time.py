#!/usr/bin/env python3
"""Windowed decode (WindowPlan / decode_windows_tensor) against the full
decode on the c3 workload, in one process.

The batch is bench.py's c3 (1,024 independently seeded streams x 1,024 frames,
synth.encode_batch seeds 1..1024).  The legs of a comparison alternate inside
every round, each window of --steps launches bracketed by a device
synchronise and timed with HIP events on the launch stream; a leg's time is
the median of its windows.

  (a) launch: the windowed plan alone -- one window of --seconds per stream at
      seeded random starts -- against the full MP3G_OUT_F32_PLANAR launch on
      the same streams (the existing instantiations are the parent's,
      instruction for instruction: DESIGN.md section 9b), with the ratio of
      decoded granules (lead included) to all granules beside the measured one.
  (b) store: the windowed store against the plain planar / float-mono stores,
      full-length windows at start 0 (the same granules, every one stored).
  (c) end to end: decode_windows_tensor against decode_streams_tensor plus
      slicing into a batch, host wall time, with the host scan's share.

Writes one JSON line per part to profiles/windows_c3.json (and prints them).

  python tools/windows_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--frames 1024]
                               [--parts abc] [--out FILE]

(MP3G_LIB=another build of the library: the A/B of a kernel variant, e.g. part b
with -DMP3G_WIN_INSIDE_PATH=1.)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--e2e-rounds", type=int, default=2)
    ap.add_argument("--parts", default="abc", help="which of the parts (a, b, c) to run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "windows_c3.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("windows_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    datas, g, c, s = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    n, per = len(g), 2 * a.frames
    N = 576 * per  # samples per stream
    T = int(round(a.seconds * 44100))
    rng = np.random.default_rng(2024)
    starts = rng.integers(0, N - T, a.streams)
    d_g = torch.from_numpy(g.view(np.uint8)).to(dev)
    d_c = torch.from_numpy(c.view(np.uint8).reshape(-1)).to(dev)
    base = {"tool": "tools/windows_time.py", "workload": f"c3: {a.streams} streams x {a.frames} frames",
            "granules": n, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
            "device": torch.cuda.get_device_name(dev), "lib": os.path.basename(mp3g.lib_path())}
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        """Print the line and rewrite the output file (a later part may run out of memory)."""
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

    # ---- (a) the windowed launch against the full planar launch ----
    w = mp3g.scan_windows(datas, starts, T, n_threads=16)
    ws, rows = w["streams"], w["rows"]
    # the windowed runs' descriptors and coefficients: rows of the full batch
    # (run k = granules [lo_k - lead_k, ...) of stream k)
    lo = starts // 576
    src = np.concatenate([np.arange(int(ws["n_granules"][k])) + per * k + int(lo[k]) - int(rows["lead"][k])
                          for k in range(a.streams)])
    idx = torch.from_numpy(src).to(dev)
    dw_g = d_g.view(n, -1)[idx].contiguous().view(-1)
    dw_c = d_c.view(n, -1)[idx].contiguous().view(-1)
    for mode_name, mode in (("fast", mp3g.MODE_FAST), ("exact", mp3g.MODE_EXACT)) if "a" in a.parts else ():
        full_out = torch.empty(n * 1152, dtype=torch.float32, device=dev)
        batch = torch.zeros((a.streams, 2, T), dtype=torch.float32, device=dev)
        plan = mp3g.Plan(s, mode=mode)
        wplan = mp3g.WindowPlan(ws, rows, T, mode=mode)
        ms, wins = alternate({
            "full_planar": lambda: plan.execute(d_g, d_c, full_out, stream=h, out_format=mp3g.OUT_F32_PLANAR),
            "windowed_planar": lambda: wplan.execute(dw_g, dw_c, batch, stream=h, out_format=mp3g.OUT_F32_PLANAR)})
        # the numbers are only worth keeping if the rows are the full decode's
        views = mp3g.planar_views(full_out, s)
        ok = all(torch.equal(batch[k], views[k][:, int(starts[k]):int(starts[k]) + T]) for k in range(0, a.streams, 37))
        info, winfo = plan.info(), wplan.info()
        decoded = int(ws["n_granules"].sum())
        emit(dict(base, part="a_launch", mode=mode_name, window_samples=T, ms=ms, ms_windows=wins,
                          granules_decoded=decoded, granules_ratio=round(decoded / n, 5),
                          measured_ratio=round(ms["windowed_planar"] / ms["full_planar"], 5),
                          plan_full=info, plan_windowed=winfo, rows_match_full_decode=bool(ok)))
        plan.close()
        wplan.close()
        del full_out, batch
        if not ok:
            raise SystemExit("windows_time: a windowed row differs from the full decode")
    del dw_g, dw_c, idx

    # ---- (b) the store stage: full-length windows at start 0 ----
    frows = np.zeros(a.streams, mp3g.WINDOW_ROW_DTYPE)
    frows["n_valid"] = N
    for mode_name, mode in (("fast", mp3g.MODE_FAST), ("exact", mp3g.MODE_EXACT)) if "b" in a.parts else ():
        out_a = torch.empty(n * 1152, dtype=torch.float32, device=dev)
        out_b = torch.empty((a.streams, 2, N), dtype=torch.float32, device=dev)
        plan = mp3g.Plan(s, mode=mode)
        wplan = mp3g.WindowPlan(s, frows, N, mode=mode)
        ms, wins = alternate({
            "planar": lambda: plan.execute(d_g, d_c, out_a, stream=h, out_format=mp3g.OUT_F32_PLANAR),
            "windowed_planar": lambda: wplan.execute(d_g, d_c, out_b, stream=h, out_format=mp3g.OUT_F32_PLANAR),
            "f32_mono": lambda: plan.execute(d_g, d_c, out_a, stream=h, out_format=mp3g.OUT_F32_MONO),
            "windowed_mono": lambda: wplan.execute(d_g, d_c, out_b, stream=h, out_format=mp3g.OUT_F32_MONO)})
        plan.execute(d_g, d_c, out_a, stream=h, out_format=mp3g.OUT_F32_PLANAR)
        wplan.execute(d_g, d_c, out_b, stream=h, out_format=mp3g.OUT_F32_PLANAR)
        torch.cuda.synchronize(dev)
        ok = bool(torch.equal(out_a, out_b.view(-1)))  # (a full-length row IS the stream's plane pair)
        emit(dict(base, part="b_store", mode=mode_name, ms=ms, ms_windows=wins,
                          ns_per_granule={k: round(v * 1e6 / n, 3) for k, v in ms.items()},
                          ratio={"planar": round(ms["windowed_planar"] / ms["planar"], 4),
                                 "mono": round(ms["windowed_mono"] / ms["f32_mono"], 4)},
                          full_length_rows_match=ok))
        plan.close()
        wplan.close()
        del out_a, out_b
        if not ok:
            raise SystemExit("windows_time: full-length windowed rows differ from the planar output")
    del d_g, d_c
    torch.cuda.empty_cache()

    # ---- (c) end to end, host wall time ----
    e2e = {"windowed": [], "windowed_scan": [], "full_then_slice": [], "full_scan": []}
    for _ in range(a.e2e_rounds if "c" in a.parts else 0):
        t0 = time.perf_counter()
        batch, lengths, _ = mp3g.decode_windows_tensor(datas, starts, T, mode=mp3g.MODE_FAST, n_threads=16)
        torch.cuda.synchronize(dev)
        e2e["windowed"].append(time.perf_counter() - t0)
        e2e["windowed_scan"].append(mp3g.scan_windows(datas, starts, T, n_threads=16)["scan_s"])
        t0 = time.perf_counter()
        out, views, _, _ = mp3g.decode_streams_tensor(datas, mode=mp3g.MODE_FAST, n_threads=16)
        ref = torch.zeros((a.streams, 2, T), dtype=torch.float32, device=dev)
        for k in range(a.streams):
            ref[k] = views[k][:, int(starts[k]):int(starts[k]) + T]
        torch.cuda.synchronize(dev)
        e2e["full_then_slice"].append(time.perf_counter() - t0)
        ok = bool(torch.equal(ref, batch))
        del out, views, ref, batch
        torch.cuda.empty_cache()
        e2e["full_scan"].append(mp3g.scan_streams(datas, n_threads=16)["scan_s"])
        if not ok:
            raise SystemExit("windows_time: decode_windows_tensor differs from the sliced full decode")
    if "c" not in a.parts:
        return
    emit(dict(base, part="c_end_to_end", mode="fast", window_samples=T, host_threads=16,
                      seconds={k: [round(x, 4) for x in v] for k, v in e2e.items()},
                      best_seconds={k: round(min(v), 4) for k, v in e2e.items()},
                      speedup=round(min(e2e["full_then_slice"]) / min(e2e["windowed"]), 2)))


if __name__ == "__main__":
    main()
