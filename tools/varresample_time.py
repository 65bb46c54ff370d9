#!/usr/bin/env python3
"""The variable-ratio resampler (VarResampler.rows) on the c3 workload, in one
process, against the polyphase Resampler.rows where that can do the job.

The batch is bench.py's c3 (1,024 independently seeded 44.1 kHz streams x 1,024
frames, synth.encode_batch seeds 1..1024); every stream gives one window of
--seconds at --rate (16 kHz) that starts at a seeded random source position.
One windowed decode (fast mode) fills the intermediate tensor every leg reads.
The legs of a comparison alternate inside every round; a leg's time is the
median of its windows (HIP events on the launch stream).

  (a) generality: every row at speed 1 (441/160), the one-launch kernel with
      its table in global memory (L2) and in LDS, against Resampler.rows "fast".
  (b) speeds 9/10, 1, 11/10 dealt round-robin, "fast": one launch, against
      three polyphase Resamplers (39690, 44100, 48510 -> 16000) and three launches.
  (c) the same, "best": one launch; the polyphase table for 48510 -> 16000 is
      over MP3G_RESAMPLE_MAX_TAPS, so the parent has no counterpart (recorded).
  (d) a factor of its own per row: --streams distinct ratios in [0.9, 1.1].

Writes one JSON line per part to profiles/varresample_c3.json (and prints them).

  python tools/varresample_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--frames 1024]
                                   [--rate 16000] [--parts abcd] [--out FILE]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import json
import os
import statistics
import sys
from fractions import Fraction

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
    ap.add_argument("--rate", type=int, default=16000)
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "varresample_c3.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("varresample_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    h = st.cuda_stream
    fi, B = 44100, a.streams
    datas, _, _, _ = synth.encode_batch(range(1, 1 + B), a.frames, n_threads=16)
    N = 1152 * a.frames  # samples per stream
    T = int(round(a.seconds * a.rate))

    def make(quality, where):
        os.environ["MP3G_VARRESAMPLE_TABLE"] = where  # (read when the object is made)
        v = mp3g.VarResampler(*mp3g.RESAMPLE_QUALITY[quality], device=0)
        del os.environ["MP3G_VARRESAMPLE_TABLE"]
        return v

    vr = {("fast", "l2"): make("fast", "l2"), ("fast", "lds"): make("fast", "lds"), ("best", "l2"): make("best", "l2")}
    v0 = vr[("best", "l2")]
    three = [Fraction(9, 10), Fraction(1), Fraction(11, 10)]
    # every leg's window of stream k starts at source sample pos[k]; the decoded window holds the widest one
    widest = v0.ratio(fi, a.rate, three[2])
    margin = v0.half_width(*widest) + 8
    rng = np.random.default_rng(2024)
    need = (T * widest[0]) // widest[1] + 2 * margin
    pos = rng.integers(margin, N - need, B)
    win = np.zeros(B, mp3g.WINDOW_DTYPE)
    win["start"], win["n_samples"] = pos - margin, need
    s = mp3g._scan_windows(datas, win["start"], win["n_samples"], False, 16)
    n = len(s["granules"])
    d_g = torch.from_numpy(s["granules"].view(np.uint8)).to(dev)
    d_j = torch.from_numpy(s["jobs"].view(np.uint8)).to(dev)
    d_m = torch.from_numpy(s["main_data"]).to(dev)
    d_c = torch.empty(n * 1152, dtype=torch.int16, device=dev)
    mp3g.huffman_execute(d_j, n, d_m, d_g, d_c, stream=h,
                         flags=mp3g.HUFF_ROWS_COUNT1 | mp3g.huffman_stage_flags(s["jobs"], n))
    inter = torch.zeros((B, 2, need), dtype=torch.float32, device=dev)
    batch = torch.zeros((B, 2, T), dtype=torch.float32, device=dev)
    wplan = mp3g.WindowPlan(s["streams"], s["rows"], need, mode=mp3g.MODE_FAST)
    wplan.execute(d_g, d_c, inter, stream=h, out_format=mp3g.OUT_F32_PLANAR)
    torch.cuda.synchronize(dev)
    wplan.close()
    x = inter.cpu().numpy()
    n_valid = s["rows"]["n_valid"]

    base = {"tool": "tools/varresample_time.py",
            "workload": f"c3: {B} streams x {a.frames} frames, {fi} Hz -> {a.rate} Hz windows of {T} samples",
            "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "source_row_samples": int(need),
            "device": torch.cuda.get_device_name(dev), "lib": os.path.basename(mp3g.lib_path())}
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for y in lines:
                fh.write(json.dumps(y) + "\n")

    def alternate(legs):
        """legs: {name: fn}; ({name: median ms per call}, {name: windows})."""
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize(dev)
        w = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record(st)
                for _ in range(a.steps):
                    fn()
                e1.record(st)
                torch.cuda.synchronize(dev)
                w[k].append(e0.elapsed_time(e1) / a.steps)
        return ({k: round(statistics.median(t), 4) for k, t in w.items()},
                {k: [round(y, 4) for y in t] for k, t in w.items()})

    def var_rows(speeds):
        """Rows of the one-launch kernel: stream k at speeds[k], its window starting at source sample pos[k]."""
        rows = np.zeros(B, mp3g.VARRESAMPLE_ROW_DTYPE)
        for k in range(B):
            num, den = v0.ratio(fi, a.rate, speeds[k])
            rows[k] = (-(-int(pos[k]) * den // num), int(win["start"][k]), k, k, int(n_valid[k]), T, num, den, 1.0, 0)
        return rows

    def poly_rows(r, ks):
        rows = np.zeros(len(ks), mp3g.RESAMPLE_ROW_DTYPE)
        for i, k in enumerate(ks):
            rows[i] = (-(-int(pos[k]) * r.L // r.M), int(win["start"][k]), k, k, int(n_valid[k]), T)
        return rows

    def up(rows):
        return torch.from_numpy(rows.view(np.uint8).copy()).to(dev)

    def var_matches(v, rows):
        v.rows(inter, batch, up(rows), stream=h)
        torch.cuda.synchronize(dev)
        got = batch.cpu().numpy()
        ok = True
        for k in range(0, B, 97):
            r = rows[k]
            want = v.host(x[k, 1, :int(r["n_src"])], int(r["src_origin"]), int(r["out_start"]), T, int(r["num"]),
                          int(r["den"]))
            ok = ok and np.array_equal(got[k, 1].view(np.uint32), want.view(np.uint32))
        return bool(ok)

    def taps(v, rows):
        return float(np.mean([2 * v.half_width(int(r["num"]), int(r["den"])) for r in rows]))

    outs = B * 2 * T
    ok_all = True
    if "a" in a.parts:
        rows = var_rows([1] * B)
        d_rows = up(rows)
        r = mp3g.Resampler(fi, a.rate, *mp3g.RESAMPLE_FAST, device=0)
        d_prow = up(poly_rows(r, range(B)))
        ms, wins = alternate({
            "polyphase_rows_fast": lambda: r.rows(inter, batch, d_prow, stream=h),
            "var_rows_fast_table_l2": lambda: vr[("fast", "l2")].rows(inter, batch, d_rows, stream=h),
            "var_rows_fast_table_lds": lambda: vr[("fast", "lds")].rows(inter, batch, d_rows, stream=h)})
        ok = var_matches(vr[("fast", "l2")], rows) and var_matches(vr[("fast", "lds")], rows)
        ok_all = ok_all and ok
        emit(dict(base, part="a_speed_1", ms=ms, ms_windows=wins, taps_per_output={"polyphase": 2 * r.W, "var": taps(vr[("fast", "l2")], rows)},
                  ns_per_output={k: round(t * 1e6 / outs, 4) for k, t in ms.items()},
                  cost_of_generality=round(ms["var_rows_fast_table_l2"] / ms["polyphase_rows_fast"], 3),
                  lds_table_over_l2_table=round(ms["var_rows_fast_table_lds"] / ms["var_rows_fast_table_l2"], 3),
                  rows_match_host_reference=ok))
        r.close()
    speeds3 = [three[k % 3] for k in range(B)]
    if "b" in a.parts:
        rows = var_rows(speeds3)
        d_rows = up(rows)
        rs = [mp3g.Resampler(int(fi * sp), a.rate, *mp3g.RESAMPLE_FAST, device=0) for sp in three]
        d_prows = [up(poly_rows(rs[j], range(j, B, 3))) for j in range(3)]

        def grouped():
            for j in range(3):
                rs[j].rows(inter, batch, d_prows[j], stream=h)

        ms, wins = alternate({
            "polyphase_three_launches_fast": grouped,
            "var_one_launch_fast_table_l2": lambda: vr[("fast", "l2")].rows(inter, batch, d_rows, stream=h),
            "var_one_launch_fast_table_lds": lambda: vr[("fast", "lds")].rows(inter, batch, d_rows, stream=h)})
        ok = var_matches(vr[("fast", "l2")], rows) and var_matches(vr[("fast", "lds")], rows)
        ok_all = ok_all and ok
        emit(dict(base, part="b_three_speeds_fast", ms=ms, ms_windows=wins,
                  polyphase=[{"fi": x_.fi, "L": x_.L, "M": x_.M, "W": x_.W, "tile": x_.tile} for x_ in rs],
                  taps_per_output_var=taps(vr[("fast", "l2")], rows),
                  one_launch_over_three=round(ms["var_one_launch_fast_table_l2"] / ms["polyphase_three_launches_fast"], 3),
                  rows_match_host_reference=ok))
        for x_ in rs:
            x_.close()
    if "c" in a.parts:
        rows = var_rows(speeds3)
        d_rows = up(rows)
        parent = []
        for sp in three:
            try:
                r = mp3g.Resampler(int(fi * sp), a.rate, *mp3g.RESAMPLE_BEST)
                parent.append({"fi": r.fi, "L": r.L, "M": r.M, "W": r.W, "table_entries": int(r.L * 2 * r.W)})
                r.close()
            except mp3g.Mp3gError as e:
                parent.append({"fi": int(fi * sp), "refused_status": e.status, "error": str(e)[:160]})
        ms, wins = alternate({"var_one_launch_best": lambda: v0.rows(inter, batch, d_rows, stream=h)})
        ok = var_matches(v0, rows)
        ok_all = ok_all and ok
        emit(dict(base, part="c_three_speeds_best", ms=ms, ms_windows=wins, polyphase_best_tables=parent,
                  taps_per_output_var=taps(v0, rows), rows_match_host_reference=ok))
    if "d" in a.parts:
        speeds = [Fraction(9000 + (2000 * k) // max(1, B - 1), 10000) for k in range(B)]
        rows = var_rows(speeds)
        d_rows = up(rows)
        distinct = len({(int(r["num"]), int(r["den"])) for r in rows})
        ms, wins = alternate({
            "var_fast_table_l2": lambda: vr[("fast", "l2")].rows(inter, batch, d_rows, stream=h),
            "var_fast_table_lds": lambda: vr[("fast", "lds")].rows(inter, batch, d_rows, stream=h),
            "var_best": lambda: v0.rows(inter, batch, d_rows, stream=h)})
        ok = var_matches(vr[("fast", "l2")], rows) and var_matches(vr[("fast", "lds")], rows) and var_matches(v0, rows)
        ok_all = ok_all and ok
        emit(dict(base, part="d_ratio_per_row", distinct_ratios=distinct, ms=ms, ms_windows=wins,
                  largest_den=int(rows["den"].max()), rows_match_host_reference=ok))
    if not ok_all:
        raise SystemExit("varresample_time: a resampled row differs from the host reference")


if __name__ == "__main__":
    main()
