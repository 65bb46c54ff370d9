#!/usr/bin/env python3
"""The true peak (mp3g.true_peak) and the range launch (Loudness.execute with
d_range) on the c3 workload, in one process.

The batches are tools/loudness_time.py's: bench.py's c3 streams (independently
seeded 44.1 kHz streams x 1,024 frames), one stereo window of --seconds per
stream at its own 44.1 kHz, and the first --long-streams as one stereo
--long-seconds window at 16 kHz.  Fast mode, planar.  The legs alternate inside
every round on the same device tensor; a leg's time is the median of its
windows (HIP events on the launch stream; one untimed launch of the leg before
each window):

  true_peak         mp3g.true_peak: the tile kernel, then the row kernel
  true_peak_variant the same entry point of --variant-lib (another build of the
                    library: an experiment beside the kept kernel), when one is
                    given
  loudness          Loudness.execute: the yardstick in the same process
  loudness_range    the same with d_range: the range launch behind it
  torch_conv        the same computation in torch: conv1d with the three 12-tap
                    filters, abs, amax over phases and samples, the sample
                    peak, the maximum over planes (over all T samples of every
                    row, whatever its length)

and the shader clock (mp3g.clock_probe) while 12 launches of the first leg run.
A third line times Loudness.execute with and without d_range on ONE row of
--range-blocks short-term blocks (noise whose level wanders, made on the
device): the selection's cost on a 10-minute row.

read_once_ms is the time to read the batch once at 8 TB/s: arithmetic, not a
measurement.  Writes one JSON line per batch to profiles/truepeak_c3.json (and
prints them).

  python tools/truepeak_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
                                [--frames 1024] [--variant-lib FILE] [--out FILE] [--label TEXT]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-mp3_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from stft_time import clock_during  # noqa: E402  (bench.py's clock_leg around a call)

NOT_MEASURED = ["hardware counters (VALU busy, memory traffic, cache hit rates)",
                "rates other than 44,100 and 16,000 Hz", "one plane",
                "the tile kernel and the row kernel apart"]


def timed(torch, dev, st, legs, rounds, steps, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize(dev)
    win = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()  # (untimed: a window does not start on what the leg before it left behind)
            torch.cuda.synchronize(dev)
            e0.record(st)
            for _ in range(steps):
                fn()
            e1.record(st)
            torch.cuda.synchronize(dev)
            win[k].append(e0.elapsed_time(e1) / steps)
    return {k: round(statistics.median(v), 4) for k, v in win.items()}, win


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
    ap.add_argument("--range-blocks", type=int, default=6000)
    ap.add_argument("--variant-lib", default="", help="another libmp3g.so whose mp3g_true_peak_rows is timed too")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "truepeak_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("truepeak_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    variant = C.CDLL(a.variant_lib) if a.variant_lib else None
    if variant is not None:
        vp, u32 = C.c_void_p, C.c_uint32
        variant.mp3g_true_peak_rows.argtypes = [C.c_int, vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
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

    # the interpolator as a conv1d weight: y[n] = sum_t c[t] x[n - t] is a correlation with the reversed taps
    weight = torch.from_numpy(mp3g.true_peak_coefs()[:, ::-1].copy()).to(dev).reshape(3, 1, 12)
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
        d_tp = torch.zeros(B, dtype=torch.float32, device=dev)
        d_tpv = torch.zeros(B, dtype=torch.float32, device=dev)
        d_stats = torch.zeros((B, 32), dtype=torch.uint8, device=dev)
        d_range = torch.zeros((B, 32), dtype=torch.uint8, device=dev)
        d_scratch = torch.zeros(max(1, int(mp3g.lib().mp3g_true_peak_scratch_bytes(B, 2, T)) // 4),
                                dtype=torch.float32, device=dev)
        planes = x.reshape(B * 2, 1, T)

        def torch_conv():
            y = F.conv1d(planes, weight, padding=11)[..., :T]
            return torch.maximum(y.abs().amax(dim=(1, 2)), planes.abs().amax(dim=(1, 2))).reshape(B, 2).amax(dim=1)
        legs = {"true_peak": lambda: mp3g.true_peak(x, lengths=d_len, d_out=d_tp, stream=st.cuda_stream)}
        if variant is not None:
            legs["true_peak_variant"] = lambda: variant.mp3g_true_peak_rows(
                0, x.data_ptr(), B, 2, T, d_len.data_ptr(), None, 0, d_scratch.data_ptr(), d_tpv.data_ptr(),
                st.cuda_stream)
        legs["loudness"] = lambda: ld.execute(x, lengths=d_len, d_stats=d_stats, stream=st.cuda_stream)
        legs["loudness_range"] = lambda: ld.execute(x, lengths=d_len, d_stats=d_stats, d_range=d_range,
                                                    stream=st.cuda_stream)
        legs["torch_conv"] = torch_conv
        ms, win = timed(torch, dev, st, legs, a.rounds, a.steps, a.warmup)
        probe = clock_during(mp3g, torch, dev, legs["true_peak"], launches=12)
        # the numbers are only worth keeping if the results are the host reference's
        rows = x.cpu().numpy()
        ks = list(range(0, B, max(1, B // 4)))
        legs["true_peak"]()
        torch.cuda.synchronize(dev)
        got = d_tp.cpu().numpy()
        want = mp3g.true_peak_host(rows[ks], lengths[ks])
        ok = bool(np.array_equal(got[ks].view(np.uint32), want.view(np.uint32)))
        ok_variant = None
        if variant is not None:
            ok_variant = bool(np.array_equal(d_tpv.cpu().numpy().view(np.uint32), got.view(np.uint32)))
        full = lengths == T  # (torch's leg has no lengths: compared where the row is whole)
        tc = torch_conv().cpu().numpy()
        torch_close = bool(np.allclose(tc[full], got[full], rtol=1e-5, atol=1e-7)) if full.any() else None
        ld.execute(x, lengths=d_len, d_stats=d_stats, d_range=d_range, stream=st.cuda_stream)
        ok_range = mp3g.Loudness.range_stats(d_range)[ks].tobytes() == ld.range_host(rows[ks], lengths[ks]).tobytes()
        read_once = B * 2 * T * 4 / 8e12 * 1e3
        emit({"tool": "tools/truepeak_time.py", "batch": name, "label": a.label,
              "workload": f"c3: {B} streams x {a.frames} frames, one stereo {seconds:g} s window each at {rate} Hz",
              "config": {"rate": rate, "planes": 2, "tile": mp3g.true_peak_tile(),
                         "short_term_blocks_per_row": max(0, T // ld.H - 29)},
              "window_samples": T, "valid_samples_median": int(np.median(lengths)),
              "rows_of_full_length": int(full.sum()),
              "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
              "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
              "read_once_ms_at_8TBps": round(read_once, 4),
              "true_peak_over_read_once": round(ms["true_peak"] / read_once, 2),
              "true_peak_over_torch_conv": round(ms["true_peak"] / ms["torch_conv"], 3),
              "true_peak_over_loudness": round(ms["true_peak"] / ms["loudness"], 3),
              "range_launch_ms": round(ms["loudness_range"] - ms["loudness"], 4),
              "fma_per_s": round(2 * float(np.sum(lengths)) * 36 / (ms["true_peak"] * 1e-3), 0),
              "clock_probe_during_true_peak": probe, "results_match_host_reference": ok,
              "variant_matches": ok_variant, "torch_conv_close_on_whole_rows": torch_close,
              "range_records_match_host_reference": bool(ok_range),
              "not_measured": NOT_MEASURED, "device": torch.cuda.get_device_name(dev)})
        ld.close()
        del x, planes
        torch.cuda.empty_cache()
        if not (ok and ok_range) or ok_variant is False:
            raise SystemExit("truepeak_time: a result differs from the host reference")

    # one long row: the range launch's selection over --range-blocks short-term blocks
    rate = 16000
    ld = mp3g.Loudness(rate, device=0)
    T = (a.range_blocks + 29) * ld.H
    g = torch.Generator(device=dev).manual_seed(7)
    level = 10.0 ** (-1.5 + 1.2 * torch.sin(torch.arange(T, device=dev) * (6.283 / (40 * rate))))
    x = (0.3 * level * torch.randn((1, 2, T), device=dev, generator=g)).contiguous()
    d_stats = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    d_range = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    legs = {"loudness": lambda: ld.execute(x, d_stats=d_stats, stream=st.cuda_stream),
            "loudness_range": lambda: ld.execute(x, d_stats=d_stats, d_range=d_range, stream=st.cuda_stream)}
    ms, win = timed(torch, dev, st, legs, a.rounds, a.steps, a.warmup)
    legs["loudness_range"]()
    got = mp3g.Loudness.range_stats(d_range)
    want = ld.range_host(x.cpu().numpy())
    ok = got.tobytes() == want.tobytes()
    emit({"tool": "tools/truepeak_time.py", "batch": "one_row", "label": a.label,
          "workload": f"one stereo row of {T} samples at {rate} Hz: {a.range_blocks} short-term blocks",
          "record": {k: float(got[0][k]) for k in got.dtype.names}, "steps": a.steps, "warmup": a.warmup,
          "rounds": a.rounds, "ms": ms, "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
          "range_launch_ms": round(ms["loudness_range"] - ms["loudness"], 4),
          "range_record_matches_host_reference": bool(ok), "device": torch.cuda.get_device_name(dev)})
    ld.close()
    if not ok:
        raise SystemExit("truepeak_time: the range record differs from the host reference")


if __name__ == "__main__":
    main()
