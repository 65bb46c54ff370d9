#!/usr/bin/env python3
"""Delta features and frame context (mp3g.add_deltas, mp3g.stack_frames) on the c3
workload, in one process.

The batch is tools/specaug_time.py's: bench.py's c3 streams (independently seeded
44.1 kHz streams x 1,024 frames, synth.encode_batch seeds 1..), one window of
--seconds at 16 kHz from every one of --streams streams and one --long-seconds
window from the first --long-streams, both from decode_windows_resampled_tensor
(fast mode, mono).  The features are MFCC's [B, F, 40] (40 mel bins, 40
coefficients) and FBank's [B, F, 80].  Three legs, each with its own yardsticks,
alternating inside every round on the same device tensors; a leg's time is the
median of its windows (HIP events on the launch stream; one untimed launch of the
leg before each window):

  deltas_2_2   add_deltas(order=2, window=2) of the MFCC tensor  -> [B, F, 120]
  splice_3_3   stack_frames(3, 3, 1, 0) of the fbank tensor      -> [B, F, 560]
  lfr_7_6      stack_frames(**lfr_options(7, 6)) of the same     -> [B, ceil(F / 6), 560]
  <leg>.clone     torch.clone of a tensor of the leg's OUTPUT size: the floor for the bytes moved
  <leg>.torch     the torch formulation on the same device: a grouped conv1d per
                  order over the replicate-padded rows plus a cat (deltas); one
                  index_select with the clamped frame indices (the gathers).  Both
                  treat every row as F frames long: they do less than the legs.
  <leg>.features  MFCC.execute / FBank.execute on the same batch: the launch before it

Every leg's output is compared with its host reference on a subset of the rows
before a line is written, and the torch formulations on the rows that are F frames
long.  Writes one JSON line per batch to profiles/framectx_c3.json (and prints
them).

  python tools/framectx_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 1024]
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


def torch_deltas(torch, x, weights, window):
    """[B, F, C] -> [B, F, (O + 1) C]: per order a grouped conv1d over the replicate-padded rows, then a cat."""
    rows = x.transpose(1, 2)  # [B, C, F]
    blocks = [x]
    for i, w in enumerate(weights, 1):
        padded = torch.nn.functional.pad(rows, (i * window, i * window), mode="replicate")
        blocks.append(torch.nn.functional.conv1d(padded, w, groups=rows.shape[1]).transpose(1, 2))
    return torch.cat(blocks, -1)


def torch_stack(torch, x, index, n_out):
    """[B, F, C] -> [B, n_out, ctx C]: one index_select with the clamped frame indices."""
    return torch.index_select(x, 1, index).reshape(x.shape[0], n_out, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--long-streams", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--long-seconds", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "framectx_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("framectx_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    rate = 16000
    datas, _, _, _ = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    n_y = mp3g.Resampler(44100, rate).out_len(1152 * a.frames)
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for x in lines:
                fh.write(json.dumps(x) + "\n")

    def bits(t):
        return t.cpu().numpy().view(np.uint32)

    rng = np.random.default_rng(2025)
    lfr = mp3g.lfr_options(7, 6)
    for name, B, seconds in (("short", a.streams, a.seconds), ("long", min(a.long_streams, a.streams), a.long_seconds)):
        T = int(round(seconds * rate))
        starts = rng.integers(0, max(1, n_y - T), B) if T < n_y else np.zeros(B, np.int64)
        x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], starts, T, rate, mode=mp3g.MODE_FAST,
                                                                out_format=mp3g.OUT_F32_MONO, n_threads=16)
        mf, fb = mp3g.MFCC(rate, n_mels=40, n_ceps=40, device=0), mp3g.FBank(rate, device=0)
        F = fb.frames(T)
        assert mf.frames(T) == F
        mfcc, fbank = mf.execute(x).clone(), fb.execute(x).clone()
        flen = np.clip((lengths - fb.N) // fb.hop + 1, 0, F)
        d_flen = torch.from_numpy(flen.astype(np.int32)).to(dev)
        F_lfr = mp3g.stack_frames_count(F, lfr["step"], 0)
        outs = {"deltas_2_2": torch.empty((B, F, 120), dtype=torch.float32, device=dev),
                "splice_3_3": torch.empty((B, F, 560), dtype=torch.float32, device=dev),
                "lfr_7_6": torch.empty((B, F_lfr, 560), dtype=torch.float32, device=dev)}
        scratch = {"mfcc": torch.empty_like(mfcc), "fbank": torch.empty_like(fbank)}
        weights = [torch.from_numpy(s.copy()).to(dev)[None, None, :].repeat(40, 1, 1)
                   for s in mp3g.delta_scales(2, 2)[1:]]

        def index_of(left, right, step, n_out):
            t = torch.arange(n_out, device=dev)[:, None] * step - left
            return (t + torch.arange(left + right + 1, device=dev)[None, :]).clamp_(0, F - 1).reshape(-1)
        idx = {"splice_3_3": index_of(3, 3, 1, F), "lfr_7_6": index_of(lfr["left"], lfr["right"], lfr["step"], F_lfr)}
        kw = dict(stream=st.cuda_stream)
        ours = {"deltas_2_2": lambda: mp3g.add_deltas(mfcc, d_flen, 2, 2, out=outs["deltas_2_2"], **kw),
                "splice_3_3": lambda: mp3g.stack_frames(fbank, d_flen, 3, 3, 1, 0, out=outs["splice_3_3"], **kw),
                "lfr_7_6": lambda: mp3g.stack_frames(fbank, d_flen, out=outs["lfr_7_6"], **lfr, **kw)}
        legs = dict(ours)
        for k in ours:
            legs[k + ".clone"] = (lambda k=k: outs[k].clone())
        legs["deltas_2_2.torch"] = lambda: torch_deltas(torch, mfcc, weights, 2)
        legs["splice_3_3.torch"] = lambda: torch_stack(torch, fbank, idx["splice_3_3"], F)
        legs["lfr_7_6.torch"] = lambda: torch_stack(torch, fbank, idx["lfr_7_6"], F_lfr)
        legs["deltas_2_2.features"] = lambda: mf.execute(x, scratch["mfcc"], stream=st.cuda_stream)
        legs["splice_3_3.features"] = lambda: fb.execute(x, scratch["fbank"], stream=st.cuda_stream)
        # every leg against the host reference on a subset of the rows, before anything is timed
        ks = list(range(0, B, max(1, B // 8)))
        full = [k for k in range(B) if flen[k] == F][:8]
        h_mfcc, h_fbank = mfcc[ks].cpu().numpy(), fbank[ks].cpu().numpy()
        want = {"deltas_2_2": mp3g.add_deltas_host(h_mfcc, flen[ks], 2, 2),
                "splice_3_3": mp3g.stack_frames_host(h_fbank, flen[ks], 3, 3, 1, 0)[0],
                "lfr_7_6": mp3g.stack_frames_host(h_fbank, flen[ks], **lfr)[0]}
        ok, ok_torch = True, True
        for k, fn in ours.items():
            got = fn()
            got = got[0] if isinstance(got, tuple) else got
            ok = ok and np.array_equal(bits(got[ks]), want[k].view(np.uint32))
            if full and k != "deltas_2_2":
                ok_torch = ok_torch and np.array_equal(bits(legs[k + ".torch"]()[full]), bits(got[full]))
        delta_diff = None
        if full:  # (another summation order: the largest difference, not an equality)
            delta_diff = float((legs["deltas_2_2.torch"]()[full] - outs["deltas_2_2"][full]).abs().max())
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
        ms["lfr_7_6.features"] = ms["splice_3_3.features"]
        src = {"deltas_2_2": mfcc, "splice_3_3": fbank, "lfr_7_6": fbank}
        # one read of the input, one write of the output
        moved = {k: (src[k].numel() + outs[k].numel()) * 4 for k in ours}
        emit({"tool": "tools/framectx_time.py", "batch": name, "label": a.label,
              "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {rate} Hz, mono",
              "shapes": {k: [list(src[k].shape), list(outs[k].shape)] for k in ours},
              "valid_frames_median": int(np.median(flen)), "rows_of_full_length": int((flen == F).sum()),
              "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
              "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
              "bytes_moved": moved,
              "tb_per_s": {k: round(moved[k] / ms[k] / 1e9, 3) for k in ours},
              "clone_tb_per_s": {k: round(2 * outs[k].numel() * 4 / ms[k + ".clone"] / 1e9, 3) for k in ours},
              "over_clone": {k: round(ms[k] / ms[k + ".clone"], 3) for k in ours},
              "over_torch": {k: round(ms[k] / ms[k + ".torch"], 3) for k in ours},
              "over_features": {k: round(ms[k] / ms[k + ".features"], 3) for k in ours},
              "torch_gathers_match_on_full_rows": bool(ok_torch), "torch_deltas_max_abs_diff_on_full_rows": delta_diff,
              "outputs_match_host_reference": bool(ok), "device": torch.cuda.get_device_name(dev)})
        mf.close()
        fb.close()
        del mfcc, fbank, outs, scratch, x
        torch.cuda.empty_cache()
        if not ok:
            raise SystemExit("framectx_time: an output differs from the host reference")


if __name__ == "__main__":
    main()
