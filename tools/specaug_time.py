#!/usr/bin/env python3
"""SpecAugment (mp3g.spec_augment) on the c3 workload, in one process.

The batch is tools/frameops_time.py's: bench.py's c3 streams (independently
seeded 44.1 kHz streams x 1,024 frames, synth.encode_batch seeds 1..), one
window of --seconds at 16 kHz from every one of --streams streams and one
--long-seconds window from the first --long-streams, both from
decode_windows_resampled_tensor (fast mode, mono).  The features are FBank's
[B, F, 80] (time-major) and LogMel's [B, 80, F] (frequency-major); the policy is
the paper's LD (time_warp=80, two frequency masks up to 27, two time masks up to
100), drawn once by spec_augment_rows with a seeded generator and uploaded once.
The legs alternate inside every round on the same device tensors; a leg's time is
the median of its windows (HIP events on the launch stream; one untimed launch of
the leg before each window):

  warp_out            (a) out of place with the warp
  masks_out           (b) out of place, masks only
  masks_inplace       (c) in place, masks only
  warp_out_mean       (d) (a) with fill="mean": the sums launch first
  masks_inplace_mean  (d) (c) with fill="mean"
  clone               torch.clone of the same tensor: read once, write once
  copy                Tensor.copy_ into an existing tensor: the same without the allocation
  features_execute    FBank.execute / LogMel.execute on the same batch: the launch this pass follows
  torch_masks         the masks in torch: broadcast compares and one masked_fill
  torch_warp          the warp in torch: the per-row loop of two bicubic
                      interpolate calls on --torch-rows rows, scaled to the batch

Every leg's output is compared with mp3g.spec_augment_host on a subset of the
rows before a line is written.  Writes one JSON line per batch and layout to
profiles/specaug_c3.json (and prints them).

  python tools/specaug_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 1024]
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

LD = dict(time_warp=80, freq_mask_width=27, n_freq_masks=2, time_mask_width=100, n_time_masks=2, time_mask_ratio=1.0)


def torch_masks(torch, feats, rows_t, freq_major):
    """The union of the masks written with 0: time masks (inside each row's length as spec_augment_rows
    draws them) and frequency masks over the row's valid frames."""
    t_lo, t_hi, f_lo, f_hi, n = rows_t
    F, nb = (feats.shape[-1], feats.shape[-2]) if freq_major else (feats.shape[-2], feats.shape[-1])
    t = torch.arange(F, device=feats.device)[None, :, None]
    b = torch.arange(nb, device=feats.device)[None, :, None]
    mt = ((t >= t_lo[:, None, :]) & (t < t_hi[:, None, :])).any(-1)  # [B, F]
    mf = ((b >= f_lo[:, None, :]) & (b < f_hi[:, None, :])).any(-1)  # [B, nb]
    valid = t[:, :, 0] < n[:, None]  # [B, F]
    if freq_major:
        m = (mf[:, :, None] & valid[:, None, :]) | mt[:, None, :]
    else:
        m = (valid[:, :, None] & mf[:, None, :]) | mt[:, :, None]
    return feats.masked_fill(m, 0.0)


def torch_warp(torch, feats, flen, rows, ks, freq_major):
    """ESPnet's time_warp, row by row: two bicubic interpolate calls and a cat."""
    out = []
    for k in ks:
        n, c, w = int(flen[k]), int(rows["warp_center"][k]), int(rows["warp_to"][k])
        x = feats[k].transpose(0, 1) if freq_major else feats[k]  # [F, nb]
        if c == 0:
            out.append(x)
            continue
        live = x[None, None, :n]
        left = torch.nn.functional.interpolate(live[:, :, :c], (w, x.shape[-1]), mode="bicubic", align_corners=False)
        right = torch.nn.functional.interpolate(live[:, :, c:], (n - w, x.shape[-1]), mode="bicubic",
                                                align_corners=False)
        out.append(torch.cat([left[0, 0], right[0, 0], x[n:]], 0))
    return out


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
    ap.add_argument("--torch-rows", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "specaug_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("specaug_time: no gfx950 device")
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
    for name, B, seconds in (("short", a.streams, a.seconds), ("long", min(a.long_streams, a.streams), a.long_seconds)):
        T = int(round(seconds * rate))
        starts = rng.integers(0, max(1, n_y - T), B) if T < n_y else np.zeros(B, np.int64)
        x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], starts, T, rate, mode=mp3g.MODE_FAST,
                                                                out_format=mp3g.OUT_F32_MONO, n_threads=16)
        for layout in ("time_major", "freq_major"):
            fm = layout == "freq_major"
            if fm:
                ob = mp3g.LogMel(rate, device=0)
                F = min(ob.frames(T), T // ob.hop)
                feats = ob.execute(x, n_frames=F).clone()
                flen = np.minimum(F, -(-lengths // ob.hop))
            else:
                ob = mp3g.FBank(rate, device=0)
                F = ob.frames(T)
                feats = ob.execute(x).clone()
                flen = np.clip((lengths - ob.N) // ob.hop + 1, 0, F)
            rows = mp3g.spec_augment_rows(np.random.default_rng(7), flen, 80, **LD)
            d_rows = torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
            d_flen = torch.from_numpy(flen.astype(np.int32)).to(dev)
            out, work, scratch = torch.empty_like(feats), feats.clone(), torch.empty_like(feats)
            kw = dict(freq_major=fm, stream=st.cuda_stream)

            def clip(m, extent):  # (lo, hi) device tensors [B, masks] of the masks in use
                lo = np.minimum(m[..., 0].astype(np.int64), extent)
                hi = np.minimum(lo + m[..., 1], extent)
                return torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)
            rows_t = clip(rows["time"][:, :2], flen[:, None]) + clip(rows["freq"][:, :2], 80) + (d_flen.to(torch.int64),)
            sub = list(range(min(a.torch_rows, B)))
            legs = {"warp_out": lambda: mp3g.spec_augment(feats, d_flen, d_rows, out=out, **kw),
                    "masks_out": lambda: mp3g.spec_augment(feats, d_flen, d_rows, warp=False, out=out, **kw),
                    "masks_inplace": lambda: mp3g.spec_augment(work, d_flen, d_rows, warp=False, out=work, **kw),
                    "warp_out_mean": lambda: mp3g.spec_augment(feats, d_flen, d_rows, fill="mean", out=out, **kw),
                    "masks_inplace_mean": lambda: mp3g.spec_augment(work, d_flen, d_rows, fill="mean", warp=False,
                                                                    out=work, **kw),
                    "clone": lambda: feats.clone(), "copy": lambda: out.copy_(feats),
                    "features_execute": (lambda: ob.execute(x, scratch, n_frames=F, stream=st.cuda_stream)) if fm
                    else (lambda: ob.execute(x, scratch, stream=st.cuda_stream)),
                    "torch_masks": lambda: torch_masks(torch, feats, rows_t, fm),
                    "torch_warp": lambda: torch_warp(torch, feats, flen, rows, sub, fm)}
            # every leg against the host reference on a subset of the rows, before anything is timed
            ks = list(range(0, B, max(1, B // 8)))
            h = feats.cpu().numpy()
            ok = True
            for warp, fill in ((True, 0.0), (False, 0.0), (True, "mean"), (False, "mean")):
                want = mp3g.spec_augment_host(h[ks], flen[ks], rows[ks], fill=fill, freq_major=fm, warp=warp)
                got = mp3g.spec_augment(feats, d_flen, d_rows, fill=fill, warp=warp, out=out, **kw)
                if fill == "mean":
                    ok = ok and np.array_equal(bits(got[1])[ks], want[1].view(np.uint32))
                    got, want = got[0], want[0]
                ok = ok and np.array_equal(bits(got)[ks], want.view(np.uint32))
                if not warp:
                    work.copy_(feats)
                    mp3g.spec_augment(work, d_flen, d_rows, fill=fill, warp=False, out=work, **kw)
                    ok = ok and np.array_equal(bits(work)[ks], want.view(np.uint32))
                    if fill == 0.0:  # the torch formulation of the masks: the same words
                        ok_torch = np.array_equal(bits(torch_masks(torch, feats, rows_t, fm))[ks], want.view(np.uint32))
            work.copy_(feats)
            masked_share = float((bits(mp3g.spec_augment(feats, d_flen, d_rows, warp=False, out=out, **kw))
                                  != bits(feats)).mean())
            for fn in legs.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize(dev)
            win = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    steps = 1 if k == "torch_warp" else a.steps
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    fn()  # (untimed: a window does not start on what the leg before it left behind)
                    torch.cuda.synchronize(dev)
                    e0.record(st)
                    for _ in range(steps):
                        fn()
                    e1.record(st)
                    torch.cuda.synchronize(dev)
                    win[k].append(e0.elapsed_time(e1) / steps)
            ms = {k: round(statistics.median(v), 4) for k, v in win.items()}
            ms["torch_warp_scaled"] = round(ms["torch_warp"] * B / len(sub), 3)
            nbytes = feats.numel() * 4
            emit({"tool": "tools/specaug_time.py", "batch": name, "layout": layout, "label": a.label,
                  "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {rate} Hz, mono",
                  "policy": LD, "shape": list(feats.shape), "valid_frames_median": int(np.median(flen)),
                  "rows_warped": int((rows["warp_center"] > 0).sum()), "masked_share_of_words": round(masked_share, 4),
                  "tensor_bytes": nbytes, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                  "torch_rows": len(sub), "ms": ms,
                  "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
                  "over_clone": {k: round(ms[k] / ms["clone"], 3) for k in ms if k not in ("clone", "torch_warp")},
                  "over_copy": {k: round(ms[k] / ms["copy"], 3) for k in ms if k not in ("copy", "torch_warp")},
                  "copy_gb_per_s": round(2 * nbytes / ms["copy"] / 1e6, 1),
                  "masks_out_over_features_execute": round(ms["masks_out"] / ms["features_execute"], 3),
                  "masks_out_gb_per_s": round(2 * nbytes / ms["masks_out"] / 1e6, 1),
                  "warp_out_gb_per_s": round(2 * nbytes / ms["warp_out"] / 1e6, 1),
                  "torch_masks_match_host_reference": bool(ok_torch),
                  "outputs_match_host_reference": bool(ok), "device": torch.cuda.get_device_name(dev)})
            ob.close()
            del feats, out, work, scratch, h
            torch.cuda.empty_cache()
            if not ok:
                raise SystemExit("specaug_time: an output differs from the host reference")
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
