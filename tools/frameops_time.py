#!/usr/bin/env python3
"""The sliding-window CMN, the energy VAD and the voiced-frame selection
(mp3g.sliding_cmn, mp3g.vad_energy, mp3g.select_frames) on the c3 workload, in
one process.

The batch is tools/mfcc_time.py's: bench.py's c3 streams (independently seeded
44.1 kHz streams x 1,024 frames, synth.encode_batch seeds 1..), one window of
--seconds at 16 kHz from every one of --streams streams (1,024 x 198 frames) and
one --long-seconds window from the first --long-streams (128 x 2,998 frames),
both from decode_windows_resampled_tensor (fast mode, mono).  For 30 and 40
coefficients (n_mels = n_ceps) the legs alternate inside every round on the same
device tensors; a leg's time is the median of its windows (HIP events on the
launch stream; one untimed launch of the leg before each window):

  sliding_cmn        mp3g.sliding_cmn, centred, 300 frames, the mean only
  sliding_cmn_var    the same with norm_vars
  vad_energy         mp3g.vad_energy, the voxceleb options, on coefficient 0
  select_frames      mp3g.select_frames of the VAD's flags
  front_end          the three launches of the recipe: VAD, sliding mean, selection
  cmvn               mp3g.cmvn (mean only) after the copy that restores its input
  copy_only          that copy
  mfcc_execute       MFCC.execute on the same batch: the stage these follow
  torch_front_end    the same three steps in torch: a float64 cumsum of the
                     tensor, two gathers, the VAD by two convolutions, a
                     boolean-index compaction (it synchronises) and a re-pad;
                     checked against the host references before it is timed

Writes one JSON line per batch and configuration to profiles/frameops_c3.json
(and prints them).

  python tools/frameops_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
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

VOXCELEB = dict(energy_threshold=5.5, energy_mean_scale=0.5, proportion_threshold=0.12, frames_context=2)
W = 300


def torch_front_end(torch, feats, d_flen):
    """(normalised [B, F, S], voiced bool [B, F], selected and re-padded [B, F, S]) in torch."""
    B, F, S = feats.shape
    dev = feats.device
    n = d_flen.to(torch.int64)[:, None]
    t = torch.arange(F, device=dev)[None, :]
    valid = t < n
    # the centred window of include/mp3g.h
    s = (t - W // 2).expand(B, F)
    e = s + W
    e = torch.where(s < 0, e - s, e)
    s = s.clamp(min=0)
    over = (e - n).clamp(min=0)
    s = (s - over).clamp(min=0)
    e = torch.minimum(e, n)
    s = torch.where(valid, s, torch.zeros_like(s))
    e = torch.where(valid, e, torch.ones_like(e))
    x64 = feats.double()
    cs = torch.cat([torch.zeros((B, 1, S), dtype=torch.float64, device=dev), x64.cumsum(1)], dim=1)
    tot = cs.gather(1, e[..., None].expand(B, F, S)) - cs.gather(1, s[..., None].expand(B, F, S))
    mean = tot / (e - s)[..., None].double()
    norm = torch.where(valid[..., None], (x64 - mean).float(), feats)
    # the VAD on the raw log energy
    e0 = feats[..., 0]
    mean0 = (e0.double() * valid).sum(1) / n[:, 0].clamp(min=1).double()
    thr = (VOXCELEB["energy_threshold"] + VOXCELEB["energy_mean_scale"] * mean0).float()
    c = VOXCELEB["frames_context"]
    ones = torch.ones((1, 1, 2 * c + 1), dtype=torch.float32, device=dev)
    above = ((e0 > thr[:, None]) & valid).float()
    num = torch.nn.functional.conv1d(above[:, None, :], ones, padding=c)[:, 0]
    den = torch.nn.functional.conv1d(valid.float()[:, None, :], ones, padding=c)[:, 0]
    voiced = (num >= den * VOXCELEB["proportion_threshold"]) & valid
    # compaction and re-pad
    picked = norm[voiced]                          # (synchronises: the number of rows is data)
    rows = torch.arange(B, device=dev)[:, None].expand(B, F)[voiced]
    place = (voiced.cumsum(1) - 1)[voiced]
    out = torch.zeros_like(feats)
    out[rows, place] = picked
    return norm, voiced, out


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frameops_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("frameops_time: no gfx950 device")
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

    rng = np.random.default_rng(2025)
    for name, B, seconds in (("short", a.streams, a.seconds), ("long", min(a.long_streams, a.streams), a.long_seconds)):
        T = int(round(seconds * rate))
        starts = rng.integers(0, max(1, n_y - T), B) if T < n_y else np.zeros(B, np.int64)
        x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], starts, T, rate, mode=mp3g.MODE_FAST,
                                                                out_format=mp3g.OUT_F32_MONO, n_threads=16)
        for n_ceps in (30, 40):
            mf = mp3g.MFCC(rate, n_mels=n_ceps, n_ceps=n_ceps, device=0)
            F = mf.frames(T)
            flen = np.clip((lengths - mf.N) // mf.hop + 1, 0, F)
            d_flen = torch.from_numpy(flen.astype(np.int32)).to(dev)
            feats = mf.execute(x).clone()
            work, norm, sel = torch.empty_like(feats), torch.empty_like(feats), torch.empty_like(feats)
            scratch = torch.empty_like(feats)
            voiced, counts = mp3g.vad_energy(feats, d_flen, **VOXCELEB)
            kw = dict(stream=st.cuda_stream)

            def cmvn_leg():  # (in place: every step starts from the same features)
                work.copy_(feats)
                return mp3g.cmvn(work, d_flen, **kw)

            def front_end():
                mp3g.vad_energy(feats, d_flen, out=(voiced, counts), **VOXCELEB, **kw)
                mp3g.sliding_cmn(feats, d_flen, W, 100, True, False, out=norm, **kw)
                return mp3g.select_frames(norm, voiced, d_flen, out=sel, **kw)

            legs = {"mfcc_execute": lambda: mf.execute(x, scratch, **kw),
                    "sliding_cmn": lambda: mp3g.sliding_cmn(feats, d_flen, W, 100, True, False, out=norm, **kw),
                    "sliding_cmn_var": lambda: mp3g.sliding_cmn(feats, d_flen, W, 100, True, True, out=scratch, **kw),
                    "vad_energy": lambda: mp3g.vad_energy(feats, d_flen, out=(voiced, counts), **VOXCELEB, **kw),
                    "select_frames": lambda: mp3g.select_frames(norm, voiced, d_flen, out=sel, **kw),
                    "front_end": front_end, "cmvn": cmvn_leg, "copy_only": lambda: work.copy_(feats),
                    "torch_front_end": lambda: torch_front_end(torch, feats, d_flen)}
            # the torch formulation against the host references, before anything is timed: its float64 sums run
            # in another order (an error near 1e-12, far below a float32 ulp), so a word may land on the other
            # side of one float32 rounding -- 2 ulp at the largest |x| allowed -- and a frame whose energy
            # lies within such a distance of the threshold may flip (counted, at most 1 in 10,000)
            ks = list(range(0, B, max(1, B // 4)))
            h_feats = feats.cpu().numpy()
            want_norm = mp3g.sliding_cmn_host(h_feats[ks], flen[ks], W, 100, True, False)
            want_v, want_c = mp3g.vad_energy_host(h_feats[ks], flen[ks], **VOXCELEB)
            t_norm, t_voiced, t_out = torch_front_end(torch, feats, d_flen)
            tol = 2.0 ** -22 * float(np.abs(h_feats[ks]).max())
            torch_norm_err = float(np.abs(t_norm.cpu().numpy()[ks].astype(np.float64) - want_norm).max())
            flips = int((t_voiced.cpu().numpy()[ks] != (want_v != 0)).sum())
            ok_torch = torch_norm_err <= tol and flips <= max(1, want_v.size // 10000)
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
            # the numbers are only worth keeping if the outputs are the host references'
            out_sel, out_m = front_end()
            torch.cuda.synchronize(dev)
            want_sel, want_m = mp3g.select_frames_host(want_norm, want_v, flen[ks])
            ok = (np.array_equal(norm.cpu().numpy()[ks].view(np.uint32), want_norm.view(np.uint32))
                  and np.array_equal(voiced.cpu().numpy()[ks], want_v) and np.array_equal(counts.cpu().numpy()[ks], want_c)
                  and np.array_equal(out_sel.cpu().numpy()[ks].view(np.uint32), want_sel.view(np.uint32))
                  and np.array_equal(out_m.cpu().numpy()[ks], want_m))
            got_var = mp3g.sliding_cmn(feats, d_flen, W, 100, True, True, out=scratch, **kw).cpu().numpy()[ks]
            ok = ok and np.array_equal(got_var.view(np.uint32),
                                       mp3g.sliding_cmn_host(h_feats[ks], flen[ks], W, 100, True, True).view(np.uint32))
            three = ms["sliding_cmn"] + ms["vad_energy"] + ms["select_frames"]
            emit({"tool": "tools/frameops_time.py", "batch": name, "label": a.label,
                  "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {rate} Hz, mono",
                  "config": {"n_mels": n_ceps, "n_ceps": n_ceps, "cmn_window": W, "center": True, "vad": VOXCELEB},
                  "window_samples": T, "frames": F, "valid_frames_median": int(np.median(flen)),
                  "voiced_frames_median": int(np.median(counts.cpu().numpy())),
                  "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
                  "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
                  "three_calls_sum_ms": round(three, 4),
                  "front_end_over_mfcc_execute": round(ms["front_end"] / ms["mfcc_execute"], 3),
                  "torch_front_end_over_front_end": round(ms["torch_front_end"] / ms["front_end"], 2),
                  "cmvn_less_copy_ms": round(ms["cmvn"] - ms["copy_only"], 4),
                  "sliding_cmn_bytes_in_and_out": int(2 * feats.numel() * 4),
                  "torch_norm_max_abs_error": torch_norm_err, "torch_norm_tolerance": tol,
                  "torch_vad_flips": flips, "torch_matches_host_reference": bool(ok_torch),
                  "outputs_match_host_reference": bool(ok), "device": torch.cuda.get_device_name(dev)})
            mf.close()
            del feats, work, norm, sel, scratch, voiced, counts
            torch.cuda.empty_cache()
            if not (ok and ok_torch):
                raise SystemExit("frameops_time: an output differs from the host reference")
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
