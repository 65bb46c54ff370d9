#!/usr/bin/env python3
"""The Kaldi MFCC features (MFCC.execute) and the per-row normalisation
(mp3g.cmvn) on the c3 workload, in one process.

The batch is bench.py's c3 (independently seeded 44.1 kHz streams x 1,024
frames, synth.encode_batch seeds 1..): every one of --streams streams gives one
window of --seconds at 16 kHz, and the first --long-streams give one
--long-seconds window (the streams are 26.7 s long: its tail is the dense
batch's zero padding).  Both come from decode_windows_resampled_tensor (fast
mode, mono).  For (n_mels, n_ceps) = (23, 13) and (40, 40) the legs alternate
inside every round on the same device tensor; a leg's time is the median of its
windows (HIP events on the launch stream; one untimed launch of the leg before
each window):

  mfcc_no_energy     MFCC.execute, use_energy off
  mfcc_raw_energy    MFCC.execute, use_energy on, raw_energy on
  mfcc_win_energy    MFCC.execute, use_energy on, raw_energy off
  fbank_execute      FBank.execute at the same (N, hop, n_mels): the yardstick
  fbank_then_matmul  the two launches the fused kernel replaces: FBank.execute,
                     then torch.matmul with D^T and the lifter multiply
  cmvn               mp3g.cmvn (mean and variance) on the MFCC tensor
  torch_cmvn         a masked torch mean / variance normalisation of the same

Writes one JSON line per batch and configuration to profiles/mfcc_c3.json (and
prints them).

  python tools/mfcc_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mfcc_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    ap.add_argument("--no-remove-dc", action="store_true", help="without the per-frame mean (what the mean's chain costs)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("mfcc_time: no gfx950 device")
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
        for n_mels, n_ceps in ((23, 13), (40, 40)):
            kw = dict(n_mels=n_mels, n_ceps=n_ceps, remove_dc=not a.no_remove_dc, device=0)
            objs = {"mfcc_no_energy": mp3g.MFCC(rate, use_energy=False, **kw),
                    "mfcc_raw_energy": mp3g.MFCC(rate, **kw),
                    "mfcc_win_energy": mp3g.MFCC(rate, raw_energy=False, **kw)}
            mf = objs["mfcc_no_energy"]
            fb = mp3g.FBank(rate, n_mels=n_mels, remove_dc=not a.no_remove_dc, device=0)
            F = mf.frames(T)
            assert F == fb.frames(T)
            flen = np.clip((lengths - mf.N) // mf.hop + 1, 0, F)
            d_flen = torch.from_numpy(flen.astype(np.int32)).to(dev)
            dt = torch.from_numpy(mf.dct.T.copy()).to(dev)          # [n_mels, n_ceps]
            lift = torch.from_numpy(mf.lifter.copy()).to(dev)
            out = torch.empty((B, F, n_ceps), dtype=torch.float32, device=dev)
            out_fb = torch.empty((B, F, n_mels), dtype=torch.float32, device=dev)
            out_mm = torch.empty((B, F, n_ceps), dtype=torch.float32, device=dev)
            feats = objs["mfcc_raw_energy"].execute(x).clone()
            work = torch.empty_like(feats)
            mask = (torch.arange(F, device=dev)[None, :] < d_flen[:, None]).unsqueeze(-1)
            count = d_flen.clamp(min=1).to(torch.float32)[:, None, None]

            def two_launches():
                fb.execute(x, out_fb, stream=st.cuda_stream)
                torch.matmul(out_fb, dt, out=out_mm)
                return out_mm.mul_(lift)

            def cmvn_leg():  # (in place: every step starts from the same features)
                work.copy_(feats)
                return mp3g.cmvn(work, d_flen, norm_vars=True, stream=st.cuda_stream)

            def torch_cmvn():
                work.copy_(feats)
                m = (work * mask).sum(dim=1, keepdim=True) / count
                v = ((work * work) * mask).sum(dim=1, keepdim=True) / count - m * m
                return torch.where(mask, (work - m) * torch.rsqrt(v.clamp(min=1e-20)), work)

            # (the long kernels side by side, the short ones after them)
            legs = {"fbank_execute": lambda: fb.execute(x, out_fb, stream=st.cuda_stream),
                    "fbank_then_matmul": two_launches}
            legs.update({k: (lambda o=o: o.execute(x, out, stream=st.cuda_stream)) for k, o in objs.items()})
            legs.update({"cmvn": cmvn_leg, "torch_cmvn": torch_cmvn, "copy_only": lambda: work.copy_(feats)})
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
            # the numbers are only worth keeping if the features are the host reference's
            rows = x.cpu().numpy()
            ks = range(0, B, max(1, B // 4))
            ok = True
            for o in objs.values():  # (four rows of one object, the first row of the others: the host is slow)
                got = o.execute(x, out, stream=st.cuda_stream).cpu().numpy()
                ok = ok and all(np.array_equal(got[k].view(np.uint32), o.host(rows[k], F).view(np.uint32))
                                for k in (ks if o is mf else ks[:1]))
            diff = float((two_launches() - mf.execute(x, out, stream=st.cuda_stream)).abs().max())
            got = cmvn_leg().cpu().numpy()
            sub = list(ks)
            ok_cmvn = np.array_equal(got[sub].view(np.uint32),
                                     mp3g.cmvn_host(feats.cpu().numpy()[sub], flen[sub], True).view(np.uint32))
            emit({"tool": "tools/mfcc_time.py", "batch": name, "label": a.label,
                  "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {rate} Hz, mono",
                  "config": {"N": mf.N, "hop": mf.hop, "P": mf.P, "K": mf.K, "n_mels": n_mels, "n_ceps": n_ceps,
                             "remove_dc": mf.remove_dc, "tile_frames": mf.tile_frames, "dct_in_lds": mf.dct_in_lds},
                  "window_samples": T, "frames": F, "valid_frames_median": int(np.median(flen)),
                  "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ms": ms,
                  "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
                  "mfcc_no_energy_over_fbank": round(ms["mfcc_no_energy"] / ms["fbank_execute"], 3),
                  "mfcc_no_energy_over_two_launches": round(ms["mfcc_no_energy"] / ms["fbank_then_matmul"], 3),
                  "raw_energy_cost_ms": round(ms["mfcc_raw_energy"] - ms["mfcc_no_energy"], 4),
                  "win_energy_cost_ms": round(ms["mfcc_win_energy"] - ms["mfcc_no_energy"], 4),
                  "cmvn_less_copy_ms": round(ms["cmvn"] - ms["copy_only"], 4),
                  "torch_cmvn_less_copy_ms": round(ms["torch_cmvn"] - ms["copy_only"], 4),
                  "max_abs_difference_from_two_launches": diff,
                  "features_match_host_reference": bool(ok), "cmvn_matches_host_reference": bool(ok_cmvn),
                  "device": torch.cuda.get_device_name(dev)})
            for o in objs.values():
                o.close()
            fb.close()
            del out, out_fb, out_mm, feats, work, mask
            torch.cuda.empty_cache()
            if not (ok and ok_cmvn):
                raise SystemExit("mfcc_time: a feature row differs from the host reference")
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
