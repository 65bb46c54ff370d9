#!/usr/bin/env python3
"""The reverberation and noise mixing (mp3g.augment) on the c3 workload, in one
process.

The batches are tools/mfcc_time.py's: bench.py's c3 streams (independently
seeded 44.1 kHz streams x 1,024 frames, synth.encode_batch seeds 1..), one
window of --seconds at 16 kHz from every one of --streams streams (1,024 x 2 s)
and one --long-seconds window from the first --long-streams (128 x 30 s), both
from decode_windows_resampled_tensor (fast mode, mono).  For responses of 4,000
and 16,000 taps (a bank of 16, one drawn per row) and one wrapping noise slot
per row, the legs alternate inside every round on the same device tensors; a
leg's time is the median of its windows (HIP events on the launch stream; one
untimed launch of the leg before each window).  The library's legs go through
the C call on arguments prepared once, so no upload falls into a window:

  power, forward, convolve, mix, scale   the five launches, one at a time
                     (mp3g_augment_debug_launch, on buffers a whole call filled)
  augment            mp3g_augment_rows: the five launches
  resample           the Resampler.rows launch that makes a batch of this shape
                     from 44.1 kHz rows: the stage before, as the yardstick
  torch              the same computation in torch: torch.fft.rfft / irfft at
                     the next power of two above T + L - 1 (the responses'
                     spectra made once, outside the timed call), gathers for
                     the responses and the noise, float64 reductions; checked
                     against the host reference before it is timed
Beside them decode_resample_wall_ms, the wall time of the
decode_windows_resampled_tensor call that made the batch (host scan included).

Writes one JSON line per batch and tap count to profiles/reverb_c3.json (and
prints them).

  python tools/reverb_time.py [--steps 10] [--warmup 3] [--rounds 5] [--streams 1024] [--long-streams 128]
                              [--frames 1024] [--out FILE] [--label TEXT]

Needs the GPU: without one it fails (there is no CPU path to fall back to).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "go-mp3_amd"))


def torch_spectra(torch, h, table, n_fft):
    """The bank's spectra at n_fft points, of h and of its early part: made once, as the library's object makes its own."""
    t = torch.arange(h.shape[1], device=h.device)[None, :]
    he = torch.where((t >= table["es"][:, None]) & (t < table["ee"][:, None]), h, torch.zeros_like(h))
    return torch.fft.rfft(h, n=n_fft), torch.fft.rfft(he, n=n_fft)


def torch_augment(torch, x, n, H, He, n_fft, table, ri, noise, pn, slot):
    """(out [B, T], stats [B, 4]) of mono rows of n [B] samples (zero past them) in torch."""
    B, T = x.shape
    dev = x.device
    peak, es, ee = (table[k][ri] for k in ("peak", "es", "ee"))
    X = torch.fft.rfft(x, n=n_fft)
    full = torch.fft.irfft(X * H[ri], n=n_fft)
    y = full.gather(1, peak[:, None] + torch.arange(T, device=dev)[None, :])
    early = torch.fft.irfft(X * He[ri], n=n_fft)
    tt = torch.arange(n_fft, device=dev)[None, :]
    inside = (tt >= es[:, None]) & (tt < (n + ee - 1)[:, None])
    valid = torch.arange(T, device=dev)[None, :] < n[:, None]
    power_before = x.double().square().sum(1) / n
    signal_power = (early.double().square() * inside).sum(1) / (n + (ee - es) - 1).double()
    idx, ratio, offset, length = slot
    g = torch.sqrt(ratio * signal_power / pn[idx]).float()
    at = (offset[:, None] + torch.arange(T, device=dev)[None, :]) % length[:, None]
    v = torch.where(valid, torch.addcmul(y, g[:, None], noise[idx[:, None], at]), torch.zeros_like(y))
    power_after = v.double().square().sum(1) / n
    scale = torch.sqrt(power_before / power_after)
    out = (v.double() * scale[:, None]).float()
    return out, torch.stack([power_before, signal_power, power_after, scale], dim=1)


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reverb_c3.json"))
    ap.add_argument("--label", default="", help="copied into every line (which build was timed)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mp3g
    from mp3g import synth
    if not torch.cuda.is_available() or mp3g.device_count() < 1:
        raise SystemExit("reverb_time: no gfx950 device")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    stream = C.c_void_p(st.cuda_stream) if st.cuda_stream else None
    rate = 16000
    datas, _, _, _ = synth.encode_batch(range(1, 1 + a.streams), a.frames, n_threads=16)
    rs = mp3g.Resampler(44100, rate, device=0)
    n_y = rs.out_len(1152 * a.frames)
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as fh:
            for x in lines:
                fh.write(json.dumps(x) + "\n")

    rng = np.random.default_rng(2026)
    M, Tn = 8, 160000
    h_noise = (0.05 * rng.standard_normal((M, Tn))).astype(np.float32)
    nl = np.array([Tn, Tn // 2, Tn, 100001, Tn, 7777, Tn, Tn], np.uint32)
    d_noise = torch.from_numpy(h_noise).to(dev)
    d_nl = torch.from_numpy(nl.astype(np.int32)).to(dev)
    d_pn = mp3g.row_power(d_noise, d_nl)
    for name, B, seconds in (("short", a.streams, a.seconds), ("long", min(a.long_streams, a.streams), a.long_seconds)):
        T = int(round(seconds * rate))
        starts = rng.integers(0, max(1, n_y - T), B) if T < n_y else np.zeros(B, np.int64)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            x, lengths, _, _ = mp3g.decode_windows_resampled_tensor(datas[:B], starts, T, rate, mode=mp3g.MODE_FAST,
                                                                    out_format=mp3g.OUT_F32_MONO, n_threads=16)
            torch.cuda.synchronize(dev)
            walls.append((time.perf_counter() - t0) * 1e3)
        lengths = np.minimum(lengths, T)
        # the resample launch of this shape: 44.1 kHz rows of the window's source span, one output row each
        s0, s1 = rs.src_window(0, T)
        d_src = torch.randn((B, s1 - s0), dtype=torch.float32, device=dev)
        rrows = np.zeros(B, mp3g.RESAMPLE_ROW_DTYPE)
        for k in range(B):
            rrows[k] = (0, s0, k, k, s1 - s0, T)
        d_rs_out = torch.empty((B, T), dtype=torch.float32, device=dev)
        for taps in (4000, 16000):
            R = 16
            h = (rng.standard_normal((R, taps)) * np.exp(-np.arange(taps) / (taps / 7.0))).astype(np.float32)
            h[np.arange(R), rng.integers(20, 120, R)] = 6.0
            rv = mp3g.Reverb(h, None, rate, device=0)
            info = rv.info()
            ri = rng.integers(0, R, B).astype(np.int32)
            add = dict(index=rng.integers(0, M, (B, 1)), snr_db=rng.uniform(0, 15, (B, 1)),
                       offset=rng.integers(0, 7777, (B, 1)), wrap=np.ones((B, 1), np.int64))
            slots = mp3g._augment_slots(add, B)
            d_ri = torch.from_numpy(ri).to(dev)
            d_slots = torch.from_numpy(slots.view(np.uint8).reshape(-1).copy()).to(dev)
            d_len = torch.from_numpy(lengths.astype(np.int32)).to(dev)
            out = torch.empty_like(x)
            stats = torch.zeros((B, 4), dtype=torch.float64, device=dev)
            need = int(mp3g.lib().mp3g_reverb_scratch_bytes(rv._h, B, 1, T))
            scratch = torch.empty(need // 8 + 1, dtype=torch.float64, device=dev)
            args = mp3g._AugmentArgs()
            args.x, args.out, args.lengths, args.rir_index = x.data_ptr(), out.data_ptr(), d_len.data_ptr(), d_ri.data_ptr()
            args.noise, args.noise_lengths, args.noise_power = d_noise.data_ptr(), d_nl.data_ptr(), d_pn.data_ptr()
            args.slots, args.stats = d_slots.data_ptr(), stats.data_ptr()
            args.n_rows, args.n_planes, args.T, args.n_noise, args.Tn, args.A = B, 1, T, M, Tn, 1
            args.flags = mp3g.AUGMENT_NORMALIZE
            call = (rv._h, 0, C.byref(args), ri.ctypes.data, nl.ctypes.data, slots.ctypes.data, scratch.data_ptr(),
                    need, stream)

            def whole():
                mp3g._check(mp3g.lib().mp3g_augment_rows(*call))

            def launch(which):
                return lambda: mp3g._check(mp3g.lib().mp3g_augment_debug_launch(*call, which))

            # the torch formulation's inputs, on the device once
            table = {k: torch.from_numpy(info[k]).to(dev) for k in ("peak", "es", "ee")}
            t_h, t_ri, t_n = torch.from_numpy(h).to(dev), d_ri.long(), d_len.long()
            t_slot = (torch.from_numpy(slots["noise_index"][:, 0].astype(np.int64)).to(dev),
                      torch.from_numpy(slots["snr_ratio"][:, 0]).to(dev),
                      torch.from_numpy(slots["offset"][:, 0].astype(np.int64)).to(dev), None)
            t_slot = t_slot[:3] + (d_nl.long()[t_slot[0]],)

            n_fft = 1 << (T + taps - 2).bit_length()
            t_H, t_He = torch_spectra(torch, t_h, table, n_fft)

            def torch_leg():
                return torch_augment(torch, x, t_n, t_H, t_He, n_fft, table, t_ri, d_noise, d_pn, t_slot)

            legs = {"power": launch(0), "forward": launch(1), "convolve": launch(2), "mix": launch(3),
                    "scale": launch(4), "augment": whole,
                    "resample": lambda: rs.rows(d_src, d_rs_out, rrows, stream=st.cuda_stream), "torch": torch_leg}
            # the outputs against the host reference bit for bit, and torch against it, before anything is timed.
            # Both are float32 transforms that err by a few 2^-24 of a row's largest sample (the CPU tests hold the
            # host to four times an independent float32 formulation's error, at least 2^-23 max|y|): torch may
            # differ from the host by 2^-20 of the row's largest sample, the records by 2^-20 relatively
            whole()
            torch.cuda.synchronize(dev)
            ks = list(range(0, B, max(1, B // 3)))[:3]
            h_x = x.cpu().numpy()
            want, want_stats = mp3g.augment_host(h_x[ks], lengths[ks], reverb=rv, rir_index=ri[ks], noise=h_noise,
                                                 noise_lengths=nl, additive={k: v[ks] for k, v in add.items()})
            ok = (np.array_equal(out.cpu().numpy()[ks].view(np.uint32), want.view(np.uint32))
                  and np.array_equal(stats.cpu().numpy()[ks].view(np.uint64), want_stats.view(np.uint64)))
            ok_torch, torch_err, torch_tol = True, 0.0, 0.0
            t_out, t_stats = torch_leg()
            t_out, t_stats = t_out.cpu().numpy(), t_stats.cpu().numpy()
            for i, k in enumerate(ks):
                tol = 2.0 ** -20 * float(np.abs(want[i]).max())
                err = float(np.abs(t_out[k].astype(np.float64) - want[i]).max())
                torch_err, torch_tol = max(torch_err, err), max(torch_tol, tol)
                ok_torch = ok_torch and err <= tol and np.allclose(t_stats[k], want_stats[i], rtol=2.0 ** -20, atol=0.0)
            del t_out
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
            P = int(info["P"][0])
            lay_blocks_in, lay_blocks_out = (T + 1023) // 1024 + 1, (T + taps - 2) // 1024 + 1
            emit({"tool": "tools/reverb_time.py", "batch": name, "label": a.label,
                  "workload": f"c3: {B} streams x {a.frames} frames, one {seconds:g} s window each at {rate} Hz, mono",
                  "config": {"taps": taps, "partitions": P, "responses": R, "noise_slots": 1, "wrap": True,
                             "normalize": True},
                  "window_samples": T, "valid_samples_median": int(np.median(lengths)), "steps": a.steps, "warmup": a.warmup,
                  "rounds": a.rounds, "ms": ms, "ms_windows": {k: [round(v, 4) for v in w] for k, w in win.items()},
                  "launches_sum_ms": round(sum(ms[k] for k in ("power", "forward", "convolve", "mix", "scale")), 4),
                  "decode_resample_wall_ms": round(statistics.median(walls), 2),
                  "augment_over_resample": round(ms["augment"] / ms["resample"], 2),
                  "torch_over_augment": round(ms["torch"] / ms["augment"], 2),
                  "scratch_bytes": need, "spectra_bytes_written": B * lay_blocks_in * 2048 * 8,
                  "convolve_bytes_read": B * lay_blocks_out * min(P, lay_blocks_in) * 2 * 2048 * 8,
                  "torch_max_abs_error": torch_err, "torch_tolerance": torch_tol,
                  "torch_matches_host_reference": bool(ok_torch),
                  "outputs_match_host_reference": bool(ok), "device": torch.cuda.get_device_name(dev)})
            rv.close()
            del out, stats, scratch
            torch.cuda.empty_cache()
            if not (ok and ok_torch):
                raise SystemExit("reverb_time: an output differs from the host reference")
        del x, d_src, d_rs_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
