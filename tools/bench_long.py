#!/usr/bin/env python3
"""Long recordings and streaming (openvoice_amd/longform.py): ms per minute of audio and peak device allocation of the
one-pass conversion against the windowed one at several file lengths, the windowed output's distance from the one-pass
output, and the real-time factor and latency of the streaming converter at two window sizes.
Measurement tool: python tools/bench_long.py [--minutes 5 12 20 45] [--window-frames 4096] [--windows-per-launch 4]
                                             [--stream-windows 1024 4096] [--stream-minutes 5] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR, HOP, NFFT = 22050, 256, 1024


def speechlike(n, dev, seed=0):
    """A few drifting partials under a syllable-rate envelope plus a little noise, generated on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64, device=dev) / SR
    phase = 2 * math.pi * (140.0 * t - 40.0 / (2 * math.pi * 0.3) * torch.cos(2 * math.pi * 0.3 * t))
    y = 0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5) + 0.05 * torch.sin(7.3 * phase)
    y = y * (0.6 + 0.4 * torch.sin(2 * math.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=g, dtype=torch.float64, device=dev)).float()


def timed(fn, dev):
    """(result, wall ms, peak bytes allocated during fn)."""
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return out, (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[5, 12, 20, 45])
    ap.add_argument("--window-frames", type=int, default=None)
    ap.add_argument("--windows-per-launch", type=int, default=None)
    ap.add_argument("--stream-windows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--stream-minutes", type=float, default=5)
    ap.add_argument("--stream-block", type=int, default=SR // 10, help="samples per push (default 100 ms)")
    ap.add_argument("--no-one-pass", action="store_true")
    ap.add_argument("--sweep-minutes", type=float, default=20, help="file length of the (window, batch) sweep; 0 = none")
    ap.add_argument("--sweep-windows", type=int, nargs="+", default=[2048, 4096, 8192])
    ap.add_argument("--sweep-wpl", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from openvoice_amd import longform
    from openvoice_amd.mel_processing import spectrogram_torch
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.params import synthetic_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    dev = torch.device("cuda:0")
    Tw = args.window_frames or longform.DEFAULT_WINDOW_FRAMES
    wpl = args.windows_per_launch or longform.DEFAULT_WINDOWS_PER_LAUNCH
    model = SynthesizerTrn(0, 513, n_speakers=0, zero_g=True, **CFG)
    model.load_state_dict(synthetic_state_dict(CFG, 513, seed=1234), strict=True)
    model = model.to(dev).eval()
    eng = model.engine()
    gen = torch.Generator().manual_seed(1)
    g_src, g_tgt = (0.3 * torch.randn(1, 256, 1, generator=gen)).to(dev), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(dev)
    conv = longform.WindowedConverter(model, NFFT, HOP, window_frames=Tw, windows_per_launch=wpl)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    emit({"what": "setup", "window_frames": Tw, "windows_per_launch": wpl, "context_frames": conv.context,
          "core_frames": conv.core, "grid_frames": conv.grid, "frames_computed_per_output_frame": round(Tw / conv.core, 4),
          "one_pass_limit_frames": longform.one_pass_limit_frames(CFG), "device": torch.cuda.get_device_name(dev)})
    # warm-up: kernels loaded, occupancy caches filled, the windowed workspace shape allocated once
    w = speechlike(SR * 120, dev, 9)
    conv.convert(w, g_src, g_tgt, tau=0.3)
    torch.cuda.synchronize(dev)
    del w
    for minutes in args.minutes:
        n = int(minutes * 60 * SR)
        wave = speechlike(n, dev, int(minutes))
        T = longform.frames_of(n, NFFT, HOP)
        noise = torch.randn(1, 192, T, device=dev)
        rec = {"what": "file", "minutes": minutes, "frames": T}
        eng._ws.clear()
        torch.cuda.empty_cache()
        conv.convert(wave, g_src, g_tgt, tau=0.3, noise=noise)          # this length's last-batch shape seen once
        win, ms, peak = timed(lambda: conv.convert(wave, g_src, g_tgt, tau=0.3, noise=noise), dev)
        rec.update(windowed_ms=round(ms, 1), windowed_ms_per_audio_min=round(ms / minutes, 2),
                   windowed_peak_gib=round(peak / 2**30, 3))
        if not args.no_one_pass and T < longform.one_pass_limit_frames(CFG):
            eng._ws.clear()
            torch.cuda.empty_cache()

            def one_pass():
                spec = spectrogram_torch(wave[None], NFFT, SR, HOP, NFFT, center=False)
                return model.voice_conversion(spec, torch.tensor([T], device=dev), g_src, g_tgt, tau=0.3, noise=noise)[0]
            one_pass()                                                       # workspace of this length allocated
            o, ms1, peak1 = timed(one_pass, dev)
            rec.update(one_pass_ms=round(ms1, 1), one_pass_ms_per_audio_min=round(ms1 / minutes, 2),
                       one_pass_peak_gib=round(peak1 / 2**30, 3), windowing_overhead=round(ms / ms1 - 1.0, 4),
                       max_abs_windowed_vs_one_pass=float((o[0, 0] - win).abs().max().item()))
            del o
            eng._ws.clear()
            torch.cuda.empty_cache()
        elif not args.no_one_pass:
            rec["one_pass"] = "refused: at or beyond one_pass_limit_frames (OV_E_BADARG)"
        emit(rec)
        del wave, noise, win
    # (window frames, windows per launch) sweep at one file length: what the defaults were picked from
    if args.sweep_minutes > 0:
        n = int(args.sweep_minutes * 60 * SR)
        wave = speechlike(n, dev, 5)
        noise = torch.randn(1, 192, longform.frames_of(n, NFFT, HOP), device=dev)
        for sw in args.sweep_windows:
            for k in args.sweep_wpl:
                c = longform.WindowedConverter(model, NFFT, HOP, window_frames=sw, windows_per_launch=k)
                eng._ws.clear()
                torch.cuda.empty_cache()
                c.convert(wave, g_src, g_tgt, tau=0.3, noise=noise)
                _, ms, peak = timed(lambda: c.convert(wave, g_src, g_tgt, tau=0.3, noise=noise), dev)
                emit({"what": "sweep", "minutes": args.sweep_minutes, "window_frames": sw, "windows_per_launch": k,
                      "ms": round(ms, 1), "ms_per_audio_min": round(ms / args.sweep_minutes, 2),
                      "peak_gib": round(peak / 2**30, 3)})
        del wave, noise
        eng._ws.clear()
        torch.cuda.empty_cache()
    # streaming: blocks of --stream-block samples pushed as they would arrive, as fast as the converter takes them
    n = int(args.stream_minutes * 60 * SR)
    wave = speechlike(n, dev, 77)
    for sw in args.stream_windows:
        st = longform.WindowedConverter(model, NFFT, HOP, window_frames=sw, windows_per_launch=1).stream(g_src, g_tgt, 0.3)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pushed, first_at, emitted, worst_push_ms = 0, None, 0, 0.0
        while pushed < n:
            blk = wave[pushed:pushed + args.stream_block]
            tp = time.perf_counter()
            o = st.push(blk)
            torch.cuda.synchronize(dev)
            worst_push_ms = max(worst_push_ms, (time.perf_counter() - tp) * 1e3)
            pushed += blk.numel()
            emitted += o.numel()
            if o.numel() and first_at is None:
                first_at = pushed
        emitted += st.close().numel()
        torch.cuda.synchronize(dev)
        wall = time.perf_counter() - t0
        emit({"what": "stream", "window_frames": sw, "minutes": args.stream_minutes, "block_samples": args.stream_block,
              "real_time_factor": round(n / SR / wall, 1), "latency_samples": st.latency_samples,
              "latency_s": round(st.latency_samples / SR, 3), "first_output_after_samples": first_at,
              "worst_push_ms": round(worst_push_ms, 2), "output_samples": emitted})
    if args.out:
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    return lines


if __name__ == "__main__":
    main()
