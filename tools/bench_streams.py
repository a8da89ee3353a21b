#!/usr/bin/env python3
"""Many live streams on one GPU (openvoice_amd/longform.py): N solo ConversionStreams stepped in turn against one
StreamPool, on synthetic speech-like audio arriving in 100 ms pushes.  For each (window, N, mode): wall ms per 100 ms
tick (pushes + conversions + a device sync), the aggregate real-time factor, and the peak device allocation; per
(window, mode) the largest N that stays real time.
Measurement tool: python tools/bench_streams.py [--streams 1 8 32 128] [--windows 255 512 1024]
                                                [--max-windows-per-launch 32] [--min-ticks 20] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR, HOP, NFFT = 22050, 256, 1024
TICK = SR // 10                    # samples per 100 ms push


def speechlike(n, seed=0):
    """A few drifting partials under a syllable-rate envelope plus a little noise (host tensor: live input)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / SR
    phase = 2 * math.pi * (140.0 * t - 40.0 / (2 * math.pi * 0.3) * torch.cos(2 * math.pi * 0.3 * t))
    y = 0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5) + 0.05 * torch.sin(7.3 * phase)
    y = y * (0.6 + 0.4 * torch.sin(2 * math.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=g, dtype=torch.float64)).float()


def run(model, eng, Tw, N, mode, M, min_ticks, dev, wave, ses):
    from openvoice_amd import longform
    conv = longform.WindowedConverter(model, NFFT, HOP, window_frames=Tw, windows_per_launch=1)
    period = math.ceil(conv.core * HOP / TICK)            # ticks between two windows of one stream
    warm, ticks = period + 2, max(min_ticks, period)
    eng._ws.clear()
    eng.resident_workspaces = 1
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    if mode == "pool":
        pool = conv.stream_pool(tau=0.3, max_windows_per_launch=M)
        sizes = pool.ladder
    else:
        streams = [conv.stream(*ses[i % len(ses)], tau=0.3) for i in range(N)]
        sizes = [1]
    for B in sizes:                                        # every launch shape built before the clock runs
        model.voice_conversion(torch.zeros(B, 513, Tw, device=dev), torch.full((B,), Tw, device=dev),
                               torch.cat([ses[0][0]] * B), torch.cat([ses[0][1]] * B), tau=0.3)
    latency = conv.stream(None, None).latency_samples
    gen = torch.Generator().manual_seed(N * 7 + Tw)
    # random phases: stream i starts up to one window period short of its first output, so windows spread over ticks
    pos = [latency - 1 - int(torch.randint(0, conv.core * HOP, (1,), generator=gen)) for _ in range(N)]
    offs = [int(torch.randint(0, wave.numel() // 4, (1,), generator=gen)) for _ in range(N)]
    if mode == "pool":
        hs = [pool.open(*ses[i % len(ses)]) for i in range(N)]
        for i, h in enumerate(hs):
            pool.push(h, wave[offs[i]:offs[i] + pos[i]])
    else:
        for i, st in enumerate(streams):
            st.push(wave[offs[i]:offs[i] + pos[i]])
    out_samples = 0
    t0 = None
    for tick in range(warm + ticks):
        if tick == warm:
            torch.cuda.synchronize(dev)
            t0, out_samples = time.perf_counter(), 0
        if mode == "pool":
            for i, h in enumerate(hs):
                pool.push(h, wave[offs[i] + pos[i]:offs[i] + pos[i] + TICK])
                pos[i] += TICK
            out_samples += sum(o.numel() for o in pool.step().values())
        else:
            for i, st in enumerate(streams):
                out_samples += st.push(wave[offs[i] + pos[i]:offs[i] + pos[i] + TICK]).numel()
                pos[i] += TICK
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3 / ticks
    return {"what": "streams", "mode": mode, "window_frames": Tw, "streams": N, "ticks": ticks,
            "max_windows_per_launch": M if mode == "pool" else 1, "windows": round(out_samples / (conv.core * HOP), 1),
            "ms_per_tick": round(ms, 2), "real_time_factor": round(N * 100.0 / ms, 2), "real_time": ms <= 100.0,
            "peak_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 3),
            "latency_s": round(latency / SR, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--windows", type=int, nargs="+", default=[255, 512, 1024])
    ap.add_argument("--max-windows-per-launch", type=int, default=None)
    ap.add_argument("--min-ticks", type=int, default=20)
    ap.add_argument("--modes", nargs="+", default=["solo", "pool"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from openvoice_amd import longform
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.params import synthetic_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    dev = torch.device("cuda:0")
    M = args.max_windows_per_launch or longform.DEFAULT_POOL_WINDOWS_PER_LAUNCH
    model = SynthesizerTrn(0, 513, n_speakers=0, zero_g=True, **CFG)
    model.load_state_dict(synthetic_state_dict(CFG, 513, seed=1234), strict=True)
    model = model.to(dev).eval()
    eng = model.engine()
    gen = torch.Generator().manual_seed(1)
    ses = [((0.3 * torch.randn(1, 256, 1, generator=gen)).to(dev), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(dev))
           for _ in range(8)]
    wave = speechlike(SR * 120, 9)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    emit({"what": "setup", "tick_samples": TICK, "max_windows_per_launch": M, "ladder": longform.launch_ladder(M),
          "device": torch.cuda.get_device_name(dev)})
    for Tw in args.windows:
        for mode in args.modes:
            best = 0
            for N in args.streams:
                rec = run(model, eng, Tw, N, mode, M, args.min_ticks, dev, wave, ses)
                emit(rec)
                if rec["real_time"]:
                    best = N
            emit({"what": "summary", "mode": mode, "window_frames": Tw, "largest_real_time_streams_measured": best})
    eng.resident_workspaces = 1
    if args.out:
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    return lines


if __name__ == "__main__":
    main()
