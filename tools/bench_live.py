#!/usr/bin/env python3
"""Low-latency live streams on one GPU (openvoice_amd/live.py) against the windowed StreamPool, same method as
tools/bench_streams.py: N streams of synthetic speech-like audio arriving in 100 ms pushes, one step() per tick.  For
each (chunk, N): wall ms per 100 ms tick (pushes + conversions + a device sync), the aggregate real-time factor, the
latency bound and the peak device allocation; the windowed pool at Tw = 255 frames is measured in the same run as the
comparison row.
With ``--sr-in`` / ``--sr-out`` every live stream takes its pushes (100 ms of audio each) at that rate and returns its output
at that rate (openvoice_amd/rates.py: one resampler launch per direction and step); the model-rate live rows are then
measured in the same run as the baseline.
With ``--generator fp32 bf16`` every (chunk, N) row is measured once per generator, one after the other in the same run
(``LivePool(generator=...)``: the kernels of the generator units; the records carry ``generator``).
With ``--lookahead A [A ...]`` every (chunk, N, generator) row is measured first plain (``lookahead_frames`` None) and
then once per A in the same run (``LivePool(lookahead_frames=A)``, default cross-fade); the records carry
``lookahead_frames``, the latency bound of that A and ``x_plain`` = the row's ms per tick over its plain row's.
Measurement tool: python tools/bench_live.py [--streams 1 8 32 128] [--chunks 15 30 60] [--max-streams-per-launch 32]
                                             [--min-ticks 20] [--sr-in HZ] [--sr-out HZ] [--generator fp32 bf16]
                                             [--lookahead A [A ...]] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_streams import HOP, NFFT, SR, TICK, run as run_windowed, speechlike  # noqa: E402


def run_live(model, chunk, N, M, min_ticks, dev, wave, ses, sr_in=None, sr_out=None, generator="fp32", lookahead=None):
    from openvoice_amd import live
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    pool = live.LivePool(model, tau=0.3, chunk_frames=chunk, max_streams_per_launch=M, n_fft=NFFT, hop=HOP,
                         generator=generator, lookahead_frames=lookahead)
    latency = live.live_latency_samples(model.model_cfg, chunk, NFFT, HOP)      # warm up past the plain bound in any case
    r_in, r_out = sr_in or SR, sr_out or SR
    push_n = r_in // 10                           # input samples per 100 ms push
    gen = torch.Generator().manual_seed(N * 7 + chunk)
    offs = [int(torch.randint(0, wave.numel() // 4, (1,), generator=gen)) for _ in range(N)]
    # random phases within one chunk period, so chunks spread over ticks as they would for independent users
    pos = [int(torch.randint(0, chunk * HOP, (1,), generator=gen)) * r_in // SR for _ in range(N)]
    hs = [pool.open(*ses[i % len(ses)], sr_in=sr_in, sr_out=sr_out) for i in range(N)]
    lat_s = float(pool.latency_of(hs[0])[0])
    for i, h in enumerate(hs):
        pool.push(h, wave[offs[i]:offs[i] + pos[i]])
    warm = math.ceil(latency / TICK) + 3          # past the first output of every stream: the steady state
    ticks = max(min_ticks, math.ceil(chunk * HOP / TICK))
    out_samples, t0 = 0, None
    for tick in range(warm + ticks):
        if tick == warm:
            torch.cuda.synchronize(dev)
            t0, out_samples = time.perf_counter(), 0
        for i, h in enumerate(hs):
            pool.push(h, wave[offs[i] + pos[i]:offs[i] + pos[i] + push_n])
            pos[i] += push_n
        out_samples += sum(o.numel() for o in pool.step().values())
    torch.cuda.synchronize(dev)
    ms = (time.perf_counter() - t0) * 1e3 / ticks
    rec = {"what": "live", "mode": "live_pool", "generator": generator, "chunk_frames": chunk, "streams": N, "ticks": ticks,
           "max_streams_per_launch": M, "out_s_per_s": round(out_samples / r_out / (ticks / 10.0), 2),
           "ms_per_tick": round(ms, 2), "real_time_factor": round(N * 100.0 / ms, 2), "real_time": ms <= 100.0,
           "peak_gib": round(torch.cuda.max_memory_allocated(dev) / 2**30, 3), "latency_s": round(lat_s, 3),
           "state_mib_per_stream": round(pool.state_bytes_per_stream() / 2**20, 3)}
    if lookahead is not None:
        rec.update(lookahead_frames=lookahead, crossfade_samples=pool.crossfade)
    if sr_in or sr_out:
        rec.update(sr_in=r_in, sr_out=r_out, resampler_launches=pool._rin.launches + pool._rout.launches)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32, 128])
    ap.add_argument("--chunks", type=int, nargs="+", default=[15, 30, 60])
    ap.add_argument("--max-streams-per-launch", type=int, default=32)
    ap.add_argument("--min-ticks", type=int, default=20)
    ap.add_argument("--no-windowed", action="store_true", help="skip the windowed Tw = 255 comparison rows")
    ap.add_argument("--sr-in", type=int, default=None, help="rate of the pushes (default: the model rate)")
    ap.add_argument("--sr-out", type=int, default=None, help="rate of the output (default: the model rate)")
    ap.add_argument("--generator", nargs="+", choices=["fp32", "bf16"], default=["fp32"],
                    help="the live pools' generator kernels; both: every row once per generator, in the same run")
    ap.add_argument("--lookahead", type=int, nargs="+", default=[],
                    help="lookahead_frames values; each row is measured plain first, then once per value")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.params import synthetic_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    dev = torch.device("cuda:0")
    M = args.max_streams_per_launch
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

    emit({"what": "setup", "tick_samples": TICK, "max_streams_per_launch": M, "device": torch.cuda.get_device_name(dev)})
    rated = args.sr_in is not None or args.sr_out is not None
    wave_in = wave
    if args.sr_in is not None and args.sr_in != SR:
        from openvoice_amd import audio_io
        wave_in = audio_io.resample_on_device(wave.to(dev), SR, args.sr_in).cpu()
    for chunk in args.chunks:
        for N in args.streams:
            for generator in args.generator:
                if rated:                         # the model-rate row of the same run, then the resampled one
                    emit(run_live(model, chunk, N, M, args.min_ticks, dev, wave, ses, generator=generator))
                plain = run_live(model, chunk, N, M, args.min_ticks, dev, wave_in, ses, args.sr_in, args.sr_out, generator)
                emit(plain)
                for A in args.lookahead:
                    rec = run_live(model, chunk, N, M, args.min_ticks, dev, wave_in, ses, args.sr_in, args.sr_out,
                                   generator, lookahead=A)
                    rec["x_plain"] = round(rec["ms_per_tick"] / plain["ms_per_tick"], 2)
                    emit(rec)
    if not args.no_windowed:
        eng._live_ws.clear()                       # the windowed rows' peak memory without the live workspaces
        eng._live_ws_bf16.clear()
        for N in args.streams:
            emit(run_windowed(model, eng, 255, N, "pool", M, args.min_ticks, dev, wave, ses))
        eng.resident_workspaces = 1
    if args.out:
        with open(args.out, "a") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")
    return lines


if __name__ == "__main__":
    main()
