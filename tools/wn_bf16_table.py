#!/usr/bin/env python3
"""What the bf16 WaveNet layer (``ov_wn_layer_bf16``) costs next to the fp32 layers.  Method of
DESIGN section 6: warm-up 2, then the median of 7 wall times around a device synchronise, one process, fp32 first.

* (a) per layer, in us: the 16-layer posterior stack through ``ConverterEngine._wavenet`` with the fp32 policy (Winograd
  where ``wn_wino_policy`` says so, the row-split pair for one or two utterances) against ``wavenet="bf16"``, at batch
  1, 4, 16, 32, 64 x 861 frames; the stack's wall time divided by its 16 launches (launch overhead included: what a
  conversion pays);
* (b) the whole conversion at batch 32 x 861 for generator {fp32, bf16} x wavenet {fp32, bf16}, and the share of each
  fp32-WaveNet conversion spent in its 48 WaveNet layers (48 x the batch-32 per-layer time of (a), same run);
* (c) the live pool tick at 128 streams, chunk 15, ``generator="bf16"``, both wavenet values (``tools/bench_live.py``'s
  ``run_live``: 100 ms pushes, one ``step()`` per tick, wall ms per tick in the steady state; the pool follows the
  engine's ``use_bf16_wavenet`` switch);
* (d) the V1 TTS batch of BASELINE.json configs[3] (16 x 100 symbols, ``skip_padding``) on the bf16 generator, both
  wavenet values.

    python tools/wn_bf16_table.py [--out profiles/wn_bf16_table.json]

Prints one JSON line (and writes it to ``--out``).  Synthetic weights: timings do not depend on the values.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from openvoice_amd import _lib  # noqa: E402
from openvoice_amd.models import SynthesizerTrn  # noqa: E402
from openvoice_amd.params import synthetic_state_dict, synthetic_tts_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG  # noqa: E402

DEV = "cuda:0"
RUNS, WARMUP = 7, 2
T = 861


def wall_ms(fn, runs=RUNS, warmup=WARMUP):
    times = []
    for _ in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times[warmup:])), 4)


def layer_table(eng):
    rows = []
    gen = torch.Generator().manual_seed(0)
    for B in (1, 4, 16, 32, 64):
        ws = eng._workspace(B, T)
        _lib.call("ov_sequence_mask_f32", torch.full((B,), T, dtype=torch.int64, device=DEV), ws["mask"], B, T, ws["Tp"])
        ws["h"][:, :, :T] = torch.randn(B, eng.hidden, T, generator=gen).to(DEV)
        cond = eng._wn_cond(eng.q_wn, (0.3 * torch.randn(1, eng.gin, generator=gen)).to(DEV))
        row = {"batch": B, "frames": T, "tile_bf16": _lib.call("ov_wn_layer_bf16_tile", B, T, 0)}
        for choice in ("fp32", "bf16"):             # fp32 first
            def stack():
                with eng.wavenet_scope(choice):
                    eng._wavenet(eng.q_wn, ws, B, T, cond, ws["mask"])
            row[f"us_per_layer_{choice}"] = round(1e3 * wall_ms(stack) / eng.q_wn.n_layers, 2)
        rows.append(row)
    return rows


def conversion_table(model, B=32):
    gen = torch.Generator().manual_seed(1)
    spec = (2.0 * torch.rand(B, 513, T, generator=gen)).to(DEV)
    lengths = torch.full((B,), T, dtype=torch.int64, device=DEV)
    g_src, g_tgt = ((0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV) for _ in range(2))
    noise = torch.randn(B, 192, T, generator=gen).to(DEV)
    out = {"batch": B, "frames": T}
    for generator in ("fp32", "bf16"):
        for wavenet in ("fp32", "bf16"):
            out[f"ms_generator_{generator}_wavenet_{wavenet}"] = wall_ms(
                lambda: model.voice_conversion(spec, lengths, g_src, g_tgt, tau=0.3, noise=noise, generator=generator,
                                               wavenet=wavenet))
    return out


def live_table(N=128, chunk=15, M=32, min_ticks=20):
    """A model of its own with ``zero_g`` as tools/bench_live.py builds it; fp32 first."""
    from tools.bench_live import run_live
    from tools.bench_streams import SR, speechlike
    dev = torch.device(DEV)
    model = SynthesizerTrn(0, 513, n_speakers=0, zero_g=True, **CFG)
    model.load_state_dict(synthetic_state_dict(CFG, 513, seed=1234), strict=True)
    model = model.to(dev).eval()
    gen = torch.Generator().manual_seed(1)
    ses = [((0.3 * torch.randn(1, 256, 1, generator=gen)).to(dev), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(dev))
           for _ in range(8)]
    wave = speechlike(SR * 120, 9)
    out = {"streams": N, "chunk_frames": chunk, "generator": "bf16", "max_streams_per_launch": M}
    for wavenet in ("fp32", "bf16"):
        model.engine().use_bf16_wavenet(wavenet == "bf16")
        try:
            out[f"ms_per_tick_wavenet_{wavenet}"] = run_live(model, chunk, N, M, min_ticks, dev, wave, ses,
                                                             generator="bf16")["ms_per_tick"]
        finally:
            model.engine().use_bf16_wavenet(False)
    return out


def tts_table(B=16, Tx=100):
    model = SynthesizerTrn(68, 513, n_speakers=10, **CFG)
    model.load_state_dict(synthetic_tts_state_dict(CFG), strict=True)
    model = model.to(DEV).eval()
    gen = torch.Generator().manual_seed(0)
    tok = torch.randint(0, 68, (B, Tx), generator=gen).to(DEV)
    lengths = torch.full((B,), Tx, dtype=torch.long, device=DEV)
    sid = (torch.arange(B) % 10).to(DEV)
    noise_w, noise_z = torch.randn(B, 2, Tx, generator=gen).to(DEV), torch.randn(B, 192, 16 * Tx, generator=gen).to(DEV)
    out = {"batch": B, "tokens": Tx, "generator": "bf16"}
    for wavenet in ("fp32", "bf16"):
        out[f"ms_wavenet_{wavenet}"] = wall_ms(
            lambda: model.infer(tok, lengths, sid=sid, noise_scale=0.667, noise_scale_w=0.6, length_scale=1.0,
                                noise_w=noise_w, noise_z=noise_z, skip_padding=True, generator="bf16", wavenet=wavenet))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    model = SynthesizerTrn(0, 513, n_speakers=0, **CFG)
    model.load_state_dict(synthetic_state_dict(CFG, 513, seed=1234), strict=False)
    model = model.to(DEV).eval()
    eng = model.engine()
    eng.resident_workspaces = 1
    rec = {"method": f"warm-up {WARMUP}, median of {RUNS} wall times around a device synchronise, fp32 first",
           "device": torch.cuda.get_device_name(0), "per_layer": layer_table(eng), "conversion": conversion_table(model)}
    us32 = next(r for r in rec["per_layer"] if r["batch"] == 32)["us_per_layer_fp32"]
    layers = eng.q_wn.n_layers + 2 * sum(cp["wn"].n_layers for cp in eng.couplings)
    for generator in ("fp32", "bf16"):
        rec["conversion"][f"wavenet_fp32_share_generator_{generator}"] = round(
            layers * us32 * 1e-3 / rec["conversion"][f"ms_generator_{generator}_wavenet_fp32"], 4)
    rec["conversion"]["wavenet_layers"] = layers
    del model, eng
    torch.cuda.empty_cache()
    rec["live_pool"] = live_table()
    rec["tts_v1"] = tts_table()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
