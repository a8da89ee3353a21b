#!/usr/bin/env python3
"""What enrolling many voices costs: a loop of per-voice ``extract_se_from_audio`` calls (the path every enrolment took
before ``extract_se_many`` existed; its code is unchanged) against ONE ``extract_se_many`` call over the same pieces.

For V in {1, 8, 32} synthetic 30 s recordings, each cut into three pieces whose lengths differ by 1 to 2000 samples (what
``get_se`` produces after silence removal: no two pieces of a recording are equally long, so the per-voice path runs
three spectrogram + ``ref_enc`` launch sequences per voice).  The pieces are on the device before the clock starts; a
repetition is host wall time around work that ends in a device synchronise, after warm-up of both paths, the two paths
alternating inside one loop.  Reported: the median and all repetitions per path, their ratio, the launches' batch sizes,
and the largest difference between the two results.

    python tools/enrol_timing.py [--reps 9] [--out profiles/enrol_timing.json]

Prints one JSON line (and writes it to ``--out``).  Synthetic converter weights: timings do not depend on the values.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from openvoice_amd import api  # noqa: E402
from openvoice_amd.params import synthetic_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
SR = 22050


def recording_pieces(v):
    """Three pieces of recording ``v``: 30 s of a modulated two-tone voice, cut at bounds moved by 1..2000 samples."""
    rng = np.random.default_rng(1000 + v)
    n = 30 * SR
    t = np.arange(n) / SR
    y = (0.35 * np.sin(2 * np.pi * (140 + 3 * v) * t) + 0.15 * np.sin(2 * np.pi * 470 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * t))
    y = (y + 0.01 * rng.standard_normal(n)).astype(np.float32)
    d1, d2 = int(rng.integers(1, 301)), int(rng.integers(301, 601))
    bounds = [0, n // 3 - d1, 2 * n // 3 + d2, n]                # lengths n/3 - d1, n/3 + d1 + d2, n/3 - d2
    pieces = [y[bounds[i]:bounds[i + 1]] for i in range(3)]
    lens = sorted(len(p) for p in pieces)
    assert 1 <= lens[1] - lens[0] and 1 <= lens[2] - lens[1] and lens[2] - lens[0] <= 2000, lens
    return pieces


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    work = tempfile.mkdtemp(prefix="enrol_timing_")
    hps = default_converter_hparams("v2")
    with open(os.path.join(work, "config.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, seed=1234)}, os.path.join(work, "checkpoint.pth"))
    tcc = api.ToneColorConverter(os.path.join(work, "config.json"), device=DEV, enable_watermark=False)
    tcc.load_ckpt(os.path.join(work, "checkpoint.pth"))

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "seconds_per_recording": 30,
              "pieces_per_recording": 3, "clock": "host wall time around a device synchronise, after 2 warm-up rounds"}
    for V in (1, 8, 32):
        voices = [[torch.from_numpy(p).to(DEV) for p in recording_pieces(v)] for v in range(V)]
        lens = [[int(p.numel()) for p in voice] for voice in voices]

        def per_voice():
            out, batches = [], []
            for voice in voices:
                out.append(tcc.extract_se_from_audio(voice))
                batches += tcc.last_extract_se_batches
            return torch.cat(out), batches

        def one_call():
            return tcc.extract_se_many(voices), list(tcc.last_extract_se_batches)

        for _ in range(2):
            per_voice(); one_call()
        loop, many = [], []
        for _ in range(args.reps):
            ms, (se_loop, loop_batches) = wall_ms(per_voice)
            loop.append(ms)
            ms, (se_many, many_batches) = wall_ms(one_call)
            many.append(ms)
        res = {"piece_samples_min": min(min(x) for x in lens), "piece_samples_max": max(max(x) for x in lens),
               "per_voice_loop": {"median_ms": float(np.median(loop)), "all_ms": loop,
                                  "launch_sequences": len(loop_batches)},
               "extract_se_many": {"median_ms": float(np.median(many)), "all_ms": many,
                                   "launch_sequences": len(many_batches), "batches": many_batches},
               "max_abs_difference": float((se_loop - se_many).abs().max().item())}
        res["loop_over_many"] = res["per_voice_loop"]["median_ms"] / res["extract_se_many"]["median_ms"]
        result[f"V{V}"] = res
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
