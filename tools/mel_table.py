#!/usr/bin/env python3
"""What the device STFT and mel features cost (openvoice_amd/mel_processing.py, csrc/stft.hip).

For B = 1 and B = 32 waveforms of 10 s at 22.05 kHz:

* ``spectrogram_torch`` at the released shape 1024 / 256 / 1024 (``ov_frame_hops_f32`` + the framing conv: two launches);
* ``stft_magnitude`` at the same shape (``ov_stft_mag_f32``: one launch of the general kernel);
* ``stft_magnitude`` at 1024 / 320 / 1024 and at 2048 / 512 / 2048;
* ``spec_to_mel_torch`` with 80 mels on the 1024 / 256 spectrogram (``ov_mel_log_f32``);
* ``mel_spectrogram_torch`` with 80 mels at 1024 / 256 / 1024.  There is no fused kernel: the function IS the two-launch
  composition, so its time is set against the sum of its two parts, and ``spectrogram_bytes`` is what the linear
  spectrogram's round trip through memory moves (written once, read once).

Host wall time around a device synchronise, median of ``--reps`` after two warm-up rounds, the cases alternating inside
one loop; every repetition is reported.  Times of this size (tens of microseconds at B = 1) are mostly launch and
synchronise overhead: they say what a caller waits, not what the kernel does.

    python tools/mel_table.py [--reps 7] [--out profiles/mel_table.json]
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

from openvoice_amd import mel_processing as mp  # noqa: E402

DEV = "cuda:0"
SR = 22050


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "seconds_per_item": 10, "sampling_rate": SR,
              "fused_mel_kernel": False,
              "clock": "host wall time around a device synchronise, after 2 warm-up rounds, the cases alternating"}
    gen = torch.Generator().manual_seed(3)
    for B in (1, 32):
        t = torch.arange(10 * SR, dtype=torch.float32) / SR
        y = (0.6 * torch.sin(2 * torch.pi * (200 + 30 * torch.arange(B)[:, None]) * t)
             + 0.05 * torch.randn(B, 10 * SR, generator=gen)).to(DEV)
        spec = mp.spectrogram_torch(y, 1024, SR, 256, 1024)
        cases = {
            "spectrogram_torch_1024_256_1024": lambda: mp.spectrogram_torch(y, 1024, SR, 256, 1024),
            "stft_magnitude_1024_256_1024": lambda: mp.stft_magnitude(y, 1024, 256, 1024),
            "stft_magnitude_1024_320_1024": lambda: mp.stft_magnitude(y, 1024, 320, 1024),
            "stft_magnitude_2048_512_2048": lambda: mp.stft_magnitude(y, 2048, 512, 2048),
            "spec_to_mel_torch_80": lambda: mp.spec_to_mel_torch(spec, 1024, 80, SR, 0, None),
            "mel_spectrogram_torch_80_two_launches": lambda: mp.mel_spectrogram_torch(y, 1024, 80, SR, 256, 1024, 0, None),
        }
        for _ in range(2):
            for fn in cases.values():
                wall_ms(fn)
        times = {name: [] for name in cases}
        for _ in range(args.reps):
            for name, fn in cases.items():
                times[name].append(wall_ms(fn)[0])
        row = {name: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "all_ms": v}
               for name, v in times.items()}
        row["frames"] = int(spec.shape[2])
        row["spectrogram_bytes"] = int(2 * spec.shape[0] * spec.shape[1] * spec.stride(1) * 4)
        row["sum_of_parts_ms"] = row["stft_magnitude_1024_256_1024"]["median_ms"] + row["spec_to_mel_torch_80"]["median_ms"]
        result[f"B{B}"] = row
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
