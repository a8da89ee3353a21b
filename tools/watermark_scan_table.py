#!/usr/bin/env python3
"""What finding the native watermark at every offset costs (openvoice_amd/watermark.py "the scan",
csrc/watermark_scan.hip).

For B = 1 and B = 32 device waveforms of 10 s at 22.05 kHz (a modulated two-tone plus noise; waveform 0 carries the
message in repeating windows and has 1237 samples cut from its front):

* ``find``: ``NativeWatermark.find(waves, "@MyShell")`` -- the gather, ``ov_wm_scan_f32``, ``ov_wm_scan_pick``, the copy
  of the hit lists to the host and the chains;
* ``scan_kernel``: the ``ov_wm_scan_f32`` launch alone on the gathered buffer, and from it the executed matrix FLOP/s,
  ``2 * 500 * 32 * S`` useful FLOP over the time, against the 157.3 TF/s fp32 MFMA peak (the kernel issues 8/7 of that:
  neighbouring waves compute their shared tile twice);
* ``brute_force``: the only means there was before -- ``ov_wm_detect_windows_f32`` with one 16 000-sample window per
  offset, in launches of 65 535 records.  Its record tables are built and uploaded BEFORE the clock starts (the host
  loop that would make 6.5 million tuples at B = 32 is left out, in the baseline's favour), and every launch writes
  into the same output rows.

Also counted, not timed: the blind hits (``pmin >= 0.98 level``) and the exact-word hits among all offsets of the
unmarked waveforms.

Host wall time around a device synchronise, median of ``--reps`` after two warm-up rounds, the cases alternating inside
one loop; every repetition is reported.

    python tools/watermark_scan_table.py [--reps 7] [--out profiles/watermark_scan_table.json]
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

from openvoice_amd import _lib, watermark as wm  # noqa: E402

DEV = "cuda:0"
SR = 22050
KEY = 0x1234ABCD5678
MESSAGE = "@MyShell"
PEAK_TFLOPS = 157.3


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def waves_of(B):
    gen = torch.Generator().manual_seed(3)
    n = 10 * SR
    t = torch.arange(n, dtype=torch.float64) / SR
    out = []
    for b in range(B):
        phase = 2 * np.pi * torch.cumsum(140.0 + 5.0 * b + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / SR
        y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
        out.append((y + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float().to(DEV))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    model = wm.NativeWatermark(KEY).to(DEV)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "seconds_per_item": 10, "sampling_rate": SR,
              "peak_fp32_mfma_tflops": PEAK_TFLOPS,
              "clock": "host wall time around a device synchronise, after 2 warm-up rounds, the cases alternating"}
    for B in (1, 32):
        waves = waves_of(B)
        unmarked = [w.clone() for w in waves]
        model.mark_many([waves[0]], MESSAGE, message_repeat=True)
        waves[0] = waves[0][1237:].clone()
        src = torch.cat(waves)
        recs, picks, so, oo = [], [], 0, 0
        for w in waves:
            recs.append((so, w.numel(), oo))
            picks.append((oo, w.numel() - wm.WINDOW + 1))
            so, oo = so + w.numel(), oo + w.numel() - wm.WINDOW + 1
        S = oo
        # the brute-force tables: one window per offset, uploaded before the clock
        chunks = []
        for so_, n_, _ in recs:
            offs = torch.arange(n_ - wm.WINDOW + 1, dtype=torch.int64) + so_
            chunks.append(torch.stack([offs, torch.zeros_like(offs), torch.full_like(offs, wm.WINDOW), torch.zeros_like(offs)], 1))
        table = torch.cat(chunks).to(DEV)
        q = torch.empty(wm.MAX_RECORDS, wm.BITS, device=DEV)
        level = torch.empty(wm.MAX_RECORDS, device=DEV)

        def brute():
            for i in range(0, S, wm.MAX_RECORDS):
                part = table[i:i + wm.MAX_RECORDS]
                _lib.call("ov_wm_detect_windows_f32", src, src.numel(), part, part.shape[0], KEY, model.strength, model.floor,
                          q, level)

        cases = {"find": lambda: model.find(waves, MESSAGE),
                 "scan_kernel": lambda: wm.scan(src, recs, KEY, model.strength, model.floor, out_elems=S),
                 "brute_force": brute}
        times = {k: [] for k in cases}
        for rep in range(args.reps + 2):
            for k, fn in cases.items():
                ms, _ = wall_ms(fn)
                if rep >= 2:
                    times[k].append(ms)
        found = model.find(waves, MESSAGE)
        assert found[0]["marked"] and found[0]["offset"] == wm.STRIDE - 1237 and not any(f["marked"] for f in found[1:])
        entry = {"offsets": S, "brute_force_launches": (S + wm.MAX_RECORDS - 1) // wm.MAX_RECORDS,
                 "brute_force_samples_read": S * wm.WINDOW}
        for k, v in times.items():
            entry[k] = {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v), "all_ms": v}
        flop = 2.0 * 500 * 32 * S
        entry["scan_kernel"]["useful_tflops"] = flop / (entry["scan_kernel"]["median_ms"] * 1e-3) / 1e12
        entry["scan_kernel"]["share_of_peak"] = entry["scan_kernel"]["useful_tflops"] / PEAK_TFLOPS
        entry["scan_kernel"]["note"] = ("the time includes the allocation and fill of the three output arrays (torch.zeros / "
                                        "torch.full) and the upload of the record table")
        entry["speedup_find_over_brute_force"] = entry["brute_force"]["median_ms"] / entry["find"]["median_ms"]
        # unmarked audio: hits among all offsets
        blind = model.find(unmarked, None)
        known = model.find(unmarked, MESSAGE)
        entry["unmarked"] = {"offsets": sum(w.numel() - wm.WINDOW + 1 for w in unmarked),
                             "blind_hits_at_margin_0.98": sum(f["hits"] for f in blind),
                             "exact_word_hits": sum(f["hits"] for f in known),
                             "called_marked": sum(f["marked"] for f in blind) + sum(f["marked"] for f in known)}
        result[f"B{B}"] = entry
        print(json.dumps({f"B{B}": {k: entry[k] if not isinstance(entry[k], dict) or "all_ms" not in entry[k] else
                                    {kk: vv for kk, vv in entry[k].items() if kk != "all_ms"} for k in entry}}))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
