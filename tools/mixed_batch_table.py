#!/usr/bin/env python3
"""What per-item synthesis controls buy a batch of cloning requests that mixes speeds and base speakers (DESIGN
section 21).  Method of DESIGN section 6: warm-up, then the median of 7 wall times around a device synchronise.

The workload is the README's clone figure, 32 requests of 3 sentences (the texts of ``tools/clone_timing.py``), with K
distinct ``(speed, speaker)`` keys dealt round-robin over the requests, K in {1, 4, 8, 16}, on the fp32 and on the bf16
generator.  ``VoiceCloner.speak_ids_many`` keyed (one ``infer`` launch sequence per key: the default) against
``mixed=True`` (all 96 sentences in shared launches, the per-item kernels), in the same process, the two alternating
call by call so that a drift of the machine lands on both.  ``noise_w`` is explicit, so every sentence has the same
durations in every call and keyed and mixed synthesise the same frames; the other draws are made on the device.
``synthesize_many`` alone (TTS + join, no conversion) is timed the same way: the conversion half is the same work on
both sides.  The keyed K = 1 row is measured ``--repeats`` times over; the spread of its medians is the noise floor
against which a difference counts.

    python tools/mixed_batch_table.py [--out profiles/mixed_batch_table.json] [--repeats 4]

Prints one JSON line (and writes it to ``--out``).  Synthetic weights: timings do not depend on the values.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from openvoice_amd import api, clone  # noqa: E402

DEV = "cuda:0"
RUNS, WARMUP = 7, 2
KEYS = (1, 4, 8, 16)
SPEEDS = (1.0, 0.8, 1.3, 1.1, 0.9, 1.2, 0.85, 1.15)


def key_of(k):
    """Key k of 16 distinct ``(speed, speaker id)`` pairs: 8 speeds x the 10 speakers of the synthetic table."""
    return SPEEDS[k % 8], k % 10


def alternating_ms(fns, runs=RUNS, warmup=WARMUP):
    """``fns``: name -> callable.  One round calls each in turn; ``warmup`` rounds, then ``runs`` timed ones."""
    times = {name: [] for name in fns}
    for _ in range(warmup + runs):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": round(float(np.median(t[warmup:])), 3), "all_ms": [round(x, 3) for x in t[warmup:]]}
            for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=4)
    args = ap.parse_args()
    import clone_timing
    n = args.requests
    tts, conv = clone_timing.models(tempfile.mkdtemp(prefix="mixed_batch_"))
    vc = clone.VoiceCloner(tts, conv)
    gen = torch.Generator().manual_seed(0)
    se = lambda: 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV)
    api.BaseSpeakerTTS.text_to_sequence = staticmethod(lambda text, symbols, cleaners: [1 + (ord(c) % 67) for c in text])
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ids = [tts.text_to_ids(clone_timing.text_of(100 * n + i), "English") for i in range(n)]
    finally:
        api.BaseSpeakerTTS.text_to_sequence = None
    ses = [(se(), se()) for _ in ids]
    noise_w = [[torch.randn(2, len(s), generator=gen).to(DEV) for s in req] for req in ids]
    result = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "requests": n,
              "sentences_per_request": 3, "ids_per_sentence_mean": float(np.mean([len(s) for req in ids for s in req])),
              "keys": [key_of(k) for k in range(max(KEYS))], "rows": []}

    def requests_of(K):
        return [(i, key_of(r % K)[1], s, t, key_of(r % K)[0]) for r, (i, (s, t)) in enumerate(zip(ids, ses))]

    with torch.no_grad():
        for generator in ("fp32", "bf16"):
            for K in KEYS:
                requests = requests_of(K)
                reqs = vc._parse(requests, noise_w, None, None, None)
                speak = lambda mixed: vc.speak_ids_many(requests, noise_w=noise_w, generator=generator, mixed=mixed)
                synth = lambda mixed: vc.synthesize_many(reqs, noise_w, generator=generator, mixed=mixed)
                row = {"generator": generator, "keys": K}
                for what, fn in (("speak_ids_many", speak), ("synthesize_many", synth)):
                    t = alternating_ms({"keyed": lambda: fn(False), "mixed": lambda: fn(True)})
                    t["keyed_over_mixed"] = round(t["keyed"]["median_ms"] / t["mixed"]["median_ms"], 3)
                    row[what] = t
                fn(False)
                row["keyed_infer_launches"] = vc.last_launches["infer"]
                fn(True)
                row["mixed_infer_launches"] = vc.last_launches["infer"]
                row["frames"] = int(sum(w.numel() for w in synth(True))) // int(tts.hps.data.hop_length)
                result["rows"].append(row)
        # the noise floor: the keyed K = 1 row again and again
        spread = {}
        for generator in ("fp32", "bf16"):
            requests = requests_of(1)
            medians = [alternating_ms({"keyed": lambda: vc.speak_ids_many(requests, noise_w=noise_w, generator=generator)})
                       ["keyed"]["median_ms"] for _ in range(args.repeats)]
            spread[generator] = {"keyed_k1_medians_ms": medians, "spread_ms": round(max(medians) - min(medians), 3),
                                 "spread_rel": round((max(medians) - min(medians)) / min(medians), 4)}
        result["keyed_k1_spread"] = spread
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
