#!/usr/bin/env python3
"""What length grouping buys the bf16 generator on ragged batches.  Method of DESIGN section 6:
warm-up, then the median of 7 wall times around a device synchronise.

* (a) ``group_cost`` in item-frames: the time of a ``B = 1, T = 1`` ``GeneratorBf16.decode`` (what one more pass over
  the launch sequence costs whatever its size) divided by the per-item-frame time of a ``B = 64, T = 861`` decode;
* (b) the V1 TTS batch of BASELINE.json configs[3] (16 x 100 symbols, the inputs of ``bench.py``'s ``config_tts_v1``):
  ``infer`` on fp32 with ``skip_padding``, on bf16 padded, and on bf16 grouped at ``max_groups`` = 1, 2, 3, 4, 6, 8 (with
  the measured ``group_cost``, and once more with free groups: what a cut really costs), each plan's groups and
  item-frames next to its time;
* (c) the README's clone figure, 32 requests of 3 sentences (the texts of ``tools/clone_timing.py``), ``speak_ids_many``
  on fp32 against bf16.

    python tools/bf16_groups_table.py [--out profiles/bf16_groups_table.json] [--skip-clone]

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

from openvoice_amd import api, bf16, clone  # noqa: E402
from openvoice_amd.models import SynthesizerTrn  # noqa: E402
from openvoice_amd.params import synthetic_state_dict, synthetic_tts_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG  # noqa: E402

DEV = "cuda:0"
RUNS, WARMUP = 7, 2
GROUPS = (1, 2, 3, 4, 6, 8)


def wall_ms(fn, runs=RUNS, warmup=WARMUP):
    times = []
    for _ in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(times[warmup:])), 4), "all_ms": [round(t, 3) for t in times[warmup:]]}


def measure_group_cost(gen):
    g = torch.Generator().manual_seed(0)
    small_z, big_z = torch.randn(1, 192, 1, generator=g).to(DEV), torch.randn(64, 192, 861, generator=g).to(DEV)
    cond = (0.3 * torch.randn(1, 256, 1, generator=g)).to(DEV)
    small = wall_ms(lambda: gen.decode(small_z, cond))
    big = wall_ms(lambda: gen.decode(big_z, cond))
    per_item_frame_ms = big["median_ms"] / (64 * 861)
    return {"decode_b1_t1": small, "decode_b64_t861": big, "per_item_frame_us": round(per_item_frame_ms * 1e3, 5),
            "group_cost_item_frames": round(small["median_ms"] / per_item_frame_ms, 1)}


def measure_tts(group_cost):
    model = SynthesizerTrn(68, 513, n_speakers=10, **CFG)
    model.load_state_dict(synthetic_tts_state_dict(CFG), strict=True)
    model = model.to(DEV).eval()
    gen = torch.Generator().manual_seed(0)
    B, Tx = 16, 100
    tok = torch.randint(0, 68, (B, Tx), generator=gen).to(DEV)
    lengths = torch.full((B,), Tx, dtype=torch.long, device=DEV)
    sid = (torch.arange(B) % 10).to(DEV)
    noise_w = torch.randn(B, 2, Tx, generator=gen).to(DEV)
    noise_z = torch.randn(B, 192, 16 * Tx, generator=gen).to(DEV)
    call = lambda **kw: model.infer(tok, lengths, sid=sid, noise_scale=0.667, noise_scale_w=0.6, length_scale=1.0,
                                    noise_w=noise_w, noise_z=noise_z, **kw)
    y_mask = call(skip_padding=True)[2]
    frames = y_mask[:, 0].sum(1).long().tolist()
    g16 = model.engine().core.bf16_generator()
    res = {"batch": B, "symbols": Tx, "frames": frames, "padded_frames": max(frames), "margin": g16.margin,
           "fp32_skip_padding": wall_ms(lambda: call(skip_padding=True)),
           "fp32_padded": wall_ms(lambda: call()),
           "bf16_padded": wall_ms(lambda: call(generator="bf16"))}
    # with the measured group cost (what the planner really does), then with free groups (what a cut really costs)
    for tag, cost in (("bf16_grouped", group_cost), ("bf16_grouped_free_groups", 0)):
        g16.group_cost = cost
        for G in GROUPS:
            g16.max_groups = G
            t = wall_ms(lambda: call(generator="bf16", skip_padding=True))
            t["groups"] = [(len(idx), L) for idx, L in g16.last_plan]
            t["item_frames"] = sum(len(idx) * L for idx, L in g16.last_plan)
            res[f"{tag}_max_groups_{G}"] = t
    g16.max_groups, g16.group_cost = bf16.DEFAULT_MAX_GROUPS, bf16.DEFAULT_GROUP_COST
    return res


def measure_clone(n=32):
    import clone_timing
    work = tempfile.mkdtemp(prefix="bf16_groups_")
    tts, conv = clone_timing.models(work)
    vc = clone.VoiceCloner(tts, conv)
    gen = torch.Generator().manual_seed(0)
    se = lambda: 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV)
    api.BaseSpeakerTTS.text_to_sequence = staticmethod(lambda text, symbols, cleaners: [1 + (ord(c) % 67) for c in text])
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ids = [tts.text_to_ids(clone_timing.text_of(100 * n + i), "English") for i in range(n)]
    finally:
        api.BaseSpeakerTTS.text_to_sequence = None
    requests = [(i, "default", se(), se()) for i in ids]
    res = {"requests": n, "sentences_per_request": 3,
           "speak_ids_many_fp32": wall_ms(lambda: vc.speak_ids_many(requests)),
           "speak_ids_many_bf16": wall_ms(lambda: vc.speak_ids_many(requests, generator="bf16"))}
    res["fp32_over_bf16"] = round(res["speak_ids_many_fp32"]["median_ms"] / res["speak_ids_many_bf16"]["median_ms"], 3)
    res["max_groups"], res["group_cost"] = bf16.DEFAULT_MAX_GROUPS, bf16.DEFAULT_GROUP_COST
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-clone", action="store_true")
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP}
    with torch.no_grad():
        gen = bf16.GeneratorBf16(synthetic_state_dict(CFG, 513, seed=1234), CFG, DEV)
        result["group_cost"] = measure_group_cost(gen)
        del gen
        torch.cuda.empty_cache()
        result["tts_v1_batch"] = measure_tts(result["group_cost"]["group_cost_item_frames"])
        if not args.skip_clone:
            result["clone_32x3"] = measure_clone()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
