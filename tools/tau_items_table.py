#!/usr/bin/env python3
"""What a per-item ``tau`` buys a service whose callers want different taus, and what it costs a batch that does not
(DESIGN section "One tau per item").  Method of DESIGN section 6: warm-up, then the median of 7 wall times around a
device synchronise; the two sides of a comparison alternate block by block in one process, so that a drift of the
machine lands on both.

* Live pools: 128 live streams (15-frame chunks, 100 ms pushes, ``tools/bench_live.py``'s signal and phases) whose
  callers want K distinct taus, K in {1, 2, 4}.  ``split`` = K ``LivePool``s of 128 / K streams, one tau each, stepped
  back to back every tick -- all a pool with one launch scalar allows; ``mixed`` = one pool of 128 streams opened with
  ``open(tau=)``.  ms per 100 ms tick, a block = 7 ticks (four chunk periods).
* Conversion: ``convert_batch`` of 32 utterances x 861 frames with ``tau=0.3`` against the same call with a list of 32
  values (validated and uploaded per call) and with a float32 device tensor.  The scalar side is measured ``--repeats``
  times over; the spread of its medians is the noise floor against which a difference counts.

    python tools/tau_items_table.py [--out profiles/tau_items_table.json] [--repeats 4] [--streams 128]

Prints one JSON line (and writes it to ``--out``).  Synthetic weights: timings do not depend on the values.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from openvoice_amd import api, live  # noqa: E402
from openvoice_amd.params import synthetic_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG, default_converter_hparams  # noqa: E402
from tools.bench_streams import HOP, NFFT, SR, TICK, speechlike  # noqa: E402

DEV = "cuda:0"
RUNS, WARMUP = 7, 2
BLOCK_TICKS = 7
TAUS = (0.3, 0.1, 0.6, 0.9)
CHUNK, M = 15, 32


def converter(work):
    hps = default_converter_hparams("v2")
    with open(os.path.join(work, "config.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CFG, 513, seed=1234)}, os.path.join(work, "checkpoint.pth"))
    tcc = api.ToneColorConverter(os.path.join(work, "config.json"), device=DEV, enable_watermark=False)
    tcc.load_ckpt(os.path.join(work, "checkpoint.pth"))
    return tcc


def median_ms(times):
    return {"median_ms": round(float(np.median(times)), 3), "all_ms": [round(t, 3) for t in times]}


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
    return {name: median_ms(t[warmup:]) for name, t in times.items()}


class Side:
    """N live streams over one or more pools; ``tick()`` pushes 100 ms into every stream and steps every pool."""

    def __init__(self, model, N, K, mixed, wave, ses, offs, pos):
        taus = [TAUS[i % K] for i in range(N)]
        if mixed:
            self.pools = [live.LivePool(model, tau=TAUS[0], chunk_frames=CHUNK, max_streams_per_launch=M, n_fft=NFFT, hop=HOP)]
            owner = [0] * N
        else:
            self.pools = [live.LivePool(model, tau=TAUS[k], chunk_frames=CHUNK, max_streams_per_launch=M, n_fft=NFFT, hop=HOP)
                          for k in range(K)]
            owner = [i % K for i in range(N)]
        self.wave, self.offs, self.pos = wave, offs, list(pos)
        self.streams = []
        for i in range(N):
            pool = self.pools[owner[i]]
            h = pool.open(*ses[i % len(ses)], tau=taus[i]) if mixed else pool.open(*ses[i % len(ses)])
            pool.push(h, wave[offs[i]:offs[i] + pos[i]])
            self.streams.append((pool, h))

    def tick(self):
        for i, (pool, h) in enumerate(self.streams):
            a = self.offs[i] + self.pos[i]
            pool.push(h, self.wave[a:a + TICK])
            self.pos[i] += TICK
        for pool in self.pools:
            pool.step()

    def block(self):
        for _ in range(BLOCK_TICKS):
            self.tick()


def live_rows(model, N, wave, ses):
    rows = []
    gen = torch.Generator().manual_seed(N * 7 + CHUNK)
    offs = [int(torch.randint(0, wave.numel() // 4, (1,), generator=gen)) for _ in range(N)]
    pos = [int(torch.randint(0, CHUNK * HOP, (1,), generator=gen)) for _ in range(N)]
    warm_ticks = math.ceil(live.LivePool(model, chunk_frames=CHUNK, n_fft=NFFT, hop=HOP).latency_samples / TICK) + 3
    for K in (1, 2, 4):
        sides = {"split": Side(model, N, K, False, wave, ses, offs, pos), "mixed": Side(model, N, K, True, wave, ses, offs, pos)}
        for side in sides.values():                 # past the first output of every stream: the steady state
            for _ in range(warm_ticks):
                side.tick()
        t = alternating_ms({name: side.block for name, side in sides.items()})
        row = {"taus": K, "streams": N, "pools_split": K}
        for name in sides:
            row[name] = {"ms_per_tick": round(t[name]["median_ms"] / BLOCK_TICKS, 3),
                         "all_ms_per_tick": [round(x / BLOCK_TICKS, 3) for x in t[name]["all_ms"]]}
        row["split_over_mixed"] = round(row["split"]["ms_per_tick"] / row["mixed"]["ms_per_tick"], 3)
        row["mixed_launch_vectors"] = len(sides["mixed"].pools[0]._tau_rows)
        rows.append(row)
        del sides
        model.engine()._live_ws.clear()
        torch.cuda.empty_cache()
    return rows


def conversion(tcc, repeats, B=32, T=861):
    gen = torch.Generator().manual_seed(3)
    waves = (0.3 * torch.randn(B, T * HOP, generator=gen)).to(DEV)
    noise = torch.randn(B, 192, T, generator=gen).to(DEV)
    src, tgt = (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)
    values = [TAUS[i % len(TAUS)] for i in range(B)]
    vec = torch.tensor(values, dtype=torch.float32, device=DEV)
    run = lambda tau: tcc.convert_batch(waves, src, tgt, tau=tau, noise=noise)
    t = alternating_ms({"scalar": lambda: run(0.3), "list": lambda: run(values), "device_tensor": lambda: run(vec)})
    medians = [alternating_ms({"scalar": lambda: run(0.3)})["scalar"]["median_ms"] for _ in range(repeats)]
    spread = max(medians) - min(medians)
    rec = {"batch": B, "frames": T, **t, "scalar_repeat_medians_ms": medians, "scalar_spread_ms": round(spread, 3)}
    for name in ("list", "device_tensor"):
        d = t[name]["median_ms"] - t["scalar"]["median_ms"]
        rec[f"{name}_minus_scalar_ms"] = round(d, 3)
        rec[f"{name}_within_spread"] = bool(abs(d) <= spread)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--streams", type=int, default=128)
    args = ap.parse_args()
    tcc = converter(tempfile.mkdtemp(prefix="tau_items_"))
    gen = torch.Generator().manual_seed(1)
    ses = [((0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV))
           for _ in range(8)]
    result = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "warmup": WARMUP, "block_ticks": BLOCK_TICKS,
              "chunk_frames": CHUNK, "max_streams_per_launch": M, "tick_samples": TICK, "taus": list(TAUS)}
    with torch.no_grad():
        result["conversion"] = conversion(tcc, args.repeats)
        result["live_pools"] = live_rows(tcc.model, args.streams, speechlike(SR * 120, 9), ses)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
