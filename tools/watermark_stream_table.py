#!/usr/bin/env python3
"""What the block-wise watermark of streams (openvoice_amd/watermark.py, "streams") costs and how loud it is.

* Signal-to-mark ratio ``10 log10(sum x^2 / sum (y - x)^2)`` over the two carrier windows of a synthetic 10 s
  conversion's output, per hold H: the whole output goes through ``watermark.StreamMarker`` (the stream's own path) once
  per H, and the mark is read back with ``NativeWatermark.decode``.
* ms per tick of a live pool of ``--streams`` streams (chunk 15, 100 ms pushes) without messages and with one per
  stream (``--hold``, ``message_repeat=True`` so that every tick marks).  The two pools alternate inside one loop;
  median and min .. max of ``--reps`` rounds of ``--ticks`` ticks each, host wall time around a device synchronise.
* ``--parent-tree DIR`` (a built checkout of the parent commit): the unmarked pool alone, timed in fresh processes on
  that tree and on this one, alternating (parent, this, parent, this).  It shows what ``message=None`` costs next to the
  parent's own run-to-run spread.

    python tools/watermark_stream_table.py [--parent-tree DIR] [--out profiles/watermark_stream_table.json]

Prints one JSON line (and writes it to ``--out``).  Synthetic converter weights: timings do not depend on the values.
``--plain-only --tree DIR`` is the child mode: the unmarked pool of the package under DIR, one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SR = 22050
MESSAGE = "@MyShell"
PUSH = SR // 10


def voice(v, seconds=10):
    rng = np.random.default_rng(2000 + v)
    n = seconds * SR
    t = np.arange(n) / SR
    phase = 2 * np.pi * np.cumsum(140.0 + 3 * v + 40.0 * np.sin(2 * np.pi * 0.3 * t)) / SR
    y = (0.35 * np.sin(phase) + 0.15 * np.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * t))
    return torch.from_numpy((y + 0.01 * rng.standard_normal(n)).astype(np.float32))


def converter(api, **kw):
    from openvoice_amd.params import synthetic_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG, default_converter_hparams
    work = tempfile.mkdtemp(prefix="watermark_stream_table_")
    hps = default_converter_hparams("v2")
    with open(os.path.join(work, "config.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, seed=1234)}, os.path.join(work, "checkpoint.pth"))
    tcc = api.ToneColorConverter(os.path.join(work, "config.json"), device=DEV, **kw)
    tcc.load_ckpt(os.path.join(work, "checkpoint.pth"))
    return tcc


class Ticker:
    """A live pool of N streams fed 100 ms per tick from a looping 10 s signal."""

    def __init__(self, tcc, ses, n, **open_kw):
        self.pool = tcc.live_pool(chunk_frames=15)
        self.hs = [self.pool.open(*ses, seed=(3, i), **open_kw) for i in range(n)]
        self.wave, self.at = voice(0).to(DEV), 0

    def ticks(self, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            x = self.wave[self.at:self.at + PUSH]
            self.at = (self.at + PUSH) % (self.wave.numel() - PUSH)
            for h in self.hs:
                self.pool.push(h, x)
            self.pool.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / count


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": [float(x) for x in v]}


def plain_only(args):
    sys.path.insert(0, args.tree)
    from openvoice_amd import api
    tcc = converter(api, enable_watermark=False)
    gen = torch.Generator().manual_seed(11)
    ses = [(0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV) for _ in range(2)]
    t = Ticker(tcc, ses, args.streams)
    t.ticks(args.warmup)
    print(json.dumps({"tree": os.path.abspath(args.tree), "ms_per_tick": stats([t.ticks(args.ticks) for _ in range(args.reps)])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--hold", type=int, default=3200)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.plain_only:
        return plain_only(args)

    sys.path.insert(0, REPO)
    from openvoice_amd import api, watermark
    result = {"reps": args.reps, "ticks_per_rep": args.ticks, "streams": args.streams, "chunk_frames": 15,
              "push_samples": PUSH, "message": MESSAGE,
              "clock": "host wall time around a device synchronise, per tick, the pools alternating inside one loop"}
    # the children first: one process with the GPU open at a time
    if args.parent_tree:
        runs = []
        for tree in (args.parent_tree, REPO, args.parent_tree, REPO):
            cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--tree", tree, "--reps", str(args.reps),
                   "--ticks", str(args.ticks), "--warmup", str(args.warmup), "--streams", str(args.streams)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
            runs.append(dict(json.loads(out), which="parent" if tree == args.parent_tree else "this"))
        result["unmarked_pool_by_tree"] = runs
        par = [r["ms_per_tick"]["median"] for r in runs if r["which"] == "parent"]
        own = [r["ms_per_tick"]["median"] for r in runs if r["which"] == "this"]
        result["parent_run_to_run_ms"] = abs(par[0] - par[1])
        result["this_minus_parent_ms"] = float(np.mean(own) - np.mean(par))

    tcc = converter(api, watermark="native")
    result["device"] = torch.cuda.get_device_name(0)
    gen = torch.Generator().manual_seed(11)
    ses = [(0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV) for _ in range(2)]

    # ---- how loud, per hold
    native = tcc.watermark_model
    tcc.watermark_model = None
    x = torch.from_numpy(tcc.convert_many([voice(0).to(DEV)], *ses, seed=1)[0]).to(DEV)
    tcc.watermark_model = native
    bits = torch.tensor(api.string_to_bits(MESSAGE).reshape(-1, 32), dtype=torch.float32).to(DEV)
    wins = lambda w: torch.stack([w[s:s + watermark.WINDOW] for s in (0, watermark.STRIDE)]).double()
    result["smr"] = {}
    for H in watermark.HOLDS:
        y = watermark.StreamMarker(watermark.stream_mark(native, MESSAGE, H), DEV).close(x.clone())
        xd, yd = wins(x), wins(y)
        per = 10.0 * torch.log10((xd * xd).sum(1) / ((yd - xd) ** 2).sum(1))
        read_ok = bool(torch.equal(native.decode(wins(y).float()) >= 0.5, bits == 1))
        result["smr"][str(H)] = {"db": float(10.0 * torch.log10((xd * xd).sum() / ((yd - xd) ** 2).sum())),
                                 "per_window_db": [float(v) for v in per], "reads_back": read_ok}

    # ---- how long: the same pool with and without messages, alternating
    pools = {"unmarked": Ticker(tcc, ses, args.streams),
             "marked": Ticker(tcc, ses, args.streams, message=MESSAGE, watermark_hold=args.hold, message_repeat=True)}
    for p in pools.values():
        p.ticks(args.warmup)
    times = {name: [] for name in pools}
    before = native.launches
    for _ in range(args.reps):
        for name, p in pools.items():
            times[name].append(p.ticks(args.ticks))
    result["hold"] = args.hold
    result["mark_launches_per_tick"] = (native.launches - before) / (args.reps * args.ticks)
    result["live_pool_ms_per_tick"] = {name: stats(v) for name, v in times.items()}
    result["marked_minus_unmarked_ms"] = (result["live_pool_ms_per_tick"]["marked"]["median"] -
                                          result["live_pool_ms_per_tick"]["unmarked"]["median"])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
