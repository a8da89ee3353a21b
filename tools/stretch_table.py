#!/usr/bin/env python3
"""What ``speed=`` costs (openvoice_amd/stretch.py, csrc/stretch.hip): ``convert_batch`` of 32 waveforms of 861 frames
(10 s at 22.05 kHz, synthetic weights) at ``speed`` None / 0.75 / 1.0 / 1.5, next to the unstretched conversion of a batch
of ``T_out`` frames -- what a stretched call should be close to, since the generator is 98 % of the work and runs on
``T_out`` frames -- and the ``ov_stretch_rows_f32`` launch alone (32 x 192 rows).

Host wall time around a device synchronise, median of ``--reps`` after two warm-up rounds, the cases alternating inside
one loop; every repetition is reported.  On a tree without ``openvoice_amd/stretch.py`` (the parent commit) only the
``speed=None`` case runs: write that to a file and hand it to ``--parent`` on this tree, and the table records both.
``speed=None`` is expected within the run-to-run spread of the parent, ``speed=1.0`` equal to ``speed=None`` (it
launches nothing).  Perceptual quality is NOT measured here or anywhere: the weights are synthetic and no listening test
is possible.

    python tools/stretch_table.py [--reps 7] [--parent parent.json] [--out profiles/stretch_table.json]
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

try:
    from openvoice_amd import stretch
except ImportError:          # the parent commit: the speed=None case alone
    stretch = None

DEV = "cuda:0"
B, T, HOP = 32, 861, 256


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def converter():
    d = tempfile.mkdtemp(prefix="stretch_table_")
    hps = default_converter_hparams("v2")
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, seed=0)}, os.path.join(d, "checkpoint.pth"))
    t = api.ToneColorConverter(os.path.join(d, "config.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(os.path.join(d, "checkpoint.pth"))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent", default=None, help="this tool's output on the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tcc = converter()
    gen = torch.Generator().manual_seed(3)
    g_src, g_tgt = ((0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV) for _ in range(2))
    wave = lambda frames: (0.3 * torch.randn(B, HOP * frames, generator=gen)).to(DEV)
    y = wave(T)
    cases = {"speed_none": lambda: tcc.convert_batch(y, g_src, g_tgt, tau=0.3, seed=1)}
    frames = {"speed_none": T}
    if stretch is not None:
        from openvoice_amd.engine import stretch_rows
        eng = tcc.model.engine()
        for speed in (0.75, 1.0, 1.5):
            step = stretch.step_of(speed)
            n = stretch.t_out(T, step)
            frames[f"speed_{speed}"] = n
            cases[f"speed_{speed}"] = lambda speed=speed: tcc.convert_batch(y, g_src, g_tgt, tau=0.3, seed=1, speed=speed)
            if n != T:
                yn = wave(n)
                frames[f"unstretched_{n}_frames"] = n
                cases[f"unstretched_{n}_frames"] = lambda yn=yn: tcc.convert_batch(yn, g_src, g_tgt, tau=0.3, seed=1)
                src = torch.randn(B * 192 * T, generator=gen).to(DEV)
                dst = torch.empty(B * 192 * n, device=DEV)
                host = torch.tensor([v for b in range(B) for v in stretch.record(b * 192 * T, b * 192 * n, 192, T, n, T, 0, 0, n,
                                                                                  step)], dtype=torch.int64)
                table = host.to(DEV)
                frames[f"kernel_alone_{speed}"] = n
                cases[f"kernel_alone_{speed}"] = lambda a=(table, host, B, src, dst): stretch_rows(*a)
        eng.resident_workspaces = 4          # the cases alternate between three shapes: keep their workspaces
    for _ in range(2):
        for fn in cases.values():
            wall_ms(fn)
    times = {name: [] for name in cases}
    for _ in range(args.reps):
        for name, fn in cases.items():
            times[name].append(wall_ms(fn))
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "batch": B, "frames_in": T,
              "tree": "this commit" if stretch is not None else "parent commit (no openvoice_amd/stretch.py)",
              "clock": "host wall time around a device synchronise, after 2 warm-up rounds, the cases alternating",
              "perceptual_quality": "not measured: synthetic weights, no listening test possible",
              "cases": {name: {"frames_out": frames[name], "median_ms": float(np.median(v)), "min_ms": float(min(v)),
                               "max_ms": float(max(v)), "all_ms": v} for name, v in times.items()}}
    if args.parent:
        with open(args.parent) as fh:
            parent = json.loads(fh.readline())
        result["parent_speed_none"] = dict(parent["cases"]["speed_none"], tree=parent["tree"], device=parent["device"])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
