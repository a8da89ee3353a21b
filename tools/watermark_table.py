#!/usr/bin/env python3
"""What the native watermark (openvoice_amd/watermark.py) costs and how loud it is.

* Signal-to-mark ratio ``10 log10(sum x^2 / sum (y - x)^2)`` over the carrier windows of a synthetic 10 s conversion's
  output and of a speech-like test signal (a modulated two-tone voice), at strength 0.01, 0.02 (the default) and 0.05.
  Expectation from the scheme: the projection of unmarked audio on 500 chips is about rms / sqrt(500) = 0.045 rms, more
  than the default level 0.02 rms, so a bit that needs correcting moves its samples by about 1 / sqrt(500) of the rms
  and the mark's power is about 1 / 500 of the window's: upper 20s of dB at the default strength, falling slowly as
  the strength grows.
* Time of ``convert_many`` of 32 x 10 s: without a watermark, with ``watermark="native"`` (one launch marks all 64
  windows on the device), and with the same model behind the host-loop hook (one copy to the device and back per window).
  Median of ``--reps`` with a device synchronise, the three alternating inside one loop; all repetitions reported.
* ``mark_many`` alone on the 32 converted waveforms.

    python tools/watermark_table.py [--reps 7] [--out profiles/watermark_table.json]

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

from openvoice_amd import api, watermark  # noqa: E402
from openvoice_amd.params import synthetic_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
SR = 22050
MESSAGE = "@MyShell"


def voice(v, seconds=10):
    rng = np.random.default_rng(2000 + v)
    n = seconds * SR
    t = np.arange(n) / SR
    phase = 2 * np.pi * np.cumsum(140.0 + 3 * v + 40.0 * np.sin(2 * np.pi * 0.3 * t)) / SR
    y = (0.35 * np.sin(phase) + 0.15 * np.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * t))
    return torch.from_numpy((y + 0.01 * rng.standard_normal(n)).astype(np.float32))


class HostLoop:
    """The same model behind the per-window host loop of ``add_watermark``: any object that is not a NativeWatermark."""

    def __init__(self, wm):
        self.encode, self.decode = wm.encode, wm.decode


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def windows_of(wave):
    """[groups, 16000]: the carrier windows of a waveform that hold the 8-character message."""
    return torch.stack([wave[s:s + watermark.WINDOW] for s in (0, watermark.STRIDE)])


def smr_db(x, strength):
    wm = watermark.NativeWatermark(strength=strength).to(DEV)
    bits = torch.tensor(api.string_to_bits(MESSAGE).reshape(-1, 32), dtype=torch.float32)
    y = wm.encode(x, bits)
    xd, yd = x.double(), y.double()
    per = 10.0 * torch.log10((xd * xd).sum(1) / ((yd - xd) ** 2).sum(1))
    total = 10.0 * torch.log10((xd * xd).sum() / ((yd - xd) ** 2).sum())
    q, level = wm.read(x)
    b = 2.0 * bits.to(DEV) - 1.0
    return {"db": float(total), "per_window_db": [float(v) for v in per],
            "bits_corrected": int((b * q < level[:, None]).sum()), "bits": int(bits.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    work = tempfile.mkdtemp(prefix="watermark_table_")
    hps = default_converter_hparams("v2")
    with open(os.path.join(work, "config.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, seed=1234)}, os.path.join(work, "checkpoint.pth"))
    tcc = api.ToneColorConverter(os.path.join(work, "config.json"), device=DEV, watermark="native")
    tcc.load_ckpt(os.path.join(work, "checkpoint.pth"))
    native = tcc.watermark_model
    gen = torch.Generator().manual_seed(11)
    ses = [(0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV) for _ in range(2)]
    waves = [voice(v).to(DEV) for v in range(args.items)]

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "items": args.items, "seconds_per_item": 10,
              "windows_marked": 2 * args.items, "message": MESSAGE,
              "clock": "host wall time around a device synchronise, after 2 warm-up rounds, the paths alternating"}

    # ---- how loud
    tcc.watermark_model = None
    converted = torch.from_numpy(tcc.convert_many(waves[:1], *ses, seed=1)[0]).to(DEV)
    result["smr"] = {name: {str(s): smr_db(windows_of(sig), s) for s in (0.01, 0.02, 0.05)}
                     for name, sig in (("conversion_output", converted), ("speech_like_signal", waves[0]))}

    # ---- how long
    models = {"none": None, "native": native, "host_loop": HostLoop(native)}

    def run(name):
        tcc.watermark_model = models[name]
        return tcc.convert_many(waves, *ses, message=MESSAGE, seed=1)

    for _ in range(2):
        outs = {name: run(name) for name in models}
    assert all(np.array_equal(a, b) for a, b in zip(outs["native"], outs["host_loop"]))
    assert not np.array_equal(outs["native"][0], outs["none"][0])
    times = {name: [] for name in models}
    for _ in range(args.reps):
        for name in models:
            times[name].append(wall_ms(lambda: run(name))[0])
    result["convert_many_ms"] = {name: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "all": v}
                                 for name, v in times.items()}
    med = {name: result["convert_many_ms"][name]["median"] for name in models}
    result["native_minus_none_ms"] = med["native"] - med["none"]
    result["host_loop_minus_none_ms"] = med["host_loop"] - med["none"]

    # ---- the marking alone, on waveforms laid out like convert_many's outputs (views of one tensor)
    packed = torch.cat([torch.from_numpy(o) for o in outs["none"]]).to(DEV)
    views, acc = [], 0
    for o in outs["none"]:
        views.append(packed[acc:acc + len(o)])
        acc += len(o)
    for _ in range(2):
        native.mark_many(views, MESSAGE)
    alone, before = [], native.launches
    for _ in range(args.reps):
        alone.append(wall_ms(lambda: native.mark_many(views, MESSAGE))[0])
    result["mark_many_ms"] = {"median": float(np.median(alone)), "min": float(min(alone)), "max": float(max(alone)),
                              "all": alone, "launches_per_call": (native.launches - before) / args.reps}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
