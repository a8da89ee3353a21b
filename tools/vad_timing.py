#!/usr/bin/env python3
"""What silence removal costs (openvoice_amd/vad.py, csrc/vad.hip), measured with HIP events after warm-up:

* the three launches (frame energy, segments, compaction) for one 60 s recording and for 32 x 60 s in one call, next to
  the spectrogram + ``ref_enc`` of the same audio (what ``extract_se`` runs on it: the bound the detector must stay under);
* ``get_se`` wall time on a 60 s WAV without a silent frame, ``vad=True`` against ``vad=False`` (``vad=False`` is the
  path every ``get_se`` call took before the detector existed: ``split_audio_equal`` + ``extract_se``).

    python tools/vad_timing.py [--iters 50] [--out profiles/vad_timing.json]

Prints one JSON line (and writes it to ``--out``).  Synthetic converter weights: timings do not depend on the values.
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

from openvoice_amd import _lib, api, audio_io, se_extractor, vad  # noqa: E402
from openvoice_amd.params import synthetic_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
SR, H = 22050, 256


def speechlike(n, seed, pauses=True):
    """A modulated two-tone voice; with ``pauses`` every fifth second is -70 dBFS noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    y = (0.35 * np.sin(2 * np.pi * 150 * t) + 0.15 * np.sin(2 * np.pi * 470 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * t))
    y = y + 0.01 * rng.standard_normal(n)
    if pauses:
        y = y * ((t % 5.0) < 3.8)
    return (y + 10 ** (-70 / 20) * rng.standard_normal(n)).astype(np.float32)


def events_ms(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters


def three_launches(R, iters):
    """Per-kernel and total milliseconds of the three launches on R x 60 s, buffers allocated once."""
    n = 60 * SR
    stride = -(-n // 4) * 4
    pool = torch.cat([torch.from_numpy(np.pad(speechlike(n, r), (0, stride - n))) for r in range(R)]).to(DEV)
    records = torch.tensor([[r * stride, n] for r in range(R)], dtype=torch.int64).to(DEV)
    out_bases = records[:, 0].contiguous()
    ldT = -(-n // H)
    energy = torch.empty(R, ldT, dtype=torch.float32, device=DEV)
    mask = torch.empty(R, ldT, dtype=torch.int32, device=DEV)
    offsets = torch.empty(R, ldT, dtype=torch.int64, device=DEV)
    n_active = torch.empty(R, dtype=torch.int64, device=DEV)
    out = torch.empty_like(pool)
    p = vad.VadParams()
    floor_lin, range_lin = p.linear()
    frames = p.frames(SR, H)

    def k_energy():
        _lib.call("ov_vad_frame_energy_f32", pool, pool.numel(), records, R, H, ldT, energy)

    def k_segments():
        _lib.call("ov_vad_segments_i32", energy, records, R, H, ldT, floor_lin, range_lin, *frames, mask, offsets, n_active)

    def k_compact():
        _lib.call("ov_vad_compact_f32", pool, pool.numel(), records, R, H, ldT, mask, offsets, out_bases, out, out.numel())

    def all_three():
        k_energy(); k_segments(); k_compact()

    res = {"energy_ms": events_ms(k_energy, iters), "segments_ms": events_ms(k_segments, iters),
           "compact_ms": events_ms(k_compact, iters), "three_launches_ms": events_ms(all_three, iters)}
    res["kept_fraction"] = float(n_active.sum().item()) / (R * n)
    return res, pool, stride, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    work = tempfile.mkdtemp(prefix="vad_timing_")
    hps = default_converter_hparams("v2")
    with open(os.path.join(work, "config.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, seed=1234)}, os.path.join(work, "checkpoint.pth"))
    tcc = api.ToneColorConverter(os.path.join(work, "config.json"), device=DEV, enable_watermark=False)
    tcc.load_ckpt(os.path.join(work, "checkpoint.pth"))

    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    for R in (1, 32):
        res, pool, stride, n = three_launches(R, args.iters)
        # the same audio through what extract_se runs on it: 6 x 10 s pieces per recording, one spectrogram + ref_enc
        pieces = torch.stack([pool[r * stride:r * stride + n].reshape(6, n // 6) for r in range(R)]).reshape(6 * R, n // 6)

        def spec_ref_enc():
            with torch.no_grad():
                tcc.model.ref_enc(tcc._spec(pieces).transpose(1, 2))
        res["spectrogram_ref_enc_ms"] = events_ms(spec_ref_enc, max(5, args.iters // 5), warmup=3)
        res["vad_over_spectrogram_ref_enc"] = res["three_launches_ms"] / res["spectrogram_ref_enc_ms"]
        result[f"R{R}x60s"] = res

    wav = os.path.join(work, "active60.wav")
    audio_io.write(wav, speechlike(60 * SR, 99, pauses=False), SR)
    walls = {}
    for flag in (True, False):
        times = []
        for i in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                se_extractor.get_se(wav, tcc, target_dir=os.path.join(work, f"p{int(flag)}_{i}"), vad=flag)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        walls["vad_true" if flag else "vad_false"] = {"median_ms": float(np.median(times[2:])), "all_ms": times}
        walls["pieces"] = tcc.last_extract_se_batches
    result["get_se_60s_all_active"] = walls
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
