"""Time to first audio of streaming synthesis against the one-pass calls, on synthetic weights.

For one sentence of about 100 symbols and one request of three such sentences, at ``chunk_frames`` 15 and 60, on the
fp32 and the bf16 generator: wall time of ``tts_from_ids`` (the one-pass call), of the first chunk that
``tts_stream_from_ids`` yields and of the whole stream, and the same for ``speak_ids`` against ``speak_stream_ids``.
Every figure is taken with a device synchronise and is the median of ``--repeats`` (7) runs after a warm-up run.
Writes ``profiles/tts_stream_table.json``.  Run on the GPU: ``python tools/tts_stream_table.py``.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from openvoice_amd import api, clone, tts_live  # noqa: E402
from openvoice_amd.params import synthetic_state_dict, synthetic_tts_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG as CFG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"


def build(d):
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=True),
           "model": dict(CFG), "symbols": [f"s{i}" for i in range(68)], "speakers": {"default": 1}}
    with open(os.path.join(d, "tts.json"), "w") as fh:
        json.dump(cfg, fh)
    torch.save({"model": synthetic_tts_state_dict(CFG, 68, 10, 513, seed=4321)}, os.path.join(d, "tts.pth"))
    tts = api.BaseSpeakerTTS(os.path.join(d, "tts.json"), device=DEV)
    tts.load_ckpt(os.path.join(d, "tts.pth"))
    hps = default_converter_hparams("v2")
    with open(os.path.join(d, "conv.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CFG, 513, seed=1234)}, os.path.join(d, "conv.pth"))
    conv = api.ToneColorConverter(os.path.join(d, "conv.json"), device=DEV, enable_watermark=False)
    conv.load_ckpt(os.path.join(d, "conv.pth"))
    return tts, conv


def timed(fn, repeats):
    """``fn() -> dict`` run once to warm up, then ``repeats`` times: the median of every ``*_ms`` entry (seconds in,
    milliseconds out); the other entries are counts and pass through."""
    fn()
    runs = [fn() for _ in range(repeats)]
    return {k: round(1e3 * statistics.median(r[k] for r in runs), 3) if k.endswith("_ms") else runs[0][k] for k in runs[0]}


def one_pass(call):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return {"one_pass_ms": time.perf_counter() - t0}
    return run


def stream(make):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen = make()
        first = next(gen)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n = first.numel() + sum(o.numel() for o in gen)
        torch.cuda.synchronize()
        return {"first_chunk_ms": t1 - t0, "stream_total_ms": time.perf_counter() - t0, "samples": n,
                "first_chunk_samples": first.numel()}
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tts_stream_table.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        tts, conv = build(d)
    cloner = clone.VoiceCloner(tts, conv)
    gen = torch.Generator().manual_seed(7)
    sentence = lambda: api.intersperse(torch.randint(1, 68, (50,), generator=gen).tolist(), 0)      # 101 symbols
    requests = {"one_sentence": [sentence()], "three_sentences": [sentence() for _ in range(3)]}
    src, tgt = (0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV) for _ in range(2))
    rows, seed = [], 11
    for name, seqs in requests.items():
        for generator in ("fp32", "bf16"):
            base = timed(one_pass(lambda: tts.tts_from_ids(seqs, 1, seed=seed, generator=generator)), args.repeats)
            speak = timed(one_pass(lambda: cloner.speak_ids(seqs, 1, src, tgt, generator=generator)), args.repeats)
            for chunk in (15, 60):
                t = timed(stream(lambda: tts.tts_stream_from_ids(seqs, 1, seed=seed, chunk_frames=chunk,
                                                                 generator=generator)), args.repeats)
                s = timed(stream(lambda: cloner.speak_stream_ids(seqs, 1, src, tgt, seed=seed, chunk_frames=chunk,
                                                                 generator=generator)), args.repeats)
                row = dict(request=name, generator=generator, chunk_frames=chunk,
                           first_audio_frames=tts_live.first_audio_frames(CFG, chunk),
                           audio_seconds=round(t["samples"] / 22050, 3),
                           tts_one_pass_ms=base["one_pass_ms"], tts_first_chunk_ms=t["first_chunk_ms"],
                           tts_stream_total_ms=t["stream_total_ms"],
                           tts_first_chunk_samples=t["first_chunk_samples"],
                           speak_one_pass_ms=speak["one_pass_ms"], speak_first_chunk_ms=s["first_chunk_ms"],
                           speak_stream_total_ms=s["stream_total_ms"])
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, weights="synthetic",
               note="milliseconds, median of the repeats, each with a device synchronise; one_pass = tts_from_ids / "
                    "speak_ids (per-sentence loop, results copied to the host), stream = tts_stream_from_ids / "
                    "speak_stream_ids (device tensors)", rows=rows)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
