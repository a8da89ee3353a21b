#!/usr/bin/env python3
"""What "say this text in that voice" costs, for 1, 8 and 32 requests of 3 sentences x ~60 symbol ids (wall time with a
device sync, median of 5 after warm-up):

* (a) the file chain as a user writes it without ``openvoice_amd.clone``: per request ``BaseSpeakerTTS.tts`` to a WAV,
  then ``ToneColorConverter.convert`` from that file (two host round trips, one file, two batch-1 passes per request);
* (b) ``VoiceCloner.speak_ids_many`` on the same sentences (and ``speak_many``, which adds the text front end (a)
  pays too);
* the join launches of (b) on their own (HIP events), against the conversion they feed.

    python tools/clone_timing.py [--out profiles/clone_timing.json]

Prints one JSON line (and writes it to ``--out``).  Synthetic weights: timings do not depend on the values.  The text
front end is a one-line stand-in (a character -> id table), as in the tests: it is third-party CPU code in the reference.
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

from openvoice_amd import api, clone  # noqa: E402
from openvoice_amd.params import synthetic_state_dict, synthetic_tts_state_dict  # noqa: E402
from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
WORDS = "the quick brown fox jumps over a lazy dog near an old mill by this river bank".split()


def text_of(seed):
    """Three sentences of 12 words, ~60 characters each (more than split_sentence's 10 words: they stay apart)."""
    rng = np.random.default_rng(seed)
    return " ".join(" ".join(rng.choice(WORDS, size=12)) + "." for _ in range(3))


def models(work):
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=False),
           "model": dict(CONVERTER_MODEL_CONFIG), "symbols": [f"s{i}" for i in range(68)], "speakers": {"default": 1}}
    with open(os.path.join(work, "tts.json"), "w") as fh:
        json.dump(cfg, fh)
    torch.save({"model": synthetic_tts_state_dict(CONVERTER_MODEL_CONFIG, 68, 10, 513, seed=4321)},
               os.path.join(work, "tts.pth"))
    hps = default_converter_hparams("v2")
    with open(os.path.join(work, "conv.json"), "w") as fh:
        json.dump({"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}, fh)
    torch.save({"model": synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, seed=1234)}, os.path.join(work, "conv.pth"))
    with contextlib.redirect_stdout(io.StringIO()):
        tts = api.BaseSpeakerTTS(os.path.join(work, "tts.json"), device=DEV)
        tts.load_ckpt(os.path.join(work, "tts.pth"))
        conv = api.ToneColorConverter(os.path.join(work, "conv.json"), device=DEV, enable_watermark=False)
        conv.load_ckpt(os.path.join(work, "conv.pth"))
    return tts, conv


def wall_ms(fn, runs=5, warmup=2):
    times = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(times[warmup:])), "all_ms": [round(t, 3) for t in times[warmup:]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--requests", type=int, nargs="*", default=[1, 8, 32])
    args = ap.parse_args()
    work = tempfile.mkdtemp(prefix="clone_timing_")
    tts, conv = models(work)
    vc = clone.VoiceCloner(tts, conv)
    gen = torch.Generator().manual_seed(0)
    se = lambda: 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV)
    api.BaseSpeakerTTS.text_to_sequence = staticmethod(lambda text, symbols, cleaners: [1 + (ord(c) % 67) for c in text])
    result = {"device": torch.cuda.get_device_name(0), "sentences_per_request": 3, "runs": 5}
    for n in args.requests:
        texts = [text_of(100 * n + i) for i in range(n)]
        srcs, tgts = [se() for _ in range(n)], [se() for _ in range(n)]
        with contextlib.redirect_stdout(io.StringIO()):
            ids = [tts.text_to_ids(t, "English") for t in texts]
        requests = [(i, "default", s, t) for i, s, t in zip(ids, srcs, tgts)]

        def file_chain():
            for i, text in enumerate(texts):
                wav = os.path.join(work, f"base{i}.wav")
                tts.tts(text, wav, speaker="default", language="English", speed=1.0)
                conv.convert(wav, srcs[i], tgts[i], output_path=os.path.join(work, f"out{i}.wav"))

        def cloner_files():
            vc.speak_ids_many(requests, output_paths=[os.path.join(work, f"clone{i}.wav") for i in range(n)])

        res = {"ids_per_sentence_mean": float(np.mean([len(s) for req in ids for s in req])),
               "file_chain": wall_ms(file_chain),
               "speak_ids_many": wall_ms(lambda: vc.speak_ids_many(requests)),
               "speak_ids_many_writing_wavs": wall_ms(cloner_files),
               "speak_many_from_text": wall_ms(lambda: vc.speak_many(texts, "default", srcs, tgts))}
        res["file_chain_over_speak_ids_many"] = res["file_chain"]["median_ms"] / res["speak_ids_many"]["median_ms"]
        res["file_chain_over_speak_ids_many_writing_wavs"] = (res["file_chain"]["median_ms"] /
                                                              res["speak_ids_many_writing_wavs"]["median_ms"])
        res["infer_launches"] = vc.last_launches["infer"]

        # the join on its own: the launches speak_ids_many issues, replayed on the last call's TTS outputs
        reqs = vc._parse(requests, None, None, None, None)
        launches = []
        real = clone._launch_join
        clone._launch_join = lambda o, records, dst: (launches.append((o, records, dst)), real(o, records, dst))
        try:
            with torch.no_grad():
                waves = vc.synthesize_many(reqs)
        finally:
            clone._launch_join = real
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def events_ms(fn, iters=20):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            torch.cuda.synchronize()
            return start.elapsed_time(stop) / iters

        res["join_launches"] = len(launches)
        res["join_samples"] = int(sum(w.numel() for w in waves))
        res["join_ms"] = events_ms(lambda: [real(*a) for a in launches])
        from openvoice_amd import longform
        windowed = conv._windowed(longform.DEFAULT_WINDOW_FRAMES, longform.DEFAULT_MANY_WINDOWS_PER_LAUNCH)
        res["convert_many_ms"] = events_ms(lambda: windowed.convert_many(waves, srcs, tgts, tau=0.3), iters=5)
        res["join_over_convert_many"] = res["join_ms"] / res["convert_many_ms"]
        result[f"requests_{n}"] = res
    api.BaseSpeakerTTS.text_to_sequence = None
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
