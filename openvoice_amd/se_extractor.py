"""``get_se`` -- tone-colour embedding of a reference recording (thin shim).

Keeps the reference signature and return value (reference: openvoice/se_extractor.py:129-152):
``get_se(audio_path, vc_model, target_dir='processed', vad=True) -> (se [1,gin,1], audio_name)``.

``vad=True`` (the default) follows the reference's ``split_audio_vad`` (se_extractor.py:77-116): everything a
voice-activity detector calls silence is removed, what is left is concatenated, and only then are the
``num_splits = round(dur / 10)`` equal pieces cut (se_extractor.py:99-115) that ``vc_model.extract_se`` averages over,
written under ``target_dir/<name>/wavs`` like the reference.  The reference's detector is a third-party network (silero
through whisper_timestamped) whose weights are out of scope; the PROCEDURE is honoured with
the deterministic energy detector of ``openvoice_amd/vad.py``, which runs on the device (three HIP launches) with the
reference's ``min_speech_duration = 0.1`` and ``min_silence_duration = 1``.  Parity with silero's decisions is not
claimed and cannot be pinned offline.  A recording without a frame below the detector's threshold is cut into exactly
the pieces ``split_audio_equal`` cuts.

``vad=False`` selects the reference's ASR splitter (faster_whisper, se_extractor.py:19-74), which stays out of scope:
``split_audio_equal`` stands in for it and cuts the raw recording into equal pieces, pauses included.
"""
import base64
import hashlib
import os
from glob import glob

import numpy as np

from . import audio_io


def hash_numpy_array(audio_path):
    """reference: openvoice/se_extractor.py:118-127 (sha256 of the decoded samples, base64[:16])."""
    try:
        import librosa
        array, _ = librosa.load(audio_path, sr=None, mono=True)
    except ImportError:
        array, _ = audio_io.read_native(audio_path)
    array = np.asarray(array, dtype=np.float32)
    if array.ndim > 1:
        array = array.mean(axis=1)
    digest = hashlib.sha256(np.ascontiguousarray(array).tobytes()).digest()
    return base64.b64encode(digest).decode("utf-8")[:16].replace("/", "_^")


def split_audio_equal(audio_path, audio_name, target_dir, sampling_rate, split_seconds=10.0):
    audio, sr = audio_io.load(audio_path, sr=sampling_rate)
    dur = len(audio) / float(sr)
    wavs_folder = os.path.join(target_dir, audio_name, "wavs")
    os.makedirs(wavs_folder, exist_ok=True)
    num_splits = int(np.round(dur / split_seconds))
    assert num_splits > 0, "input audio is too short"
    bounds = np.linspace(0, len(audio), num_splits + 1).astype(np.int64)
    for i in range(num_splits):
        audio_io.write(os.path.join(wavs_folder, f"{audio_name}_seg{i}.wav"), audio[bounds[i]:bounds[i + 1]], sr)
    return wavs_folder


def split_audio_vad(audio_path, audio_name, target_dir, split_seconds=10.0, sampling_rate=None, device=None,
                    hop_length=None):
    """reference: openvoice/se_extractor.py:77-116, with the energy detector of ``vad.remove_silence`` on ``device``.
    ``sampling_rate`` / ``hop_length`` default to the converter's (22 050 Hz / 256), ``device`` to ``cuda:0``."""
    from . import vad
    from .utils import default_converter_hparams
    data = default_converter_hparams("v2").data
    sr = int(sampling_rate or data.sampling_rate)
    audio = audio_io.load_to_device(audio_path, sr, device or "cuda:0")
    active, segments = vad.remove_silence(audio, sr, int(hop_length or data.hop_length))
    print([(s / sr, e / sr) for s, e in segments])
    audio_active = active.cpu().numpy()
    audio_dur = len(audio_active) / float(sr)
    print(f"after vad: dur = {audio_dur}")
    wavs_folder = os.path.join(target_dir, audio_name, "wavs")
    os.makedirs(wavs_folder, exist_ok=True)
    num_splits = int(np.round(audio_dur / split_seconds))
    assert num_splits > 0, "input audio is too short"
    bounds = np.linspace(0, len(audio_active), num_splits + 1).astype(np.int64)
    for i in range(num_splits):
        audio_io.write(os.path.join(wavs_folder, f"{audio_name}_seg{i}.wav"), audio_active[bounds[i]:bounds[i + 1]], sr)
    return wavs_folder


def get_se(audio_path, vc_model, target_dir="processed", vad=True):
    version = vc_model.version
    print("OpenVoice version:", version)
    audio_name = f"{os.path.basename(audio_path).rsplit('.', 1)[0]}_{version}_{hash_numpy_array(audio_path)}"
    se_path = os.path.join(target_dir, audio_name, "se.pth")
    data = vc_model.hps.data
    if vad:
        wavs_folder = split_audio_vad(audio_path, audio_name, target_dir, sampling_rate=data.sampling_rate,
                                      device=vc_model.device, hop_length=data.hop_length)
    else:
        wavs_folder = split_audio_equal(audio_path, audio_name, target_dir, data.sampling_rate)
    audio_segs = sorted(glob(f"{wavs_folder}/*.wav"))
    if len(audio_segs) == 0:
        raise NotImplementedError("No audio segments found!")
    return vc_model.extract_se(audio_segs, se_save_path=se_path), audio_name


def _write_pieces(audio, sr, audio_name, target_dir, split_seconds=10.0):
    """The cut of ``split_audio_vad`` / ``split_audio_equal``: ``round(dur / 10)`` pieces between ``np.linspace``
    bounds, written under ``target_dir/<audio_name>/wavs``.  Returns the folder."""
    wavs_folder = os.path.join(target_dir, audio_name, "wavs")
    os.makedirs(wavs_folder, exist_ok=True)
    num_splits = int(np.round(len(audio) / float(sr) / split_seconds))
    assert num_splits > 0, "input audio is too short"
    bounds = np.linspace(0, len(audio), num_splits + 1).astype(np.int64)
    for i in range(num_splits):
        audio_io.write(os.path.join(wavs_folder, f"{audio_name}_seg{i}.wav"), audio[bounds[i]:bounds[i + 1]], sr)
    return wavs_folder


def get_se_many(audio_paths, vc_model, target_dir="processed", vad=True):
    """``get_se`` for many recordings with shared launches: ``[(se [1,gin,1], audio_name), ...]`` in the order of
    ``audio_paths``, each pair and the files under ``target_dir/<audio_name>`` (the pieces under ``wavs``, ``se.pth``)
    what ``get_se(path, vc_model, target_dir, vad)`` produces for that path.  All recordings are decoded first; with
    ``vad=True`` their silence is removed in ONE ``vad.remove_silence_many`` call; the pieces are cut and written as
    ``split_audio_vad`` / ``split_audio_equal`` do and read back from the files (the WAV round trip is part of what
    ``get_se`` computes); then ONE ``vc_model.extract_se_many`` call embeds every piece of every recording, whatever
    their lengths, and averages per recording."""
    import torch
    if isinstance(audio_paths, (str, bytes)) or len(audio_paths) == 0:
        raise ValueError("get_se_many: audio_paths must be a non-empty list of paths")
    version = vc_model.version
    print("OpenVoice version:", version)
    data = vc_model.hps.data
    sr = int(data.sampling_rate)
    names = [f"{os.path.basename(p).rsplit('.', 1)[0]}_{version}_{hash_numpy_array(p)}" for p in audio_paths]
    if vad:
        from . import vad as vad_mod
        audios = [audio_io.load_to_device(p, sr, vc_model.device) for p in audio_paths]
        kept, segments = vad_mod.remove_silence_many(audios, sr, int(data.hop_length))
        actives = []
        for active, segs in zip(kept, segments):
            print([(s / sr, e / sr) for s, e in segs])
            actives.append(active.cpu().numpy())
            print(f"after vad: dur = {len(actives[-1]) / float(sr)}")
    else:
        actives = [audio_io.load(p, sr=sr)[0] for p in audio_paths]
    voices = []
    for audio, name in zip(actives, names):
        wavs_folder = _write_pieces(audio, sr, name, target_dir)
        audio_segs = sorted(glob(f"{wavs_folder}/*.wav"))
        if len(audio_segs) == 0:
            raise NotImplementedError("No audio segments found!")
        voices.append([audio_io.load_to_device(f, sr, vc_model.device) for f in audio_segs])
    gs = vc_model.extract_se_many(voices)
    out = []
    for v, name in enumerate(names):
        se = gs[v:v + 1].clone()
        se_path = os.path.join(target_dir, name, "se.pth")
        os.makedirs(os.path.dirname(se_path), exist_ok=True)
        torch.save(se.cpu(), se_path)
        out.append((se, name))
    return out
