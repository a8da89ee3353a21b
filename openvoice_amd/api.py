"""Public API of the tone-colour converter, re-hosted on the MI355X engine.

Same class names, constructor/ method signatures, attributes (``model``, ``hps``, ``device``,
``version``, ``watermark_model``) and return types as the reference API layer
(reference: openvoice/api.py:14-201), so the upstream notebooks run unchanged
(``from openvoice.api import ToneColorConverter`` resolves here through the ``openvoice`` alias
package at the repo root).  What differs, on purpose:

* the model behind ``self.model`` is ``openvoice_amd.models.SynthesizerTrn`` whose
  ``voice_conversion`` / ``ref_enc`` run hand-written gfx950 kernels -- there is no eager PyTorch
  compute and no CPU fallback (a 'cpu' device is rejected at construction);
* ``ToneColorConverter.__init__`` strips ``enable_watermark`` before calling the base class (the
  reference forwards it and raises TypeError);
* ``convert_batch`` (new) is the batched entry the benchmark configs use; ``convert`` is file I/O
  around ``convert_batch`` with B = 1;
* audio decode / WAV write go through ``openvoice_amd.audio_io`` (librosa/soundfile when present);
* the watermark (third-party ``wavmark``) stays an optional post-processing hook; ``watermark="native"`` installs the
  project's own device watermark (``openvoice_amd.watermark``, not wavmark-compatible) behind the same hook.
"""
import os
import re

import numpy as np
import torch

from . import _lib, audio_io, longform, rates, utils
from . import stretch as stretch_mod
from .engine import item_tau, wavenet_keyword
from . import noise as noise_mod
from . import watermark as watermark_mod
from .mel_processing import spectrogram_torch
from .models import SynthesizerTrn


class OpenVoiceBaseClass(object):
    """reference: openvoice/api.py:14-39."""

    def __init__(self, config_path, device="cuda:0"):
        if "cuda" in device:
            assert torch.cuda.is_available()
        else:
            raise RuntimeError(f"device {device!r}: the MI355X engine has no CPU path; use 'cuda:N'")
        hps = utils.get_hparams_from_file(config_path)
        model = SynthesizerTrn(
            len(getattr(hps, "symbols", [])),
            hps.data.filter_length // 2 + 1,
            n_speakers=hps.data.n_speakers,
            **hps.model,
        ).to(device)
        model.eval()
        self.model = model
        self.hps = hps
        self.device = device

    def load_ckpt(self, ckpt_path):
        checkpoint_dict = torch.load(ckpt_path, map_location=torch.device(self.device))
        a, b = self.model.load_state_dict(checkpoint_dict["model"], strict=False)
        print("Loaded checkpoint '{}'".format(ckpt_path))
        print("missing/unexpected keys:", a, b)


class BaseSpeakerTTS(OpenVoiceBaseClass):
    """V1 base-speaker TTS (reference: openvoice/api.py:42-98).  The model half
    (``SynthesizerTrn.infer``: text encoder, duration predictors, spline flows, flow, generator) runs on
    the MI355X engine.  The TEXT front end of the reference (``openvoice/text``: cleaners built on
    inflect / eng_to_ipa / pypinyin / jieba) is third-party CPU string
    processing and is not re-implemented: plug a ``text_to_sequence(text, symbols, cleaner_names)``
    callable into ``BaseSpeakerTTS.text_to_sequence`` (the reference's own function works unchanged), or
    call ``tts_from_ids`` with symbol ids."""

    language_marks = {"english": "EN", "chinese": "ZH"}
    text_to_sequence = None     # hook: callable(text, symbols, cleaner_names) -> list[int]

    @classmethod
    def get_text(cls, text, hps, is_symbol):
        """reference: openvoice/api.py:48-54."""
        if cls.text_to_sequence is None and is_symbol:
            # already-cleaned (IPA / symbol) text needs no third-party cleaner: plain symbol lookup
            text_norm = utils.cleaned_text_to_sequence(text, hps.symbols)
            if hps.data.add_blank:
                text_norm = intersperse(text_norm, 0)
            return torch.LongTensor(text_norm)
        if cls.text_to_sequence is None:
            raise RuntimeError("no text front end registered: set BaseSpeakerTTS.text_to_sequence to a "
                               "text_to_sequence(text, symbols, cleaner_names) callable (e.g. the reference's "
                               "openvoice.text.text_to_sequence) or use tts_from_ids()")
        text_norm = cls.text_to_sequence(text, hps.symbols, [] if is_symbol else hps.data.text_cleaners)
        if hps.data.add_blank:
            text_norm = intersperse(text_norm, 0)
        return torch.LongTensor(text_norm)

    @staticmethod
    def audio_numpy_concat(segment_data_list, sr, speed=1.0):
        """reference: openvoice/api.py:56-63 -- segments joined with 50 ms / speed of silence after
        each (built with one allocation instead of a Python list of samples)."""
        gap = np.zeros(int((sr * 0.05) / speed), dtype=np.float32)
        parts = []
        for segment in segment_data_list:
            parts += [np.asarray(segment, dtype=np.float32).reshape(-1), gap]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)

    @staticmethod
    def split_sentences_into_pieces(text, language_str):
        """reference: openvoice/api.py:65-71 (prints the pieces like the reference does)."""
        texts = utils.split_sentence(text, language_str=language_str)
        print(" > Text splitted to sentences.")
        print("\n".join(texts))
        print(" > ===========================")
        return texts

    @staticmethod
    def _batch_noise(noises, width=None):
        """Per-sentence noise tensors ``[C, >= own length]`` -> one ``[B, C, W]`` batch, each cut / zero-padded to ``W``
        columns (``width``, or the widest of them)."""
        noises = [torch.as_tensor(z, dtype=torch.float32) for z in noises]
        W = max(z.shape[-1] for z in noises) if width is None else int(width)
        out = torch.zeros(len(noises), noises[0].shape[-2], W, dtype=torch.float32, device=noises[0].device)
        for i, z in enumerate(noises):
            w = min(W, z.shape[-1])
            out[i, :, :w] = z.reshape(-1, z.shape[-1])[:, :w].to(out.device)
        return out

    @staticmethod
    def per_sentence(name, value, n, integer=False, positive=False):
        """A synthesis control that is one value for all ``n`` sentences, or a list / tuple / array / tensor with one
        per sentence.  Returns ``(False, value)`` for the one value, untouched, and ``(True, [n numbers])`` for the
        list -- ints where ``integer``, floats otherwise.  A list of another length, a non-finite entry, or (where
        ``positive``) an entry ``<= 0`` is a ValueError."""
        if isinstance(value, torch.Tensor):
            value = value.detach().cpu().numpy()
        if isinstance(value, np.ndarray):
            if value.ndim == 0:
                return False, value.item()
            value = value.reshape(-1).tolist()
        if not isinstance(value, (list, tuple)):
            return False, value
        if len(value) != n:
            raise ValueError(f"{name}: one value, or one per sentence ({n}), got {len(value)}")
        if integer:
            return True, [int(v) for v in value]
        vals = [float(v) for v in value]
        if not all(np.isfinite(vals)):
            raise ValueError(f"{name}: non-finite value in {vals}")
        if positive and not all(v > 0 for v in vals):
            raise ValueError(f"{name}: every value must be positive, got {vals}")
        return True, vals

    def _wavenet_cores(self):
        return self.model._wavenet_cores()

    @wavenet_keyword
    @torch.no_grad()
    def infer_padded(self, id_sequences, speaker_id, speed=1.0, noise_scale=0.667, noise_scale_w=0.6, noise_w=None,
                     noise_z=None, *, seed=None, generator="fp32"):
        """One padded ``infer(..., skip_padding=True)`` over already-tokenised sentences, results left on the device:
        ``(o [B, 1, ld], frames [B] int64)`` -- row b holds ``frames[b] * hop`` samples, what lies beyond them in the
        row is padding.  ``noise_w`` / ``noise_z``: None or one ``[2, Tx_b]`` / ``[192, >= Ty_b]`` per sentence (the
        explicit forms of ``infer``'s two draws; in the batch each is zero-padded to the widest); ``seed`` (instead of
        them): counter-based noise (``noise.py``), an int ``s`` giving sentence ``i`` the stream ``(s, i)``, or a list
        with one seed / pair per sentence.  ``generator``: ``"fp32"`` (default) or ``"bf16"`` -- the generator on the
        bf16 kernels, the ragged batch as dense length groups (``TtsEngine.infer``).  ``speaker_id``, ``speed``,
        ``noise_scale`` and ``noise_scale_w``: one value for the batch, or a list with one per sentence (``per_sentence``)
        -- sentences of different speakers and speeds then share this one launch sequence (``infer`` with per-item
        controls), each getting what a batch of its own values gives it.  This is the launch
        sequence behind ``tts_from_ids(batched=True)`` and ``clone.VoiceCloner``."""
        _lib.check_generator(generator)
        noise_mod.exclusive(seed, noise_w=noise_w, noise_z=noise_z)
        device = self.device
        seqs = [torch.as_tensor(s, dtype=torch.long).reshape(-1) for s in id_sequences]
        many_speakers, speaker_id = self.per_sentence("speaker_id", speaker_id, len(seqs), integer=True)
        many_speeds, speed = self.per_sentence("speed", speed, len(seqs), positive=True)
        noise_scale = self.per_sentence("noise_scale", noise_scale, len(seqs))[1]
        noise_scale_w = self.per_sentence("noise_scale_w", noise_scale_w, len(seqs))[1]
        length_scale = [1.0 / s for s in speed] if many_speeds else 1.0 / speed
        if seed is not None:
            seed = noise_mod.per_item(seed, len(seqs))
        for name, nz in (("noise_w", noise_w), ("noise_z", noise_z)):
            if nz is not None and len(nz) != len(seqs):
                raise ValueError(f"{name}: one tensor per sentence ({len(seqs)}), got {len(nz)}")
        lengths = torch.tensor([s.numel() for s in seqs], dtype=torch.long)
        x = torch.zeros(len(seqs), int(lengths.max()), dtype=torch.long)
        for i, s in enumerate(seqs):
            x[i, :s.numel()] = s
        if many_speakers:
            sid = torch.tensor(speaker_id, dtype=torch.long)
        else:
            sid = torch.full((len(seqs),), int(speaker_id), dtype=torch.long)
        if noise_w is not None:
            noise_w = self._batch_noise(noise_w, x.shape[1])
        if noise_z is not None:
            noise_z = self._batch_noise(noise_z)
        # padded batch: the generator computes length + margin (16-20) frames per sentence, not the longest one's (the
        # samples returned below are bit-identical either way)
        o, _, y_mask, _ = self.model.infer(x.to(device), lengths.to(device), sid=sid.to(device), noise_scale=noise_scale,
                                           noise_scale_w=noise_scale_w, length_scale=length_scale, noise_w=noise_w,
                                           noise_z=noise_z, skip_padding=True, **noise_mod.kw(seed),
                                           **self._generator_kw(generator))
        return o, y_mask[:, 0].sum(1).long()

    @staticmethod
    def _generator_kw(generator):
        """The keyword for ``infer``, left out for the default so that the fp32 call is today's call."""
        return {} if generator == "fp32" else {"generator": generator}

    @wavenet_keyword
    @torch.no_grad()
    def tts_from_ids(self, id_sequences, speaker_id, speed=1.0, batched=False, noise_scale=0.667,
                     noise_scale_w=0.6, noise_w=None, noise_z=None, *, seed=None, generator="fp32"):
        """Synthesize already-tokenised sentences (symbol ids, blanks interspersed by the caller if the
        config asks for it).  ``batched=False`` runs one ``infer`` per sentence exactly as the reference loop
        (api.py:78-94); ``batched=True`` pads them into one batch (one pass over the GPU; because the
        generator is unmasked, the last ~13 frames of the shorter items then differ slightly from a
        per-sentence run).  ``noise_w`` / ``noise_z``: None (drawn on the device) or lists with one ``[2, Tx]`` /
        ``[192, >= Ty]`` tensor per sentence, passed on to ``infer``.  ``seed`` (instead of them): counter-based noise,
        an int ``s`` giving sentence ``i`` the stream ``(s, i)`` in the batched and in the per-sentence loop alike (so
        both draw the same durations), or a list with one seed / pair per sentence; a seeded call is reproducible
        without anyone guessing ``Ty``.  ``generator``: ``"fp32"`` (default) or ``"bf16"``, the generator's kernels in
        either loop (``TtsEngine.infer``).  ``speaker_id``, ``speed``, ``noise_scale`` and ``noise_scale_w``: one value,
        or a list with one per sentence -- in the per-sentence loop sentence ``i`` runs with its own scalars, in the
        batched path the lists become ``infer``'s per-item vectors (``infer_padded``).  Returns a list of float32 numpy
        waveforms."""
        _lib.check_generator(generator)
        noise_mod.exclusive(seed, noise_w=noise_w, noise_z=noise_z)
        device = self.device
        hop = self.hps.data.hop_length
        if not batched:
            seqs = [torch.as_tensor(s, dtype=torch.long).reshape(-1) for s in id_sequences]
            seeds = [None] * len(seqs) if seed is None else noise_mod.per_item(seed, len(seqs))
            for name, nz in (("noise_w", noise_w), ("noise_z", noise_z)):
                if nz is not None and len(nz) != len(seqs):
                    raise ValueError(f"{name}: one tensor per sentence ({len(seqs)}), got {len(nz)}")
            row = lambda nz, i: None if nz is None else torch.as_tensor(nz[i], dtype=torch.float32)[None]
            # sentence i gets its own scalars: every call below is the scalar launch sequence
            controls = [self.per_sentence("speaker_id", speaker_id, len(seqs), integer=True),
                        self.per_sentence("speed", speed, len(seqs), positive=True),
                        self.per_sentence("noise_scale", noise_scale, len(seqs)),
                        self.per_sentence("noise_scale_w", noise_scale_w, len(seqs))]
            out = []
            for i, s in enumerate(seqs):
                speaker_id, speed, noise_scale, noise_scale_w = (v[i] if many else v for many, v in controls)
                o = self.model.infer(s[None].to(device), torch.LongTensor([s.numel()]).to(device),
                                     sid=torch.LongTensor([speaker_id]).to(device), noise_scale=noise_scale,
                                     noise_scale_w=noise_scale_w, length_scale=1.0 / speed, noise_w=row(noise_w, i),
                                     noise_z=row(noise_z, i), **noise_mod.kw(seeds[i]),
                                     **self._generator_kw(generator))[0]
                out.append(o[0, 0].data.cpu().float().numpy())
            return out
        o, frames = self.infer_padded(id_sequences, speaker_id, speed=speed, noise_scale=noise_scale,
                                      noise_scale_w=noise_scale_w, noise_w=noise_w, noise_z=noise_z, **noise_mod.kw(seed),
                                      **self._generator_kw(generator))
        frames = frames.cpu().tolist()
        o = o[:, 0].data.cpu().float().numpy()
        return [o[i, :frames[i] * hop] for i in range(len(frames))]

    def text_to_ids(self, text, language="English"):
        """The text half of ``tts`` (reference: openvoice/api.py:73-82): sentence pieces, language marks, ``get_text``
        -> one id tensor per sentence."""
        mark = self.language_marks.get(language.lower(), None)
        assert mark is not None, f"language {language} is not supported"
        texts = self.split_sentences_into_pieces(text, mark)
        ids = []
        for t in texts:
            t = re.sub(r"([a-z])([A-Z])", r"\1 \2", t)
            t = f"[{mark}]{t}[{mark}]"
            ids.append(self.get_text(t, self.hps, False))
        return ids

    @wavenet_keyword
    def tts(self, text, output_path, speaker, language="English", speed=1.0, batched=False, *, seed=None,
            generator="fp32"):
        """reference: openvoice/api.py:73-98.  ``seed``: as for ``tts_from_ids`` (sentence ``i`` on stream ``(seed,
        i)``); ``generator``: ``"fp32"`` (default) or ``"bf16"``, as for ``tts_from_ids``."""
        _lib.check_generator(generator)
        ids = self.text_to_ids(text, language)
        audio_list = self.tts_from_ids(ids, self.hps.speakers[speaker], speed=speed, batched=batched,
                                       **noise_mod.kw(seed), **self._generator_kw(generator))
        audio = self.audio_numpy_concat(audio_list, sr=self.hps.data.sampling_rate, speed=speed)
        if output_path is None:
            return audio
        audio_io.write(output_path, audio, self.hps.data.sampling_rate)

    # ---- streaming synthesis (tts_live.py) ---------------------------------------------------------------------------
    def tts_live_pool(self, chunk_frames=60, max_streams_per_launch=32, generator="fp32", *, wavenet=None,
                      lookahead_frames=None):
        """A ``tts_live.TtsLivePool``: many sentences synthesised as streams in shared launches -- ``open(ids,
        speaker_id, speed=1.0, noise_scale=0.667, noise_scale_w=0.6, sdp_ratio=0.2, seed=None)`` -> handle, ``step()``
        -> ``{handle: new samples}``.  Each sentence equals its solo ``infer`` with the same ``(seed, stream)`` pair and
        controls.  ``chunk_frames``: a positive multiple of 15; ``generator`` / ``wavenet``: as for
        ``ToneColorConverter.live_pool``.  ``lookahead_frames`` is the converter's keyword: anything but None raises
        ``ValueError`` (streaming TTS emits committed samples only)."""
        from . import tts_live
        return tts_live.TtsLivePool(self.model, chunk_frames=chunk_frames, max_streams_per_launch=max_streams_per_launch,
                                    generator=generator, wavenet=wavenet, lookahead_frames=lookahead_frames)

    def tts_stream_from_ids(self, id_sequences, speaker_id, speed=1.0, noise_scale=0.667, noise_scale_w=0.6, *,
                            seed=None, chunk_frames=60, generator="fp32", wavenet=None):
        """``tts_from_ids`` as a Python generator of device tensors: sentence 0's samples chunk by chunk as they leave
        the generator, then ``clone.gap_samples(sr, speed)`` zeros, then sentence 1, and so on.  The first chunk leaves
        after ``first_audio_frames`` (60 at the default chunk) of the sentence's frames have been through the flow,
        not after the whole utterance.  Concatenated, the output is ``audio_numpy_concat`` of the per-sentence
        (``batched=False``) ``tts_from_ids(..., seed=seed)`` outputs: sentence ``i`` runs on stream ``k + i`` of ``seed``
        (``noise.per_item``; None: one seed drawn from torch's generator) -- bit for bit with direct kernels, within
        1e-4 with the default ones.  ``chunk_frames`` / ``generator`` / ``wavenet``: as for ``tts_live_pool``."""
        from . import tts_live
        pool = tts_live.TtsLivePool(self.model, chunk_frames=chunk_frames, max_streams_per_launch=2,
                                    generator=generator, wavenet=wavenet)
        return tts_live.stream_sentences(pool, id_sequences, int(speaker_id), speed, noise_scale, noise_scale_w, seed,
                                         self.hps.data.sampling_rate)

    def tts_stream(self, text, speaker, language="English", speed=1.0, **kwargs):
        """``tts_stream_from_ids`` of a text (``text_to_ids``: the text half of ``tts``)."""
        return self.tts_stream_from_ids(self.text_to_ids(text, language), self.hps.speakers[speaker], speed=speed,
                                        **kwargs)


def intersperse(lst, item):
    """reference: openvoice/commons.py:22-25."""
    result = [item] * (len(lst) * 2 + 1)
    result[1::2] = lst
    return result


def string_to_bits(string, pad_len=8):
    """ASCII -> [pad_len, 8] bit matrix, MSB first, short strings padded with 0b00100000 (space);
    reference: openvoice/utils.py:46-62."""
    codes = np.frombuffer(string.encode("latin-1", "replace")[:pad_len], dtype=np.uint8)
    full = np.full(pad_len, 0x20, dtype=np.uint8)
    full[:len(codes)] = codes
    return np.unpackbits(full[:, None], axis=1).astype(np.int64)


def bits_to_string(bits_array):
    """reference: openvoice/utils.py:65-75."""
    vals = np.packbits(np.asarray(bits_array).astype(np.uint8), axis=1).reshape(-1)
    return "".join(chr(int(v)) for v in vals)


def plan_enrol_chunks(n_pieces, max_pieces_per_launch):
    """The launches of ``extract_se_many``: ``[(start, end), ...]`` covering pieces ``0 .. n_pieces`` in order, each
    chunk at most ``max_pieces_per_launch`` pieces."""
    cap = int(max_pieces_per_launch)
    if cap < 1:
        raise ValueError(f"max_pieces_per_launch must be >= 1, got {max_pieces_per_launch}")
    return [(lo, min(lo + cap, int(n_pieces))) for lo in range(0, int(n_pieces), cap)]


def _flatten_voices(voices):
    """``voices`` (one list of 1-D waveforms per voice) -> ``(pieces per voice, all pieces in the caller's order)``;
    an empty list, a voice without pieces and a piece that is not 1-D or holds no sample are ValueErrors."""
    if isinstance(voices, (str, bytes)) or not hasattr(voices, "__len__") or len(voices) == 0:
        raise ValueError("extract_se_many: voices must be a non-empty list with one list of waveforms per voice")
    counts, flat = [], []
    for v, pieces in enumerate(voices):
        if isinstance(pieces, (torch.Tensor, np.ndarray)) and pieces.ndim == 1:
            raise ValueError(f"extract_se_many: voice {v} is a waveform, expected a list of waveforms")
        if len(pieces) == 0:
            raise ValueError(f"extract_se_many: voice {v} has no pieces")
        for i, a in enumerate(pieces):
            shape = tuple(a.shape) if hasattr(a, "shape") else (len(a),)
            if len(shape) != 1 or shape[0] == 0:
                raise ValueError(f"extract_se_many: piece {i} of voice {v} must be a non-empty 1-D waveform, "
                                 f"got shape {shape}")
            flat.append(a)
        counts.append(len(pieces))
    return counts, flat


class ToneColorConverter(OpenVoiceBaseClass):
    """reference: openvoice/api.py:101-201."""

    def __init__(self, *args, **kwargs):
        enable_watermark = kwargs.pop("enable_watermark", True)
        watermark, watermark_key = kwargs.pop("watermark", None), kwargs.pop("watermark_key", 0)
        if watermark not in (None, "native"):
            raise ValueError(f"watermark must be None (the wavmark hook, when installed) or 'native', got {watermark!r}")
        super().__init__(*args, **kwargs)
        self.watermark_model = None
        if enable_watermark and watermark == "native":
            # the project's own keyed mark (openvoice_amd/watermark.py): on the device, NOT wavmark-compatible
            self.watermark_model = watermark_mod.NativeWatermark(key=watermark_key).to(self.device)
        elif enable_watermark:
            try:
                import wavmark   # third-party, not part of the reference tree (requirements.txt:4)
                self.watermark_model = wavmark.load_model().to(self.device)
            except ImportError:
                print("wavmark is not installed: watermarking disabled")
        self.version = getattr(self.hps, "_version_", "v1")
        self.use_graphs = False

    def enable_graphs(self, enable=True):
        """Replay conversions of an already-seen (batch, frames, tau) shape from a captured HIP graph: one
        ``hipGraphLaunch`` instead of ~330 launches through Python.  Pays at small batches (a single file is
        launch-bound in eager mode); each distinct shape costs one capture and keeps its workspace resident
        (the 4 most recent shapes are kept).  Off by default."""
        self.use_graphs = bool(enable)
        return self

    def enable_split_bf16x3(self, enable=True, products=6):
        """Run the generator's MRF stages with C >= 64 on the split-precision kernels (``ConverterEngine.use_split_bf16x3``:
        three bf16 planes per fp32 operand, six plane products, fp32 accumulation -- fp32-level results on the bf16 matrix
        pipe, 1.3x the fp32 path's speed on a batch).  Off by default; call after ``load_ckpt``
        (the engine is rebuilt when the weights change)."""
        self.model.engine().use_split_bf16x3(enable, products=products)
        return self

    # ---- spectrogram helpers ---------------------------------------------------------------------
    def _spec(self, y):
        d = self.hps.data
        return spectrogram_torch(y, d.filter_length, d.sampling_rate, d.hop_length, d.win_length, center=False)

    def extract_se(self, ref_wav_list, se_save_path=None, vad=False):
        """Mean reference-encoder embedding over the given audio files -> ``[1, gin, 1]``
        (reference: openvoice/api.py:114-139, which runs one spectrogram + one ``ref_enc`` call per file).  Here the
        files of equal length -- the ~10 s pieces ``se_extractor.get_se`` cuts a recording into -- are stacked into ONE
        ``[N, samples]`` spectrogram launch pair and ONE ``ref_enc`` launch sequence (the kernels take N); files of
        other lengths keep the per-file path.  The mean runs over files in the caller's order either way.
        ``vad=True`` (opt-in) removes silence from every file first (``extract_se_from_audio``)."""
        if isinstance(ref_wav_list, str):
            ref_wav_list = [ref_wav_list]
        # (decoded on the host, resampled -- where the file's rate differs -- by the device kernel: audio_io.load_to_device)
        audios = [audio_io.load_to_device(f, self.hps.data.sampling_rate, self.device) for f in ref_wav_list]
        gs = self.extract_se_from_audio(audios, vad=vad)
        if se_save_path is not None:
            os.makedirs(os.path.dirname(se_save_path), exist_ok=True)
            torch.save(gs.cpu(), se_save_path)
        return gs

    @torch.no_grad()
    def extract_se_from_audio(self, audios, vad=False):
        """``extract_se`` on decoded float32 waveforms (list of 1-D arrays / tensors at the model's sampling rate).
        ``vad=True`` first removes silence from every item on the device, all items in one set of launches
        (``openvoice_amd.vad.remove_silence_many``, the detector ``se_extractor.get_se`` applies); off by default."""
        if vad:
            from . import vad as vad_mod
            d = self.hps.data
            audios, _ = vad_mod.remove_silence_many(
                [torch.as_tensor(a, dtype=torch.float32).to(self.device) for a in audios], d.sampling_rate, d.hop_length)
            if any(len(a) == 0 for a in audios):
                raise ValueError("extract_se(vad=True): an input holds no frame above the detector's threshold")
        groups = {}
        for i, a in enumerate(audios):
            groups.setdefault(len(a), []).append(i)
        embs = [None] * len(audios)
        self.last_extract_se_batches = []          # (files in the ref_enc call) per call, for tests / logs
        for length, idx in groups.items():
            y = torch.stack([torch.as_tensor(audios[i], dtype=torch.float32) for i in idx]).to(self.device)
            spec = self._spec(y)                                             # [n, 513, T], one launch pair
            g = self.model.ref_enc(spec.transpose(1, 2))                     # [n, gin], one launch sequence
            self.last_extract_se_batches.append(len(idx))
            for row, i in enumerate(idx):
                embs[i] = g[row]
        return torch.stack(embs).mean(0).reshape(1, -1, 1).detach()

    def _spec_ragged(self, pieces):
        """Spectrograms of 1-D device waveforms of DIFFERENT lengths in one launch pair: ``(spec [P, bins, Tw],
        frames)`` with ``Tw`` the longest item's frame count and ``frames[p]`` item p's own.  The pieces go into one
        pool and ``_NativeSpectrogram.windows_multi`` frames span p as its own waveform (reflect padding at its two
        ends, record ``(base, n_samples, 0)``), so columns ``[0, frames[p])`` of row p are the item's own spectrogram;
        the columns beyond hold the span's reflected end followed by zeros -- defined values that the ragged
        ReferenceEncoder never reads."""
        from .mel_processing import native_spectrogram
        d = self.hps.data
        eng = native_spectrogram(self.device, d.filter_length, d.hop_length)
        pad = (d.filter_length - d.hop_length) // 2
        lens = [int(p.numel()) for p in pieces]
        if min(lens) <= pad:
            raise ValueError("waveform shorter than the reflect padding")       # as spectrogram_torch raises
        frames = [(n + 2 * pad - d.filter_length) // d.hop_length + 1 for n in lens]
        bases = [0]
        for n in lens[:-1]:
            bases.append(bases[-1] + n)
        # one launch; the framing kernel reads the pool with scalar loads, so the bases need no alignment
        pool = torch.cat(pieces) if len(pieces) > 1 else pieces[0].contiguous()
        records = torch.tensor([[b, n, 0] for b, n in zip(bases, lens)], dtype=torch.int64).to(self.device)
        return eng.windows_multi(pool, records, max(frames)), frames

    @torch.no_grad()
    def extract_se_many(self, voices, vad=False, max_pieces_per_launch=64, return_pieces=False):
        """Enrol many voices at once: ``voices`` is a list with one entry per voice, each a list of 1-D float32
        waveforms (arrays / tensors at the model's sampling rate, of ANY lengths) -> ``[V, gin, 1]``, row v the mean
        reference-encoder embedding over voice v's pieces, i.e. what ``extract_se_from_audio(voices[v])`` returns
        (pieces: the same launch-for-launch arithmetic per item; means: a sequential fp32 sum in piece order divided
        by the count, so they agree within summation order).  All pieces of all voices, in the caller's order, are cut
        into chunks of at most ``max_pieces_per_launch``; a chunk is ONE ragged spectrogram launch pair and ONE
        ``reference_encoder_ragged`` launch sequence, whatever the pieces' lengths.  The result does not depend on the
        cap (64 bounds the first conv's output, about 14 MB per 10 s piece).  ``vad=True`` removes silence from every
        piece first, all voices in one ``remove_silence_many`` call.  ``return_pieces=True`` also returns the
        ``[P, gin]`` piece embeddings.  ``last_extract_se_batches`` holds the chunk sizes afterwards."""
        counts, flat = _flatten_voices(voices)
        plan = plan_enrol_chunks(len(flat), max_pieces_per_launch)
        pieces = [torch.as_tensor(a, dtype=torch.float32).to(self.device).reshape(-1) for a in flat]
        if vad:
            from . import vad as vad_mod
            d = self.hps.data
            pieces, _ = vad_mod.remove_silence_many(pieces, d.sampling_rate, d.hop_length)
            if any(len(a) == 0 for a in pieces):
                raise ValueError("extract_se(vad=True): an input holds no frame above the detector's threshold")
        engine = self.model.engine()
        self.last_extract_se_batches = []
        embs = []
        for lo, hi in plan:
            spec, frames = self._spec_ragged(pieces[lo:hi])                  # [n, 513, Tw], one launch pair
            embs.append(engine.ref_enc.reference_encoder_ragged(spec, frames))  # [n, gin], one launch sequence
            self.last_extract_se_batches.append(hi - lo)
        g = torch.cat(embs) if len(embs) > 1 else embs[0]
        # per-voice mean: row P of gz is zero, and a voice with fewer pieces than the longest adds it (x + 0 = x)
        P, width = len(flat), max(counts)
        gz = torch.cat([g, torch.zeros(1, g.shape[1], dtype=g.dtype, device=g.device)])
        idx, first = [], 0
        for n in counts:
            idx.append(list(range(first, first + n)) + [P] * (width - n))
            first += n
        idx = torch.tensor(idx, dtype=torch.int64).to(g.device)              # [V, width], one copy
        acc = gz[idx[:, 0]]
        for j in range(1, width):
            acc = acc + gz[idx[:, j]]
        se = (acc / torch.tensor(counts, dtype=torch.float32).to(g.device)[:, None]).unsqueeze(-1).detach()
        return (se, g.detach()) if return_pieces else se

    def _wavenet_cores(self):
        return self.model._wavenet_cores()

    @wavenet_keyword
    @torch.no_grad()
    def convert_batch(self, waveforms, src_se, tgt_se, tau=0.3, noise=None, *, seed=None, speed=None):
        """Batched conversion, everything on the device.

        ``waveforms``: float32 tensor ``[B, N]`` (equal lengths), or a list of 1-D tensors/arrays of
        different lengths (each gets its own spectrogram, exactly as a per-file ``convert`` would,
        then the batch is zero-padded in frames and masked by ``spec_lengths``).  Returns
        ``(o_hat [B, 1, hop*T_max] on the device, lengths_in_samples [B])``.  Note the reference
        decoder is unmasked, so for ragged batches samples within ~13 frames of an utterance's end
        differ from a per-utterance run (hard part 6); trim with the returned
        lengths.  ``seed`` (instead of ``noise``): counter-based noise (``openvoice_amd.noise``) -- an int ``s`` gives
        item ``b`` the stream ``(s, b)``, a list holds one seed or ``(seed, stream)`` pair per item; item ``b`` then
        draws ``noise.normal((s, b), 192, 0, T)``, whatever the batch it is in.  ``tau``: one number, or one value per
        waveform (a sequence, or a 1-D float32 device tensor; ``engine.item_tau``): item ``b`` is then converted with
        ``tau[b]`` in the same launches, bit for bit what the batch gives with that number for all (a per-item ``tau``
        runs eagerly: captured graphs are keyed on one ``tau``).  ``speed`` (keyword only; None: all of the above, launch
        for launch): one number in ``[0.5, 2.0]`` or one per waveform -- item ``b`` comes out ``speed[b]`` times faster at
        unchanged pitch: its masked latent is resampled along time on the device in front of the generator
        (``openvoice_amd/stretch.py``, the project's own definition; ``ov_stretch_rows_f32``), which then makes
        ``T_out[b] = stretch.t_out(T[b], step)`` frames.  The returned lengths are ``T_out * hop``, the padded tail is
        zero; ``tau``, ``seed`` and ``noise`` act before the stretch; a stretched call runs eagerly.  ``speed=1.0`` is
        the identity and launches nothing.  ValueError outside the range.  The one-pass launch limit
        (``longform.one_pass_limit_frames``, 63 551 frames) holds for ``T_out`` as it does for ``T``: slowed down, a
        waveform of half that length already reaches it (``OvError`` from the generator's launchers); ``convert`` routes
        on ``max(T, T_out)`` and hands such a file to ``convert_long``."""
        noise_mod.exclusive(seed, noise=noise)
        tau = item_tau(len(waveforms), tau)
        hop = self.hps.data.hop_length
        ragged = isinstance(waveforms, (list, tuple))
        if ragged:
            specs = [self._spec(torch.as_tensor(w, dtype=torch.float32).to(self.device).reshape(1, -1))[0]
                     for w in waveforms]
            frames = [s.shape[1] for s in specs]
            spec = torch.zeros(len(specs), specs[0].shape[0], max(frames), dtype=torch.float32, device=self.device)
            for i, s in enumerate(specs):
                spec[i, :, :s.shape[1]] = s
            spec_lengths = torch.tensor(frames, dtype=torch.int64, device=self.device)
        else:
            y = torch.as_tensor(waveforms, dtype=torch.float32).to(self.device)
            spec = self._spec(y)
            spec_lengths = torch.full((spec.shape[0],), spec.shape[2], dtype=torch.int64, device=self.device)
        if seed is not None:
            seed = noise_mod.per_item(seed, spec.shape[0])
        frames = frames if ragged else [spec.shape[2]] * spec.shape[0]
        steps = stretch_mod.resolve_items(speed, None, frames, hop, self.hps.data.sampling_rate)
        if steps is not None and any(s != stretch_mod.ONE for s in steps):
            o_hat = self.model.voice_conversion(spec, torch.tensor(frames, dtype=torch.int64), sid_src=src_se,
                                                sid_tgt=tgt_se, tau=tau, noise=noise, stretch=steps,
                                                **noise_mod.kw(seed))[0]
            out_frames = [stretch_mod.t_out(T, s) for T, s in zip(frames, steps)]
            return o_hat, torch.tensor(out_frames, dtype=torch.int64).to(self.device) * hop
        if self.use_graphs:
            # the graph's outputs are static buffers: hand the caller its own copy
            o_hat = self.model.voice_conversion(spec, spec_lengths, sid_src=src_se, sid_tgt=tgt_se, tau=tau,
                                                noise=noise, graph=True, skip_padding=ragged,
                                                **noise_mod.kw(seed))[0].clone()
        else:
            # ragged batch: the generator skips what lies beyond length + margin (16-20) frames of each utterance (the
            # samples within the returned lengths are bit-identical to the full computation; the padded tail is zero)
            o_hat = self.model.voice_conversion(spec, spec_lengths, sid_src=src_se, sid_tgt=tgt_se, tau=tau,
                                                noise=noise, skip_padding=ragged, **noise_mod.kw(seed))[0]
        return o_hat, spec_lengths * hop

    @torch.no_grad()
    def convert_batch_sharded(self, waveforms, src_se, tgt_se, tau=0.3, noise=None, gather=True):
        """``convert_batch`` across the GPUs of one node: call it from every rank of an
        initialised ``torch.distributed`` process group (backend "nccl" = RCCL; one process per GPU, this converter on
        the rank's own device) with the same ``waveforms`` -- a ``[N, samples]`` tensor, or a list of N waveforms of
        different lengths.  Rank 0's speaker embeddings are broadcast (2 KiB, the only collective on the path; other
        ranks may pass None), rank r converts utterances ``parallel.shard_range(N, r, world)``, and with ``gather``
        every rank receives the whole ``[N, 1, hop*T_max]`` batch (one all-gather), else ``(local_o_hat, (start,
        end))``.  ``noise`` [N, 192, T] is per utterance, so the result does not depend on the number of ranks.  For a
        list the return value is ``(o_hat, lengths_in_samples [N])`` as from ``convert_batch`` (every rank knows every
        length, so the padded width is agreed on without a collective).  ``tau``: one number, or one value per
        utterance of the WHOLE batch, the same on every rank; rank r converts its utterances with its slice
        (``parallel.convert_sharded(tau=...)``).  Without a process group this is ``convert_batch``."""
        from . import parallel
        gin = self.model.model_cfg["gin_channels"]
        d = self.hps.data
        hop = d.hop_length
        frames_of = lambda n: (int(n) + (d.filter_length - hop) // 2 * 2 - d.filter_length) // hop + 1
        ragged = isinstance(waveforms, (list, tuple))
        if ragged:
            frames = [frames_of(len(w)) for w in waveforms]
            items = list(waveforms)
        else:
            items = torch.as_tensor(waveforms, dtype=torch.float32)
            frames = [frames_of(items.shape[1])] * len(items)
        width = max(frames) * hop                        # samples of the padded batch, the same on every rank

        tau = item_tau(len(items), tau)

        def convert(shard, s, t, nz, tau):
            if len(shard) == 0:         # more ranks than utterances: an empty shard of the agreed width
                return torch.zeros(0, 1, width, dtype=torch.float32, device=self.device)
            # (nz arrives cut to the shard's own longest length: parallel.convert_sharded(frames=...))
            o = self.convert_batch(shard, s, t, tau=tau, noise=nz)[0]
            if o.shape[2] < width:      # a shard whose longest utterance is shorter than the batch's
                o = torch.nn.functional.pad(o, (0, width - o.shape[2]))
            return o
        out = parallel.convert_sharded(convert, items, src_se, tgt_se, gin, self.device, noise=noise, gather=gather,
                                       frames=frames, tau=tau)
        if ragged and gather:
            return out, torch.tensor(frames, dtype=torch.int64, device=self.device) * hop
        return out

    @wavenet_keyword
    def convert(self, audio_src_path, src_se, tgt_se, output_path=None, tau=0.3, message="default", *, seed=None,
                message_repeat=False, speed=None, duration=None):
        """reference: openvoice/api.py:141-160.  A file at or beyond the one-pass launch limit
        (``longform.one_pass_limit_frames``: 63 551 frames = 12.3 min for the released configuration), which one pass
        cannot convert, goes through ``convert_long`` with its defaults; every shorter file is converted in one pass.
        ``seed``: counter-based noise of stream ``(seed, 0)`` (or of a pair), the same whichever of the two paths
        runs.  ``message_repeat`` (native watermark only): every carrier window of the file carries group ``n % G`` of
        the message, not the first ``G`` alone (``NativeWatermark.mark_many``).  ``speed`` (a number in ``[0.5, 2.0]``) or
        ``duration`` (seconds; the speed is then ``T * hop / (duration * sr)``, same range) -- one of them, ValueError for
        both -- change the length of the result at unchanged pitch (``convert_batch``); they go with an over-length file
        to ``convert_long``.  The watermark is made on the stretched waveform."""
        if seed is not None:
            seed = noise_mod.check_seed(seed)
        self._check_repeat(message_repeat)
        if speed is not None and duration is not None:
            stretch_mod.resolve(speed, duration)
        hps = self.hps
        y = audio_io.load_to_device(audio_src_path, hps.data.sampling_rate, self.device)
        d = hps.data
        T = longform.frames_of(y.numel(), d.filter_length, d.hop_length)
        step = stretch_mod.resolve(speed, duration, T, d.hop_length, d.sampling_rate) if T >= 1 else None
        # the generator runs on T_out frames: a file slowed down past the one-pass limit goes to the windows too
        longest = T if step is None else max(T, stretch_mod.t_out(T, step))
        if longest >= longform.one_pass_limit_frames(self.model.model_cfg):
            return self.convert_long(y, src_se, tgt_se, output_path=output_path, tau=tau, message=message,
                                     message_repeat=message_repeat, **noise_mod.kw(seed),
                                     **stretch_mod.kw(speed=speed, duration=duration))
        o_hat, n = self.convert_batch(y.unsqueeze(0), src_se, tgt_se, tau=tau,
                                      **noise_mod.kw(None if seed is None else [seed]),
                                      **stretch_mod.kw(speed=None if step is None else step / stretch_mod.ONE))
        if step is not None:
            o_hat = o_hat[:, :, :int(n[0])]
        if self._native_watermark():         # marked on the device, before the copy to the host
            self.watermark_model.mark_many([o_hat[0, 0].data], message, message_repeat=message_repeat)
        audio = o_hat[0, 0].data.cpu().float().numpy()
        if not self._native_watermark():
            audio = self.add_watermark(audio, message)
        if output_path is None:
            return audio
        audio_io.write(output_path, audio, hps.data.sampling_rate)

    # ---- recordings of any length (openvoice_amd/longform.py) -----------------------------------------------------------
    def _windowed(self, window_frames, windows_per_launch=1, wavenet=None):
        d = self.hps.data
        return longform.WindowedConverter(self.model, n_fft=d.filter_length, hop=d.hop_length, window_frames=window_frames,
                                          windows_per_launch=windows_per_launch, graph=self.use_graphs,
                                          model_sr=d.sampling_rate, wavenet=wavenet,
                                          watermark_model=self.watermark_model)

    def _to_model_rate(self, audio_or_path, sr):
        """(device waveform at the model rate, its rate before resampling or None): a path is decoded and resampled on
        load as always; an array at ``sr`` Hz (None: the model rate) is resampled on the device."""
        msr = self.hps.data.sampling_rate
        if isinstance(audio_or_path, (str, os.PathLike)):
            return audio_io.load_to_device(audio_or_path, msr, self.device)
        y = torch.as_tensor(audio_or_path, dtype=torch.float32).reshape(-1).to(self.device)
        return y if sr is None or int(sr) == int(msr) else audio_io.resample_on_device(y, sr, msr)

    def _native_watermark(self):
        """True when the hook's model is the project's own (``watermark="native"``): the outputs are then marked on the
        device by ``NativeWatermark.mark_many``, one launch per call, instead of the host loop of ``add_watermark``."""
        return isinstance(self.watermark_model, watermark_mod.NativeWatermark)

    def _check_repeat(self, message_repeat):
        """``message_repeat=True`` on a file needs the native watermark (the wavmark hook marks the leading windows
        only); ValueError otherwise, at the call."""
        if message_repeat and not self._native_watermark():
            raise ValueError('message_repeat=True needs the native watermark: ToneColorConverter(..., watermark="native")')

    def _finish_many(self, outs, message, out_srs, message_repeat=False):
        """``_finish`` of many converted waveforms: without a model, or with the native one (which marks every carrier
        window of every item in ONE launch first), the rate conversion is one launch for all items; any other model
        keeps the per-item host loop."""
        msr = self.hps.data.sampling_rate
        if self.watermark_model is not None and not self._native_watermark():
            return [self._finish(o, message, r) for o, r in zip(outs, out_srs)]
        if self._native_watermark():
            self.watermark_model.mark_many(outs, message, message_repeat=message_repeat)
        outs = rates.resample_many(outs, [(msr, r) for r in out_srs], self.device)
        return [o.cpu().numpy() for o in outs]

    def _finish(self, o, message, out_sr, message_repeat=False):
        """Converted device waveform at the model rate -> host audio at ``out_sr`` (None: the model rate).  The watermark
        hook runs at the model rate, before the rate conversion."""
        msr = self.hps.data.sampling_rate
        resample = out_sr is not None and int(out_sr) != int(msr)
        if self._native_watermark():
            self.watermark_model.mark_many([o], message, message_repeat=message_repeat)
        if self.watermark_model is None or self._native_watermark():
            return (audio_io.resample_on_device(o, msr, out_sr) if resample else o).cpu().numpy()
        audio = self.add_watermark(o.cpu().numpy(), message)
        if resample:
            audio = audio_io.resample_on_device(torch.from_numpy(audio).to(self.device), msr, out_sr).cpu().numpy()
        return audio

    @wavenet_keyword
    def convert_long(self, audio_or_path, src_se, tgt_se, output_path=None, tau=0.3, message="default",
                     window_frames=longform.DEFAULT_WINDOW_FRAMES, windows_per_launch=longform.DEFAULT_WINDOWS_PER_LAUNCH,
                     noise=None, sr=None, out_sr=None, *, seed=None, message_repeat=False, speed=None, duration=None):
        """``convert`` for a recording of any length: overlapping windows of ``window_frames`` frames, up to
        ``windows_per_launch`` of them per launch (``longform.WindowedConverter``); device memory is bounded by the window,
        not by the file.  ``audio_or_path``: a file path, or a 1-D float32 waveform (host or device) at ``sr`` Hz (None:
        the model rate; otherwise resampled on the device first).  ``noise``: ``[1, 192, >= T]`` or None -- then
        ``torch.randn(1, 192, T)`` on the device, the draw of a seeded one-pass ``convert``; T counts frames at the model
        rate; or ``seed`` (an int: stream ``(seed, 0)``, or a pair): counter-based noise, each window generating its own
        frames, the same values as a one-pass ``convert(seed=...)``, a ``stream`` or a ``live_stream`` with that seed
        draws.  ``out_sr``: the rate of the returned / written audio (None: the model rate).  Otherwise the same return
        value / file output as ``convert``.  ``message_repeat``: as for ``convert``.  ``speed`` / ``duration``: as for
        ``convert`` (``duration`` is that of the result at the model rate's clock, whatever ``out_sr``); the windows are
        cut on source frames as always, each stretched with its global position, so the result is the one-pass
        ``convert_batch(speed=...)`` of the recording within the windows' contract
        (``WindowedConverter.convert``).  The watermark and ``out_sr`` act on the stretched waveform."""
        noise_mod.exclusive(seed, noise=noise)
        self._check_repeat(message_repeat)
        if speed is not None and duration is not None:
            stretch_mod.resolve(speed, duration)
        sr, out_sr = rates.check_rate(sr, "sr"), rates.check_rate(out_sr, "out_sr")
        y = self._to_model_rate(audio_or_path, sr)
        d = self.hps.data
        step = stretch_mod.resolve(speed, duration, longform.frames_of(y.numel(), d.filter_length, d.hop_length),
                                   d.hop_length, d.sampling_rate)
        o = self._windowed(window_frames, windows_per_launch).convert(y, src_se, tgt_se, tau=tau, noise=noise,
                                                                      **noise_mod.kw(seed), **stretch_mod.kw(step=step))
        audio = self._finish(o, message, out_sr, message_repeat)
        if output_path is None:
            return audio
        audio_io.write(output_path, audio, self.hps.data.sampling_rate if out_sr is None else out_sr)

    def stream(self, src_se, tgt_se, tau=0.3, window_frames=longform.DEFAULT_STREAM_WINDOW_FRAMES, noise=None, sr_in=None,
               sr_out=None, *, seed=None, wavenet=None, message=None, watermark_hold=watermark_mod.DEFAULT_HOLD,
               message_repeat=False, speed=None, duration=None):
        """A ``longform.ConversionStream``: ``push(samples)`` -> newly finished converted samples (device tensor, maybe
        empty), ``close()`` -> the rest, ``latency_samples`` = ``(window_frames - 1) * hop + n_fft - (n_fft - hop) / 2``
        at the model rate.  ``sr_in`` / ``sr_out``: the rate of the pushes / of the output (None: the model rate); the
        stream resamples inside, carrying the filter state across pushes, and ``latency_samples`` (output samples) /
        ``latency_seconds`` then include the resamplers' waits.  ``noise`` ``[1, 192, >= T]`` makes it reproducible,
        and so does
        ``seed`` (stream ``(seed, 0)``, or a pair), which needs no length and keeps no noise tensor.  The
        output equals ``convert_long(..., windows_per_launch=1)`` of the whole input, bit for bit -- with rates, of the
        input resampled to the model rate, and resampled to ``sr_out`` after (``audio_io.resample_on_device``).

        ``message`` (keyword only; None: the stream is not marked, all of the above unchanged): with
        ``watermark="native"`` the output carries the block-wise form of the native watermark (``watermark.py``,
        "streams"), made at the model rate before the output resampler and read by ``detect_watermark``.
        ``watermark_hold`` = H, one of 16000, 8000, 4000, 3200, 1600, 800, 640: a sample leaves once its block of H
        samples is whole, at most H - 1 samples later than unmarked (``latency_samples`` says so); at 16000 the output
        is the unmarked stream's passed through ``mark_many``, bit for bit; a shorter hold costs signal-to-mark ratio
        (DESIGN.md section 27).  ``message_repeat``: window n carries group n % G for the stream's life, instead of the
        first G windows only.  The samples of a block unfinished at ``close()`` leave unmarked.  ValueError, at the
        call, for a message without the native watermark and for a hold outside the list.  ``speed`` / ``duration``:
        ValueError -- streams are not stretched (``stretch.reject_stream``)."""
        stretch_mod.reject_stream("stream", speed, duration)
        return self._windowed(window_frames, 1, wavenet).stream(src_se, tgt_se, tau=tau, noise=noise, sr_in=sr_in, sr_out=sr_out,
                                                       message=message, watermark_hold=watermark_hold,
                                                       message_repeat=message_repeat, **noise_mod.kw(seed))

    # ---- many streams and recordings in shared launches -------------------------------------------------------------
    def stream_pool(self, tau=0.3, window_frames=longform.DEFAULT_STREAM_WINDOW_FRAMES,
                    max_windows_per_launch=longform.DEFAULT_POOL_WINDOWS_PER_LAUNCH, *, wavenet=None, speed=None,
                    duration=None):
        """A ``longform.StreamPool``: many live streams (``open(src_se, tgt_se, noise=None, sr_in=None, sr_out=None,
        seed=None, tau=None, message=None, watermark_hold=16000, message_repeat=False)`` ->
        handle, ``push(h, samples)``, ``close(h)``), whose ready windows one ``step()`` converts together, up to
        ``max_windows_per_launch`` per launch -> ``{handle: newly finished samples}``; streams at rates of their own are
        resampled in one launch per direction and step.  Each stream's output equals a ``stream(...)`` fed the same
        samples with the same noise and rates.  ``tau`` is the pool's default: ``open(..., tau=None)`` gives a stream its
        own for life, and windows of streams with different ``tau`` still share launches (one value per launch row).
        ``speed`` / ``duration``: ValueError -- streams are not stretched."""
        stretch_mod.reject_stream("stream_pool", speed, duration)
        return self._windowed(window_frames, 1, wavenet).stream_pool(tau=tau, max_windows_per_launch=max_windows_per_launch)

    # ---- low-latency live streams ------------------------------------------------------------------------------------
    def live_stream(self, src_se, tgt_se, tau=0.3, chunk_frames=15, noise=None, sr_in=None, sr_out=None,
                    generator="fp32", *, seed=None, wavenet=None, lookahead_frames=None, crossfade_samples=None,
                    message=None, watermark_hold=watermark_mod.DEFAULT_HOLD, message_repeat=False, speed=None,
                    duration=None):
        """A ``live.LiveStream``: the conversion as a cascade of units that carry their recent input as state.
        ``push(samples)`` -> newly finished samples, ``close()`` -> the rest, ``latency_samples`` =
        ``live.live_latency_samples`` (1.45 s at 15 frames).  ``chunk_frames``: a positive multiple of 15 (the Winograd
        grid).  ``generator``: ``"fp32"`` (default) or ``"bf16"`` -- the kernels of the generator units of THIS stream
        (same latency and state); ``wavenet`` (keyword only): None follows ``use_bf16_wavenet``, ``"fp32"`` / ``"bf16"``
        choose the WaveNet layers' kernels of the posterior-encoder and flow units of THIS stream; the engine-wide switches stay off (ValueError
        with use_bf16_generator / enable_split_bf16x3).  Never graph-captured.
        ``sr_in`` / ``sr_out``: the rate of the pushes / of the output (None: the model rate); ``latency_samples`` (in
        output samples) and ``latency_seconds`` then include the resamplers' waits (``rates.stream_latency``).  With
        ``noise`` ``[1, 192, >= T]`` the output equals ``convert_long`` of the whole input (resampled to the model rate
        before and to ``sr_out`` after by ``audio_io.resample_on_device``), with ``generator="bf16"`` the one made with
        ``use_bf16_generator``.  ``seed`` (an int: stream ``(seed, 0)``, or a pair) does the same without a length: the
        noise of frames ``[f0, f0 + n)`` is generated when the chunk is fed, so the output does not depend on the push
        sizes, equals ``convert_long(seed=...)``, and no noise tensor is held however long the call lasts.

        ``lookahead_frames`` (keyword only; None: all of the above, unchanged): an integer A >= 0 makes the stream emit
        ``[0, hop * max(0, F - A))`` once it has taken F interior frames, instead of waiting for every sample's whole
        receptive field (1.26 s): ``latency_samples`` becomes ``hop * (A + chunk_frames) + (n_fft - hop) / 2`` (0.19 s
        at A = 0).  The piece a round emits is that piece of the one-pass conversion of the first F frames -- the input
        so far, as if it ended there (same embeddings, ``tau`` and ``seed`` / ``noise``) -- not of the whole input;
        samples whose receptive field had arrived are the same in both.  ``close()`` returns the rest from the exact
        path.  With ``hop * A >= live.live_right_samples`` (A >= 109) nothing is approximated and nothing extra is
        launched.  ``crossfade_samples`` = X: the first X samples of a piece are blended with what the previous round's
        preview held for them (raised-cosine fade-in, ``ov_crossfade_rows_f32``); ``0 <= X <= min(hop * A, hop *
        chunk_frames)``, default ``min(hop, hop * A)`` -- a default nobody has measured on a real voice.  X = 0 keeps
        the contract above bit for bit.

        ``message`` / ``watermark_hold`` / ``message_repeat`` (keyword only): as for ``stream`` -- the block-wise native
        watermark of what the stream emits (emitted samples are final; the crossfade runs before the mark), at most
        ``watermark_hold - 1`` samples later, which ``latency_samples`` includes.  ``speed`` / ``duration``: ValueError --
        streams are not stretched."""
        stretch_mod.reject_stream("live_stream", speed, duration)
        from . import live
        d = self.hps.data
        return live.LiveStream(self.model, src_se, tgt_se, tau=tau, chunk_frames=chunk_frames, noise=noise,
                               n_fft=d.filter_length, hop=d.hop_length, sr_in=sr_in, sr_out=sr_out,
                               model_sr=d.sampling_rate, generator=generator, wavenet=wavenet,
                               lookahead_frames=lookahead_frames, crossfade_samples=crossfade_samples,
                               watermark_model=self.watermark_model, message=message, watermark_hold=watermark_hold,
                               message_repeat=message_repeat, **noise_mod.kw(seed))

    def live_pool(self, tau=0.3, chunk_frames=15, max_streams_per_launch=32, generator="fp32", *, wavenet=None,
                  lookahead_frames=None, crossfade_samples=None, speed=None, duration=None):
        """A ``live.LivePool``: many live streams (``open(src_se, tgt_se, noise=None, sr_in=None, sr_out=None,
        seed=None, tau=None, message=None, watermark_hold=16000, message_repeat=False)`` /
        ``push`` / ``close``), every stream with a ready chunk converted by one ``step()`` in launches of up to
        ``max_streams_per_launch`` rows per unit; streams at rates of their own are resampled in one launch per direction
        and step.  Each stream equals its solo ``live_stream``.  ``tau`` is the pool's default: ``open(..., tau=None)``
        gives a stream its own for life, and streams with different ``tau`` share the pool's launches (one value per
        launch row).  One ``generator`` (``"fp32"`` or
        ``"bf16"``) for the pool; pools of both kinds may be open on one converter at once.  ``wavenet`` (keyword only):
        the WaveNet layers' kernels of the pool's posterior-encoder and flow units, None (follow ``use_bf16_wavenet``),
        ``"fp32"`` or ``"bf16"``.  ``lookahead_frames`` / ``crossfade_samples`` (keyword only, pool-wide like
        ``chunk_frames``): as for ``live_stream``; the streams' previews share launches like their committed rounds.
        ``speed`` / ``duration``: ValueError -- streams are not stretched."""
        stretch_mod.reject_stream("live_pool", speed, duration)
        from . import live
        d = self.hps.data
        return live.LivePool(self.model, tau=tau, chunk_frames=chunk_frames, max_streams_per_launch=max_streams_per_launch,
                             n_fft=d.filter_length, hop=d.hop_length, model_sr=d.sampling_rate, generator=generator,
                             wavenet=wavenet, lookahead_frames=lookahead_frames, crossfade_samples=crossfade_samples,
                             watermark_model=self.watermark_model)

    @wavenet_keyword
    def convert_many(self, items, src_se, tgt_se, tau=0.3, window_frames=longform.DEFAULT_WINDOW_FRAMES,
                     windows_per_launch=longform.DEFAULT_MANY_WINDOWS_PER_LAUNCH, noise=None, output_paths=None,
                     message="default", sr=None, out_sr=None, *, seed=None, generator=None, message_repeat=False,
                     speed=None, duration=None):
        """``convert_long`` of many recordings with their windows packed ACROSS recordings into launches of up to
        ``windows_per_launch`` (``longform.WindowedConverter.convert_many``).  ``items``: file paths (any rate, decoded
        and resampled like ``convert_long``) or 1-D waveforms at ``sr`` Hz (None: the model rate; one rate, or a list
        with one per item).  ``out_sr``: the rate of the results (None: the model rate; one, or one per item).  The
        array items are resampled to the model rate in ONE launch, and the results to ``out_sr`` in one more
        (``rates.resample_many``).  ``src_se`` / ``tgt_se``: one ``[1, 256, 1]`` for every item, or a list with one per
        item.  ``noise``: None or a list of ``[1, 192, >= T_i]``; ``seed`` (instead): an int ``s``
        gives item ``i`` the stream ``(s, i)``, or a list with one seed / pair per item.  Returns a list of numpy
        arrays (watermark hook applied
        per item, at the model rate), or writes ``output_paths[i]`` (at its ``out_sr``) instead.  Each item equals
        ``convert_long`` of it with the same ``window_frames``, noise and rates.  ``generator`` (keyword only): None
        follows ``use_bf16_generator``, ``"fp32"`` / ``"bf16"`` choose the generator's kernels for this call.  ``tau``:
        one number, or one per item; windows of items with different ``tau`` share launches, and each item still equals
        its ``convert_long`` with its own ``tau``.  ``message_repeat``: as for ``convert``.  ``speed`` / ``duration``
        (keyword only): one value, or a list with one per item (None in a list: that item is left alone); per item one of
        the two, as for ``convert_long``, which each item still equals.  The stretched items' windows share launches
        with each other; the watermark and ``out_sr`` act on the stretched waveforms."""
        _lib.check_generator(generator, optional=True)
        self._check_repeat(message_repeat)
        hps = self.hps
        msr = hps.data.sampling_rate
        items = list(items)
        n = len(items)
        noise_mod.exclusive(seed, noise=noise)
        if seed is not None:
            seed = noise_mod.per_item(seed, n)
        per_item = lambda se: list(se) if isinstance(se, (list, tuple)) else [se] * n
        srcs, tgts = per_item(src_se), per_item(tgt_se)
        srs = [rates.check_rate(r, "sr") for r in per_item(sr)]
        out_srs = [rates.check_rate(r, "out_sr") for r in per_item(out_sr)]
        if output_paths is not None and len(output_paths) != n:
            raise ValueError("convert_many: one output path per item")
        if len(srs) != n or len(out_srs) != n:
            raise ValueError("convert_many: one sr / out_sr per item")
        waves = [audio_io.load_to_device(x, msr, self.device) if isinstance(x, (str, os.PathLike))
                 else torch.as_tensor(x, dtype=torch.float32).reshape(-1).to(self.device) for x in items]
        paths = [isinstance(x, (str, os.PathLike)) for x in items]
        waves = rates.resample_many(waves, [(None, None) if p else (r, msr) for p, r in zip(paths, srs)], self.device)
        d = hps.data
        steps = stretch_mod.resolve_items(speed, duration, [longform.frames_of(w.numel(), d.filter_length, d.hop_length)
                                                            for w in waves], d.hop_length, msr)
        outs = self._windowed(window_frames, windows_per_launch).convert_many(waves, srcs, tgts, tau=tau, noises=noise,
                                                                              **noise_mod.kw(seed, "seeds"),
                                                                              **_lib.generator_kw(generator),
                                                                              **stretch_mod.kw(steps=steps))
        audios = self._finish_many(outs, message, out_srs, message_repeat)
        if output_paths is None:
            return audios
        for path, audio, r in zip(output_paths, audios, out_srs):
            audio_io.write(path, audio, msr if r is None else r)

    # ---- optional watermark hook (third-party model; behaviour of the reference's openvoice/api.py:162-201) ----------
    # The message travels as 32-bit groups, group n in the 16 000-sample window that starts at sample 32 000 n (every other
    # window of the waveform stays untouched); ``watermark_model`` is any object with ``encode(signal [1, 16000], bits
    # [1, 32]) -> signal`` and ``decode(signal [1, 16000]) -> scores [1, 32]`` (wavmark's interface).
    WATERMARK_WINDOW = 16000
    WATERMARK_STRIDE = 2 * WATERMARK_WINDOW
    WATERMARK_GROUP_BITS = 32

    def _watermark_windows(self, audio, count):
        """(n, start, stop) of the first ``count`` carrier windows that lie wholly inside ``audio``; stops at the first
        that does not."""
        for n in range(count):
            start = n * self.WATERMARK_STRIDE
            if start + self.WATERMARK_WINDOW > len(audio):
                return
            yield n, start, start + self.WATERMARK_WINDOW

    def add_watermark(self, audio, message):
        """Embed ``message`` (padded / cut to 8 latin-1 characters) into ``audio`` (1-D float array, modified in place and
        returned).  A waveform too short for all groups carries the leading ones and a notice is printed, as upstream."""
        if self.watermark_model is None:
            return audio
        payload = string_to_bits(message).reshape(-1)
        groups = len(payload) // self.WATERMARK_GROUP_BITS
        done = 0
        with torch.no_grad():
            for n, start, stop in self._watermark_windows(audio, groups):
                carrier = torch.as_tensor(audio[start:stop], dtype=torch.float32, device=self.device).unsqueeze(0)
                bits = torch.as_tensor(payload[n * self.WATERMARK_GROUP_BITS:(n + 1) * self.WATERMARK_GROUP_BITS],
                                       dtype=torch.float32, device=self.device).unsqueeze(0)
                audio[start:stop] = self.watermark_model.encode(carrier, bits).detach().cpu().reshape(-1).numpy()
                done += 1
        if done < groups:
            print("Audio too short, fail to add watermark")
        return audio

    def detect_watermark(self, audio, n_repeat):
        """Read ``n_repeat`` 32-bit groups back (threshold 0.5 on the model's scores) and decode them to characters;
        the string "Fail" when the waveform does not hold that many carrier windows."""
        groups = []
        with torch.no_grad():
            for _, start, stop in self._watermark_windows(audio, n_repeat):
                carrier = torch.as_tensor(audio[start:stop], dtype=torch.float32, device=self.device).unsqueeze(0)
                scores = self.watermark_model.decode(carrier)
                groups.append((scores >= 0.5).to(torch.uint8).detach().cpu().reshape(-1).numpy())
        if len(groups) < n_repeat:
            print("Audio too short, fail to detect watermark")
            return "Fail"
        return bits_to_string(np.stack(groups).reshape(-1, 8))

    def find_watermark(self, audio, message=None, **kw):
        """Find the native watermark wherever it starts: ``audio`` is a file path (decoded and resampled to the model
        rate like ``convert``'s input) or a 1-D float array / tensor AT THE MODEL RATE (audio at another rate is out of
        scope: the chips are counted in model-rate samples).  Every offset is scanned on the device
        (``NativeWatermark.find``, whose keywords ``max_errors``, ``margin``, ``max_false_alarm`` and ``capacity`` pass
        through) and the verdict for the one waveform is returned: ``marked``, ``offset``, ``first_group``, ``message``,
        ``windows``, ``false_alarm``, ``hits``, ``overflow``.  ``message=None`` is the blind mode, a heuristic.  Needs
        ``watermark="native"``: ValueError otherwise.  ``detect_watermark`` is untouched."""
        if not self._native_watermark():
            raise ValueError('find_watermark needs the native watermark: ToneColorConverter(..., watermark="native")')
        if isinstance(audio, (str, os.PathLike)):
            y = audio_io.load_to_device(audio, self.hps.data.sampling_rate, self.device)
        else:
            y = torch.as_tensor(audio, dtype=torch.float32).reshape(-1).to(self.device)
        return self.watermark_model.find([y], message, **kw)[0]
