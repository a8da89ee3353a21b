"""Text (or symbol ids) to audio in a cloned voice without leaving the device, for many requests in shared launches.

OpenVoice is mostly used as one chain (reference demo_part1, the app's ``predict()``): ``BaseSpeakerTTS.tts`` reads the
text in a base voice, ``ToneColorConverter.convert`` gives that audio the target's tone colour.  Between the two the
reference copies every sentence to the host, joins them in numpy (``audio_numpy_concat``, api.py:56-63), writes a WAV,
decodes it again and uploads it.  ``VoiceCloner`` runs the same chain with the join on the device:

1. every sentence of every request goes through ``BaseSpeakerTTS.infer_padded`` (``infer(..., skip_padding=True)``), in
   batches chosen by ``sentence_batches`` -- a pure function of the request list;
2. one ``ov_join_segments_f32`` launch per batch (csrc/clone.hip) writes each sentence and its 50 ms / speed of silence
   to its place in its request's waveform;
3. where the two models' sampling rates differ, one ``rates.resample_many`` launch;
4. ``WindowedConverter.convert_many`` with one embedding pair per request: requests share generator launches and a text
   of any length converts;
5. watermark hook and ``out_sr`` as in ``ToneColorConverter.convert_many``.

Contract: ``speak_ids_many`` equals, bit for bit, the chain made of the public pieces -- per batch of
``sentence_batches`` one ``tts_from_ids(batched=True)`` with the same noise, ``audio_numpy_concat`` per request, then
``ToneColorConverter.convert_many`` with the same window, noise and rates.  Because the generator is unmasked, the last
~13 frames of a sentence depend on whether it is the longest of its batch (``tts_from_ids`` says so), so the result
depends on the batch composition: on the other requests of the call and on ``max_sentences_per_launch``, never on
timing.

``mixed=True`` (off by default) lets requests of different speeds and base speakers share ``infer`` launches:
``sentence_batches`` then makes one pool of all sentences, and each batch is one ``infer_padded`` with a speaker and a
speed per sentence.  The contract reads the same with that call as the public piece.
"""
import numpy as np

from . import _lib, longform, rates
from . import stretch as stretch_mod
from .engine import item_tau, rows_tau, wavenet_keyword

RECORD_FIELDS = 4           # ov_join_segments_f32's record: (src_off, n, dst_off, gap)
MAX_RECORDS = 65535
DEFAULT_SENTENCES_PER_LAUNCH = 32


def gap_samples(sr, speed=1.0):
    """Zeros after every sentence: ``int((sr * 0.05) / speed)`` (reference api.py:62)."""
    return int((sr * 0.05) / speed)


def _per_utterance(gap, n):
    gaps = [int(g) for g in gap] if isinstance(gap, (list, tuple, np.ndarray)) else [int(gap)] * n
    if len(gaps) != n or any(g < 0 for g in gaps):
        raise ValueError("gap: one non-negative number of samples, or one per utterance")
    return gaps


def join_plan(lengths, gap):
    """Where ``audio_numpy_concat`` puts things.  ``lengths[u]``: the sample counts of utterance u's segments in order;
    ``gap``: zeros after EVERY segment, the last included (one int, or one per utterance).  Returns ``(records, totals)``:
    ``records[u][s] = (n, dst_off, gap)`` with ``dst_off`` relative to the utterance's first sample, ``totals[u]`` the
    utterance's length."""
    gaps = _per_utterance(gap, len(lengths))
    records, totals = [], []
    for segs, g in zip(lengths, gaps):
        recs, at = [], 0
        for n in segs:
            n = int(n)
            if n < 0:
                raise ValueError(f"segment length {n}")
            recs.append((n, at, g))
            at += n + g
        records.append(recs)
        totals.append(at)
    return records, totals


def join_segments_host(segments, gap):
    """``join_segments`` restated in float64 numpy: ``segments[u]`` a list of 1-D arrays -> one float64 array per
    utterance, every segment followed by ``gap`` zeros."""
    records, totals = join_plan([[np.asarray(x).reshape(-1).shape[0] for x in segs] for segs in segments], gap)
    outs = []
    for segs, recs, total in zip(segments, records, totals):
        out = np.zeros(total, dtype=np.float64)
        for x, (n, at, _) in zip(segs, recs):
            out[at:at + n] = np.asarray(x, dtype=np.float64).reshape(-1)
        outs.append(out)
    return outs


def _bases(totals):
    """Every utterance starts 16-byte aligned in the packed output: ``(bases, pool length)``."""
    bases, acc = [], 0
    for t in totals:
        bases.append(acc)
        acc += -(-t // 4) * 4
    return bases, acc


def _launch_join(o, records, dst):
    """One ``ov_join_segments_f32`` launch: ``o`` the padded TTS output (any shape, contiguous), ``records`` host rows
    ``(src_off, n, dst_off, gap)``, ``dst`` the packed 1-D output."""
    import torch
    if not records:
        return
    if len(records) > MAX_RECORDS:
        raise ValueError(f"at most {MAX_RECORDS} segments per launch")
    recs = torch.tensor(records, dtype=torch.int64).to(dst.device)                  # one host -> device copy
    _lib.call("ov_join_segments_f32", o, o.numel(), recs, len(records), dst, dst.numel(),
              max(r[1] + r[3] for r in records))


def join_segments(o, lengths, groups, gap):
    """The device form of ``audio_numpy_concat`` for many utterances: ONE launch.

    ``o``: the padded TTS output ``[B, 1, ld]`` (or ``[B, ld]``), float32 on a ROCm device; ``lengths``: the valid
    samples of each row -- a ``[B]`` integer device tensor (then this makes one small device-to-host copy: the counts
    size the output) or a host sequence; ``groups[u]``: the rows of utterance u, in order; ``gap``: zeros after every
    segment (one int, or one per utterance).  Returns one 1-D device waveform per utterance (views of one packed
    tensor), equal to ``audio_numpy_concat`` of the rows' valid samples."""
    import torch
    o = o.detach()
    if o.dtype != torch.float32 or not o.is_contiguous() or o.dim() not in (2, 3) or (o.dim() == 3 and o.shape[1] != 1):
        raise ValueError("o must be a contiguous float32 [B, 1, ld] or [B, ld] tensor")
    B, ld = o.shape[0], o.shape[-1]
    lens = lengths.to(torch.int64).cpu().tolist() if isinstance(lengths, torch.Tensor) else [int(n) for n in lengths]
    if len(lens) != B or any(n < 0 or n > ld for n in lens):
        raise ValueError("lengths: one count in [0, ld] per row of o")
    if any(b < 0 or b >= B for rows in groups for b in rows):
        raise ValueError("groups name a row that o does not have")
    plan, totals = join_plan([[lens[b] for b in rows] for rows in groups], gap)
    bases, total = _bases(totals)
    dst = torch.empty(max(total, 1), dtype=torch.float32, device=o.device)
    records = [(b * ld, n, base + at, g) for rows, recs, base in zip(groups, plan, bases)
               for b, (n, at, g) in zip(rows, recs)]
    _launch_join(o, records, dst)
    return [dst[b:b + t] for b, t in zip(bases, totals)]


def sentence_batches(lengths, keys, max_sentences_per_launch=DEFAULT_SENTENCES_PER_LAUNCH, mixed=False):
    """Which sentences share an ``infer`` launch: a pure function of its arguments.  ``lengths[r]``: the id counts of
    request r's sentences; ``keys[r]``: what a keyed ``infer`` call has a single value of -- ``(speed, speaker id)``,
    the scalar ``speed`` and ``speaker_id`` of ``tts_from_ids``, which the keyed contract is stated against.
    Requests of one key (taken in order of first appearance) pool their sentences, longest first (ties: request, then
    sentence order) so that padding is small, and the pool is cut into batches of at most ``max_sentences_per_launch``.
    ``mixed=True``: one pool for all requests whatever their key (``infer`` with per-item controls), ordered and cut
    the same way; the key of every such batch is None and the caller takes each item's speed and speaker from its
    request.  Returns ``[(key, [(request, sentence), ...]), ...]``; every sentence appears exactly once."""
    m = int(max_sentences_per_launch)
    if m < 1:
        raise ValueError(f"max_sentences_per_launch = {max_sentences_per_launch}")
    if len(lengths) != len(keys):
        raise ValueError("one key per request")
    pools = {}
    for r, (lens, key) in enumerate(zip(lengths, keys)):
        pools.setdefault(None if mixed else key, []).extend((-int(n), r, s) for s, n in enumerate(lens))
    batches = []
    for key, pool in pools.items():
        pool.sort()
        for i0 in range(0, len(pool), m):
            batches.append((key, [(r, s) for _, r, s in pool[i0:i0 + m]]))
    return batches


class _Request:
    __slots__ = ("ids", "speaker", "src_se", "tgt_se", "speed", "out_sr", "tau", "convert_step")


class VoiceCloner:
    """``BaseSpeakerTTS`` + ``ToneColorConverter`` as one device-resident chain (module docstring).  The two models
    must sit on one device; their sampling rates may differ (the joined audio is then resampled on the device)."""

    def __init__(self, tts, converter):
        import torch
        norm = lambda d: (lambda t: (t.type, 0 if t.index is None else t.index))(torch.device(d))
        if norm(tts.device) != norm(converter.device):
            raise ValueError(f"VoiceCloner: the TTS is on {tts.device!r}, the converter on {converter.device!r}; "
                             f"both must be on one device")
        self.tts, self.converter = tts, converter
        self.device = tts.device
        self.tts_sr = int(tts.hps.data.sampling_rate)
        self.hop = int(tts.hps.data.hop_length)
        self.last_batches = None          # sentence_batches of the last call, for tests / logs
        self.last_launches = None         # {"infer": n, "join": n} of the last call

    # ---- requests ----------------------------------------------------------------------------------------------------
    def _speaker_id(self, speaker):
        if isinstance(speaker, str):
            return int(self.tts.hps.speakers[speaker])
        return int(speaker)

    def _parse(self, requests, noise_w, noise_z, noise, output_paths):
        reqs = []
        for i, q in enumerate(requests):
            if isinstance(q, dict):
                q = (q["ids"], q["speaker"], q["src_se"], q["tgt_se"], q.get("speed", 1.0), q.get("out_sr"), q.get("tau"),
                     q.get("convert_speed"))
            if not 4 <= len(q) <= 8:
                raise ValueError(f"request {i}: (id sequences, speaker, src_se, tgt_se[, speed[, out_sr[, tau[, "
                                 f"convert_speed]]]])")
            r = _Request()
            r.ids = [np.asarray(s, dtype=np.int64).reshape(-1) for s in q[0]]
            if not r.ids or any(s.shape[0] == 0 for s in r.ids):
                raise ValueError(f"request {i}: at least one sentence, and no empty one")
            r.speaker, r.src_se, r.tgt_se = self._speaker_id(q[1]), q[2], q[3]
            r.speed = float(q[4]) if len(q) > 4 and q[4] is not None else 1.0
            if not r.speed > 0:
                raise ValueError(f"request {i}: speed {q[4]!r}")
            r.out_sr = rates.check_rate(q[5] if len(q) > 5 else None, "out_sr")
            r.tau = item_tau(1, q[6]) if len(q) > 6 and q[6] is not None else None      # None: the call's tau=
            if r.tau is not None and not isinstance(r.tau, float):
                raise _lib.OvError(f"request {i}: tau is one number per request")
            # convert_speed: the CONVERTER's speed= (the latent stretch of convert_many), distinct from the TTS speed
            r.convert_step = stretch_mod.step_of(q[7]) if len(q) > 7 and q[7] is not None else None
            reqs.append(r)
        n = len(reqs)
        for name, per_request in (("noise_w", noise_w), ("noise_z", noise_z)):
            if per_request is None:
                continue
            if len(per_request) != n:
                raise ValueError(f"{name}: one list per request ({n}), got {len(per_request)}")
            for i, (r, per_sentence) in enumerate(zip(reqs, per_request)):
                if len(per_sentence) != len(r.ids):
                    raise ValueError(f"{name}[{i}]: one tensor per sentence ({len(r.ids)}), got {len(per_sentence)}")
        if noise is not None and len(noise) != n:
            raise ValueError(f"noise: one [1, 192, >= T] tensor per request ({n}), got {len(noise)}")
        if output_paths is not None and len(output_paths) != n:
            raise ValueError("output_paths: one per request")
        return reqs

    # ---- the chain ---------------------------------------------------------------------------------------------------
    def synthesize_many(self, reqs, noise_w=None, noise_z=None, noise_scale=0.667, noise_scale_w=0.6,
                        max_sentences_per_launch=DEFAULT_SENTENCES_PER_LAUNCH, generator="fp32", mixed=False):
        """Steps 1 and 2 for parsed requests: the joined base-speaker waveforms, one 1-D device tensor per request at
        the TTS model's rate.  ``generator``: ``"fp32"`` (default) or ``"bf16"``, handed to ``infer_padded``.
        ``mixed``: False (default) -- one launch sequence per ``(speed, speaker)`` key; True -- the sentences of all
        requests in shared launches (``sentence_batches(mixed=True)``), ``infer_padded`` getting one speaker and one
        speed per sentence."""
        import torch
        gen_kw = {} if _lib.check_generator(generator) == "fp32" else {"generator": generator}
        batches = sentence_batches([[s.shape[0] for s in r.ids] for r in reqs], [(r.speed, r.speaker) for r in reqs],
                                   max_sentences_per_launch, mixed=bool(mixed))
        self.last_batches = batches
        pick = lambda nz, items: None if nz is None else [nz[r][s] for r, s in items]
        outs, counts = [], []
        for key, items in batches:
            if key is None:         # a mixed batch: every sentence brings its request's speaker and speed
                speaker, speed = [reqs[r].speaker for r, _ in items], [reqs[r].speed for r, _ in items]
            else:
                speed, speaker = key
            o, frames = self.tts.infer_padded([reqs[r].ids[s] for r, s in items], speaker, speed=speed,
                                              noise_scale=noise_scale, noise_scale_w=noise_scale_w,
                                              noise_w=pick(noise_w, items), noise_z=pick(noise_z, items), **gen_kw)
            outs.append(o)
            counts.append(frames)
        # the one copy to the host: the frame counts size the requests' waveforms
        frames = torch.cat(counts).cpu().tolist()
        samples, at = {}, 0
        for _, items in batches:
            for item in items:
                samples[item] = frames[at] * self.hop
                at += 1
        gaps = [gap_samples(self.tts_sr, r.speed) for r in reqs]
        plan, totals = join_plan([[samples[(i, s)] for s in range(len(r.ids))] for i, r in enumerate(reqs)], gaps)
        bases, total = _bases(totals)
        dst = torch.empty(max(total, 1), dtype=torch.float32, device=outs[0].device)
        for o, (_, items) in zip(outs, batches):            # one launch per infer batch, into the requests' waveforms
            ld = o.shape[-1]
            records = []
            for row, (r, s) in enumerate(items):
                n, off, g = plan[r][s]
                records.append((row * ld, n, bases[r] + off, g))
            _launch_join(o, records, dst)
        self.last_launches = {"infer": len(batches), "join": len(batches)}
        return [dst[b:b + t] for b, t in zip(bases, totals)]

    def _wavenet_cores(self):
        """Both halves of the chain: the TTS model's flow and the converter's posterior encoder and flow."""
        return tuple(self.tts._wavenet_cores()) + tuple(self.converter._wavenet_cores())

    @wavenet_keyword
    def speak_ids_many(self, requests, tau=0.3, noise_w=None, noise_z=None, noise=None, output_paths=None,
                       message="default", window_frames=longform.DEFAULT_WINDOW_FRAMES,
                       windows_per_launch=longform.DEFAULT_MANY_WINDOWS_PER_LAUNCH,
                       max_sentences_per_launch=DEFAULT_SENTENCES_PER_LAUNCH, noise_scale=0.667, noise_scale_w=0.6,
                       generator="fp32", mixed=False):
        """Many "say this in that voice" requests in shared launches.  ``requests[i]``: ``(id sequences, speaker, src_se,
        tgt_se[, speed[, out_sr[, tau]]])`` (or a dict with those keys) -- the sentences as symbol ids (blanks interspersed by
        the caller if the config asks for it), the base speaker's name or id, the two ``[1, 256, 1]`` embeddings, the
        speed (default 1.0), the rate of the result (None: the converter's) and the request's own ``tau`` (None: the
        ``tau=`` of the call, one number or one per request), and ``convert_speed`` (None: none): the converter's
        ``speed=`` for this request (``convert_many``: the converted latent stretched in front of the generator, a number
        in ``[0.5, 2.0]``), distinct from the TTS ``speed``.  Requests with different ``tau`` still go through ONE
        ``convert_many``, their windows sharing its launches.  Explicit noise makes a call
        reproducible: ``noise_w[i][s]`` ``[2, Tx]`` and ``noise_z[i][s]`` ``[192, >= Ty]`` per sentence, ``noise[i]``
        ``[1, 192, >= T]`` per request for the converter; None: drawn on the device.  Returns one float32 numpy array
        per request (watermark hook applied at the converter's rate), and writes ``output_paths[i]`` when given.  The
        result equals the chain of the public pieces (module docstring) and depends on the batch composition.
        ``generator``: ``"fp32"`` (default) or ``"bf16"`` -- both halves of the chain run their generator on those
        kernels (``tts_from_ids(generator=)``, ``convert_many(generator=)``; the contract above holds with the same
        keyword on the public pieces).  ``mixed=True``: requests of different speeds and base speakers share ``infer``
        launches too (``synthesize_many``); the public piece is then ``infer_padded`` with the per-sentence speaker and
        speed lists of each batch of ``last_batches``.  The default keeps one launch sequence per ``(speed, speaker)``."""
        import torch
        from . import audio_io
        _lib.check_generator(generator)
        gen_kw = {} if generator == "fp32" else {"generator": generator}
        conv = self.converter
        reqs = self._parse(requests, noise_w, noise_z, noise, output_paths)
        if not reqs:
            return []
        tau = item_tau(len(reqs), tau)
        if torch.is_tensor(tau):
            tau = tau.tolist()
        tau = rows_tau([(tau if isinstance(tau, float) else tau[i]) if r.tau is None else r.tau
                        for i, r in enumerate(reqs)])
        with torch.no_grad():
            waves = self.synthesize_many(reqs, noise_w, noise_z, noise_scale, noise_scale_w, max_sentences_per_launch,
                                         mixed=mixed, **gen_kw)
            msr = int(conv.hps.data.sampling_rate)
            waves = rates.resample_many(waves, [(self.tts_sr, msr)] * len(waves), self.device)
            steps = None
            if any(r.convert_step is not None for r in reqs):
                steps = [stretch_mod.ONE if r.convert_step is None else r.convert_step for r in reqs]
            outs = conv._windowed(window_frames, windows_per_launch).convert_many(
                waves, [r.src_se for r in reqs], [r.tgt_se for r in reqs], tau=tau, noises=noise, **gen_kw,
                **stretch_mod.kw(steps=steps))
            out_srs = [r.out_sr for r in reqs]
            audios = conv._finish_many(outs, message, out_srs)
        if output_paths is not None:
            for path, audio, r in zip(output_paths, audios, out_srs):
                audio_io.write(path, audio, msr if r is None else r)
        return audios

    def speak_ids(self, id_sequences, speaker, src_se, tgt_se, speed=1.0, out_sr=None, output_path=None, noise_w=None,
                  noise_z=None, noise=None, generator="fp32", mixed=False, **kwargs):
        """``speak_ids_many`` of one request: its audio (and ``output_path`` written when given).  ``mixed``: as for
        ``speak_ids_many`` (one request has one key: the same sentences share the launches either way, ``mixed=True``
        runs them on the per-item kernels)."""
        _lib.check_generator(generator)
        one = lambda x: None if x is None else [x]
        return self.speak_ids_many([(id_sequences, speaker, src_se, tgt_se, speed, out_sr)], noise_w=one(noise_w),
                                   noise_z=one(noise_z), noise=one(noise), output_paths=one(output_path),
                                   generator=generator, mixed=mixed, **kwargs)[0]

    def speak_many(self, texts, speaker, src_se, tgt_se, language="English", speed=1.0, out_sr=None, generator="fp32",
                   mixed=False, **kwargs):
        """``speak_ids_many`` of texts, each through ``BaseSpeakerTTS.text_to_ids`` (sentence pieces, language marks,
        ``get_text``: exactly what ``tts`` does; the same RuntimeError when no text front end is registered).
        ``speaker`` / ``src_se`` / ``tgt_se`` / ``language`` / ``speed`` / ``out_sr``: one for all, or a list with one
        per text; ``generator`` and ``mixed``: as for ``speak_ids_many``."""
        _lib.check_generator(generator)
        texts = list(texts)
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * len(texts)
        cols = [per(v) for v in (speaker, src_se, tgt_se, language, speed, out_sr)]
        if any(len(c) != len(texts) for c in cols):
            raise ValueError("speak_many: one value, or one per text")
        requests = [(self.tts.text_to_ids(t, lang), spk, s, g, spd, r)
                    for t, spk, s, g, lang, spd, r in zip(texts, *cols)]
        return self.speak_ids_many(requests, generator=generator, mixed=mixed, **kwargs)

    def speak_stream_ids(self, id_sequences, speaker, src_se, tgt_se, speed=1.0, *, seed=None, tau=0.3, out_sr=None,
                         chunk_frames=60, live_chunk_frames=15, generator="fp32", wavenet=None, noise_scale=0.667,
                         noise_scale_w=0.6, lookahead_frames=None, message=None, watermark_hold=16000,
                         message_repeat=False):
        """``speak_ids`` as a Python generator of device tensors: every chunk of ``tts_stream_from_ids`` (gaps
        included) is pushed into one stream of a converter ``LivePool`` (``sr_in`` = the TTS model's rate where the two
        differ, ``sr_out=out_sr``) and what that stream returns is yielded; the stream is closed at the end.
        Concatenated, the output equals ``converter.convert_long(joined, src_se, tgt_se, seed=seed, tau=tau, sr=the TTS
        rate, out_sr=out_sr)`` of the concatenated ``tts_stream_from_ids(..., seed=seed)`` output (bit for bit with
        direct kernels and equal rates; within the rates' bar otherwise).  ``seed``: the TTS sentences take streams
        ``k + i`` of it, the converter's posterior noise stream ``k`` (purpose 0); None: nothing is reproducible.
        ``chunk_frames`` / ``live_chunk_frames``: the chunk of the synthesis / of the conversion stream.
        ``message`` / ``watermark_hold`` / ``message_repeat``: the conversion stream's block-wise native watermark, as
        for ``ToneColorConverter.live_stream`` (checked at the call; ``tts_live_pool`` speech itself is never marked)."""
        if lookahead_frames is not None:          # at the call, not at the first next()
            raise ValueError("lookahead_frames belongs to the converter's live streams (live_stream / live_pool): "
                             "speak_stream* emits committed samples only")
        from . import watermark as watermark_mod
        watermark_mod.stream_mark(self.converter.watermark_model, message, watermark_hold, message_repeat)
        return self._speak_stream_ids(id_sequences, speaker, src_se, tgt_se, speed, seed, tau, out_sr, chunk_frames,
                                      live_chunk_frames, generator, wavenet, noise_scale, noise_scale_w,
                                      dict(message=message, watermark_hold=watermark_hold, message_repeat=message_repeat))

    def _speak_stream_ids(self, id_sequences, speaker, src_se, tgt_se, speed, seed, tau, out_sr, chunk_frames,
                          live_chunk_frames, generator, wavenet, noise_scale, noise_scale_w, mark_kw):
        conv = self.converter
        chunks = self.tts.tts_stream_from_ids(id_sequences, self._speaker_id(speaker), speed=speed,
                                              noise_scale=noise_scale, noise_scale_w=noise_scale_w, seed=seed,
                                              chunk_frames=chunk_frames, generator=generator, wavenet=wavenet)
        msr = int(conv.hps.data.sampling_rate)
        pool = conv.live_pool(tau=tau, chunk_frames=live_chunk_frames, max_streams_per_launch=1, generator=generator,
                              wavenet=wavenet)
        from . import noise as noise_mod
        h = pool.open(src_se, tgt_se, sr_in=None if self.tts_sr == msr else self.tts_sr, sr_out=out_sr,
                      **mark_kw, **noise_mod.kw(seed))
        for chunk in chunks:
            pool.push(h, chunk)
            o = pool.step().get(h)
            if o is not None and o.numel():
                yield o
        pool.close(h)
        o = pool.step().get(h)
        if o is not None and o.numel():
            yield o

    def speak_stream(self, text, speaker, src_se, tgt_se, language="English", speed=1.0, **kwargs):
        """``speak_stream_ids`` of a text (``BaseSpeakerTTS.text_to_ids``)."""
        return self.speak_stream_ids(self.tts.text_to_ids(text, language), speaker, src_se, tgt_se, speed=speed, **kwargs)

    def speak(self, text, speaker, src_se, tgt_se, language="English", speed=1.0, out_sr=None, output_path=None,
              noise_w=None, noise_z=None, noise=None, generator="fp32", **kwargs):
        """``speak_many`` of one text."""
        _lib.check_generator(generator)
        return self.speak_ids(self.tts.text_to_ids(text, language), speaker, src_se, tgt_se, speed=speed, out_sr=out_sr,
                              output_path=output_path, noise_w=noise_w, noise_z=noise_z, noise=noise,
                              generator=generator, **kwargs)
