"""Streaming synthesis: audio leaves while the sentence is still being generated.

``TtsEngine.infer`` returns after the whole utterance has been through the flow and the four generator stages, so its
time to first audio is its time to last audio.  Everything behind the prior sample ``z_p`` is a ``ConverterEngine``
(``TtsEngine.core``) and already runs as carried-state units (``live.py``); with ``seed=`` the noise of ``z_p`` is a pure
function of ``(seed, stream, channel, frame)`` (``noise.py``, purpose 2).  What this module adds is the producer:

* the token-rate front half (``TtsEngine.front``: text encoder, duration predictors, durations) runs once per sentence
  -- for all sentences opened since the last step as one padded batch -- and leaves ``m`` / ``logs`` of every token and
  the duration prefix sums ``cum`` in the sentence's slot of a token arena;
* every round, ONE ``ov_expand_prior_rows_f32`` launch (csrc/tts_live.hip) writes the next ``chunk_frames`` frames of
  ``z_p`` of every open sentence straight into the state row of its first unit -- noise, expansion and carry in one;
* the units ``[r, g0 .. g3]`` (``live.live_units`` without ``q`` and ``f``) then run exactly as in ``live.LivePool``:
  the ``Cascade``, the arena, the carries, the launch ladder and the bf16 generator units are ``live.UnitPool``'s.

Contract: a stream's concatenated output equals ``infer`` of that sentence alone (B = 1) with the same ``(seed,
stream)`` pair and controls -- bit for bit with direct kernels (``use_winograd = False``), within the project's live bar
(1e-4) with the default ones.  Streams are always counter-based: without ``seed=`` one is drawn at ``open`` from torch's
global generator.
"""
import torch

from . import _lib, clone
from . import noise as noise_mod
from .live import DEFAULT_LIVE_STREAMS_PER_LAUNCH, Cascade, UnitPool, check_chunk, live_units
from .tts_engine import check_token_count

DEFAULT_CHUNK_FRAMES = 60     # chosen from profiles/tts_stream_table.json
RECORD_FIELDS = 13          # ov_expand_prior_rows_f32's record (include/openvoice_amd.h)
MAX_RECORDS = 65535


def tts_units(cfg):
    """The unit table of streaming synthesis: ``live_units`` without the posterior encoder and the forward flow --
    ``[r, g0 .. g3]``, reaches and alignments unchanged."""
    return [u for u in live_units(cfg) if u["kind"] in ("r", "g")]


def first_audio_need(units):
    """Input columns of the first unit before the last unit can emit its first column: unit k emits once it holds more
    than ``right_k`` columns, and hands ``(n_k - right_k) * stride_k`` columns on, so going backwards from one column
    past the last unit's right reach, ``need_k = ceil(need_{k+1} / stride_k) + right_k``."""
    need = units[-1]["right"] + 1
    for u in reversed(units[:-1]):
        need = -(-need // u["stride"]) + u["right"]
    return need


def first_audio_frames(cfg, chunk_frames):
    """``z_p`` frames a sentence must have been fed before its first sample leaves: ``first_audio_need`` rounded up to
    whole chunks (a shorter sentence emits when it ends).  The released configurations need 45 frames (32 of them the
    reverse flow's right reach, 11 stage 0's): 45 at a chunk of 15, 60 at a chunk of 60."""
    c = check_chunk(cfg, chunk_frames)
    return -(-first_audio_need(tts_units(cfg)) // c) * c


def stream_plan(sample_counts, sr, speed=1.0):
    """Where a request's sentences and gaps lie in its stream: ``clone.join_plan`` of one utterance with
    ``clone.gap_samples(sr, speed)`` zeros after every sentence -> ``([(n, offset, gap)], total samples)``."""
    records, totals = clone.join_plan([list(sample_counts)], clone.gap_samples(sr, speed))
    return records[0], totals[0]


class _Sentence:
    """One stream of a ``TtsLivePool``: its controls, cascade bookkeeping and arena slots."""

    def __init__(self, pool, slot, ids, speaker, speed, noise_scale, noise_scale_w, sdp_ratio, seed):
        self.slot, self.ids, self.speaker, self.speed = slot, ids, speaker, speed
        self.noise_scale, self.noise_scale_w, self.sdp_ratio, self.seed = noise_scale, noise_scale_w, sdp_ratio, seed
        self.cas = Cascade(pool.units, pool.chunk)
        K = len(pool.units)
        self.stored, self.s0, self.half = [0] * K, [0] * K, [0] * K
        self.Tx, self.T, self.conds = int(ids.numel()), None, None     # T: frames, known after the front half


class TtsLivePool(UnitPool):
    """Many sentences synthesised as streams, stepped together.  ``open(ids, speaker_id, ...)`` -> handle (host work
    only); ``step()`` runs the front half of every sentence opened since the last step (one padded batch, one host sync
    for the frame counts), then ONE round: every open sentence is fed ``chunk_frames`` more ``z_p`` frames (its last
    round fewer) by one ``ov_expand_prior_rows_f32`` launch and the units run, in launches of up to
    ``max_streams_per_launch`` rows -> ``{handle: new samples}`` (device tensors).  A sentence that has emitted its
    last sample is retired; ``active`` lists the others.  ``generator`` / ``wavenet``: as for ``live.LivePool``.
    ``frames_fed[h]`` / ``frames[h]``: ``z_p`` frames fed so far / of the whole sentence, while ``h`` is active.
    ``front_batch=False`` runs the front half per sentence instead of as one padded batch."""

    def __init__(self, model, chunk_frames=DEFAULT_CHUNK_FRAMES, max_streams_per_launch=DEFAULT_LIVE_STREAMS_PER_LAUNCH,
                 generator="fp32", wavenet=None, front_batch=True, lookahead_frames=None):
        if lookahead_frames is not None:
            raise ValueError("lookahead_frames belongs to the converter's live streams (live_stream / live_pool): "
                             "streaming TTS emits committed samples only")
        self.model = model
        self.tts = model.engine()
        cfg = model.model_cfg
        super().__init__(self.tts.core, cfg, tts_units(cfg), chunk_frames, max_streams_per_launch, generator=generator,
                         wavenet=wavenet)
        self.front_batch = bool(front_batch)
        self.first_audio_frames = first_audio_frames(cfg, self.chunk)
        self._streams, self._pending, self._next = {}, [], 0
        self.frames_fed, self.frames = {}, {}
        self.tok = self.cum = None          # token arena: [slots][2 * inter][tok_cap] fp32 and [slots][tok_cap] int32
        self.tok_cap = 0

    @property
    def active(self):
        return list(self._streams)

    def open(self, ids, speaker_id, speed=1.0, noise_scale=0.667, noise_scale_w=0.6, sdp_ratio=0.2, *, seed=None):
        """A new sentence -> its handle.  ``ids``: its symbol ids; ``speaker_id``: a row of the speaker table;
        ``speed`` > 0; ``seed``: an int (stream 0) or a ``(seed, stream)`` pair, None: drawn from torch's generator."""
        eng = self.engine
        if getattr(eng, "_bf16_on", False) or getattr(eng, "_split3_on", False):
            raise ValueError("live streams run the fp32 generator only: turn use_bf16_generator / enable_split_bf16x3 off")
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu()
        if ids.numel() == 0:
            raise ValueError("open: an empty sentence")
        check_token_count(ids.numel())
        if int(ids.min()) < 0 or int(ids.max()) >= self.tts.n_vocab:
            raise IndexError("token id out of range")
        speaker = int(speaker_id)
        if not 0 <= speaker < self.tts.n_speakers:
            raise IndexError("speaker id out of range")
        speed = float(speed)
        if not speed > 0:
            raise ValueError(f"open: speed {speed!r}")
        if seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)).item())
        st = _Sentence(self, None, ids, speaker, speed, float(noise_scale), float(noise_scale_w), float(sdp_ratio),
                       noise_mod.check_seed(seed))
        st.slot = self._take_slot()
        h = self._next
        self._next += 1
        self._streams[h] = st
        self._pending.append(h)
        self.frames_fed[h] = 0
        return h

    # ---- the token-rate front half ---------------------------------------------------------------------------------
    def _ensure_tok(self, Tx):
        """The token arena holds every slot at ``tok_cap`` tokens; a longer sentence or more slots regrow it (the open
        sentences' rows are copied)."""
        cap = max(self.tok_cap, -(-int(Tx) // 64) * 64)
        rows = 2 * self.inter
        if self.tok is not None and cap == self.tok_cap and self.tok.shape[0] >= self._slots:
            return
        tok = torch.zeros(self._slots, rows, cap, dtype=torch.float32, device=self.device)
        cum = torch.zeros(self._slots, cap, dtype=torch.int32, device=self.device)
        if self.tok is not None:
            n = self.tok.shape[0]
            tok[:n, :, :self.tok_cap].copy_(self.tok)
            cum[:n, :self.tok_cap].copy_(self.cum)
        self.tok, self.cum, self.tok_cap = tok, cum, cap

    @torch.no_grad()
    def _front(self, handles):
        """``TtsEngine.front`` of the sentences ``handles`` as one padded batch with per-item controls, then two carries
        move each sentence's ``stats`` columns and ``cum`` row into its slot of the token arena."""
        sts = [self._streams[h] for h in handles]
        Tx = max(st.Tx for st in sts)
        tokens = torch.zeros(len(sts), Tx, dtype=torch.int64)
        for b, st in enumerate(sts):
            tokens[b, :st.Tx] = st.ids
        fh = self.tts.front(tokens, torch.tensor([st.Tx for st in sts], dtype=torch.int64),
                            torch.tensor([st.speaker for st in sts], dtype=torch.int64),
                            noise_scale=[st.noise_scale for st in sts], length_scale=[1.0 / st.speed for st in sts],
                            noise_scale_w=[st.noise_scale_w for st in sts], sdp_ratio=[st.sdp_ratio for st in sts],
                            seed=[st.seed for st in sts])
        y_len = fh["y_len"].cpu().tolist()                   # the one host sync, as in infer
        self._ensure_tok(Tx)
        Lx, rows, cap = fh["Lx"], 2 * self.inter, self.tok_cap
        rec_tok = [(b * rows * Lx, st.slot * rows * cap, rows, st.Tx, Lx, cap) for b, st in enumerate(sts)]
        rec_cum = [(b * Lx, st.slot * cap, 1, st.Tx, Lx, cap) for b, st in enumerate(sts)]
        stats, cum = fh["stats"], fh["cum"].view(torch.float32)           # bits move unchanged through a 32-bit copy
        _lib.call("ov_carry_rows_f32", torch.tensor(rec_tok, dtype=torch.int64).to(self.device), len(sts), stats,
                  stats.numel(), self.tok, self.tok.numel())
        _lib.call("ov_carry_rows_f32", torch.tensor(rec_cum, dtype=torch.int64).to(self.device), len(sts), cum,
                  cum.numel(), self.cum.view(torch.float32), self.cum.numel())
        core = self.engine
        for b, (h, st) in enumerate(zip(handles, sts)):
            st.T = self.frames[h] = int(y_len[b])
            g = fh["g"][b:b + 1].contiguous()                # the launches of a solo infer: one row each
            st.conds = dict(tgt=[core._wn_cond(cp["wn"], g) for cp in core.couplings],
                            d=core.generator.cond(g))
            if self.generator == "bf16":
                st.conds["d16"] = core.live_cond_bf16(g)

    # ---- rounds ----------------------------------------------------------------------------------------------------
    def _plan_round(self):
        """Host bookkeeping of one round: ``(jobs, plans)`` -- ``jobs`` = [(stream, new frames, first frame)] for the
        feed, ``plans`` = [(handle, stream, pieces)] for the units."""
        jobs, plans = [], []
        for h, st in self._streams.items():
            if st.T is None or st.cas.done:
                continue
            f0 = st.cas.n[0]
            nf = min(self.chunk, st.T - f0)
            plans.append((h, st, st.cas.round(nf, final=f0 + nf == st.T)))
            if nf > 0:
                jobs.append((st, nf, f0))
                self.frames_fed[h] = f0 + nf
        return jobs, plans

    def _feed_records(self, jobs):
        """The records of a round's ``ov_expand_prior_rows_f32`` launch, one per job: the piece lands behind what the
        stream's first unit already stores (``(stored - s0)`` columns into its current state half, row stride
        ``cap[0]``), and that unit's stored count moves on."""
        C, cap, recs = self.inter, self.tok_cap, []
        for st, nf, f0 in jobs:
            col = st.stored[0] - st.s0[0]
            if col + nf > self.cap[0]:
                raise RuntimeError("live stream state overflow (unit r)")
            m_off = st.slot * 2 * C * cap
            recs.append(st.seed + (f0, nf, st.Tx, st.T, m_off, cap, m_off + C * cap, cap, st.slot * cap,
                                   self._state(st, 0, st.half[0]) + col, self.cap[0]))
            st.stored[0] += nf
        return recs

    def _feed(self, jobs):
        recs = self._feed_records(jobs)
        for i in range(0, len(recs), MAX_RECORDS):
            part = recs[i:i + MAX_RECORDS]
            scales = torch.tensor([st.noise_scale for st, _, _ in jobs[i:i + MAX_RECORDS]], dtype=torch.float32)
            _lib.call("ov_expand_prior_rows_f32", torch.tensor(part, dtype=torch.int64).to(self.device), len(part),
                      self.inter, self.tok, self.tok.numel(), self.cum, self.cum.numel(), scales.to(self.device),
                      self.mem, self.mem.numel(), max(r[3] for r in part))

    @torch.no_grad()
    def step(self):
        """The front half of the sentences opened since the last step, then one round -> ``{handle: new samples}``."""
        if self._pending:
            pending, self._pending = self._pending, []
            for group in ([pending] if self.front_batch else [[h] for h in pending]):
                self._front(group)
        jobs, plans = self._plan_round()
        if not plans:
            return {}
        self._feed(jobs)
        out = self._run_units(plans)
        for h, st, _ in plans:
            if st.cas.done:
                self._free_slots.append(self._streams.pop(h).slot)
                self.frames_fed.pop(h), self.frames.pop(h)
        return out

    def fed_whole(self, h):
        """True once every ``z_p`` frame of sentence ``h`` has been fed (what remains of it is the units draining)."""
        return h not in self._streams or (h in self.frames and self.frames_fed[h] == self.frames[h])


class TtsLiveStream:
    """One sentence as a stream (a ``TtsLivePool`` of one): ``step()`` -> its new samples (a device tensor, possibly
    empty), ``done`` once the last sample has left; iterating yields the non-empty chunks to the end.
    ``first_audio_frames``: the pool's."""

    def __init__(self, model, ids, speaker_id, speed=1.0, noise_scale=0.667, noise_scale_w=0.6, sdp_ratio=0.2, *,
                 seed=None, chunk_frames=DEFAULT_CHUNK_FRAMES, generator="fp32", wavenet=None):
        self._pool = TtsLivePool(model, chunk_frames=chunk_frames, max_streams_per_launch=1, generator=generator,
                                 wavenet=wavenet)
        self._h = self._pool.open(ids, speaker_id, speed=speed, noise_scale=noise_scale, noise_scale_w=noise_scale_w,
                                  sdp_ratio=sdp_ratio, seed=seed)
        self.first_audio_frames = self._pool.first_audio_frames

    @property
    def done(self):
        return self._h not in self._pool._streams

    def step(self):
        if self.done:
            raise RuntimeError("step() after the sentence's last sample")
        o = self._pool.step().get(self._h)
        return o if o is not None else torch.empty(0, dtype=torch.float32, device=self._pool.device)

    def __iter__(self):
        while not self.done:
            o = self.step()
            if o.numel():
                yield o


def stream_sentences(pool, id_sequences, speaker_id, speed, noise_scale, noise_scale_w, seed, sr):
    """The generator behind ``BaseSpeakerTTS.tts_stream_from_ids``: the sentences in order through ``pool``, each
    followed by ``clone.gap_samples(sr, speed)`` zeros.  Sentence ``i`` runs on stream ``k + i`` of ``seed``
    (``noise.per_item``).  Sentence ``i + 1`` is opened once sentence ``i`` has been fed whole, so the units stay busy
    while ``i`` drains; its samples wait until ``i``'s last one and gap have been yielded."""
    seqs = [torch.as_tensor(s, dtype=torch.int64).reshape(-1) for s in id_sequences]
    if seed is None:
        seed = int(torch.randint(0, 1 << 62, (1,)).item())
    seeds = noise_mod.per_item(seed, len(seqs))
    gap = clone.gap_samples(sr, speed)
    handles, held, cur = [], {}, 0

    def open_next():
        i = len(handles)
        handles.append(pool.open(seqs[i], speaker_id, speed=speed, noise_scale=noise_scale,
                                 noise_scale_w=noise_scale_w, seed=seeds[i]))
        held[handles[i]] = []

    if seqs:
        open_next()
    while cur < len(seqs):
        for h, o in pool.step().items():
            held[h].append(o)
        if len(handles) < len(seqs) and pool.fed_whole(handles[-1]):
            open_next()
        while cur < len(handles):
            h = handles[cur]
            for o in held[h]:
                yield o
            held[h] = []
            if h in pool._streams:
                break
            if gap:
                yield torch.zeros(gap, dtype=torch.float32, device=pool.device)
            cur += 1
