"""Low-latency live streams: the conversion as a cascade of units that keep their recent input as state.

``longform.ConversionStream`` recomputes 2 x 120 frames of context per window, so its latency is the window
(3.0 s at the smallest) and at low latency most of its work is context.  Here every stage of the conversion is a
**unit** that runs the engine's own launches on a buffer ``[left history | new columns]`` with the kernels' "same" zero
padding and keeps only the output columns whose receptive field lies inside the buffer:

* ``q``: posterior encoder (q_pre, 16 WaveNet layers, q_proj with the noise), frame rate;
* ``f`` / ``r``: the flow forward with ``g_src`` / reverse with ``g_tgt``, frame rate;
* ``g0 .. g3``: one generator stage each (leaky_relu, ConvTranspose, MRF; conv_pre + cond in ``g0``, conv_post + tanh in
  the last one), at that stage's input column rate.

A unit with input columns ``[0, n)`` received emits the output of input columns ``[e, n - right)`` (everything, once its
input is complete).  The buffer it runs on starts ``left`` columns before ``e``, rounded down to the unit's ``align``
grid: for a generator stage that grid puts the buffer's first output column on the stage's Winograd tile grid
(``4 x dil`` columns, lcm over the dilations), so tiles keep their one-pass phase.  At the file start the kernels' zero
padding is what one pass sees; at the end (``close``) the spectrogram's reflect padding is applied and every unit runs
once more up to its true right end, never past frame ``T`` (the generator is unmasked).

Only the input chunk is quantised: the stream advances the posterior encoder by ``chunk_frames`` interior frames at a
time; every downstream unit emits all it can.  A sample therefore leaves ``live_latency_samples`` =
``R + hop * chunk + (n_fft - hop) / 2`` input samples after it arrived at most, ``R`` = the units' right reaches in
samples (``live_right_samples``).

Device side, a ``LivePool`` keeps each stream's unit states in one arena slot per stream (two halves per unit, so a
history shift never overlaps itself).  For every unit and launch, ``ov_carry_rows_f32`` gathers the ready streams'
buffers into batch rows (and shifts their kept history into the other half) in one launch, the unit runs on the batch,
and a second carry scatters the new columns into the next unit's state.  ``LiveStream`` is a pool of one.

A stream opened with ``sr_in`` / ``sr_out`` (``rates``) takes its pushes at ``sr_in`` and returns samples at ``sr_out``: a
step first resamples the new input of every such stream to the model rate in one launch, runs the rounds, then
resamples every stream's new output in one more launch.

``generator="bf16"`` (pool or stream) runs the ``g`` units on the bf16 channels-last generator (``bf16.GeneratorBf16``)
instead of the fp32 kernels; ``q``, ``f`` and ``r`` keep their fp32 kernels (``wavenet="bf16"``
chooses their WaveNet layers separately).  The cascade, the reaches, the arena and the carries are
the same -- state stays fp32 channels-first -- so each ``g`` unit changes layout on the way in
(``ov_rows_f32_to_cl_bf16``) and on the way out (``ov_cl_bf16_to_rows_f32``; the last stage writes fp32 itself).  What
one stage hands the next is a bf16 value held in fp32, so the arena adds no rounding: the stream computes the one-pass
bf16 conversion.  The choice belongs to the pool, not to the engine: fp32 and bf16 pools run side by side on one model.
"""
import math

import torch

from . import _lib, rates
from . import noise as noise_mod
from . import watermark as watermark_mod
from .engine import rows_tau
from .generator import generator_stages, samples_per_frame
from .longform import launch_ladder, stream_end_frames, winograd_grid_frames
from .params import ENC_Q_KERNEL, ENC_Q_LAYERS, FLOW_KERNEL, FLOW_LAYERS, N_FLOWS
from .streams import PushedPool, WaveBuffer

DEFAULT_CHUNK_FRAMES = 15
DEFAULT_LIVE_STREAMS_PER_LAUNCH = 32
CONV_PRE_KERNEL = 7
CONV_POST_KERNEL = 7
GENERATORS = ("fp32", "bf16")


def check_generator(generator):
    if generator not in GENERATORS:
        raise ValueError(f"generator must be 'fp32' or 'bf16', got {generator!r}")
    return generator


def _stage_tile(cfg):
    """Winograd tile grid of a generator stage in its own columns: lcm of 4 * dil over dilation 1 (the convs2) and the
    configured ones (the convs1) -- what ``winograd_grid_frames`` aligns."""
    tile = 4
    for d in [1] + [v for dl in cfg["resblock_dilation_sizes"] for v in dl]:
        tile = tile * 4 * d // math.gcd(tile, 4 * d)
    return tile


def live_units(cfg):
    """The unit table, a pure function of the config: one dict per unit in cascade order with

    * ``name``, ``kind`` (``q`` / ``f`` / ``r`` / ``g``), ``stage`` (generator stage or None);
    * ``rate``: input columns per frame; ``stride``: output columns per input column;
    * ``left`` / ``right``: the reach of one output column into the unit's input, in input columns;
    * ``align``: the buffer start is a multiple of it (input columns);
    * ``history``: input columns kept before the first column still to emit, at most (``left + align - 1``).

    Frame-rate units: a WaveNet of n layers of kernel k (dilation 1) reaches n (k - 1) / 2 frames each way; q_pre,
    q_proj and the coupling pre / post are 1 x 1.  Generator stage i (stride s, kernel 2 s, padding (k - s) / 2): the MRF
    reaches rho = max over ResBlocks of (k - 1) / 2 * (sum(dil) + len(dil)) output columns (+ (7 - 1) / 2 for conv_post
    on the last stage); the ConvTranspose maps output column j to inputs [ceil((j + pad - k + 1) / s), floor((j + pad) /
    s)], so right = floor((s - 1 + rho + pad) / s) and left = floor((rho + k - 1 - pad) / s); conv_pre adds 3 frames to
    both on stage 0.  Released configurations: q / f / r 32 each way, g0 11, g1 8, g2 31, g3 32 (input columns)."""
    units = [dict(name="q", kind="q", stage=None, rate=1, stride=1, left=ENC_Q_LAYERS * (ENC_Q_KERNEL - 1) // 2,
                  right=ENC_Q_LAYERS * (ENC_Q_KERNEL - 1) // 2, align=1)]
    flow = N_FLOWS * FLOW_LAYERS * (FLOW_KERNEL - 1) // 2
    units.append(dict(name="f", kind="f", stage=None, rate=1, stride=1, left=flow, right=flow, align=1))
    units.append(dict(name="r", kind="r", stage=None, rate=1, stride=1, left=flow, right=flow, align=1))
    tile = _stage_tile(cfg)
    rho_mrf = max((k - 1) // 2 * (sum(d) + len(d)) for k, d in
                  zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]))
    rates, kernels = cfg["upsample_rates"], cfg["upsample_kernel_sizes"]
    rate = 1
    for i, (s, k) in enumerate(zip(rates, kernels)):
        pad = (k - s) // 2
        rho = rho_mrf + ((CONV_POST_KERNEL - 1) // 2 if i == len(rates) - 1 else 0)
        right = (s - 1 + rho + pad) // s
        left = (rho + k - 1 - pad) // s
        if i == 0:
            left += (CONV_PRE_KERNEL - 1) // 2
            right += (CONV_PRE_KERNEL - 1) // 2
        units.append(dict(name=f"g{i}", kind="g", stage=i, rate=rate, stride=s, left=left, right=right,
                          align=tile // math.gcd(tile, s)))
        rate *= s
    for u in units:
        u["history"] = u["left"] + u["align"] - 1
    return units


def live_right_samples(cfg):
    """Sum of the units' right reaches in output samples (each unit's right reach x the samples one of its input
    columns spans).  27 836 (108.7 frames) for the released configurations."""
    spf = samples_per_frame(cfg)
    return sum(u["right"] * spf // u["rate"] for u in live_units(cfg))


def check_chunk(cfg, chunk_frames):
    g = winograd_grid_frames(cfg)
    if isinstance(chunk_frames, bool) or not isinstance(chunk_frames, int) or chunk_frames <= 0 or chunk_frames % g:
        raise ValueError(f"chunk_frames must be a positive multiple of {g} (the Winograd grid), got {chunk_frames!r}")
    return chunk_frames


def check_lookahead(lookahead_frames):
    """``lookahead_frames``: None (emit committed samples only) or an integer >= 0."""
    A = lookahead_frames
    if A is None:
        return None
    if isinstance(A, bool) or not isinstance(A, int) or A < 0:
        raise ValueError(f"lookahead_frames must be None or an integer >= 0, got {A!r}")
    return A


def check_crossfade(crossfade_samples, lookahead_frames, chunk_frames, hop=256):
    """``crossfade_samples`` of a look-ahead stream: None = ``min(hop, hop * A)``, else an integer in
    ``[0, min(hop * A, hop * chunk_frames)]`` -- the previous preview reaches ``hop * A`` samples past the frontier, and a
    piece is ``hop * chunk_frames`` samples long."""
    A, X = lookahead_frames, crossfade_samples
    if A is None:
        if X is not None:
            raise ValueError("crossfade_samples needs lookahead_frames")
        return 0
    top = min(hop * A, hop * chunk_frames)
    if X is None:
        return min(hop, top)
    if isinstance(X, bool) or not isinstance(X, int) or not 0 <= X <= top:
        raise ValueError(f"crossfade_samples must be an integer in [0, {top}] (min(hop * lookahead_frames, hop * "
                         f"chunk_frames)), got {X!r}")
    return X


def crossfade_weights(X):
    """The fade-in of the seam, ``w[i] = 0.5 - 0.5 cos(pi (i + 1) / (X + 1))`` for i < X: float64 on the host, rounded
    once to float32 (one element, unused, when X = 0)."""
    i = torch.arange(1, max(X, 1) + 1, dtype=torch.float64)
    return (0.5 - 0.5 * torch.cos(math.pi * i / (X + 1))).to(torch.float32)


def live_latency_samples(cfg, chunk_frames, n_fft=1024, hop=256, lookahead_frames=None):
    """The bound no output sample's delay exceeds: input samples that arrive after sample t before sample t of the
    output leaves.  Output sample t leaves once the posterior encoder has taken ``m = floor((t + R) / hop) + 1`` frames
    rounded up to the chunk, i.e. frames up to ``c * ceil(m / c)``; frame f is interior (no end reflect padding can
    reach it) from ``f * hop + n_fft - pad`` samples on.  The worst case over t is
    ``R + hop * chunk_frames + (n_fft - hop) / 2`` (R = ``live_right_samples``, hop = samples per frame): 32 060
    samples (1.45 s at 22.05 kHz) at 15 frames for the released configurations.

    With ``lookahead_frames`` = A the stream emits ``[0, hop * max(0, F - A))`` once the posterior encoder has taken F
    frames, whatever the units' reaches: sample t leaves once ``F >= floor(t / hop) + A + 1``, rounded up to the chunk,
    i.e. at ``F <= floor(t / hop) + A + chunk_frames``, and frame F - 1 is interior from ``(F - 1) * hop + n_fft - pad``
    samples on.  The worst case (t a multiple of hop whose frame count rounds up by a whole chunk less one) is
    ``hop * (A + chunk_frames - 1) + n_fft - pad`` = ``hop * (A + chunk_frames) + (n_fft - hop) / 2``: 4 224 samples
    (0.19 s) at A = 0 and 15 frames, 8 064 (0.37 s) at A = 15."""
    check_chunk(cfg, chunk_frames)
    A = check_lookahead(lookahead_frames)
    if A is not None:
        return hop * (A + chunk_frames - 1) + n_fft - (n_fft - hop) // 2
    return live_right_samples(cfg) + hop * chunk_frames + (n_fft - hop) // 2


def interior_frames(n_samples, n_fft, hop):
    """Spectrogram frames whose samples have all arrived (no end reflect padding reaches them)."""
    pad = (n_fft - hop) // 2
    n = int(n_samples) + pad - n_fft
    return 0 if n < 0 else n // hop + 1


def _start(u, e):
    """First input column of a buffer whose first emitted column is e: ``left`` before it, down to ``align``."""
    return max(0, (e - u["left"]) // u["align"] * u["align"])


class Cascade:
    """Host bookkeeping of one stream through the units (no device work): ``round(new_frames, final)`` appends
    posterior-encoder input and returns the pieces the units run this round, in cascade order, at most one per unit:
    ``(k, b0, end, e0, e1)`` = unit k runs on input columns ``[b0, end)`` and keeps the output of ``[e0, e1)``.  A unit
    emits ``[e, n - right)`` (``[e, n)`` once its input is complete), at most ``chunk x rate`` columns per round, so a
    buffer never exceeds ``history + chunk x rate + right`` columns (``width``) and a unit's stored input
    ``history + right + 2 x chunk x rate`` (``capacity``)."""

    def __init__(self, units, chunk_frames):
        self.units, self.c = units, int(chunk_frames)
        K = len(units)
        self.n = [0] * K            # input columns received
        self.e = [0] * K            # input columns whose output has been emitted
        self.s0 = [0] * K           # first input column still stored
        self.final = False

    def width(self, k):
        u = self.units[k]
        return u["history"] + self.c * u["rate"] + u["right"]

    def capacity(self, k):
        u = self.units[k]
        return u["history"] + u["right"] + 2 * self.c * u["rate"]

    @property
    def done(self):
        return self.final and all(e == n for e, n in zip(self.e, self.n))

    def round(self, new_frames, final=False):
        self.n[0] += int(new_frames)
        self.final = self.final or bool(final)
        pieces, complete = [], self.final
        for k, u in enumerate(self.units):
            complete = complete and (k == 0 or self.e[k - 1] == self.n[k - 1])
            n, e0 = self.n[k], self.e[k]
            e1 = min(n if complete else n - u["right"], e0 + self.c * u["rate"])
            if e1 <= e0:
                continue
            b0, end = _start(u, e0), min(n, e1 + u["right"])
            pieces.append((k, b0, end, e0, e1))
            self.e[k] = e1
            self.s0[k] = _start(u, e1)
            if k + 1 < len(self.units):
                self.n[k + 1] += (e1 - e0) * u["stride"]
        return pieces


def preview_plan(units, n, e, lo, hi):
    """The pieces of a preview: the units run "as if the input ended now" on what a stream holds -- ``n[k]`` input
    columns stored, ``e[k]`` of them emitted (a ``Cascade``'s ``n`` / ``e`` after a round) -- to produce the samples
    ``[lo, hi)`` of the last unit's output, ``lo`` >= the committed end.  Back-propagated from the last unit the way
    ``tts_live.first_audio_need`` goes: unit k must hand on its output columns ``[olo, ohi)``, i.e. emit the input
    columns ``[olo // stride, ceil(ohi / stride))``; its buffer starts ``left`` columns before, down to the ``align``
    grid (the committed buffers' tile phase), and ends ``right`` columns after or at the end of the input,
    ``n[0] x rate``; what of that buffer lies past ``n[k]`` is unit k - 1's to hand on.  Returns
    ``[(k, b0, end, olo, ohi)]`` in cascade order: unit k runs on input columns ``[b0, end)`` -- stored ones up to
    ``n[k]``, then unit k - 1's -- and hands on its output columns ``[olo, ohi)``.  Units whose buffers lie inside the
    stored input of their successor do not appear.  A buffer whose output rows would not be a whole number of 16-byte
    vectors takes one column more (the fp32 MRF kernels of the stride-2 stages have vector instances only; committed
    buffers there are even because chunk, ``align`` and the rates are)."""
    pieces, olo, ohi = [], int(lo), int(hi)
    for k in range(len(units) - 1, -1, -1):
        if ohi <= olo:
            break
        u = units[k]
        s, total = u["stride"], n[0] * u["rate"]
        pe0, pe1 = olo // s, min(total, -(-ohi // s))
        if pe0 < e[k] or pe1 <= pe0:
            raise ValueError(f"preview range [{lo}, {hi}) reaches before the committed end of unit {u['name']}")
        b0, end = _start(u, pe0), min(total, pe1 + u["right"])
        if (end - b0) * s % 4 and end < total:      # dense output rows of whole 16-byte vectors, as a committed buffer's
            end += 1
        if u["kind"] == "g" and (end - b0) * s % 4:
            # a buffer that ends with the input: whole vectors only if ``align`` and ``rate`` make it so (they do for the
            # released configurations: both even on the stride-2 stages); the kernels have no scalar instance to fall to
            raise ValueError(f"preview buffer of unit {u['name']} [{b0}, {end}) has no whole number of 16-byte output rows")
        pieces.append((k, b0, end, olo, min(ohi, pe1 * s)))
        olo, ohi = max(b0, n[k]), end
    return pieces[::-1]


def lookahead_schedule(units, chunk_frames, lookahead_frames, crossfade_samples, rounds, hop=256):
    """The emission schedule of a look-ahead stream over ``rounds`` full chunks, from a ``Cascade`` run (host only):
    per round ``dict(F, C, E0, E, lo, hi, plan)`` -- F frames taken, committed end C, the piece ``[E0, E)`` with
    ``E = hop * max(0, F - A)``, and, when the piece leaves the committed samples, the preview range
    ``[lo, hi) = [max(C, E0), E + X)`` with its ``preview_plan`` (else ``plan`` None)."""
    cas, A, X = Cascade(units, chunk_frames), lookahead_frames, crossfade_samples
    last, E0, C, out = len(units) - 1, 0, 0, []
    for _ in range(rounds):
        for k, _, _, e0, e1 in cas.round(chunk_frames):
            if k == last:
                C += (e1 - e0) * units[k]["stride"]
        F = cas.n[0]
        E = hop * max(0, F - A)
        rec = dict(F=F, C=C, E0=E0, E=E, lo=None, hi=None, plan=None)
        if E > max(C, E0):
            rec["lo"], rec["hi"] = max(C, E0), min(E + X, hop * F)
            rec["plan"] = preview_plan(units, cas.n, cas.e, rec["lo"], rec["hi"])
        out.append(rec)
        E0 = E
    return out


def preview_widths(units, chunk_frames, lookahead_frames, crossfade_samples, hop=256):
    """Widest preview buffer of every unit, in input columns: the schedule repeats once every unit is in its steady
    state (each round then moves every buffer by ``chunk x rate`` columns, a multiple of ``align``), so the maximum over
    the rounds up to four chunks past the first committed sample and past frame A is the maximum for good."""
    reach = -(-sum(u["right"] * hop // u["rate"] for u in units) // hop)
    rounds = (reach + lookahead_frames) // chunk_frames + 5
    widths = [0] * len(units)
    for rec in lookahead_schedule(units, chunk_frames, lookahead_frames, crossfade_samples, rounds, hop):
        for k, b0, end, _, _ in rec["plan"] or []:
            widths[k] = max(widths[k], end - b0)
    return widths


class _Slabs:
    """Batch slabs of M rows per unit (in / out) in one tensor ``mem``, for buffers of ``widths[k]`` columns: what a
    unit launch reads its geometry from.  ``UnitPool`` is its own (committed) instance; the preview pass has a second."""

    def __init__(self, pool, widths, tag):
        self.tag, self.width, self.mem = tag, list(widths), None
        self.ld_in, self.ld_out, self.in_off, self.out_off, self.elems = pool._slab_geometry(widths)


class _Live:
    """One stream of a ``LivePool``: waveform buffer, noise, cascade bookkeeping and its arena slot (``slot``, given by
    ``LivePool.open`` once the stream is known to be valid)."""

    def __init__(self, pool, src_se, tgt_se, noise, seed=None):
        noise_mod.exclusive(seed, noise=noise)
        self.pool, self.slot = pool, None
        self.seed = None if seed is None else noise_mod.check_seed(seed)      # (seed, stream): frames made on demand
        dev = pool.device
        self.cas = Cascade(pool.units, pool.chunk)
        self.wave = WaveBuffer(dev)
        self.noise = noise.to(dev, torch.float32) if noise is not None else None
        if self.noise is not None and (self.noise.dim() != 3 or self.noise.shape[:2] != (1, pool.inter)):
            raise ValueError(f"noise must be [1, {pool.inter}, >= T], got {tuple(self.noise.shape)}")
        eng = pool.engine
        g_src = src_se.to(dev, torch.float32).reshape(1, -1)
        g_tgt = tgt_se.to(dev, torch.float32).reshape(1, -1)
        self.conds = eng.live_conds(g_src, g_tgt)
        if pool.generator == "bf16":        # the bf16 generator's own conv_pre bias row (conv_pre's bias folded in)
            self.conds["d16"] = eng.live_cond_bf16(g_tgt)
        K = len(pool.units)
        self.stored = [0] * K       # executor view: input columns stored = [s0, stored)
        self.s0 = [0] * K
        self.half = [0] * K
        self.closed = False
        self.T = None

    def noise_for(self, f0, nf):
        p = self.pool
        if self.noise is None:
            return torch.randn(p.inter, nf, dtype=torch.float32, device=p.device)
        if self.noise.shape[2] < f0 + nf:
            raise ValueError(f"noise has {self.noise.shape[2]} frames, the stream needs {f0 + nf}")
        return self.noise[0, :, f0:f0 + nf]

    def ready(self):
        """New posterior-encoder frames of the next round (None: no round)."""
        c = self.pool.chunk
        if self.closed:
            return None if self.cas.done else min(c, self.T - self.cas.n[0])
        if interior_frames(self.wave.n, self.pool.n_fft, self.pool.hop) >= self.cas.n[0] + c:
            return c
        return None


class UnitPool:
    """What every pool of cascaded units shares, whatever feeds its first unit (``LivePool``: spectrogram frames of
    pushed audio; ``tts_live.TtsLivePool``: the prior sample of a sentence): the unit table's memory layout (batch
    slabs, one arena slot per stream with two state halves per unit), the record-driven carries, the launch ladder and
    the unit launches themselves.  A stream object brings ``slot``, ``cas`` (its ``Cascade``), ``stored`` / ``s0`` /
    ``half`` per unit and ``conds`` (the conditioning rows its units read).  ``units``: a slice of ``live_units``;
    ``engine``: the ``ConverterEngine`` whose launches the units are."""

    def __init__(self, engine, cfg, units, chunk_frames, max_streams_per_launch, generator="fp32", wavenet=None):
        self.generator = check_generator(generator)
        # the WaveNet layers' kernels of the q / f / r units: None follows the engine's use_bf16_wavenet switch
        self.wavenet = _lib.check_wavenet(wavenet, optional=True)
        self.cfg = cfg
        self.chunk = check_chunk(self.cfg, chunk_frames)
        if getattr(engine, "_bf16_on", False) or getattr(engine, "_split3_on", False):
            raise ValueError("live streams run the fp32 generator only: turn use_bf16_generator / enable_split_bf16x3 off")
        self.engine = engine
        self.device = engine.device
        self.inter = self.cfg["inter_channels"]
        self.spf = samples_per_frame(self.cfg)
        self.ladder = launch_ladder(max_streams_per_launch)
        self.M = self.ladder[-1]
        self.units = units
        self._layout()
        self._free_slots, self._slots = [], 0
        self.mem = None

    def _take_slot(self):
        """An arena slot for a new stream; the arena doubles when none is free (streams already open keep theirs)."""
        if not self._free_slots:
            grown = max(1, 2 * self._slots)
            self._free_slots = list(range(grown - 1, self._slots - 1, -1)) + self._free_slots
            self._slots = grown
            self._ensure_mem()
        return self._free_slots.pop()

    def _run_units(self, plans):
        """The units of one round after its feed: ``plans`` = [(handle, stream, pieces of ``Cascade.round``)] ->
        ``{handle: the last unit's new output columns}``."""
        outputs, acc = {}, 0
        K = len(self.units)
        for h, st, pieces in plans:
            n = sum((e1 - e0) * self.units[k]["stride"] for k, _, _, e0, e1 in pieces if k == K - 1)
            outputs[st] = [acc, 0, h]
            acc += n
        out = torch.empty(acc, dtype=torch.float32, device=self.device)
        for k in range(K):
            items = [(st, p) for h, st, pieces in plans for p in pieces if p[0] == k]
            if not items:
                continue
            self._run_unit(k, items, outputs, out)
        return {o[2]: out[o[0]:o[0] + o[1]] for st, o in outputs.items() if o[1]}

    # ---- memory layout --------------------------------------------------------------------------------------------
    def _slab_geometry(self, widths):
        """Row strides and offsets (elements) of the batch slabs of M rows per unit for buffers of ``widths[k]``
        columns -> ``(ld_in, ld_out, in_off, out_off, total elements)``."""
        pad4 = lambda n: (n + 3) // 4 * 4
        from .engine import padded_frames
        ld_in, ld_out = [], []
        for u, W in zip(self.units, widths):
            if u["kind"] == "g":
                ld_in.append(pad4(W))
                ld_out.append(W * u["stride"])                # dense per launch: ld = L * stride
            else:
                ld_in.append(padded_frames(W))                    # the frame units' workspace layout (ld = Tp)
                ld_out.append(padded_frames(W))
        off, M, in_off, out_off = 0, self.M, [], []
        for k in range(len(self.units)):
            in_off.append(off)
            off += pad4(M * self.rows[k] * ld_in[k])
            out_off.append(off)
            off += pad4(M * self.cout[k] * ld_out[k])
        return ld_in, ld_out, in_off, out_off, off

    def _layout(self):
        """Offsets (elements) in the one device tensor ``mem``: the batch slabs of M rows per unit (in / out) and the
        staging rows of new frames first, then one arena slot per stream (every unit's two state halves)."""
        pad4 = lambda n: (n + 3) // 4 * 4
        cas = Cascade(self.units, self.chunk)
        stages = generator_stages(self.cfg)
        self.rows, self.cap, self.width, self.cout = [], [], [], []
        for k, u in enumerate(self.units):
            self.width.append(cas.width(k))
            self.cap.append(pad4(cas.capacity(k)))
            if u["kind"] == "g":
                st = stages[u["stage"]]
                cin = self.inter if st.index == 0 else st.cin
                cout = 1 if st.last else st.ch
            else:
                cin = self.bins + self.inter if u["kind"] == "q" else self.inter
                cout = self.inter
            self.rows.append(cin)
            self.cout.append(cout)
        self.tag = None                                           # the committed slabs: this pool is its own ``_Slabs``
        self.ld_in, self.ld_out, self.in_off, self.out_off, off = self._slab_geometry(self.width)
        self.stage_ld = pad4(self.chunk)                          # a round appends at most one chunk of frames
        self.stage_off = off
        off += self.M * self.rows[0] * self.stage_ld
        self.arena_off = off
        self.state_off, so = [], 0
        for k in range(len(self.units)):
            self.state_off.append(so)
            so += 2 * self.rows[k] * self.cap[k]
        self.slot_elems = so

    def _state(self, st, k, half):
        return self.arena_off + st.slot * self.slot_elems + self.state_off[k] + half * self.rows[k] * self.cap[k]

    def _ensure_mem(self):
        need = self.arena_off + self._slots * self.slot_elems
        if self.mem is None or self.mem.numel() < need:
            grown = torch.zeros(need, dtype=torch.float32, device=self.device)
            if self.mem is not None:
                grown[:self.mem.numel()].copy_(self.mem)
            self.mem = grown

    # ---- stepping -------------------------------------------------------------------------------------------------
    def _carry(self, recs, dst=None, src=None):
        if not recs:
            return
        dst = self.mem if dst is None else dst
        src = self.mem if src is None else src
        table = torch.tensor(recs, dtype=torch.int64).to(self.device)
        for i in range(0, len(recs), 65535):
            _lib.call("ov_carry_rows_f32", table[i:i + 65535], min(65535, len(recs) - i), src, src.numel(),
                      dst, dst.numel())

    def _batches(self, items, key):
        """Items grouped by ``key`` in order, in launches of up to M, each padded up to a ladder size."""
        groups = {}
        for it in items:
            groups.setdefault(key(it), []).append(it)
        for kv, its in groups.items():
            for i in range(0, len(its), self.M):
                chunk = its[i:i + self.M]
                B = min(b for b in self.ladder if b >= len(chunk))
                yield kv, chunk, B

    def _run_unit(self, k, items, outputs, out):
        """Unit k for ``items`` = [(stream, (k, b0, end, e0, e1))], per launch: one carry gathers the rows' buffers
        (and shifts their kept history into the other state half), the unit runs, one carry scatters the kept output
        columns into unit k + 1's state (the last unit's into ``out``) before the next launch reuses the slab."""
        u = self.units[k]
        for L, chunk, B in self._batches(items, key=lambda it: it[1][2] - it[1][1]):
            rows = chunk + [chunk[-1]] * (B - len(chunk))
            R, ldi = self.rows[k], self.ld_in[k]
            gather, shift = [], []
            for r, (st, (_, b0, end, e0, e1)) in enumerate(rows):
                src = self._state(st, k, st.half[k])
                gather.append((src + (b0 - st.s0[k]), self.in_off[k] + r * R * ldi, R, L, self.cap[k], ldi))
                if r < len(chunk):
                    nb = _start(u, e1)
                    keep = st.stored[k] - nb
                    if keep > 0:
                        shift.append((src + (nb - st.s0[k]), self._state(st, k, 1 - st.half[k]), R, keep, self.cap[k],
                                      self.cap[k]))
            self._carry(gather + shift)
            for st, (_, b0, end, e0, e1) in chunk:
                st.s0[k] = _start(u, e1)
                st.half[k] ^= 1
            self._launch(k, rows, B, L)
            recs = self._scatter(k, chunk, L, outputs)
            if k == len(self.units) - 1:
                self._carry(recs, dst=out)
            else:
                self._carry(recs)

    def _launch(self, k, rows, B, L, lay=None):
        with self.engine.wavenet_scope(self.wavenet):
            self._launch_unit(k, rows, B, L, self if lay is None else lay)

    def _launch_unit(self, k, rows, B, L, lay):
        """Unit k on the first ``B`` rows of ``lay``'s slabs (``lay``: this pool for a committed round, the preview's
        ``_Slabs`` for a preview), ``L`` columns each."""
        u, eng, mem = self.units[k], self.engine, lay.mem
        bf16 = u["kind"] == "g" and self.generator == "bf16"
        key = (u["name"], lay.width[k]) if lay.tag is None else (u["name"], lay.tag, lay.width[k])
        ws = (eng.live_workspace_bf16 if bf16 else eng.live_workspace)(key, B, lay.width[k], stage=u["stage"])
        R, ldi = self.rows[k], lay.ld_in[k]
        x = mem[lay.in_off[k]:]
        out = mem[lay.out_off[k]:]
        cat = lambda t: torch.cat([t_ for t_ in t])
        if u["kind"] == "q":
            self._launch_posterior(k, rows, B, L, ws, lay)
        elif u["kind"] in ("f", "r"):
            key = "src" if u["kind"] == "f" else "tgt"
            conds = [torch.cat([st.conds[key][f] for st, _ in rows]) for f in range(len(rows[0][0].conds[key]))]
            eng.live_flow(x, out, B, L, conds, u["kind"] == "r", ws)
        elif bf16:
            cond = cat([st.conds["d16"] for st, _ in rows]) if u["stage"] == 0 else None
            eng.live_generator_stage_bf16(u["stage"], x, ldi, R * ldi, out, B, L, ws, cond_d=cond)
        else:
            cond = cat([st.conds["d"] for st, _ in rows]) if u["stage"] == 0 else None
            eng.live_generator_stage(u["stage"], x, ldi, R * ldi, out, B, L, ws, cond_d=cond)

    def _scatter(self, k, chunk, L, outputs):
        """Records moving unit k's kept output columns of a launch's rows into unit k + 1's state (or into the round's
        output)."""
        u = self.units[k]
        s = u["stride"]
        last = k == len(self.units) - 1
        recs = []
        C = self.cout[k]
        ldo = L * s if u["kind"] == "g" else self.ld_out[k]
        for r, (st, (_, b0, end, e0, e1)) in enumerate(chunk):
            src = self.out_off[k] + r * C * ldo + (e0 - b0) * s
            n = (e1 - e0) * s
            if last:
                o = outputs[st]
                recs.append((src, o[0] + o[1], 1, n, ldo, n))
                o[1] += n
                continue
            col = st.stored[k + 1] - st.s0[k + 1]
            if col + n > self.cap[k + 1]:
                raise RuntimeError(f"live stream state overflow (unit {self.units[k + 1]['name']})")
            recs.append((src, self._state(st, k + 1, st.half[k + 1]) + col, C, n, ldo, self.cap[k + 1]))
            st.stored[k + 1] += n
        return recs


class LivePool(UnitPool, PushedPool):
    """Many live streams stepped together (see the module docstring).  ``open(src_se, tgt_se, noise=None)`` -> handle;
    ``push(h, samples)`` buffers; ``step()`` runs every stream with a ready chunk (and every closed stream's remaining
    rounds) -> ``{handle: newly finished samples}`` (device tensors); ``close(h)`` marks the end of h's input.  Rounds:
    every ready stream advances by one chunk per round, each unit runs its streams' buffers in launches of up to
    ``max_streams_per_launch`` rows grouped by buffer width (steady-state streams share one width; a stream's first
    rounds and its end run narrower), padded up to the ``launch_ladder`` sizes.  ``tau`` is the pool's default;
    ``open(..., tau=)`` gives a stream its own, kept for life, and the rows of a posterior-encoder launch each carry
    their stream's (``ov_conv1d_params.scale_b``; a launch whose rows agree is the scalar launch it always was).
    Live units run eagerly, never from a captured graph.  ``generator``: ``"fp32"`` (default) or ``"bf16"`` -- the
    kernels of the ``g`` units (module docstring); everything else, the latency and the state size included, is the
    same for both.  ``wavenet``: None (follow ``ConverterEngine.use_bf16_wavenet``), ``"fp32"`` or ``"bf16"`` -- the
    WaveNet layers of the ``q`` / ``f`` / ``r`` units on ``ov_wn_layer_bf16`` (bf16 matrix operands, fp32 state); the
    layer's results do not depend on tile, row or batch, so a stream still equals the one-pass conversion with the same
    keyword.  ``lookahead_frames`` = A (None: all of the above, unchanged): the pool emits ``[0, hop * max(0, F - A))``
    of every stream once it has taken F interior frames -- each round's piece is that piece of the one-pass conversion of
    the first F frames, from a preview pass after the committed units (``_emit_ahead``, ``preview_plan``); committed
    state is never built from previewed columns, and ``close`` is exact.  ``crossfade_samples`` = X blends the first X
    samples of a piece with the previous preview's (``ov_crossfade_rows_f32``); the default, ``min(hop, hop * A)``, has
    not been measured on a real voice.  Cost (chunk 15): a tick takes 1.6 - 1.9 x the plain one at
    A = 0, 15 and 45 alike.  Streams of one pool that still fit a 100 ms tick on one GPU: 256 on fp32 at each A (90 ms
    at A = 0, 96 - 97 ms at 15 and 45, measured: the practical limit; 52 ms plain), and 256 on bf16 with half the tick
    to spare (51 - 54 ms; about 480 - 500 extrapolated from the cost per added stream, not run)."""

    def __init__(self, model, tau=0.3, chunk_frames=DEFAULT_CHUNK_FRAMES,
                 max_streams_per_launch=DEFAULT_LIVE_STREAMS_PER_LAUNCH, n_fft=1024, hop=256, model_sr=rates.MODEL_RATE,
                 generator="fp32", wavenet=None, lookahead_frames=None, crossfade_samples=None, watermark_model=None):
        self.model, self.tau = model, float(tau)
        self.watermark_model = watermark_model      # the converter's: what open(message=) marks with
        self.lookahead = check_lookahead(lookahead_frames)
        self._tau_rows = {}         # taus of a launch's rows -> their float32 device vector (uploaded once)
        self.n_fft, self.hop, self.pad = int(n_fft), int(hop), (int(n_fft) - int(hop)) // 2
        self.bins = self.n_fft // 2 + 1
        check_generator(generator), _lib.check_wavenet(wavenet, optional=True), check_chunk(model.model_cfg, chunk_frames)
        super().__init__(model.engine(), model.model_cfg, live_units(model.model_cfg), chunk_frames,
                         max_streams_per_launch, generator=generator, wavenet=wavenet)
        self._core_latency = live_latency_samples(self.cfg, self.chunk, self.n_fft, self.hop, self.lookahead)
        self.crossfade = check_crossfade(crossfade_samples, self.lookahead, self.chunk, self.hop)
        # look-ahead streams whose frontier stays inside the committed samples never run a preview
        self._pv = self._fade = self._fade_w = None               # preview slabs, seam buffer, fade-in weights (lazy)
        self._init_streams(self.device, model_sr)

    @property
    def latency_samples(self):
        """The bound at the model rate: ``live_latency_samples``, plus ``H - 1`` samples of the longest hold among the
        open streams that carry a message (``latency_of(h)`` is stream h's own)."""
        return self._core_latency + self._hold_wait()

    def state_bytes_per_stream(self):
        """Device bytes one open stream adds: its arena slot (every unit's two state halves) and its conditioning rows
        (the WaveNet gate biases of the posterior encoder and of both flow directions, the generator's cond bias).  Its
        waveform buffer (>= 256 KiB, trimmed to the frames still to come) and an explicit noise tensor come on top.
        5.6 MB at 15 frames for the released configurations."""
        H, cfg = self.cfg["hidden_channels"], self.cfg
        conds = 2 * H * ENC_Q_LAYERS + 2 * N_FLOWS * 2 * H * FLOW_LAYERS + cfg["upsample_initial_channel"]
        return 4 * (self.slot_elems + conds)

    # ---- streams --------------------------------------------------------------------------------------------------
    def open(self, src_se, tgt_se, noise=None, sr_in=None, sr_out=None, *, seed=None, tau=None, message=None,
             watermark_hold=watermark_mod.DEFAULT_HOLD, message_repeat=False):
        """A new stream -> its handle.  ``tau``: None = the pool's, else this stream's own number, for life.
        ``message`` (None: unmarked, today's path): the stream's output carries the block-wise native watermark of it
        (``watermark.py``, "streams"), made at the model rate after the crossfade and before the output resampler, all
        marked streams of a step in one launch; ``watermark_hold`` = H, one of ``watermark.HOLDS``: a sample leaves at
        most H - 1 samples later; ``message_repeat``: window n carries group n % G for the stream's life instead of
        the first G windows only.  ValueError for a message on a pool whose converter has no native watermark.
        ``sr_in`` / ``sr_out``: the rate of its pushes / of its output (None or the
        model rate: no resampler in that direction).  ``noise`` ``[1, inter, >= T]``, or ``seed`` (an int: stream
        ``(seed, 0)``, or a pair): counter-based noise (``noise.py``) generated chunk by chunk into the staging rows --
        the stream then equals ``convert_long(seed=...)`` of its whole input whatever the push sizes and whoever shares
        the pool, and holds no noise tensor; neither: drawn from torch's generator per chunk."""
        noise_mod.exclusive(seed, noise=noise)
        tau = self._stream_tau(tau, "LivePool.open")
        mark = watermark_mod.stream_mark(self.watermark_model, message, watermark_hold, message_repeat)
        sr_in, sr_out = rates.check_rate(sr_in, "sr_in"), rates.check_rate(sr_out, "sr_out")
        st = _Live(self, src_se, tgt_se, noise, seed=seed)
        st.tau, st.mark = tau, mark
        st.E = st.C = 0             # look-ahead: samples emitted / committed so far
        st.pend, st.pend_n = [], 0  # committed samples past the emitted ones, oldest first
        st.has_tail = False         # the last preview's samples [E, E + X) are kept in this stream's seam slot
        st.slot = self._take_slot()         # nothing after this raises: a failed open leaves the pool as it was
        return self._register(st, sr_in, sr_out)

    def latency_of(self, h):
        """``(seconds, samples)``: the latency bound of stream h at its own rates (``rates.stream_latency``; samples in
        its output rate, ``latency_samples`` when it resamples nothing)."""
        st = self._stream(h)
        return rates.stream_latency(self._core_latency, self.model_sr, st.sr_in, st.sr_out,
                                    hold_samples=watermark_mod.hold_wait(st.mark))

    def close(self, h):
        """End of h's input; too short an input raises ValueError here and retires h (the others are untouched)."""
        n = self._end_input(h)
        st = self._streams[h]
        try:
            st.T = stream_end_frames(n, self.n_fft, self.hop)
            if st.noise is not None and st.noise.shape[2] < st.T:
                raise ValueError(f"noise has {st.noise.shape[2]} frames, the stream needs {st.T}")
        except ValueError:
            self._retire(h)
            raise

    def _released(self, st):
        self._free_slots.append(st.slot)

    def _feed(self, jobs):
        """New posterior-encoder frames of every ready stream: the spectrogram of frames [n_q, n_q + nf) of its
        waveform (bit-identical to the whole file's) and its noise into the staging rows, then carried onto the end of
        the stream's posterior state."""
        from .mel_processing import native_spectrogram
        spec_eng = native_spectrogram(self.device, self.n_fft, self.hop)
        bins, rows0, sld = self.bins, self.rows[0], self.stage_ld
        for nf, chunk, _ in self._batches([j for j in jobs if j[1] > 0], key=lambda j: j[1]):
            srcs, recs, acc = [], [], 0
            for st, _, f0 in chunk:
                srcs.append(st.wave.valid())
                recs.append((acc, st.wave.len, f0 - st.wave.base // self.hop))
                acc += st.wave.len
            pool = srcs[0] if len(srcs) == 1 else torch.cat(srcs)
            rec_dev = torch.tensor(recs, dtype=torch.int64).to(self.device)
            spec = spec_eng.windows_multi(pool, rec_dev, nf)
            W = len(chunk)
            stage = self.mem[self.stage_off:self.stage_off + W * rows0 * sld].view(W, rows0, sld)
            stage[:, :bins, :nf].copy_(spec)
            if all(st.seed is None for st, _, _ in chunk):
                stage[:, bins:, :nf].copy_(torch.stack([st.noise_for(f0, nf) for st, _, f0 in chunk]))
            else:
                # every seeded stream of the launch in ONE fill launch, straight into its staging rows; the others copy
                fills = []
                for w, (st, _, f0) in enumerate(chunk):
                    if st.seed is None:
                        stage[w, bins:, :nf].copy_(st.noise_for(f0, nf))
                    else:
                        fills.append(st.seed + (noise_mod.PURPOSE_POSTERIOR, f0, nf,
                                                self.stage_off + (w * rows0 + bins) * sld, sld))
                noise_mod.fill(fills, self.inter, self.mem)
            carry = []
            for w, (st, _, f0) in enumerate(chunk):
                k = 0
                col = st.stored[k] - st.s0[k]
                if col + nf > self.cap[k]:
                    raise RuntimeError("live stream state overflow (unit q)")
                carry.append((self.stage_off + w * rows0 * sld, self._state(st, k, st.half[k]) + col, rows0, nf, sld,
                              self.cap[k]))
                st.stored[k] += nf
            self._carry(carry)

    def _launch_posterior(self, k, rows, B, L, ws, lay):
        R, ldi, ldo, C, mem = self.rows[k], lay.ld_in[k], lay.ld_out[k], self.cout[k], lay.mem
        cond = torch.cat([st.conds["q"] for st, _ in rows])
        self.engine.live_posterior(mem[lay.in_off[k]:], ldi, R * ldi, mem[lay.in_off[k] + self.bins * ldi:], R * ldi,
                                   mem[lay.out_off[k]:], ldo, C * ldo, B, L, cond, self._launch_tau(rows), ws)

    def _launch_tau(self, rows):
        """``tau`` of a posterior-encoder launch: the number when its rows agree, else their per-row device vector --
        uploaded the first time this combination of rows is launched, so a steady pool uploads nothing per tick."""
        tau = rows_tau([st.tau for st, _ in rows])
        if isinstance(tau, float):
            return tau
        key = tuple(tau)
        vec = self._tau_rows.get(key)
        if vec is None:
            if len(self._tau_rows) >= 256:          # pools whose membership keeps changing: start over, stay bounded
                self._tau_rows.clear()
            vec = self._tau_rows[key] = torch.tensor(tau, dtype=torch.float32).to(self.device)
        return vec

    @torch.no_grad()
    def _round(self, streams):
        """One round: every stream in ``streams`` ([(h, st, new_frames)]) advances by one chunk (or its end)."""
        jobs, plans = [], []
        for h, st, nf in streams:
            f0 = st.cas.n[0]
            plans.append((h, st, st.cas.round(nf, final=st.closed and f0 + nf == st.T)))
            jobs.append((st, nf, f0))
        if self.lookahead is not None:       # a regular round: a whole chunk of interior frames, closed or not
            for st, nf, f0 in jobs:
                st.regular = nf == self.chunk and f0 + nf <= interior_frames(st.wave.n, self.n_fft, self.hop)
        self._feed(jobs)
        for st, nf, f0 in jobs:
            if not st.closed:           # no later frame reads before the reflect padding of the next one
                st.wave.trim(st.cas.n[0], self.hop, self.pad)
        outs = self._run_units(plans)
        return outs if self.lookahead is None else self._emit_ahead(streams, outs)

    # ---- bounded look-ahead ---------------------------------------------------------------------------------------
    def _seam_layout(self):
        """One seam slot per arena slot in ``_fade``: ``[tail: X | piece area]``, the piece area holding a round's new
        piece and the X samples after it (the next tail); the longest piece is the one at ``close``."""
        X, pad4 = self.crossfade, lambda n: (n + 3) // 4 * 4
        self.tail_ld = pad4(X)
        self.seam_elems = self.tail_ld + pad4((self.lookahead + 2 * self.chunk + 8) * self.hop + X)
        need = self._slots * self.seam_elems
        if self._fade is None or self._fade.numel() < need:
            grown = torch.zeros(need, dtype=torch.float32, device=self.device)
            if self._fade is not None:
                grown[:self._fade.numel()].copy_(self._fade)
            self._fade = grown
        if self._fade_w is None:
            self._fade_w = crossfade_weights(X).to(self.device)

    def _emit_ahead(self, streams, outs):
        """What the streams of a round emit under ``lookahead_frames``: ``outs`` = the round's committed samples ->
        ``{handle: the piece [E_{n-1}, E_n)}``.  Committed samples past the frontier wait in ``pend``; a piece takes them
        first and the rest from a preview of what the stream holds (``_preview``); the first X samples of a piece that
        begins past the committed samples, and of a closed stream's rest, are blended with the previous preview's
        (``ov_crossfade_rows_f32``, one launch for the round).  A closed stream's last
        rounds (reflect-padded frames) emit nothing until its cascade is done, then everything committed."""
        A, X, hop = self.lookahead, self.crossfade, self.hop
        res, jobs = {}, []
        for h, st, nf in streams:
            com = outs.get(h)
            if com is not None:
                k = max(0, st.E - st.C)                 # already emitted from previews
                if k < com.numel():
                    st.pend.append(com[k:])
                    st.pend_n += com.numel() - k
                st.C += com.numel()
            if st.regular:
                E = hop * max(0, st.cas.n[0] - A)
            elif st.cas.done:
                E = st.C
            else:
                continue
            if E <= st.E:
                continue
            m = min(st.pend_n, E - st.E)
            head = None
            if m:
                pend = st.pend[0] if len(st.pend) == 1 else torch.cat(st.pend)
                head, rest = pend[:m], pend[m:]
                st.pend, st.pend_n = ([rest] if rest.numel() else []), rest.numel()
            # the seam: a piece that begins inside committed samples is exact there and is not blended (old = new);
            # the rest of a closed stream is blended with the last preview's tail like any previewed piece
            st.fade = st.has_tail and (m == 0 or not st.regular)
            if st.E + m == E and not st.fade:           # committed samples only, no seam: no launch
                st.has_tail = False
                res[h], st.E = head, E
                continue
            jobs.append((h, st, E, head))
        if not jobs:
            return res
        self._seam_layout()
        total, recs, keep, previews = 0, [], [], []
        for h, st, E, head in jobs:
            base = st.slot * self.seam_elems
            new, m, n = base + self.tail_ld, 0 if head is None else head.numel(), E - st.E
            if n + X > self.seam_elems - self.tail_ld:
                raise RuntimeError("live stream seam overflow")
            if m:
                self._fade[new:new + m].copy_(head)
            lo = st.E + m
            if lo < E:                                  # the piece leaves the committed samples: preview [lo, E + X)
                hi = min(E + X, hop * st.cas.n[0])
                previews.append((st, lo, hi, new + m))
                if X and hi - E == X:
                    keep.append((new + n, base, 1, X, X, X))
            recs.append((base, new, total, n, X if st.fade else 0))
            st.has_tail = lo < E and X > 0 and hi - E == X
            st.E = E
            total += n
        self._preview(previews)
        out = torch.empty(total, dtype=torch.float32, device=self.device)
        table = torch.tensor(recs, dtype=torch.int64).to(self.device)
        _lib.call("ov_crossfade_rows_f32", table, len(recs), self._fade_w, self._fade_w.numel(), self._fade,
                  self._fade.numel(), out, total)
        self._carry(keep, dst=self._fade, src=self._fade)          # the next tails, after this round's were read
        for (h, st, E, head), r in zip(jobs, recs):
            res[h] = out[r[2]:r[2] + r[3]]
        return res

    def _preview(self, jobs):
        """``jobs`` = [(stream, lo, hi, dst)]: the samples ``[lo, hi)`` of each stream's conversion as if its input
        ended with the frames it holds, written to ``_fade[dst:]``.  Every unit of its ``preview_plan`` runs through
        ``_launch_unit`` on slabs of the preview's own (``_pv``): the stored part of a buffer is gathered from the arena
        as it is -- no history shift, no write to the arena -- and the rest is what the unit before handed on.  Streams
        whose plans have the same buffer widths share launches, on the pool's ladder."""
        if not jobs:
            return
        if self._pv is None:
            widths = preview_widths(self.units, self.chunk, self.lookahead, self.crossfade, self.hop)
            self._pv = _Slabs(self, widths, "preview")
            self._pv.mem = torch.zeros(self._pv.elems, dtype=torch.float32, device=self.device)
        pv, K = self._pv, len(self.units)
        plans = [(st, preview_plan(self.units, st.cas.n, st.cas.e, lo, hi), dst) for st, lo, hi, dst in jobs]
        for sig, chunk, B in self._batches(plans, key=lambda p: tuple((k, end - b0) for k, b0, end, _, _ in p[1])):
            rows = chunk + [chunk[-1]] * (B - len(chunk))
            for i, (k, L) in enumerate(sig):
                if L > pv.width[k]:
                    raise RuntimeError(f"live preview wider than its slab (unit {self.units[k]['name']})")
                R, ldi, C, s = self.rows[k], pv.ld_in[k], self.cout[k], self.units[k]["stride"]
                gather = []
                for r, (st, plan, _) in enumerate(rows):
                    b0 = plan[i][1]
                    n = min(plan[i][2], st.stored[k]) - b0
                    if n > 0:
                        gather.append((self._state(st, k, st.half[k]) + (b0 - st.s0[k]), pv.in_off[k] + r * R * ldi, R, n,
                                       self.cap[k], ldi))
                self._carry(gather, dst=pv.mem)
                self._launch(k, [(st, None) for st, _, _ in rows], B, L, pv)
                ldo = L * s if self.units[k]["kind"] == "g" else pv.ld_out[k]
                hand = []
                for r, (st, plan, dst) in enumerate(rows):
                    _, b0, _, olo, ohi = plan[i]
                    src = pv.out_off[k] + r * C * ldo + (olo - b0 * s)
                    if k < K - 1:
                        nb0, ldn = plan[i + 1][1], pv.ld_in[k + 1]
                        hand.append((src, pv.in_off[k + 1] + r * C * ldn + (olo - nb0), C, ohi - olo, ldo, ldn))
                    elif r < len(chunk):
                        hand.append((src, dst, 1, ohi - olo, ldo, ohi - olo))
                self._carry(hand, dst=pv.mem if k < K - 1 else self._fade, src=pv.mem)

    @torch.no_grad()
    def step(self):
        """Rounds until no stream has a ready chunk; closed streams run to their end and are retired.  Streams with an
        input rate of their own first receive their new input at the model rate (one resampler launch for all of
        them); streams with an output rate of their own get theirs resampled after the rounds (one more launch)."""
        self._take_input()
        res, routs = {}, self._output_rates()
        while True:
            ready = [(h, st, st.ready()) for h, st in self._streams.items()]
            ready = [r for r in ready if r[2] is not None]
            if not ready:
                break
            for h, o in self._round(ready).items():
                res.setdefault(h, []).append(o)
            for h, st, _ in ready:
                if st.closed and st.cas.done:
                    self._retire(h, finished=True)
        out = {h: (v[0] if len(v) == 1 else torch.cat(v)) for h, v in res.items()}
        return self._deliver(out, routs)


class LiveStream:
    """One live stream (a ``LivePool`` of one): ``push(samples)`` -> newly finished samples (device tensor, possibly
    empty), ``close()`` -> the rest, ``latency_samples`` the bound no output sample's delay exceeds (in output samples;
    ``latency_seconds`` the same bound in seconds).  ``sr_in`` / ``sr_out``: rates of the pushes / of the output (None:
    the model rate).  ``generator``: as for ``LivePool``.  ``message`` / ``watermark_hold`` / ``message_repeat``: as for
    ``LivePool.open``, marked with ``watermark_model``; the latency figures include the hold."""

    def __init__(self, model, src_se, tgt_se, tau=0.3, chunk_frames=DEFAULT_CHUNK_FRAMES, noise=None, n_fft=1024,
                 hop=256, sr_in=None, sr_out=None, model_sr=rates.MODEL_RATE, generator="fp32", seed=None, wavenet=None,
                 lookahead_frames=None, crossfade_samples=None, watermark_model=None, message=None,
                 watermark_hold=watermark_mod.DEFAULT_HOLD, message_repeat=False):
        noise_mod.exclusive(seed, noise=noise)
        self._pool = LivePool(model, tau=tau, chunk_frames=chunk_frames, max_streams_per_launch=1, n_fft=n_fft, hop=hop,
                              model_sr=model_sr, generator=generator, wavenet=wavenet, lookahead_frames=lookahead_frames,
                              crossfade_samples=crossfade_samples, watermark_model=watermark_model)
        self._h = self._pool.open(src_se, tgt_se, noise=noise, sr_in=sr_in, sr_out=sr_out, message=message,
                                  watermark_hold=watermark_hold, message_repeat=message_repeat, **noise_mod.kw(seed))
        self.latency_seconds, self.latency_samples = self._pool.latency_of(self._h)
        self._closed = False

    def _out(self, res):
        o = res.get(self._h)
        return o if o is not None else torch.empty(0, dtype=torch.float32, device=self._pool.device)

    def push(self, samples):
        if self._closed:
            raise RuntimeError("push() after close()")
        self._pool.push(self._h, samples)
        return self._out(self._pool.step())

    def close(self):
        if self._closed:
            raise RuntimeError("close() called twice")
        self._closed = True
        self._pool.close(self._h)
        return self._out(self._pool.step())
