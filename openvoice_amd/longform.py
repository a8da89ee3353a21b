"""Recordings of any length: overlapping fixed-size windows (``WindowedConverter``) and a streaming converter
(``ConversionStream``).

The one-pass path (``ToneColorConverter.convert``, reference: openvoice/api.py:141-160) converts a file as ONE utterance:
its workspace grows with the file (~0.3 MB per frame at batch 1) and the generator's per-utterance 32-bit offsets
refuse a file of 63 551 frames (12.3 min at 22.05 kHz; ``one_pass_limit_frames``).  The model itself does not need the whole file:
its receptive field is bounded (``context_frames``), so windows of a fixed length that overlap by that much context
reproduce the one-pass result on their cores:

* device memory is bounded by the window size, not by the file length, and there is no length ceiling;
* the same window grid serves a stream whose converted audio comes out after a fixed delay.

A window is a batch item of the unchanged ``voice_conversion`` (reference: openvoice/models.py:492-499) with
``spec_lengths = Tw``; its spectrogram is framed straight out of the long waveform (``ov_frame_hops_windows_f32`` + the
K = 4 framing conv of ``mel_processing``), so it equals ``spectrogram_torch(whole)[:, :, f0:f0 + Tw]`` bit for bit; its
core samples are copied into the long output by ``ov_stitch_window_cores_f32``.

Many sources share launches: ``StreamPool`` steps many live streams and ``WindowedConverter.convert_many`` converts many
recordings, both framing every window of a launch from its own source span (``ov_frame_hops_multi_f32``) and stitching
the cores into one packed output.
"""
import math

import torch

from . import _lib, rates
from .engine import item_tau, rows_tau, wavenet_keyword
from . import noise as noise_mod
from . import stretch as stretch_mod
from .streams import PushedPool, WaveBuffer
from . import watermark as watermark_mod
from .generator import GENERATOR_MARGIN, generator_margin_frames, generator_stages, samples_per_frame
from .params import ENC_Q_KERNEL, ENC_Q_LAYERS, FLOW_KERNEL, FLOW_LAYERS, N_FLOWS

# Defaults, picked with tools/bench_long.py (profiles/r07_bench_long.jsonl, 20 min file): 8192-frame windows (95 s, 3 % of
# the frames computed twice), two per launch -- 20.7 ms per minute of audio at 3.5 GiB peak, the peak of 4096 x 4 (21.4 ms)
# and within 7 % of one pass (19.3-20.1 ms); 8192 x 4 gains 2.5 % more for 6.2 GiB.  Beyond the fixed workspace a file
# costs its waveform, output and noise: 8 bytes per sample + 768 per frame (2.8 KB per frame; one pass: ~0.3 MB).
DEFAULT_WINDOW_FRAMES = 8192
DEFAULT_WINDOWS_PER_LAUNCH = 2
# streams: the window sets the latency (256 Tw + 384 samples): 11.9 s at 1024 frames, ~980x real time
DEFAULT_STREAM_WINDOW_FRAMES = 1024
# StreamPool: windows per launch at most (the ladder of launch sizes is the powers of two below it, and it)
DEFAULT_POOL_WINDOWS_PER_LAUNCH = 32
# convert_many: windows per launch
DEFAULT_MANY_WINDOWS_PER_LAUNCH = 8


def winograd_grid_frames(cfg):
    """Smallest G (frames) such that a shift of the input by a multiple of G frames moves every Winograd tile of every
    generator stage by a whole number of tiles: a tile covers 4 * dil columns at its stage's rate, so G * rate must be a
    multiple of lcm(4 * dil) over the dilations of that stage (1 for the convs2, the configured ones for the convs1).
    15 for the released configurations (stage 0: lcm(4, 12, 20) = 60 columns at 8 columns per frame)."""
    tile = 4
    for d in [1] + [v for dl in cfg["resblock_dilation_sizes"] for v in dl]:
        tile = tile * 4 * d // math.gcd(tile, 4 * d)
    g = 1
    for st in generator_stages(cfg):
        gi = tile // math.gcd(tile, st.rate_out)
        g = g * gi // math.gcd(g, gi)
    return g


def context_frames(cfg):
    """One-sided reach, in frames, of a whole conversion (spectrogram frames + noise -> waveform), rounded up to the
    window grid (``winograd_grid_frames``): the posterior encoder's WaveNet (reference: openvoice/models.py:442-448,
    16 layers of kernel 5, dilation 1: 32 frames), the flow forward and reverse (models.py:374-397: 4 couplings x 4 WN
    layers of kernel 5 each way: 2 x 32) and the generator (``max(GENERATOR_MARGIN, generator_margin_frames(cfg))``: 16).
    112 -> 120 for the released configurations."""
    reach = ENC_Q_LAYERS * (ENC_Q_KERNEL - 1) // 2
    reach += 2 * N_FLOWS * FLOW_LAYERS * (FLOW_KERNEL - 1) // 2
    reach += max(GENERATOR_MARGIN, generator_margin_frames(cfg))
    g = winograd_grid_frames(cfg)
    return -(-reach // g) * g


def frame_reach_frames():
    """One-sided reach, in frames, of the frame-rate part of a conversion -- the posterior encoder's WaveNet and the
    flow forward and reverse (``context_frames`` without the generator's term): 96."""
    return ENC_Q_LAYERS * (ENC_Q_KERNEL - 1) // 2 + 2 * N_FLOWS * FLOW_LAYERS * (FLOW_KERNEL - 1) // 2


def generator_context_frames(cfg):
    """The generator's term of ``context_frames``: ``max(GENERATOR_MARGIN, generator_margin_frames(cfg))`` frames AT THE
    GENERATOR'S INPUT RATE -- output frames of a stretched conversion."""
    return max(GENERATOR_MARGIN, generator_margin_frames(cfg))


def stretch_context_frames(cfg, step):
    """``context_frames`` of a conversion whose latent is stretched by ``step`` in front of the generator
    (``stretch.context_frames``): the generator's reach is counted in OUTPUT frames, which are ``speed`` source frames
    each, so the source-frame context grows with ``max(1, speed)``; 120 at speed <= 1, 150 at speed 2."""
    return stretch_mod.context_frames(frame_reach_frames(), generator_context_frames(cfg), step, winograd_grid_frames(cfg))


def plan_windows(T, window_frames, context, grid=1):
    """Window records ``(first_frame, core_lo, core_hi)`` for a file of ``T`` frames.

    * Every window has ``window_frames`` frames (one workspace shape for the whole file), except when
      ``T <= window_frames``: then one window of ``T`` frames, the one-pass conversion.
    * The cores partition ``[0, T)`` in order; the first window starts at 0 and the last one ends exactly at ``T``
      (shifted left over its neighbour: never padded past ``T``, where an unmasked generator would see bias-driven
      frames instead of the zero padding of a one-pass run).
    * Every core edge that is not a file edge has at least ``context`` frames of real input beyond it.
    * Regular window k starts at ``k * core`` (``core`` = the largest multiple of ``grid`` <= ``window_frames - 2 *
      context``) and keeps ``[k * core + context, (k + 1) * core + context)`` (window 0 from 0); it is in the plan iff
      it ends before ``T``, so the regular windows of a length are a prefix of those of any longer length (what
      ``ConversionStream`` relies on).  The last window starts at ``T - window_frames``."""
    T, Tw, ctx, grid = int(T), int(window_frames), int(context), int(grid)
    if T < 1:
        raise ValueError(f"plan_windows: T = {T} frames")
    if T <= Tw:
        return [(0, 0, T)]
    core = window_core(Tw, ctx, grid)
    plan, k = [], 0
    while k * core + Tw < T:
        f0 = k * core
        plan.append((f0, 0 if k == 0 else f0 + ctx, f0 + ctx + core))
        k += 1
    plan.append((T - Tw, plan[-1][2] if plan else 0, T))
    return plan


def window_core(window_frames, context, grid=1):
    """Frames a regular window keeps: the largest multiple of ``grid`` that leaves ``context`` frames on both sides."""
    core = (int(window_frames) - 2 * int(context)) // int(grid) * int(grid)
    if core < 1:
        raise ValueError(f"window of {window_frames} frames leaves no core with {context} frames of context on each side "
                         f"(grid {grid}): use at least {2 * context + grid} frames")
    return core


def one_pass_limit_frames(cfg):
    """Smallest T whose one-pass conversion a generator launch refuses with OV_E_BADARG, from the launchers' own checks:
    ``ov_conv1d_f32`` once an utterance's input rows (Cin x x_ld) or output rows ((M + 32) x out_ld) span 2^32 elements,
    ``ov_conv1d_wino_f32`` once Cout x out_ld reaches 2^31.  The binding launch of the released configuration is stage
    1's ConvTranspose (M = 128 channels x 8 phase rows, out_ld = 64 T): 1056 x 64 T >= 2^32 at T = 63 551 frames
    (12.3 min at 22.05 kHz); the Winograd bound alone would be 262 144 frames (50.7 min)."""
    u32, s32 = (1 << 32) - 1, (1 << 31) - 1
    checks = []                                    # (elements per frame, largest accepted element count)
    for _, cin, ch, u, rate_in, rate, _ in generator_stages(cfg):
        checks.append((cin * rate_in, u32))                      # ConvTranspose (phase conv) input rows
        checks.append(((ch * u + 32) * rate, u32))               # ... its ch x u phase rows of L x u columns
        checks += [(ch * rate, u32), ((ch + 32) * rate, u32)]    # direct ResBlock convs
        checks.append((ch * rate, s32))                          # Winograd ResBlock convs
    return min(bound // per_frame + 1 for per_frame, bound in checks)


def launch_ladder(max_windows):
    """Launch sizes of a ``StreamPool``: the powers of two below ``max_windows``, and ``max_windows`` itself."""
    m = int(max_windows)
    if m < 1:
        raise ValueError(f"max_windows_per_launch = {max_windows}")
    ladder, b = [], 1
    while b < m:
        ladder.append(b)
        b *= 2
    return ladder + [m]


def frames_of(n_samples, n_fft, hop):
    """Frames of ``spectrogram_torch`` (center=False, reflect pad (n_fft - hop) / 2) for ``n_samples``."""
    pad = (n_fft - hop) // 2
    return (int(n_samples) + 2 * pad - n_fft) // hop + 1


def stream_end_frames(n_samples, n_fft, hop):
    """Frames ``T`` of a stream that ended after ``n_samples`` samples; ValueError for input shorter than the reflect
    padding or one frame, like ``spectrogram_torch``."""
    if (int(n_fft) - int(hop)) // 2 >= n_samples:
        raise ValueError("waveform shorter than the reflect padding")       # spectrogram_torch raises too
    T = frames_of(n_samples, n_fft, hop)
    if T < 1:
        raise ValueError("waveform shorter than one frame")
    return T


class WindowedConverter:
    """Runs a window plan through ``SynthesizerTrn.voice_conversion`` in launches of up to ``windows_per_launch``
    windows.  ``graph=True`` replays each launch shape from a captured HIP graph (the window shape is fixed, so a file
    captures at most three shapes: full batches, the last partial batch, and the single-window case)."""

    def __init__(self, model, n_fft=1024, hop=256, window_frames=DEFAULT_WINDOW_FRAMES,
                 windows_per_launch=DEFAULT_WINDOWS_PER_LAUNCH, graph=False, model_sr=rates.MODEL_RATE, wavenet=None,
                 watermark_model=None):
        self.model = model
        self.watermark_model = watermark_model      # the converter's: what a stream opened with message= marks with
        # the WaveNet layers' kernels of every launch of THIS converter (its streams and pools included): None follows
        # the engine's use_bf16_wavenet switch or the running call's wavenet=
        self.wavenet = _lib.check_wavenet(wavenet, optional=True)
        self.model_sr = int(model_sr)
        self.cfg = model.model_cfg
        self.n_fft, self.hop, self.pad = int(n_fft), int(hop), (int(n_fft) - int(hop)) // 2
        self.window_frames = int(window_frames)
        self.windows_per_launch = int(windows_per_launch)
        if self.windows_per_launch < 1:
            raise ValueError(f"windows_per_launch = {windows_per_launch}")
        self.graph = bool(graph)
        self.grid = winograd_grid_frames(self.cfg)
        self.context = context_frames(self.cfg)
        self.core = window_core(self.window_frames, self.context, self.grid)
        self.spf = samples_per_frame(self.cfg)
        self.inter = self.cfg["inter_channels"]

    def _device(self):
        return next(self.model.parameters()).device

    def _spectrogram(self):
        from .mel_processing import native_spectrogram
        return native_spectrogram(self._device(), self.n_fft, self.hop)

    def _launch(self, wave, n_samples, plan_dev, firsts_dev, Tw, src_se, tgt_se, tau, nz, out, out_frame0, seed=None):
        """One launch of W = len(firsts_dev) windows: framing -> spectrogram -> voice_conversion -> their cores into
        ``out`` (``plan_dev`` [W, 3] int64 records, ``nz`` [W, inter, Tw] noise, or ``seed``: one ``(seed, stream, first
        frame)`` per window, generated inside ``voice_conversion``)."""
        W = firsts_dev.shape[0]
        spec = self._spectrogram().windows(wave, n_samples, firsts_dev, Tw)
        lengths = torch.full((W,), Tw, dtype=torch.int64, device=wave.device)
        o_hat = self.model.voice_conversion(spec, lengths, sid_src=src_se, sid_tgt=tgt_se, tau=tau, noise=nz,
                                            graph=self.graph, **noise_mod.kw(seed), **_lib.wavenet_kw(self.wavenet))[0]
        _lib.call("ov_stitch_window_cores_f32", o_hat, plan_dev, W, Tw, self.spf, out, out.numel(), out_frame0)

    def _launch_multi(self, pool, records_dev, Tw, src_se, tgt_se, tau, nz, out, stitch_dev, n_out, seed=None,
                      generator=None):
        """One launch of W = len(records_dev) windows, each from its own span of ``pool`` (``records_dev`` [W, 3] int64
        (base, n_samples, first_frame)): framing -> spectrogram -> voice_conversion with per-window embedding rows ->
        the cores of the first ``n_out`` windows into the packed ``out`` (``stitch_dev`` [n_out, 3] virtual records,
        out_frame0 = 0); rows past ``n_out`` pad the launch to a ladder size and their output is dropped."""
        W = records_dev.shape[0]
        spec = self._spectrogram().windows_multi(pool, records_dev, Tw)
        lengths = torch.full((W,), Tw, dtype=torch.int64, device=pool.device)
        o_hat = self.model.voice_conversion(spec, lengths, sid_src=src_se, sid_tgt=tgt_se, tau=tau, noise=nz,
                                            graph=self.graph, **noise_mod.kw(seed), **_lib.generator_kw(generator),
                                            **_lib.wavenet_kw(self.wavenet))[0]
        _lib.call("ov_stitch_window_cores_f32", o_hat, stitch_dev, n_out, Tw, self.spf, out, out.numel(), 0)

    def _run_jobs(self, sources, jobs, tau, out, max_windows, ladder=None, generator=None):
        """Windows of many sources in shared launches.  ``sources``: 1-D device waveforms (spans); ``jobs``: window
        jobs ``(source, f0, lo, hi, Tw, noise [1, inter, Tw], src_se [1, gin, 1], tgt_se, dst)`` with frames relative to
        the source span (``noise``: a tensor, or the ``(seed, stream, first frame)`` of a seeded source's window) and
        ``dst`` the packed output frame of the core's first frame.  Jobs of equal ``Tw`` share
        launches of up to ``max_windows`` in the given order; a partial launch is padded up to the next ``ladder`` size
        (None: launched as it is) with copies of its last window.  ``generator``: handed to ``voice_conversion`` when
        not None.  ``tau``: one number, or a list with one per SOURCE; a launch whose windows' sources disagree carries
        one value per row (``rows_tau``), so sources with different ``tau`` share launches.  Returns the number of
        launches."""
        if not jobs:
            return 0
        bases, acc = [], 0
        for x in sources:
            bases.append(acc)
            acc += x.numel()
        pool = sources[0] if len(sources) == 1 else torch.cat(sources)
        groups = {}
        for j in jobs:
            groups.setdefault(j[4], []).append(j)
        launches = 0
        for Tw, js in groups.items():
            for i0 in range(0, len(js), max_windows):
                chunk = js[i0:i0 + max_windows]
                r = len(chunk)
                W = r if ladder is None else min(b for b in ladder if b >= r)
                rows = chunk + [chunk[-1]] * (W - r)
                recs = [(bases[j[0]], sources[j[0]].numel(), j[1]) for j in rows]
                recs += [(j[8] - (j[2] - j[1]), j[8], j[8] + j[3] - j[2]) for j in chunk]
                recs_dev = torch.tensor(recs, dtype=torch.int64).to(pool.device)      # one host -> device copy
                seeded = [not torch.is_tensor(j[5]) for j in rows]
                if all(seeded):                 # generated inside voice_conversion, straight into its rows
                    nz, seed = None, [j[5] for j in rows]
                elif not any(seeded):
                    nz, seed = torch.cat([j[5] for j in rows]), None
                else:                           # a launch that mixes both kinds: the seeded rows in one fill launch
                    nz, seed = torch.empty(W, self.inter, Tw, dtype=torch.float32, device=pool.device), None
                    for w, j in enumerate(rows):
                        if not seeded[w]:
                            nz[w].copy_(j[5][0])
                    noise_mod.fill([(j[5][0], j[5][1], noise_mod.PURPOSE_POSTERIOR, j[5][2], Tw, w * self.inter * Tw, Tw)
                                    for w, j in enumerate(rows) if seeded[w]], self.inter, nz)
                g_src = torch.cat([j[6].reshape(1, -1, 1) for j in rows])
                g_tgt = torch.cat([j[7].reshape(1, -1, 1) for j in rows])
                launch_tau = rows_tau([tau[j[0]] for j in rows]) if isinstance(tau, list) else tau
                self._launch_multi(pool, recs_dev[:W], Tw, g_src, g_tgt, launch_tau, nz, out, recs_dev[W:], r,
                                   **noise_mod.kw(seed), **_lib.generator_kw(generator))
                launches += 1
        return launches

    def _prepare(self, wave, noise, dev, seed=None):
        """(device waveform, T, noise [1, inter, >= T]) of one recording, checked like ``convert``; with ``seed`` the
        third item is the ``(seed, stream)`` pair instead and no tensor exists."""
        noise_mod.exclusive(seed, noise=noise)
        wave = torch.as_tensor(wave, dtype=torch.float32).reshape(-1).to(dev).contiguous()
        N = wave.numel()
        if self.pad >= N:
            raise ValueError("waveform shorter than the reflect padding")       # spectrogram_torch raises too
        T = frames_of(N, self.n_fft, self.hop)
        if T < 1:
            raise ValueError("waveform shorter than one frame")
        if seed is not None:
            noise = noise_mod.check_seed(seed)
        elif noise is None:
            noise = torch.randn(1, self.inter, T, dtype=torch.float32, device=dev)
        else:
            noise = noise.to(dev, torch.float32)
            if noise.dim() != 3 or noise.shape[0] != 1 or noise.shape[1] != self.inter or noise.shape[2] < T:
                raise ValueError(f"noise must be [1, {self.inter}, >= {T}], got {tuple(noise.shape)}")
        return wave, T, noise

    def _wavenet_cores(self):
        return self.model._wavenet_cores()

    @torch.no_grad()
    @wavenet_keyword
    def convert_many(self, waves, src_ses, tgt_ses, tau=0.3, noises=None, *, seeds=None, generator=None, steps=None):
        """``convert`` of many recordings with their windows packed across recordings into launches of up to
        ``windows_per_launch`` (``ov_frame_hops_multi_f32``: each window framed from its own recording).  ``src_ses`` /
        ``tgt_ses``: one embedding per recording; ``noises``: None or one ``[1, inter, >= T_i]`` (or None) per
        recording -- drawn in order like ``convert`` otherwise; ``seeds`` (instead): an int ``s`` gives recording ``i``
        the counter-based noise of ``(s, i)``, or a list with one seed / pair per recording.  Every recording runs the
        windows of its own
        ``plan_windows``; recordings of ``T <= window_frames`` frames are one ``T``-frame window each and share launches
        with the recordings of equal ``T``.  Returns the converted waveforms (device tensors, views of one packed
        output), each equal to ``convert`` of that recording with the same noise (bit for bit with direct kernels).
        ``generator`` (keyword only): None follows the engine's ``use_bf16_generator`` switch, ``"fp32"`` / ``"bf16"``
        choose the generator's kernels for this call (``ConverterEngine.voice_conversion``); the windows of a launch
        have one length, so the bf16 generator runs them as the dense batch they are.  ``tau``: one number, or one per
        recording (``engine.item_tau``); every window carries the ``tau`` of its recording.  ``steps`` (None: all of the
        above): one ``stretch.step_of(speed)`` per recording (``stretch.ONE``: left alone); the stretched recordings run
        ``_convert_stretched`` and share launches with each other, the others run as always."""
        _lib.check_generator(generator, optional=True)
        dev = self._device()
        n = len(waves)
        tau = item_tau(n, tau)
        if torch.is_tensor(tau):        # windows are regrouped on the host: a device vector is read back once
            tau = tau.tolist()
        if steps is not None and any(int(s) != stretch_mod.ONE for s in steps):
            if len(steps) != n or len(src_ses) != n or len(tgt_ses) != n or (noises is not None and len(noises) != n):
                raise ValueError("convert_many: one src / tgt embedding, step (and noise) per recording")
            noise_mod.exclusive(seeds, noises=noises)
            seeds = [None] * n if seeds is None else noise_mod.per_item(seeds, n)
            outs = [None] * n
            # two subsets, each through its own path: the recordings left alone (today's launches) and the stretched ones
            for stretched in (False, True):
                idx = [i for i in range(n) if (int(steps[i]) != stretch_mod.ONE) == stretched]
                if not idx:
                    continue
                pick = lambda xs: [xs[i] for i in idx]
                sub = dict(tau=pick(tau) if isinstance(tau, list) else tau, noises=None if noises is None else pick(noises),
                           **noise_mod.kw(None if seeds[0] is None else pick(seeds), "seeds"), **_lib.generator_kw(generator))
                if stretched:
                    res = self._convert_stretched(pick(waves), pick(src_ses), pick(tgt_ses), steps=pick(steps), **sub)
                else:
                    res = self.convert_many(pick(waves), pick(src_ses), pick(tgt_ses), **sub)
                for i, o in zip(idx, res):
                    outs[i] = o
            return outs
        if len(src_ses) != n or len(tgt_ses) != n or (noises is not None and len(noises) != n):
            raise ValueError("convert_many: one src / tgt embedding (and noise) per recording")
        noise_mod.exclusive(seeds, noises=noises)
        seeds = [None] * n if seeds is None else noise_mod.per_item(seeds, n)
        items = [self._prepare(w, None if noises is None else noises[i], dev, **noise_mod.kw(seeds[i]))
                 for i, w in enumerate(waves)]
        jobs, offs, acc = [], [], 0
        for i, (wave, T, noise) in enumerate(items):
            offs.append(acc)
            Tw = min(T, self.window_frames)
            for f0, lo, hi in plan_windows(T, self.window_frames, self.context, self.grid):
                nz = noise + (f0,) if seeds[i] is not None else noise[:, :, f0:f0 + Tw]
                jobs.append((i, f0, lo, hi, Tw, nz, src_ses[i], tgt_ses[i], acc + lo))
            acc += T
        out = torch.empty(acc * self.spf, dtype=torch.float32, device=dev)
        # windows of full length first (one shape), then the short recordings grouped by length
        jobs.sort(key=lambda j: j[4] != self.window_frames)
        self._run_jobs([w for w, _, _ in items], jobs, tau, out, self.windows_per_launch, generator=generator)
        return [out[o * self.spf:(o + T) * self.spf] for o, (_, T, _) in zip(offs, items)]

    def _convert_stretched(self, waves, src_ses, tgt_ses, tau, steps, noises=None, seeds=None, generator=None):
        """``convert_many`` of recordings that are all stretched (``steps[i]``: recording i's step).  Windows are cut on
        SOURCE frames as always (``plan_windows``, with the context ``stretch_context_frames`` derives for the step);
        window w of a recording is framed and converted like any window, and inside ``voice_conversion`` its latent is
        stretched with its global position (``stretch=(step, f0, ja, n)``: source column 0 is frame ``f0``, the output
        frames ``[ja, ja + n)`` are made -- ``stretch.plan_windows``) before the generator runs on those ``n`` frames;
        the window then emits the output frames whose ``i`` lies in its core.  Windows of equal ``(Tw, n)`` share
        launches of up to ``windows_per_launch``; every launch is a dense batch.  Never graph-captured.  Returns the
        stretched waveforms, ``stretch.t_out(T_i, steps[i]) * spf`` samples each (views of one packed output)."""
        dev = self._device()
        n_items = len(waves)
        seeds = [None] * n_items if seeds is None else seeds
        items = [self._prepare(w, None if noises is None else noises[i], dev, **noise_mod.kw(seeds[i]))
                 for i, w in enumerate(waves)]
        R, M = frame_reach_frames(), generator_context_frames(self.cfg)
        jobs, offs, acc = [], [], 0
        for i, (wave, T, noise) in enumerate(items):
            step = int(steps[i])
            offs.append(acc)
            Tw = min(T, self.window_frames)
            plan = plan_windows(T, self.window_frames, stretch_context_frames(self.cfg, step), self.grid)
            for (f0, lo, hi), (ja, n, j_lo, j_hi) in zip(plan, stretch_mod.plan_windows(plan, T, self.window_frames, step,
                                                                                       R, M)):
                nz = noise + (f0,) if seeds[i] is not None else noise[:, :, f0:f0 + Tw]
                jobs.append((i, f0, Tw, ja, n, j_lo, j_hi, nz, src_ses[i], tgt_ses[i], acc + j_lo, step))
            acc += stretch_mod.t_out(T, step)
        out = torch.empty(acc * self.spf, dtype=torch.float32, device=dev)
        sources = [w for w, _, _ in items]
        bases, b = [], 0
        for x in sources:
            bases.append(b)
            b += x.numel()
        pool = sources[0] if len(sources) == 1 else torch.cat(sources)
        groups = {}
        for j in jobs:
            groups.setdefault((j[2], j[4]), []).append(j)
        for (Tw, n), js in groups.items():
            for c0 in range(0, len(js), self.windows_per_launch):
                rows = js[c0:c0 + self.windows_per_launch]
                W = len(rows)
                recs = [(bases[j[0]], sources[j[0]].numel(), j[1]) for j in rows]
                # the stitch's (first_frame, core_lo, core_hi), in output frames of the packed output
                recs += [(j[10] - (j[5] - j[3]), j[10], j[10] + j[6] - j[5]) for j in rows]
                recs_dev = torch.tensor(recs, dtype=torch.int64).to(dev)
                if torch.is_tensor(rows[0][7]):
                    nz, seed = torch.cat([j[7] for j in rows]), None
                else:
                    nz, seed = None, [j[7] for j in rows]
                g_src = torch.cat([j[8].reshape(1, -1, 1) for j in rows])
                g_tgt = torch.cat([j[9].reshape(1, -1, 1) for j in rows])
                launch_tau = rows_tau([tau[j[0]] for j in rows]) if isinstance(tau, list) else tau
                spec = self._spectrogram().windows_multi(pool, recs_dev[:W], Tw)
                o_hat = self.model.voice_conversion(spec, torch.full((W,), Tw, dtype=torch.int64), sid_src=g_src,
                                                    sid_tgt=g_tgt, tau=launch_tau, noise=nz,
                                                    stretch=[(j[11], j[1], j[3], n) for j in rows], **noise_mod.kw(seed),
                                                    **_lib.generator_kw(generator), **_lib.wavenet_kw(self.wavenet))[0]
                _lib.call("ov_stitch_window_cores_f32", o_hat, recs_dev[W:], W, n, self.spf, out, out.numel(), 0)
        return [out[o * self.spf:(o + stretch_mod.t_out(T, int(steps[i]))) * self.spf]
                for i, (o, (_, T, _)) in enumerate(zip(offs, items))]

    @torch.no_grad()
    @wavenet_keyword
    def convert(self, wave, src_se, tgt_se, tau=0.3, noise=None, *, seed=None, step=None):
        """``wave``: 1-D float32 waveform at the model rate (host or device).  ``noise``: ``[1, inter, >= T]`` or None
        (then ``torch.randn(1, inter, T)`` on the device: the stream of a seeded one-pass ``convert``); ``seed``
        (instead of ``noise``): the counter-based noise of ``(seed, 0)`` (or of a pair), each window generating its own
        frames -- no ``[1, inter, T]`` tensor exists.  Returns the converted waveform ``[spf * T]`` on the device (spf =
        the generator's samples per frame = hop), ``T`` = frames of ``spectrogram_torch``.  ``step`` (None or
        ``stretch.ONE``: all of the above): the recording stretched by ``stretch.step_of(speed)``
        (``_convert_stretched``) -> ``[spf * stretch.t_out(T, step)]``, the one-pass ``voice_conversion(stretch=[step])``
        of the recording: bit for bit with direct kernels, within the cross-family bar with the defaults."""
        if step is not None and int(step) != stretch_mod.ONE:
            noise_mod.exclusive(seed, noise=noise)
            return self._convert_stretched([wave], [src_se], [tgt_se], tau, [int(step)],
                                           noises=None if noise is None else [noise],
                                           seeds=None if seed is None else [noise_mod.check_seed(seed)])[0]
        dev = self._device()
        wave, T, noise = self._prepare(wave, noise, dev, **noise_mod.kw(seed))
        N = wave.numel()
        plan = plan_windows(T, self.window_frames, self.context, self.grid)
        Tw = min(T, self.window_frames)
        plan_dev = torch.tensor(plan, dtype=torch.int64).to(dev)
        firsts_dev = plan_dev[:, 0].contiguous()
        out = torch.empty(T * self.spf, dtype=torch.float32, device=dev)
        for i0 in range(0, len(plan), self.windows_per_launch):
            i1 = min(len(plan), i0 + self.windows_per_launch)
            # each window's noise is a slice of the file's [1, inter, T] draw (voice_conversion copies it into its rows)
            if seed is not None:
                nz, rows = None, [noise + (f0,) for f0, _, _ in plan[i0:i1]]
            else:
                nz, rows = torch.stack([noise[0, :, f0:f0 + Tw] for f0, _, _ in plan[i0:i1]]), None
            self._launch(wave, N, plan_dev[i0:i1], firsts_dev[i0:i1], Tw, src_se, tgt_se, tau, nz, out, 0,
                         **noise_mod.kw(rows))
        return out

    def stream(self, src_se, tgt_se, tau=0.3, noise=None, sr_in=None, sr_out=None, *, seed=None, message=None,
               watermark_hold=watermark_mod.DEFAULT_HOLD, message_repeat=False):
        return ConversionStream(self, src_se, tgt_se, tau=tau, noise=noise, sr_in=sr_in, sr_out=sr_out, message=message,
                                watermark_hold=watermark_hold, message_repeat=message_repeat, **noise_mod.kw(seed))

    def stream_pool(self, tau=0.3, max_windows_per_launch=DEFAULT_POOL_WINDOWS_PER_LAUNCH):
        return StreamPool(self, tau=tau, max_windows_per_launch=max_windows_per_launch)


class _StreamState:
    """Bookkeeping of one stream on the window grid, shared by ``ConversionStream`` (one window per launch) and
    ``StreamPool`` (many streams per launch): the buffered tail of the input, the next regular window, the readiness
    rule, the end-of-input plan, the noise, and the rates of the input / output (``sr_in`` / ``sr_out``, None: the
    model rate)."""

    def __init__(self, conv, src_se, tgt_se, noise=None, sr_in=None, sr_out=None, seed=None, message=None,
                 watermark_hold=watermark_mod.DEFAULT_HOLD, message_repeat=False):
        noise_mod.exclusive(seed, noise=noise)
        # message=: the block-wise native watermark of the output (watermark.py, "streams"); None: unmarked
        self.mark = watermark_mod.stream_mark(conv.watermark_model, message, watermark_hold, message_repeat)
        self.conv, self.src_se, self.tgt_se = conv, src_se, tgt_se
        self._seed = None if seed is None else noise_mod.check_seed(seed)     # (seed, stream): frames made on demand
        self.dev = conv._device()
        c = conv
        self._Tw, self._core, self._ctx = c.window_frames, c.core, c.context
        self.sr_in, self.sr_out = rates.check_rate(sr_in, "sr_in"), rates.check_rate(sr_out, "sr_out")
        # (Tw - 1) * hop + n_fft - pad at the model rate; the resamplers' waits and a message's hold on top
        # (rates.stream_latency)
        self.latency_seconds, self._latency = rates.stream_latency((self._Tw - 1) * c.hop + c.n_fft - c.pad, c.model_sr,
                                                                   self.sr_in, self.sr_out,
                                                                   hold_samples=watermark_mod.hold_wait(self.mark))
        self.rin = self.rout = None
        self.wave = WaveBuffer(self.dev)
        self._k = 0                 # next regular window
        self._emitted = 0           # frames of output handed out
        self._noise = noise.to(self.dev, torch.float32) if noise is not None else None
        # drawn noise, frames [_nz0, ..); a seeded stream keeps none
        self._nz = None if seed is not None else torch.empty(1, c.inter, 0, dtype=torch.float32, device=self.dev)
        self._nz0 = 0
        self.closed = False
        self._tail = None           # StreamPool: the end-of-input plan, taken by close()

    @property
    def latency_samples(self):
        return self._latency

    @property
    def _len(self):
        """Samples buffered right now: what the tests of bounded memory read."""
        return self.wave.len

    def _need(self, k):
        """Samples after which regular window k can run."""
        c = self.conv
        end = k * self._core + self._Tw
        interior = (end - 1) * c.hop + c.n_fft - c.pad
        longer = end * c.hop + c.n_fft - 2 * c.pad          # frames_of(n) >= end + 1: the file extends past the window
        return max(interior, longer)

    def _noise_for(self, f0, Tw):
        """[1, inter, Tw] noise of frames [f0, f0 + Tw): a slice of the caller's tensor, or drawn once per frame; of a
        seeded stream ``(seed, stream, f0)``: the launch generates the frames where it needs them."""
        if self._seed is not None:
            return self._seed + (f0,)
        if self._noise is not None:
            if self._noise.shape[2] < f0 + Tw:
                raise ValueError(f"noise has {self._noise.shape[2]} frames, the stream needs {f0 + Tw}")
            return self._noise[:, :, f0:f0 + Tw]
        have = self._nz0 + self._nz.shape[2]
        if f0 + Tw > have:
            fresh = torch.randn(1, self.conv.inter, f0 + Tw - have, dtype=torch.float32, device=self.dev)
            self._nz = torch.cat([self._nz, fresh], dim=2)
        return self._nz[:, :, f0 - self._nz0:f0 - self._nz0 + Tw]

    def _regular(self, k):
        f0 = k * self._core
        return (f0, 0 if k == 0 else f0 + self._ctx, f0 + self._ctx + self._core)

    def _trim(self, keep_from_frame):
        """Drop buffered samples and noise no later window reads (whole hops, kept from before the reflect padding)."""
        self.wave.trim(keep_from_frame, self.conv.hop, self.conv.pad)
        if self._noise is None and self._seed is None and keep_from_frame > self._nz0:
            self._nz = self._nz[:, :, keep_from_frame - self._nz0:].clone()
            self._nz0 = keep_from_frame

    def _tail_plan(self, n=None):
        """At the end of the input: ``[(record, Tw)]`` of the windows still to run -- the regular windows of the plan not
        yet run (those whose last frames reach into the end's reflect padding are only now defined) and the last
        window, aligned to the end (``T`` frames when ``T <= Tw``).  Raises ValueError for input shorter than the reflect
        padding or one frame, like ``spectrogram_torch``.  ``n``: the input's total length, when samples are still to
        be appended (an input resampler's tail); the samples received otherwise."""
        c = self.conv
        T = stream_end_frames(self.wave.n if n is None else n, c.n_fft, c.hop)
        plan, k, emitted = [], self._k, self._emitted
        if T > self._Tw:
            while k * self._core + self._Tw < T:
                rec = self._regular(k)
                plan.append((rec, self._Tw))
                emitted = rec[2]
                k += 1
        Tw = min(T, self._Tw)
        plan.append(((T - Tw, emitted, T), Tw))
        return plan


class ConversionStream(_StreamState):
    """Streaming conversion on the window grid of ``WindowedConverter`` (one window per launch).

    ``push(samples)`` appends 1-D float32 samples at the model rate (host or device) and returns the newly finished
    output samples as a device tensor (possibly empty); ``close()`` applies the end-of-file reflect padding, runs the last
    window (aligned to the end) and returns the rest.  Regular window k runs as soon as all its frames are interior
    (no reflect padding at the end can reach them) and the file is certain to extend past it:
    ``(f0 + Tw - 1) * hop + n_fft - pad`` samples, f0 = k * core.  The concatenated output equals
    ``WindowedConverter(windows_per_launch=1).convert`` of the whole input with the same noise, bit for bit.

    ``latency_samples``: input samples that arrive before the first output sample leaves, and the upper bound of any
    sample's delay: ``(Tw - 1) * hop + n_fft - pad``.  Device memory stays bounded: the waveform and noise buffers are
    trimmed as windows finish.

    ``sr_in`` / ``sr_out``: the rate of the pushes / of the output (None: the model rate).  Pushes then pass through a
    ``rates.StreamResampler`` to the model rate and the output through another one, one launch each per push;
    ``latency_samples`` (in output samples) and ``latency_seconds`` include their waits (``rates.stream_latency``).

    ``message`` (None: unmarked, today's path): the output carries the block-wise native watermark of it, made at the
    model rate before the output resampler (``watermark.StreamMarker``, one launch per push with output);
    ``watermark_hold`` = H: a sample leaves at most H - 1 samples later, which the latency figures include;
    ``message_repeat``: window n carries group n % G for the stream's life."""

    def __init__(self, conv, src_se, tgt_se, tau=0.3, noise=None, sr_in=None, sr_out=None, seed=None, message=None,
                 watermark_hold=watermark_mod.DEFAULT_HOLD, message_repeat=False):
        super().__init__(conv, src_se, tgt_se, noise, sr_in=sr_in, sr_out=sr_out, seed=seed, message=message,
                         watermark_hold=watermark_hold, message_repeat=message_repeat)
        self.tau = tau
        self._marker = None if self.mark is None else watermark_mod.StreamMarker(self.mark, self.dev)
        if self.sr_in is not None and self.sr_in != conv.model_sr:
            self.rin = rates.StreamResampler(self.sr_in, conv.model_sr, self.dev)
        if self.sr_out is not None and self.sr_out != conv.model_sr:
            self.rout = rates.StreamResampler(conv.model_sr, self.sr_out, self.dev)

    def _run(self, rec, Tw):
        """One window of the stream: its core samples as a fresh device tensor.  The buffer starts ``wave.base`` samples
        into the file (whole hops), so the window is framed at its first frame relative to the buffer; only a window
        at the file's start (``wave.base`` 0) or end reads reflect padding, and the buffer holds that end."""
        c = self.conv
        f0, lo, hi = rec
        rel = f0 - self.wave.base // c.hop
        assert self.wave.base == 0 or rel * c.hop - c.pad >= 0, "stream buffer trimmed past a window's first sample"
        plan_dev = torch.tensor([(rel, rel + lo - f0, rel + hi - f0)], dtype=torch.int64).to(self.dev)
        out = torch.empty((hi - lo) * c.spf, dtype=torch.float32, device=self.dev)
        nz = self._noise_for(f0, Tw)
        seed = None
        if self._seed is not None:
            nz, seed = None, [nz]
        c._launch(self.wave.valid(), self.wave.len, plan_dev, plan_dev[:, 0].contiguous(), Tw, self.src_se, self.tgt_se,
                  self.tau, nz, out, rel + lo - f0, **noise_mod.kw(seed))
        self._emitted = hi
        return out

    @torch.no_grad()
    def push(self, samples):
        if self.closed:
            raise RuntimeError("push() after close()")
        x = torch.as_tensor(samples, dtype=torch.float32).reshape(-1).to(self.dev)
        self.wave.append(x if self.rin is None else self.rin.push(x))
        outs = []
        while self.wave.n >= self._need(self._k):
            rec = self._regular(self._k)
            outs.append(self._run(rec, self._Tw))
            self._k += 1
            self._trim(rec[0] + 1)      # every later window (regular or the last one) starts after this one
        if not outs:
            y = torch.empty(0, dtype=torch.float32, device=self.dev)
        else:
            y = outs[0] if len(outs) == 1 else torch.cat(outs)
        if self._marker is not None:
            y = self._marker.push(y)
        return y if self.rout is None else self.rout.push(y)

    @torch.no_grad()
    def close(self):
        if self.closed:
            raise RuntimeError("close() called twice")
        self.closed = True
        if self.rin is not None:
            self.wave.append(self.rin.close())
        outs = [self._run(rec, Tw) for rec, Tw in self._tail_plan()]
        self.wave.release()
        y = outs[0] if len(outs) == 1 else torch.cat(outs)
        if self._marker is not None:
            y = self._marker.close(y)
        return y if self.rout is None else self.rout.close(y)


class StreamPool(PushedPool):
    """Many live streams on one window grid, their ready windows converted together: one ``step()`` runs every ready
    window of every open stream in ``ceil(R / max_windows_per_launch)`` launches (fewer per stream than one launch per
    window, which is what the solo ``ConversionStream`` costs).

    ``open(src_se, tgt_se, noise=None, seed=None)`` -> a handle (per-stream embeddings; ``noise`` ``[1, inter, >= T]``,
    or ``seed``: the counter-based noise of ``(seed, 0)`` / of a pair, or neither: drawn lazily per stream); ``push(h,
    samples)`` only buffers (a host -> device copy); ``step()`` -> ``{handle: newly
    finished samples}`` (device tensors, views of one packed output) for the streams with output; ``close(h)`` marks the
    end of h's input -- its last window(s) run in the next ``step()``, which retires h.  A window becomes ready exactly
    when it would in ``ConversionStream`` (the same ``_need`` / ``_tail_plan``), so each stream's concatenated output
    equals a solo stream's fed the same samples with the same noise: bit for bit with direct kernels, and within the
    cross-family bar with the defaults (the Winograd choice depends on the launch size).

    Launch sizes come from a fixed ladder (``launch_ladder``: 1, 2, 4, ..., max_windows_per_launch); a partial launch
    is padded with copies of one of its windows whose output is dropped, and the engine keeps one workspace per ladder
    size resident (``ConverterEngine.resident_workspaces`` is raised to len(ladder) + 1, the one spare for the T-frame
    final windows of streams shorter than a window).  ``tau`` is the pool's default; ``open(..., tau=)`` gives a stream
    its own, kept for life, and the windows of a launch each carry their stream's (``ov_conv1d_params.scale_b``; a
    launch whose windows agree is the scalar launch it always was).

    ``open(..., sr_in=None, sr_out=None)``: the stream's pushes / output at rates of their own.  A ``step()`` then first
    resamples the new input of every such stream to the model rate in ONE launch (``rates.ResamplerBank``) and, after the
    windows, the new output of every such stream in one more; ``latency_of(h)`` is the stream's own bound."""

    def __init__(self, conv, tau=0.3, max_windows_per_launch=DEFAULT_POOL_WINDOWS_PER_LAUNCH):
        self.conv, self.tau = conv, item_tau(1, tau)
        if not isinstance(self.tau, float):
            raise _lib.OvError("StreamPool: the pool's tau is one number; give a stream its own with open(tau=)")
        self.ladder = launch_ladder(max_windows_per_launch)
        self.max_windows_per_launch = self.ladder[-1]
        self._init_streams(conv._device(), conv.model_sr)      # handle -> _StreamState
        engine = getattr(conv.model, "engine", None)
        if callable(engine):
            eng = engine()
            eng.resident_workspaces = max(eng.resident_workspaces, len(self.ladder) + 1)

    @property
    def latency_samples(self):
        """As ``ConversionStream.latency_samples``: ``(Tw - 1) * hop + n_fft - pad`` (plus the wait for the next
        ``step()``), plus ``H - 1`` samples of the longest hold among the open streams that carry a message."""
        c = self.conv
        return (c.window_frames - 1) * c.hop + c.n_fft - c.pad + self._hold_wait()

    def open(self, src_se, tgt_se, noise=None, sr_in=None, sr_out=None, *, seed=None, tau=None, message=None,
             watermark_hold=watermark_mod.DEFAULT_HOLD, message_repeat=False):
        """A new stream -> its handle.  ``tau``: None = the pool's, else this stream's own number, for life.
        ``message`` / ``watermark_hold`` / ``message_repeat``: as for ``ConversionStream``; the marked streams of a step
        share one launch (``watermark.MarkBank``)."""
        tau = self._stream_tau(tau, "StreamPool.open")
        st = _StreamState(self.conv, src_se, tgt_se, noise, sr_in=sr_in, sr_out=sr_out, seed=seed, message=message,
                          watermark_hold=watermark_hold, message_repeat=message_repeat)
        st.tau = tau
        return self._register(st, st.sr_in, st.sr_out)

    def latency_of(self, h):
        """``(seconds, samples)``: stream h's latency bound at its own rates (samples in its output rate)."""
        st = self._stream(h)
        return st.latency_seconds, st.latency_samples

    def close(self, h):
        """End of h's input.  Input shorter than the reflect padding or one frame raises ValueError here and retires h
        (the other streams are untouched)."""
        n = self._end_input(h)
        st = self._streams[h]
        try:
            st._tail = st._tail_plan(n)
        except ValueError:
            self._retire(h)
            raise

    @torch.no_grad()
    def step(self):
        c = self.conv
        self._take_input()
        routs = self._output_rates()
        sources, taus, jobs, spans, acc = [], [], [], {}, 0
        for h, st in self._streams.items():
            if st.closed:
                recs = st._tail
            else:
                recs = []
                while st.wave.n >= st._need(st._k):
                    recs.append((st._regular(st._k), st._Tw))
                    st._k += 1
            if not recs:
                continue
            first = acc
            sh = st.wave.base // c.hop
            for (f0, lo, hi), Tw in recs:
                assert st.wave.base == 0 or (f0 - sh) * c.hop - c.pad >= 0, "stream buffer trimmed past a window's first sample"
                jobs.append((len(sources), f0 - sh, lo - sh, hi - sh, Tw, st._noise_for(f0, Tw), st.src_se, st.tgt_se,
                             acc))
                acc += hi - lo
            sources.append(st.wave.valid())
            taus.append(st.tau)
            spans[h] = (first, acc, recs[-1][0])
        if not jobs:
            return {}
        out = torch.empty(acc * c.spf, dtype=torch.float32, device=sources[0].device)
        # windows of full length first (the ladder's shapes), then the T-frame final windows grouped by length
        jobs.sort(key=lambda j: j[4] != c.window_frames)
        c._run_jobs(sources, jobs, taus, out, self.max_windows_per_launch, ladder=self.ladder)
        outs = {}
        for h, (a, b, (f0, _, hi)) in spans.items():
            outs[h] = out[a * c.spf:b * c.spf]
            st = self._streams[h]
            st._emitted = hi
            if st.closed:
                self._retire(h, finished=True)
            else:
                st._trim(f0 + 1)        # every later window (regular or the last one) starts after this one
        return self._deliver(outs, routs)
