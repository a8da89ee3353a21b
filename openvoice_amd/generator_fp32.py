"""The fp32 generator (reference: openvoice/models.py:272-291) on the MI355X kernels: the launch policy of its MRF convs
(fused pairs, Winograd-domain launches, multi launches), and ``GeneratorFp32`` -- weights, switches, decoder scratch and
the launch sequence of ``decode``.  The sibling of ``bf16.GeneratorBf16``; both walk ``generator.generator_stages``.
``engine`` re-exports the module-level names."""
import torch

from . import _lib
from ._lib import EPI_CONVT, F_CONVT_GROUPED
from .generator import (FINAL_LRELU_SLOPE, GENERATOR_MARGIN, LRELU_SLOPE, conv_transpose_as_conv, generator_margin_frames,
                        generator_stages, resblock_convs, samples_per_frame, scratch_per_frame)
from .launch import PackedConv, padded_frames
from .params import effective_weight

LIMIT_MAX_BATCH = 256   # ovk::LIMIT_MAX_BATCH: utterances per launch the kernels' prefix table holds


def convt_row_order(cout, stride):
    """Packed row order of the grouped ConvTranspose kernels (``F_CONVT_GROUPED``, include/openvoice_amd.h
    OV_EPI_CONVT): natural row ``cout*stride + phase`` of ``conv_transpose_as_conv`` -> 32-row tiles that hold ONE
    phase group each -- tile 2q the phases < stride/2 (their tap x[t+1] is all zeros), tile 2q+1 the phases >=
    stride/2 (tap x[t-1] all zeros) of the same output channels -- so the kernel skips a third of the matrix
    work.  Returns None when the shape cannot be grouped (the natural order + generic kernel are used then)."""
    s = stride
    if s == 8 and cout % 8 == 0:
        per_tile = 8          # channels per tile pair; row-in-tile = 4 * (cout % 8) + phase % 4
    elif s == 2 and cout % 32 == 0:
        per_tile = 32         # row-in-tile = cout % 32
    else:
        return None
    idx = []
    for q in range(cout // per_tile):
        for grp in range(2):
            for c in range(per_tile):
                for ph in range(s // 2):
                    idx.append((q * per_tile + c) * s + grp * (s // 2) + ph)
    return torch.tensor(idx, dtype=torch.long)


_pair_supported = {}


def pair_supported(C, K, dil):
    key = (C, K, dil)
    if key not in _pair_supported:
        _pair_supported[key] = bool(_lib.call("ov_resblock_pair_supported", C, K, dil))
    return _pair_supported[key]


# Where the fused pair beats its two launches on MI355X (profiles/r02_s5_pair_vs_two_launches.txt, B = 32 x 10 s):
# C = 32, k = 3: 0.91 vs 1.09 ms; C = 32, k = 7: 1.75 vs 1.85; C = 64, k = 3: 1.60 vs 1.64.  The MFMA-bound shapes
# (C = 32 k = 11, C = 64 k = 7) run 4-9 % SLOWER fused (32 accumulator registers per wave instead of 64: less matrix
# work per LDS operand) and stay on the two-launch path.  Round 6: at C = 64, k = 3 two Winograd-domain launches (0.56 +
# 0.73 ms, profiles/r06_s17) beat the fused direct pair (1.62 ms), so that shape left the policy.
PAIR_POLICY = {(32, 3), (32, 7)}


def wino_policy(C, K, dil):
    """Where a Winograd-domain launch (csrc/conv1d_wino.h) beats the direct conv it replaces (profiles/r06_s17, B = 32 x
    10 s): every instance at C >= 64; at C = 32 (K = 11, one 32-row fragment per workgroup: the input transform is shared by
    a single row fragment and its helper waves set the pace) the dilation-1 convs only (1.03 vs 1.21 ms; the dilated
    instances tie with the direct kernel and lose in the residual form)."""
    return C >= 64 or dil == 1


# A Winograd launch deals (utterance, column block, row block) items to ONE workgroup per CU; below about half of the
# chip's CUs in items the direct kernel's small tiles fill the machine better (profiles/r06_s20, r06_s21: generator stage 0,
# C = 256, 6 888 columns -- batch 1: 54 items, Winograd 0.45-0.6x the direct conv; batch 2: 108 items, 0.8-1.0x; batch 3:
# 162 items, ahead; batch 4: 216 items, 1.4-1.7x as at batch 32; every other stage has >= 216 items at batch 1 and runs
# 1.1-1.65x faster).  Batch 1 with the rule: 7.50 -> 6.18 ms.
WINO_MIN_ITEMS = 136

# Default of GeneratorFp32.use_multi_launch (DESIGN.md section 8 has the measurement behind it)
USE_MULTI_LAUNCH = True

# Opt-in split-precision path (use_split_bf16x3): generator stages with at least this many channels run on ov_conv1d_split3
SPLIT_MIN_CHANNELS = 128


def _wino_mw(cout):
    return 4 if cout % 128 == 0 else (2 if cout % 64 == 0 else 1)


def wino_ncol(cout, dil):
    """Output columns of one ov_conv1d_wino_f32 N-block (csrc/conv1d_wino.h: 256 columns per matrix wave at dilation 1,
    4 * (64 // dil) * dil at dilation dil; 4 / MW column sub-blocks per workgroup)."""
    return (256 if dil == 1 else 4 * (64 // dil) * dil) * (4 // _wino_mw(cout))


def wino_items(cout, dil, B, L):
    """Work items of one ov_conv1d_wino_f32 launch: (utterance, N-block, M-block)."""
    ncol = wino_ncol(cout, dil)
    return B * ((L + ncol - 1) // ncol) * (cout // (32 * _wino_mw(cout)))


# Columns per work item of the direct kernel (csrc/conv1d_mfma.h N_BLK): the launcher picks 128, 256 or 512 by row count
# and device size.  Under a column limit a launch computes whole items, so the smallest is what skip_padding can rely on.
DIRECT_MIN_NCOL = 128


def conv_reach(family, K, dil=1):
    """(left, right): output column t of a stride-1 'same' K-tap conv run by kernel ``family`` can depend, in floating
    point and NaN propagation included, on input columns t - left .. t + right only.
    'direct' (ov_conv1d_f32), 'pair' (ov_resblock_pair_f32, per conv) and 'split3' (ov_conv1d_split3): the taps,
    (K - 1) / 2 * dil each way.  'wino' (ov_conv1d_wino_f32): an F(4, 3) tile computes the 4 outputs r + dil (4j + i)
    from the 3 (G - 1) + 6 inputs r + dil (4j + m) - PAD dil, PAD = (K - 1) / 2 + lead (wino.LEAD_TAPS), and the inputs
    reach outputs they cancel out of only in exact arithmetic: wider than the taps.  The window's first input enters point
    0 alone (Bt row 0), which only output 0 reads (At column 0), its last one point infinity alone, which only output 3
    reads; every other input reaches all 4 outputs.  So K = 3: 3 dil each way, K = 7: 6 dil, K = 11: 7 dil back and 8 dil
    ahead (tests/test_gpu_wino.py measures it, NaN propagation included)."""
    if family in ("direct", "pair", "split3"):
        r = (K - 1) // 2 * dil
        return r, r
    if family == "wino":
        from . import wino
        G = (K + 2) // 3
        pad = (K - 1) // 2 + wino.LEAD_TAPS[K]
        return (pad + 2) * dil, (3 * (G - 1) + 4 - pad) * dil
    raise ValueError(f"unknown conv family {family!r}")


def resblock_families(C, K, dils, B, L, use_winograd=True, fuse_pairs=True):
    """Kernel family of each conv of one ResBlock1 chain (C channels, kernel K, one (dilated, plain) pair per entry of
    ``dils``) in a (B, L) launch of the fp32 generator: [(family of conv 1, family of conv 2)] with 'pair' (both convs in
    one fused launch), 'wino' or 'direct'.  The policy GeneratorFp32._mrf runs -- PAIR_POLICY, wino_policy,
    WINO_MIN_ITEMS -- and the one limit_margin_frames prices; nothing else restates it."""
    from . import wino
    if fuse_pairs and L % 4 == 0 and all((C, K) in PAIR_POLICY and pair_supported(C, K, d) for d in dils):
        return [("pair", "pair")] * len(dils)
    fam = lambda d: ("wino" if use_winograd and L % 4 == 0 and wino.supported(C, C, K, d) and wino_policy(C, K, d)
                     and wino_items(C, d, B, L) >= WINO_MIN_ITEMS else "direct")
    return [(fam(d), fam(1)) for d in dils]


def limit_margin_frames(cfg, B, T, use_winograd=True, fuse_pairs=True):
    """Frames beyond an utterance's length that the fp32 generator computes under ``skip_padding`` in a (B, T) launch:
    the receptive field of ``generator_margin_frames`` with every ResBlock conv charged the reach of the kernel that runs
    it (conv_reach of resblock_families), at least GENERATOR_MARGIN.  The columns beyond the computed ones hold stale
    scratch; a Winograd conv reads 2-3 dil columns further than its taps, so a direct-only launch keeps 16 while one with
    Winograd stages needs more (tests/test_host_algebra_cpu.py simulates every launch of decode() column by column)."""
    stages = generator_stages(cfg)

    def chain_reach(i, k, dils):
        C, L = stages[i].ch, T * stages[i].rate_out
        fams = resblock_families(C, k, dils, B, L, use_winograd, fuse_pairs)
        return sum(conv_reach(f1, k, d)[1] + conv_reach(f2, k, 1)[1] for (f1, f2), d in zip(fams, dils))

    return max(GENERATOR_MARGIN, generator_margin_frames(cfg), generator_margin_frames(cfg, chain_reach=chain_reach))


def multi_launch_scratch_buffers(cfg):
    """Decoder scratch buffers a multi-launch MRF needs beyond the workspace's t1 / ra: every ResBlock keeps a t1 and an ra of
    its own while the three run side by side (generator.scratch_per_frame sizes each)."""
    return 2 * (len(cfg["resblock_kernel_sizes"]) - 1)


_DEC_BUFFERS = 5         # decoder scratch buffers of a workspace: the stage input, the ConvTranspose output, t1 / ra, the MRF sum


def scratch_elems(cfg, B, T):
    """Float32 elements of what ``GeneratorFp32.add_workspace(ws, B, T)`` allocates: ``(the conv_pre output, each of the
    _DEC_BUFFERS decoder scratch buffers)`` -- the one size computation behind it and ``ConverterEngine.workspace_bytes``."""
    return B * generator_stages(cfg)[0].cin * padded_frames(T), B * T * scratch_per_frame(cfg)


def col_limits(limits, scale):
    """Launch keywords of the length-aware work lists (skip_padding): ``limits`` (int32 [B] frames, or None: the whole
    tensors) x ``scale`` columns per frame of the launch's tensors."""
    return dict(col_limit=limits, col_limit_scale=scale) if limits is not None else {}


def _resblock_tree(sd, cfg, make, keep=lambda stage: True):
    """``[stage][ResBlock][(conv 1, conv 2) per dilation]`` of ``make(c, weight, bias, dilation)`` over
    ``resblock_convs(cfg)`` (``c``: the pair's record); None in place of a stage that ``keep(stage index)`` refuses."""
    convs = list(resblock_convs(cfg))
    layer = lambda c, name, d: make(c, effective_weight(sd, name), sd[name + ".bias"], d)
    return [[[(layer(c, f"{c.prefix}.convs1.{c.n}", c.dil), layer(c, f"{c.prefix}.convs2.{c.n}", 1))
              for c in convs if (c.stage, c.j) == (i, j)]
             for j in range(len(cfg["resblock_kernel_sizes"]))] if keep(i) else None
            for i in range(len(cfg["upsample_rates"]))]


class GeneratorFp32:
    """The fp32 generator of one checkpoint on one device.  ``sd``: the float32 host state dict (kept by reference: the
    split-precision weights are packed from it on first use); ``launcher``: the ``launch.Launcher`` its launches go
    through."""

    def __init__(self, sd, cfg, device, launcher):
        self.cfg, self.device, self.launcher, self._sd = cfg, torch.device(device), launcher, sd
        dev = self.device
        self.conv_pre = PackedConv(sd["dec.conv_pre.weight"], sd["dec.conv_pre.bias"], dev, K=7)
        self.dec_cond_w = sd["dec.cond.weight"][:, :, 0].contiguous().to(dev)
        self.dec_cond_b = sd["dec.cond.bias"].contiguous().to(dev)
        self.stages = generator_stages(cfg)
        self.ups = []
        for i, _, ch, u, *_ in self.stages:
            wc = conv_transpose_as_conv(effective_weight(sd, f"dec.ups.{i}"), u)
            bias = sd[f"dec.ups.{i}.bias"].repeat_interleave(u)
            order = convt_row_order(ch, u)
            if order is not None:
                wc, bias = wc[order], bias[order]
            self.ups.append(dict(conv=PackedConv(wc, bias, dev, K=3, cout=ch), stride=u,
                                 flags=F_CONVT_GROUPED if order is not None else 0))
        self.resblocks = _resblock_tree(sd, cfg, lambda c, w, b, d: PackedConv(w, b, dev, K=c.K, dil=d))
        # Winograd-domain twins (csrc/conv1d_wino.h) of the ResBlock convs of the MFMA-bound stages: the same fp32 conv
        # with 1.6-2x fewer executed multiplies; per stage / ResBlock / pair (w1 | None, w2 | None)
        from . import wino as _wino
        self.wino_resblocks = _resblock_tree(sd, cfg, lambda c, w, b, d: _wino.PackedConvWino(w, b, dev, dil=d)
                                             if _wino.supported(c.ch, c.ch, c.K, d) and wino_policy(c.ch, c.K, d) else None)
        self.final_channels = self.stages[-1].ch
        self.post_w = sd["dec.conv_post.weight"][0].contiguous().to(dev)   # [C, 7]
        self.total_upsample = samples_per_frame(cfg)
        self._limit_margins = {}
        # independent ResBlock chains of a generator stage on this many HIP streams when the batch is at most
        # chain_streams_max_batch utterances (decode()); 1 = always the serial one-stream order
        # Measured (round 4, profiles/r04_s14_sweep_chain_ab.txt): batch 1 8.75 vs 8.81 ms, batch 4 20.4 vs 20.2 ms -- the
        # chains do overlap, but every kernel then runs proportionally longer (the chip is occupied by one-tile
        # workgroups either way) -- so the default is the serial order; results are bit-identical both ways.
        self.chain_streams = 1
        self.chain_streams_max_batch = 8
        # frames the generator computes beyond an utterance's length under skip_padding: this checkpoint's own
        # receptive field (larger ResBlock kernels / dilations or other upsampling than the released models' would
        # silently corrupt the last samples with a hard-wired 16)
        self.generator_margin = max(GENERATOR_MARGIN, generator_margin_frames(self.cfg))
        self.fuse_pairs = True   # ResBlock pairs of the HBM-bound stages as one launch each (PAIR_POLICY)
        # ResBlock convs in the Winograd domain where wino_policy() says so (ov_conv1d_wino_f32):
        # fp32 arithmetic, 6 G / (4 K) of the direct form's multiplies, ~4x its rounding error.
        # The one stored switch: the engine's WaveNet layers read it too (ConverterEngine.use_winograd forwards here)
        self.use_winograd = True
        # The three ResBlocks' convs of one MRF step (k = 3 / 7 / 11, independent of each other) as ONE persistent launch
        # (ov_conv1d_wino_multi_f32) on the stages whose convs are all Winograd launches; bit-identical to the single
        # launches (False: one launch per conv, ResBlock by ResBlock)
        self.use_multi_launch = USE_MULTI_LAUNCH
        self._cus = None         # compute units of the device (read on first use)
        # opt-in split-precision MRF stages: fp32-level products on the bf16 matrix pipe
        self._split3_on = False
        self.split3_products = 6
        self.split_resblocks = None      # per stage: None, or [[(c1, c2) PackedConvSplit3 pairs] per ResBlock]

    def cond(self, g):
        """The generator's cond bias of ``g`` [rows, gin] (a T = 1 GEMV, models.py:275)."""
        return self.launcher.linear(g, self.dec_cond_w, self.dec_cond_b)

    def use_split_bf16x3(self, enable=True, products=6):
        """The switch behind ``ConverterEngine.use_split_bf16x3`` (which documents the path): packs the split-precision
        twins of the stages that take it on first use."""
        if products not in (6, 3):
            raise _lib.OvError(f"use_split_bf16x3: products must be 6 or 3, got {products!r}")
        if enable and self.split_resblocks is None:
            from . import split3
            convs = list(resblock_convs(self.cfg))
            # C = 64 (stage 2) stays on the fp32 Winograd launches: its split convs tie with them (20.9 vs 21.5 ms) and
            # cost two layout passes over the stage's tensors (1.3 ms): 104.3 -> 102.8 ms (profiles/r06_s34_*)
            keep = lambda i: all(c.ch >= SPLIT_MIN_CHANNELS and split3.supported(c.ch, c.ch, c.K, c.dil)
                                 and split3.supported(c.ch, c.ch, c.K, 1) for c in convs if c.stage == i)
            self.split_resblocks = _resblock_tree(self._sd, self.cfg, lambda c, w, b, d:
                                                  split3.PackedConvSplit3(w, b, self.device, dil=d), keep)
        self._split3_on = bool(enable)
        self.split3_products = products

    # ---- decoder scratch ---------------------------------------------------------------------------------------------
    def add_workspace(self, ws, B, T):
        """The generator's entries of a ``ConverterEngine._workspace(B, T)``: ``pre`` (the conv_pre output, zero-filled
        like the frame-rate tensors), ``dec`` (the _DEC_BUFFERS decoder scratch buffers) and ``dec_extra``."""
        ws["pre"] = torch.zeros(B, self.stages[0].cin, padded_frames(T), dtype=torch.float32, device=self.device)
        dec = scratch_elems(self.cfg, B, T)[1]
        ws["dec"] = [torch.empty(dec, dtype=torch.float32, device=self.device) for _ in range(_DEC_BUFFERS)]
        # a multi launch keeps every ResBlock's t1 / ra live at once: part of the workspace, not of a step
        self._chain_scratch(ws, self._multi_launch_scratch(B, T))

    def workspace_buffers(self, B, T):
        """Decoder scratch buffers ``add_workspace(ws, B, T)`` allocates, of ``scratch_elems(cfg, B, T)[1]`` elements each
        (the multi launches' included while ``use_multi_launch`` is on; the opt-in paths' lazily added ones not)."""
        return _DEC_BUFFERS + self._multi_launch_scratch(B, T)

    def _chain_scratch(self, ws, n):
        """``n`` more decoder scratch buffers (the t1 / ra of the ResBlocks beyond the first: concurrent chains and multi
        launches keep them live at once), allocated on first use."""
        extra = ws.setdefault("dec_extra", [])
        while len(extra) < n:
            extra.append(torch.empty_like(ws["dec"][0]))
        return extra

    def _split_buffers(self, ws, B, st, L):
        """Plane tensors (3, B, L, ch) bf16 of split-precision stage ``st``: the activated stage input, the conv1 output,
        two ping-pong pair outputs and one result per ResBlock; allocated once per workspace at the largest stage."""
        nk = len(self.cfg["resblock_kernel_sizes"])
        need = 3 * B * L * st.ch
        bufs = ws.get("split3")
        if bufs is None:
            # sized ONCE per workspace, at the largest split stage of this (batch, frames) -- stage i has ch_i channels at
            # frames x rate_out_i columns -- and never from a capturing graph's private pool
            if torch.cuda.is_current_stream_capturing():
                raise _lib.OvError("split-precision plane buffers must exist before graph capture: run one eager conversion "
                                   "of this (batch, frames) shape first")
            frames = L // st.rate_out
            largest = max([need] + [3 * B * frames * o.rate_out * o.ch for o in self.stages
                                    if self.split_resblocks[o.index] is not None])
            bufs = ws["split3"] = [torch.empty(largest, dtype=torch.bfloat16, device=self.device) for _ in range(4 + nk)]
        assert bufs[0].numel() >= need
        return [b[:need].view(3, B, L, st.ch) for b in bufs]

    def live_workspace(self, stage, B, width):
        """Scratch of one live launch of generator stage ``stage``, ``B`` rows of ``width`` input columns at most: the
        conv_pre output (stage 0), the ConvTranspose output and the two MRF scratch buffers, and the MRF output of the
        last stage (conv_post reads it).  ``ConverterEngine.live_workspace`` caches it."""
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.device)
        st, Tp = self.stages[stage], padded_frames(width)
        n = B * st.ch * width * st.stride
        ws = dict(Tp=Tp, dec=[z(n) for _ in range(3)])
        if stage == 0:
            ws["pre"] = z(B, st.cin, Tp)
        if st.last:
            ws["acc"] = z(n)
        return ws

    # ---- the launch sequence -------------------------------------------------------------------------------------------
    def _mrf_split(self, st, u, acc, ws, B, L, limits=None):
        """The MRF of stage ``st`` on the split-precision kernels: u (B, ch, L) fp32 raw -> acc (B, ch, L) fp32 = mean of the
        ResBlock1 outputs.  Tensors between the launches are plane tensors stored ACTIVATED (the producer applies the
        next conv's leaky ReLU before it splits); conv2 reads its residual from the pair's activated input and inverts
        the activation in fp32; the last pair of a ResBlock stores raw; the sum / mean is the layout kernel back."""
        from . import split3
        stage, ch = self.split_resblocks[st.index], st.ch
        nk = len(stage)
        bufs = self._split_buffers(ws, B, st, L)
        xa, t, ping, pong, results = bufs[0], bufs[1], bufs[2], bufs[3], bufs[4:]
        prod = self.split3_products
        # length-aware work lists (skip_padding): 128-column tiles beyond an utterance's limit are dropped from every
        # conv's (dense) work list; the two layout kernels stream whole tensors
        lim = col_limits(limits, st.rate_out)
        timed = self.launcher.timed
        uv = u[:B * ch * L].view(B, ch, L)
        timed("split_layout", 0.0, lambda: split3.to_planes(uv, LRELU_SLOPE, out=xa))
        for j, pairs in enumerate(stage):
            cur = xa
            for n, (c1, c2) in enumerate(pairs):
                last = n == len(pairs) - 1
                flops = 2.0 * ch * ch * c1.K * L * B
                timed("mrf_split", flops, lambda: split3.launch_conv_split3(c1, cur, t, out_slope=LRELU_SLOPE, products=prod, **lim))
                dst = results[j] if last else (pong if cur is ping else ping)
                timed("mrf_split", flops, lambda: split3.launch_conv_split3(c2, t, dst, res=cur, res_slope=LRELU_SLOPE,
                                                                             out_slope=1.0 if last else LRELU_SLOPE,
                                                                             products=prod, **lim))
                cur = dst
        ops = list(results[:nk]) + [None] * (3 - nk)
        if nk > 3:
            raise _lib.OvError("split-precision MRF: at most 3 ResBlocks per stage")
        av = acc[:B * ch * L].view(B, ch, L)
        timed("split_layout", 0.0, lambda: split3.from_planes(ops[0], ops[1], ops[2], in_slope=1.0, scale=1.0 / nk, out=av))

    def limit_margin(self, B, T):
        """``limit_margin_frames`` of this generator's configuration for a (B, T) launch under the CURRENT
        ``use_winograd`` / ``fuse_pairs`` (they may be switched after construction); at least ``generator_margin``."""
        key = (int(B), int(T), bool(self.use_winograd), bool(self.fuse_pairs))
        cache = self._limit_margins
        if key not in cache:
            cache[key] = max(self.generator_margin, limit_margin_frames(self.cfg, *key))
        return cache[key]

    def frame_limits(self, lengths, T):
        """Two int32 [B] device vectors (``ov_frame_limits_i32``, no host sync): the frames of each utterance the
        generator must COMPUTE so that its first ``lengths[b]`` frames are unaffected by what lies beyond
        (``length + limit_margin(B, T)``), and the frames it KEEPS (``length``): ``conv_post`` writes zeros beyond them,
        so the whole of ``o_hat`` is defined -- what lies between the two is computed from neighbours that were skipped
        and must not leak into the result."""
        B = lengths.shape[0]
        lim = torch.empty(2, B, dtype=torch.int32, device=self.device)
        _lib.call("ov_frame_limits_i32", lengths, lim[0], B, int(T), self.limit_margin(B, T))
        _lib.call("ov_frame_limits_i32", lengths, lim[1], B, int(T), 0)
        return lim

    def _upsample(self, i, x, x_ld, u, B, L, cin, ch, **lim):
        """leaky_relu(0.1) + ConvTranspose1d of generator stage ``i`` (models.py:278-279): x [B, cin, x_ld] with ``L``
        valid columns -> u, dense [B, ch, L * stride]."""
        up = self.ups[i]
        s = up["stride"]
        self.launcher.conv(up["conv"], x, 0, cin * x_ld, u, 0, ch * L * s, B, L, epi=EPI_CONVT, in_slope=LRELU_SLOPE,
                           flags=up["flags"], phase_s=s, x_ld=x_ld, tag="ups", alg_flops=2.0 * cin * ch * 2 * s * L * B, **lim)

    def _mrf(self, i, u, t1, ra, acc, ws, B, ch, L, limits, rate):
        """MRF of generator stage ``i`` on the fp32 kernels: u (dense [B, ch, L]) -> acc = mean of the ResBlock1
        outputs; t1 / ra are scratch of the same size.  ``limits`` / ``rate``: the length-aware work lists of decode()."""
        nk = len(self.cfg["resblock_kernel_sizes"])
        lim, run = col_limits(limits, rate), self.launcher
        bs = ch * L
        # MRF: mean of the 3 ResBlock1 outputs (models.py:280-286, modules.py:296-306).  The three ResBlocks of a
        # stage are independent chains until the sum.  At small batches one launch does not fill the chip (batch 1,
        # stage 0: 108 workgroups for 512 slots; stages 1-3: one partial round of 431), so there the chains run on
        # separate HIP streams and fill each other's ramps and tails; chain j's last launch waits for chain j - 1's
        # (the running sum keeps its order: bit-identical to the serial sequence).
        concurrent = (self.chain_streams > 1 and nk > 1 and B <= self.chain_streams_max_batch and run.profile is None
                      # the chains' extra scratch is allocated lazily: never from a capturing graph's private pool
                      and not (torch.cuda.is_current_stream_capturing() and len(ws.get("dec_extra", [])) < 2 * (nk - 1)))
        scratch = [(t1, ra)]
        if concurrent:
            extra = self._chain_scratch(ws, 2 * (nk - 1))
            scratch += [(extra[2 * j], extra[2 * j + 1]) for j in range(nk - 1)]

        def chain(j, pairs):
            t1_, ra_ = scratch[j if concurrent else 0]
            cur = u
            # fused pairs, or Winograd-domain convs where an instance exists, wino_policy() picks it and the launch has
            # WINO_MIN_ITEMS items; all carry the same length-aware work lists (skip_padding)
            fams = resblock_families(ch, pairs[0][0].K, [c1.dil for c1, _ in pairs], B, L, self.use_winograd,
                                     self.fuse_pairs)
            fused = fams[0][0] == "pair"
            wn = self.wino_resblocks[i][j]
            for n, (c1, c2) in enumerate(pairs):
                last = n == len(pairs) - 1
                if last and concurrent and j > 0:
                    torch.cuda.current_stream(self.device).wait_event(done[j - 1])
                add = acc if (last and j > 0) else None
                scale = 1.0 / nk if (last and j == nk - 1) else 1.0
                if fused:
                    # one launch per pair, intermediate in LDS; out must not alias x: ra / t1 ping-pong
                    dst = acc if last else (t1_ if cur is ra_ else ra_)
                    run.pair(c1, c2, cur, dst, bs, B, L, add, scale, **lim)
                else:
                    w1, w2 = (w if f == "wino" else None for w, f in zip(wn[n], fams[n]))
                    # t1 is read by c2 only, which activates it: a Winograd c1 stores it activated (the same
                    # values, modules.py:298-301) and c2 -- either kernel -- stages it as is
                    if w1 is not None:
                        run.wino(w1, cur, t1_, bs, B, L, out_slope=LRELU_SLOPE, **lim)
                    else:
                        run.conv(c1, cur, 0, bs, t1_, 0, bs, B, L, in_slope=LRELU_SLOPE, tag="mrf", **lim)
                    c2_slope = 1.0 if w1 is not None else LRELU_SLOPE
                    dst = acc if last else ra_
                    if w2 is not None:
                        run.wino(w2, t1_, dst, bs, B, L, res=cur, add=add, scale=scale, in_slope=c2_slope, **lim)
                    else:
                        run.conv(c2, t1_, 0, bs, dst, 0, bs, B, L, in_slope=c2_slope, res=cur, res_bs=bs,
                                 add=add, add_bs=bs, scale=scale, tag="mrf", **lim)
                cur = dst

        if not concurrent and self._mrf_multi(i, u, t1, ra, acc, ws, B, ch, L, lim):
            return
        if not concurrent:
            for j, pairs in enumerate(self.resblocks[i]):
                chain(j, pairs)
        else:
            main = torch.cuda.current_stream(self.device)
            side = run.side_streams(nk)
            fork = torch.cuda.Event()
            fork.record(main)
            done = [None] * nk
            for j, pairs in enumerate(self.resblocks[i]):
                with torch.cuda.stream(side[j]):
                    side[j].wait_event(fork)
                    chain(j, pairs)
                    done[j] = torch.cuda.Event()
                    done[j].record(side[j])
            for j in range(nk):                     # every chain's scratch is free again before the next stage
                main.wait_event(done[j])

    def _multi_launch_stage(self, i, B, ch, L):
        """Whether the MRF of stage ``i`` runs as multi launches in a (B, ch, L) conversion: the switches, three (or two)
        ResBlocks of different kernel sizes and equal dilations, every conv a Winograd launch (``resblock_families``: an
        instance, wino_policy, WINO_MIN_ITEMS) of the 64- or 128-row families -- and more items per conv than the device has
        CUs.  Up to one item per workgroup there is no tail to level and the three launches already run one item each; with
        every ResBlock on scratch of its own the stage then only loses the cache hits that shared t1 / ra buffers give a
        small conversion (batch 1 x 10 s: 6.02 ms against 5.95), so those stay launch by launch."""
        blocks = self.resblocks[i]
        nk = len(blocks)
        ks = [pairs[0][0].K for pairs in blocks]
        dils = [[c1.dil for c1, _ in pairs] for pairs in blocks]
        if not (self.use_multi_launch and self.use_winograd and 2 <= nk <= 3 and len(set(ks)) == nk and set(ks) <= {3, 7, 11}
                and ch % 64 == 0 and all(d == dils[0] for d in dils)):
            return False
        if self._cus is None:
            self._cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if wino_items(ch, 1, B, L) <= self._cus:
            return False
        fams = [resblock_families(ch, k, d, B, L, self.use_winograd, self.fuse_pairs) for k, d in zip(ks, dils)]
        return all(f == ("wino", "wino") for fam in fams for f in fam)

    def _multi_launch_scratch(self, B, T):
        """``multi_launch_scratch_buffers`` when some stage of a (B, T) conversion runs multi launches, else 0."""
        return (multi_launch_scratch_buffers(self.cfg)
                if any(self._multi_launch_stage(st.index, B, st.ch, T * st.rate_out) for st in self.stages) else 0)

    def _mrf_multi(self, i, u, t1, ra, acc, ws, B, ch, L, lim):
        """The MRF of stage ``i`` walked PAIR BY PAIR with the three ResBlocks' convs of a step in one launch
        (ov_conv1d_wino_multi_f32): c1 of every ResBlock, then c2 of every ResBlock.  The c2 of the LAST pair adds the
        running MRF sum of the ResBlock before it, so those stay single launches in ResBlock order: the same operations on
        the same operands as ``_mrf``'s chains, bit for bit.  Returns False -- nothing launched -- where the stage is not made
        of Winograd launches of one shape (``_mrf`` then runs it launch by launch)."""
        blocks, wn, run = self.resblocks[i], self.wino_resblocks[i], self.launcher
        nk = len(blocks)
        dils = [[c1.dil for c1, _ in pairs] for pairs in blocks]
        if not self._multi_launch_stage(i, B, ch, L):
            return False
        need = multi_launch_scratch_buffers(self.cfg)
        if torch.cuda.is_current_stream_capturing() and len(ws.get("dec_extra", [])) < need:
            return False           # the scratch is never allocated from a capturing graph's private pool
        extra = self._chain_scratch(ws, need)
        ts, ras = [t1] + extra[0:need:2], [ra] + extra[1:need:2]
        bs, npairs = ch * L, len(dils[0])
        cur = [u] * nk
        for n in range(npairs):
            run.wino_multi([dict(layer=wn[j][n][0], x=cur[j], out=ts[j], bs=bs, in_slope=LRELU_SLOPE, out_slope=LRELU_SLOPE)
                            for j in range(nk)], B, L, **lim)
            if n < npairs - 1:
                run.wino_multi([dict(layer=wn[j][n][1], x=ts[j], out=ras[j], bs=bs, res=cur[j]) for j in range(nk)], B, L, **lim)
                cur = list(ras)
            else:
                for j in range(nk):
                    run.wino(wn[j][n][1], ts[j], acc, bs, B, L, res=cur[j], add=acc if j > 0 else None,
                             scale=1.0 / nk if j == nk - 1 else 1.0, in_slope=1.0, **lim)
        return True

    def stage(self, st, x, x_ld, x_bs, bufs, out, ws, B, L, cond_d=None, limits=None, keep=None):
        """Generator stage ``st`` (models.py:274-291) on the fp32 kernels: [conv_pre + cond into ``ws["pre"]`` (stage 0)],
        leaky_relu + ConvTranspose, the MRF, [leaky_relu(0.01) + conv_post + tanh into ``out`` (last stage)].  ``x``
        [B rows of ``x_bs``][cin][``x_ld``] with ``L`` columns; ``bufs`` = (u, t1, ra, acc), dense [B, ch, L * stride]
        each: the ConvTranspose output, the MRF's two scratch buffers -- None for a split-precision stage, which takes
        its plane buffers from ``ws`` -- and the MRF mean.  ``limits`` / ``keep``: the two rows of ``frame_limits``."""
        if st.index == 0:
            Tp = ws["Tp"]
            self.launcher.conv(self.conv_pre, x, 0, x_bs, ws["pre"], 0, st.cin * Tp, B, L, bias_b=cond_d,
                               bias_b_bs=0 if cond_d.shape[0] == 1 else cond_d.shape[1], x_ld=x_ld, out_ld=Tp, tag="conv_pre",
                               **col_limits(limits, 1))
            x, x_ld = ws["pre"], Tp
        u, t1, ra, acc = bufs
        self._upsample(st.index, x, x_ld, u, B, L, st.cin, st.ch, **col_limits(limits, st.rate_in))
        L *= st.stride
        if t1 is None:
            self._mrf_split(st, u, acc, ws, B, L, limits=limits)
        else:
            self._mrf(st.index, u, t1, ra, acc, ws, B, st.ch, L, limits, st.rate_out)
        if st.last and keep is not None:
            _lib.call("ov_conv_post_tanh_limited_f32", acc, self.post_w, out, B, st.ch, L, self.post_w.shape[1],
                      FINAL_LRELU_SLOPE, keep, st.rate_out)
        elif st.last:
            _lib.call("ov_conv_post_tanh_f32", acc, self.post_w, out, B, st.ch, L, self.post_w.shape[1], FINAL_LRELU_SLOPE)

    def decode(self, z_hat, cond_d, ws, T=None, limits=None):
        """Generator (models.py:272-291).  ``z_hat`` is [B, C, ld] with ``T`` valid frames per row
        (``T`` defaults to the full row, i.e. a dense tensor); ``ws``: the engine's workspace of (B, T)
        (``add_workspace``).  ``limits`` (``frame_limits``): frames per utterance
        to compute -- time tiles wholly beyond are dropped from every launch's work list."""
        B, C, ld = z_hat.shape
        T = ld if T is None else T
        keep = None
        if limits is not None:
            limits, keep = limits[0], limits[1]
            if B > LIMIT_MAX_BATCH:
                # the conv kernels' prefix table holds 256 utterances: beyond that every launch computes the whole
                # tensors, but conv_post (a per-utterance limit, no table) still keeps `length` frames and writes zeros
                # beyond them -- the skip_padding contract ("the padded tail of o_hat is zero") holds at any batch size
                limits = None
        o_hat = torch.empty(B, 1, T * self.total_upsample, dtype=torch.float32, device=self.device)
        x, x_ld, x_bs = z_hat, ld, C * ld
        free = list(ws["dec"])
        for st in self.stages:
            u = free.pop()
            if st.index > 0:
                free.append(x)            # the stage's input is free once its ConvTranspose has read it: it serves as t1
            # a split-precision stage (opt-in) keeps its intermediates in plane buffers of its own
            split = self._split3_on and self.split_resblocks[st.index] is not None
            t1, ra = (None, None) if split else (free.pop(), free.pop())
            acc = free.pop()
            self.stage(st, x, x_ld, x_bs, (u, t1, ra, acc), o_hat, ws, B, T * st.rate_in, cond_d, limits, keep)
            free += [u] if split else [u, t1, ra]
            x, x_ld = acc, T * st.rate_out
        return o_hat

    def live_stage(self, i, x, x_ld, x_bs, out, B, L, ws, cond_d=None):
        """Generator stage ``i`` as a live unit on ``ws`` from ``live_workspace`` (``ConverterEngine.live_generator_stage``
        documents the contract): ``decode``'s own launches on caller-given buffers."""
        st = self.stages[i]
        u, t1, ra = ws["dec"]
        self.stage(st, x, x_ld, x_bs, (u, t1, ra, ws["acc"] if st.last else out), out, ws, B, L, cond_d)
