"""Host helpers of the bf16 channels-last generator kernels (csrc/conv1d_bf16.hip): weight packing and launch.
Activations are ``torch.bfloat16`` tensors of shape (B, L, C) -- channels contiguous."""
import ctypes

import torch

from . import _lib
from ._lib import ConvBf16Params
from .generator import (FINAL_LRELU_SLOPE, GENERATOR_MARGIN, LRELU_SLOPE, conv_transpose_as_conv, generator_margin_frames,
                        generator_stages, resblock_convs, samples_per_frame, scratch_per_frame)
from .params import effective_weight


class PackedConvBf16:
    """One conv layer in bf16 kernel-ready form: B-fragment-ordered bf16 weights + fp32 bias."""

    def __init__(self, w_dense, bias, device, dil=1):
        w = w_dense.detach().to(torch.float32).cpu().contiguous()
        self.cout, self.cin, self.K = w.shape
        self.dil = dil
        n = _lib.call("ov_conv1d_bf16_pack_size", self.cout, self.cin, self.K)
        if n == 0:
            raise _lib.OvError(f"bf16 conv needs Cin % 32 == 0 (got {self.cin})")
        packed = torch.empty(n, dtype=torch.int16)
        _lib.call("ov_conv1d_bf16_pack", w, self.cout, self.cin, self.K, packed)
        self.w = packed.to(device)
        # the second-generation fused pair runs on 16x16x32 fragments: its own record order (ov_conv1d_bf16_pack16)
        self.w16 = None
        if self.cout == self.cin and _lib.call("ov_resblock_pair2_bf16_supported", self.cin, self.K, dil):
            packed16 = torch.empty(n, dtype=torch.int16)
            _lib.call("ov_conv1d_bf16_pack16", w, self.cout, self.cin, self.K, packed16)
            self.w16 = packed16.to(device)
        self.bias = None if bias is None else bias.detach().float().contiguous().to(device)


def launch_conv_bf16(layer, x, out, in_slope=1.0, scale=1.0, res=None, add=None, layout=0, out_slope=1.0, dbg=None):
    """out = (conv1d(lrelu(x, in_slope)) + bias [+ res] [+ add]) * scale on torch's current stream.
    x (B, L, Cin), out / res / add (B, L, Cout), all contiguous bfloat16."""
    B, L, cin = x.shape
    assert cin == layer.cin and out.shape == (B, L, layer.cout)
    for t in (x, out, res, add):
        assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous())
    if _lib.use_torch_binding():
        _lib.torch_op("conv1d_bf16cl", x, layer.w, layer.bias, out, res, add, dbg,
                      [B, L, cin, layer.cout, layer.K, layer.dil, 0, 0, layout], [in_slope, scale, out_slope])
        return
    p = ConvBf16Params()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    p.x, p.w, p.bias, p.out, p.res, p.add = vp(x), vp(layer.w), vp(layer.bias), vp(out), vp(res), vp(add)
    p.B, p.L, p.Cin, p.Cout, p.K, p.dil = B, L, cin, layer.cout, layer.K, layer.dil
    p.in_slope, p.scale, p.layout, p.out_slope = in_slope, scale, layout, out_slope
    p.dbg = vp(dbg)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(_lib.load().ov_conv1d_bf16cl(ctypes.byref(p), stream), "ov_conv1d_bf16cl")


def launch_pair_bf16(c1, c2, x, out, add=None, scale=1.0, slope=0.1, nwg=0, dbg=None):
    """One fused ResBlock1 iteration on bf16 channels-last tensors (``ov_resblock_pair_bf16cl``):
    out = bf16((c2(lrelu(bf16(c1(lrelu(x))))) + x [+ add]) * scale).  x / out / add (B, L, C) contiguous bfloat16;
    ``out`` must not alias ``x``."""
    B, L, C = x.shape
    assert c1.cin == c1.cout == c2.cin == c2.cout == C and c1.K == c2.K and c2.dil == 1 and out.shape == x.shape
    for t in (x, out, add):
        assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous())
    if _lib.use_torch_binding():
        _lib.torch_op("resblock_pair_bf16cl", x, c1.w, c1.bias, c2.w, c2.bias, out, add, dbg,
                      [B, L, C, c1.K, c1.dil, nwg], [slope, scale])
        return
    p = _lib.RespairBf16Params()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    p.x, p.w1, p.b1, p.w2, p.b2, p.out, p.add = vp(x), vp(c1.w), vp(c1.bias), vp(c2.w), vp(c2.bias), vp(out), vp(add)
    p.B, p.L, p.C, p.K, p.dil, p.nwg = B, L, C, c1.K, c1.dil, nwg
    p.slope, p.scale = slope, scale
    p.dbg = vp(dbg)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(_lib.load().ov_resblock_pair_bf16cl(ctypes.byref(p), stream), "ov_resblock_pair_bf16cl")


def launch_pair2_bf16(c1, c2, x, out, add=None, scale=1.0, slope=0.1, out_slope=1.0, nwg=0, dbg=None, exp_flags=0):
    """One fused ResBlock1 iteration of the matrix-bound stages (``ov_resblock_pair2_bf16cl``, C in {64, 128}) on
    bf16 channels-last tensors stored ACTIVATED: ``x`` = bf16(lrelu(x_raw, slope));
    out = bf16(lrelu((c2(bf16(lrelu(c1(x) + b1))) + b2 + x_raw [+ add]) * scale, out_slope)), ``add`` raw.
    x / out / add (B, L, C) contiguous bfloat16; ``out`` must not alias ``x``."""
    B, L, C = x.shape
    assert c1.cin == c1.cout == c2.cin == c2.cout == C and c1.K == c2.K and c2.dil == 1 and out.shape == x.shape
    for t in (x, out, add):
        assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous())
    if c1.w16 is None or c2.w16 is None:
        raise _lib.OvError(f"ov_resblock_pair2_bf16cl: no 16x16x32 weight stream for C={C} K={c1.K} dil={c1.dil}")
    if _lib.use_torch_binding():
        _lib.torch_op("resblock_pair2_bf16cl", x, c1.w16, c1.bias, c2.w16, c2.bias, out, add, dbg,
                      [B, L, C, c1.K, c1.dil, nwg, exp_flags], [slope, scale, out_slope])
        return
    p = _lib.Respair2Bf16Params()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    p.x, p.w1, p.b1, p.w2, p.b2, p.out, p.add = vp(x), vp(c1.w16), vp(c1.bias), vp(c2.w16), vp(c2.bias), vp(out), vp(add)
    p.B, p.L, p.C, p.K, p.dil, p.nwg = B, L, C, c1.K, c1.dil, nwg
    p.slope, p.scale, p.out_slope, p.exp_flags = slope, scale, out_slope, exp_flags
    p.dbg = vp(dbg)
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(_lib.load().ov_resblock_pair2_bf16cl(ctypes.byref(p), stream), "ov_resblock_pair2_bf16cl")


_pair_supported = {}
_pair2_supported = {}


def pair2_bf16_supported(C, K, dil):
    key = (C, K, dil)
    if key not in _pair2_supported:
        _pair2_supported[key] = bool(_lib.call("ov_resblock_pair2_bf16_supported", C, K, dil))
    return _pair2_supported[key]


def pair_bf16_supported(C, K, dil):
    key = (C, K, dil)
    if key not in _pair_supported:
        _pair_supported[key] = bool(_lib.call("ov_resblock_pair_bf16_supported", C, K, dil))
    return _pair_supported[key]


def _launch(layer, x, out, L, in_slope=1.0, scale=1.0, res=None, add=None, phase_s=0, bias=None, bias_bstride=0,
            out_slope=1.0):
    B = x.shape[0]
    bias = layer.bias if bias is None else bias
    if _lib.use_torch_binding():
        _lib.torch_op("conv1d_bf16cl", x, layer.w, bias, out, res, add, None,
                      [B, L, layer.cin, layer.cout, layer.K, layer.dil, phase_s, bias_bstride, 0],
                      [in_slope, scale, out_slope])
        return
    p = ConvBf16Params()
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    p.x, p.w, p.bias, p.out, p.res, p.add = vp(x), vp(layer.w), vp(bias), vp(out), vp(res), vp(add)
    p.B, p.L, p.Cin, p.Cout, p.K, p.dil = B, L, layer.cin, layer.cout, layer.K, layer.dil
    p.phase_s, p.bias_bstride, p.in_slope, p.scale, p.out_slope = phase_s, bias_bstride, in_slope, scale, out_slope
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(_lib.load().ov_conv1d_bf16cl(ctypes.byref(p), stream), "ov_conv1d_bf16cl")


def generator_alg_bytes(cfg, B, T, esize=2, z_channels=192, fused=True):
    """Algorithmic HBM bytes of one generator pass: every tensor pass of the launch sequence (conv_pre; per stage
    the ups read + write and the MRF -- per ResBlock pair 2 passes when it is one fused launch (read x, write out),
    5 as two launches (conv1 r + w, conv2 r + res + w) -- plus the 2 running-sum reads; conv_post)."""
    stages = generator_stages(cfg)
    total = B * T * (z_channels + stages[0].cin) * esize
    kernels, dils = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    for _, cin, ch, _, rate_in, rate_out, _ in stages:
        total += B * T * rate_in * cin * esize
        L = T * rate_out
        tensor = B * L * ch * esize
        passes = 1                                                  # the ups write
        for j, (k, rd) in enumerate(zip(kernels, dils)):
            one = fused and all(pair_bf16_supported(ch, k, d) or pair2_bf16_supported(ch, k, d) for d in rd)
            passes += len(rd) * (2 if one else 5) + (1 if j > 0 else 0)
        total += tensor * passes
    return total + B * L * ch * esize + B * L * 4


# ---- a ragged batch as dense length groups (csrc/ragged_bf16.hip) -------------------------------------------------------
MAX_GROUPS_CAP = 8              # the launch count of decode_groups stays bounded: at most 8 passes over the generator
# Defaults of GeneratorBf16.max_groups / .group_cost, measured on an MI355X (tools/bf16_groups_table.py, DESIGN section
# 20): a B = 1, T = 1 decode -- one more pass over the ~80 launches, whatever its size -- takes 0.697 ms, an item-frame
# of a B = 64, T = 861 decode 0.625 us: one more group costs what 1114 item-frames cost.  On the V1 TTS batch (16 x 100
# symbols, 191 .. 328 frames, 5248 padded item-frames) no cut saves that much, the planner keeps one group and the
# grouped run equals the padded one (8.56 against 8.54 ms): grouping is NOT faster there, so the default is one group.
DEFAULT_MAX_GROUPS = 1
DEFAULT_GROUP_COST = 1100       # item-frames one more pass over the launch sequence costs
PACK_FIELDS, UNPACK_FIELDS = 5, 4      # (src_off, src_ld, dst_off, cols, L) / (src_off, dst_off, keep, row)


def plan_groups(lengths, Td, margin, max_groups, group_cost):
    """Cut a ragged batch into dense groups: pure host code, a function of its arguments alone.

    ``lengths[b]``: item b's own frames (clamped to ``[0, Td]``); ``Td``: the frames of the padded run; ``margin``: the
    frames an item must be computed beyond its own length so that its first ``length`` frames do not feel the group's
    right edge (``GeneratorBf16.margin``); ``max_groups >= 1``; ``group_cost``: what one more group costs, in
    item-frames (rounded to an integer).  The items are sorted by length (stable: ties stay in batch order); a dynamic
    programme over the contiguous cuts of the sorted list minimises ``sum_g(B_g * L_g) + n_groups * group_cost`` with
    ``L_g = min(Td, longest length of the group + margin)`` over at most ``max_groups`` groups; among equal costs the
    fewest groups, then the earliest cuts.  Returns ``[(batch indices, L_g), ...]`` in ascending length order -- a
    partition of ``range(len(lengths))``.  One group has ``L = min(Td, longest + margin)``: ``Td`` whenever ``Td`` is
    the longest item's length, as it is in ``infer``."""
    Td, margin, G, gc = int(Td), int(margin), int(max_groups), int(round(group_cost))
    if Td < 1 or margin < 0 or G < 1 or gc < 0:
        raise ValueError(f"plan_groups: Td = {Td}, margin = {margin}, max_groups = {max_groups}, group_cost = {group_cost}")
    lens = [min(max(int(n), 0), Td) for n in lengths]
    if not lens:
        return []
    order = sorted(range(len(lens)), key=lambda b: lens[b])
    need = [max(1, min(Td, lens[b] + margin)) for b in order]
    # a cut between two items of equal need never pays: the runs of equal need are the units of the programme
    ends = [j + 1 for j in range(len(need)) if j + 1 == len(need) or need[j + 1] != need[j]]
    R = len(ends)
    starts = [0] + ends[:-1]
    G = min(G, R)
    INF = float("inf")
    best = [[INF] * R for _ in range(G + 1)]          # best[k][r]: runs 0 .. r in exactly k groups
    cut = [[0] * R for _ in range(G + 1)]             # the first run of the last group
    for r in range(R):
        best[1][r] = ends[r] * need[ends[r] - 1] + gc
    for k in range(2, G + 1):
        for r in range(k - 1, R):
            L = need[ends[r] - 1]
            for i in range(k - 1, r + 1):             # the last group is runs i .. r
                c = best[k - 1][i - 1] + (ends[r] - starts[i]) * L + gc
                if c < best[k][r]:
                    best[k][r], cut[k][r] = c, i
    k = min(range(1, G + 1), key=lambda k: (best[k][R - 1], k))
    groups, r = [], R - 1
    while k >= 1:
        i = cut[k][r] if k > 1 else 0
        groups.append((order[starts[i]:ends[r]], need[ends[r] - 1]))
        r, k = i - 1, k - 1
    return groups[::-1]


def plan_cost(plan, group_cost):
    """``sum_g(B_g * L_g) + n_groups * group_cost`` of a plan, the quantity ``plan_groups`` minimises."""
    return sum(len(idx) * L for idx, L in plan) + len(plan) * int(round(group_cost))


def group_records(plan, lengths, Td, C, ld, spf):
    """The two record tables of a plan, as host lists.  Item b's source row is ``z_rows[b]`` ([C][ld] fp32, offset
    ``b * C * ld``); group g's dense bf16 tensor [B_g][L_g][C] starts at ``x_off[g]`` of the packed input arena, its
    fp32 waveform [B_g][L_g * spf] at ``o_off[g]`` of the packed output arena; item b's row of the padded result
    [B][Td * spf] starts at ``b * Td * spf``.  Returns ``(pack [n][5], unpack [n][4], x_off, o_off, x_elems, o_elems)``."""
    pack, unpack, x_off, o_off, xa, oa = [], [], [], [], 0, 0
    for idx, L in plan:
        x_off.append(xa)
        o_off.append(oa)
        for j, b in enumerate(idx):
            n = min(max(int(lengths[b]), 0), Td, L)
            pack.append((b * C * ld, ld, xa + j * L * C, n, L))
            unpack.append((oa + j * L * spf, b * Td * spf, n * spf, Td * spf))
        xa += len(idx) * L * C
        oa += len(idx) * L * spf
    return pack, unpack, x_off, o_off, xa, oa


def pack_groups_host(src, records, C, dst):
    """``ov_pack_groups_cl_bf16`` restated on host tensors (``src`` flat float32, ``dst`` flat bfloat16), record checks
    included: the layout's definition, and what the kernel is compared against."""
    for so, sld, do, cols, L in records:
        if min(so, sld, do, cols) < 0 or L < 1 or cols > L or do + L * C > dst.numel():
            continue
        if cols > 0 and so + (C - 1) * sld + cols > src.numel():
            continue
        rows = torch.as_strided(src, (C, cols), (sld, 1), so)
        blk = dst[do:do + L * C].view(L, C)
        blk[:cols] = rows.t().to(torch.bfloat16)
        blk[cols:] = 0
    return dst


def unpack_groups_host(src, records, dst):
    """``ov_unpack_groups_f32`` restated on flat float32 host tensors, record checks included."""
    for so, do, keep, row in records:
        if min(so, do, keep) < 0 or row < keep or so + keep > src.numel() or do + row > dst.numel():
            continue
        dst[do:do + keep] = src[so:so + keep]
        dst[do + keep:do + row] = 0
    return dst


class GeneratorBf16:
    """HiFi-GAN generator (reference: openvoice/models.py:272-291) with bf16 activations in HBM, channels-last,
    fp32 accumulation -- BASELINE.json configs[4].  Same load-time algebra as the fp32 engine (weight-norm folded,
    ConvTranspose as a 3-tap phase conv, MRF mean folded into the last conv's scale); the residual and the MRF
    running sum are added on the matrix pipe (identity rounds, csrc/conv1d_bf16.hip)."""

    def __init__(self, state_dict, model_cfg, device):
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        cfg = dict(model_cfg.items()) if hasattr(model_cfg, "items") else dict(model_cfg)
        self.cfg, self.device = cfg, torch.device(device)
        dev = self.device
        self.conv_pre = PackedConvBf16(sd["dec.conv_pre.weight"], sd["dec.conv_pre.bias"], dev)
        self.cond_w = sd["dec.cond.weight"][:, :, 0].contiguous().to(dev)
        self.cond_b = (sd["dec.cond.bias"] + sd["dec.conv_pre.bias"]).contiguous().to(dev)   # conv_pre bias folded in
        self.stages = generator_stages(cfg)
        self.ups = []
        for i, cin, co, u, *_ in self.stages:
            wc = conv_transpose_as_conv(effective_weight(sd, f"dec.ups.{i}"), u)      # rows co*u + ph
            wc = wc.reshape(co, u, cin, 3).transpose(0, 1).reshape(u * co, cin, 3)     # rows ph*co + c
            bias = sd[f"dec.ups.{i}.bias"].repeat(u)
            self.ups.append(dict(conv=PackedConvBf16(wc, bias, dev), stride=u))
        layer = lambda name, d: PackedConvBf16(effective_weight(sd, name), sd[name + ".bias"], dev, dil=d)
        convs = list(resblock_convs(cfg))
        self.resblocks = [[[(layer(f"{c.prefix}.convs1.{c.n}", c.dil), layer(f"{c.prefix}.convs2.{c.n}", 1))
                            for c in convs if (c.stage, c.j) == (st.index, j)]
                           for j in range(len(cfg["resblock_kernel_sizes"]))] for st in self.stages]
        self.final_channels = self.stages[-1].ch
        self.post_w = sd["dec.conv_post.weight"][0].contiguous().to(dev)              # [C, 7] fp32
        self._ws = {}
        # ResBlock pairs of the HBM-bound stages as ONE launch each (csrc/conv1d_bf16_pair.hip): C = 32 every kernel
        # size, C = 64 K = 3 -- 1.7-2.0x faster than two launches on MI355X.  The fused kernel is bit-identical to two
        # PLAIN launches (t = bf16(lrelu(bf16(v)))); the unfused pairs below store t activated (out_slope: one rounding,
        # t = bf16(lrelu(v))), which can differ from that by one bf16 ulp of t on negative values -- fuse_pairs on / off
        # therefore agree within bf16 rounding, not bit for bit (tests/test_gpu_bf16_pair.py)
        self.fuse_pairs = True
        # Stages whose every ResBlock pair has a second-generation fused instance (csrc/conv1d_bf16_pair2.hip: C = 64 /
        # 128, every kernel size) keep their tensors ACTIVATED in HBM: the ConvTranspose stores lrelu(u), each pair
        # stores lrelu(x_n), the residual add inverts it in fp32, the chains' sums stay raw (round 4).  False = the
        # round-3 launch sequence (first-generation pairs where they exist, two launches elsewhere).
        self.act_hbm = True
        # independent ResBlock chains of a stage on this many HIP streams (1 = one stream, the serial order).  Measured
        # (round 3, batch 64): 3 streams 45.46 ms vs 45.86 ms on one -- a launch of 2 workgroups per CU owns the chip,
        # so kernels of different streams overlap only at their ramps and tails -- 0.9 %, not worth a default that makes
        # per-kernel profiles harder to read: off unless asked for
        self.chain_streams = 1
        self._streams = []
        # decode_groups: the frames an item is computed beyond its own length.  The bf16 kernels read exactly their taps
        # (no Winograd tiles, no work lists), so this is the direct kernels' margin, not limit_margin_frames
        self.margin = max(GENERATOR_MARGIN, generator_margin_frames(cfg))
        self.samples_per_frame = samples_per_frame(cfg)
        self.max_groups, self.group_cost = DEFAULT_MAX_GROUPS, DEFAULT_GROUP_COST
        self._arena = None
        self.last_plan = None               # plan_groups of the last decode_groups call, for tests / logs

    def _side_streams(self, n):
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(self.device))
        return self._streams[:n]

    def _workspace(self, B, T):
        key = (B, T, self.chain_streams > 1)
        if key not in self._ws:
            self._ws.clear()
            f = lambda n: torch.empty(n, dtype=torch.bfloat16, device=self.device)
            # stage input, ups output, running sum + (t1, ra) per concurrent chain: ONE pair for the default serial order
            # (chain_streams == 1: 5 buffers, 4.5 GB at batch 64), one per chain only when concurrency is on (9, 8.1 GB)
            nbuf = 3 + 2 * (max(1, len(self.cfg["resblock_kernel_sizes"])) if self.chain_streams > 1 else 1)
            self._ws[key] = dict(pre=f(B * T * self.stages[0].cin),
                                 dec=[f(B * T * scratch_per_frame(self.cfg)) for _ in range(nbuf)])
        return self._ws[key]

    def _stage_flags(self, i):
        """``(act, fused, mean_act)`` of stage i, a function of the configuration and of ``fuse_pairs`` / ``act_hbm``:
        ``act`` -- the stage keeps its tensors activated in HBM (second-generation pairs); ``fused[j]`` -- ResBlock j
        runs first-generation fused pairs; ``mean_act`` -- the stage stores its output, the MRF mean, activated."""
        ch = self.stages[i].ch
        nk = len(self.cfg["resblock_kernel_sizes"])
        act = (self.act_hbm and self.fuse_pairs and
               all(pair2_bf16_supported(ch, c1.K, c1.dil) for pairs in self.resblocks[i] for c1, _ in pairs))
        fused = [self.fuse_pairs and all(pair_bf16_supported(ch, c1.K, c1.dil) for c1, _ in pairs)
                 for pairs in self.resblocks[i]]
        # can the launch that writes the MRF mean apply an activation?  (the first-generation fused pair cannot)
        mean_act = i + 1 < len(self.ups) and (act or not fused[nk - 1])
        return act, fused, mean_act

    def stage_scratch_elems(self, i, B, L):
        """Elements of each of the scratch buffers ``stage(i, ...)`` takes for ``B`` rows of ``L`` input columns."""
        return B * L * self.stages[i].stride * self.stages[i].ch

    @torch.no_grad()
    def stage(self, i, x, out, B, L, cond=None, bufs=None, pre=None, side=None):
        """Generator stage ``i`` on caller-given dense channels-last tensors: [conv_pre with the per-row ``cond`` bias
        (stage 0)], the ConvTranspose, the MRF, [conv_post and tanh (last stage)] -- ``decode`` is a loop over it.

        ``x``: bf16 [B, L, C_in].  Stage 0 takes the raw latent ([B, L, inter]) and ``cond`` [B, ch] fp32; a later stage
        takes exactly what stage i - 1 stored: the MRF mean, activated (``lrelu(x)`` in bf16) when that stage's
        ``_stage_flags`` say ``mean_act``, raw otherwise.  ``out``: bf16 [B, L * stride, C_in / 2], or fp32
        [B, 1, L * stride] from the last stage.  ``bufs``: a list of flat bf16 scratch tensors of at least
        ``stage_scratch_elems(i, B, L)`` elements each, none aliasing ``x`` or ``out`` -- 3 are taken from its end (4 by
        the last stage; 2 more per further chain with ``side``); ``pre`` (stage 0): flat bf16 of B * L * ch elements.
        ``side``: the HIP streams of ``chain_streams > 1`` (``decode`` passes them); a live unit leaves it None and its
        launches go to the current stream in the serial order, whatever ``chain_streams`` says."""
        _, cin, ch, s, _, _, last_stage = self.stages[i]
        nk = len(self.cfg["resblock_kernel_sizes"])
        if i == 0:
            p = pre[: B * L * cin].view(B, L, cin)
            # every tensor a ConvTranspose reads is stored ACTIVATED by its producer (conv_pre here, the MRF mean below):
            # its loaders then copy instead of unpacking / activating / re-packing every vector
            _launch(self.conv_pre, x, p, L, bias=cond, bias_bstride=cin, out_slope=LRELU_SLOPE)
            cur_x, cur_act = p, True                      # cur_act: cur_x holds lrelu(x) already
        else:
            cur_x, cur_act = x, self._stage_flags(i - 1)[2]
        act, fused, mean_act = self._stage_flags(i)
        concurrent = side is not None
        u = bufs.pop()[: B * L * s * ch].view(B, L * s, ch)
        _launch(self.ups[i]["conv"], cur_x, u, L, in_slope=1.0 if cur_act else LRELU_SLOPE, phase_s=s,
                out_slope=LRELU_SLOPE if act else 1.0)
        L *= s
        acc = bufs.pop()[: B * L * ch].view(B, L, ch) if last_stage else out
        nchains = nk if concurrent else 1
        scratch = [tuple(bufs.pop()[: B * L * ch].view(B, L, ch) for _ in range(2)) for _ in range(nchains)]
        cur = [u] * nk
        npairs = len(self.resblocks[i][0])

        def pair(j, n):
            c1, c2 = self.resblocks[i][j][n]
            t1, ra = scratch[j if concurrent else 0]
            last = n == npairs - 1
            add = acc if (last and j > 0) else None
            scale = 1.0 / nk if (last and j == nk - 1) else 1.0
            # the MRF mean feeds the next stage's ConvTranspose, which wants it activated; the last stage's feeds
            # conv_post (its own slope, applied there); the chains' partial sums stay raw
            mean_slope = LRELU_SLOPE if (last and j == nk - 1 and mean_act) else 1.0
            if act:            # activated tensors between the launches
                dst = acc if last else (t1 if cur[j] is ra else ra)
                launch_pair2_bf16(c1, c2, cur[j], dst, add=add, scale=scale, slope=LRELU_SLOPE,
                                  out_slope=mean_slope if last else LRELU_SLOPE)
            elif fused[j]:       # one launch per pair, intermediate in LDS; out must not alias x: ra / t1 ping-pong
                dst = acc if last else (t1 if cur[j] is ra else ra)
                launch_pair_bf16(c1, c2, cur[j], dst, add=add, scale=scale, slope=LRELU_SLOPE)
            else:
                # t1 is consumed by c2 only, which activates it: store it activated (one rounding instead of
                # two) and let c2's loaders copy it as is
                _launch(c1, cur[j], t1, L, in_slope=LRELU_SLOPE, out_slope=LRELU_SLOPE)
                dst = acc if last else ra
                _launch(c2, t1, dst, L, in_slope=1.0, res=cur[j], add=add, scale=scale, out_slope=mean_slope)
            cur[j] = dst

        if not concurrent:
            for j in range(nk):
                for n in range(npairs):
                    pair(j, n)
        else:
            main = torch.cuda.current_stream(self.device)
            fork = torch.cuda.Event()
            fork.record(main)
            done = [None] * nk
            for n in range(npairs):                 # round-robin over the chains: every queue has work early
                for j in range(nk):
                    with torch.cuda.stream(side[j]):
                        if n == 0:
                            side[j].wait_event(fork)
                        if n == npairs - 1 and j > 0:
                            side[j].wait_event(done[j - 1])      # the running sum is accumulated in chain order
                        pair(j, n)
                        if n == npairs - 1:
                            done[j] = torch.cuda.Event()
                            done[j].record(side[j])
            main.wait_event(done[nk - 1])
        if last_stage:
            _lib.call("ov_conv_post_tanh_bf16", acc, self.post_w, out, B, ch, L, self.post_w.shape[1], FINAL_LRELU_SLOPE)

    @torch.no_grad()
    def decode(self, z, g):
        """``z`` [B, inter, T] fp32 (channels-first, as the flow produces it), ``g`` [B or 1, gin, 1] ->
        waveform [B, 1, T * prod(upsample_rates)] fp32."""
        dev = self.device
        B, C, T = z.shape
        ws = self._workspace(B, T)
        x = z.to(dev, torch.float32).transpose(1, 2).to(torch.bfloat16).contiguous()        # [B, T, C] bf16
        cond = self.cond_rows(g).expand(B, -1).contiguous()                                  # [B, 512] fp32
        nk = len(self.cfg["resblock_kernel_sizes"])
        # The three ResBlocks of a stage (k = 3, 7, 11) are independent chains until the MRF sum.  In bf16 they bound
        # DIFFERENT resources -- the k = 3 convs HBM (3.4 TB/s at 33 % matrix-busy), the k = 11 convs the power-limited
        # matrix pipe (60 % busy at 1.5 TB/s) -- so with chain_streams > 1 they are issued on separate HIP streams;
        # the sum keeps its order (chain j's last launch waits for chain j - 1's), so the result is bit-identical to
        # the serial order.  Not under graph capture (the engine captures on one stream).
        concurrent = self.chain_streams > 1 and nk > 1 and not torch.cuda.is_current_stream_capturing()
        side = self._side_streams(nk) if concurrent else None
        out = torch.empty(B, 1, T * self.samples_per_frame, dtype=torch.float32, device=dev)
        self._decode_dense(x, cond, out, B, T, ws["dec"], ws["pre"], side)
        return out

    def _group_arena(self, x_elems, o_elems, rows_frames):
        """The buffers of ``decode_groups``, kept across calls and only ever grown (``_workspace`` would drop its cache at
        every new (B, T)): the groups' packed bf16 inputs and fp32 outputs, and ONE set of stage scratch sized for the
        plan's largest group (``rows_frames`` = its B_g * L_g)."""
        want = dict(x=x_elems, o=o_elems, pre=rows_frames * self.stages[0].cin,
                    dec=rows_frames * scratch_per_frame(self.cfg))
        a = self._arena
        if a is None or any(a["size"][k] < n for k, n in want.items()):
            size = want if a is None else {k: max(n, a["size"][k]) for k, n in want.items()}
            self._arena = a = None              # free the old buffers before the new ones are taken
            f = lambda n: torch.empty(max(n, 8), dtype=torch.bfloat16, device=self.device)
            a = dict(size=size, x=f(size["x"]), pre=f(size["pre"]), dec=[f(size["dec"]) for _ in range(5)],
                     o=torch.empty(max(size["o"], 4), dtype=torch.float32, device=self.device))
            self._arena = a
        return a

    @torch.no_grad()
    def decode_groups(self, z_rows, ld, cond, lengths_host, Td, max_groups=None):
        """``decode`` of a ragged batch as a few dense groups.  ``z_rows``: fp32 [B, inter, ld] contiguous, as the flow
        leaves it in the workspace -- item b valid (and zero beyond its own length, the flow's mask) on its first
        ``lengths_host[b]`` columns; the columns beyond an item's length are never read.  ``cond``: the conv_pre bias
        rows [B or 1, ch] fp32 (``cond_rows``); ``lengths_host``: a HOST sequence of B ints; ``Td``: the frames of the
        padded run; ``max_groups``: None = ``self.max_groups``, at most ``MAX_GROUPS_CAP``.  Returns fp32
        [B, 1, Td * samples_per_frame]: samples ``[0, length_b * spf)`` of row b are the bits ``decode`` of the padded
        batch ``z_rows[:, :, :Td]`` gives, every sample beyond them is zero.

        One ``ov_pack_groups_cl_bf16`` launch, per group (``plan_groups``) the loop over ``stage`` that ``decode`` runs,
        at the group's own ``L_g``, one ``ov_unpack_groups_f32`` launch; the chains of a stage stay on one stream."""
        dev = self.device
        B, C = int(z_rows.shape[0]), int(z_rows.shape[1])
        ld, Td = int(ld), int(Td)
        if (z_rows.dtype != torch.float32 or z_rows.dim() != 3 or not z_rows.is_contiguous() or z_rows.shape[2] != ld
                or z_rows.device != dev or C != self.conv_pre.cin):
            raise _lib.OvError(f"decode_groups: z_rows must be a contiguous float32 [B, {self.conv_pre.cin}, ld] tensor on "
                               f"{dev}, got {tuple(z_rows.shape)} {z_rows.dtype} on {z_rows.device}")
        lens = [int(n) for n in lengths_host]
        if len(lens) != B or not 1 <= Td <= ld:
            raise _lib.OvError(f"decode_groups: {len(lens)} lengths for {B} rows, Td = {Td}, ld = {ld}")
        G = self.max_groups if max_groups is None else int(max_groups)
        if G < 1:
            raise _lib.OvError(f"decode_groups: max_groups = {max_groups}")
        plan = plan_groups(lens, Td, self.margin, min(G, MAX_GROUPS_CAP), self.group_cost)
        self.last_plan = plan
        spf = self.samples_per_frame
        pack, unpack, x_off, o_off, x_elems, o_elems = group_records(plan, lens, Td, C, ld, spf)
        arena = self._group_arena(x_elems, o_elems, max(len(idx) * L for idx, L in plan))
        # one host -> device copy: both record tables and the batch order of the plan
        order = [b for idx, _ in plan for b in idx]
        table = torch.tensor([v for r in pack for v in r] + [v for r in unpack for v in r] + order,
                             dtype=torch.int64).to(dev)
        n_pack, n_unpack = B * PACK_FIELDS, B * UNPACK_FIELDS
        _lib.call("ov_pack_groups_cl_bf16", z_rows, z_rows.numel(), table[:n_pack], B, C, arena["x"],
                  arena["x"].numel())
        cond = cond.to(dev, torch.float32)
        if cond.shape[0] == 1:
            cond_sorted = cond.reshape(1, -1).expand(B, -1).contiguous()
        else:
            cond_sorted = cond.reshape(B, -1).index_select(0, table[n_pack + n_unpack:])
        at = 0
        for (idx, L), xo, oo in zip(plan, x_off, o_off):
            Bg = len(idx)
            x = arena["x"][xo: xo + Bg * L * C].view(Bg, L, C)
            out = arena["o"][oo: oo + Bg * L * spf].view(Bg, 1, L * spf)
            self._decode_dense(x, cond_sorted[at:at + Bg], out, Bg, L, arena["dec"], arena["pre"])
            at += Bg
        o = torch.empty(B, 1, Td * spf, dtype=torch.float32, device=dev)
        _lib.call("ov_unpack_groups_f32", arena["o"], arena["o"].numel(), table[n_pack:n_pack + n_unpack], B, o, o.numel())
        return o

    def _decode_dense(self, x, cond, out, B, T, dec, pre, side=None):
        """The stage loop on caller-given buffers: ``x`` bf16 [B, T, inter], ``cond`` [B, ch] (contiguous rows), ``out``
        fp32 [B, 1, T * spf], ``dec`` the flat bf16 scratch buffers (five; two more per further chain with ``side``, the
        HIP streams of ``chain_streams > 1``), ``pre`` the conv_pre output."""
        cur_x, free = x, list(dec)
        for i, _, ch, _, rate_in, rate_out, last in self.stages:
            # the ups output takes the last free buffer, the stage's output the one before it
            o = out if last else free.pop(-2)[: B * T * rate_out * ch].view(B, T * rate_out, ch)
            self.stage(i, cur_x, o, B, T * rate_in, cond=cond if i == 0 else None, bufs=free, pre=pre, side=side)
            # every scratch buffer except the one holding this stage's output is free again
            free = [buf for buf in dec if buf.data_ptr() != o.data_ptr()]
            cur_x = o

    def cond_rows(self, g):
        """``g`` [rows, gin(, 1)] -> the conv_pre bias rows [rows, ch] fp32 (dec.cond + both biases), as ``decode``
        computes them."""
        g2 = g.to(self.device, torch.float32).reshape(g.shape[0], -1).contiguous()
        cond = torch.empty(g2.shape[0], self.cond_w.shape[0], dtype=torch.float32, device=self.device)
        _lib.call("ov_linear_f32", g2, self.cond_w, self.cond_b, cond, g2.shape[0], self.cond_w.shape[0],
                  self.cond_w.shape[1])                                                      # dec.cond, T = 1 GEMV
        return cond
