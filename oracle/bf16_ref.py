"""ORACLE (test infrastructure, never the product path): float64 mirrors of the bf16 generator kernels and an
element-wise acceptance limit.  Plain PyTorch on the CPU; only ``tests/`` imports it.

The kernels (openvoice_amd/csrc/conv1d_bf16.hip, conv1d_bf16_pair.hip, conv1d_bf16_pair2.h) read bf16 operands,
accumulate in fp32 and round to nearest even ONCE per stored value.  A correct kernel is therefore within half a bf16
ulp of the exact result plus its fp32 summation error, on EVERY element:

    |out - ref64| <= 0.5 * ulp_bf16(ref64) + S * absacc (+ flip)                                  (``limit``)

``ref64``  the mirror below: same bf16-rounded operands, same roundings at the same storage points, float64 sums;
           it is the value BEFORE the last rounding (the kernel's stored value is its rounding).
``absacc`` the same expression on absolute values (sum |x| |w| + |bias| + |res| + |add|, times |scale|): the
           quantity fp32 summation error is proportional to.
``flip``   fused pairs only.  An intermediate t whose fp32 pre-rounding value lies on the other side of a bf16
           rounding midpoint than the float64 one is stored one grid step away, and shifts every output it feeds by
           that step times |w2|.  An element of t is *ambiguous* when its float64 pre-rounding value lies within
           ``S * absacc1`` of a midpoint; ``flip = conv(|w2|, ambiguous * gap)`` with ``gap`` the distance between the
           two values t can take (one ulp of t for the second-generation pair; for the first generation's
           t = bf16(lrelu(bf16(v))) the two candidates of bf16(v) are both pushed through the second rounding, so the
           gap is exact: 0.1 ulp of v re-rounded is up to two ulps of t).

S, the fp32 accumulation allowance -- measured, reference against reference, never from a kernel
-------------------------------------------------------------------------------------------------
``python -m oracle.bf16_ref`` prints max |conv_fp32 - conv_fp64| / absacc of PyTorch's CPU fp32 conv on the test
files' operand generators (x = bf16(lrelu(bf16(randn))), w = bf16(randn (C K)^-1/2), L = 600, B = 2), five seeds,
for every parametrised (C, K, d):

    C =  32: k3d1 1.12e-07  k3d3 1.59e-07  k3d5 1.52e-07  k7d1 1.22e-07  k7d3 1.30e-07  k7d5 1.30e-07  k11d1 1.25e-07  k11d3 1.30e-07  k11d5 1.30e-07
    C =  64: k3d1 9.27e-08  k3d3 9.69e-08  k3d5 9.17e-08  k7d1 7.86e-08  k7d3 8.69e-08  k7d5 9.52e-08  k11d1 8.26e-08  k11d3 7.93e-08  k11d5 7.79e-08
    C = 128: k3d1 6.80e-08  k3d3 7.18e-08  k3d5 6.96e-08  k7d1 6.19e-08  k7d3 5.59e-08  k7d5 5.92e-08  k11d1 5.02e-08  k11d3 5.06e-08  k11d5 5.97e-08
    C = 256: k3d1 6.60e-08  k3d3 6.35e-08  k3d5 6.22e-08  k7d1 4.67e-08  k7d3 4.58e-08  k7d5 5.06e-08  k11d1 4.01e-08  k11d3 4.26e-08  k11d5 4.39e-08
    largest 1.592e-07 = 2^-22.58 (about 1.3 fp32 ulps of absacc)

The kernels sum in MFMA order with up to 11 x 256 terms, PyTorch in its own: factor 4 on the largest value.

    S = 4 * 1.592e-07 = 6.4e-07 (2^-20.6)

At this S 0.7 % - 2.3 % of the first-generation pair's t and 2.8 % - 8.5 % of the second generation's are ambiguous at
(C, K, d) = (32, 3, 1) ... (128, 11, 5) (tests/test_bf16_criterion_cpu.py prints them and asserts < 1/2); the honest
fp32 stand-in lands at a worst err / lim of 0.990 - 1.000 there, every wrong variant above 1.3.

The mirrors take channels-last (B, L, C) tensors like the kernels.  ``dtype=torch.float32`` evaluates the same mirror
with fp32 PyTorch convs and ``.bfloat16()`` roundings: the honest stand-in for a correct kernel, and the second
reference of the per-stage noise floors."""
import math

import numpy as np
import torch
import torch.nn.functional as F

S = 6.4e-7              # 4 x the largest measured value (docstring); never widened to make a kernel pass

F64 = torch.float64


def f32(v):
    """The fp32 value of a Python float, as a Python float (what a kernel receives through a ``float`` field)."""
    return float(np.float32(v))


def ulp_bf16(x):
    """Spacing of the bf16 grid in the binade of |x| (8 significant bits; the tests stay far from subnormals)."""
    _, e = torch.frexp(x.to(F64).abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(x, dtype=F64), e - 8)


def rbf16(x):
    """Round to the nearest bf16, ties to even, DIRECTLY from the given precision (float64 is not rounded to fp32
    first: that would be a double rounding the kernels do not perform on an fp32 accumulator)."""
    if x.dtype != F64:
        return x.to(torch.bfloat16).to(x.dtype)
    u = ulp_bf16(x)
    return torch.round(x / u) * u            # torch.round: half to even; x / u is exact (u a power of two)


def bf16_neighbours(x):
    """(lo, hi): the two bf16 grid points around float64 ``x`` in its binade, lo <= x <= hi in magnitude order of the
    real line (hi - lo = one ulp; lo == x when x is on the grid)."""
    u = ulp_bf16(x)
    lo = torch.floor(x / u) * u
    return lo, lo + u


def _lrelu(x, slope):
    """Leaky ReLU as the kernels evaluate it: v > 0 ? v : v * slope with the fp32 slope."""
    if slope == 1.0:
        return x
    return torch.where(x > 0, x, x * f32(slope))


def act_store(x, slope):
    """bf16(lrelu(x)) of a bf16-exact tensor as a loader stages it: the product with the fp32 slope is rounded to fp32
    (exact in float64: 8 x 24 bits) and then to bf16."""
    if slope == 1.0:
        return x
    return _lrelu(x, slope).float().to(torch.bfloat16).to(x.dtype)


def _conv(x, w, dil=1):
    """x (B, L, Cin), w (Cout, Cin, K) -> (B, L, Cout), 'same' padding."""
    k = w.shape[-1]
    return F.conv1d(x.transpose(1, 2), w, None, dilation=dil, padding=(k - 1) * dil // 2).transpose(1, 2)


def _conv_abs(x, w, dil=1):
    return _conv(x.abs(), w.abs(), dil)


def _opt(t, dtype):
    return None if t is None else t.to(dtype)


def conv_single(x, w, bias=None, dil=1, in_slope=1.0, res=None, add=None, scale=1.0, out_slope=1.0,
                bias_rows=None, dtype=F64):
    """``ov_conv1d_bf16cl``: out = bf16(lrelu((conv(bf16(lrelu(x, in_slope))) + bias [+ res] [+ add]) * scale,
    out_slope)).  ``bias_rows`` [B, Cout]: the per-utterance bias (conv_pre).  Returns ``(ref, absacc)``, ``ref``
    before the output rounding."""
    x, w = x.to(dtype), w.to(dtype)
    xin = act_store(x, in_slope)
    acc, absacc = _conv(xin, w, dil), _conv_abs(xin, w, dil)
    for t in (_opt(bias, dtype), None if bias_rows is None else bias_rows.to(dtype)[:, None, :],
              _opt(res, dtype), _opt(add, dtype)):
        if t is not None:
            acc, absacc = acc + t, absacc + t.abs()
    s = f32(scale)
    return _lrelu(acc * s, out_slope), absacc * abs(s)


def conv_transpose(x, w, bias, stride, in_slope=1.0, out_slope=1.0, dtype=F64):
    """The ConvTranspose1d (kernel 2 * stride, padding stride / 2) the kernels run as a 3-tap phase conv: the same
    products, two per output element.  ``w`` [Cin, Cout, 2 * stride] (torch layout).  Returns ``(ref, absacc)``."""
    x, w, bias = x.to(dtype), w.to(dtype), bias.to(dtype)
    xin = act_store(x, in_slope).transpose(1, 2)
    acc = F.conv_transpose1d(xin, w, bias, stride=stride, padding=stride // 2).transpose(1, 2)
    absacc = F.conv_transpose1d(xin.abs(), w.abs(), bias.abs(), stride=stride, padding=stride // 2).transpose(1, 2)
    return _lrelu(acc, out_slope), absacc


def pair1(x, w1, b1, w2, b2, dil, add=None, scale=1.0, slope=0.1, dtype=F64):
    """First-generation fused pair (``ov_resblock_pair_bf16cl``, and the two plain launches it is bit-identical to):
    t = bf16(lrelu(bf16(c1(bf16(lrelu(x))) + b1))), out = bf16((c2(t) + b2 + x [+ add]) * scale).
    Returns ``(ref, absacc, inter)``; ``inter``: the pre-rounding value of t (``v1``), its ``absacc1``, the two
    values t can take (``gap`` = their distance), ``w2`` and ``scale`` -- what ``flip`` needs."""
    x, w1, b1, w2, b2 = (t.to(dtype) for t in (x, w1, b1, w2, b2))
    xin = act_store(x, slope)
    v1, abs1 = _conv(xin, w1, dil) + b1, _conv_abs(xin, w1, dil) + b1.abs()
    t = act_store(rbf16(v1), slope)
    acc, absacc = _conv(t, w2) + b2 + x, _conv_abs(t, w2) + b2.abs() + x.abs()
    if add is not None:
        acc, absacc = acc + add.to(dtype), absacc + add.to(dtype).abs()
    s = f32(scale)
    lo, hi = bf16_neighbours(v1.to(F64))
    gap = (act_store(hi, slope) - act_store(lo, slope)).abs()
    return acc * s, absacc * abs(s), dict(v1=v1, absacc1=abs1, gap=gap, w2=w2, scale=abs(s))


def pair2(xa, w1, b1, w2, b2, dil, add=None, scale=1.0, slope=0.1, out_slope=1.0, dtype=F64):
    """Second-generation fused pair (``ov_resblock_pair2_bf16cl``) on the ACTIVATED input xa = bf16(lrelu(x)):
    t = bf16(lrelu(c1(xa) + b1)); x~ = xa >= 0 ? xa : xa * fp32(1 / slope) (rounded to fp32);
    y = c2(t) + b2 + x~; out = bf16(lrelu(y * scale, out_slope)), or with the running sum
    out = bf16(lrelu((bf16(y) + add) * scale, out_slope)) (conv1d_bf16_pair2.h:5-7, 245-247).
    Returns ``(ref, absacc, inter)``; with ``add`` ``inter`` also carries ``y`` (pre-rounding) and its ``absacc_y``."""
    xa, w1, b1, w2, b2 = (t.to(dtype) for t in (xa, w1, b1, w2, b2))
    v1, abs1 = _conv(xa, w1, dil) + b1, _conv_abs(xa, w1, dil) + b1.abs()
    a1 = _lrelu(v1, slope)
    t = rbf16(a1)
    inv = float(np.float32(1.0) / np.float32(slope))
    x_raw = torch.where(xa >= 0, xa, (xa * inv).float().to(dtype))
    y, absy = _conv(t, w2) + b2 + x_raw, _conv_abs(t, w2) + b2.abs() + x_raw.abs()
    s = f32(scale)
    lo, hi = bf16_neighbours(a1.to(F64))
    inter = dict(v1=a1, absacc1=abs1, gap=hi - lo, w2=w2, scale=abs(s))
    if add is None:
        return _lrelu(y * s, out_slope), absy * abs(s), inter
    add = add.to(dtype)
    yr = rbf16(y)
    inter.update(y=y, absacc_y=absy)
    return _lrelu((yr + add) * s, out_slope), (yr.abs() + add.abs()) * abs(s), inter


def ambiguous(v, tol):
    """Elements of float64 ``v`` within ``tol`` of a bf16 rounding midpoint."""
    lo, hi = bf16_neighbours(v.to(F64))
    return (v.to(F64) - 0.5 * (lo + hi)).abs() <= tol


def flip(inter, s=None):
    """The allowance for intermediates that may round the other way than in float64 (module docstring)."""
    s = S if s is None else s
    amb = ambiguous(inter["v1"], s * inter["absacc1"].to(F64))
    f = _conv(amb.to(F64) * inter["gap"], inter["w2"].to(F64).abs())
    if "y" in inter:
        # bf16(y) of the running-sum form is stored too: ambiguous within its own fp32 error plus what t's flips moved
        ulp_y = ulp_bf16(inter["y"])
        amb_y = ambiguous(inter["y"], s * inter["absacc_y"].to(F64) + f)
        f = f + amb_y.to(F64) * ulp_y
    return f * inter["scale"]


def ambiguous_share(inter, s=None):
    s = S if s is None else s
    return ambiguous(inter["v1"], s * inter["absacc1"].to(F64)).double().mean().item()


def limit(ref64, absacc, flip=None, s=None):
    """0.5 * ulp_bf16(ref64) + S * absacc (+ flip).  The ulp is taken at |ref64| + the fp32 allowance: an fp32
    accumulator that lands just across a power of two from ref64 is rounded on the coarser grid."""
    s = S if s is None else s
    slack = s * absacc.to(F64)
    if flip is not None:
        slack = slack + flip
    return 0.5 * ulp_bf16(ref64.to(F64).abs() + slack) + slack


def worst_ratio(out, ref64, lim):
    err = (out.detach().to("cpu", F64) - ref64.to(F64)).abs()
    return (err / lim).max().item()


WORST = {}              # family -> worst err / lim seen in this process (the GPU files print it per family)


def assert_within(out, ref64, lim, what, family=None):
    """``out`` (any device / dtype) against the float64 mirror, element by element.  NaN fails."""
    o = out.detach().to("cpu", F64)
    assert o.shape == ref64.shape, (what, o.shape, ref64.shape)
    err = (o - ref64.to(F64)).abs()
    ratio = torch.where(torch.isfinite(err), err / lim, torch.full_like(err, float("inf")))
    worst = ratio.max().item()
    if family is not None:
        WORST[family] = max(WORST.get(family, 0.0), worst)
        print(f"[bf16 criterion] {family}: {what}: worst err/lim {worst:.4f} (family so far {WORST[family]:.4f})")
    if worst > 1.0:
        idx = np.unravel_index(int(ratio.argmax()), tuple(ratio.shape))
        bad = int((ratio > 1.0).sum())
        raise AssertionError(f"{what}: worst err/lim {worst:.3f} at {tuple(int(i) for i in idx)} (out {o[idx].item():.9g}, "
                             f"ref64 {ref64[idx].item():.9g}, lim {lim[idx].item():.3e}); {bad} of {ratio.numel()} "
                             f"elements over the limit")
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# The generator, stage by stage
# ---------------------------------------------------------------------------------------------------------------------
class GeneratorMirror:
    """The weights of ``openvoice_amd.bf16.GeneratorBf16`` as the kernels see them: weight-norm folded in fp32, conv
    weights rounded to bf16 (``ov_conv1d_bf16_pack``: nearest even), biases and conv_post in fp32."""

    def __init__(self, sd, cfg):
        from openvoice_amd.params import effective_weight
        sd = {k: v.detach().float().cpu() for k, v in sd.items()}
        r = lambda w: w.to(torch.bfloat16).float()
        self.cfg = cfg = dict(cfg.items())
        self.pre_w = r(sd["dec.conv_pre.weight"])
        self.cond_w, self.cond_b = sd["dec.cond.weight"][:, :, 0], sd["dec.cond.bias"] + sd["dec.conv_pre.bias"]
        self.ups, self.resblocks = [], []
        nk = len(cfg["resblock_kernel_sizes"])
        for i, u in enumerate(cfg["upsample_rates"]):
            self.ups.append((r(effective_weight(sd, f"dec.ups.{i}")), sd[f"dec.ups.{i}.bias"], u))
            stage = []
            for j, rd in enumerate(cfg["resblock_dilation_sizes"]):
                rb = f"dec.resblocks.{i * nk + j}"
                stage.append([(r(effective_weight(sd, f"{rb}.convs1.{n}")), sd[f"{rb}.convs1.{n}.bias"],
                               r(effective_weight(sd, f"{rb}.convs2.{n}")), sd[f"{rb}.convs2.{n}.bias"], d)
                              for n, d in enumerate(rd)])
            self.resblocks.append(stage)
        self.post_w = sd["dec.conv_post.weight"][0]                     # [C, 7] fp32

    def cond_rows(self, g, dtype=F64):
        """dec.cond(g) + both biases: the per-row conv_pre bias ``GeneratorBf16.cond_rows`` computes, [rows, ch]."""
        return (g.reshape(g.shape[0], -1).to(dtype) @ self.cond_w.to(dtype).t() + self.cond_b.to(dtype)).float()


def conv_post_tanh(x, post_w, slope, dtype=F64):
    """``ov_conv_post_tanh_bf16``: tanh(conv1d(lrelu(x, slope), w)), x (B, L, C) bf16-exact, ``post_w`` [C, K] fp32,
    no bias, fp32 output [B, 1, L]; the activation is NOT re-rounded (it stays in fp32 registers).
    Returns ``(ref, absacc)`` with ``absacc`` of the conv sum (tanh' <= 1)."""
    x, w = x.to(dtype), post_w.to(dtype)[None]
    xin = _lrelu(x, slope)
    acc, absacc = _conv(xin, w), _conv_abs(xin, w)
    return torch.tanh(acc).transpose(1, 2), absacc.transpose(1, 2)


def generator_stage(gm, i, x, flags, in_act=False, cond=None, dtype=F64, slope=0.1, final_slope=0.01):
    """Mirror of ``GeneratorBf16.stage(i, ...)`` (openvoice_amd/bf16.py) for the ``flags = (act, fused, mean_act)``
    its ``_stage_flags(i)`` returns and ``in_act = _stage_flags(i - 1)[2]``: which tensors are stored activated, which
    pairs are fused (first generation: double rounding of t), where the running sum joins (the last pair of chains
    j > 0; on the rounded pair output in the activated form), the MRF scale 1 / nk on the last chain's last pair, the
    activated mean.  ``x`` (B, L, C) bf16-exact: the raw latent (stage 0, with ``cond`` [B, ch] fp32) or what stage
    i - 1 stored.  Returns what the stage stores: (B, L * stride, C / 2) bf16-exact, or the fp32 waveform
    [B, 1, L * stride] from the last stage (not rounded to fp32 in float64 mode)."""
    act, fused, mean_act = flags
    nstage, nk = len(gm.ups), len(gm.resblocks[i])
    x = x.to(dtype)
    if i == 0:
        v, _ = conv_single(x, gm.pre_w, bias_rows=cond, out_slope=slope, dtype=dtype)
        cur, cur_act = rbf16(v), True
    else:
        cur, cur_act = x, in_act
    w, b, s = gm.ups[i]
    v, _ = conv_transpose(cur, w, b, s, in_slope=1.0 if cur_act else slope, out_slope=slope if act else 1.0, dtype=dtype)
    u = rbf16(v)
    acc = None
    for j in range(nk):
        cur = u
        npairs = len(gm.resblocks[i][j])
        for n, (w1, b1, w2, b2, d) in enumerate(gm.resblocks[i][j]):
            last = n == npairs - 1
            add = acc if (last and j > 0) else None
            scale = 1.0 / nk if (last and j == nk - 1) else 1.0
            mean_slope = slope if (last and j == nk - 1 and mean_act) else 1.0
            if act:
                v = pair2(cur, w1, b1, w2, b2, d, add=add, scale=scale, slope=slope,
                          out_slope=mean_slope if last else slope, dtype=dtype)[0]
            elif fused[j]:
                v = pair1(cur, w1, b1, w2, b2, d, add=add, scale=scale, slope=slope, dtype=dtype)[0]
            else:
                t = rbf16(conv_single(cur, w1, b1, dil=d, in_slope=slope, out_slope=slope, dtype=dtype)[0])
                v = conv_single(t, w2, b2, res=cur, add=add, scale=scale, out_slope=mean_slope, dtype=dtype)[0]
            cur = rbf16(v)
        acc = cur
    if i == nstage - 1:
        return conv_post_tanh(acc, gm.post_w, final_slope, dtype=dtype)[0]
    return acc


def reference_stage_flags(cfg, i, fuse_pairs, act_hbm, pair_supported, pair2_supported):
    """``GeneratorBf16._stage_flags`` restated on the two ``*_supported`` predicates (host-side table look-ups of the
    kernel library), so that the CPU measurements below use the launch sequence the GPU takes."""
    ch = cfg["upsample_initial_channel"] >> (i + 1)
    kd = [[(k, d) for d in rd] for k, rd in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])]
    act = act_hbm and fuse_pairs and all(pair2_supported(ch, k, d) for pairs in kd for k, d in pairs)
    fused = [fuse_pairs and all(pair_supported(ch, k, d) for k, d in pairs) for pairs in kd]
    mean_act = i + 1 < len(cfg["upsample_rates"]) and (act or not fused[-1])
    return act, fused, mean_act


def generator_decode(gm, z, g, flags_of, dtype=F64):
    """Mirror of ``GeneratorBf16.decode``: ``z`` [B, inter, T] fp32, ``g`` [B or 1, gin, 1]; ``flags_of(i)`` returns
    stage i's flags."""
    x = z.float().transpose(1, 2).to(torch.bfloat16).float()
    cond = gm.cond_rows(g).expand(z.shape[0], -1)
    for i in range(len(gm.ups)):
        x = generator_stage(gm, i, x, flags_of(i), in_act=flags_of(i - 1)[2] if i else False,
                            cond=cond if i == 0 else None, dtype=dtype)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# Measurements (reference against reference): python -m oracle.bf16_ref [S | stages]
# ---------------------------------------------------------------------------------------------------------------------
KD = [(3, 1), (3, 3), (3, 5), (7, 1), (7, 3), (7, 5), (11, 1), (11, 3), (11, 5)]


def _rand(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def measure_s(channels=(32, 64, 128, 256), seeds=5, L=600, B=2):
    """max |conv_fp32 - conv_fp64| / absacc per (C, K, d) over ``seeds`` seeds; returns {(C, K, d): value}."""
    r = lambda t: t.to(torch.bfloat16).float()
    table = {}
    for c in channels:
        for k, d in KD:
            worst = 0.0
            for seed in range(seeds):
                x = r(F.leaky_relu(r(_rand(B, L, c, seed=100 * seed + 1)), 0.1))
                w = r(_rand(c, c, k, seed=100 * seed + 4, scale=(c * k) ** -0.5))
                e = (_conv(x, w, d).double() - _conv(x.double(), w.double(), d)).abs() / _conv_abs(x.double(), w.double(), d)
                worst = max(worst, e.max().item())
            table[(c, k, d)] = worst
    return table


def conv_post_case(L, B=3, C=32, K=7):
    """Inputs of the conv_post test at length ``L``: bf16-exact x (B, L, C) and weights [C, K]."""
    r = lambda t: t.to(torch.bfloat16).float()
    return r(_rand(B, L, C, seed=L)), r(_rand(C, K, seed=1000 + L, scale=(C * K) ** -0.5))


CONV_POST_LENGTHS = (1, 3, 6, 7, 255, 256, 257, 262, 513)


def measure_conv_post(slope=0.01):
    """max |fp32 PyTorch - float64| of tanh(conv1d(lrelu(x))) over the test's lengths."""
    worst = 0.0
    for L in CONV_POST_LENGTHS:
        x, w = conv_post_case(L)
        worst = max(worst, (conv_post_tanh(x, w, slope, dtype=torch.float32)[0].double()
                            - conv_post_tanh(x, w, slope)[0]).abs().max().item())
    return worst


STAGE_B, STAGE_L = 2, 9
STAGE_SETTINGS = [(True, True), (True, False), (False, True), (False, False)]        # (fuse_pairs, act_hbm)


def stage_cases(gm, flags_of, seed):
    """The per-stage inputs of the stage tests under one setting: ``[(x, in_act, cond)]``.  Stage 0 takes a bf16-rounded
    random latent (B = 2, L = 9) and the cond rows of a random g; stage i > 0 takes the first 9 time rows of what the
    float64 MIRROR of stage i - 1 stores (bf16-exact), so that errors do not chain across stages."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(STAGE_B, STAGE_L, gm.pre_w.shape[1], generator=gen).to(torch.bfloat16).float()
    cond = gm.cond_rows(0.3 * torch.randn(STAGE_B, gm.cond_w.shape[1], 1, generator=gen))
    cases = []
    for i in range(len(gm.ups)):
        in_act = flags_of(i - 1)[2] if i else False
        cases.append((x, in_act, cond if i == 0 else None))
        if i + 1 < len(gm.ups):
            x = generator_stage(gm, i, x, flags_of(i), in_act=in_act, cond=cases[-1][2])[:, :STAGE_L].float().contiguous()
    return cases


def measure_stage_floors(gm, flags_of, seeds=5):
    """Per stage, the largest (rms, max-abs) difference over ``seeds`` seeds between the fp32-order mirror and the
    float64 mirror of that stage on the same input."""
    floors = [(0.0, 0.0)] * len(gm.ups)
    for seed in range(seeds):
        for i, (x, in_act, cond) in enumerate(stage_cases(gm, flags_of, seed)):
            a = generator_stage(gm, i, x, flags_of(i), in_act=in_act, cond=cond)
            b = generator_stage(gm, i, x, flags_of(i), in_act=in_act, cond=cond, dtype=torch.float32).double()
            d = a - b
            floors[i] = (max(floors[i][0], d.pow(2).mean().sqrt().item()), max(floors[i][1], d.abs().max().item()))
    return floors


def _main_stages(seeds):
    from openvoice_amd.bf16 import pair2_bf16_supported, pair_bf16_supported
    from openvoice_amd.params import synthetic_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    from oracle import vc_oracle
    sd = synthetic_state_dict(CFG, 513, seed=1234)
    gm = GeneratorMirror(sd, CFG)
    for fuse, act in STAGE_SETTINGS:
        flags_of = lambda i: reference_stage_flags(gm.cfg, i, fuse, act, pair_bf16_supported, pair2_bf16_supported)
        print(f"fuse_pairs={fuse} act_hbm={act}: flags {[flags_of(i) for i in range(len(gm.ups))]}")
        print("   floors (rms, max-abs) per stage: " + ", ".join(f"({r:.3e}, {m:.3e})" for r, m in measure_stage_floors(gm, flags_of, seeds)))
    print(f"conv_post: fp32 PyTorch against float64 {measure_conv_post():.3e}")
    flags_of = lambda i: reference_stage_flags(gm.cfg, i, True, True, pair_bf16_supported, pair2_bf16_supported)
    gen = torch.Generator().manual_seed(9)
    z, g = torch.randn(2, 192, 9, generator=gen), 0.3 * torch.randn(2, 256, 1, generator=gen)
    with torch.no_grad():
        ref = vc_oracle.generator(sd, z, g, CFG)
    err = generator_decode(gm, z, g, flags_of) - ref.double()
    print(f"decode mirror (float64 sums, bf16 storage) against the fp32 oracle, B=2 T=9: max-abs {err.abs().max().item():.3e}, "
          f"rel RMS {(err.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()).item():.3e}")


if __name__ == "__main__":
    import sys
    if sys.argv[1:2] == ["stages"]:
        _main_stages(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
        sys.exit(0)
    tab = measure_s()
    for c in (32, 64, 128, 256):
        print(f"C = {c:3d}: " + "  ".join(f"k{k}d{d} {tab[(c, k, d)]:.2e}" for k, d in KD))
    m = max(tab.values())
    print(f"largest {m:.3e} = 2^{math.log2(m):.2f}; x 4 = {4 * m:.3e} = 2^{math.log2(4 * m):.2f}")
