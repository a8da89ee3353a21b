"""ORACLE (test infrastructure, never the product path): float64 mirrors of the frame-rate fp32 conv epilogues and an
element-wise acceptance limit.  Plain PyTorch on the CPU; only ``tests/`` imports it.

The kernels -- the non-LINEAR epilogues of openvoice_amd/csrc/conv1d_mfma.h (GATE, RESSKIP, COUPLE, POSTERIOR, CONVT and
its S8 / S2 grouped forms, MAGNITUDE), its frame-rate LINEAR instances and the fused WaveNet layer of
openvoice_amd/csrc/wn_layer.hip -- read fp32 operands and sum them on the fp32 matrix pipe, an exact fmaf chain in the
MFMA's own order.  A correct kernel is therefore, on EVERY element, within

    |out - ref64| <= S32 * absacc + N                                                              (``Ref.lim``)

``ref64``  the mirror below: the same fp32 operands, the same storage points (the leaky-ReLU product of the loaders is
           an fp32 value), float64 sums.
``absacc`` the same expression on absolute values: sum |w||x| + |bias| + |batch bias| + |res| + |add|, times |scale|
           (and times the mask where the kernel multiplies by it): what fp32 summation error is proportional to.
``N``      zero for the linear epilogues (LINEAR, RESSKIP after exact inputs, COUPLE, CONVT), otherwise:
  gate       the pre-activation error S32 * absacc_pre carried through |d/dt| and |d/ds| of tanh(t) sigmoid(s) (float64),
             plus G * 2^-24 absolute for the hardware exp2 / rcp of ``wn_gate`` and for libm tanhf / expf (EPI_GATE);
  res_skip   after a gate: the gate's limit, as the error of its input, convolved with |w_rs|;
  posterior  |noise tau exp(logs)| * (S32 * absacc_logs + 4 * 2^-24): a relative error of exp equal to the absolute
             error of logs, and 4 roundings (noise * tau, expf at 1 ulp = 2, the product) of 2^-24 each;
  magnitude  the DFT errors carried through sqrt(re^2 + im^2 + eps): (|re| d_re + |im| d_im) / |out| with
             d = (S32 + 2^-24) * absacc -- the mirror is a float64 DFT with the exact window, the kernel's weights are
             its fp32 roundings (2^-24 relative each) -- plus 4 * 2^-24 |out| for the two squares, two adds and sqrtf.

No element is left out: where ``lim`` is zero (a masked column, a half the coupling must not touch, a gate whose rows are
all zeros with an exact tanh(0) = 0) the kernel has to give the reference's value exactly.

S32, the fp32 accumulation allowance -- measured, reference against reference, never from a kernel
-------------------------------------------------------------------------------------------------
``python -m oracle.fp32_ref`` prints max |v_fp32 - v_fp64| / absacc of PyTorch's CPU fp32 conv (conv_transpose1d,
matmul for the DFT) on the operand generators below (the ones both test files use), seeds 0 .. 4, every T of
``T_EDGES``, B = 3, benign and stress data:

    linear_k1   96->192    4.32e-07    linear_k5  192->192    1.02e-07    linear_k3   64->96     1.40e-07
    linear_k7  192->64     7.83e-08    gate       192->384    8.12e-08    gate_stress 192->384   8.26e-08
    res_skip   192->384    3.51e-07    couple     192->96     3.31e-07    posterior  192->384    3.75e-07
    posterior_stress       3.75e-07    convt_s8    64->32     4.69e-07    convt_s2    64->32     3.72e-07
    convt_s4    32->32     3.67e-07    magnitude   32->65x2   6.53e-07
    largest 6.531e-07 = 2^-20.55 (about 11 fp32 roundings of absacc; the 1x1 convs, conv_transpose1d and the DFT's
    matrix product, which PyTorch sums in long sequential runs, sit 4-8 times above the k = 5 / 7 convs)

The kernels sum in MFMA order, PyTorch in its own: factor 4 on the largest value (oracle/bf16_ref.py takes the same
margin for the same reason).

    S32 = 4 * 6.531e-07 = 2.612e-06 (2^-18.55)

G, the gate's absolute allowance in units of 2^-24 -- measured the same way
---------------------------------------------------------------------------
An fp32 CPU restatement of ``wn_gate`` (``gate_formula``: torch.exp2, reciprocal, every step rounded to fp32) against
float64 tanh(t) sigmoid(s) on exact fp32 (t, s) over the stress ranges of the GPU suite:

    |t|,|s| <= 30 (dense grid)   3.377    s in [-100, -30]   0.000    t = 0 or s = 0 exactly   0.909
    |t| in [1e-5, 1e-3]          0.248    libm form (tanh * sigmoid), |t|,|s| <= 30    2.271
    largest 3.377

    G = 4 * 3.377 = 13.508

The case one expects to need an allowance of its own -- 1 - a with a = e^-2|t| -> 1 at |t| ~ 1e-4, a RELATIVE error of
1 - a of about 3e-4 -- needs none: it is an absolute error of one rounding of a (2^-25) times r <= 1/2, a quarter of
2^-24 in the table above, far inside G * 2^-24.  For s << 0 the formula's e^-s = inf gives (1 - a) * rcp(inf) = 0 against
a true value below 2^-126: exact to the table's three decimals.

The MRF kernels (sample rate) -- S32_MRF and S_W, measured the same way
-----------------------------------------------------------------------
The direct OV_EPI_LINEAR ResBlock instances (conv1d_inst_a .. f.hip) and the fused pair keep the criterion above with an
allowance measured on their own operands (``mrf_operands``: C in {32, 64, 128, 256}, every (k, dilation) of 3 / 7 / 11 x
1 / 3 / 5, seeds 0 .. 4, every length of ``MRF_LS``, B = 3, benign and stress data).  The Winograd-domain kernels sum in the
transform domain -- per 4-column tile and tap group g they form At [U_g (.) (Bt d_g)], U_g = fp32(G w_g), d_g the six-sample
window of lrelu(x) -- so their error is proportional to
    absacc_w = sum over ci, g of |At| (|U_g| (.) (|Bt| |d_g|)) + |bias| + |res| + |add|,  times |scale|
(a dilated conv = ``dil`` interleaved undilated ones; per column the maximum over the four tile alignments), and their limit
is S_W * absacc_w.  S_W is measured on an fp32 restatement of the algorithm (``wino_conv``) against the float64 conv.
``python -m oracle.fp32_ref`` prints, per (C, k, d): max |conv_fp32 - conv_fp64| / absacc of PyTorch's CPU conv, max
|wino_fp32 - conv_fp64| / absacc_w of the restatement, and the median of absacc_w / absacc on the stress data:

    C=32  k=3  d=1  7.06e-07 2.50e-07 11.53   C=32  k=3  d=3  5.19e-07 2.44e-07 11.26   C=32  k=3  d=5  5.78e-07 2.21e-07 11.30
    C=32  k=7  d=1  6.44e-07 1.51e-07 11.06   C=32  k=7  d=3  5.71e-07 1.53e-07 11.25   C=32  k=7  d=5  6.26e-07 1.30e-07 10.95
    C=32  k=11 d=1  6.22e-07 1.39e-07 10.45   C=32  k=11 d=3  5.68e-07 1.64e-07 10.11   C=32  k=11 d=5  5.61e-07 1.34e-07 10.14
    C=64  k=3  d=1  4.51e-07 2.14e-07 11.47   C=64  k=3  d=3  4.38e-07 2.29e-07 11.12   C=64  k=3  d=5  4.89e-07 2.47e-07 11.01
    C=64  k=7  d=1  4.21e-07 1.23e-07 11.29   C=64  k=7  d=3  4.48e-07 1.58e-07 11.29   C=64  k=7  d=5  4.20e-07 1.60e-07 11.18
    C=64  k=11 d=1  4.11e-07 1.05e-07 10.45   C=64  k=11 d=3  4.33e-07 1.33e-07 10.37   C=64  k=11 d=5  3.98e-07 1.58e-07 10.24
    C=128 k=3  d=1  3.16e-07 2.48e-07 11.10   C=128 k=3  d=3  3.00e-07 3.03e-07 11.18   C=128 k=3  d=5  6.60e-07 2.50e-07 11.08
    C=128 k=7  d=1  3.16e-07 1.26e-07 11.41   C=128 k=7  d=3  3.69e-07 1.38e-07 11.33   C=128 k=7  d=5  2.78e-07 1.52e-07 11.23
    C=128 k=11 d=1  2.83e-07 1.04e-07 10.50   C=128 k=11 d=3  2.50e-07 1.58e-07 10.44   C=128 k=11 d=5  2.51e-07 1.52e-07 10.39
    C=256 k=3  d=1  2.70e-07 2.36e-07 11.17   C=256 k=3  d=3  2.66e-07 2.93e-07 11.26   C=256 k=3  d=5  5.20e-07 2.77e-07 11.19
    C=256 k=7  d=1  1.86e-07 1.31e-07 11.41   C=256 k=7  d=3  2.13e-07 1.35e-07 11.37   C=256 k=7  d=5  2.53e-07 1.56e-07 11.32
    C=256 k=11 d=1  1.81e-07 9.75e-08 10.51   C=256 k=11 d=3  1.98e-07 2.23e-07 10.47   C=256 k=11 d=5  1.90e-07 2.05e-07 10.46
    direct largest 7.056e-07 (above the frame-rate table's 6.531e-07, so the MRF tests get an allowance of their own)
    Winograd largest 3.030e-07;  median absacc_w / absacc over all stress shapes 11.02

    S32_MRF = 4 * 7.056e-07 = 2.822e-06          S_W = 4 * 3.030e-07 = 1.212e-06

absacc_w is about 11 times absacc: that factor is how much looser Winograd legitimately is (its transforms multiply the
operands by coefficients up to 8 and cancel them again), beside a transient as elsewhere; S_W itself is below S32_MRF.
The fused pair stores h in fp32: its limit carries S32_MRF absacc_1 + 2^-24 |h| through |w2| (``pair``).  A row whose
weights and bias are all zero has the explicit limit of ``_zero_row_lim``.
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

S32 = 4 * 6.531e-07     # 4 x the largest measured value (docstring); never widened to make a kernel pass
G = 4 * 3.377           # 4 x the largest measured value (docstring), in units of 2^-24
# the sample-rate ResBlock (MRF) kernels (docstring, "The MRF kernels"): 4 x the largest measured values, never widened to
# make a kernel pass; only tests/test_mrf_criterion_cpu.py and tests/test_gpu_mrf_kernels.py use them
S32_MRF = 4 * 7.056e-07         # direct kernels and the fused pair: per absacc; set by C = 32, k = 3, dilation 1
S_W = 4 * 3.030e-07             # Winograd-domain kernels: per absacc_w; set by C = 128, k = 3, dilation 3
S32_MRF_SET_BY, S_W_SET_BY = (32, 3, 1), (128, 3, 3)
EPS = 2.0 ** -24

F64, F32 = torch.float64, torch.float32

# ---- the shapes both test files run ---------------------------------------------------------------------------------
B = 3
T_EDGES = (1, 2, 3, 4, 5, 127, 128, 129, 257)
H = 192                 # WaveNet hidden width (ov_wn_layer_supported: 192 only); flow / posterior channels
KG = 5                  # gate conv taps
TAUS = (0.0, 0.3, 1.0)
# LINEAR instances at frame rate: (K, cin, cout)
LINEAR_SHAPES = {1: (96, 192), 5: (192, 192), 3: (64, 96), 7: (192, 64)}
# ConvTranspose: stride -> (cin, cout); 8 and 2 have grouped forms, 4 runs the generic kernel only
CONVT_SHAPES = {8: (64, 32), 2: (64, 32), 4: (32, 32)}
MAG_NFFT, MAG_HOP = 128, 32          # K = n_fft / hop = 4 framing taps, 65 bins: Cout is no multiple of 32

Ref = collections.namedtuple("Ref", "ref absacc lim")


def f32(v):
    """The fp32 value of a Python float, as a Python float (what a kernel receives through a ``float`` field)."""
    return float(np.float32(v))


def lengths(T):
    """The ragged lengths every masked case uses: T, 1 and about T / 2."""
    return [T, 1, max(1, T // 2)]


def seq_mask(T):
    return (torch.arange(T)[None, :] < torch.tensor(lengths(T))[:, None]).float()


def rand(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ratio(got, r):
    """Element-wise err / lim against ``Ref`` r: inf where lim is zero and the value is not exact, or where ``got`` is
    not finite although the reference is."""
    ref = r.ref.to(F64)
    err = (got.detach().cpu().to(F64) - ref).abs()
    q = torch.where(r.lim > 0, err / r.lim.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
    return torch.where(torch.isfinite(ref), q, torch.zeros_like(q))


def worst(got, r):
    return ratio(got, r).max().item()


# ---- building blocks ------------------------------------------------------------------------------------------------
def _lrelu(x, slope):
    """The loaders' leaky ReLU: v > 0 ? v : v * slope in fp32 -- the product is an fp32 value whatever the mirror's dtype."""
    if slope == 1.0:
        return x
    return torch.where(x > 0, x, (x.float() * f32(slope)).to(x.dtype))


def _conv(x, w, dil=1):
    k = w.shape[-1]
    return F.conv1d(x, w, None, dilation=dil, padding=(k - 1) * dil // 2)


def _affine(x, w, bias=None, bias_b=None, dil=1, in_slope=1.0, dtype=F64):
    """conv(lrelu(x)) + bias + per-utterance bias and the same on absolute values: (v, absacc), both ``dtype`` / float64."""
    xin = _lrelu(x.float(), in_slope)
    v = _conv(xin.to(dtype), w.to(dtype), dil)
    a = _conv(xin.to(F64).abs(), w.to(F64).abs(), dil)
    if bias is not None:
        v, a = v + bias.to(dtype)[None, :, None], a + bias.to(F64).abs()[None, :, None]
    if bias_b is not None:
        v, a = v + bias_b.to(dtype)[:, :, None], a + bias_b.to(F64).abs()[:, :, None]
    return v, a


def _lin_ref(v, a):
    return Ref(v, a, S32 * a)


# ---- mirrors ----------------------------------------------------------------------------------------------------------
def linear(x, w, bias=None, in_slope=1.0, bias_b=None, res=None, add=None, scale=1.0, mask=None, dil=1, dtype=F64):
    """OV_EPI_LINEAR: ((conv + bias + bias_b) [* mask, OV_F_MASK_V] + res + add) * scale."""
    v, a = _affine(x, w, bias, bias_b, dil, in_slope, dtype)
    if mask is not None:
        v, a = v * mask.to(dtype)[:, None], a * mask.to(F64)[:, None]
    for t in (res, add):
        if t is not None:
            v, a = v + t.to(dtype), a + t.to(F64).abs()
    return _lin_ref(v * f32(scale), a * abs(f32(scale)))


def gate_formula(t, s):
    """``wn_gate`` of wn_layer.hip restated in the dtype of ``t`` (fp32: every step rounded like the kernel's):
    sign(t) (1 - a) / ((1 + a)(1 + e^-s)), a = e^-2|t| through exp2."""
    a = torch.exp2(t.abs() * t.new_tensor(-2.8853900817779268))
    e = torch.exp2(s * s.new_tensor(-1.4426950408889634))
    r = torch.reciprocal((1 + a) * (1 + e))
    return torch.copysign((1 - a) * r, t)


def gate_exact(t, s):
    return torch.tanh(t.to(F64)) * torch.sigmoid(s.to(F64))


def gate_limit(t, s, at, as_):
    """N of the gate + its linear part: S32 * absacc of each pre-activation through the float64 partial derivatives of
    tanh(t) sigmoid(s), plus G * 2^-24."""
    th, sg = torch.tanh(t), torch.sigmoid(s)
    return (1 - th * th) * sg * (S32 * at) + th.abs() * sg * (1 - sg) * (S32 * as_) + G * EPS


def gate(x, w_in, b_in, g=None, dtype=F64, formula="libm"):
    """OV_EPI_GATE / phase 1 of the fused layer: tanh(pre[:H]) * sigmoid(pre[H:]), pre = conv_k(x) + b_in + g[b].
    ``formula`` matters for the fp32 stand-in only: "libm" = tanh * sigmoid, "hw" = ``gate_formula``."""
    v, a = _affine(x, w_in, b_in, g, dtype=dtype)
    h = v.shape[1] // 2
    t, s = v[:, :h], v[:, h:]
    if dtype == F64:
        ref = gate_exact(t, s)
    else:
        ref = gate_formula(t, s) if formula == "hw" else torch.tanh(t) * torch.sigmoid(s)
    v64 = v if dtype == F64 else _affine(x, w_in, b_in, g)[0]
    return Ref(ref, a, gate_limit(v64[:, :h], v64[:, h:], a[:, :h], a[:, h:]))


def res_skip(acts, w_rs, b_rs, h, skip, mask, split, first=False, acts_err=None, dtype=F64):
    """OV_EPI_RESSKIP / phase 2 of the fused layer: rows < split: (h + rs) * mask; rows >= split: skip (+)= rs
    ('=' when ``first``: OV_F_OUT2_INIT).  ``split = 0`` is the last layer (all rows skip, h untouched -> None).
    ``acts_err`` [B, H, T]: the element-wise error of ``acts`` (a gate's limit).  Returns (Ref h', Ref skip')."""
    v, a = _affine(acts, w_rs, b_rs, dtype=dtype)
    n = torch.zeros_like(a)
    if acts_err is not None:
        n = _conv(acts_err.to(F64), w_rs.to(F64).abs())
    out_h = None
    if split > 0:
        m, m64 = mask.to(dtype)[:, None], mask.to(F64)[:, None]
        ah = (a[:, :split] + h.to(F64).abs()) * m64
        out_h = Ref((h.to(dtype) + v[:, :split]) * m, ah, S32 * ah + n[:, :split] * m64)
    vs, as_ = v[:, split:], a[:, split:]
    if not first:
        vs, as_ = vs + skip.to(dtype), as_ + skip.to(F64).abs()
    return out_h, Ref(vs, as_, S32 * as_ + n[:, split:])


def couple(h, w, b, x, mask, reverse=False, flipped=False, dtype=F64):
    """OV_EPI_COUPLE, in place on the PHYSICAL [B, C, T] tensor ``x``: the logical tensor is its channel reverse when
    ``flipped``; x1 = logical[:, C/2:] becomes (m + x1) * mask (forward) / (x1 - m) * mask (reverse), m = conv1x1(h);
    the other half must come back bit for bit (lim = 0).  ``w`` / ``b`` are in logical row order."""
    half = x.shape[1] // 2
    m, a = _affine(h, w, b, dtype=dtype)
    logical = torch.flip(x, [1]) if flipped else x
    x1 = logical[:, half:]
    mk, mk64 = mask.to(dtype)[:, None], mask.to(F64)[:, None]
    x1n = (x1.to(dtype) - m) * mk if reverse else (m + x1.to(dtype)) * mk
    a1 = (a + x1.to(F64).abs()) * mk64
    new = torch.cat([logical[:, :half].to(dtype), x1n], 1)
    acc = torch.cat([torch.zeros_like(a1), a1], 1)
    if flipped:
        new, acc = torch.flip(new, [1]), torch.flip(acc, [1])
    return _lin_ref(new, acc)


def posterior(h, w, b, noise, tau, mask, dtype=F64):
    """OV_EPI_POSTERIOR: (m * mask + noise * tau * exp(logs * mask)) * mask; rows [:C] of the 1x1 conv are m, [C:] logs."""
    v, a = _affine(h, w, b, dtype=dtype)
    c = v.shape[1] // 2
    mk, mk64 = mask.to(dtype)[:, None], mask.to(F64)[:, None]
    m, logs = v[:, :c] * mk, v[:, c:] * mk
    p = noise.to(dtype) * f32(tau) * torch.exp(logs)
    a_m = a[:, :c] * mk64
    lim = (S32 * a_m + p.to(F64).abs() * (S32 * a[:, c:] * mk64 + 4 * EPS)) * mk64
    return Ref((m + p) * mk, a_m, lim)


def conv_transpose(x, w, b, s, in_slope=1.0, dtype=F64):
    """OV_EPI_CONVT (generic and grouped): lrelu + ConvTranspose1d(k = 2s, stride s, padding s/2) from
    ``F.conv_transpose1d`` itself, not from the phase conv the kernel runs.  ``w`` is [Cin, Cout, 2s]."""
    xin = _lrelu(x.float(), in_slope)
    k = w.shape[-1]
    v = F.conv_transpose1d(xin.to(dtype), w.to(dtype), b.to(dtype), stride=s, padding=(k - s) // 2)
    a = F.conv_transpose1d(xin.to(F64).abs(), w.to(F64).abs(), b.to(F64).abs(), stride=s, padding=(k - s) // 2)
    return _lin_ref(v, a)


def _dft_parts(n_fft):
    n = torch.arange(n_fft, dtype=F64)
    window = 0.5 - 0.5 * torch.cos(2 * math.pi * n / n_fft)                  # periodic Hann
    ang = 2 * math.pi * torch.arange(n_fft // 2 + 1, dtype=F64)[:, None] * n[None, :] / n_fft
    return window, window * torch.cos(ang), -window * torch.sin(ang)


def _frames(hops, n_fft, hop):
    Bn, _, U = hops.shape
    return hops.transpose(1, 2).reshape(Bn, U * hop).unfold(1, n_fft, hop)


def magnitude(hops, n_fft, hop, eps, dtype=F64):
    """OV_EPI_MAGNITUDE on the hop matrix [B, hop, U] (sample hop * u + c at [c][u]): sqrt(|DFT(window * frame)|^2 + eps),
    frames hop apart, T = U - n_fft / hop + 1 of them.  float64: ``torch.fft.rfft`` of the framed signal; the fp32
    stand-in multiplies by the fp32-rounded DFT matrix as the kernel does."""
    frames = _frames(hops, n_fft, hop)                                      # [B, T, n_fft]
    window, cw, sw = _dft_parts(n_fft)
    if dtype == F64:
        spec = torch.fft.rfft(frames.to(F64) * window, dim=-1)
        re, im = spec.real, spec.imag
    else:
        re, im = frames.to(dtype) @ cw.to(dtype).t(), frames.to(dtype) @ sw.to(dtype).t()
    fa = frames.to(F64).abs()
    a_re, a_im = fa @ cw.abs().t(), fa @ sw.abs().t()
    e = torch.tensor(f32(eps), dtype=dtype)
    ref = torch.sqrt(re * re + im * im + e)
    r64, i64 = re.to(F64).abs(), im.to(F64).abs()
    out = ref.to(F64)
    lim = (r64 * a_re + i64 * a_im) * (S32 + EPS) / out + 4 * EPS * out
    return Ref(ref.transpose(1, 2), (a_re + a_im).transpose(1, 2), lim.transpose(1, 2)), \
        (re.transpose(1, 2), im.transpose(1, 2), a_re.transpose(1, 2), a_im.transpose(1, 2))


def wn_layer(x, g, mask, skip, w_in, b_in, w_rs, b_rs, first=False, last=False, dtype=F64, formula="hw"):
    """The fused layer (and the EPI_GATE + EPI_RESSKIP pair): gate, then res/skip with the gate's limit as the error of
    its input.  ``w_rs`` has H rows when ``last``.  Returns (Ref acts, Ref h' or None, Ref skip')."""
    acts = gate(x, w_in, b_in, g, dtype=dtype, formula=formula)
    hn = x.shape[1]
    out_h, out_s = res_skip(acts.ref.to(F32) if dtype != F64 else acts.ref, w_rs, b_rs, x, skip, mask,
                            0 if last else hn, first, acts_err=acts.lim, dtype=dtype)
    return acts, out_h, out_s


# ---- operand generators (seeded; the tests and the S32 table use these and nothing else) ------------------------------
def linear_operands(K, T, seed=0):
    cin, cout = LINEAR_SHAPES[K]
    s = 100 * seed
    return dict(x=rand(B, cin, T, seed=s + 1), w=rand(cout, cin, K, seed=s + 2, scale=(cin * K) ** -0.5),
                bias=rand(cout, seed=s + 3, scale=0.1), bias_b=rand(B, cout, seed=s + 4, scale=0.3),
                res=rand(B, cout, T, seed=s + 5), add=rand(B, cout, T, seed=s + 6), mask=seq_mask(T))


def wn_operands(T, seed=0, stress=False, last=False):
    """One WaveNet layer.  ``stress``: per channel c (tanh row c, sigmoid row H + c), by c % 8:
    0 both rows x 10 (|t|, |s| to about 30); 1 sigmoid bias -100 (e^-s overflows); 2 tanh row all zeros (t = 0 exactly);
    3 tanh row x 1e-4 without bias (|t| ~ 1e-4); 4 both rows zero; 5 sigmoid row zero (s = 0); 6 tanh x 10 and sigmoid
    bias -88 (e^-s next to FLT_MAX); 7 as trained."""
    s = 100 * seed + 1000
    x, skip = rand(B, H, T, seed=s + 1), rand(B, H, T, seed=s + 2)
    mask = seq_mask(T)
    x = x * mask[:, None]                  # the WaveNet input is always masked (reference modules.py:207)
    g = rand(B, 2 * H, seed=s + 3, scale=0.3)
    w_in, b_in = rand(2 * H, H, KG, seed=s + 4, scale=(KG * H) ** -0.5), rand(2 * H, seed=s + 5, scale=0.1)
    rows = H if last else 2 * H
    w_rs, b_rs = rand(rows, H, 1, seed=s + 6, scale=H ** -0.5), rand(rows, seed=s + 7, scale=0.1)
    if stress:
        c = torch.arange(H)
        sel = lambda k: c[c % 8 == k]
        for r in (sel(0), sel(0) + H, sel(6)):
            w_in[r] *= 10.0
        for r in (sel(2), sel(4), sel(4) + H, sel(5) + H):
            w_in[r], b_in[r], g[:, r] = 0.0, 0.0, 0.0
        w_in[sel(3)] *= 1e-4
        b_in[sel(3)], g[:, sel(3)] = 0.0, 0.0
        b_in[sel(1) + H] = -100.0
        b_in[sel(6) + H] = -88.0
    return dict(x=x, g=g, mask=mask, skip=skip, w_in=w_in, b_in=b_in, w_rs=w_rs, b_rs=b_rs)


def couple_operands(T, seed=0):
    s = 100 * seed + 2000
    return dict(h=rand(B, H, T, seed=s + 1), x=rand(B, H, T, seed=s + 2), mask=seq_mask(T),
                w=rand(H // 2, H, 1, seed=s + 3, scale=H ** -0.5), b=rand(H // 2, seed=s + 4, scale=0.1))


def posterior_operands(T, seed=0, stress=False):
    """``stress``: logs rows with weights x 0.01 and a bias spread evenly over [-20, 20]."""
    s = 100 * seed + 3000
    w, b = rand(2 * H, H, 1, seed=s + 3, scale=H ** -0.5), rand(2 * H, seed=s + 4, scale=0.1)
    if stress:
        w[H:] *= 0.01
        b[H:] = torch.linspace(-20.0, 20.0, H)
    return dict(h=rand(B, H, T, seed=s + 1), noise=rand(B, H, T, seed=s + 2), mask=seq_mask(T), w=w, b=b)


def convt_operands(stride, T, seed=0):
    cin, cout = CONVT_SHAPES[stride]
    s = 100 * seed + 4000 + stride
    return dict(x=rand(B, cin, T, seed=s + 1), w=rand(cin, cout, 2 * stride, seed=s + 2, scale=(2 * cin) ** -0.5),
                b=rand(cout, seed=s + 3, scale=0.1))


def magnitude_operands(T, seed=0):
    """The hop matrix of a sinusoid + noise per utterance, U = T + 3 columns."""
    U = T + MAG_NFFT // MAG_HOP - 1
    n = torch.arange(U * MAG_HOP, dtype=torch.float32)
    y = 0.6 * torch.sin(2 * math.pi * (0.03 + 0.05 * torch.arange(B)[:, None]) * n) \
        + rand(B, U * MAG_HOP, seed=100 * seed + 5000, scale=0.05)
    return dict(hops=y.reshape(B, U, MAG_HOP).transpose(1, 2).contiguous())


# ---- the measurements behind S32 and G --------------------------------------------------------------------------------
def _pre_pairs(T, seed):
    """name -> list of (v_fp32, v_fp64, absacc) of every linear part the suite computes at (T, seed)."""
    out = {}

    def both(fn):
        v32, _ = fn(F32)
        v64, a = fn(F64)
        return v32, v64, a

    for K, (cin, cout) in LINEAR_SHAPES.items():
        o = linear_operands(K, T, seed)
        out[f"linear_k{K} {cin}->{cout}"] = [both(lambda dt: _affine(o["x"], o["w"], o["bias"], o["bias_b"], in_slope=0.1, dtype=dt))]
    for stress in (False, True):
        o = wn_operands(T, seed, stress)
        out["gate_stress 192->384" if stress else "gate 192->384"] = [
            both(lambda dt: _affine(o["x"], o["w_in"], o["b_in"], o["g"], dtype=dt))]
        if not stress:
            acts = gate(o["x"], o["w_in"], o["b_in"], o["g"], dtype=F32).ref
            out["res_skip 192->384"] = [both(lambda dt: _affine(acts, o["w_rs"], o["b_rs"], dtype=dt))]
        p = posterior_operands(T, seed, stress)
        out["posterior_stress" if stress else "posterior 192->384"] = [both(lambda dt: _affine(p["h"], p["w"], p["b"], dtype=dt))]
    c = couple_operands(T, seed)
    out["couple 192->96"] = [both(lambda dt: _affine(c["h"], c["w"], c["b"], dtype=dt))]
    for s, (cin, cout) in CONVT_SHAPES.items():
        o = convt_operands(s, T, seed)
        out[f"convt_s{s} {cin}->{cout}"] = [both(lambda dt: conv_transpose(o["x"], o["w"], o["b"], s, 0.1, dtype=dt)[:2])]
    # the DFT as the matrix product the kernel runs, in both precisions (not against rfft: where a weight is a rounding
    # residue of sin(pi n), rfft's exact zero would make the quotient meaningless)
    frames = _frames(magnitude_operands(T, seed)["hops"], MAG_NFFT, MAG_HOP)
    _, cw, sw = _dft_parts(MAG_NFFT)
    out["magnitude 32->65x2"] = [(frames @ m.float().t(), frames.to(F64) @ m.float().to(F64).t(), frames.to(F64).abs() @ m.abs().t())
                                 for m in (cw, sw)]
    return out


def measure_s32(seeds=range(5), ts=T_EDGES):
    table = collections.OrderedDict()
    for seed in seeds:
        for T in ts:
            for name, pairs in _pre_pairs(T, seed).items():
                for v32, v64, a in pairs:
                    ok = a > 0
                    q = ((v32.to(F64) - v64).abs()[ok] / a[ok]).max().item() if ok.any() else 0.0
                    table[name] = max(table.get(name, 0.0), q)
    return table


def gate_stress_grids():
    """name -> (t, s) fp32 grids covering what ``wn_operands(stress=True)`` produces."""
    lin = torch.linspace(-30.0, 30.0, 1201)
    tiny = torch.cat([-torch.logspace(-5, -3, 200), torch.logspace(-5, -3, 200)])
    zero = torch.zeros(1)
    grid = lambda a, b: tuple(m.reshape(-1) for m in torch.meshgrid(a, b, indexing="ij"))
    return collections.OrderedDict([
        ("|t|,|s| <= 30 (dense grid)", grid(lin, lin)),
        ("s in [-100, -30]", grid(lin, torch.linspace(-100.0, -30.0, 701))),
        ("t = 0 or s = 0 exactly", tuple(torch.cat(p) for p in zip(grid(zero, lin), grid(lin, zero)))),
        ("|t| in [1e-5, 1e-3]", grid(tiny, lin)),
    ])


def measure_g():
    table = collections.OrderedDict()
    for name, (t, s) in gate_stress_grids().items():
        table[name] = ((gate_formula(t, s).to(F64) - gate_exact(t, s)).abs().max() / EPS).item()
    t, s = gate_stress_grids()["|t|,|s| <= 30 (dense grid)"]
    table["libm form, |t|,|s| <= 30"] = (((torch.tanh(t) * torch.sigmoid(s)).to(F64) - gate_exact(t, s)).abs().max()
                                         / EPS).item()
    return table


# =====================================================================================================================
# The sample-rate ResBlock (MRF) kernels: the direct OV_EPI_LINEAR instances of conv1d_inst_a .. f.hip, the fused pair
# (ov_resblock_pair_f32), the Winograd-domain conv (ov_conv1d_wino_f32) and its multi launch.  The docstring quotes
# the measurements; tests/test_mrf_criterion_cpu.py and tests/test_gpu_mrf_kernels.py use these mirrors and generators.
# =====================================================================================================================
MRF_CS = (32, 64, 128, 256)
MRF_KD = tuple((k, d) for k in (3, 7, 11) for d in (1, 3, 5))
# every length the GPU file runs: {4, N - 4, N, N + 4, 2 N + 4} of the direct tiles N = 128 / 256 / 512, the pair's list
# and the Winograd kernels' list (multiples of 4: the pair and the Winograd kernels take nothing else)
PAIR_LS = (4, 124, 128, 132, 256, 260, 516)
WINO_LS = (4, 252, 256, 260, 516)
MRF_LS = (4, 124, 128, 132, 252, 256, 260, 508, 512, 516, 1028)
# F(4, 3), points 0, 1, -1, 2, -2, infinity: the matrices of openvoice_amd/wino.py (restated so that the oracle loads
# without the native library; tests/test_mrf_criterion_cpu.py holds the two copies equal)
WINO_BT = ((4, 0, -5, 0, 1, 0), (0, -4, -4, 1, 1, 0), (0, 4, -4, -1, 1, 0), (0, -2, -1, 2, 1, 0), (0, 2, -1, -2, 1, 0),
           (0, 4, 0, -5, 0, 1))
WINO_G = ((1 / 4, 0, 0), (-1 / 6, -1 / 6, -1 / 6), (-1 / 6, 1 / 6, -1 / 6), (1 / 24, 1 / 12, 1 / 6), (1 / 24, -1 / 12, 1 / 6),
          (0, 0, 1))
WINO_AT = ((1, 1, 1, 1, 1, 0), (0, 1, -1, 2, -2, 0), (0, 1, 1, 4, 4, 0), (0, 1, -1, 8, -8, 1))
WINO_LEAD_TAPS = {3: 0, 7: 1, 11: 0}


def mrf_operands(C, K, dil, L, seed=0, stress=False):
    """One ResBlock conv (and the pair's second, dilation-1 conv): x [B = 3, C, L], w [C, C, K] at scale (C K)^-1/2, bias,
    res, add, w2, b2.  ``dil`` does not change the operands (it belongs to the conv); it separates the seeds.
    ``stress``: input channel c by c % 8 (x, and res / add rows alike so that a quiet row stays quiet end to end):
    0 x 1e3; 1 x 1e-3; 2 exactly zero; 3 all negative (only the leaky branch runs); 4 a 1e-3 row with one loud transient
    (+1e3 at column L // 2, -1e3 at column L - 1); 5 .. 7 as trained.  Output row o by o % 4: weights (of w and w2) x 1,
    x 1e-2, x 1e2 and exactly zero with a zero bias -- such a row must come back as exactly res + add (``_zero_row_lim``)."""
    s = 100 * seed + 7000 + 10 * K + dil
    sc = (C * K) ** -0.5
    o = dict(x=rand(B, C, L, seed=s + 1), w=rand(C, C, K, seed=s + 2, scale=sc), bias=rand(C, seed=s + 3, scale=0.1),
             res=rand(B, C, L, seed=s + 4), add=rand(B, C, L, seed=s + 5), w2=rand(C, C, K, seed=s + 6, scale=sc),
             b2=rand(C, seed=s + 7, scale=0.1))
    if stress:
        c = torch.arange(C)
        for name in ("x", "res", "add"):
            t = o[name]
            t[:, c % 8 == 0] *= 1e3
            t[:, c % 8 == 1] *= 1e-3
            t[:, c % 8 == 2] = 0.0
            t[:, c % 8 == 4] *= 1e-3
        o["x"][:, c % 8 == 3] = -o["x"][:, c % 8 == 3].abs()
        o["x"][:, c % 8 == 4, L // 2] = 1e3
        o["x"][:, c % 8 == 4, L - 1] = -1e3
        for wn, bn in (("w", "bias"), ("w2", "b2")):
            o[wn][c % 4 == 1] *= 1e-2
            o[wn][c % 4 == 2] *= 1e2
            o[wn][c % 4 == 3] = 0.0
            o[bn][c % 4 == 3] = 0.0
    return o


def _lrelu64(v, slope):
    """Leaky ReLU of a float64 mirror value (an fp32 slope, the product not rounded)."""
    return v if slope == 1.0 else torch.where(v > 0, v, v * f32(slope))


def _zero_row_lim(lim, w, bias, terms, scale):
    """Rows whose weights and bias are all exactly zero: the kernel's sum is (res + add) * scale and nothing else, so
    the limit is stated explicitly instead of S * absacc: one rounding of res + add and one of the product with scale,
    2 * 2^-24 (1 + 2^-24) (|res| + |add|) |scale| -- zero without res and add: the output is exactly zero."""
    zero = (w.reshape(w.shape[0], -1) == 0).all(1) & (bias == 0)
    if not zero.any():
        return lim
    a = sum(t.to(F64).abs() for t in terms if t is not None)
    lz = a * (2 * EPS * (1 + EPS) * abs(f32(scale))) if torch.is_tensor(a) else torch.zeros_like(lim)
    return torch.where(zero[None, :, None], lz, lim)


def mrf_linear(x, w, bias, dil=1, in_slope=0.1, res=None, add=None, scale=1.0, dtype=F64, S=None, core=None):
    """A direct OV_EPI_LINEAR ResBlock instance: ``linear`` without mask and batch bias (ov_conv1d_params has no
    out_slope: nothing to add) with the MRF allowance ``S`` (default S32_MRF) and the explicit limit of all-zero rows.
    ``core`` = ``_affine``'s (conv + bias, absacc) computed before, for callers that run several operand forms."""
    S = S32_MRF if S is None else S
    v, a = _affine(x, w, bias, dil=dil, in_slope=in_slope, dtype=dtype) if core is None else core
    for t in (res, add):
        if t is not None:
            v, a = v + t.to(dtype), a + t.to(F64).abs()
    a = a * abs(f32(scale))
    return Ref(v * f32(scale), a, _zero_row_lim(S * a, w, bias, (res, add), scale))


def pair(x, w1, b1, w2, b2, K, dil, add=None, scale=1.0, slope=0.1, dtype=F64, S=None):
    """ov_resblock_pair_f32: out = (c2(lrelu(h)) + b2 + x [+ add]) * scale, h = c1_dil(lrelu(x)) + b1.
    h is an fp32 STORAGE POINT of the kernel (it stays in LDS): it lies within lim_h = S absacc_1 + 2^-24 |h64| of the
    float64 h64, its leaky ReLU (1-Lipschitz, one more fp32 product) within lim_h + 2^-24 |lrelu(h64)|, and that error
    reaches the output through |w2|:  lim = (S absacc_2 + conv(|w2|, lim_h + 2^-24 |lrelu h64|)) |scale|.
    h outside [0, L) is ZERO -- the second conv zero-pads h itself (reference modules.py:298-301); it is NOT the first conv
    evaluated on zero-padded x (which would be b1 + the taps that still reach x): ``F.conv1d``'s own padding of h below.
    ``dtype`` = float32: fp32 conv -> fp32 h -> fp32 conv, the honest stand-in."""
    S = S32_MRF if S is None else S
    assert w1.shape[-1] == K and w2.shape[-1] == K
    h, a1 = _affine(x, w1, b1, dil=dil, in_slope=slope, dtype=dtype)
    h64 = h if dtype == F64 else _affine(x, w1, b1, dil=dil, in_slope=slope)[0]
    act64 = _lrelu64(h64, slope)
    lim_act = S * a1 + EPS * h64.abs() + EPS * act64.abs()
    act = act64 if dtype == F64 else _lrelu(h, slope)
    v = _conv(act.to(dtype), w2.to(dtype)) + b2.to(dtype)[None, :, None] + x.to(dtype)
    a2 = _conv(act64.abs(), w2.to(F64).abs()) + b2.to(F64).abs()[None, :, None] + x.to(F64).abs()
    if add is not None:
        v, a2 = v + add.to(dtype), a2 + add.to(F64).abs()
    sc = abs(f32(scale))
    lim = (S * a2 + _conv(lim_act, w2.to(F64).abs())) * sc
    return Ref(v * f32(scale), a2 * sc, _zero_row_lim(lim, w2, b2, (x, add), scale))


# ---- the Winograd-domain conv ------------------------------------------------------------------------------------------
def wino_u(w, K):
    """U[o][c][g][p] = fp32(sum_k G[p][k] w'[o][c][3 g + k]) of the zero-extended filter w' (``WINO_LEAD_TAPS`` zero taps in
    front, zeros behind up to 3 G taps), summed in float64 and rounded once: the packer's values."""
    O, C, _ = w.shape
    Gn = (K + 2) // 3
    wp = torch.zeros(O, C, 3 * Gn, dtype=F64)
    wp[:, :, WINO_LEAD_TAPS[K]:WINO_LEAD_TAPS[K] + K] = w.to(F64)
    return torch.einsum("pk,ocgk->ocgp", torch.tensor(WINO_G, dtype=F64), wp.view(O, C, Gn, 3)).float()


def _wino_phase(s, u, K, bias, a, dtype, absolute):
    """One dilation-1 problem s [B, C, M] (already activated) with tiles of 4 outputs starting at 4 n - a: At [sum over ci,
    then g, of U (.) (Bt d)] per tile -- on absolute values when ``absolute`` -- -> [B, O, M].  ``bias`` starts the point-1
    accumulator, as in the kernel (column 1 of At is all ones)."""
    Bn, C, M = s.shape
    Gn = (K + 2) // 3
    pad, nv = (K - 1) // 2 + WINO_LEAD_TAPS[K], 3 * (Gn - 1) + 6
    nt = (M + a + 3) // 4
    bt, at = torch.tensor(WINO_BT, dtype=dtype), torch.tensor(WINO_AT, dtype=dtype)
    s, u = s.to(dtype), u.to(dtype)
    if absolute:
        bt, at, s, u = bt.abs(), at.abs(), s.abs(), u.abs()
    win = F.pad(s, (pad + a, 4 * (nt - 1) + nv - (pad + a) - M)).unfold(-1, nv, 4)           # [B, C, nt, nv]
    d = torch.stack([win[..., 3 * g:3 * g + 6] for g in range(Gn)], 3)                          # [B, C, nt, G, 6]
    v = torch.einsum("pj,bcngj->bcngp", bt, d)
    y = torch.einsum("ocgp,bcngp->gbonp", u, v)                                               # summed over ci ...
    acc = y[0]
    for g in range(1, Gn):                                                                      # ... then over g
        acc = acc + y[g]
    if bias is not None:
        acc = acc.clone()
        acc[..., 1] += (bias.abs() if absolute else bias).to(dtype)[None, :, None]
    out = torch.einsum("ip,bonp->boni", at, acc).reshape(Bn, u.shape[0], 4 * nt)
    return out[..., a:a + M]


def wino_conv(x, w, bias, K, dil=1, in_slope=1.0, dtype=F32, absolute=False, aligns=(0,), u=None):
    """conv(lrelu(x)) + bias computed the Winograd way: a dilated conv is ``dil`` interleaved undilated ones, each on the
    subsequence of one residue class of columns.  ``dtype`` = float32 is the RESTATEMENT of the kernel's algorithm (fp32 input
    transform, fp32 U, fp32 products summed over ci then g, fp32 output transform) -- the honest stand-in and the reference of
    S_W; ``absolute`` the same on absolute values in float64, per column the maximum over the tile alignments ``aligns``."""
    xin = _lrelu(x.float(), in_slope)
    u = wino_u(w, K) if u is None else u               # (``u``: a caller's own transformed weights, for wrong variants)
    out = None
    for a in aligns:
        o = torch.empty(x.shape[0], w.shape[0], x.shape[2], dtype=dtype)
        for ph in range(dil):
            if ph < x.shape[2]:
                o[..., ph::dil] = _wino_phase(xin[..., ph::dil], u, K, bias, a, dtype, absolute)
        out = o if out is None else torch.maximum(out, o)
    return out


def wino_absacc(x, w, bias, K, dil=1, in_slope=1.0):
    """absacc_w before res / add / scale: where the kernel really sums.  Per output tile of 4 columns and tap group g it forms
    At [U_g (.) (Bt d_g)], so the sum its roundings are proportional to is
        sum over ci, g of |At| (|U_g| (.) (|Bt| |d_g|)) + |bias|
    The value depends on where the tiles start; per column the maximum over the four alignments is taken, which copies no
    tiling decision of the kernel into the oracle."""
    return wino_conv(x, w, bias, K, dil, in_slope, dtype=F64, absolute=True, aligns=(0, 1, 2, 3))


def wino_linear(x, w, bias, K, dil=1, in_slope=0.1, out_slope=1.0, res=None, add=None, scale=1.0, dtype=F64, S=None,
                core=None):
    """ov_conv1d_wino_f32 / ov_conv1d_wino_multi_f32: lrelu_out(((conv_dil(lrelu(x)) + bias) + res + add) * scale).  The
    float64 ``ref`` is ``linear``'s; ``absacc`` = (``wino_absacc`` + |res| + |add|) |scale|; lim = S_W absacc, plus
    2^-24 |ref| for the fp32 product of the output activation (``out_slope`` < 1, 1-Lipschitz otherwise).  ``dtype`` =
    float32: the restatement ``wino_conv``.  ``core`` = (float64 conv + bias, wino_absacc) computed before, for callers
    that run several operand forms on the same x and w."""
    S = S_W if S is None else S
    if core is None:
        core = (_affine(x, w, bias, dil=dil, in_slope=in_slope)[0], wino_absacc(x, w, bias, K, dil, in_slope))
    v, a = core
    if dtype != F64:
        v = wino_conv(x, w, bias, K, dil, in_slope, dtype=dtype)
    for t in (res, add):
        if t is not None:
            v, a = v + t.to(dtype), a + t.to(F64).abs()
    v, a = v * f32(scale), a * abs(f32(scale))
    lim = _zero_row_lim(S * a, w, bias, (res, add), scale)
    if out_slope != 1.0:
        v = _lrelu64(v, out_slope) if dtype == F64 else _lrelu(v, out_slope)
        lim = lim + EPS * (core[0] * f32(scale)).abs()
    return Ref(v, a, lim)


# ---- the measurements behind S32_MRF and S_W ---------------------------------------------------------------------------
def measure_mrf(cs=MRF_CS, kds=MRF_KD, seeds=range(5), ls=MRF_LS, datas=(False, True)):
    """(C, K, dil) -> [max |conv_fp32 - conv_fp64| / absacc of PyTorch's CPU fp32 conv,
                       max |wino_fp32 - conv_fp64| / absacc_w of the fp32 restatement,
                       median absacc_w / absacc on the stress data]."""
    table = collections.OrderedDict()
    for C in cs:
        for K, dil in kds:
            row = table.setdefault((C, K, dil), [0.0, 0.0, []])
            for seed in seeds:
                for L in ls:
                    for stress in datas:
                        o = mrf_operands(C, K, dil, L, seed, stress)
                        v64, a = _affine(o["x"], o["w"], o["bias"], dil=dil, in_slope=0.1)
                        v32 = _affine(o["x"], o["w"], o["bias"], dil=dil, in_slope=0.1, dtype=F32)[0]
                        aw = wino_absacc(o["x"], o["w"], o["bias"], K, dil, 0.1)
                        w32 = wino_conv(o["x"], o["w"], o["bias"], K, dil, 0.1)
                        ok = a > 0
                        if ok.any():
                            row[0] = max(row[0], ((v32.to(F64) - v64).abs()[ok] / a[ok]).max().item())
                            row[1] = max(row[1], ((w32.to(F64) - v64).abs()[ok] / aw[ok]).max().item())
                            if stress:
                                row[2].append((aw[ok] / a[ok]).median().item())
    return table


def main():
    torch.set_num_threads(max(1, min(4, torch.get_num_threads())))
    _main_frame()
    mrf = measure_mrf()
    print("MRF: max |v_fp32 - v_fp64| / absacc (direct, PyTorch fp32 conv) and / absacc_w (fp32 Winograd restatement),")
    print("     median absacc_w / absacc on stress data; seeds 0..4, L in", MRF_LS, ", benign and stress")
    for (C, K, dil), (d, w, m) in mrf.items():
        print(f"    C={C:<3d} k={K:<2d} d={dil}   direct {d:.2e}   wino {w:.2e}   absacc_w/absacc {float(np.median(m)):.2f}")
    dtop, wtop = max(v[0] for v in mrf.values()), max(v[1] for v in mrf.values())
    print(f"    direct largest {dtop:.3e};  4 x largest = {4 * dtop:.3e};  module S32_MRF = {S32_MRF:.3e} (S32 = {S32:.3e})")
    print(f"    wino   largest {wtop:.3e};  4 x largest = {4 * wtop:.3e};  module S_W = {S_W:.3e}")
    print(f"    median absacc_w / absacc over all stress shapes {float(np.median([x for v in mrf.values() for x in v[2]])):.2f}")


def _main_frame():
    s32 = measure_s32()
    print("S32: max |v_fp32 - v_fp64| / absacc, seeds 0..4, T in", T_EDGES)
    for name, v in s32.items():
        print(f"    {name:<24s} {v:.2e}")
    top = max(s32.values())
    print(f"    largest {top:.3e} = 2^{math.log2(top):.2f};  4 x largest = {4 * top:.3e};  module S32 = {S32:.3e}")
    g = measure_g()
    print("G: max |gate_formula_fp32 - gate_fp64| / 2^-24")
    for name, v in g.items():
        print(f"    {name:<30s} {v:.3f}")
    gtop = max(g.values())
    print(f"    largest {gtop:.3f};  4 x largest = {4 * gtop:.3f};  module G = {G:.3f}")


if __name__ == "__main__":
    main()
