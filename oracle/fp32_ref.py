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
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

S32 = 4 * 6.531e-07     # 4 x the largest measured value (docstring); never widened to make a kernel pass
G = 4 * 3.377           # 4 x the largest measured value (docstring), in units of 2^-24
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


def main():
    torch.set_num_threads(max(1, min(4, torch.get_num_threads())))
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
