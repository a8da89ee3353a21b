"""The element-wise bf16 criterion (oracle/bf16_ref.py: half a bf16 ulp + S * absacc + flip against a float64 mirror)
can tell right from wrong -- on the CPU, reference against reference, no kernel involved.

Honest stand-in: the same mirror evaluated with fp32 PyTorch convs and ``.bfloat16()`` roundings (what a correct kernel
computes, in another summation order) is ACCEPTED for the single conv and both fused-pair forms.

Every deliberately wrong fp32 restatement below is REJECTED.  Record of the gap: the old global bound of the GPU files,
max|out - ref| <= 1e-2 * max(1, max|ref|), ACCEPTS all of these at all three shapes (asserted below):
  truncate            output truncated to bf16 instead of rounded to nearest even
  no_reround          leaky-ReLU output not re-rounded to bf16 before the matrix product
  slope_bf16          slope taken as bf16(0.1) instead of fp32 0.1
  round_before_scale  rounded before the ``scale`` multiply (double rounding)
  t_unrounded         the intermediate t not rounded at all (pairs)
and rejects these only through their largest term (printed, not asserted: they sit at the old bound, and the same
fault on a typical product of |x w| = 0.01 passes it):
  drop_product        one (channel, tap) product of conv2 dropped at every 64th time column (pairs)
  missing_tap         one whole tap missing at one time column next to the right edge
  zero_weight_column  one (input channel, tap) weight column zeroed
Shapes (C, K, d): (32, 3, 1), (64, 7, 3), (128, 11, 5); B = 2, L = 601."""
import pytest
import torch
import torch.nn.functional as F

from oracle import bf16_ref as R

SHAPES = [(32, 3, 1), (64, 7, 3), (128, 11, 5)]
B, L = 2, 601
F32 = torch.float32
OLD_BOUND_ACCEPTS = ("truncate", "no_reround", "slope_bf16", "round_before_scale", "t_unrounded")


def _rand(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _r(t):
    return t.to(torch.bfloat16).float()


def _trunc(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _conv(x, w, d=1):
    return R._conv(x, w, d)


def _ops(c, k, seed=0):
    w1, b1 = _r(_rand(c, c, k, seed=seed + 1, scale=(c * k) ** -0.5)), _rand(c, seed=seed + 2, scale=0.1)
    w2, b2 = _r(_rand(c, c, k, seed=seed + 3, scale=0.5 * (c * k) ** -0.5)), _rand(c, seed=seed + 4, scale=0.1)
    x, res, add = (_r(_rand(B, L, c, seed=seed + 5 + i)) for i in range(3))
    return x, res, add, w1, b1, w2, b2


def _finish(acc, scale, variant):
    """The last storage point of every form: scale, round."""
    if variant == "round_before_scale":
        return _r(_r(acc) * scale)
    if variant == "truncate":
        return _trunc(acc * scale)
    return _r(acc * scale)


def _slope(variant):
    return torch.tensor(0.1).to(torch.bfloat16).item() if variant == "slope_bf16" else 0.1


def _single(x, res, add, w, b, k, d, scale, variant=None):
    """fp32 restatement of the single conv (tests/test_gpu_bf16.py), optionally wrong."""
    xin = F.leaky_relu(x, _slope(variant))
    if variant != "no_reround":
        xin = _r(xin)
    if variant == "zero_weight_column":
        w = w.clone()
        w[:, 7, 1] = 0
    acc = _conv(xin, w, d) + b + res + add
    if variant == "missing_tap":          # tap 0 of time column L - 2 reads row L - 2 - pad (inside the tensor)
        acc[:, L - 2, :] -= xin[:, L - 2 - (k - 1) * d // 2, :] @ w[:, :, 0].t()
    return _finish(acc, scale, variant)


def _drop(y, t, w2, k):
    """Drop the product (input channel 5, centre tap) of conv2 at every 64th time column."""
    y = y.clone()
    y[:, ::64, :] -= t[:, ::64, 5:6] * w2[:, 5, (k - 1) // 2][None, None, :]
    return y


def _pair1(x, add, w1, b1, w2, b2, k, d, scale, variant=None):
    """fp32 restatement of the first-generation pair (tests/test_gpu_bf16_pair.py::_reference), optionally wrong."""
    s = _slope(variant)
    v = _conv(_r(F.leaky_relu(x, s)), w1, d) + b1
    if variant == "t_unrounded":
        t = F.leaky_relu(v, s)
    elif variant == "no_reround":
        t = F.leaky_relu(_r(v), s)
    else:
        t = _r(F.leaky_relu(_r(v), s))
    y = _conv(t, w2) + b2
    if variant == "drop_product":
        y = _drop(y, t, w2, k)
    return _finish(y + x + add, scale, variant)


def _pair2(xa, add, w1, b1, w2, b2, k, d, scale, variant=None):
    """fp32 restatement of the second-generation pair with the running sum (tests/test_gpu_bf16_pair2.py), optionally
    wrong; ``round_before_scale`` is this form's own design and ``no_reround`` has no counterpart here."""
    s = _slope(variant)
    t = F.leaky_relu(_conv(xa, w1, d) + b1, s)
    if variant != "t_unrounded":
        t = _r(t)
    inv = torch.tensor(1.0) / torch.tensor(0.1)
    y = _conv(t, w2) + b2
    if variant == "drop_product":
        y = _drop(y, t, w2, k)
    y = y + torch.where(xa >= 0, xa, xa * inv)
    return _finish(_r(y) + add, scale, variant)


def _verdicts(out, ref64, lim):
    """(worst err / lim, offending elements, accepted by the old global bound)."""
    err = (out.double() - ref64).abs()
    ratio = err / lim
    refmax = R.rbf16(ref64).abs().max().item()
    return ratio.max().item(), int((ratio > 1).sum()), err.max().item() <= 1e-2 * max(1.0, refmax)


def _judge(name, variant, out, ref64, lim, old_ok):
    worst, bad, old = _verdicts(out, ref64, lim)
    print(f"{name} {variant or 'honest'}: worst err/lim {worst:.3f}, {bad} elements over, old global bound "
          f"{'accepts' if old else 'rejects'}")
    if variant is None:
        assert worst <= 1.0, f"{name}: the honest fp32 stand-in is rejected ({worst:.3f}, {bad} elements)"
        assert old
    else:
        assert worst > 1.0 and bad > 0, f"{name}: wrong variant {variant} is accepted (worst {worst:.3f})"
        if variant in old_ok:
            assert old, f"{name} {variant}: the record in the docstring says the old bound accepts this"


@pytest.mark.parametrize("c,k,d", SHAPES)
def test_single_conv_criterion(c, k, d):
    x, res, add, w, b, _, _ = _ops(c, k)
    scale = 1.0 / 3.0
    ref64, absacc = R.conv_single(x, w, b, dil=d, in_slope=0.1, res=res, add=add, scale=scale)
    lim = R.limit(ref64, absacc)
    honest = R.rbf16(R.conv_single(x, w, b, dil=d, in_slope=0.1, res=res, add=add, scale=scale, dtype=F32)[0])
    assert torch.equal(honest, _single(x, res, add, w, b, k, d, R.f32(scale)))      # the two restatements are one
    _judge(f"single C={c} k={k} d={d}", None, honest, ref64, lim, ())
    for variant in ("truncate", "no_reround", "slope_bf16", "round_before_scale", "missing_tap", "zero_weight_column"):
        _judge(f"single C={c} k={k} d={d}", variant, _single(x, res, add, w, b, k, d, R.f32(scale), variant), ref64, lim,
               OLD_BOUND_ACCEPTS)
    # the output activation of the two-launch path (conv1 stores t activated)
    ref64, absacc = R.conv_single(x, w, b, dil=d, in_slope=0.1, out_slope=0.1)
    honest = R.rbf16(R.conv_single(x, w, b, dil=d, in_slope=0.1, out_slope=0.1, dtype=F32)[0])
    _judge(f"single+out_slope C={c} k={k} d={d}", None, honest, ref64, R.limit(ref64, absacc), ())


@pytest.mark.parametrize("c,k,d", SHAPES)
def test_first_generation_pair_criterion(c, k, d):
    x, _, add, w1, b1, w2, b2 = _ops(c, k)
    scale = 1.0 / 3.0
    ref64, absacc, inter = R.pair1(x, w1, b1, w2, b2, d, add=add, scale=scale)
    share = R.ambiguous_share(inter)
    print(f"pair C={c} k={k} d={d}: ambiguous share of t {share:.2e}")
    assert share < 0.5, "flip would cover everything: the criterion hides failures"
    lim = R.limit(ref64, absacc, R.flip(inter))
    honest = R.rbf16(R.pair1(x, w1, b1, w2, b2, d, add=add, scale=scale, dtype=F32)[0])
    assert torch.equal(honest, _pair1(x, add, w1, b1, w2, b2, k, d, R.f32(scale)))
    _judge(f"pair C={c} k={k} d={d}", None, honest, ref64, lim, ())
    for variant in ("truncate", "no_reround", "slope_bf16", "round_before_scale", "drop_product", "t_unrounded"):
        _judge(f"pair C={c} k={k} d={d}", variant, _pair1(x, add, w1, b1, w2, b2, k, d, R.f32(scale), variant), ref64,
               lim, OLD_BOUND_ACCEPTS)


@pytest.mark.parametrize("c,k,d", SHAPES)
def test_second_generation_pair_criterion(c, k, d):
    x, _, add, w1, b1, w2, b2 = _ops(c, k)
    xa = _r(F.leaky_relu(x, 0.1))
    scale = 1.0 / 3.0
    ref64, absacc, inter = R.pair2(xa, w1, b1, w2, b2, d, add=add, scale=scale)
    share = R.ambiguous_share(inter)
    print(f"pair2 C={c} k={k} d={d}: ambiguous share of t {share:.2e}")
    assert share < 0.5, "flip would cover everything: the criterion hides failures"
    lim = R.limit(ref64, absacc, R.flip(inter))
    honest = R.rbf16(R.pair2(xa, w1, b1, w2, b2, d, add=add, scale=scale, dtype=F32)[0])
    assert torch.equal(honest, _pair2(xa, add, w1, b1, w2, b2, k, d, R.f32(scale)))
    _judge(f"pair2 C={c} k={k} d={d}", None, honest, ref64, lim, ())
    for variant in ("truncate", "slope_bf16", "drop_product", "t_unrounded"):
        _judge(f"pair2 C={c} k={k} d={d}", variant, _pair2(xa, add, w1, b1, w2, b2, k, d, R.f32(scale), variant), ref64,
               lim, OLD_BOUND_ACCEPTS)
    # without the running sum: one rounding on the way out, output activation
    ref64, absacc, inter = R.pair2(xa, w1, b1, w2, b2, d, out_slope=0.1)
    honest = R.rbf16(R.pair2(xa, w1, b1, w2, b2, d, out_slope=0.1, dtype=F32)[0])
    _judge(f"pair2+out_slope C={c} k={k} d={d}", None, honest, ref64, R.limit(ref64, absacc, R.flip(inter)), ())


def test_rounding_helpers_agree_with_torch_bfloat16():
    x = torch.randn(100000, generator=torch.Generator().manual_seed(0)) * 3
    assert torch.equal(R.rbf16(x.double()).float(), x.to(torch.bfloat16).float())
    ties = torch.tensor([1.00390625, 1.01171875, -2.0078125, 0.99609375 + 2 ** -9])      # midpoints: ties to even
    assert torch.equal(R.rbf16(ties.double()).float(), ties.to(torch.bfloat16).float())
    lo, hi = R.bf16_neighbours(x.double())
    assert ((lo <= x.double()) & (x.double() <= hi)).all() and torch.equal(hi - lo, R.ulp_bf16(x.double()))
    assert R.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -0.75])).tolist() == [2 ** -7, 2 ** -7, 2 ** -6, 2 ** -8]
