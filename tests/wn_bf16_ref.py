"""Test helper (not a test): float64 mirror of ``ov_wn_layer_bf16`` (openvoice_amd/csrc/wn_layer_bf16.hip) and its
element-wise acceptance limit.  Plain PyTorch on the CPU.

    x_in = conv_k5(bf16(W_in), bf16(h)) + b_in + cond       float64 sums of the SAME bf16-rounded operands
    acts = bf16(tanh(x_in[:H]) * sigmoid(x_in[H:]))         one rounding to nearest even, directly from float64
    rs   = conv_1x1(bf16(W_rs), acts) + b_rs
    out  = (h + rs[:H]) * mask     skip = (first ? 0 : skip) + rs[H:]       with the unrounded h; last: rs is all skip

Limit per output element (fp32 outputs, so the storage term is half an fp32 ulp, not half a bf16 ulp):

    |out - ref64| <= S * absacc2 + flip + 1/2 ulp_f32(ref64)

``S``        6.4e-7, the fp32 accumulation allowance of oracle/bf16_ref.py, unchanged (measured there, reference against
             reference, x 4).
``absacc2``  the res/skip expression on absolute values: sum |acts| |w_rs| + |b_rs| + |h| (or + |skip_in|), times the mask
             for ``out``.
``flip``     an ``acts`` element whose fp32 value lies on the other side of a bf16 rounding midpoint than the float64 one is
             stored one grid step away and moves every output it feeds by that step times |bf16(w_rs)|:
             ``flip = sum |bf16(W_rs)| * ambiguous * gap`` over the acts whose float64 value lies within
             ``S * absacc1 + G`` of a midpoint.  ``absacc1``: the gate conv's sum on absolute values carried through the
             float64 partial derivatives of tanh(t) sigmoid(s) (what fp32 summation error of t and s can move the gate by).
``G``        the allowance for evaluating the gate itself in fp32 (the kernel: two v_exp_f32 and one v_rcp_f32).  Derived
             reference against reference like S: ``python tests/wn_bf16_ref.py`` prints max |fp32 tanh * sigmoid - float64|
             of PyTorch's CPU fp32 over the pre-activations of the GPU test's parametrised cases (B in {1, 3} x T in
             {1, 2, 3, 15, 16, 17, 129, 130}), five seeds:

                 largest 1.235e-07 (about one fp32 ulp of a value in [0.5, 1))        G = 4 x = 4.94e-7

             against the header's prior for the hardware form, "<= 4e-7 absolute" (include/openvoice_amd.h,
             ov_wn_layer_f32): the same size.  Never widened to make a kernel pass.
The half ulp is taken at |ref64| + slack, as ``oracle.bf16_ref.limit`` takes its half bf16 ulp: an accumulator that lands
just across a power of two from ref64 is rounded on the coarser grid.

``dtype=torch.float32`` evaluates the same expression with fp32 PyTorch convs, fp32 tanh * sigmoid and ``.bfloat16()``
roundings: the honest stand-in for a correct kernel; ``mutant=`` breaks it in one named way (tests/test_wn_bf16_criterion_cpu.py).
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.bf16_ref import S, ambiguous, assert_within, bf16_neighbours, flip, limit, rbf16, ulp_bf16  # noqa: E402,F401

F64 = torch.float64
H, K = 192, 5
G = 4.94e-7             # 4 x 1.235e-07 (module docstring); never widened to make a kernel pass

BATCHES = (1, 3)
LENGTHS = (1, 2, 3, 15, 16, 17, 129, 130)
SEEDS = 5
MUTANTS = ("truncate", "acts_unrounded", "acts_rounded_twice", "residual_from_rounded_h", "missing_tap",
           "halo_shifted", "no_b_rs", "first_ignored", "last_writes_out")


def rand(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ulp_f32(x):
    """Spacing of the fp32 grid in the binade of |x| (24 significant bits; clamped far above subnormals)."""
    _, e = torch.frexp(x.to(F64).abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(x, dtype=F64), e - 24)


def item_lengths(B, T):
    """Ragged lengths of a case: the full length, then T - 5 (at least 1), then a ZERO-length item."""
    return [T, max(1, T - 5), 0][:B]


def case(B, T, seed=0, first=False, last=False, cond="item", lengths=None):
    """Operands of one layer, dense fp32: x [B, H, T] (masked: the WN input always is, modules.py:207), skip, mask,
    g [B or 1, 2H] or None, weights in the reference's NATURAL row order (w_rs has H rows when ``last``).
    Scales: x ~ 0.5 N(0, 1) and b_in ~ N(0, 1), so that the exactly added bias carries a good part of the gate's
    pre-activation and the 960-term sum less: with x ~ N(0, 1) and b_in ~ 0.1 N(0, 1) 2.5 - 2.9 % of ``acts`` are
    ambiguous, above the 2 % the criterion's condition allows (tests/test_wn_bf16_criterion_cpu.py measures the share
    with the reference alone)."""
    s = 1000 * seed + 10 * T + B
    lengths = item_lengths(B, T) if lengths is None else lengths
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).float()
    x = 0.5 * rand(B, H, T, seed=s + 1) * mask[:, None]
    g = None if cond is None else rand(B if cond == "item" else 1, 2 * H, seed=s + 3, scale=0.3)
    rows = H if last else 2 * H
    return dict(x=x, skip=rand(B, H, T, seed=s + 2), mask=mask, g=g,
                w_in=rand(2 * H, H, K, seed=s + 4, scale=(K * H) ** -0.5), b_in=rand(2 * H, seed=s + 5, scale=1.0),
                w_rs=rand(rows, H, 1, seed=s + 6, scale=H ** -0.5), b_rs=rand(rows, seed=s + 7, scale=0.1),
                first=first, last=last)


def _trunc_bf16(t):
    """Round toward zero to bf16 (a wrong kernel: the low 16 bits dropped)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def layer(c, dtype=F64, mutant=None):
    """The layer on the operands ``c`` (``case``).  float64: the mirror -- returns dict(out (None when last), skip,
    lim_out, lim_skip, share) with the limits of the module docstring and the ambiguous share of ``acts``.  float32: the
    stand-in (or a ``mutant`` of it) -- returns dict(out, skip) in fp32, ``out`` None when it writes none."""
    assert mutant is None or (mutant in MUTANTS and dtype == torch.float32)
    x, mask, first, last = c["x"], c["mask"], c["first"], c["last"]
    B = x.shape[0]
    rnd = _trunc_bf16 if mutant == "truncate" else (lambda t: t.float().to(torch.bfloat16).float())
    xb, wi, wr = rnd(x).to(dtype), rnd(c["w_in"]).to(dtype), rnd(c["w_rs"]).to(dtype)
    if mutant == "missing_tap":
        wi = wi.clone()
        wi[:, :, K - 1] = 0
    bias = c["b_in"].to(dtype)[None, :, None]
    if c["g"] is not None:
        bias = bias + c["g"].to(dtype).expand(B, -1)[:, :, None]
    pad = (K - 1) // 2
    xp = F.pad(xb, (pad + 1, pad - 1) if mutant == "halo_shifted" else (pad, pad))
    pre = F.conv1d(xp, wi) + bias
    t, s = pre[:, :H], pre[:, H:]
    a = torch.tanh(t) * torch.sigmoid(s)
    if dtype == F64:
        acts = rbf16(a)
    elif mutant == "acts_unrounded":
        acts = a
    elif mutant == "acts_rounded_twice":      # each gate half stored rounded, the product rounded again
        acts = rnd(rnd(torch.tanh(t)) * rnd(torch.sigmoid(s)))
    else:
        acts = rnd(a).to(dtype)
    b_rs = torch.zeros_like(c["b_rs"]) if mutant == "no_b_rs" else c["b_rs"]
    rs = F.conv1d(acts, wr) + b_rs.to(dtype)[None, :, None]
    keep_skip = (not first) or mutant == "first_ignored"
    skip_in = c["skip"].to(dtype) if keep_skip else torch.zeros_like(rs[:, :H])
    h = xb if mutant == "residual_from_rounded_h" else x.to(dtype)
    m = mask.to(dtype)[:, None]
    if last:
        out, skip = None, skip_in + rs
        if mutant == "last_writes_out":
            out = h * m
    else:
        out, skip = (h + rs[:, :H]) * m, skip_in + rs[:, H:]
    if dtype != F64:
        return dict(out=out, skip=skip)
    # ---- limits (float64 only) -------------------------------------------------------------------------------------
    abs_pre = F.conv1d(F.pad(xb.abs(), (pad, pad)), wi.abs()) + bias.abs()
    th, sg = torch.tanh(t), torch.sigmoid(s)
    absacc1 = (1 - th * th) * sg * abs_pre[:, :H] + th.abs() * sg * (1 - sg) * abs_pre[:, H:]
    lo, hi = bf16_neighbours(a)
    # oracle.bf16_ref.flip on channels-last tensors; its tolerance s * absacc1 becomes S * absacc1 + G
    inter = dict(v1=a.transpose(1, 2), absacc1=(absacc1 + G / S).transpose(1, 2), gap=(hi - lo).transpose(1, 2),
                 w2=wr, scale=1.0)
    fl = flip(inter).transpose(1, 2)
    share = ambiguous(a, S * absacc1 + G).double().mean().item()
    abs_rs = F.conv1d(acts.abs(), wr.abs()) + c["b_rs"].to(F64).abs()[None, :, None]

    def lim(ref, absacc, f):
        slack = S * absacc + f
        return slack + 0.5 * ulp_f32(ref.abs() + slack)

    if last:
        return dict(out=None, skip=skip, lim_out=None, lim_skip=lim(skip, abs_rs + skip_in.abs(), fl), share=share)
    return dict(out=out, skip=skip, lim_out=lim(out, (abs_rs[:, :H] + x.to(F64).abs()) * m, fl[:, :H] * m),
                lim_skip=lim(skip, abs_rs[:, H:] + skip_in.abs(), fl[:, H:]), share=share)


def check(got_out, got_skip, ref, what, family=None, out_before=None):
    """Every element of a result against the mirror ``ref`` (``layer(c)``).  ``got_out`` None = nothing written; with
    ``last`` the mirror writes no ``out``: then ``got_out`` must be None or bit-equal ``out_before``.  Returns the worst
    err / lim."""
    worst = assert_within(got_skip, ref["skip"], ref["lim_skip"], what + " skip", family)
    if ref["out"] is None:
        if got_out is not None:
            assert out_before is not None and torch.equal(got_out.cpu(), out_before.cpu()), f"{what}: out written by a last layer"
        return worst
    assert got_out is not None, f"{what}: no out"
    return max(worst, assert_within(got_out, ref["out"], ref["lim_out"], what + " out", family))


def measure_g(seeds=SEEDS):
    """max |fp32 tanh(t) sigmoid(s) - float64| over the pre-activations of the parametrised cases: {(B, T): value}."""
    table = {}
    for B in BATCHES:
        for T in LENGTHS:
            worst = 0.0
            for seed in range(seeds):
                c = case(B, T, seed)
                r = lambda v: v.to(torch.bfloat16).float()
                pre = F.conv1d(r(c["x"]), r(c["w_in"]), c["b_in"], padding=(K - 1) // 2) + c["g"][:, :, None]
                t, s = pre[:, :H], pre[:, H:]
                d = (torch.tanh(t) * torch.sigmoid(s)).double() - torch.tanh(t.double()) * torch.sigmoid(s.double())
                worst = max(worst, d.abs().max().item())
            table[(B, T)] = worst
    return table


# ---------------------------------------------------------------------------------------------------------------------
# The end-to-end bar: the fp32 oracle with this module's operand rounding hooked into its WaveNet layers
# ---------------------------------------------------------------------------------------------------------------------
E2E_B, E2E_LENGTHS = 2, (40, 64)
# ``measure_e2e`` on the calibrated synthetic converter weights (``synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, 1234)``),
# five seeds: ``python tests/wn_bf16_ref.py e2e`` prints them, tests/test_wn_bf16_criterion_cpu.py recomputes them.  The GPU
# test's bar is 3 x each (the project's practice for chained roundings).
E2E_MEASURED = dict(z=1.561e-2, z_p=2.053e-2, z_hat=1.883e-2, o_hat=5.337e-3)


def oracle_wavenet_bf16(sd, prefix, x, mask, g, n_layers):
    """``oracle.vc_oracle.wavenet`` with the matrix operands of ``ov_wn_layer_bf16`` rounded where the kernel rounds them
    (bf16(h), bf16(W_in), bf16(acts), bf16(W_rs)); the state, the sums and the gate stay fp32 PyTorch."""
    from openvoice_amd.params import effective_weight
    r = lambda t: t.to(torch.bfloat16).float()
    hidden = x.shape[1]
    out = torch.zeros_like(x)
    g_all = F.conv1d(g, effective_weight(sd, prefix + ".cond_layer"), sd[prefix + ".cond_layer.bias"])
    for i in range(n_layers):
        w_in = effective_weight(sd, f"{prefix}.in_layers.{i}")
        x_in = F.conv1d(r(x), r(w_in), sd[f"{prefix}.in_layers.{i}.bias"], padding=(w_in.shape[2] - 1) // 2)
        in_act = x_in + g_all[:, 2 * hidden * i: 2 * hidden * (i + 1)]
        acts = r(torch.tanh(in_act[:, :hidden]) * torch.sigmoid(in_act[:, hidden:]))
        rs = F.conv1d(acts, r(effective_weight(sd, f"{prefix}.res_skip_layers.{i}")), sd[f"{prefix}.res_skip_layers.{i}.bias"])
        if i < n_layers - 1:
            x = (x + rs[:, :hidden]) * mask
            out = out + rs[:, hidden:]
        else:
            out = out + rs
    return out * mask


def e2e_inputs(T, seed, B=E2E_B, bins=513, gin=256):
    gen = torch.Generator().manual_seed(7000 + 10 * T + seed)
    spec = torch.rand(B, bins, T, generator=gen) * 2.0
    lengths = torch.tensor([T, T - 9][:B])
    g_src, g_tgt = 0.3 * torch.randn(B, gin, 1, generator=gen), 0.3 * torch.randn(B, gin, 1, generator=gen)
    return spec, lengths, g_src, g_tgt, torch.randn(B, 192, T, generator=gen)


def measure_e2e(sd, cfg, seeds=SEEDS, tau=0.3):
    """Largest |hooked oracle - fp32 oracle| per output (z, z_p, z_hat, o_hat) over ``E2E_LENGTHS`` and ``seeds`` seeds."""
    from oracle import vc_oracle
    worst = dict(z=0.0, z_p=0.0, z_hat=0.0, o_hat=0.0)
    plain = vc_oracle.wavenet
    for T in E2E_LENGTHS:
        for seed in range(seeds):
            spec, lengths, g_src, g_tgt, noise = e2e_inputs(T, seed)
            with torch.no_grad():
                o0, _, lat0 = vc_oracle.voice_conversion(sd, cfg, spec, lengths, g_src, g_tgt, tau, noise)
                vc_oracle.wavenet = oracle_wavenet_bf16
                try:
                    o1, _, lat1 = vc_oracle.voice_conversion(sd, cfg, spec, lengths, g_src, g_tgt, tau, noise)
                finally:
                    vc_oracle.wavenet = plain
            for name, a, b in zip(("z", "z_p", "z_hat", "o_hat"), lat1 + (o1,), lat0 + (o0,)):
                worst[name] = max(worst[name], (a - b).abs().max().item())
    return worst


if __name__ == "__main__":
    if sys.argv[1:2] == ["e2e"]:
        from openvoice_amd.params import synthetic_state_dict
        from openvoice_amd.utils import CONVERTER_MODEL_CONFIG
        print({k: f"{v:.3e}" for k, v in measure_e2e(synthetic_state_dict(CONVERTER_MODEL_CONFIG, 513, seed=1234),
                                                     CONVERTER_MODEL_CONFIG).items()})
        sys.exit(0)
    tab = measure_g()
    for B in BATCHES:
        print(f"B = {B}: " + "  ".join(f"T{T} {tab[(B, T)]:.3e}" for T in LENGTHS))
    print(f"largest {max(tab.values()):.3e}; x 4 = {4 * max(tab.values()):.3e}")
