"""The ReferenceEncoder kernels of csrc/ref_enc.hip one by one through the C ABI -- ``ov_layernorm_freq_f32``,
``ov_conv2d_s2_relu_f32``, ``ov_gru_f32`` -- each against PyTorch's own operator for the same operation in float64 on
the CPU (``F.layer_norm``, ``F.conv2d``, ``torch.nn.GRU``; never the oracle's restatement), every element compared;
then ``model.ref_enc`` end to end against the oracle with a trained-looking LayerNorm affine and visible biases, at
lengths and batches the rest of the suite does not run.

Tolerance of the kernel tests: the convention of tests/test_gpu_tts.py::_close for fp32 VALU kernels against
PyTorch, max-abs err <= 2e-5 * max(1, |ref|max) with the reference in float64.  Plain fp32 on the CPU sits 20-100x
inside it (LayerNorm 6e-7..9e-7 at scale 3.6, conv 2e-6 at scale 10, GRU 3e-7); the cases whose conditioning is not
obvious assert that themselves, on the CPU, before they look at the device result (``cpu_self_checks()`` runs all of
those checks without a GPU).  The end-to-end bar is the project's own 1e-4 max-abs on ``se`` (tests/test_gpu_e2e.py).

Every device buffer is ``TAIL`` floats longer than the operation needs and the surplus is NaN: an output's surplus must
still be all NaN afterwards (dense outputs have no ``ld``, an overrun would otherwise go unseen), and a read past the
end of an input turns up in the result."""
import ctypes
import math
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib  # noqa: E402
from openvoice_amd.engine import _ptr  # noqa: E402

DEV = "cuda:0"
TAIL = 384
REL = 2e-5
OV_E_BADARG, OV_E_UNSUPPORTED = -1, -2
H = 128                                  # REF_ENC_GRU: the one hidden size ov_gru_f32 has


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bar(ref):
    return REL * max(1.0, ref.abs().max().item())


def _err(got, ref):
    return (got.double() - ref).abs().max().item()


def _dev_in(t):
    """``t`` flat on the device, followed by TAIL NaNs."""
    buf = torch.full((t.numel() + TAIL,), float("nan"))
    buf[:t.numel()] = t.reshape(-1)
    return buf.to(DEV)


def _dev_out(numel):
    return torch.full((numel + TAIL,), float("nan"), device=DEV)


def _check(buf, ref, what):
    """Every element of the device buffer against the float64 ``ref``; the surplus must still be NaN."""
    torch.cuda.synchronize()
    flat = buf.cpu()
    assert torch.isnan(flat[ref.numel():]).all(), f"{what}: the kernel wrote past the end of its output"
    got = flat[:ref.numel()].view(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output (unwritten element, or a read past an input's end)"
    err, bar = _err(got, ref), _bar(ref)
    print(f"{what}: max-abs err {err:.3e} (bar {bar:.3e}, |ref|max {ref.abs().max().item():.3g})")
    assert err <= bar, f"{what}: max-abs err {err:.3e} > {bar:.3e}"
    return got


# ---- 1. ov_layernorm_freq_f32 ----------------------------------------------------------------------------------------
def _ln_ref(x, gamma, beta, eps):
    """float64 F.layer_norm over the frequency axis of [N][F][T]."""
    return F.layer_norm(x.double().transpose(1, 2), (x.shape[1],), gamma.double(), beta.double(), eps).transpose(1, 2)


def _ln_fp32_two_pass(x, gamma, beta, eps):
    """Plain fp32 restatement, variance from the centred values (what the kernel's comment promises)."""
    mean = x.sum(1, keepdim=True) / x.shape[1]
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / x.shape[1]
    return d / torch.sqrt(var + eps) * gamma[None, :, None] + beta[None, :, None]


def _ln_fp32_one_pass(x, gamma, beta, eps):
    """Plain fp32 restatement with the variance as E[x^2] - E[x]^2: what a lost second pass would compute."""
    mean = x.sum(1, keepdim=True) / x.shape[1]
    var = ((x * x).sum(1, keepdim=True) / x.shape[1] - mean * mean).clamp_min(0.0)
    return (x - mean) / torch.sqrt(var + eps) * gamma[None, :, None] + beta[None, :, None]


def _ln_inputs(kind, affine, N, Fq, T):
    g = _gen(1000 * Fq + 10 * T + N)
    if kind == "spec":          # what the product feeds it: magnitudes falling with frequency (test_gpu_e2e.py)
        x = torch.rand(N, Fq, T, generator=g) * torch.linspace(3, 0.05, Fq)[None, :, None]
    else:
        x = torch.randn(N, Fq, T, generator=g)
    if Fq == 2:
        # two rows: y = +-(d / 2) / sqrt(d^2 / 4 + eps) with d = x0 - x1.  At |x| ~ 1 that is a sign function wherever
        # |d| >> sqrt(eps), and where it is not, the rounding of x0 + x1 (6e-8 |x|) times rstd = 316 reaches the bar in
        # fp32 on the CPU too (measured 1.4e-5 against 2.1e-5).  At |x| ~ 0.01 the output moves smoothly through
        # (-1, 1) and fp32 is 100x inside the bar.
        x = 0.01 * x
    if kind == "offset":        # large mean over f relative to its spread: the two-pass case
        x = 40.0 + x
    if kind == "const_col":
        # columns constant over f: variance exactly 0 for that (n, t) alone.  The constants are ones whose running
        # sums are exact in fp32 (2.5 k and 0 for every k <= F), so the mean is exact in ANY summation order and the
        # expected output is beta itself; an arbitrary constant c leaves mean - c of a few ulp(F c) / F behind, which
        # rstd = 316 turns into an error of the summation order, not of the kernel.
        x[0, :, T // 2] = 2.5
        x[N - 1, :, 0] = 0.0
        x[N - 1, :, T - 1] = 2.5
    if affine == "identity":
        gamma, beta = torch.ones(Fq), torch.zeros(Fq)
    else:
        gamma, beta = 1 + 0.3 * torch.randn(Fq, generator=g), 0.3 * torch.randn(Fq, generator=g)
    return x, gamma, beta


# (kind, affine, N, F, T, eps).  F = 1: zero variance everywhere; F = 2, 7: tiny rows; T around the 256-thread block.
LN_CASES = [("randn", "random", N, Fq, T, 1e-5) for Fq in (513, 7, 2, 1) for T in (1, 255, 256, 257, 861, 3000)
            for N in (1, 3)]
LN_CASES += [("randn", "identity", 3, 513, 257, 1e-5),        # control: the affine the synthetic weights carry
             ("const_col", "random", 3, 513, 300, 1e-5),
             ("const_col", "random", 1, 7, 257, 1e-5),
             ("spec", "random", 3, 513, 861, 1e-5),
             ("spec", "random", 1, 513, 65, 1e-5),
             ("randn", "random", 2, 513, 300, 1e-3),          # eps is an argument, not a constant
             ("spec", "random", 2, 513, 300, 1e-3)]
LN_TWO_PASS_CASE = ("offset", "random", 2, 513, 300, 1e-5)


def _ln_id(c):
    return f"{c[0]}-{c[1]}-N{c[2]}-F{c[3]}-T{c[4]}-eps{c[5]:g}"


def _ln_conditioning(case):
    """CPU only: the float64 reference of a case, after asserting that a plain fp32 two-pass restatement is within a
    quarter of the bar -- F = 2 and near-constant columns can cancel, and such an input would test the summation
    order instead of the kernel."""
    kind, affine, N, Fq, T, eps = case
    x, gamma, beta = _ln_inputs(kind, affine, N, Fq, T)
    ref = _ln_ref(x, gamma, beta, eps)
    e32 = _err(_ln_fp32_two_pass(x, gamma, beta, eps), ref)
    assert e32 <= _bar(ref) / 4, f"{_ln_id(case)}: ill-conditioned input, fp32 on the CPU is {e32:.3e} from float64"
    return x, gamma, beta, ref, e32


def _ln_two_pass_margins(case=LN_TWO_PASS_CASE):
    """CPU only: the two-pass case keeps its teeth -- fp32 two-pass at most a fifth of the bar, fp32 one-pass at least
    three times the bar (measured: 1.7e-5 and 2.3e-3 against a bar of 1.3e-4..1.7e-4)."""
    kind, affine, N, Fq, T, eps = case
    x, gamma, beta = _ln_inputs(kind, affine, N, Fq, T)
    ref = _ln_ref(x, gamma, beta, eps)
    bar = _bar(ref)
    two, one = _err(_ln_fp32_two_pass(x, gamma, beta, eps), ref), _err(_ln_fp32_one_pass(x, gamma, beta, eps), ref)
    print(f"layernorm two-pass case: fp32 two-pass {two:.3e}, fp32 one-pass {one:.3e}, bar {bar:.3e}")
    assert two <= bar / 5, f"two-pass fp32 restatement {two:.3e} > a fifth of the bar {bar:.3e}: case too harsh"
    assert one >= 3 * bar, f"one-pass fp32 restatement {one:.3e} < three times the bar {bar:.3e}: case too mild"
    return x, gamma, beta, ref


def _ln_device(x, gamma, beta, eps):
    N, Fq, T = x.shape
    xd, gd, bd, yd = _dev_in(x), _dev_in(gamma), _dev_in(beta), _dev_out(x.numel())
    rc = _lib.load().ov_layernorm_freq_f32(_ptr(xd), _ptr(gd), _ptr(bd), _ptr(yd), N, Fq, T, eps, _st())
    assert rc == 0, rc
    return yd


@pytest.mark.parametrize("case", LN_CASES, ids=_ln_id)
def test_layernorm_freq(case):
    x, gamma, beta, ref, _ = _ln_conditioning(case)
    got = _check(_ln_device(x, gamma, beta, case[5]), ref, "layernorm " + _ln_id(case))
    kind, _, N, Fq, T, _ = case
    want_beta = beta[:, None].expand(Fq, T)
    if Fq == 1:      # x - mean is exactly 0, so rstd = 1 / sqrt(eps) multiplies a zero
        assert torch.equal(got, want_beta[None].expand(N, Fq, T)), "F = 1 must give beta exactly"
    if kind == "const_col":
        for n, t in ((0, T // 2), (N - 1, 0), (N - 1, T - 1)):
            assert torch.equal(got[n, :, t], beta), f"constant column ({n}, {t}) must give beta exactly"


def test_layernorm_freq_two_pass_variance():
    """Mean 40, spread 1 over f: E[x^2] - E[x]^2 in fp32 loses the variance's low digits (2.3e-3 on the output),
    the centred second pass does not (1.7e-5).  Both margins are asserted on the CPU first."""
    x, gamma, beta, ref = _ln_two_pass_margins()
    _check(_ln_device(x, gamma, beta, LN_TWO_PASS_CASE[5]), ref, "layernorm " + _ln_id(LN_TWO_PASS_CASE))


def test_layernorm_freq_bad_arguments():
    lib = _lib.load()
    x, gamma, beta = _ln_inputs("randn", "random", 2, 7, 5)
    xd, gd, bd, yd = _dev_in(x), _dev_in(gamma), _dev_in(beta), _dev_out(x.numel())
    ptrs = [_ptr(xd), _ptr(gd), _ptr(bd), _ptr(yd)]
    for i in range(4):
        args = list(ptrs)
        args[i] = None
        assert lib.ov_layernorm_freq_f32(*args, 2, 7, 5, 1e-5, _st()) == OV_E_BADARG, f"null pointer {i}"
    for N, Fq, T in ((0, 7, 5), (65536, 7, 5), (-1, 7, 5), (2, 0, 5), (2, 7, 0)):
        assert lib.ov_layernorm_freq_f32(*ptrs, N, Fq, T, 1e-5, _st()) == OV_E_BADARG, (N, Fq, T)
    torch.cuda.synchronize()
    assert torch.isnan(yd).all(), "a refused call must not launch"


# ---- 2. ov_conv2d_s2_relu_f32 ----------------------------------------------------------------------------------------
def _conv_inputs(N, Cin, Cout, Fi, Ti):
    """Weights never symmetric in kh / kw; a bias large enough that dropping or mis-indexing it is far outside the
    bar, and that a good share of the outputs is clamped by the ReLU."""
    g = _gen(((N * 131 + Cin) * 131 + Cout) * 1031 + Fi * 4099 + Ti)
    x = torch.randn(N, Cin, Fi, Ti, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = 0.5 * torch.randn(Cout, generator=g)
    return x, w, b


def _conv_pre64(x, w, b):
    """float64 pre-activation in the kernel's [N][C][F][T] layout: the weight's kh runs along time, kw along
    frequency, so PyTorch sees the image as [N][C][T][F]."""
    return F.conv2d(x.double().transpose(2, 3), w.double(), b.double(), stride=2, padding=1).transpose(2, 3)


def _conv_case(N, Cin, Cout, Fi, Ti):
    x, w, b = _conv_inputs(N, Cin, Cout, Fi, Ti)
    pre = _conv_pre64(x, w, b)
    ref = pre.relu()
    Fo, To = (Fi - 1) // 2 + 1, (Ti - 1) // 2 + 1
    assert ref.shape == (N, Cout, Fo, To)
    xd, wd, bd, yd = _dev_in(x), _dev_in(w), _dev_in(b), _dev_out(ref.numel())
    rc = _lib.load().ov_conv2d_s2_relu_f32(_ptr(xd), _ptr(wd), _ptr(bd), _ptr(yd), N, Cin, Cout, Fi, Ti, _st())
    assert rc == 0, rc
    got = _check(yd, ref, f"conv2d N{N} {Cin}->{Cout} {Fi}x{Ti} (Fo*To = {Fo * To})")
    clamped = pre < -_bar(ref)
    assert clamped.any(), "the case must exercise the ReLU"
    assert (got[clamped] == 0.0).all(), "outputs whose float64 pre-activation is below minus the bar must be exactly 0"


CONV_STACK = [(1, 32, 513), (32, 32, 257), (32, 64, 129), (64, 64, 65), (64, 128, 33), (128, 128, 17)]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("Ti", [1, 2, 3, 14, 27])
@pytest.mark.parametrize("layer", range(6))
def test_conv2d_s2_relu_stack_layers(layer, Ti, N):
    """The six layers at their real channel counts and frequency sizes."""
    Cin, Cout, Fi = CONV_STACK[layer]
    _conv_case(N, Cin, Cout, Fi, Ti)


@pytest.mark.parametrize("layer,Ti", [(0, 861), (5, 64)])
def test_conv2d_s2_relu_stack_layers_long(layer, Ti):
    Cin, Cout, Fi = CONV_STACK[layer]
    _conv_case(3, Cin, Cout, Fi, Ti)


@pytest.mark.parametrize("Fi,Ti", [(1, 1), (1, 5), (5, 1), (2, 2), (4, 6), (5, 6), (6, 5), (7, 7)])
def test_conv2d_s2_relu_small_images(Fi, Ti):
    """Every parity and the degenerate sizes: on an odd size the last output reads the zero padding on the far side,
    on an even size it does not."""
    _conv_case(2, 16, 16, Fi, Ti)


@pytest.mark.parametrize("Fi,Ti,prod", [(29, 34, 255), (30, 33, 255), (31, 32, 256), (32, 31, 256), (2, 514, 257),
                                        (513, 1, 257), (32, 63, 512), (53, 38, 513), (54, 37, 513)])
def test_conv2d_s2_relu_block_seam(Fi, Ti, prod):
    """Fo * To on either side of a multiple of the 256-thread block: the seam of p = fo * To + to and the
    p >= Fo * To guard are both crossed."""
    assert ((Fi - 1) // 2 + 1) * ((Ti - 1) // 2 + 1) == prod
    _conv_case(2, 16, 16, Fi, Ti)


def test_conv2d_s2_relu_batch_40():
    _conv_case(40, 16, 16, 6, 5)


def test_conv2d_s2_relu_bad_arguments():
    lib = _lib.load()
    x, w, b = _conv_inputs(2, 16, 16, 4, 6)
    xd, wd, bd, yd = _dev_in(x), _dev_in(w), _dev_in(b), _dev_out(2 * 16 * 2 * 3)
    ptrs = [_ptr(xd), _ptr(wd), _ptr(bd), _ptr(yd)]
    assert lib.ov_conv2d_s2_relu_f32(*ptrs, 1, 16, 24, 4, 6, _st()) == OV_E_UNSUPPORTED, "Cout = 24"
    for i in range(4):
        args = list(ptrs)
        args[i] = None
        assert lib.ov_conv2d_s2_relu_f32(*args, 2, 16, 16, 4, 6, _st()) == OV_E_BADARG, f"null pointer {i}"
    for dims in ((0, 16, 16, 4, 6), (2, 0, 16, 4, 6), (2, 16, 0, 4, 6), (2, 16, 16, 0, 6), (2, 16, 16, 4, 0),
                 (65536, 16, 16, 4, 6)):
        assert lib.ov_conv2d_s2_relu_f32(*ptrs, *dims, _st()) == OV_E_BADARG, dims
    torch.cuda.synchronize()
    assert torch.isnan(yd).all(), "a refused call must not launch"


# ---- 3. ov_gru_f32 ---------------------------------------------------------------------------------------------------
def _gru_setup(N, T, gain, n_in=16):
    """A float64 torch.nn.GRU with random parameters, and a random input.  W_hh = gain * randn / sqrt(H) with gain in
    {1, 2} only: above that the recurrence is chaotic and fp32 itself diverges (fp32 vs float64 on the CPU at T = 400:
    2.2e-7 at gain 1, 2.7e-7 at gain 2, 7.1e-7 at gain 3, 1.8 at gain 4).  b_hh = 0.5 randn, and W_ih x + b_ih of scale
    1.5 so that the gates leave their linear range.  The parameters are drawn in fp32 and widened, so handing them to
    the kernel rounds nothing."""
    assert gain in (1, 2)
    g = _gen(7919 * gain + 31 * T + N)
    gru = torch.nn.GRU(n_in, H, batch_first=True).double()
    with torch.no_grad():
        gru.weight_ih_l0.copy_(1.5 * torch.randn(3 * H, n_in, generator=g) / math.sqrt(n_in))
        gru.bias_ih_l0.copy_(0.3 * torch.randn(3 * H, generator=g))
        gru.weight_hh_l0.copy_(gain * torch.randn(3 * H, H, generator=g) / math.sqrt(H))
        gru.bias_hh_l0.copy_(0.5 * torch.randn(3 * H, generator=g))
    x = torch.randn(N, T, n_in, generator=g).double()
    return gru, x


def _gru_gi(gru, x):
    """W_ih x + b_ih in float64, rounded to fp32 into the kernel's [N][3H][T] layout."""
    with torch.no_grad():
        return (x @ gru.weight_ih_l0.t() + gru.bias_ih_l0).float().transpose(1, 2).contiguous()


def _gru_ref(gru, x):
    with torch.no_grad():
        return gru(x)[1][0]                  # final state [N, H], float64


def _gru_fp32(gi, whh, bhh):
    """Plain fp32 restatement of the recurrence on the inputs the kernel gets (conditioning check only)."""
    h = torch.zeros(gi.shape[0], H)
    for t in range(gi.shape[2]):
        gh = h @ whh.t() + bhh
        r = torch.sigmoid(gi[:, :H, t] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H, t] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:, t] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
    return h


def _gru_conditioning(gru, x):
    """CPU only: (gi, W_hh, b_hh, float64 final state) after asserting that fp32 on the CPU is within a tenth of the
    bar -- a later change of seeds or scales cannot turn the case into noise."""
    gi, ref = _gru_gi(gru, x), _gru_ref(gru, x)
    whh, bhh = gru.weight_hh_l0.detach().float(), gru.bias_hh_l0.detach().float()
    e32 = _err(_gru_fp32(gi, whh, bhh), ref)
    assert e32 <= _bar(ref) / 10, f"ill-conditioned recurrence: fp32 on the CPU is {e32:.3e} from float64"
    return gi, whh, bhh, ref, e32


def _gru_case(gru, x, what):
    gi, whh, bhh, ref, _ = _gru_conditioning(gru, x)
    N, _, T = gi.shape
    gid, wd, bd, hd = _dev_in(gi), _dev_in(whh.t().contiguous()), _dev_in(bhh), _dev_out(N * H)
    rc = _lib.load().ov_gru_f32(_ptr(gid), _ptr(wd), _ptr(bd), _ptr(hd), N, H, T, _st())
    assert rc == 0, rc
    _check(hd, ref, what)


GRU_T, GRU_N, GRU_GAIN = [1, 2, 14, 47, 400], [1, 5, 33], [1, 2]


@pytest.mark.parametrize("gain", GRU_GAIN)
@pytest.mark.parametrize("N", GRU_N)
@pytest.mark.parametrize("T", GRU_T)
def test_gru_final_state(T, N, gain):
    """Against torch.nn.GRU itself: pins the gate order (r, z, n), the place of r (it multiplies W_hn h + b_hn, bias
    included) and the transposed [H][3H] weight layout."""
    gru, x = _gru_setup(N, T, gain)
    _gru_case(gru, x, f"gru T{T} N{N} gain{gain}")


@pytest.mark.parametrize("gain", GRU_GAIN)
@pytest.mark.parametrize("steps", [1, 2, 3])
def test_gru_first_steps_of_a_long_sequence(steps, gain):
    """The T = 400 sequence cut after its first steps: the state after each of them, compared on its own before the
    recurrence can forget."""
    gru, x = _gru_setup(5, 400, gain)
    _gru_case(gru, x[:, :steps].contiguous(), f"gru first {steps} of T400 N5 gain{gain}")


def test_gru_bad_arguments():
    lib = _lib.load()
    gru, x = _gru_setup(2, 3, 1)
    gid, wd = _dev_in(_gru_gi(gru, x)), _dev_in(gru.weight_hh_l0.detach().float().t().contiguous())
    bd, hd = _dev_in(gru.bias_hh_l0.detach().float()), _dev_out(2 * H)
    ptrs = [_ptr(gid), _ptr(wd), _ptr(bd), _ptr(hd)]
    assert lib.ov_gru_f32(*ptrs, 2, 64, 3, _st()) == OV_E_UNSUPPORTED, "H = 64"
    for i in range(4):
        args = list(ptrs)
        args[i] = None
        assert lib.ov_gru_f32(*args, 2, H, 3, _st()) == OV_E_BADARG, f"null pointer {i}"
    for N, T in ((0, 3), (2, 0), (-1, 3)):
        assert lib.ov_gru_f32(*ptrs, N, H, T, _st()) == OV_E_BADARG, (N, T)
    torch.cuda.synchronize()
    assert torch.isnan(hd).all(), "a refused call must not launch"


# ---- 4. the encoder end to end, where the suite has not been ---------------------------------------------------------
SE_TOL = 1e-4


def _trained_looking_sd(sd):
    """A copy of the synthetic weights with what they leave trivial in ref_enc made visible: a LayerNorm affine that
    differs for every f, and conv / GRU biases of std 0.3 instead of 0.02."""
    out = OrderedDict((k, v.clone()) for k, v in sd.items())
    g = _gen(2718)
    n = out["ref_enc.layernorm.weight"].numel()
    out["ref_enc.layernorm.weight"] = 1 + 0.3 * torch.randn(n, generator=g)
    out["ref_enc.layernorm.bias"] = 0.3 * torch.randn(n, generator=g)
    for k in [f"ref_enc.convs.{i}.bias" for i in range(6)] + ["ref_enc.gru.bias_ih_l0", "ref_enc.gru.bias_hh_l0"]:
        out[k] = out[k] * (0.3 / out[k].std())
    return out


@pytest.fixture(scope="module")
def trained_looking(synth_sd):
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG
    sd = _trained_looking_sd(synth_sd)
    assert torch.equal(synth_sd["ref_enc.layernorm.weight"], torch.ones(513)), "the shared weights stay as they are"
    model = SynthesizerTrn(0, 513, n_speakers=0, zero_g=False, **CONVERTER_MODEL_CONFIG)
    model.load_state_dict(sd, strict=True)
    return sd, model.to(DEV).eval()


def _spec(N, T, seed):
    return torch.rand(N, 513, T, generator=_gen(seed)) * torch.linspace(3, 0.05, 513)[None, :, None]


@pytest.mark.parametrize("N,T", [(3, 1), (3, 2), (3, 3), (3, 5), (3, 33), (3, 200), (3, 861), (3, 3000), (40, 65)])
def test_reference_encoder_trained_looking_weights_matches_oracle(trained_looking, N, T):
    """One to three frames (every To collapses to 1, one GRU step, a 1-column gru_in conv), a five-minute-scale clip
    (47 GRU steps) and a batch of 40, with every affine and bias of the encoder visible."""
    from oracle import vc_oracle
    sd, model = trained_looking
    spec = _spec(N, T, 100 * T + N)
    with torch.no_grad():
        ref = vc_oracle.reference_encoder(sd, spec.transpose(1, 2))
    se = model.ref_enc(spec.to(DEV).transpose(1, 2))
    torch.cuda.synchronize()
    assert se.shape == ref.shape == (N, 256)
    err = (se.cpu() - ref).abs().max().item()
    print(f"ref_enc N{N} T{T}: max-abs err {err:.3e} (bar {SE_TOL:.0e}, |se|max {ref.abs().max().item():.3g})")
    assert err <= SE_TOL, err


@pytest.mark.parametrize("T", [3, 200])
def test_reference_encoder_rows_do_not_depend_on_batch_position(trained_looking, T):
    """The same clip twice in one batch and alone: bit-identical rows; a re-run of the batch: bit-identical."""
    _, model = trained_looking
    clips = _spec(2, T, 4242 + T).to(DEV)
    batch = torch.stack([clips[0], clips[1], clips[0]])
    se = model.ref_enc(batch.transpose(1, 2)).clone()
    again = model.ref_enc(batch.transpose(1, 2)).clone()
    alone = model.ref_enc(clips[:1].transpose(1, 2)).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(se).all())
    assert torch.equal(se, again), "same batch twice must be bit-identical"
    assert torch.equal(se[0], se[2]), "the same clip at rows 0 and 2 of one batch must give the same bits"
    assert torch.equal(se[0], alone[0]), "a clip must give the same bits alone and inside a batch"
    assert not torch.equal(se[0], se[1])


# ---- the CPU-side checks of this file, runnable without a GPU --------------------------------------------------------
def cpu_self_checks():
    """Every conditioning / margin assertion the tests above make before they touch the device:
    ``python -c "import sys; sys.path[:0] = ['.', 'tests']; import test_gpu_ref_enc as t; t.cpu_self_checks()"``."""
    worst = (0.0, "")
    for c in LN_CASES:
        ref, e32 = _ln_conditioning(c)[3:]
        worst = max(worst, (e32 / _bar(ref), _ln_id(c)))
    print(f"layernorm: worst fp32 / bar over {len(LN_CASES)} cases = {worst[0]:.3f} ({worst[1]})")
    _ln_two_pass_margins()
    for gain in GRU_GAIN:
        for T in GRU_T:
            for N in GRU_N:
                ref, e32 = _gru_conditioning(*_gru_setup(N, T, gain))[3:]
                print(f"gru T{T} N{N} gain{gain}: fp32 on the CPU {e32:.3e} from float64 (bar {_bar(ref):.1e})")
        for steps in (1, 2, 3):
            gru, x = _gru_setup(5, 400, gain)
            _gru_conditioning(gru, x[:, :steps].contiguous())
    print("cpu self-checks passed")
