"""The criterion of the waveform-edge kernels (oracle/edge_ref.py: S_POST * absacc + T_TANH * 2^-24 |ref| for
conv_post + tanh, S_LIN * absacc for the conditioning GEMV, exact equality for the copy and framing kernels) can tell right
from wrong -- on the CPU, reference against reference, no kernel involved.

Honest stand-ins: ``F.conv1d`` in fp32 followed by ``torch.tanh``, and an fp32 ``x @ w.T + b`` (PyTorch's own summation
order), land at err / lim <= 1 on every element at every shape of tests/test_gpu_edge_kernels.py, benign and stress data;
the fp32 restatements of the kernels' own order (``conv_post_chain``, ``linear_chain``) do too.  The worst ratio per
kernel is printed.

Every deliberately wrong variant exceeds its limit (differs, for the exact mirrors) on at least one element at the
smallest shape at which the fault exists:
  conv_post: centre tap dropped (L = 1); the left halo of a 4-sample group read as zero (L = 8, sample 4); the right halo
  read as zero (L = 8, sample 3); a limit applied one group late.  linear: lanes >= 32 dropped from the butterfly
  (Kdim = 33); the bias row off by one.  mask: ``<=`` for ``<``.  framing: reflection k = -i - 1 in place of -i; right
  reflection 2 n - i in place of 2 (n - 1) - i; zero beyond the pad replaced by further reflection.  stitch: the source
  offset taken from core_lo instead of core_lo - first_frame.  unpad: ``ld`` used as the destination stride.

The exact mirrors agree with independent PyTorch formulations on random small cases: ``F.pad(mode="reflect")`` +
``unfold`` for the framing, ``arange < lengths`` (openvoice/commons.py:121-125) for the mask, plain slicing for stitch
and unpad."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import edge_ref as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


def _report(what, w):
    print(f"RATIO {what} {w:.3f}")
    return w


# ---- honest stand-ins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", E.POST_CS)
def test_honest_conv_post_stand_ins_are_accepted(C):
    worst = {"conv1d+tanh": 0.0, "chain+tanh": 0.0}
    for c, K, L in E.POST_SHAPES:
        if c != C:
            continue
        for stress in (False, True):
            o = E.post_operands(C, K, L, stress=stress)
            ref = E.conv_post_tanh(o["x"], o["w"])
            got = E.conv_post_tanh(o["x"], o["w"], dtype=F32).ref
            assert got.dtype == F32 and torch.isfinite(got).all()
            worst["conv1d+tanh"] = max(worst["conv1d+tanh"], E.worst(got, ref))
            worst["chain+tanh"] = max(worst["chain+tanh"], E.worst(torch.tanh(E.conv_post_chain(o["x"], o["w"])), ref))
            if stress:                                           # the all-zero item: lim = 0 and an exact 0
                assert (ref.lim[2] == 0).all() and (got[2] == 0).all()
    for name, w in worst.items():
        _report(f"stand-in conv_post C={C} {name}", w)
    assert all(w <= 1.0 for w in worst.values()), worst


def test_honest_linear_stand_ins_are_accepted():
    worst = {"matmul": 0.0, "chain": 0.0}
    for M, Kd in E.LIN_SHAPES:
        for stress in (False, True):
            o = E.linear_operands(M, Kd, stress=stress)
            for bias in (o["bias"], None):
                ref = E.linear(o["x"], o["w"], bias)
                worst["matmul"] = max(worst["matmul"], E.worst(E.linear(o["x"], o["w"], bias, dtype=F32).ref, ref))
                worst["chain"] = max(worst["chain"], E.worst(E.linear_chain(o["x"], o["w"], bias), ref))
    for name, w in worst.items():
        _report(f"stand-in linear {name}", w)
    assert all(w <= 1.0 for w in worst.values()), worst


# ---- wrong variants with a limit: fp32 computations with one fault each -------------------------------------------------------
def _post(L, C=32, K=7):
    o = E.post_operands(C, K, L)
    return o["x"], o["w"]


def _wrong_centre_tap():
    x, w = _post(1)
    bad = w.clone()
    bad[:, 3] = 0                                    # the only tap a single sample has
    return E.conv_post_tanh(x, bad, dtype=F32).ref, E.conv_post_tanh(x, w), None


def _group_with_zero_halo(x, w, t0, side):
    """Samples [t0, t0 + 4) as the 16-byte path computes them, with the ``side`` halo vector read as zero."""
    z = x.clone()
    if side == "lo":
        z[:, :, :t0] = 0
    else:
        z[:, :, t0 + 4:] = 0
    good = E.conv_post_tanh(x, w, dtype=F32).ref
    good[:, t0:t0 + 4] = E.conv_post_tanh(z, w, dtype=F32).ref[:, t0:t0 + 4]
    return good


def _wrong_left_halo():
    x, w = _post(8)
    return _group_with_zero_halo(x, w, 4, "lo"), E.conv_post_tanh(x, w), 4


def _wrong_right_halo():
    x, w = _post(8)
    return _group_with_zero_halo(x, w, 0, "hi"), E.conv_post_tanh(x, w), 3


def _wrong_limit_one_group_late():
    x, w = _post(16)
    limit = [0, 4, 12]
    full = E.conv_post_tanh(x, w, dtype=F32).ref
    late = torch.arange(16)[None, :] < (torch.tensor(limit) + 4)[:, None]
    return full * late, E.conv_post_tanh(x, w, limit=limit), None


def _lin(M, Kd):
    o = E.linear_operands(M, Kd)
    return o["x"], o["w"], o["bias"]


def _wrong_half_butterfly():
    x, w, b = _lin(7, 33)
    return E.linear_chain(x, w, b, lanes=32), E.linear(x, w, b), None


def _wrong_bias_row():
    x, w, b = _lin(7, 33)
    return E.linear_chain(x, w, torch.roll(b, 1)), E.linear(x, w, b), None


WRONG = [("centre_tap", _wrong_centre_tap), ("left_halo_zero", _wrong_left_halo), ("right_halo_zero", _wrong_right_halo),
         ("limit_one_group_late", _wrong_limit_one_group_late), ("half_butterfly", _wrong_half_butterfly),
         ("bias_row_off_by_one", _wrong_bias_row)]


@pytest.mark.parametrize("name,fn", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_variants_are_rejected(name, fn):
    got, ref, sample = fn()
    q = E.ratio(got, ref)
    w = _report(f"wrong {name}", q.max().item())
    assert w > 1.0
    if sample is not None:                           # the sample the fault is named after shows it
        assert q[:, sample].max().item() > 1.0
    print(f"      elements over the limit: {(q > 1).sum().item()} of {q.numel()}")


def test_the_limited_mirror_is_zero_with_a_zero_limit_beyond_the_limit():
    x, w = _post(16)
    r, full = E.conv_post_tanh(x, w, limit=[0, 5, 100]), E.conv_post_tanh(x, w)
    assert (r.ref[0] == 0).all() and (r.lim[0] == 0).all()
    assert torch.equal(r.ref[1, :5], full.ref[1, :5]) and (r.ref[1, 5:] == 0).all() and (r.lim[1, 5:] == 0).all()
    assert torch.equal(r.ref[2], full.ref[2]) and torch.equal(r.lim[2], full.lim[2])


# ---- the exact mirrors: kernel-style restatements with one fault each, and independent PyTorch formulations ---------------
def _gather_frames(wave, hop, pad, U, f0=0, fault=None):
    """The framing as an index expression (the form the kernels use), for the wrong variants only: the mirror itself builds
    ypad.  ``wave`` carries one extra trailing element that a correct gather never reads (the faulty right reflection does)."""
    n = len(wave) - 1
    out = np.zeros((hop, U), wave.dtype)
    for c in range(hop):
        for u in range(U):
            i = hop * (f0 + u) + c - pad
            beyond = i < -pad or i >= n + pad
            if beyond and fault != "reflect_beyond_pad":
                continue
            if i < 0:
                k = -i - 1 if fault == "left_minus_one" else -i
            elif i >= n:
                k = 2 * n - i if fault == "right_plus_two" else 2 * (n - 1) - i
            else:
                k = i
            if 0 <= k <= n:
                out[c, u] = wave[k]
    return out


def _wave(n, seed=0):
    return np.concatenate([E.rand(n, seed=seed).numpy(), np.float32([12345.0])])


@pytest.mark.parametrize("fault,hop,n", [("left_minus_one", 1, 2), ("right_plus_two", 1, 2), ("reflect_beyond_pad", 3, 37)])
def test_wrong_framing_variants_differ_from_the_mirror(fault, hop, n):
    pad, U = (3 * hop) // 2, 31
    wave = _wave(n)
    ref = E.frame_hops(wave[:n], hop, pad, U)
    assert np.array_equal(_gather_frames(wave, hop, pad, U), ref)
    bad = _gather_frames(wave, hop, pad, U, fault=fault)
    print(f"EXACT wrong framing {fault}: {(bad != ref).sum()} of {ref.size} elements differ")
    assert (bad != ref).any()


def test_wrong_mask_stitch_and_unpad_variants_differ_from_the_mirrors():
    lengths = torch.tensor([-3, 0, 1, 4, 5, 9, 1 << 40])
    ref = E.sequence_mask(lengths, 5)
    assert (ref != (np.arange(5)[None, :] <= lengths.numpy()[:, None]).astype(np.float32)).any()       # <= for <
    # stitch: the source offset from core_lo instead of core_lo - first_frame
    Tw, spf, W = 8, 3, 2
    o_hat = E.rand(W, Tw * spf, seed=1).numpy()
    windows = np.array([[2, 3, 5], [8, 9, 12]])
    out = np.full(16 * spf, np.nan, np.float32)
    ref = E.stitch_window_cores(o_hat, windows, Tw, spf, out)
    bad = out.copy()
    for w, (f0, lo, hi) in enumerate(windows):
        src = o_hat.reshape(-1)[w * Tw * spf + lo * spf:][:(hi - lo) * spf]
        bad[lo * spf:lo * spf + len(src)] = src
    assert not np.array_equal(bad, ref, equal_nan=True)
    assert np.array_equal(ref[3 * spf:5 * spf], o_hat[0, spf:3 * spf]) and np.isnan(ref[:3 * spf]).all()
    # unpad: ld as the destination stride
    rows, T, ld = 3, 5, 8
    src = E.rand(rows * ld, seed=2).numpy()
    ref = E.unpad_rows(src, rows, T, ld)
    bad = np.full(rows * ld, np.nan, np.float32)
    for r in range(rows):
        bad[r * ld:r * ld + T] = src[r * ld:r * ld + T]
    assert not np.array_equal(bad[:rows * T].reshape(rows, T), ref, equal_nan=True)


def _torch_frames(wave, hop, pad, U, f0):
    y = F.pad(wave[None, None], (pad, pad), mode="reflect")[0, 0] if pad else wave
    y = torch.cat([y, torch.zeros(max(0, hop * (f0 + U) - len(y)))])
    return y[hop * f0:hop * (f0 + U)].unfold(0, hop, hop).t()


@pytest.mark.parametrize("seed", range(4))
def test_exact_mirrors_agree_with_independent_pytorch_formulations(seed):
    rng = np.random.default_rng(seed)
    for _ in range(8):
        hop = int(rng.integers(1, 9))
        pad = (3 * hop) // 2
        n = pad + 1 + int(rng.integers(0, 40))
        U, f0 = int(rng.integers(1, 40)), int(rng.integers(0, 12))
        wave = E.rand(n, seed=int(rng.integers(1 << 30)))
        assert np.array_equal(E.frame_hops(wave, hop, pad, U, f0), _torch_frames(wave, hop, pad, U, f0).numpy())
        firsts = [0, f0, f0 + 3]
        assert np.array_equal(E.frame_hops_windows(wave, firsts, hop, pad, U),
                              torch.stack([_torch_frames(wave, hop, pad, U, f) for f in firsts]).numpy())
        # multi: two spans of one pool and the three refused records
        pool = torch.cat([wave, torch.full((3,), float("nan")), wave.flip(0)])
        recs = [[0, n, f0], [n + 3, n, 0], [-1, n, 0], [0, pad, 0], [n + 3, n + 1, 0]]
        got = E.frame_hops_multi(pool, recs, hop, pad, U)
        assert np.array_equal(got[0], _torch_frames(wave, hop, pad, U, f0).numpy())
        assert np.array_equal(got[1], _torch_frames(wave.flip(0), hop, pad, U, 0).numpy())
        assert (got[2:] == 0).all()
        # mask / limits
        T = int(rng.integers(1, 20))
        lengths = torch.tensor(rng.integers(-3, T + 6, size=7).tolist() + [1 << 40])
        assert np.array_equal(E.sequence_mask(lengths, T), (torch.arange(T)[None, :] < lengths[:, None]).float().numpy())
        margin = int(rng.integers(0, 15))
        assert np.array_equal(E.frame_limits(lengths, T, margin),
                              (lengths.clamp_min(0) + margin).clamp_max(T).to(torch.int32).numpy())
        # unpad / stitch by plain slicing
        rows, ld = int(rng.integers(1, 6)), T + int(rng.integers(0, 5))
        src = E.rand(rows * ld, seed=seed + 7)
        assert np.array_equal(E.unpad_rows(src, rows, T, ld), src.view(rows, ld)[:, :T].numpy())
        Tw, spf, F0 = 8, int(rng.integers(1, 6)), int(rng.integers(0, 6))
        o_hat = E.rand(3, Tw * spf, seed=seed + 8)
        windows = [[F0, F0 + 1, F0 + 5], [F0 + 6, F0 + 6, F0 + 14], [F0 + 14, F0 + 15, F0 + 23]]      # the last: hi > f0 + Tw
        out = torch.full((24 * spf,), float("nan"))
        want = out.clone()
        want[spf:5 * spf] = o_hat[0, spf:5 * spf]
        want[6 * spf:14 * spf] = o_hat[1]
        assert np.array_equal(E.stitch_window_cores(o_hat, windows, Tw, spf, out, F0), want.numpy(), equal_nan=True)


def test_every_refusal_of_the_stitch_header_is_a_refusal_of_the_mirror():
    Tw, spf = 8, 2
    o_hat = E.rand(1, Tw * spf, seed=3)
    out = np.full(10 * spf, np.nan, np.float32)
    for rec in ([5, 4, 8], [5, 7, 6], [5, 6, 14], [2, 4, 6], [5, 12, 16]):       # out_frame0 = 5, out_len = 10 frames
        assert np.isnan(E.stitch_window_cores(o_hat, [rec], Tw, spf, out, 5)).all(), rec
    assert np.isnan(E.stitch_window_cores(o_hat, [[5, 7, 7]], Tw, spf, out, 5)).all()             # empty core
    assert (~np.isnan(E.stitch_window_cores(o_hat, [[7, 7, 15]], Tw, spf, out, 5))).sum() == 8 * spf   # ends at out_len


# ---- the constants ------------------------------------------------------------------------------------------------------------
def test_constants_are_four_times_the_measured_maxima():
    """T_TANH is re-measured in full (a fraction of a second); S_POST and S_LIN on the shapes that set them (the whole
    tables take a few seconds: ``python -m oracle.edge_ref``).  All are quoted in the module docstring and in DESIGN.md."""
    t = max(E.measure_t_tanh().values())
    assert abs(4 * t - E.T_TANH) <= 0.001 * E.T_TANH, (t, E.T_TANH)
    sp = max(q for q, _ in E.measure_s_post(shapes=(E.S_POST_SET_BY,)).values())
    assert abs(4 * sp - E.S_POST) <= 0.001 * E.S_POST, (sp, E.S_POST)
    sl = max(E.measure_s_lin(shapes=(E.S_LIN_SET_BY,)).values())
    assert abs(4 * sl - E.S_LIN) <= 0.001 * E.S_LIN, (sl, E.S_LIN)
    assert E.S_POST_SET_BY in E.POST_SHAPES and E.S_LIN_SET_BY in E.LIN_SHAPES
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for text in ("4.113e-07", "1.645e-06", "1.054", "4.216", "7.558e-08", "3.023e-07"):
        assert E.__doc__.count(text) and design.count(text), text
