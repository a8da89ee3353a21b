"""The element-wise criteria of the sample-rate ResBlock (MRF) kernels (oracle/fp32_ref.py: ``mrf_linear`` S32_MRF * absacc,
``pair`` with the fp32 storage of h, ``wino_linear`` S_W * absacc_w) can tell right from wrong -- on the CPU, reference
against reference, no kernel involved.

Honest stand-ins land at err / lim <= 1 on every element at every shape tests/test_gpu_mrf_kernels.py runs, benign and
stress data: PyTorch's fp32 conv for the direct instances, the fp32 Winograd restatement ``wino_conv``, and fp32 conv ->
fp32 store -> fp32 conv for the pair.  The worst ratio per kernel is printed.

Every deliberately wrong variant exceeds its limit on at least one element at the smallest L at which the fault exists:
  dilated_tap_dropped (L = 6: k = 3, dilation 5 -- column 0 reads column 5), tile_halo_zero (129: the column that starts the
  second 128-column tile), res_after_scale (1), add_not_scaled (1), slope_on_res (1), quiet_channel_dropped (1),
  pair_h_halo_computed (1), pair_second_slope_missing (1), wino_point_dropped (4: output 3 of a tile is the only one that
  reads point infinity), wino_ragged_tile_shifted (2: a partial tile of two columns).
``quiet_channel_dropped`` is shown to PASS the old bar (max|err| <= 2e-5 max|ref|) and fail the new one.

The instance lists of the GPU file stay current: the OV_EPI_LINEAR X(...) lines of conv1d_inst_a.hip .. conv1d_inst_f.hip and
the answers of ov_conv1d_wino_supported / ov_resblock_pair_supported are compared with its lists."""
import importlib.util
import os
import re

import pytest
import torch

from oracle import fp32_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


def _gpu_module():
    spec = importlib.util.spec_from_file_location("mrf_gpu", os.path.join(REPO, "tests", "test_gpu_mrf_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GPU = _gpu_module()


def _report(what, w):
    print(f"RATIO {what} {w:.3f}")
    return w


# ---- honest stand-ins ---------------------------------------------------------------------------------------------------------
def _direct_forms(o):
    return (dict(), dict(res=o["res"]), dict(res=o["res"], add=o["add"], scale=1 / 3))


@pytest.mark.parametrize("K,dil", R.MRF_KD)
def test_honest_fp32_conv_is_accepted_for_the_direct_instances(K, dil):
    """Every (C, L) the GPU file runs: the tile's smallest channel count at the tile's lengths, and C = 256 at N = 128."""
    cases = {(c, L) for _, n, c in GPU.TILES.values() for L in GPU.direct_lengths(n)} | {(256, L) for L in GPU.direct_lengths(128)}
    worst = 0.0
    for C, L in sorted(cases):
        for stress in (False, True):
            o = R.mrf_operands(C, K, dil, L, stress=stress)
            for kw in _direct_forms(o):
                a = (o["x"], o["w"], o["bias"])
                worst = max(worst, R.worst(R.mrf_linear(*a, dil=dil, dtype=F32, **kw).ref, R.mrf_linear(*a, dil=dil, **kw)))
    assert _report(f"stand-in direct k={K} d={dil}", worst) <= 1.0


@pytest.mark.parametrize("C,K,dil", GPU.PAIR_SHAPES, ids=str)
def test_honest_fp32_pair_is_accepted(C, K, dil):
    worst = 0.0
    for L in R.PAIR_LS:
        for stress in (False, True):
            o = R.mrf_operands(C, K, dil, L, stress=stress)
            a = (o["x"], o["w"], o["bias"], o["w2"], o["b2"], K, dil)
            for kw in (dict(), dict(add=o["add"], scale=1 / 3)):
                worst = max(worst, R.worst(R.pair(*a, dtype=F32, **kw).ref, R.pair(*a, **kw)))
    assert _report(f"stand-in pair C={C} k={K} d={dil}", worst) <= 1.0


@pytest.mark.parametrize("C,K,dil", GPU.WINO_SHAPES, ids=str)
def test_honest_fp32_winograd_restatement_is_accepted(C, K, dil):
    worst = 0.0
    for L in R.WINO_LS:
        for stress in (False, True):
            o = R.mrf_operands(C, K, dil, L, stress=stress)
            for in_slope, out_slope, has_res, has_add, scale in GPU.WINO_FORMS.values():
                kw = dict(dil=dil, in_slope=in_slope, out_slope=out_slope, res=o["res"] if has_res else None,
                          add=o["add"] if has_add else None, scale=scale)
                a = (o["x"], o["w"], o["bias"], K)
                worst = max(worst, R.worst(R.wino_linear(*a, dtype=F32, **kw).ref, R.wino_linear(*a, **kw)))
    assert _report(f"stand-in wino C={C} k={K} d={dil}", worst) <= 1.0


def test_zero_rows_come_back_as_exactly_res_plus_add():
    """An all-zero weight row with a zero bias: the limit is the explicit one (two roundings of (res + add) * scale), zero
    without res and add, and a stand-in that is off by one part in 1e6 there is rejected."""
    o = R.mrf_operands(32, 3, 1, 8, stress=True)
    a = (o["x"], o["w"], o["bias"])
    plain = R.mrf_linear(*a)
    assert (plain.lim[:, 3::4] == 0).all() and (plain.ref[:, 3::4] == 0).all()
    ref = R.mrf_linear(*a, res=o["res"], add=o["add"], scale=1 / 3)
    z = ref.lim[:, 3::4]
    want = (o["res"].double().abs() + o["add"].double().abs())[:, 3::4] * (2 * R.EPS * (1 + R.EPS) * abs(R.f32(1 / 3)))
    assert torch.equal(z, want)
    good = R.mrf_linear(*a, res=o["res"], add=o["add"], scale=1 / 3, dtype=F32).ref
    assert R.worst(good, ref) <= 1.0
    bad = good.clone()
    bad[:, 3::4] *= 1 + 1e-6
    assert R.worst(bad, ref) > 1.0


# ---- wrong variants: fp32 restatements with one fault each --------------------------------------------------------------------
def _conv32(x, w, bias, dil, slope=0.1):
    return R._affine(x, w, bias, dil=dil, in_slope=slope, dtype=F32)[0]


def _wrong_dilated_tap_dropped(L):
    o = R.mrf_operands(32, 3, 5, L)
    w = o["w"].clone()
    w[:, :, -1] = 0                                   # the outermost tap at + dil (K - 1) / 2
    return _conv32(o["x"], w, o["bias"], 5), R.mrf_linear(o["x"], o["w"], o["bias"], dil=5)


def _wrong_tile_halo_zero(L):
    K, dil, t0 = 7, 3, 128
    o = R.mrf_operands(32, K, dil, L)
    bad = _conv32(o["x"], o["w"], o["bias"], dil)
    xa = R._lrelu(o["x"], 0.1)
    for j in range((K - 1) // 2):                     # column t0 reads t0 - 9, t0 - 6, t0 - 3 from its left neighbour: as zero
        bad[:, :, t0] -= torch.einsum("oc,bc->bo", o["w"][:, :, j], xa[:, :, t0 + (j - (K - 1) // 2) * dil])
    return bad, R.mrf_linear(o["x"], o["w"], o["bias"], dil=dil)


def _mrf(L):
    o = R.mrf_operands(32, 3, 1, L)
    return o, _conv32(o["x"], o["w"], o["bias"], 1), R.mrf_linear(o["x"], o["w"], o["bias"], res=o["res"], add=o["add"], scale=1 / 3)


def _wrong_res_after_scale(L):
    o, c, ref = _mrf(L)
    return (c + o["add"]) * R.f32(1 / 3) + o["res"], ref


def _wrong_add_not_scaled(L):
    o, c, ref = _mrf(L)
    return (c + o["res"]) * R.f32(1 / 3) + o["add"], ref


def _wrong_slope_on_res(L):
    o, c, ref = _mrf(L)
    return (c + R._lrelu(o["res"], 0.1) + o["add"]) * R.f32(1 / 3), ref


def _wrong_quiet_channel_dropped(L):
    o = R.mrf_operands(32, 3, 1, L, stress=True)
    x = o["x"].clone()
    x[:, 1::8] = 0                                    # the x 1e-3 input channels are ignored
    return _conv32(x, o["w"], o["bias"], 1), R.mrf_linear(o["x"], o["w"], o["bias"])


def _pair_ops(L):
    o = R.mrf_operands(32, 3, 3, L)
    return o, R.pair(o["x"], o["w"], o["bias"], o["w2"], o["b2"], 3, 3)


def _wrong_pair_h_halo_computed(L):
    o, ref = _pair_ops(L)
    p2 = 1
    xp = torch.nn.functional.pad(o["x"], (p2, p2))    # h at columns -1 and L from zero-padded x: b1 + the taps that reach x
    h = _conv32(xp, o["w"], o["bias"], 3)
    y = torch.nn.functional.conv1d(R._lrelu(h, 0.1), o["w2"], o["b2"])
    return y + o["x"], ref


def _wrong_pair_second_slope_missing(L):
    o, ref = _pair_ops(L)
    h = _conv32(o["x"], o["w"], o["bias"], 3)
    return R._conv(h, o["w2"]) + o["b2"][None, :, None] + o["x"], ref


def _wrong_wino_point_dropped(L):
    o = R.mrf_operands(64, 3, 1, L)
    u = R.wino_u(o["w"], 3)
    u[:, :, -1, 5] = 0                                # point infinity of the last tap group: a real product for K = 3
    return R.wino_conv(o["x"], o["w"], o["bias"], 3, 1, 0.1, u=u), R.wino_linear(o["x"], o["w"], o["bias"], 3)


def _wrong_wino_ragged_tile_shifted(L):
    o = R.mrf_operands(64, 3, 1, L)
    good = R.wino_conv(o["x"], o["w"], o["bias"], 3, 1, 0.1)
    start = (L - 1) // 4 * 4
    bad = good.clone()
    bad[:, :, start + 1:] = good[:, :, start:L - 1]   # the last partial tile lands one column late (its first column kept)
    return bad, R.wino_linear(o["x"], o["w"], o["bias"], 3)


WRONG = [("dilated_tap_dropped", _wrong_dilated_tap_dropped, 6), ("tile_halo_zero", _wrong_tile_halo_zero, 129),
         ("res_after_scale", _wrong_res_after_scale, 1), ("add_not_scaled", _wrong_add_not_scaled, 1),
         ("slope_on_res", _wrong_slope_on_res, 1), ("quiet_channel_dropped", _wrong_quiet_channel_dropped, 1),
         ("pair_h_halo_computed", _wrong_pair_h_halo_computed, 1),
         ("pair_second_slope_missing", _wrong_pair_second_slope_missing, 1),
         ("wino_point_dropped", _wrong_wino_point_dropped, 4), ("wino_ragged_tile_shifted", _wrong_wino_ragged_tile_shifted, 2)]


@pytest.mark.parametrize("name,fn,L", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_variants_are_rejected(name, fn, L):
    got, ref = fn(L)
    q = R.ratio(got, ref)
    w = _report(f"wrong {name} L={L}", q.max().item())
    assert w > 1.0
    print(f"      elements over the limit: {(q > 1).sum().item()} of {q.numel()}")


def test_quiet_channel_dropped_passes_the_old_bar_and_fails_the_new_one():
    """The point of the element-wise criterion, on the stress data: the x 1e3 channels and the 1e3 transients set max|ref|
    for the whole tensor, so the old norm-wise bar accepts a conv that ignores every x 1e-3 input channel; the element-wise
    limit rejects it (at the columns and rows where the loud terms happen to be small)."""
    for L in (1, 260):
        got, ref = _wrong_quiet_channel_dropped(L)
        err = (got.double() - ref.ref).abs().max().item()
        old = 2e-5 * max(ref.ref.abs().max().item(), 1.0)
        new = R.worst(got, ref)
        print(f"quiet_channel_dropped L={L}: max|err| {err:.3e}, old bar {old:.3e} -> {'accepted' if err <= old else 'rejected'};"
              f" RATIO new {new:.3f}")
        assert err <= old, "the old bar was expected to accept this fault"
        assert new > 1.0


# ---- the lists of the GPU file ----------------------------------------------------------------------------------------------------
def _parse(name):
    src = open(os.path.join(REPO, "openvoice_amd", "csrc", name)).read()
    rows = re.findall(r"X\((\d+), (\d+), (\w+), (\d+), (\d+), (\w+), (\d+)\)", src)
    assert rows, name
    return [(int(k), int(d), tile, int(ch), int(v), epi, int(nld)) for k, d, tile, ch, v, epi, nld in rows if epi == "OV_EPI_LINEAR"]


def test_gpu_file_names_exactly_the_instantiated_direct_kernels():
    want = sum((_parse(f"conv1d_inst_{c}.hip") for c in "abcdef"), [])
    assert len(set(want)) == len(want) == 63
    assert sorted(GPU.MRF_INSTANCES) == sorted(want)
    for inst in GPU.MRF_INSTANCES:
        assert inst[2] in GPU.TILES and inst[4] == 1 and (inst[0], inst[1]) in R.MRF_KD


def test_gpu_file_names_exactly_the_supported_winograd_and_pair_shapes():
    from openvoice_amd import _lib, wino
    lib = _lib.load()
    grid = [(c, k, d) for c in (32, 64, 96, 128, 256) for k in (3, 7, 11) for d in (1, 3, 5)]
    assert sorted(GPU.WINO_SHAPES) == [s for s in grid if lib.ov_conv1d_wino_supported(s[0], s[0], s[1], s[2])]
    assert sorted(GPU.PAIR_SHAPES) == [s for s in grid if lib.ov_resblock_pair_supported(*s)]
    # the oracle restates the F(4, 3) matrices so that it loads without the library: the copies are equal
    assert (R.WINO_BT, R.WINO_G, R.WINO_AT, R.WINO_LEAD_TAPS) == (wino.BT, wino.G, wino.AT, wino.LEAD_TAPS)


def test_winograd_restatement_is_the_conv_in_float64():
    """``wino_conv`` in float64 equals the float64 conv up to the fp32 rounding of U (2^-24 of absacc_w), at every tile
    alignment, ragged lengths and every dilation; absacc_w is never below absacc."""
    for K, dil, L in ((3, 1, 7), (7, 3, 50), (11, 5, 131)):
        o = R.mrf_operands(32, K, dil, L, stress=True)
        v, a = R._affine(o["x"], o["w"], o["bias"], dil=dil, in_slope=0.1)
        aw = R.wino_absacc(o["x"], o["w"], o["bias"], K, dil, 0.1)
        assert (aw >= a * (1 - 1e-6)).all()
        for al in range(4):
            got = R.wino_conv(o["x"], o["w"], o["bias"], K, dil, 0.1, dtype=F64, aligns=(al,))
            assert ((got - v).abs() <= R.EPS * aw).all(), (K, dil, al)


def test_constants_are_four_times_the_measured_maxima():
    """S32_MRF and S_W re-measured on the shapes that set them (``python -m oracle.fp32_ref`` prints the whole table, a few
    minutes); both are quoted in the module docstring and in DESIGN.md."""
    d = max(v[0] for v in R.measure_mrf(cs=R.S32_MRF_SET_BY[:1], kds=(R.S32_MRF_SET_BY[1:],)).values())
    assert abs(4 * d - R.S32_MRF) <= 0.01 * R.S32_MRF, (d, R.S32_MRF)
    assert d > 6.531e-07, "the MRF maximum is above the frame-rate table's: hence an allowance of its own"
    w = max(v[1] for v in R.measure_mrf(cs=R.S_W_SET_BY[:1], kds=(R.S_W_SET_BY[1:],)).values())
    assert abs(4 * w - R.S_W) <= 0.01 * R.S_W, (w, R.S_W)
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    for text in ("7.056e-07", "2.822e-06", "3.030e-07", "1.212e-06"):
        assert text in R.__doc__ and text in design, text
