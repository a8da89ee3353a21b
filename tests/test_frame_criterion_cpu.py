"""The element-wise fp32 criterion of the frame-rate kernels (oracle/fp32_ref.py: S32 * absacc + N against a float64
mirror) can tell right from wrong -- on the CPU, reference against reference, no kernel involved.

Honest stand-in: the same mirror with ``dtype=torch.float32`` (PyTorch's fp32 conv in its own summation order, libm
tanh / sigmoid / exp or the fp32 restatement of ``wn_gate``) lands at err / lim <= 1 on every element, at every shape
of tests/test_gpu_frame_kernels.py, benign and stress data.  The worst ratio per kernel is printed.

Every deliberately wrong variant exceeds the limit on at least one element at the smallest T of the suite at which the
fault exists (T = 1 where a single column shows it; T = 2 where it needs a neighbour column or a masked column):
  dropped_tap (T = 1), rows_swapped (1), mask_h_only (2), skip_assign (1), couple_sign (1), flip_off_by_one (1),
  neighbour_logs (1), phase_rotated (1), halo_zero (2).

The instance list of the GPU file stays current: the X(...) lines of conv1d_inst_s.hip, conv1d_inst_w.hip and the grouped
ConvTranspose lines of conv1d_inst_f.hip are parsed and compared with its ``INSTANCES``."""
import importlib.util
import os
import re

import pytest
import torch

from oracle import fp32_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
H = R.H


def _report(what, w):
    print(f"RATIO {what} {w:.3f}")
    return w


@pytest.mark.parametrize("T", R.T_EDGES)
def test_honest_fp32_stand_ins_are_accepted(T):
    worst = {}

    def note(name, got, ref):
        worst[name] = max(worst.get(name, 0.0), R.worst(got, ref))

    for K in R.LINEAR_SHAPES:
        o = R.linear_operands(K, T)
        for kw in (dict(in_slope=0.1, bias_b=o["bias_b"], res=o["res"], add=o["add"], scale=1 / 3),
                   dict(res=o["res"], scale=0.5, mask=o["mask"]), dict()):
            note(f"linear_k{K}", R.linear(o["x"], o["w"], o["bias"], dtype=F32, **kw).ref,
                 R.linear(o["x"], o["w"], o["bias"], **kw))
    for stress in (False, True):
        for first, last in ((False, False), (True, False), (False, True)):
            o = R.wn_operands(T, stress=stress, last=last)
            args = (o["x"], o["g"], o["mask"], o["skip"], o["w_in"], o["b_in"], o["w_rs"], o["b_rs"], first, last)
            refs = R.wn_layer(*args)
            for formula in ("hw", "libm"):
                got = R.wn_layer(*args, dtype=F32, formula=formula)
                tag = "_stress" if stress else ""
                note(f"gate{tag}_{formula}", got[0].ref, refs[0])
                assert torch.isfinite(got[0].ref).all()
                if not last:
                    note(f"wn_layer{tag}_h", got[1].ref, refs[1])
                note(f"wn_layer{tag}_skip", got[2].ref, refs[2])
        # RESSKIP on exact inputs (N = 0): the float64 gate rounded to fp32 is the operand of both
        o = R.wn_operands(T, stress=stress)
        acts = R.gate(o["x"], o["w_in"], o["b_in"], o["g"]).ref.float()
        for first, split in ((False, H), (True, H), (False, 0)):
            w_rs, b_rs = (o["w_rs"][H:], o["b_rs"][H:]) if split == 0 else (o["w_rs"], o["b_rs"])
            a = (acts, w_rs, b_rs, o["x"], o["skip"], o["mask"], split, first)
            for got, ref in zip(R.res_skip(*a, dtype=F32), R.res_skip(*a)):
                if ref is not None:
                    note("res_skip", got.ref, ref)
        p = R.posterior_operands(T, stress=stress)
        for tau in R.TAUS:
            a = (p["h"], p["w"], p["b"], p["noise"], tau, p["mask"])
            got = R.posterior(*a, dtype=F32).ref
            assert torch.isfinite(got).all()
            note("posterior_stress" if stress else "posterior", got, R.posterior(*a))
    c = R.couple_operands(T)
    for reverse in (False, True):
        for flipped in (False, True):
            a = (c["h"], c["w"], c["b"], c["x"], c["mask"], reverse, flipped)
            note("couple", R.couple(*a, dtype=F32).ref, R.couple(*a))
    for s in R.CONVT_SHAPES:
        o = R.convt_operands(s, T)
        a = (o["x"], o["w"], o["b"], s, 0.1)
        note(f"convt_s{s}", R.conv_transpose(*a, dtype=F32).ref, R.conv_transpose(*a))
    hops = R.magnitude_operands(T)["hops"]
    note("magnitude", R.magnitude(hops, R.MAG_NFFT, R.MAG_HOP, 1e-6, dtype=F32)[0].ref,
         R.magnitude(hops, R.MAG_NFFT, R.MAG_HOP, 1e-6)[0])
    for name, w in worst.items():
        _report(f"stand-in T={T} {name}", w)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


# ---- wrong variants: fp32 restatements with one fault each ----------------------------------------------------------------
def _wrong_dropped_tap(T):
    o = R.linear_operands(5, T)
    w = o["w"].clone()
    w[:, :, 2] = 0                                    # the centre tap: the only one a single column has
    return R.linear(o["x"], w, o["bias"], dtype=F32).ref, R.linear(o["x"], o["w"], o["bias"])


def _wrong_halo_zero(T):
    o = R.linear_operands(5, T)
    good = R.linear(o["x"], o["w"], o["bias"], dtype=F32).ref
    # column 1 reads column 0 through tap 1 (the left halo of a tile that starts at column 1): read as zero
    bad = good.clone()
    bad[:, :, 1] -= torch.einsum("oc,bc->bo", o["w"][:, :, 1], o["x"][:, :, 0])
    return bad, R.linear(o["x"], o["w"], o["bias"])


def _wn(T):
    o = R.wn_operands(T)
    return o, R.wn_layer(o["x"], o["g"], o["mask"], o["skip"], o["w_in"], o["b_in"], o["w_rs"], o["b_rs"])


def _wrong_rows_swapped(T):
    o, refs = _wn(T)
    w, b, g = o["w_in"].clone(), o["b_in"].clone(), o["g"].clone()
    c = 5
    w[[c, H + c]], b[[c, H + c]], g[:, [c, H + c]] = w[[H + c, c]], b[[H + c, c]], g[:, [H + c, c]]
    return R.gate(o["x"], w, b, g, dtype=F32).ref, refs[0]


def _rs32(o):
    acts = R.gate(o["x"], o["w_in"], o["b_in"], o["g"], dtype=F32).ref
    return R._affine(acts, o["w_rs"], o["b_rs"], dtype=F32)[0]


def _wrong_mask_h_only(T):
    o, refs = _wn(T)
    return o["x"] * o["mask"][:, None] + _rs32(o)[:, :H], refs[1]


def _wrong_skip_assign(T):
    o, refs = _wn(T)
    return _rs32(o)[:, H:], refs[2]


def _wrong_couple_sign(T):
    c = R.couple_operands(T)
    good = R.couple(c["h"], c["w"], c["b"], c["x"], c["mask"], True, False, dtype=F32).ref
    fwd = R.couple(c["h"], c["w"], c["b"], c["x"], c["mask"], False, False, dtype=F32).ref
    bad = good.clone()
    bad[:, H // 2:H // 2 + H // 4] = fwd[:, H // 2:H // 2 + H // 4]      # (m + x1) on one half of the x1 rows
    return bad, R.couple(c["h"], c["w"], c["b"], c["x"], c["mask"], True, False)


def _wrong_flip_off_by_one(T):
    c = R.couple_operands(T)
    good = R.couple(c["h"], c["w"], c["b"], c["x"], c["mask"], False, True, dtype=F32).ref
    bad = good.clone()
    bad[:, :H // 2] = torch.roll(good[:, :H // 2], 1, 1)               # the flipped x1 rows, one channel off
    return bad, R.couple(c["h"], c["w"], c["b"], c["x"], c["mask"], False, True)


def _wrong_neighbour_logs(T):
    p = R.posterior_operands(T)
    w, b = p["w"].clone(), p["b"].clone()
    w[H:], b[H:] = torch.roll(p["w"][H:], 1, 0), torch.roll(p["b"][H:], 1, 0)
    return R.posterior(p["h"], w, b, p["noise"], 1.0, p["mask"], dtype=F32).ref, \
        R.posterior(p["h"], p["w"], p["b"], p["noise"], 1.0, p["mask"])


def _wrong_phase_rotated(T):
    o = R.convt_operands(8, T)
    good = R.conv_transpose(o["x"], o["w"], o["b"], 8, 0.1, dtype=F32).ref
    Bn, C, L = good.shape
    return torch.roll(good.view(Bn, C, L // 8, 8), 1, 3).reshape(Bn, C, L), R.conv_transpose(o["x"], o["w"], o["b"], 8, 0.1)


WRONG = [("dropped_tap", _wrong_dropped_tap, 1), ("rows_swapped", _wrong_rows_swapped, 1),
         ("mask_h_only", _wrong_mask_h_only, 2), ("skip_assign", _wrong_skip_assign, 1),
         ("couple_sign", _wrong_couple_sign, 1), ("flip_off_by_one", _wrong_flip_off_by_one, 1),
         ("neighbour_logs", _wrong_neighbour_logs, 1), ("phase_rotated", _wrong_phase_rotated, 1),
         ("halo_zero", _wrong_halo_zero, 2)]


@pytest.mark.parametrize("name,fn,T", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_variants_are_rejected(name, fn, T):
    got, ref = fn(T)
    q = R.ratio(got, ref)
    w = _report(f"wrong {name} T={T}", q.max().item())
    assert w > 1.0
    print(f"      elements over the limit: {(q > 1).sum().item()} of {q.numel()}")


def test_ratio_counts_nan_inf_and_inexact_zero_limits():
    ref = R.Ref(torch.tensor([1.0, 0.0, 2.0], dtype=F64), None, torch.tensor([1e-6, 0.0, 1e-6], dtype=F64))
    assert R.worst(torch.tensor([1.0, 0.0, 2.0]), ref) == 0.0
    assert R.worst(torch.tensor([1.0, 1e-30, 2.0]), ref) == float("inf")        # lim = 0: exact or wrong
    assert R.worst(torch.tensor([float("nan"), 0.0, 2.0]), ref) == float("inf")
    assert R.worst(torch.tensor([1.0, 0.0, float("inf")]), ref) == float("inf")


def test_constants_are_four_times_the_measured_maxima():
    """G is re-measured here (a fraction of a second); S32's table takes ten seconds (``python -m oracle.fp32_ref``) and is
    re-measured on the two shapes that set it.  Both are quoted in the module docstring and in DESIGN.md."""
    g = max(R.measure_g().values())
    assert abs(4 * g - R.G) <= 0.01 * R.G, (g, R.G)
    s = max(R.measure_s32(seeds=range(5), ts=(1, 129)).values())
    assert 4 * s <= R.S32 * 1.0001 and 4 * s >= 0.25 * R.S32, (s, R.S32)
    doc = R.__doc__ + open(os.path.join(REPO, "DESIGN.md")).read()
    for text in ("6.531e-07", "2.612e-06", "3.377", "13.508"):
        assert R.__doc__.count(text) and doc.count(text) >= 2, text


# ---- the instance list ------------------------------------------------------------------------------------------------------
def _parse(name, keep=None):
    src = open(os.path.join(REPO, "openvoice_amd", "csrc", name)).read()
    rows = re.findall(r"X\((\d+), (\d+), (\w+), (\d+), (\d+), (\w+), (\d+)\)", src)
    assert rows, name
    out = [(int(k), int(d), tile, int(ch), int(v), epi, int(nld)) for k, d, tile, ch, v, epi, nld in rows]
    return [r for r in out if keep is None or r[5] in keep]


def test_gpu_file_names_exactly_the_instantiated_kernels():
    spec = importlib.util.spec_from_file_location("frame_gpu", os.path.join(REPO, "tests", "test_gpu_frame_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = _parse("conv1d_inst_w.hip") + _parse("conv1d_inst_s.hip") + \
        _parse("conv1d_inst_f.hip", keep=("EPI_CONVT_S8", "EPI_CONVT_S2"))
    assert len(set(want)) == len(want) == 35
    assert sorted(mod.INSTANCES) == sorted(want)
    # every instance is reachable by the test that walks them: a tile id, a layout per staging kind, a runner per epilogue
    for inst in mod.INSTANCES:
        assert inst[2] in mod.TILE_ID and inst[4] in mod.LAYOUTS_OF_VEC
        assert inst[5] in ("OV_EPI_LINEAR", "OV_EPI_GATE", "OV_EPI_RESSKIP", "OV_EPI_COUPLE", "OV_EPI_POSTERIOR",
                           "OV_EPI_CONVT", "EPI_CONVT_S8", "EPI_CONVT_S2", "OV_EPI_MAGNITUDE")
        if inst[5] == "OV_EPI_LINEAR":
            assert inst[0] in R.LINEAR_SHAPES
