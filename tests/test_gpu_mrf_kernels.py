"""The sample-rate ResBlock (MRF) fp32 conv kernels, one by one against float64 (oracle/fp32_ref.py), element by element:
|out - ref64| <= lim on every element, no norm-wise bound and nothing left out.

Kernels and their limits:
* the 63 direct MFMA OV_EPI_LINEAR instances of conv1d_inst_a.hip .. conv1d_inst_f.hip (``MRF_INSTANCES``; k = 3 / 7 / 11,
  dilation 1 / 3 / 5, four tile shapes, two chunk sizes, two loader counts), each with tile, chunk and loader count FORCED
  (an exact match or OV_E_UNSUPPORTED): ``R.mrf_linear``, lim = S32_MRF * absacc;
* the fused ResBlock pair ``ov_resblock_pair_f32`` (``PAIR_SHAPES``): ``R.pair``, whose limit carries the fp32 storage of h
  through |w2|; bit-identical to the two direct launches it replaces;
* the Winograd-domain conv ``ov_conv1d_wino_f32`` (``WINO_SHAPES``) and the three-conv launch ``ov_conv1d_wino_multi_f32``:
  ``R.wino_linear``, lim = S_W * absacc_w with absacc_w taken in the transform domain.  The direct kernel's ratio on the same
  operands is printed beside it; neither is asserted against the other.
tests/test_mrf_criterion_cpu.py keeps the three lists equal to the sources and proves that the limits tell right from wrong.

Layout: every tensor sits inside a larger NaN-filled buffer (oracle/nanbuf.py) at a nonzero offset, rows padded (ld > L,
ld % 4 == 0: these instances all use 16-byte staging), batch strides larger than C * ld; everything outside the valid
[B, C, :L] block must still be NaN afterwards.  (``launch_convs_wino`` has no row stride: dense rows there, the offset and
the batch stride as elsewhere.)
Data: ``R.mrf_operands``, benign and stress (channels x 1e3, x 1e-3, exactly zero, all negative, a 1e-3 row with a 1e3
transient in the middle and at the last column; weight rows x 1, x 1e-2, x 1e2 and exactly zero).

Each test prints ``RATIO <what> <worst err / lim>`` before it asserts.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, wino  # noqa: E402
from openvoice_amd.engine import PackedConv, launch_conv, launch_pair, wino_ncol  # noqa: E402
from oracle import fp32_ref as R  # noqa: E402
from oracle.nanbuf import DEV, NAN, Buf  # noqa: E402

B = R.B
# tile name -> (ov_conv1d_params.tile, columns per tile N, smallest channel count that fills the tile's rows)
TILES = {"128x128": (1, 128, 128), "64x256": (2, 256, 64), "32x512": (3, 512, 32), "32x256": (4, 256, 32)}
# (K, dil, tile, chunk, vec, epilogue, loader waves): the OV_EPI_LINEAR X(...) lines of conv1d_inst_a.hip .. conv1d_inst_f.hip
MRF_INSTANCES = [(k, d, tile, chunk, 1, "OV_EPI_LINEAR", nld)
                 for tile, chunk, nld in (("128x128", 32, 2), ("128x128", 16, 2), ("128x128", 32, 4), ("64x256", 32, 4),
                                          ("64x256", 16, 4), ("32x512", 16, 4), ("32x256", 16, 4))
                 for k, d in R.MRF_KD]
# (C, K, dil) with ov_resblock_pair_supported / ov_conv1d_wino_supported, C in {32, 64, 96, 128, 256}
PAIR_SHAPES = [(c, k, d) for c, ks in ((32, (3, 7, 11)), (64, (3, 7))) for k in ks for d in (1, 3, 5)]
WINO_SHAPES = [(c, k, d) for c, ks in ((32, (11,)), (64, (3, 7, 11)), (96, (11,)), (128, (3, 7, 11)), (256, (3, 7, 11)))
               for k in ks for d in (1, 3, 5)]


def direct_lengths(N):
    """4 is shorter than every receptive field; N - 4 / N / N + 4 / 2 N + 4 straddle one and two tile boundaries with a
    dilated halo of up to 25 columns."""
    return (4, N - 4, N, N + 4, 2 * N + 4)


def _inst_id(inst):
    return "k{}-d{}-{}-c{}-l{}".format(inst[0], inst[1], inst[2], inst[3], inst[6])


def _report(what, w):
    print(f"RATIO {what} {w:.3f}")
    assert w <= 1.0, f"{what}: worst err / lim = {w:.3f}"


# ---- cached operands, float64 cores and packed layers ------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _case(C, K, dil, L, stress, in_slope=0.1):
    """Operands + the float64 conv and absacc every operand form of this (x, w) shares."""
    o = R.mrf_operands(C, K, dil, L, stress=stress)
    return o, R._affine(o["x"], o["w"], o["bias"], dil=dil, in_slope=in_slope)


@functools.lru_cache(maxsize=64)
def _wino_core(C, K, dil, L, stress, in_slope):
    o, (v, _) = _case(C, K, dil, L, stress, in_slope)
    return v, R.wino_absacc(o["x"], o["w"], o["bias"], K, dil, in_slope)


@functools.lru_cache(maxsize=None)
def _direct_layer(C, K, dil, stress, second=False):
    o = R.mrf_operands(C, K, dil, 4, stress=stress)               # (the weights do not depend on L)
    return PackedConv(o["w2" if second else "w"], o["b2" if second else "bias"], DEV, K=K, dil=1 if second else dil)


@functools.lru_cache(maxsize=None)
def _wino_layer(C, K, dil, stress):
    o = R.mrf_operands(C, K, dil, 4, stress=stress)
    return wino.PackedConvWino(o["w"], o["bias"], DEV, dil=dil)


def _nan_like(t):
    return torch.full_like(t, NAN)


def _direct(layer, x, out, L, res=None, add=None, in_slope=0.1, **kw):
    """launch_conv on ``Buf``s: offsets, row strides and batch strides from them; ``add`` may be ``out`` itself."""
    if res is not None:
        kw.update(res=res.flat, res_off=res.off, res_bs=res.bs)
    if add is not None:
        kw.update(add=add.tail(), add_bs=add.bs)
    launch_conv(layer, x.flat, x.off, x.bs, out.flat, out.off, out.bs, B, L, in_slope=in_slope, x_ld=x.ld, out_ld=out.ld, **kw)


# ---- 1. the direct instances ---------------------------------------------------------------------------------------------------
def run_direct(inst, C, what):
    K, dil, tile, chunk, _, _, nld = inst
    tid, N, _ = TILES[tile]
    knobs = dict(tile=tid, chunk=chunk, loaders=nld)
    worst = 0.0
    for L in direct_lengths(N):
        for tpw in (0, 2) if L > N else (0,):
            kn = dict(knobs, tiles_per_wg=tpw)
            for form, stress in (("a", True), ("b", False), ("c", True), ("d", False)):
                o, core = _case(C, K, dil, L, stress)
                layer = _direct_layer(C, K, dil, stress)
                x = Buf(o["x"], "vec")
                args = (o["x"], o["w"], o["bias"])
                if form in ("a", "d"):                       # in_slope = 0.1, bias only; (d) under a column limit
                    ref = R.mrf_linear(*args, dil=dil, core=core)
                    out = Buf(_nan_like(o["res"]))
                    if form == "a":
                        _direct(layer, x, out, L, **kn)
                        got = out.get()
                    else:
                        limits = [L, 0, L // 2]
                        _direct(layer, x, out, L, col_limit=torch.tensor(limits, dtype=torch.int32, device=DEV),
                                col_limit_scale=1, **kn)
                        got = out.get()
                        for b, lim in enumerate(limits):      # whole tiles that start before the limit; NaN beyond
                            done = min(L, -(-lim // N) * N)
                            assert torch.isnan(got[b, :, done:]).all(), f"{what} L={L}: utterance {b} written beyond column {done}"
                            assert torch.isfinite(got[b, :, :done]).all(), f"{what} L={L}: utterance {b} not computed up to {done}"
                            got[b, :, done:] = ref.ref[b, :, done:].float()
                            ref.lim[b, :, done:] = float("inf")
                elif form == "b":                            # + res
                    ref = R.mrf_linear(*args, dil=dil, res=o["res"], core=core)
                    out = Buf(_nan_like(o["res"]))
                    _direct(layer, x, out, L, res=Buf(o["res"]), **kn)
                    got = out.get()
                else:                                        # res + the running sum aliased to out, scale 1 / 3
                    ref = R.mrf_linear(*args, dil=dil, res=o["res"], add=o["add"], scale=1 / 3, core=core)
                    out = Buf(o["add"])
                    _direct(layer, x, out, L, res=Buf(o["res"]), add=out, scale=1 / 3, **kn)
                    got = out.get()
                w = R.worst(got, ref)
                print(f"RATIO {what} L={L} tpw={tpw} form={form} {w:.3f}")
                worst = max(worst, w)
    return worst


@pytest.mark.parametrize("inst", MRF_INSTANCES, ids=_inst_id)
def test_every_direct_instance_against_its_mirror(inst):
    """The smallest channel count the tile allows (128 for 128x128, 64 for 64x256, 32 for 32x512 and 32x256)."""
    what = _inst_id(inst)
    _report(what, run_direct(inst, TILES[inst[2]][2], what))


@pytest.mark.parametrize("K,dil", R.MRF_KD)
def test_direct_instance_with_two_m_blocks(K, dil):
    """C = 256 on the 128x128 tile: two row blocks per time tile.

    This is the case that moved the running sum out of ``conv_preload``: with the accumulators started at res + add, form
    (c) at k = 11, dilation 1 reached 1.091 of the limit at L = 124 (utterance 0, row 32, column 114: res -1537.6, add
    -2630.6, so each of the C * K = 2816 chained fmas rounded at ~4168, ulp 4.9e-4) and 1.003 at L = 128.  A sequential
    fp32 chain (ci outer, tap inner) on the CPU reproduces 1.0912 with that start and 0.750 with ``add`` added after the
    chain, which is what the epilogue does now."""
    what = f"k{K}-d{dil}-128x128-c32-l2 C=256"
    _report(what, run_direct((K, dil, "128x128", 32, 1, "OV_EPI_LINEAR", 2), 256, what))


def test_forced_knobs_without_an_instance_are_refused():
    """tile / chunk / loaders are exact: no 128x128 instance has one loader wave, no 32x512 one 32-channel chunks."""
    o, _ = _case(32, 3, 1, 4, False)
    layer = _direct_layer(32, 3, 1, False)
    for knobs in (dict(tile=1, chunk=32, loaders=1), dict(tile=3, chunk=32, loaders=4), dict(tile=4, chunk=16, loaders=2)):
        out = Buf(_nan_like(o["res"]))
        with pytest.raises(_lib.OvError, match="OV_E_UNSUPPORTED"):
            _direct(layer, Buf(o["x"], "vec"), out, 4, **knobs)
        assert torch.isnan(out.get()).all()


# ---- 2. the fused pair -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K,dil", PAIR_SHAPES, ids=lambda v: str(v))
def test_fused_pair_against_its_mirror_and_the_two_launches(C, K, dil):
    """Every element against ``R.pair``; the bits of the two direct launches the pair replaces, in both forms: pair and
    direct kernel start their accumulators at x + b2 and add the running sum after the conv, (x + b2 + conv) + add
    (conv1d_pair.h; conv1d_mfma.h ``conv_preload`` / ``conv_epilogue``)."""
    worst, differs = 0.0, []
    for L in R.PAIR_LS:
        for stress in (False, True):
            o = R.mrf_operands(C, K, dil, L, stress=stress)
            c1, c2 = _direct_layer(C, K, dil, stress), _direct_layer(C, K, dil, stress, second=True)
            args = (o["x"], o["w"], o["bias"], o["w2"], o["b2"], K, dil)
            x = Buf(o["x"], "vec")
            for form in ("plain", "sum"):
                ref = R.pair(*args) if form == "plain" else R.pair(*args, add=o["add"], scale=1 / 3)
                # the two direct launches the pair replaces, on dense tensors
                xd, t = o["x"].to(DEV), torch.empty(B, C, L, device=DEV)
                two = _nan_like(xd) if form == "plain" else o["add"].to(DEV)
                launch_conv(c1, xd, 0, C * L, t, 0, C * L, B, L, in_slope=0.1)
                launch_conv(c2, t, 0, C * L, two, 0, C * L, B, L, in_slope=0.1, res=xd, res_bs=C * L,
                            **({} if form == "plain" else dict(add=two, add_bs=C * L, scale=1 / 3)))
                two = two.cpu()
                w2 = R.worst(two, ref)
                for nwg in (0, 1, 3):
                    out = Buf(_nan_like(o["x"]) if form == "plain" else o["add"])
                    kw = {} if form == "plain" else dict(add=out.tail(), add_bs=out.bs, scale=1 / 3)
                    launch_pair(c1, c2, x.tail(), x.bs, out.tail(), out.bs, B, L, ld=x.ld, nwg=nwg, **kw)
                    got = out.get()
                    w = R.worst(got, ref)
                    print(f"RATIO pair C={C} k={K} d={dil} L={L} stress={stress} form={form} nwg={nwg} {w:.3f} (two launches {w2:.3f})")
                    worst = max(worst, w, w2)
                    if not torch.equal(got.view(torch.int32), two.view(torch.int32)):
                        differs.append((L, stress, form, nwg))
    _report(f"pair C={C} k={K} d={dil}", worst)
    assert not differs, f"pair differs from its two launches at (L, stress, form, nwg): {differs}"


# ---- 3. the Winograd-domain conv -----------------------------------------------------------------------------------------------------
# form -> (in_slope, out_slope, res, add in place, scale): the first conv of a pair (activated hand-over), the second
# (its input arrives activated), the last conv of a ResBlock (residual + the running MRF sum in place, scaled)
WINO_FORMS = {"c1": (0.1, 0.1, False, False, 1.0), "c2": (1.0, 1.0, True, False, 1.0), "last": (1.0, 1.0, True, True, 1 / 3)}


def _wino_ref(C, K, dil, L, stress, form, direct=False):
    in_slope, out_slope, has_res, has_add, scale = WINO_FORMS[form]
    o, core_d = _case(C, K, dil, L, stress, in_slope)
    kw = dict(dil=dil, in_slope=in_slope, res=o["res"] if has_res else None, add=o["add"] if has_add else None, scale=scale)
    if direct:
        return R.mrf_linear(o["x"], o["w"], o["bias"], core=core_d, **kw)
    return R.wino_linear(o["x"], o["w"], o["bias"], K, out_slope=out_slope, core=_wino_core(C, K, dil, L, stress, in_slope), **kw)


def _wino_launch(C, K, dil, L, stress, form, layout="vec", **kw):
    """One ov_conv1d_wino_f32 launch of ``form`` inside NaN-filled buffers -> the output ``Buf``."""
    in_slope, out_slope, has_res, has_add, scale = WINO_FORMS[form]
    o, _ = _case(C, K, dil, L, stress, in_slope)
    x = Buf(o["x"], layout)
    out = Buf(o["add"] if has_add else _nan_like(o["x"]), layout)
    if has_res:
        res = Buf(o["res"], layout)
        kw.update(res=res.tail(), res_bs=res.bs)
    if has_add:
        kw.update(add=out.tail(), add_bs=out.bs)
    wino.launch_conv_wino(_wino_layer(C, K, dil, stress), x.tail(), x.bs, out.tail(), out.bs, B, L, in_slope=in_slope,
                          scale=scale, out_slope=out_slope, x_ld=x.ld, out_ld=out.ld, **kw)
    return out


@pytest.mark.parametrize("C,K,dil", WINO_SHAPES, ids=lambda v: str(v))
def test_wino_instance_against_its_mirror(C, K, dil):
    """Both fragment counts where the family has both (128-row blocks at dilation 1), workgroup counts 0 / 1 / 7, and once
    under a column limit with a zero-length utterance.  The direct kernel's ratio against ``R.mrf_linear`` on the same
    operands is printed for the forms it can run (it has no output activation); it is not compared with Winograd's."""
    frag_list = (1, 2) if C % 128 == 0 and dil == 1 else (2,)
    worst = 0.0
    for L in R.WINO_LS:
        for stress in (False, True):
            for form in WINO_FORMS:
                ref = _wino_ref(C, K, dil, L, stress, form)
                wd = float("nan")
                if form != "c1":
                    in_slope, _, _, has_add, scale = WINO_FORMS[form]
                    o, _ = _case(C, K, dil, L, stress, in_slope)
                    out = Buf(o["add"] if has_add else _nan_like(o["x"]))
                    _direct(_direct_layer(C, K, dil, stress), Buf(o["x"], "vec"), out, L, res=Buf(o["res"]),
                            add=out if has_add else None, in_slope=in_slope, scale=scale)
                    wd = R.worst(out.get(), _wino_ref(C, K, dil, L, stress, form, direct=True))
                    assert wd <= 1.0, f"direct kernel C={C} k={K} d={dil} L={L} form={form}: {wd:.3f}"
                for frags in frag_list:
                    for nwg in (0, 1, 7):
                        w = R.worst(_wino_launch(C, K, dil, L, stress, form, frags=frags, nwg=nwg).get(), ref)
                        print(f"RATIO wino C={C} k={K} d={dil} L={L} stress={stress} form={form} frags={frags} nwg={nwg} "
                              f"{w:.3f} (direct kernel on the same operands, its own limit: {wd:.3f})")
                        worst = max(worst, w)
    # a column limit with a zero-length utterance: whole column blocks that start before the limit, NaN beyond
    L, ncol = 516, wino_ncol(C, dil)
    limits = [L, 0, L // 2]
    ref = _wino_ref(C, K, dil, L, True, "c1")
    got = _wino_launch(C, K, dil, L, True, "c1", col_limit=torch.tensor(limits, dtype=torch.int32, device=DEV),
                       col_limit_scale=1).get()
    for b, lim in enumerate(limits):
        done = min(L, -(-lim // ncol) * ncol)
        assert torch.isnan(got[b, :, done:]).all() and torch.isfinite(got[b, :, :done]).all(), (b, done)
        got[b, :, done:] = ref.ref[b, :, done:].float()
        ref.lim[b, :, done:] = float("inf")
    w = R.worst(got, ref)
    print(f"RATIO wino C={C} k={K} d={dil} L={L} col_limit {w:.3f}")
    _report(f"wino C={C} k={K} d={dil}", max(worst, w))


@pytest.mark.parametrize("C,dil,L", [(64, 3, 260), (128, 1, 516), (256, 5, 260)])
def test_wino_multi_launch_against_the_mirrors(C, dil, L):
    """One ``launch_convs_wino`` of the kernel sizes (3, 7, 11) per row family and operand form on stress data, held to the
    float64 mirrors themselves (tests/test_gpu_wino_multi.py compares it with the single launches only)."""
    worst = 0.0
    for form, (in_slope, out_slope, has_res, has_add, scale) in WINO_FORMS.items():
        convs, outs = [], []
        for K in (3, 7, 11):
            o, _ = _case(C, K, dil, L, True, in_slope)
            x, out = Buf(o["x"], "dense"), Buf(o["add"] if has_add else _nan_like(o["x"]), "dense")
            c = dict(layer=_wino_layer(C, K, dil, True), x=x.tail(), out=out.tail(), bs=x.bs, in_slope=in_slope,
                     out_slope=out_slope, scale=scale, keep=x)
            if has_res:
                c["keep_res"] = Buf(o["res"], "dense")
                c["res"] = c["keep_res"].tail()
            if has_add:
                c["add"] = out.tail()
            convs.append(c)
            outs.append(out)
        wino.launch_convs_wino(convs, B, L)
        for K, out in zip((3, 7, 11), outs):
            w = R.worst(out.get(), _wino_ref(C, K, dil, L, True, form))
            print(f"RATIO wino_multi C={C} d={dil} L={L} form={form} k={K} {w:.3f}")
            worst = max(worst, w)
    _report(f"wino_multi C={C} d={dil}", worst)
