"""The frame-rate conv epilogues and the fused WaveNet layer, one by one against float64 (oracle/fp32_ref.py), element
by element:  |out - ref64| <= S32 * absacc + N  on every element, no norm-wise bound and nothing left out.

Kernels: the GATE, RESSKIP, COUPLE, POSTERIOR, CONVT (generic, S8, S2) and MAGNITUDE epilogues of
openvoice_amd/csrc/conv1d_mfma.h, its frame-rate LINEAR instances (K = 1, 5; K = 3, 7 with 4-byte staging) and
openvoice_amd/csrc/wn_layer.hip (fused widths, the row-split pair), through ``launch_conv`` / ``launch_wn_layer``.

* ``INSTANCES`` names every instantiation of conv1d_inst_w.hip, conv1d_inst_s.hip and the grouped ConvTranspose ones
  of conv1d_inst_f.hip (tests/test_frame_criterion_cpu.py keeps the list equal to the sources).  Each runs against its
  mirror with tile, chunk and loader count FORCED (an exact match or OV_E_UNSUPPORTED) and the staging kind chosen by
  alignment: 16-byte staging needs x_ld % 4 == 0 and a 16-byte base; the 4-byte instances run once with an odd x_ld and
  once with the base moved by one float inside an aligned allocation.
* Every epilogue at T in {1, 2, 3, 4, 5, 127, 128, 129, 257}, B = 3, ragged lengths T, 1, T / 2.
* Layout: every tensor sits inside a larger NaN-filled buffer at a nonzero offset, rows padded (x_ld > L), batch strides
  larger than C * ld; everything outside the valid [B, C, :L] block must still be NaN afterwards.
  (``launch_wn_layer`` has one batch stride, H * ld, for all its tensors: there the offsets and the row padding vary.)
* Data edges for the gate, the fused layer and the posterior: ``fp32_ref.wn_operands(stress=True)`` (|t|, |s| to 30, s to
  -100, exact zeros, |t| ~ 1e-4) and logs in [-20, 20] at tau in {0, 0.3, 1}.

Each test prints ``RATIO <what> <worst err / lim>`` before it asserts.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib  # noqa: E402
from openvoice_amd.engine import (PackedConv, conv_transpose_as_conv, convt_row_order, gate_row_order, launch_conv,  # noqa: E402
                                  launch_wn_layer, wn_fused_row_order, wn_pack)
from openvoice_amd._lib import (EPI_CONVT, EPI_COUPLE, EPI_GATE, EPI_MAGNITUDE, EPI_POSTERIOR,  # noqa: E402
                                EPI_RESSKIP, F_CONVT_GROUPED, F_MASK_V, F_OUT2_INIT)
from oracle import fp32_ref as R  # noqa: E402
from oracle.nanbuf import Buf  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
B, H = R.B, R.H

# (K, dil, tile, chunk, vec, epilogue, loader waves): the X(...) lines of conv1d_inst_w.hip, conv1d_inst_s.hip and the
# EPI_CONVT_S8 / S2 lines of conv1d_inst_f.hip
INSTANCES = [
    (5, 1, "128x128", 16, 1, "OV_EPI_GATE", 2), (5, 1, "128x128", 32, 1, "OV_EPI_GATE", 2),
    (1, 1, "128x128", 32, 1, "OV_EPI_RESSKIP", 4), (1, 1, "128x128", 32, 1, "OV_EPI_COUPLE", 4),
    (1, 1, "128x128", 32, 1, "OV_EPI_POSTERIOR", 4),
    (5, 1, "128x128", 16, 0, "OV_EPI_GATE", 2), (5, 1, "128x128", 32, 0, "OV_EPI_GATE", 2),
    (1, 1, "128x128", 32, 0, "OV_EPI_RESSKIP", 4), (1, 1, "128x128", 32, 0, "OV_EPI_COUPLE", 4),
    (1, 1, "128x128", 32, 0, "OV_EPI_POSTERIOR", 4),
    (1, 1, "128x128", 32, 1, "OV_EPI_LINEAR", 4), (5, 1, "128x128", 16, 1, "OV_EPI_LINEAR", 2),
    (3, 1, "128x128", 16, 1, "OV_EPI_CONVT", 2), (3, 1, "128x128", 16, 1, "EPI_CONVT_S8", 2),
    (3, 1, "128x128", 16, 1, "EPI_CONVT_S2", 2),
    (1, 1, "128x128", 32, 0, "OV_EPI_LINEAR", 4), (3, 1, "128x128", 16, 0, "OV_EPI_LINEAR", 2),
    (5, 1, "128x128", 16, 0, "OV_EPI_LINEAR", 2), (7, 1, "128x128", 16, 0, "OV_EPI_LINEAR", 2),
    (3, 1, "128x128", 16, 0, "OV_EPI_CONVT", 2), (3, 1, "128x128", 16, 0, "EPI_CONVT_S8", 2),
    (3, 1, "128x128", 16, 0, "EPI_CONVT_S2", 2),
    (3, 1, "128x128", 32, 1, "OV_EPI_CONVT", 2), (3, 1, "128x128", 32, 1, "EPI_CONVT_S8", 2),
    (3, 1, "128x128", 32, 1, "EPI_CONVT_S2", 2),
    (3, 1, "64x256", 16, 1, "OV_EPI_CONVT", 4), (3, 1, "64x256", 16, 1, "EPI_CONVT_S8", 4),
    (3, 1, "64x256", 16, 1, "EPI_CONVT_S2", 4),
    (3, 1, "64x256", 32, 1, "OV_EPI_CONVT", 4), (3, 1, "64x256", 32, 1, "EPI_CONVT_S8", 4),
    (3, 1, "64x256", 32, 1, "EPI_CONVT_S2", 4),
    (4, 1, "128x128", 32, 1, "OV_EPI_MAGNITUDE", 4), (4, 1, "128x128", 32, 0, "OV_EPI_MAGNITUDE", 4),
    (3, 1, "128x128", 32, 1, "EPI_CONVT_S8", 4), (3, 1, "128x128", 32, 1, "EPI_CONVT_S2", 4),
]
TILE_ID = {"128x128": 1, "64x256": 2}
LAYOUTS_OF_VEC = {1: ("vec",), 0: ("odd_ld", "shift1")}


def _inst_id(inst):
    return "k{}-{}-c{}-v{}-{}-l{}".format(inst[0], inst[2], inst[3], inst[4], inst[5].replace("OV_", ""), inst[6])


def _knobs(inst):
    return dict(tile=TILE_ID[inst[2]], chunk=inst[3], loaders=inst[6])


# ---- tensors inside larger NaN-filled buffers: oracle/nanbuf.py ``Buf`` ------------------------------------------------
def _mask_rows(mask):
    """[B, T] -> device [B, mld] with NaN pad columns; returns (tensor, mld)."""
    T = mask.shape[1]
    mld = (T + 3) // 4 * 4 + 4
    m = torch.full((mask.shape[0], mld), NAN)
    m[:, :T] = mask
    return m.to(DEV), mld


def _report(what, *ratios):
    w = max(ratios)
    print(f"RATIO {what} {w:.3f}")
    assert w <= 1.0, f"{what}: worst err / lim = {w:.3f}"


def _conv(layer, x, out, L, **kw):
    """launch_conv on two ``Buf``s (offsets, row strides and batch strides from them)."""
    row0 = kw.pop("out_row0", 0)
    launch_conv(layer, x.flat, x.off, x.bs, out.flat, out.off + row0 * out.ld, out.bs, B, L, x_ld=x.ld, out_ld=out.ld, **kw)


# ---- cached operands, packed layers and float64 references ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _linear_case(K, T):
    o = R.linear_operands(K, T)
    full = R.linear(o["x"], o["w"], o["bias"], in_slope=0.1, bias_b=o["bias_b"], res=o["res"], add=o["add"], scale=1 / 3)
    masked = R.linear(o["x"], o["w"], o["bias"], res=o["res"], scale=0.5, mask=o["mask"])
    plain = R.linear(o["x"], o["w"], o["bias"])
    return o, PackedConv(o["w"], o["bias"], DEV, K=K), full, masked, plain


def run_linear(K, T, layout, knobs):
    o, layer, full, masked, plain = _linear_case(K, T)
    cout = o["w"].shape[0]
    x = Buf(o["x"], layout)
    res, add = Buf(o["res"]), Buf(o["add"])
    bb = torch.full((B, cout + 8), NAN)
    bb[:, 4:4 + cout] = o["bias_b"]
    maskd, mld = _mask_rows(o["mask"])
    out = Buf(torch.full_like(o["res"], NAN))
    _conv(layer, x, out, T, in_slope=0.1, res=res.flat, res_off=res.off, res_bs=res.bs, add=add.tail(), add_bs=add.bs,
          scale=1 / 3, bias_b=bb.to(DEV), bias_b_off=4, bias_b_bs=cout + 8, **knobs)
    r1 = R.worst(out.get(), full)
    out = Buf(torch.full_like(o["res"], NAN))
    _conv(layer, x, out, T, res=res.flat, res_off=res.off, res_bs=res.bs, scale=0.5, flags=F_MASK_V, mask=maskd,
          mask_bs=mld, **knobs)
    r2 = R.worst(out.get(), masked)
    out = Buf(torch.full_like(o["res"], NAN))
    _conv(layer, x, out, T, **knobs)                       # the store-only path of the LINEAR epilogue
    r3 = R.worst(out.get(), plain)
    return max(r1, r2, r3)


@functools.lru_cache(maxsize=None)
def _wn_case(T, stress=False, first=False, last=False):
    o = R.wn_operands(T, stress=stress, last=last)
    refs = R.wn_layer(o["x"], o["g"], o["mask"], o["skip"], o["w_in"], o["b_in"], o["w_rs"], o["b_rs"], first, last)
    return o, refs


@functools.lru_cache(maxsize=None)
def _gate_layer(T, stress):
    o, _ = _wn_case(T, stress)
    order = gate_row_order(H)
    return PackedConv(o["w_in"][order], o["b_in"][order], DEV, K=R.KG, cout=H), o["g"][:, order].contiguous().to(DEV)


def run_gate(T, layout, knobs, stress=False):
    """EPI_GATE alone; returns (ratio, Buf of acts)."""
    o, (acts_ref, _, _) = _wn_case(T, stress)
    layer, gd = _gate_layer(T, stress)
    acts = Buf(torch.full((B, H, T), NAN))
    _conv(layer, Buf(o["x"], layout), acts, T, epi=EPI_GATE, bias_b=gd, bias_b_bs=2 * H, rows=2 * H, **knobs)
    got = acts.get()
    assert torch.isfinite(got).all()
    return R.worst(got, acts_ref), got


def run_res_skip(T, layout, knobs, stress=False):
    """EPI_RESSKIP on exact (reference-independent) inputs: the gate's float64 value rounded to fp32 is the operand, so
    N = 0; middle, first (OUT2_INIT over NaN) and last (split = 0, h untouched) forms."""
    o, (acts_ref, _, _) = _wn_case(T, stress)
    acts = acts_ref.ref.float()
    maskd, mld = _mask_rows(o["mask"])
    ratios = []
    for first, last in ((False, False), (True, False), (False, True)):
        w_rs, b_rs = (o["w_rs"][H:], o["b_rs"][H:]) if last else (o["w_rs"], o["b_rs"])
        rh, rs = R.res_skip(acts, w_rs, b_rs, o["x"], o["skip"], o["mask"], 0 if last else H, first)
        layer = PackedConv(w_rs, b_rs, DEV, K=1)
        hbuf = Buf(o["x"])
        sbuf = Buf(torch.full_like(o["skip"], NAN) if first else o["skip"])
        _conv(layer, Buf(acts, layout), hbuf, T, epi=EPI_RESSKIP, flags=F_OUT2_INIT if first else 0, out2=sbuf.tail(),
              out2_bs=sbuf.bs, mask=maskd, mask_bs=mld, split=0 if last else H, **knobs)
        ratios.append(R.worst(sbuf.get(), rs))
        if last:
            assert torch.equal(hbuf.get(), o["x"]), "the last layer must not touch h"
        else:
            ratios.append(R.worst(hbuf.get(), rh))
    return max(ratios)


@functools.lru_cache(maxsize=None)
def _couple_case(T, reverse, flipped):
    o = R.couple_operands(T)
    w, b = (torch.flip(o["w"], [0]), torch.flip(o["b"], [0])) if flipped else (o["w"], o["b"])
    return o, PackedConv(w, b, DEV, K=1), R.couple(o["h"], o["w"], o["b"], o["x"], o["mask"], reverse, flipped)


def run_couple(T, layout, knobs):
    """In place into both halves' positions: physical rows C/2.. (natural order) and 0..C/2 (flipped), both directions."""
    ratios = []
    for reverse in (False, True):
        for flipped in (False, True):
            o, layer, ref = _couple_case(T, reverse, flipped)
            maskd, mld = _mask_rows(o["mask"])
            xb = Buf(o["x"])
            _conv(layer, Buf(o["h"], layout), xb, T, epi=EPI_COUPLE, mask=maskd, mask_bs=mld,
                  scale=-1.0 if reverse else 1.0, out_row0=0 if flipped else H // 2, **knobs)
            ratios.append(R.worst(xb.get(), ref))
    return max(ratios)


@functools.lru_cache(maxsize=None)
def _posterior_case(T, stress, tau):
    o = R.posterior_operands(T, stress=stress)
    order = gate_row_order(H)
    return o, PackedConv(o["w"][order], o["b"][order], DEV, K=1, cout=H), \
        R.posterior(o["h"], o["w"], o["b"], o["noise"], tau, o["mask"])


def run_posterior(T, layout, knobs, stress=False, tau=0.3):
    o, layer, ref = _posterior_case(T, stress, tau)
    maskd, mld = _mask_rows(o["mask"])
    noise, z = Buf(o["noise"]), Buf(torch.full((B, H, T), NAN))
    _conv(layer, Buf(o["h"], layout), z, T, epi=EPI_POSTERIOR, res=noise.flat, res_off=noise.off, res_bs=noise.bs,
          scale=tau, mask=maskd, mask_bs=mld, rows=2 * H, **knobs)
    got = z.get()
    assert torch.isfinite(got).all()
    return R.worst(got, ref)


@functools.lru_cache(maxsize=None)
def _convt_case(s, T, grouped):
    o = R.convt_operands(s, T)
    cout = o["w"].shape[1]
    wc, bc = conv_transpose_as_conv(o["w"], s), o["b"].repeat_interleave(s)
    if grouped:
        order = convt_row_order(cout, s)
        assert order is not None
        wc, bc = wc[order], bc[order]
    return o, PackedConv(wc, bc, DEV, K=3, cout=cout), R.conv_transpose(o["x"], o["w"], o["b"], s, 0.1)


def run_convt(s, T, layout, knobs, grouped):
    o, layer, ref = _convt_case(s, T, grouped)
    out = Buf(torch.full((B, layer.cout, s * T), NAN))
    x = Buf(o["x"], layout)
    launch_conv(layer, x.flat, x.off, x.bs, out.flat, out.off, out.bs, B, T, epi=EPI_CONVT, in_slope=0.1, phase_s=s,
                x_ld=x.ld, out_ld=out.ld, flags=F_CONVT_GROUPED if grouped else 0, **knobs)
    return R.worst(out.get(), ref)


@functools.lru_cache(maxsize=None)
def _magnitude_case(T):
    from openvoice_amd.mel_processing import _NativeSpectrogram
    o = R.magnitude_operands(T)
    ref, _ = R.magnitude(o["hops"], R.MAG_NFFT, R.MAG_HOP, 1e-6)
    return o, _NativeSpectrogram(torch.device(DEV), R.MAG_NFFT, R.MAG_HOP), ref


def run_magnitude(T, layout, knobs):
    o, spec, ref = _magnitude_case(T)
    x = Buf(o["hops"], layout)                    # the forward-aligned K = 4 conv reads all U = T + 3 columns
    out = Buf(torch.full((B, spec.bins, T), NAN))
    launch_conv(spec.layer, x.flat, x.off, x.bs, out.flat, out.off, out.bs, B, T, epi=EPI_MAGNITUDE, scale=1e-6,
                rows=spec.layer.rows, x_ld=x.ld, out_ld=out.ld, **knobs)
    return R.worst(out.get(), ref)


def _run(epi, T, layout, knobs, K=None):
    if epi == "OV_EPI_LINEAR":
        return run_linear(K, T, layout, knobs)
    if epi == "OV_EPI_GATE":
        return run_gate(T, layout, knobs)[0]
    if epi == "OV_EPI_RESSKIP":
        return run_res_skip(T, layout, knobs)
    if epi == "OV_EPI_COUPLE":
        return run_couple(T, layout, knobs)
    if epi == "OV_EPI_POSTERIOR":
        return run_posterior(T, layout, knobs)
    if epi == "OV_EPI_MAGNITUDE":
        return run_magnitude(T, layout, knobs)
    if epi == "OV_EPI_CONVT":
        return max(run_convt(s, T, layout, knobs, False) for s in (8, 2, 4))
    return run_convt(8 if epi == "EPI_CONVT_S8" else 2, T, layout, knobs, True)


# ---- 1. every instance, chosen on purpose --------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANCES, ids=_inst_id)
def test_every_instance_against_its_mirror(inst):
    """T = 129: two 128-column tiles, the second one column wide; B = 3 with ragged lengths 129, 1, 64."""
    K, _, _, _, vec, epi, _ = inst
    for layout in LAYOUTS_OF_VEC[vec]:
        _report(f"{_inst_id(inst)} {layout}", _run(epi, 129, layout, _knobs(inst), K))


def test_forced_knobs_without_an_instance_are_refused():
    """tile / chunk / loaders are exact: no GATE instance has four loader waves, no COUPLE one 16-channel chunks."""
    with pytest.raises(_lib.OvError, match="OV_E_UNSUPPORTED"):
        run_gate(5, "vec", dict(tile=1, chunk=32, loaders=4))
    with pytest.raises(_lib.OvError, match="OV_E_UNSUPPORTED"):
        run_couple(5, "vec", dict(tile=1, chunk=16, loaders=4))
    with pytest.raises(_lib.OvError, match="OV_E_UNSUPPORTED"):
        run_posterior(5, "odd_ld", dict(tile=2, chunk=32, loaders=4))


# ---- 2. shape edges per epilogue ---------------------------------------------------------------------------------------
# the dispatcher's first choice of each epilogue, forced, so that the staging kind is the only thing alignment decides
EDGE_CASES = [("OV_EPI_LINEAR", 1, dict(tile=1, chunk=32, loaders=4)), ("OV_EPI_LINEAR", 5, dict(tile=1, chunk=16, loaders=2)),
              ("OV_EPI_LINEAR", 3, dict(tile=1, chunk=16, loaders=2)), ("OV_EPI_LINEAR", 7, dict(tile=1, chunk=16, loaders=2)),
              ("OV_EPI_GATE", 5, dict(tile=1, chunk=32, loaders=2)), ("OV_EPI_RESSKIP", 1, dict(tile=1, chunk=32, loaders=4)),
              ("OV_EPI_COUPLE", 1, dict(tile=1, chunk=32, loaders=4)), ("OV_EPI_POSTERIOR", 1, dict(tile=1, chunk=32, loaders=4)),
              ("OV_EPI_CONVT", 3, dict(tile=1, chunk=32, loaders=2)), ("EPI_CONVT_S8", 3, dict(tile=1, chunk=32, loaders=4)),
              ("EPI_CONVT_S2", 3, dict(tile=1, chunk=32, loaders=4)), ("OV_EPI_MAGNITUDE", 4, dict(tile=1, chunk=32, loaders=4))]


@pytest.mark.parametrize("T", R.T_EDGES)
@pytest.mark.parametrize("epi,K,knobs", EDGE_CASES, ids=[f"{e.replace('OV_', '')}-k{k}" for e, k, _ in EDGE_CASES])
def test_shape_edges(epi, K, knobs, T):
    """T = 1 .. 5 (fewer columns than a 16-byte vector, than the halo), 127 / 128 / 129 around one tile, 257 = three tiles;
    16-byte staging from padded rows and 4-byte staging from odd rows.  LINEAR at K = 3 / 7 is in scope with 4-byte staging
    only (its aligned run takes a ResBlock instance of the same shape, which is exact too)."""
    for layout in ("vec", "odd_ld"):
        kn = dict(knobs)
        if epi in ("OV_EPI_CONVT", "EPI_CONVT_S8", "EPI_CONVT_S2") and layout == "odd_ld":
            kn.update(chunk=16, loaders=2)           # the 4-byte ConvTranspose instances are the chunk-16 ones
        if epi == "OV_EPI_LINEAR" and K in (3, 7) and layout == "vec":
            continue
        _report(f"{epi} k{K} T={T} {layout}", _run(epi, T, layout, kn, K))


# ---- 3. data edges -----------------------------------------------------------------------------------------------------
def test_stress_operands_cover_the_ranges():
    """The generator does what its docstring says (float64 pre-activations): |t|, |s| beyond 25, s below -95, exact
    zeros, 0 < |t| < 1e-3."""
    o, _ = _wn_case(129, True)
    pre, _ = R._affine(o["x"], o["w_in"], o["b_in"], o["g"])
    t, s = pre[:, :H], pre[:, H:]
    assert t.abs().max() > 25 and s.max() > 25 and s.min() < -95
    assert (t == 0).any() and (s == 0).any() and ((t.abs() > 0) & (t.abs() < 1e-3)).any()
    p = R.posterior_operands(129, stress=True)
    logs = R._affine(p["h"], p["w"], p["b"])[0][:, H:]
    assert logs.min() < -19 and logs.max() > 19


@pytest.mark.parametrize("chunk,layout", [(32, "vec"), (16, "vec"), (32, "odd_ld"), (16, "shift1")])
@pytest.mark.parametrize("T", [5, 129])
def test_gate_epilogue_at_saturation_zeros_and_overflow(T, chunk, layout):
    r, _ = run_gate(T, layout, dict(tile=1, chunk=chunk, loaders=2), stress=True)      # asserts finite outputs
    _report(f"EPI_GATE stress T={T} chunk={chunk} {layout}", r)


@pytest.mark.parametrize("tau", R.TAUS)
@pytest.mark.parametrize("layout", ["vec", "odd_ld"])
def test_posterior_epilogue_with_logs_to_plus_minus_20(tau, layout):
    for T in (5, 129):
        _report(f"EPI_POSTERIOR stress tau={tau} T={T} {layout}",
                run_posterior(T, layout, dict(tile=1, chunk=32, loaders=4), stress=True, tau=tau))


# ---- 4. wn_layer.hip -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wn_packed(T, stress, last):
    o, _ = _wn_case(T, stress, False, last)
    order = wn_fused_row_order(H)
    w_rs, b_rs = o["w_rs"], o["b_rs"]
    if last:
        w_rs, b_rs = torch.cat([torch.zeros_like(w_rs), w_rs]), torch.cat([torch.zeros_like(b_rs), b_rs])
    return dict(hidden=H, K=R.KG, w_in=wn_pack(o["w_in"][order], DEV), b_in=o["b_in"][order].contiguous().to(DEV),
                w_rs=wn_pack(w_rs, DEV), b_rs=b_rs.contiguous().to(DEV)), o["g"][:, order].contiguous()


def _flat_rows(t, ld, off):
    """[B, C, T] -> device flat NaN buffer holding [B][C][ld] from element ``off`` (batch stride C * ld: the layer's own),
    a validity map, and the view a C caller would pass."""
    Bn, C, T = t.shape
    flat = torch.full((off + Bn * C * ld + 8,), NAN)
    valid = torch.zeros_like(flat, dtype=torch.bool)
    flat[off:off + Bn * C * ld].view(Bn, C, ld)[:, :, :T] = t
    valid[off:off + Bn * C * ld].view(Bn, C, ld)[:, :, :T] = True
    return flat.to(DEV), valid


def _unflat(flat, valid, shape, ld, off):
    Bn, C, T = shape
    host = flat.cpu()
    assert torch.isnan(host[~valid]).all(), "written outside the valid [B, C, :T] block"
    return host[off:off + Bn * C * ld].view(Bn, C, ld)[:, :, :T].clone()


def run_wn_layer(T, width, row_split=1, stress=False, first=False, last=False):
    o, (acts_ref, rh, rs) = _wn_case(T, stress, first, last)
    layer, g = _wn_packed(T, stress, last)
    ld = (T + 3) // 4 * 4 + 4                       # padded rows; offsets are multiples of 4 (16-byte bases are required)
    shape = (B, H, T)
    xf, xv = _flat_rows(o["x"], ld, 4)
    of, ov = _flat_rows(torch.full(shape, NAN), ld, 12)
    sf, sv = _flat_rows(torch.full(shape, NAN) if first else o["skip"], ld, 8)
    maskd, mld = _mask_rows(o["mask"])
    gd = torch.full((B * 2 * H + 8,), NAN)
    gd[4:4 + B * 2 * H] = g.reshape(-1)
    af = av = None
    if row_split == 3:
        af, av = _flat_rows(torch.full(shape, NAN), ld, 16)
    launch_wn_layer(layer, xf[4:], of[12:], sf[8:], maskd, B, T, ld, cond=gd.to(DEV), cond_off=4, cond_bs=2 * H,
                    first=first, last=last, width=width, mask_bs=mld, acts=None if af is None else af[16:],
                    row_split=row_split)
    torch.cuda.synchronize()
    ratios = [R.worst(_unflat(sf, sv, shape, ld, 8), rs)]
    if last:
        assert torch.isnan(of.cpu()).all(), "the last layer must not write h'"
    else:
        ratios.append(R.worst(_unflat(of, ov, shape, ld, 12), rh))
    if af is not None:
        ratios.append(R.worst(_unflat(af, av, shape, ld, 16), acts_ref))
    return max(ratios)


@pytest.mark.parametrize("T", R.T_EDGES)
@pytest.mark.parametrize("form", ["w16", "w128", "auto", "split"])
def test_wn_layer_shape_edges(form, T):
    width, row_split = {"w16": (16, 1), "w128": (128, 1), "auto": (0, 1), "split": (0, 3)}[form]
    _report(f"wn_layer {form} T={T}", run_wn_layer(T, width, row_split))


@pytest.mark.parametrize("form", ["w16", "w128", "auto", "split"])
def test_wn_layer_at_saturation_zeros_and_overflow(form):
    width, row_split = {"w16": (16, 1), "w128": (128, 1), "auto": (0, 1), "split": (0, 3)}[form]
    for T in (5, 129):
        _report(f"wn_layer stress {form} T={T}", run_wn_layer(T, width, row_split, stress=True))


@pytest.mark.parametrize("form", ["w16", "auto", "split"])
def test_wn_layer_first_and_last_forms(form):
    width, row_split = {"w16": (16, 1), "auto": (0, 1), "split": (0, 3)}[form]
    _report(f"wn_layer first {form}", run_wn_layer(129, width, row_split, first=True))
    _report(f"wn_layer last {form}", run_wn_layer(129, width, row_split, last=True))
    _report(f"wn_layer first+last {form}", run_wn_layer(5, width, row_split, stress=True, first=True, last=True))


@pytest.mark.parametrize("stress", [False, True])
@pytest.mark.parametrize("T", [5, 129, 257])
def test_generic_two_launch_path_against_the_same_mirror(T, stress):
    """EPI_GATE then EPI_RESSKIP on the device's own gate output, on the operands of the fused tests, held to the
    ``wn_layer`` mirror (not to the fused kernel): the res/skip limit carries the gate's limit through |w_rs|."""
    o, (acts_ref, rh, rs) = _wn_case(T, stress)
    r_gate, acts = run_gate(T, "vec", dict(tile=1, chunk=32, loaders=2), stress=stress)
    maskd, mld = _mask_rows(o["mask"])
    hbuf, sbuf = Buf(o["x"]), Buf(o["skip"])
    _conv(PackedConv(o["w_rs"], o["b_rs"], DEV, K=1), Buf(acts, "vec"), hbuf, T, epi=EPI_RESSKIP, out2=sbuf.tail(),
          out2_bs=sbuf.bs, mask=maskd, mask_bs=mld, split=H)
    _report(f"two-launch T={T} stress={stress}", r_gate, R.worst(hbuf.get(), rh), R.worst(sbuf.get(), rs))
