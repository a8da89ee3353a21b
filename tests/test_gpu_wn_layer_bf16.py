"""The bf16 WaveNet layer (``ov_wn_layer_bf16``, openvoice_amd/csrc/wn_layer_bf16.hip) against its float64 mirror, element
by element (tests/wn_bf16_ref.py: |out - ref64| <= S absacc2 + flip + 1/2 ulp_f32), and against itself bit for bit across
tile widths, batch rows and positions.  H = 192, K = 5; shapes are the smallest at which the kernel can go wrong: one to
three columns, one column either side of a 16-column fragment, one and two columns into a second 128-column tile."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import wn_bf16_ref as R  # noqa: E402
from openvoice_amd import _lib  # noqa: E402
from openvoice_amd.engine import launch_wn_layer, wn_bf16_pack, wn_fused_row_order  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, K = R.H, R.K
NAN = float("nan")
FAMILY = "wn bf16 criterion"


def _packed(c):
    order = wn_fused_row_order(H)
    w_rs, b_rs = c["w_rs"], c["b_rs"]
    if w_rs.shape[0] == H:                     # last layer: skip rows only, padded to 2H rows (include/openvoice_amd.h)
        w_rs, b_rs = torch.cat([torch.zeros_like(w_rs), w_rs]), torch.cat([torch.zeros_like(b_rs), b_rs])
    return dict(hidden=H, K=K, w_in_bf16=wn_bf16_pack(c["w_in"][order], DEV), b_in=c["b_in"][order].contiguous().to(DEV),
                w_rs_bf16=wn_bf16_pack(w_rs, DEV), b_rs=b_rs.contiguous().to(DEV), w_in=None, w_rs=None)


def _launch(c, width=0, ld=None, guard=1, layer=None):
    """Run the layer on the operands ``c`` in NaN-poisoned buffers: rows of ``ld`` floats (NaN in every column of x the
    entry is documented not to read -- those from T rounded up to 4 on -- and everywhere in ``skip`` when ``first``),
    ``guard`` whole rows of NaN before and after every tensor.  Returns (out, skip) as written, [B, H, ld] on the CPU,
    after asserting that guards and columns >= T are untouched."""
    B, _, T = c["x"].shape
    ld = (T + 3) // 4 * 4 + 8 if ld is None else ld
    g0 = guard * ld

    def buf(t=None, fill_cols=NAN, fill_from=T):
        flat = torch.full((g0 + B * H * ld + g0,), NAN)
        body = flat[g0:g0 + B * H * ld].view(B, H, ld)
        if t is not None:
            body[:, :, :T] = t
            body[:, :, T:fill_from] = 0.0
            body[:, :, fill_from:] = fill_cols
        return flat.to(DEV)

    t4 = (T + 3) // 4 * 4
    xf = buf(c["x"], fill_from=t4)              # columns T .. t4 - 1 are read and discarded: any finite value
    sf = buf(None if c["first"] else c["skip"])
    of = buf()
    mask = torch.full((B, ld), NAN)
    mask[:, :t4] = 0.0
    mask[:, :T] = c["mask"]
    maskd = mask.to(DEV)
    order = wn_fused_row_order(H)
    gd = None if c["g"] is None else c["g"][:, order].contiguous().to(DEV)
    view = lambda f: f[g0:g0 + B * H * ld].view(B, H, ld)
    before_out, before_skip = of.clone(), sf.clone()
    launch_wn_layer(layer or _packed(c), view(xf), view(of), view(sf), maskd, B, T, ld, cond=gd,
                    cond_bs=0 if (gd is None or gd.shape[0] == 1) else 2 * H, first=c["first"], last=c["last"], width=width,
                    mask_bs=ld, bf16=True)
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    for name, f, before in (("out", of, before_out), ("skip", sf, before_skip)):
        assert same(f[:g0], before[:g0]) and same(f[-g0:], before[-g0:]), f"{name}: guard rows written"
        assert same(view(f)[:, :, T:], view(before)[:, :, T:]), f"{name}: columns >= T written"
    if c["last"]:
        assert same(of, before_out), "a last layer must not write out"
    return view(of).cpu(), view(sf).cpu()


def _check(c, width=0, what="", **kw):
    T = c["x"].shape[2]
    out, skip = _launch(c, width, **kw)
    ref = R.layer(c)
    return R.check(None if c["last"] else out[:, :, :T], skip[:, :, :T], ref, what, family=FAMILY)


@pytest.mark.parametrize("T", R.LENGTHS)
@pytest.mark.parametrize("B", R.BATCHES)
def test_shape_sweep(B, T):
    """Launcher-chosen width; middle, first, last and first + last forms; per-item conditioning; ragged masks (B = 3 has
    a zero-length item)."""
    worst = 0.0
    for first, last in ((False, False), (True, False), (False, True), (True, True)):
        worst = max(worst, _check(R.case(B, T, 0, first=first, last=last), what=f"B={B} T={T} first={first} last={last}"))
    print(f"[wn bf16 criterion] worst err / lim {worst:.4f} (B={B} T={T})")


@pytest.mark.parametrize("width", range(16, 129, 16))
def test_every_legal_width_at_129_columns(width):
    assert _lib.call("ov_wn_layer_bf16_tile", 3, 129, width) == width
    worst = _check(R.case(3, 129, 1), width, what=f"width={width}")
    print(f"[wn bf16 criterion] worst err / lim {worst:.4f} (width={width})")


@pytest.mark.parametrize("cond", [None, "broadcast", "item"])
def test_conditioning_forms(cond):
    _check(R.case(3, 17, 2, cond=cond), what=f"cond={cond}")
    _check(R.case(3, 130, 2, cond=cond, first=True), 64, what=f"cond={cond} width=64")


def test_wide_rows_and_ragged_masks():
    """ld far beyond T; every item ragged, one of length 1, one of length 0."""
    _check(R.case(3, 130, 3, lengths=[129, 1, 0]), ld=400, what="ld=400")
    _check(R.case(3, 15, 3, lengths=[7, 15, 0], last=True), ld=64, what="ld=64 last")


def test_bit_identical_across_widths_rows_and_positions():
    c = R.case(3, 130, 4)
    layer = _packed(c)
    o16, s16 = _launch(c, 16, layer=layer)
    o128, s128 = _launch(c, 128, layer=layer)
    assert torch.equal(o16[:, :, :130], o128[:, :, :130]) and torch.equal(s16[:, :, :130], s128[:, :, :130]), "width 16 vs 128"
    # row 2 of 3 (index 1) against the same item alone
    solo = dict(c, x=c["x"][1:2], skip=c["skip"][1:2], mask=c["mask"][1:2], g=c["g"][1:2])
    o1, s1 = _launch(solo, 0, layer=layer)
    assert torch.equal(o1[0, :, :130], o128[1, :, :130]) and torch.equal(s1[0, :, :130], s128[1, :, :130]), "alone vs row 2 of 3"
    # a 130-column input against the same columns inside a 400-column input, the surrounding columns copied: interior
    # columns (two of halo) of the small input's item 0 see the same neighbourhood at offset 135
    T2, off = 400, 135
    big = R.case(3, T2, 5, lengths=[T2, T2, T2])
    big = dict(big, w_in=c["w_in"], b_in=c["b_in"], w_rs=c["w_rs"], b_rs=c["b_rs"], g=c["g"])
    small = dict(c, x=big["x"][:, :, off:off + 130].clone(), skip=big["skip"][:, :, off:off + 130].clone(),
                 mask=torch.ones(3, 130))
    ob, sb = _launch(big, 0, layer=layer)
    os_, ss = _launch(small, 0, layer=layer)
    assert torch.equal(os_[:, :, 2:128], ob[:, :, off + 2:off + 128]), "out: position inside a longer input"
    assert torch.equal(ss[:, :, 2:128], sb[:, :, off + 2:off + 128]), "skip: position inside a longer input"


def test_error_codes_match_the_fp32_entry():
    c = R.case(1, 16, 6)
    layer = _packed(c)
    x = c["x"].to(DEV).contiguous()
    mask = torch.ones(1, 16, device=DEV)
    z = lambda: torch.zeros_like(x)
    with pytest.raises(_lib.OvError, match="OV_E_BADARG"):
        launch_wn_layer(layer, x, x, z(), mask, 1, 16, 16, bf16=True)                       # out aliases x
    with pytest.raises(_lib.OvError, match="OV_E_BADARG"):
        launch_wn_layer(layer, x, z(), z(), mask, 1, 16, 16, width=24, bf16=True)           # not a multiple of 16
    with pytest.raises(_lib.OvError, match="OV_E_BADARG"):
        launch_wn_layer(layer, x, z(), z(), mask, 1, 16, 12, bf16=True)                     # ld < T
    with pytest.raises(_lib.OvError, match="OV_E_UNSUPPORTED"):
        launch_wn_layer(dict(layer, K=3), x, z(), z(), mask, 1, 16, 16, bf16=True)
    with pytest.raises(_lib.OvError, match="OV_E_ALIGN"):
        launch_wn_layer(layer, x, z(), z(), mask, 1, 14, 14, bf16=True)                     # ld not a multiple of 4
    with pytest.raises(_lib.OvError, match="OV_E_ALIGN"):
        launch_wn_layer(layer, x, z(), z(), torch.ones(20, device=DEV)[1:17].view(1, 16), 1, 16, 16, bf16=True)
    with pytest.raises(_lib.OvError, match="OV_E_BADARG"):
        launch_wn_layer(layer, x, z(), z(), torch.ones(1, 16, device=DEV), 1, 15, 16, mask_bs=12, bf16=True)
    torch.cuda.synchronize()


def test_stack_and_coupling_through_the_engine():
    """The 16-layer posterior stack and one coupling's 4-layer stack through ``ConverterEngine._wavenet`` with
    ``wavenet="bf16"``, against the mirror chained layer by layer: every layer is checked on the GPU's own input to that
    layer (captured from the ping-pong buffers), so a flipped rounding does not chain."""
    from openvoice_amd import engine as engine_mod
    from openvoice_amd.params import effective_weight, synthetic_state_dict
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    sd = synthetic_state_dict(CFG, 513, seed=1234)
    eng = engine_mod.ConverterEngine(sd, CFG, 513, DEV)
    B, T = 2, 40
    ws = eng._workspace(B, T)
    Tp = ws["Tp"]
    lengths = torch.tensor([T, T - 7], device=DEV)
    _lib.call("ov_sequence_mask_f32", lengths, ws["mask"], B, T, Tp)
    mask = ws["mask"][:, :T].cpu()
    g = 0.3 * R.rand(B, eng.gin, seed=77).to(DEV)
    real = engine_mod.launch_wn_layer
    for prefix, wn in (("enc_q.enc", eng.q_wn), ("flow.flows.0.enc", eng.couplings[0]["wn"])):
        cond = eng._wn_cond(wn, g)
        ws["h"][:, :, :T] = (R.rand(B, H, T, seed=len(prefix)) * mask[:, None]).to(DEV)
        seen = []

        def spy(layer, x, out, skip, *a, **kw):
            before = (x[:, :, :T].cpu().clone(), skip[:, :, :T].cpu().clone())
            real(layer, x, out, skip, *a, **kw)
            assert kw.get("bf16") is True
            seen.append(before + (out[:, :, :T].cpu().clone(), skip[:, :, :T].cpu().clone()))

        engine_mod.launch_wn_layer = spy
        try:
            with eng.wavenet_scope("bf16"):
                eng._wavenet(wn, ws, B, T, cond, ws["mask"])
        finally:
            engine_mod.launch_wn_layer = real
        torch.cuda.synchronize()
        assert len(seen) == wn.n_layers
        inv = torch.argsort(wn_fused_row_order(H))
        worst = 0.0
        for i, (x_in, skip_in, out, skip) in enumerate(seen):
            last = i == wn.n_layers - 1
            c = dict(x=x_in, skip=skip_in, mask=mask, g=cond[:, 2 * H * i:2 * H * (i + 1)].cpu()[:, inv],
                     w_in=effective_weight(sd, f"{prefix}.in_layers.{i}"), b_in=sd[f"{prefix}.in_layers.{i}.bias"].float(),
                     w_rs=effective_weight(sd, f"{prefix}.res_skip_layers.{i}"),
                     b_rs=sd[f"{prefix}.res_skip_layers.{i}.bias"].float(), first=i == 0, last=last)
            worst = max(worst, R.check(None if last else out, skip, R.layer(c), f"{prefix} layer {i}", family=FAMILY))
        print(f"[wn bf16 criterion] worst err / lim {worst:.4f} ({prefix}, {wn.n_layers} layers)")
