"""Several Winograd-domain convs in one persistent launch (``ov_conv1d_wino_multi_f32``, csrc/conv1d_wino.h
``conv1d_wino_multi_kernel``) against the single launches it replaces: the same bits in every output element, nothing
written anywhere else (the outputs start as NaN and are compared as bit patterns), and the same refusals.
Row families 64 (two row fragments per workgroup), 128 (four) and 256 (two M-blocks); one, two and three convs per launch
in any order; dilations 1 / 3 / 5; B = 1 and 3; forced workgroup counts 1, 3, 7 (lists dealt whole: workgroups that get no
item of a conv), 16 and 24 (XCD eighths; the cost-balanced cut of the last conv's list); column limits with a zero-length
utterance and with every utterance empty; the three operand forms the engine launches.
Lengths: the kernel takes L % 4 == 0 only (the launcher answers OV_E_ALIGN otherwise, which is tested), so the ragged
lengths around a column block are 4, 252, 260 and 1032 (one block with a single tile; just below / just above 256 columns;
several blocks with a ragged last one and fewer items than workgroups).
reference: openvoice/modules.py:296-309 (ResBlock1.forward), models.py:280-286 (MRF)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
_layers = {}


def _layer(C, K, dil):
    """One packed conv per (C, K, dil), shared by every test of the module (packing is host work)."""
    from openvoice_amd import wino
    key = (C, K, dil)
    if key not in _layers:
        gen = torch.Generator().manual_seed(1000 * C + 10 * K + dil)
        w = torch.randn(C, C, K, generator=gen) * (C * K) ** -0.5
        _layers[key] = wino.PackedConvWino(w, torch.randn(C, generator=gen) * 0.1, DEV, dil=dil)
    return _layers[key]


def _bits(t):
    return t.view(torch.int32)


def _convs(form, ks, C, dil, B, L, seed):
    """The launch of ``form`` for kernel sizes ``ks``: per conv (dict for launch_convs_wino, initial content of out)."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randn(B, C, L, generator=gen).to(DEV)
    out = []
    for k in ks:
        c = dict(layer=_layer(C, k, dil), x=rnd(), bs=C * L)
        if form == "c1":           # first conv of a pair: activated hand-over
            c.update(in_slope=0.1, out_slope=0.1)
            init = torch.full((B, C, L), NAN, device=DEV)
        elif form == "c2":         # second conv: residual
            c.update(res=rnd())
            init = torch.full((B, C, L), NAN, device=DEV)
        else:                      # last conv of a ResBlock: residual + the running MRF sum, in place, scaled
            c.update(res=rnd(), scale=1.0 / 3)
            init = rnd()
        out.append((c, init))
    return out


def _run_single(convs, B, L, nwg=0, **lim):
    from openvoice_amd import wino
    outs = []
    for c, init in convs:
        o = init.clone()
        add = o if "scale" in c else None
        wino.launch_conv_wino(c["layer"], c["x"], c["bs"], o, c["bs"], B, L, in_slope=c.get("in_slope", 1.0),
                              scale=c.get("scale", 1.0), res=c.get("res"), res_bs=c["bs"] if "res" in c else 0, add=add,
                              add_bs=c["bs"] if add is not None else 0, out_slope=c.get("out_slope", 1.0), nwg=nwg, **lim)
        outs.append(o)
    return outs


def _run_multi(convs, B, L, nwg=0, **lim):
    from openvoice_amd import wino
    outs, args = [], []
    for c, init in convs:
        o = init.clone()
        outs.append(o)
        args.append(dict(c, out=o, **({"add": o} if "scale" in c else {})))
    wino.launch_convs_wino(args, B, L, nwg=nwg, **lim)
    return outs


KS = ([11], [7], [3], [7, 3], [3, 11], [3, 7, 11], [11, 3, 7])


@pytest.mark.parametrize("B,L", [(1, 4), (3, 252), (1, 260), (3, 1032)])
@pytest.mark.parametrize("dil", [1, 3, 5])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_multi_launch_equals_the_single_launches(C, dil, B, L):
    n = 0
    for form in ("c1", "c2", "last"):
        for ks in KS:
            convs = _convs(form, ks, C, dil, B, L, seed=C + dil + L + len(ks))
            want = _run_single(convs, B, L)
            for nwg in (0, 1, 3, 7, 16):
                got = _run_multi(convs, B, L, nwg=nwg)
                for k, g, w in zip(ks, got, want):
                    assert torch.equal(_bits(g), _bits(w)), (form, ks, k, nwg)
                n += 1
    torch.cuda.synchronize()
    assert n == 3 * len(KS) * 5


@pytest.mark.parametrize("C,dil,B,L", [(64, 1, 3, 7172), (64, 5, 3, 6724), (128, 3, 3, 4780), (256, 1, 3, 2564)])
@pytest.mark.parametrize("nwg", [16, 24, 40, 0])
def test_cost_balanced_cut_covers_every_item(C, dil, B, L, nwg):
    """Lists long enough for the cost-balanced split (an XCD's eighth holds several items per workgroup and does not
    divide evenly): the K = 3 list is cut into contiguous ranges, the K = 7 list dealt from the other end; an item nobody
    computed would leave NaN behind."""
    for ks in ([3, 7, 11], [3, 11], [7, 3]):
        convs = _convs("c1", ks, C, dil, B, L, seed=C + dil + nwg)
        want = _run_single(convs, B, L)
        got = _run_multi(convs, B, L, nwg=nwg)
        for g, w in zip(got, want):
            assert not torch.isnan(g).any()
            assert torch.equal(_bits(g), _bits(w)), (ks, nwg)


@pytest.mark.parametrize("limits", [[300, 0, 1032], [0, 0, 0], [5, 1032, 260]])
@pytest.mark.parametrize("C,dil", [(64, 3), (128, 1), (256, 5)])
def test_multi_launch_under_a_column_limit(C, dil, limits):
    """Length-aware work lists: a zero-length utterance, every utterance empty (nothing is written at all), ragged limits;
    what lies beyond a limit stays NaN in both."""
    B, L = 3, 1032
    lim = dict(col_limit=torch.tensor(limits, dtype=torch.int32, device=DEV), col_limit_scale=1)
    for form in ("c1", "last"):
        convs = _convs(form, [7, 11, 3], C, dil, B, L, seed=C + dil)
        want = _run_single(convs, B, L, **lim)
        for nwg in (0, 3, 16):
            got = _run_multi(convs, B, L, nwg=nwg, **lim)
            for g, w in zip(got, want):
                assert torch.equal(_bits(g), _bits(w)), (form, nwg)
    if not any(limits):
        assert all(torch.isnan(g).all() for g in _run_multi(_convs("c1", [7, 11, 3], C, dil, B, L, 1), B, L, **lim))


def _params(convs, B, L, over=None):
    from openvoice_amd import _lib
    ps = (_lib.ConvWinoParams * len(convs))()
    for p, (layer, x, out) in zip(ps, convs):
        p.x, p.w, p.bias, p.out = (ctypes.c_void_p(t.data_ptr()) for t in (x, layer.w, layer.bias, out))
        p.B, p.Cin, p.Cout, p.L, p.K, p.dil = B, layer.cin, layer.cout, L, layer.K, layer.dil
        p.x_bstride = p.out_bstride = layer.cin * L
        p.in_slope, p.scale, p.out_slope = 0.1, 1.0, 1.0
    for (i, field), v in (over or {}).items():
        setattr(ps[i], field, v)
    return ps


def test_mismatched_convs_are_refused_and_nothing_is_written():
    from openvoice_amd import _lib
    lib = _lib.load()
    B, L, C = 2, 260, 128
    x = torch.randn(B, C, L, device=DEV)
    outs = [torch.full((B, C, L), NAN, device=DEV) for _ in range(3)]
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    mk = lambda ks, over=None, dils=(1, 1, 1): _params([(_layer(C, k, d), x, o) for k, d, o in zip(ks, dils, outs)], B, L, over)
    call = lambda ps, n=None: lib.ov_conv1d_wino_multi_f32(ps, len(ps) if n is None else n, stream)
    BADARG, UNSUPPORTED, ALIGN = -1, -2, -3
    lim = torch.zeros(B, dtype=torch.int32, device=DEV)
    assert call(mk([3, 7, 11]), 0) == BADARG and call(mk([3, 7, 11]), 4) == BADARG
    assert lib.ov_conv1d_wino_multi_f32(None, 2, stream) == BADARG
    assert call(mk([3, 7], {(1, "L"): 256})) == BADARG
    assert call(mk([3, 7], {(1, "B"): 1})) == BADARG
    assert call(mk([3, 7, 11], dils=(1, 1, 3))) == BADARG
    assert call(mk([3, 7], {(0, "col_limit"): ctypes.c_void_p(lim.data_ptr()), (0, "col_limit_scale"): 1})) == BADARG
    assert call(mk([3, 7], {(1, "out"): None})) == BADARG
    assert call(mk([3, 3])) == UNSUPPORTED                       # one conv per kernel size
    assert call(mk([3, 7], {(0, "frags"): 1, (1, "frags"): 1})) == UNSUPPORTED
    assert call(mk([3, 7], {(1, "in_slope"): 2.0})) == UNSUPPORTED
    assert call(mk([3, 7], {(0, "L"): 255, (1, "L"): 255})) == ALIGN     # L % 4: as the single launch
    mixed = _params([(_layer(C, 3, 1), x, outs[0]), (_layer(64, 7, 1), x, outs[1])], B, L)
    assert call(mixed) in (BADARG, UNSUPPORTED)
    l32 = [(_layer(32, 11, 1), x, outs[0]), (_layer(32, 11, 3), x, outs[1])]
    assert call(_params(l32, B, L)) in (BADARG, UNSUPPORTED)     # the 32-row family has no multi instance
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    assert call(mk([3, 7, 11])) == 0                             # the same tensors, consistent: runs
    torch.cuda.synchronize()
    assert not any(torch.isnan(o).any() for o in outs)


@pytest.mark.parametrize("B,T,multi_runs", [(3, 40, False), (6, 57, False), (6, 700, True)])
def test_voice_conversion_is_bit_identical_with_and_without_multi_launch(synth_sd, B, T, multi_runs):
    """(3, 40) and (6, 57): every ResBlock launch has fewer than WINO_MIN_ITEMS items, so the switch must change nothing (the
    stages stay on the direct kernels, launch by launch); (6, 700): stages 0-2 are Winograd launches of more items than the
    device has CUs and run as 5 multi + 3 single launches each instead of 18.  Whole tensors and ``skip_padding`` on a ragged batch."""
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG
    model = SynthesizerTrn(0, 513, n_speakers=0, zero_g=False, **CONVERTER_MODEL_CONFIG)
    model.load_state_dict(synth_sd, strict=True)
    model = model.to(DEV).eval()
    eng = model.engine()
    gen = torch.Generator().manual_seed(B * 100 + T)
    spec = (torch.rand(B, 513, T, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]).to(DEV)
    g1, g2 = (0.3 * torch.randn(B, 256, 1, generator=gen).to(DEV) for _ in range(2))
    noise = torch.randn(B, 192, T, generator=gen).to(DEV)
    lengths = torch.tensor([max(1, T - 9 * b) for b in range(B)], dtype=torch.long, device=DEV)
    got = {}
    for multi in (True, False):
        eng.use_multi_launch = multi
        eng.profile = []
        for skip in (False, True):
            got[multi, skip] = model.voice_conversion(spec, lengths, g1, g2, tau=0.3, noise=noise, skip_padding=skip)[0].clone()
        got[multi, "launches"] = len([r for r in eng.profile if r[0] == "mrf"])
        eng.profile = None
    eng.use_multi_launch = True
    torch.cuda.synchronize()
    per_pass = (got[False, "launches"] // 2, got[True, "launches"] // 2)
    assert per_pass == ((66, 36) if multi_runs else (66, 66)), per_pass       # stages 0-2: 18 -> 8 launches each
    for skip in (False, True):
        assert torch.equal(got[True, skip], got[False, skip]), skip
