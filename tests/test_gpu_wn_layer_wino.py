"""The Winograd-domain WaveNet layer (``ov_wn_layer_wino_f32``, openvoice_amd/csrc/wn_layer_wino.hip) against float64
PyTorch of the reference layer (openvoice/modules.py:192-209, commons.py:100-107), through the C ABI.

Every case also runs the direct fused layer (``ov_wn_layer_f32``) on the same inputs; the bar is the rule of
tests/test_gpu_wino.py: max-abs error against float64 <= 16 x the direct kernel's (floor 1e-6).  H = 192 and K = 5 are the
model's; the frame counts are the smallest at which the kernel takes another path: fewer frames than one F(4, 3) tile, T
not a multiple of 4, the k = 5 halo longer than the signal, and one frame either side of the 128-column workgroup tile.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from openvoice_amd import engine as engine_mod  # noqa: E402
from openvoice_amd.engine import launch_wn_layer, wn_fused_row_order, wn_pack, wn_wino_pack  # noqa: E402

DEV = "cuda:0"
H, K, TILE = 192, 5, 128


def _rand(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _weights(seed, last=False, only_second_group=False):
    w_in, b_in = _rand(2 * H, H, K, seed=seed, scale=(K * H) ** -0.5), _rand(2 * H, seed=seed + 1, scale=0.1)
    if only_second_group:          # w0 = w1 = w2 = 0: everything goes through group 1, whose point-infinity product is dropped
        w_in[:, :, :3] = 0
        w_in *= 1.6
    rows = H if last else 2 * H
    return w_in, b_in, _rand(rows, H, 1, seed=seed + 2, scale=H ** -0.5), _rand(rows, seed=seed + 3, scale=0.1)


_PACKED = {}


def _packed(key, w_in, b_in, w_rs, b_rs):
    if key not in _PACKED:
        order = wn_fused_row_order(H)
        if w_rs.shape[0] == H:
            w_rs, b_rs = torch.cat([torch.zeros_like(w_rs), w_rs]), torch.cat([torch.zeros_like(b_rs), b_rs])
        _PACKED[key] = dict(hidden=H, K=K, w_in=wn_pack(w_in[order], DEV), w_in_wino=wn_wino_pack(w_in[order], DEV),
                            b_in=b_in[order].contiguous().to(DEV), w_rs=wn_pack(w_rs, DEV), b_rs=b_rs.contiguous().to(DEV))
    return _PACKED[key]


def _reference(x, g, mask, skip0, w_in, b_in, w_rs, b_rs, first, last):
    d = lambda t: t.double()
    x_in = F.conv1d(d(x), d(w_in), d(b_in), padding=(K - 1) // 2) + d(g)[:, :, None]
    acts = torch.tanh(x_in[:, :H]) * torch.sigmoid(x_in[:, H:])
    rs = F.conv1d(acts, d(w_rs), d(b_rs))
    base = 0 if first else d(skip0)
    if last:
        return None, base + rs
    return (d(x) + rs[:, :H]) * d(mask)[:, None], base + rs[:, H:]


def _both(B, T, lengths, first=False, last=False, seed=20, xscale=1.0, only_second_group=False, poison=()):
    """Runs the Winograd and the direct layer on the same inputs; returns their outputs and the float64 reference.
    ``poison``: columns >= T of the padded rows of h that hold NaN (a caller's stale scratch)."""
    ld = (T + 3) // 4 * 4 + (8 if poison else 0)
    x, skip0 = _rand(B, H, T, seed=seed, scale=xscale), _rand(B, H, T, seed=seed + 1)
    g = _rand(B, 2 * H, seed=seed + 2, scale=0.3)
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).float()
    x = x * mask[:, None]                 # the WN input is always masked (modules.py:207, models.py:216)
    lw = _weights(seed + 3, last, only_second_group)
    layer = _packed((seed, last, only_second_group), *lw)
    x_ref, skip_ref = _reference(x, g, mask, skip0, *lw, first, last)
    pad = lambda t: F.pad(t, (0, ld - T)).contiguous().to(DEV)
    xd, maskd = pad(x), pad(mask)
    for col in poison:
        assert T <= col < ld
        xd[:, :, col] = float("nan")
    gd = g[:, wn_fused_row_order(H)].contiguous().to(DEV)
    res = {}
    for name, wino in (("wino", True), ("direct", False)):
        skipd = pad(skip0 if not first else torch.full_like(skip0, float("nan")))
        outd = torch.full((B, H, ld), float("nan"), device=DEV)
        launch_wn_layer(layer, xd, outd, skipd, maskd, B, T, ld, cond=gd, cond_bs=2 * H, first=first, last=last,
                        mask_bs=ld, row_split=1, winograd=wino)
        torch.cuda.synchronize()
        assert torch.isnan(outd[:, :, T:]).all(), "columns >= T of h' must not be written"
        assert (skipd[:, :, T:].cpu() == 0).all(), "columns >= T of skip must not be written"
        if last:
            assert torch.isnan(outd).all(), "the last layer does not write h'"
        res[name] = (outd[:, :, :T].cpu(), skipd[:, :, :T].cpu())
    return res, x_ref, skip_ref, mask


def _check(res, x_ref, skip_ref, what):
    """e_wino <= max(16 e_direct, 1e-6) for h' and skip; returns the two ratios."""
    ratios = []
    for idx, ref, name in ((0, x_ref, "h'"), (1, skip_ref, "skip")):
        if ref is None:
            continue
        assert torch.isfinite(res["wino"][idx]).all(), f"{what}: {name} not finite"
        e_w = (res["wino"][idx].double() - ref).abs().max().item()
        e_d = (res["direct"][idx].double() - ref).abs().max().item()
        print(f"{what}: {name} e_wino {e_w:.3e} e_direct {e_d:.3e} ratio {e_w / max(e_d, 1e-30):.2f}")
        assert e_w <= max(16 * e_d, 1e-6), (what, name, e_w, e_d)
        ratios.append(e_w / max(e_d, 1e-30))
    return ratios


@pytest.mark.parametrize("T", [1, 3, 4, 5, 7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_frame_counts_around_the_f43_tile_and_the_workgroup_tile(T):
    res, x_ref, skip_ref, _ = _both(2, T, [T, T], seed=20)
    _check(res, x_ref, skip_ref, f"T={T}")


@pytest.mark.parametrize("T", [9, TILE + 1, 2 * TILE + 3])
def test_ragged_batch_with_a_zero_length_utterance(T):
    """Lengths (T, T/2 rounded to odd, 0): masked columns of h' are exactly zero, skip beyond a length is what the direct
    kernel leaves there (bit for bit from 8 columns past the length on, where no F(4, 3) tile touches a non-zero input and
    both kernels see x_in = bias + cond exactly; to rounding in between), and the empty utterance disturbs nobody."""
    lengths = [T, (T // 2) | 1, 0]
    res, x_ref, skip_ref, mask = _both(3, T, lengths, seed=30)
    _check(res, x_ref, skip_ref, f"ragged T={T}")
    ow, sw = res["wino"]
    od, sd = res["direct"]
    assert (ow[mask[:, None].expand_as(ow) == 0] == 0).all()
    assert (ow[2] == 0).all()
    for b, n in enumerate(lengths):
        assert torch.equal(sw[b, :, min(T, n + 8):], sd[b, :, min(T, n + 8):])
        scale = max(1.0, skip_ref[b].abs().max().item())
        assert (sw[b, :, n:] - sd[b, :, n:]).abs().max().item() <= 2e-5 * scale if n < T else True


@pytest.mark.parametrize("first", [False, True])
def test_last_layer_has_skip_rows_only_and_leaves_h_alone(first):
    res, x_ref, skip_ref, _ = _both(2, TILE + 5, [TILE + 5, 77], first=first, last=True, seed=40)
    assert x_ref is None
    _check(res, x_ref, skip_ref, f"last layer first={first}")


def test_first_layer_initialises_skip_over_nan():
    res, x_ref, skip_ref, _ = _both(2, TILE + 5, [TILE + 5, 77], first=True, seed=41)
    _check(res, x_ref, skip_ref, "first layer")


def test_stale_columns_beyond_T_do_not_leak_into_a_tile():
    """T = 133: the last F(4, 3) tile (outputs 132 .. 135) reads input columns 130 .. 137 of rows that are 144 floats long.
    Column 133 -- the first one outside the utterance, INSIDE that tile's input window -- and column 138 -- the first one
    outside the window -- hold NaN, as a caller's stale scratch might; skip starts non-zero (it is accumulated, not
    overwritten).  The reference reads zeros beyond T ('same' padding), so every output column < T is finite and right."""
    T = TILE + 5
    res, x_ref, skip_ref, _ = _both(2, T, [T, T], seed=50, poison=(T, T + 5))
    _check(res, x_ref, skip_ref, "NaN beyond T")


def test_stress_magnitude_input():
    """The layer at the input magnitude of the gain-4 stress model (params.stress_state_dict: 4-fold latents into the flow)."""
    res, x_ref, skip_ref, _ = _both(2, TILE + 1, [TILE + 1, 100], seed=60, xscale=4.0)
    _check(res, x_ref, skip_ref, "stress x4")


def test_weights_in_the_second_group_only_show_the_dropped_product():
    """Only w3, w4 non-zero: the gate conv is group 1 alone, whose point-infinity product is never issued -- were its
    weight not identically zero, the result would be off by whole terms, not by rounding."""
    res, x_ref, skip_ref, _ = _both(2, TILE + 1, [TILE + 1, 100], seed=70, only_second_group=True)
    _check(res, x_ref, skip_ref, "w3, w4 only")


def test_same_inputs_twice_give_the_same_bits():
    a = _both(3, 2 * TILE + 3, [2 * TILE + 3, 131, 0], seed=30)[0]["wino"]
    b = _both(3, 2 * TILE + 3, [2 * TILE + 3, 131, 0], seed=30)[0]["wino"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_entry_point_refuses_what_it_cannot_run():
    from openvoice_amd import _lib
    assert _lib.call("ov_wn_layer_wino_tile") == TILE
    assert _lib.call("ov_wn_wino_pack_size", 2 * H, H, K) > 0 and _lib.call("ov_wn_wino_pack_size", 2 * H, H, 3) == 0
    layer = _packed((20, False, False), *_weights(23))
    x, mask = torch.zeros(1, H, 16, device=DEV), torch.ones(1, 16, device=DEV)
    with pytest.raises(_lib.OvError):
        launch_wn_layer(layer, x, x, torch.zeros_like(x), mask, 1, 16, 16, winograd=True)            # out aliases x
    with pytest.raises(_lib.OvError):
        launch_wn_layer(layer, x, torch.zeros_like(x), torch.zeros_like(x), mask, 1, 16, 16, width=64, winograd=True)
    with pytest.raises(_lib.OvError):
        launch_wn_layer(dict(layer, K=3), x, torch.zeros_like(x), torch.zeros_like(x), mask, 1, 16, 16, winograd=True)


def test_engine_policy(synth_sd, monkeypatch):
    """The Winograd layer runs where its rounds of (utterance, 128-column tile) items are WN_WINO_MIN_ITEMS full; ``use_winograd = False`` switches
    it off (every launch is then the parent's direct layer, which this change leaves byte for byte alone); batch 1 stays on
    the launcher's row-split pair (row_split = 0 with the ``acts`` scratch: tests/test_gpu_wn_layer.py)."""
    from openvoice_amd.engine import WN_WINO_MIN_ITEMS, ConverterEngine, wn_wino_items, wn_wino_policy
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    assert wn_wino_items(32, 861) == 224 >= WN_WINO_MIN_ITEMS and wn_wino_policy(32, 861)
    assert not any(wn_wino_policy(B, 861) for B in (1, 2, 4, 8, 16))
    assert not wn_wino_policy(37, 861) and wn_wino_policy(48, 861)      # 259 items: a second round that is almost empty
    seen = []
    real = engine_mod.launch_wn_layer

    def spy(*a, **kw):
        seen.append((kw.get("winograd", False), kw.get("row_split"), kw.get("acts") is not None))
        return real(*a, **kw)

    monkeypatch.setattr(engine_mod, "launch_wn_layer", spy)
    gen = torch.Generator().manual_seed(5)
    B, T = 2, 130
    spec = (torch.randn(B, 513, T, generator=gen).abs() * torch.linspace(3, 0.05, 513)[None, :, None]).to(DEV)
    lengths = torch.tensor([T, 97], dtype=torch.int64, device=DEV)
    g1, g2 = (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)
    noise = torch.randn(B, 192, T, generator=gen).to(DEV)
    eng = ConverterEngine(synth_sd, CFG, 513, DEV, zero_g=True)
    run = lambda: [t.clone() for t in eng.voice_conversion(spec, lengths, g1, g2, tau=0.3, noise=noise)[2]]
    base = run()                                                 # 4 items: below the threshold
    assert seen and not any(w for w, _, _ in seen) and all(rs == 0 and acts for _, rs, acts in seen)
    monkeypatch.setattr(engine_mod, "WN_WINO_MIN_ITEMS", 1)
    seen.clear()
    wino = run()
    assert seen and all(w for w, _, _ in seen)
    eng.use_winograd = False
    seen.clear()
    off = run()
    assert seen and not any(w for w, _, _ in seen)
    for a, b, c in zip(base, wino, off):
        assert torch.equal(a, c)                                 # the switch restores the direct path's bits
        assert (a - b).abs().max().item() <= 1e-4 * max(1.0, a.abs().max().item())
