"""CPU-side checks of the bf16 WaveNet layer's entry points (include/openvoice_amd.h: ov_wn_layer_bf16 and its helpers)
and of the ``wavenet=`` keyword's validation.  The symbols are additive within ABI 2.12, like every entry point added
since: the version the header, the library and the binding state stays the same."""
import os
import re
import sys

import pytest
import torch

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
from openvoice_amd import _lib  # noqa: E402

NEW = ("ov_wn_layer_bf16", "ov_wn_layer_bf16_supported", "ov_wn_bf16_pack_size", "ov_wn_bf16_pack", "ov_wn_layer_bf16_tile")


def test_version_and_new_symbols():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "openvoice_amd.h")).read()
    macro = int(re.search(r"#define OV_ABI_VERSION (\d+)", header).group(1))
    assert lib.ov_version() == macro == _lib.MIN_VERSION
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"^(?:int|size_t)\s+{name}\s*\(", header, flags=re.M), f"{name} not declared"
    assert "modules.py:192-209" in header[header.index("on the bf16 matrix pipe") - 200:header.index("int ov_wn_layer_bf16(")]


def test_supported_and_tile_queries():
    lib = _lib.load()
    assert lib.ov_wn_layer_bf16_supported(192, 5) == 1
    for H, K in ((192, 3), (192, 7), (128, 5), (256, 5), (0, 0), (191, 5)):
        assert lib.ov_wn_layer_bf16_supported(H, K) == 0, (H, K)
    for width in range(16, 129, 16):
        assert lib.ov_wn_layer_bf16_tile(4, 100, width) == width
    for width in (8, 24, 144, 100):
        assert lib.ov_wn_layer_bf16_tile(4, 100, width) == 0
    assert lib.ov_wn_bf16_pack_size(384, 192, 5) == 8 * 31 * 3 * 64 * 8
    assert lib.ov_wn_bf16_pack_size(384, 192, 1) == 8 * 7 * 3 * 64 * 8
    assert lib.ov_wn_bf16_pack_size(100, 192, 5) == 0 and lib.ov_wn_bf16_pack_size(384, 100, 5) == 0


@pytest.mark.parametrize("rows,cin,K", [(384, 192, 5), (384, 192, 1), (128, 32, 3)])
def test_pack_is_a_permutation_of_the_rounded_weights(rows, cin, K):
    """Every weight appears exactly once, with the bits of torch's bf16 cast (nearest even); the rest is the zero padding
    that closes each wave's stream; a spot check pins the documented fragment order."""
    w = torch.randn(rows, cin, K, generator=torch.Generator().manual_seed(rows + K))
    w[0, 0, 0], w[1, 0, 0] = 1.00390625, 1.01171875          # ties: 1 + 2^-8 -> even (down), 1 + 3 * 2^-8 -> even (up)
    # compared as multisets of bit patterns: a weight packed twice, dropped or rounded differently changes the multiset
    want = w.to(torch.bfloat16).view(torch.int16).to(torch.int32).flatten()
    n = _lib.call("ov_wn_bf16_pack_size", rows, cin, K)
    dst = torch.full((n,), 0x7fff, dtype=torch.int16)
    _lib.call("ov_wn_bf16_pack", w.contiguous(), rows, cin, K, dst.view(torch.bfloat16))
    got = dst.to(torch.int32)
    pad = n - w.numel()
    assert pad == 8 * (rows // 128) * 64 * 8 and int((got == 0).sum()) >= pad
    assert torch.equal(torch.sort(got)[0], torch.sort(torch.cat([want, torch.zeros(pad, dtype=torch.int32)]))[0])
    # [wave][k-step = chunk * K + tap][fragment][lane][8]: row = (wave * rb + frag) * 16 + (lane & 15), channel = 32 chunk + 8 (lane >> 4) + e
    rb, ns = rows // 128, (cin // 32) * K
    wb = w.to(torch.bfloat16).view(torch.int16).to(torch.int32)
    for wave, s, frag, lane, e in ((0, 0, 0, 0, 0), (7, ns - 1, rb - 1, 63, 7), (3, ns // 2, 0, 37, 5)):
        row, ci, tap = (wave * rb + frag) * 16 + (lane & 15), 32 * (s // K) + 8 * (lane >> 4) + e, s % K
        assert got[((((wave * (ns + 1) + s) * rb + frag) * 64 + lane) * 8 + e)] == wb[row, ci, tap]
    assert (got.view(8, ns + 1, -1)[:, ns] == 0).all()        # the closing zero k-step of every wave


def test_pack_rejects_bad_arguments():
    lib = _lib.load()
    w = torch.zeros(384 * 192 * 5)
    assert lib.ov_wn_bf16_pack(None, 384, 192, 5, w.data_ptr()) == -1
    assert lib.ov_wn_bf16_pack(w.data_ptr(), 100, 192, 5, w.data_ptr()) == -1


def test_check_wavenet():
    assert _lib.check_wavenet("fp32") == "fp32" and _lib.check_wavenet("bf16") == "bf16"
    assert _lib.check_wavenet(None, optional=True) is None
    for junk in (None, "BF16", "fp16", 16, True, b"bf16", ""):
        with pytest.raises(_lib.OvError):
            _lib.check_wavenet(junk)
    for junk in ("half", 0, ["bf16"]):
        with pytest.raises(_lib.OvError):
            _lib.check_wavenet(junk, optional=True)
    assert _lib.wavenet_kw(None) == {} and _lib.wavenet_kw("bf16") == {"wavenet": "bf16"}
