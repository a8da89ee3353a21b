"""Host side of many-voice enrolment (``se_extractor.get_se_many`` -> ``ToneColorConverter.extract_se_many`` ->
``ConverterEngine.reference_encoder_ragged`` -> csrc/ref_enc_ragged.hip), without a GPU: the per-layer length
recurrence against PyTorch's own conv2d output sizes, the chunk plan, the argument errors that are raised before
anything touches a device, and the three new C entry points' own argument checks (no call here can launch)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openvoice_amd import _lib, api, se_extractor
from openvoice_amd.engine import ref_enc_lengths
from openvoice_amd.params import REF_ENC_FILTERS

OV_E_BADARG, OV_E_UNSUPPORTED = -1, -2


# ---- the length table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", range(1, 41))
def test_ref_enc_lengths_are_conv2d_output_sizes(T):
    """``ref_enc_lengths(T, n)`` = [T, then the time size after each of n 3x3 stride-2 pad-1 convs], as
    ``torch.nn.functional.conv2d`` itself sizes its output."""
    x = torch.zeros(1, 1, T, 5)
    want = [T]
    for _ in range(6):
        x = F.conv2d(x, torch.zeros(1, 1, 3, 3), stride=2, padding=1)
        want.append(x.shape[2])
    assert ref_enc_lengths(T, 6) == want
    assert ref_enc_lengths(T) == want and len(REF_ENC_FILTERS) == 6
    assert ref_enc_lengths(T, 0) == [T] and ref_enc_lengths(T, 2) == want[:3]


def test_ref_enc_lengths_is_monotone_and_rejects_empty_items():
    """A shorter item never has more frames than a longer one at any layer (what lets one row stride per layer, the
    longest item's, hold every item), and T < 1 is refused."""
    rows = [ref_enc_lengths(T) for T in range(1, 900)]
    for a, b in zip(rows, rows[1:]):
        assert all(x <= y for x, y in zip(a, b))
    assert ref_enc_lengths(861)[-1] == 14
    for bad in (0, -3):
        with pytest.raises(ValueError):
            ref_enc_lengths(bad)


# ---- the chunk plan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap", [(1, 1), (1, 64), (9, 1), (9, 2), (9, 4), (9, 9), (9, 64), (64, 64), (65, 64),
                                   (300, 64)])
def test_chunk_plan_keeps_order_and_respects_the_cap(n, cap):
    plan = api.plan_enrol_chunks(n, cap)
    assert [i for lo, hi in plan for i in range(lo, hi)] == list(range(n)), "every piece once, in the caller's order"
    assert all(1 <= hi - lo <= cap for lo, hi in plan)
    assert len(plan) == -(-n // cap), "no more launches than the cap forces"
    if cap == 1:
        assert plan == [(i, i + 1) for i in range(n)]


def test_chunk_plan_rejects_a_cap_below_one():
    for cap in (0, -1):
        with pytest.raises(ValueError, match="max_pieces_per_launch"):
            api.plan_enrol_chunks(5, cap)
    assert api.plan_enrol_chunks(0, 4) == []


# ---- argument errors, raised before a device is touched -----------------------------------------------------------------
def _bare_converter():
    """A ToneColorConverter without a model or a device: the argument checks of ``extract_se_many`` come first and
    need neither (the constructor itself refuses to run without a GPU)."""
    return api.ToneColorConverter.__new__(api.ToneColorConverter)


def test_extract_se_many_argument_errors():
    tcc = _bare_converter()
    wave = np.zeros(4000, dtype=np.float32)
    with pytest.raises(ValueError, match="non-empty list"):
        tcc.extract_se_many([])
    with pytest.raises(ValueError, match="voice 1 has no pieces"):
        tcc.extract_se_many([[wave], []])
    with pytest.raises(ValueError, match="piece 1 of voice 0"):
        tcc.extract_se_many([[wave, np.zeros(0, dtype=np.float32)]])
    with pytest.raises(ValueError, match="piece 0 of voice 0"):
        tcc.extract_se_many([[torch.zeros(2, 4000)]])
    with pytest.raises(ValueError, match="voice 0 is a waveform"):
        tcc.extract_se_many([wave])
    with pytest.raises(ValueError, match="max_pieces_per_launch"):
        tcc.extract_se_many([[wave]], max_pieces_per_launch=0)


def test_flatten_voices_keeps_the_callers_order():
    a, b, c, d = (np.full(n, float(n), dtype=np.float32) for n in (3, 4, 5, 6))
    counts, flat = api._flatten_voices([[a], [b, c], [torch.from_numpy(d)]])
    assert counts == [1, 2, 1]
    assert [len(x) for x in flat] == [3, 4, 5, 6]


def test_get_se_many_argument_errors(tmp_path):
    tcc = _bare_converter()
    with pytest.raises(ValueError, match="non-empty list"):
        se_extractor.get_se_many([], tcc, target_dir=str(tmp_path))
    with pytest.raises(ValueError, match="non-empty list"):
        se_extractor.get_se_many("one.wav", tcc, target_dir=str(tmp_path))
    assert not os.listdir(tmp_path), "a refused call writes nothing"


def test_get_se_many_is_re_exported_by_the_alias_package():
    from openvoice import se_extractor as alias
    assert alias.get_se_many is se_extractor.get_se_many and alias.get_se is se_extractor.get_se


# ---- the C entry points' own checks ------------------------------------------------------------------------------------
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                               reason="libopenvoice_amd.so not built (run __graft_entry__.build())")


@needs_lib
def test_ragged_entry_points_reject_bad_arguments_without_a_gpu():
    """Null pointers (``lens`` included), N > 65535 and non-positive extents are refused before any launch; the
    made-up addresses are never dereferenced because every call here is refused."""
    lib = _lib.load()
    p = [0x10000 * (i + 1) for i in range(5)]                 # x, gamma / w, beta / bias, lens, y

    ln = lib.ov_layernorm_freq_ragged_f32
    assert ln(None, None, None, None, None, 1, 1, 1, 1e-5, None) == OV_E_BADARG
    for i in range(5):
        args = list(p)
        args[i] = None
        assert ln(*args, 2, 7, 5, 1e-5, None) == OV_E_BADARG, f"layernorm: null pointer {i}"
    for N, Fq, ld in ((0, 7, 5), (65536, 7, 5), (-1, 7, 5), (2, 0, 5), (2, 7, 0)):
        assert ln(*p, N, Fq, ld, 1e-5, None) == OV_E_BADARG, (N, Fq, ld)

    conv = lib.ov_conv2d_s2_relu_ragged_f32
    assert conv(None, None, None, None, None, 1, 1, 16, 1, 1, 1, None) == OV_E_BADARG
    for i in range(5):
        args = list(p)
        args[i] = None
        assert conv(*args, 2, 16, 16, 4, 6, 3, None) == OV_E_BADARG, f"conv: null pointer {i}"
    for dims in ((0, 16, 16, 4, 6, 3), (65536, 16, 16, 4, 6, 3), (2, 0, 16, 4, 6, 3), (2, 16, 0, 4, 6, 3),
                 (2, 16, 16, 0, 6, 3), (2, 16, 16, 4, 0, 3), (2, 16, 16, 4, 6, 2), (2, 16, 16, 4, 7, 3)):
        assert conv(*p, *dims, None) == OV_E_BADARG, dims      # the last two: ld_out below (ld_in - 1) / 2 + 1
    assert conv(*p, 1, 16, 24, 4, 6, 3, None) == OV_E_UNSUPPORTED, "Cout = 24"

    gru = lib.ov_gru_ragged_f32
    assert gru(None, None, None, None, None, 1, 128, 1, None) == OV_E_BADARG
    for i in range(5):
        args = list(p)
        args[i] = None
        assert gru(*args, 2, 128, 3, None) == OV_E_BADARG, f"gru: null pointer {i}"
    for N, ld in ((0, 3), (-1, 3), (65536, 3), (2, 0)):
        assert gru(*p, N, 128, ld, None) == OV_E_BADARG, (N, ld)
    assert gru(*p, 2, 64, 3, None) == OV_E_UNSUPPORTED, "H = 64"


@needs_lib
def test_ragged_entry_points_are_declared_bound_and_additive():
    """Header, ctypes table and torch ops carry the three names; the ABI version did not move."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "openvoice_amd.h")).read()
    ops = _lib.torch_ops()
    for name in ("ov_layernorm_freq_ragged_f32", "ov_conv2d_s2_relu_ragged_f32", "ov_gru_ragged_f32"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(ops, name[3:])
    assert "#define OV_ABI_VERSION 212" in header and _lib.MIN_VERSION == 212
    assert str(ops.gru_ragged_f32.default._schema) == (
        "openvoice_amd::gru_ragged_f32(Tensor? a0, Tensor? a1, Tensor? a2, Tensor? a3, Tensor(a4!)? a4, int a5, "
        "int a6, int a7) -> ()")
