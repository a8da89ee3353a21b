"""Host side of live streams on the bf16 generator (openvoice_amd/live.py, ``generator="bf16"``): the keyword's values,
that the schedule, the latency and the state size do not depend on it, that the engine-wide switches stay refused, and
the two layout hand-over entry points' argument checks through both bindings.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from openvoice_amd import _lib, live
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG

CFG = CONVERTER_MODEL_CONFIG
HERE = os.path.dirname(os.path.abspath(__file__))
lib_built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built")


class _FakeEngine:
    def __init__(self, bf16=False, split=False):
        self._bf16_on, self._split3_on = bf16, split
        self.device = torch.device("cpu")


class _FakeModel:
    model_cfg = CFG

    def __init__(self, **kw):
        self._e = _FakeEngine(**kw)

    def engine(self):
        return self._e


def test_generator_keyword_values():
    for bad in ("int8", "fp16", "", None, 16, True):
        with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
            live.LivePool(_FakeModel(), generator=bad)
    assert live.LivePool(_FakeModel()).generator == "fp32"
    assert live.LivePool(_FakeModel(), generator="fp32").generator == "fp32"
    assert live.LivePool(_FakeModel(), generator="bf16").generator == "bf16"


@pytest.mark.parametrize("chunk", [15, 60])
def test_bf16_pool_keeps_latency_state_and_layout(chunk):
    p32 = live.LivePool(_FakeModel(), chunk_frames=chunk)
    p16 = live.LivePool(_FakeModel(), chunk_frames=chunk, generator="bf16")
    assert p16.latency_samples == p32.latency_samples == live.live_latency_samples(CFG, chunk)
    if chunk == 15:
        assert p16.latency_samples == 32060
    assert p16.state_bytes_per_stream() == p32.state_bytes_per_stream() > 0
    assert p16.units == p32.units == live.live_units(CFG)
    for name in ("rows", "cap", "width", "ld_in", "ld_out", "cout", "in_off", "out_off", "state_off", "slot_elems",
                 "arena_off", "stage_off"):
        assert getattr(p16, name) == getattr(p32, name), name
    # the constructor leaves the engine alone: the precision belongs to the pool
    m = _FakeModel()
    live.LivePool(m, generator="bf16")
    assert m.engine()._bf16_on is False and m.engine()._split3_on is False


@pytest.mark.parametrize("generator", ["fp32", "bf16"])
def test_engine_wide_switches_stay_refused(generator):
    with pytest.raises(ValueError, match="fp32 generator"):
        live.LivePool(_FakeModel(bf16=True), generator=generator)
    with pytest.raises(ValueError, match="fp32 generator"):
        live.LivePool(_FakeModel(split=True), generator=generator)
    with pytest.raises(ValueError, match="multiple of 15"):
        live.LivePool(_FakeModel(), chunk_frames=20, generator=generator)


def test_the_generator_units_hand_over_multiples_of_32_channels():
    """``ov_rows_f32_to_cl_bf16`` / ``ov_cl_bf16_to_rows_f32`` take C % 32 == 0: every tensor a ``g`` unit reads, and
    every one it writes except the waveform (which the last stage writes in fp32 itself), is such a tensor."""
    pool = live.LivePool(_FakeModel(), generator="bf16")
    g = [k for k, u in enumerate(pool.units) if u["kind"] == "g"]
    assert [pool.rows[k] for k in g] == [192, 256, 128, 64]
    assert [pool.cout[k] for k in g] == [256, 128, 64, 1]
    assert all(pool.rows[k] % 32 == 0 for k in g) and all(pool.cout[k] % 32 == 0 for k in g[:-1])


@lib_built
def test_hand_over_entry_points_are_declared_exported_and_check_their_arguments():
    lib = _lib.load()
    header = open(os.path.join(HERE, "..", "include", "openvoice_amd.h")).read()
    assert "int ov_rows_f32_to_cl_bf16(" in header and "int ov_cl_bf16_to_rows_f32(" in header
    assert lib.ov_version() == int(re.search(r"#define OV_ABI_VERSION (\d+)", header).group(1)) >= _lib.MIN_VERSION
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below fails validation before a launch
    BAD = -1
    fwd, bwd = lib.ov_rows_f32_to_cl_bf16, lib.ov_cl_bf16_to_rows_f32
    # (src, src_bs, src_ld, dst, B, C, L, stream)
    assert fwd(None, 32 * 8, 8, fake, 1, 32, 8, None) == BAD
    assert fwd(fake, 32 * 8, 8, None, 1, 32, 8, None) == BAD
    # (src, dst, dst_bs, dst_ld, B, C, L, stream)
    assert bwd(None, fake, 32 * 8, 8, 1, 32, 8, None) == BAD
    assert bwd(fake, None, 32 * 8, 8, 1, 32, 8, None) == BAD
    for B, C, L, ld, bs in [(0, 32, 8, 8, 256), (65536, 32, 8, 8, 256), (1, 40, 8, 8, 40 * 8), (1, 0, 8, 8, 256),
                            (1, 16, 8, 8, 256), (1, 32, 0, 8, 256), (1, 32, -3, 8, 256), (1, 32, 9, 8, 32 * 9),
                            (2, 32, 8, 8, 255)]:
        assert fwd(fake, bs, ld, fake, B, C, L, None) == BAD, (B, C, L, ld, bs)
        assert bwd(fake, fake, bs, ld, B, C, L, None) == BAD, (B, C, L, ld, bs)


@lib_built
def test_torch_binding_of_the_hand_overs_rejects_cpu_tensors():
    ops = _lib.torch_ops()
    x, y = torch.zeros(32 * 8), torch.zeros(8 * 32, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.rows_f32_to_cl_bf16(x, 32 * 8, 8, y, 1, 32, 8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.cl_bf16_to_rows_f32(y, x, 32 * 8, 8, 1, 32, 8)
    with pytest.raises(RuntimeError, match="no device tensor"):
        ops.rows_f32_to_cl_bf16(None, 32 * 8, 8, None, 1, 32, 8)
