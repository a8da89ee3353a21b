"""CPU side of the per-item ``tau``: the validation helper, the sharding of a per-item ``tau`` across ranks (gloo, with a
stubbed conversion, in the style of tests/test_parallel_gloo.py) and the ABI mirror of ``ov_conv1d_params.scale_b``."""
import ctypes
import inspect
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from openvoice_amd import _lib, tts_engine
from openvoice_amd.engine import item_tau, rows_tau
from openvoice_amd.parallel import convert_sharded, shard_range

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- validation -------------------------------------------------------------------------------------------------------------
def test_item_tau_accepts_a_number_a_sequence_and_a_host_tensor():
    assert tts_engine.item_tau is item_tau                   # next to item_controls, defined where the engine can import it
    assert item_tau(3, 0.3) == 0.3 and isinstance(item_tau(3, 1), float)
    assert item_tau(3, np.float32(0.5)) == 0.5 and item_tau(3, torch.tensor(0.25)) == 0.25
    assert item_tau(3, [0, 0.3, 1.7]) == [0.0, 0.3, 1.7]
    assert item_tau(3, (0.1, 0.2, 0.3)) == [0.1, 0.2, 0.3]
    assert item_tau(2, np.array([0.5, 0.25])) == [0.5, 0.25]
    assert item_tau(2, torch.tensor([0.5, 0.25], dtype=torch.float64)) == [0.5, 0.25]
    assert item_tau(1, [0.7]) == [0.7]


@pytest.mark.parametrize("bad", [[0.1, 0.2], [0.1, 0.2, 0.3, 0.4], [], True, [True, 0.1, 0.2], [0.1, float("nan"), 0.2],
                                 [0.1, float("inf"), 0.2], "abc", "0.3", [0.1, "a", 0.2], None, [[0.1], [0.2], [0.3]],
                                 torch.zeros(3, 1), torch.tensor([True, False, True]), torch.zeros(2),
                                 torch.tensor([0.1, float("nan"), 0.2])],
                         ids=lambda v: repr(v)[:40])
def test_item_tau_raises_overror(bad):
    with pytest.raises(_lib.OvError, match="tau"):
        item_tau(3, bad)


def test_rows_tau_is_the_number_when_the_rows_agree():
    assert rows_tau([0.3, 0.3, 0.3]) == 0.3 and isinstance(rows_tau([1, 1]), float)
    assert rows_tau([0.1, 0.9]) == [0.1, 0.9]


def test_streams_and_requests_take_their_own_tau():
    from openvoice_amd import clone, live, longform
    for cls in (live.LivePool, longform.StreamPool):
        p = inspect.signature(cls.open).parameters["tau"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "tau" in clone._Request.__slots__


def test_a_graph_is_keyed_on_one_tau():
    from openvoice_amd.engine import ConverterEngine
    with pytest.raises(_lib.OvError, match="ungraphed"):
        ConverterEngine.graphed(None, 3, 65, [0.1, 0.3, 0.9])


# ---- sharding ---------------------------------------------------------------------------------------------------------------
N_UTT, HOP = 7, 256


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _stub_converter(calls):
    """A ``ToneColorConverter`` that is only its ``convert_batch_sharded``: ``convert_batch`` is stubbed to write item
    i's tau into every sample of item i (and to record what it was given)."""
    from openvoice_amd.api import ToneColorConverter
    t = object.__new__(ToneColorConverter)
    t.device = "cpu"
    t.model = types.SimpleNamespace(model_cfg={"gin_channels": 4})
    t.hps = types.SimpleNamespace(data=types.SimpleNamespace(hop_length=HOP, filter_length=1024))

    def convert_batch(shard, src_se, tgt_se, tau=0.3, noise=None):
        calls.append(tau)
        n = len(shard)
        taus = torch.full((n,), float(tau)) if isinstance(tau, float) else torch.tensor(tau, dtype=torch.float32)
        assert taus.shape == (n,)
        width = max(len(w) for w in shard) // HOP * HOP
        return taus.view(n, 1, 1).expand(n, 1, width).contiguous(), None
    t.convert_batch = convert_batch
    return t


TAUS = [0.1 * (i + 1) for i in range(N_UTT)]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        calls = []
        t = _stub_converter(calls)
        waves = torch.zeros(N_UTT, 4 * HOP)
        src, tgt = torch.ones(1, 4, 1), torch.zeros(1, 4, 1)
        se = (src, tgt) if rank == 0 else (None, None)
        full = t.convert_batch_sharded(waves, *se, tau=TAUS)
        scalar = t.convert_batch_sharded(waves, *se, tau=0.5)
        ragged, lengths = t.convert_batch_sharded([w[:(2 + i % 3) * HOP] for i, w in enumerate(waves)], *se, tau=tuple(TAUS))
        with pytest.raises(_lib.OvError):
            t.convert_batch_sharded(waves, *se, tau=TAUS[:-1])           # validated against the WHOLE batch on every rank
        torch.save(dict(full=full, scalar=scalar, ragged=ragged, calls=calls), os.path.join(out_dir, f"tau{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("world", [2, 3])
def test_per_item_tau_is_sharded_like_the_waveforms(tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = torch.tensor(TAUS)
    for r in range(world):
        rec = torch.load(tmp_path / f"tau{r}.pt")
        lo, hi = shard_range(N_UTT, r, world)
        assert rec["calls"] == [TAUS[lo:hi], 0.5, TAUS[lo:hi]]          # this rank's contiguous slice; a number as it is
        assert rec["full"].shape == (N_UTT, 1, 4 * HOP)
        assert torch.equal(rec["full"][:, 0, 0], want) and torch.equal(rec["ragged"][:, 0, 0], want)
        assert torch.equal(rec["scalar"], torch.full((N_UTT, 1, 4 * HOP), 0.5))


def test_convert_sharded_without_process_group_hands_tau_on():
    seen = []

    def convert(w, s, t, n, tau):
        seen.append(tau)
        return torch.as_tensor(w).reshape(len(w), 1, -1)
    waves = torch.arange(12.0).reshape(3, 4)
    src, tgt = torch.ones(1, 4, 1), torch.zeros(1, 4, 1)
    convert_sharded(convert, waves, src, tgt, 4, "cpu", tau=[0.1, 0.2, 0.3])
    convert_sharded(convert, waves, src, tgt, 4, "cpu", tau=0.4)
    assert seen == [[0.1, 0.2, 0.3], 0.4]
    with pytest.raises(ValueError):
        convert_sharded(convert, waves, src, tgt, 4, "cpu", tau=[0.1, 0.2])


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built (run __graft_entry__.build())")
def test_conv_params_mirror_ends_with_scale_b():
    header = open(os.path.join(REPO, "include", "openvoice_amd.h")).read()
    body = header[header.index("typedef struct ov_conv1d_params {"):header.index("} ov_conv1d_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.search(r"const float\*\s*scale_b;\s*$", body)                      # the header's last field
    name, ctype = _lib.ConvParams._fields_[-1]
    assert (name, ctype) == ("scale_b", ctypes.c_void_p)
    assert _lib.ConvParams.scale_b.offset == _lib.ConvParams.reserved0.offset + 4
    assert ctypes.sizeof(_lib.ConvParams) == _lib.ConvParams.scale_b.offset + 8
    assert int(re.search(r"OV_F_SCALE_B = (\d+)", header).group(1)) == _lib.F_SCALE_B == 16
    # a launch without OV_F_SCALE_B reads nothing from scale_b on: bad arguments are still refused first, on the host
    p = _lib.ConvParams()
    p.scale_b = 3                                   # misaligned, and not read: flags has no F_SCALE_B
    assert _lib.load().ov_conv1d_f32(ctypes.byref(p), None) == -1
