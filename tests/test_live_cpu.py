"""Host side of low-latency live streams (openvoice_amd/live.py): the unit table's reaches by perturbation against the
CPU oracle, the cascade schedule emulated with oracle units in float64 against one-pass voice_conversion, the latency
bound, the carry kernel's ABI and the argument checks.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vc_oracle
from openvoice_amd import _lib, live
from openvoice_amd.params import synthetic_state_dict
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG

CFG = CONVERTER_MODEL_CONFIG
HOP, NFFT, PAD = 256, 1024, 384
HERE = os.path.dirname(os.path.abspath(__file__))
lib_built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built")


def _weight64(sd, prefix):
    """``effective_weight`` in float64 (the oracle's own folds to float32)."""
    if prefix + ".weight" in sd:
        return sd[prefix + ".weight"].double()
    v, g = sd[prefix + ".weight_v"].double(), sd[prefix + ".weight_g"].double()
    return v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape))


@pytest.fixture(scope="module")
def sd():
    saved = vc_oracle.effective_weight
    vc_oracle.effective_weight = _weight64          # the oracle units in float64
    yield {k: v.double() for k, v in synthetic_state_dict(CFG, 513, seed=5).items()}
    vc_oracle.effective_weight = saved


def _g(seed):
    gen = torch.Generator().manual_seed(seed)
    return 0.3 * torch.randn(1, 256, 1, generator=gen, dtype=torch.float64)


def _stage(sd, i, x, g_tgt):
    """Generator stage i as a unit (oracle.generator restated per stage from resblock1 and torch functional ops)."""
    kernels, dils = CFG["resblock_kernel_sizes"], CFG["resblock_dilation_sizes"]
    u, k = CFG["upsample_rates"][i], CFG["upsample_kernel_sizes"][i]
    if i == 0:
        x = F.conv1d(x, sd["dec.conv_pre.weight"], sd["dec.conv_pre.bias"], padding=3)
        x = x + F.conv1d(g_tgt, sd["dec.cond.weight"], sd["dec.cond.bias"])
    x = F.leaky_relu(x, 0.1)
    x = F.conv_transpose1d(x, _weight64(sd, f"dec.ups.{i}"), sd[f"dec.ups.{i}.bias"], stride=u,
                           padding=(k - u) // 2)
    xs = None
    for j, (rk, rd) in enumerate(zip(kernels, dils)):
        y = vc_oracle.resblock1(sd, f"dec.resblocks.{i * len(kernels) + j}", x, rk, rd)
        xs = y if xs is None else xs + y
    x = xs / len(kernels)
    if i == len(CFG["upsample_rates"]) - 1:
        x = torch.tanh(F.conv1d(F.leaky_relu(x), sd["dec.conv_post.weight"], None, padding=3))
    return x


def _unit(sd, u, x, noise, g_src, g_tgt, tau):
    """Run unit ``u`` of the table on the buffer ``x`` [1, C, L] (``noise`` the posterior's noise columns)."""
    mask = torch.ones(1, 1, x.shape[2], dtype=x.dtype)
    if u["kind"] == "q":
        return vc_oracle.posterior_encoder(sd, x, mask, g_src, noise, tau)
    if u["kind"] == "f":
        return vc_oracle.flow(sd, x, mask, g_src, False)
    if u["kind"] == "r":
        return vc_oracle.flow(sd, x, mask, g_tgt, True)
    return _stage(sd, u["stage"], x, g_tgt)


def _unit_input(sd, u, L, seed):
    gen = torch.Generator().manual_seed(seed)
    rows = {"q": 513, "f": 192, "r": 192}.get(u["kind"])
    if rows is None:
        rows = 192 if u["stage"] == 0 else CFG["upsample_initial_channel"] >> u["stage"]
    x = torch.randn(1, rows, L, generator=gen, dtype=torch.float64)
    return x.abs() if u["kind"] == "q" else x


# ---- the unit table -------------------------------------------------------------------------------------------------
def test_unit_table_released_config():
    table = {u["name"]: (u["rate"], u["stride"], u["left"], u["right"], u["align"]) for u in live.live_units(CFG)}
    assert table == {"q": (1, 1, 32, 32, 1), "f": (1, 1, 32, 32, 1), "r": (1, 1, 32, 32, 1), "g0": (1, 8, 11, 11, 15),
                     "g1": (8, 8, 8, 8, 15), "g2": (64, 2, 31, 31, 30), "g3": (128, 2, 32, 32, 30)}
    for u in live.live_units(CFG):       # the buffer start's output column sits on the stage's Winograd tile grid
        if u["kind"] == "g":
            assert u["align"] * u["stride"] % 60 == 0


@pytest.mark.parametrize("name", ["q", "f", "r", "g0", "g1", "g2", "g3"])
def test_unit_reach_by_perturbation(sd, name):
    """Perturb one input column: every output column beyond the stated reach is unchanged, and the reach is tight."""
    u = next(v for v in live.live_units(CFG) if v["name"] == name)
    L = 2 * max(u["left"], u["right"]) + 24 if u["kind"] != "g" or u["stage"] < 2 else 2 * u["left"] + 12
    x = _unit_input(sd, u, L, 1)
    noise = torch.randn(1, 192, L, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    g_src, g_tgt = _g(3), _g(4)
    with torch.no_grad():
        y0 = _unit(sd, u, x, noise, g_src, g_tgt, 0.3)
        p = L // 2
        x1 = x.clone()
        x1[:, :, p] += 0.5
        y1 = _unit(sd, u, x1, noise, g_src, g_tgt, 0.3)
    s = u["stride"]
    changed = ((y1 - y0).abs().amax(dim=1)[0] > 0).nonzero().flatten()
    q = changed // s                              # input column each changed output column belongs to
    # output column j (input column j // s) may depend on input columns [j // s - left, j // s + right]
    assert int(q.min()) >= p - u["right"] and int(q.max()) <= p + u["left"]
    assert int(q.min()) == p - u["right"] and int(q.max()) == p + u["left"]


# ---- the cascade against one pass -----------------------------------------------------------------------------------
def _emulate(sd, wave, chunk, pushes, noise, g_src, g_tgt, tau):
    """The plan's chunk schedule with oracle units: frames become available as the samples arrive (interior frames
    only, the rest at close), every unit runs its pieces on its own stored buffer.  Returns the output and, per
    emitted sample, the samples received when it left."""
    units = live.live_units(CFG)
    spec_all = vc_oracle.spectrogram(wave[None].double())          # interior frames equal the whole file's
    N = wave.numel()
    T = spec_all.shape[2]
    cas = live.Cascade(units, chunk)
    store = [None] * len(units)                                    # per unit: (first column, [1, C, n] input so far)
    outs, when, n = [], [], 0

    def run(pieces, n_recv):
        for k, b0, end, e0, e1 in pieces:
            s0, buf = store[k]
            assert b0 >= s0 and end - b0 <= cas.width(k) and buf.shape[2] + s0 - cas.s0[k] <= cas.capacity(k) + 0
            x = buf[:, :, b0 - s0:end - s0]
            nz = noise[:, :, b0:end] if units[k]["kind"] == "q" else None
            y = _unit(sd, units[k], x, nz, g_src, g_tgt, tau)
            st = units[k]["stride"]
            y = y[:, :, (e0 - b0) * st:(e1 - b0) * st]
            keep = live._start(units[k], e1)
            store[k] = (keep, buf[:, :, keep - s0:])
            if k + 1 < len(units):
                s1, b1 = store[k + 1] if store[k + 1] is not None else (0, y[:, :, :0])
                store[k + 1] = (s1, torch.cat([b1, y], 2))
            else:
                outs.append(y.reshape(-1))
                when.extend([n_recv] * y.numel())

    def feed(nf, final, n_recv):
        f0 = cas.n[0]
        s0, b = store[0] if store[0] is not None else (0, spec_all[:, :, :0])
        store[0] = (s0, torch.cat([b, spec_all[:, :, f0:f0 + nf]], 2))
        run(cas.round(nf, final), n_recv)

    for m in pushes + [N]:
        n = min(N, n + m) if m != N else N
        while live.interior_frames(n, NFFT, HOP) >= cas.n[0] + chunk:
            feed(chunk, False, n)
        if n == N:
            break
    while not cas.done:
        nf = min(chunk, T - cas.n[0])
        feed(nf, cas.n[0] + nf == T, N)
    return torch.cat(outs), when


@pytest.mark.parametrize("chunk,n", [(15, 256 * 60 + 100), (30, 256 * 97 + 13), (60, 256 * 75 + 255), (15, 256 * 11)])
def test_cascade_equals_one_pass(sd, chunk, n):
    gen = torch.Generator().manual_seed(n)
    wave = (0.3 * torch.randn(n, generator=gen, dtype=torch.float64)).clamp(-1, 1)
    T = (n + 2 * PAD - NFFT) // HOP + 1
    noise = torch.randn(1, 192, T, generator=gen, dtype=torch.float64)
    g_src, g_tgt = _g(11), _g(12)
    rng = np.random.default_rng(n)
    pushes = [int(v) for v in rng.integers(1, 3000, size=n // 800 + 2)]
    with torch.no_grad():
        out, _ = _emulate(sd, wave, chunk, pushes, noise, g_src, g_tgt, 0.3)
        spec = vc_oracle.spectrogram(wave[None])
        ref = vc_oracle.voice_conversion(sd, CFG, spec, torch.tensor([T]), g_src, g_tgt, 0.3, noise)[0].reshape(-1)
    assert out.shape == ref.shape
    assert (out - ref).abs().max().item() <= 1e-12


def test_schedule_latency_bound_for_any_push_sizes():
    """Host schedule only (no model): every output sample leaves within latency_samples of its input sample."""
    for chunk in (15, 30, 60):
        lat = live.live_latency_samples(CFG, chunk)
        R = live.live_right_samples(CFG)
        for seed in range(4):
            rng = np.random.default_rng(seed)
            N = 256 * 700 + int(rng.integers(0, 256))
            n = 0
            cas = live.Cascade(live.live_units(CFG), chunk)
            tight = False
            while n < N:
                n = min(N, n + int(rng.integers(1, 6000 if seed else 2)))  # seed 0: one sample at a time
                while live.interior_frames(n, NFFT, HOP) >= cas.n[0] + chunk:
                    cas.round(chunk)
                out = max(0, HOP * cas.n[0] - R)
                # output sample t has left once t + latency_samples input samples have arrived
                assert out >= n - lat + 1, (chunk, seed, n, out)
                tight = tight or out == n - lat + 1
            assert tight or seed > 0         # one sample at a time reaches the bound
    assert live.live_latency_samples(CFG, 15) <= int(1.5 * 22050)
    assert live.live_latency_samples(CFG, 15) == 32060


def test_schedule_emits_what_the_cascade_emits():
    """The closed-form output count the latency proof uses equals the cascade's own emission."""
    cas = live.Cascade(live.live_units(CFG), 15)
    total = 0
    for r in range(20):
        for k, b0, end, e0, e1 in cas.round(15):
            if k == len(cas.units) - 1:
                total += (e1 - e0) * 2
        assert total == max(0, HOP * cas.n[0] - live.live_right_samples(CFG))


# ---- ABI and arguments ----------------------------------------------------------------------------------------------
@lib_built
def test_carry_entry_point_is_exported_and_version_is_2_12():
    lib = _lib.load()
    assert lib.ov_version() == 212 == _lib.MIN_VERSION
    header = open(os.path.join(HERE, "..", "include", "openvoice_amd.h")).read()
    assert int(re.search(r"#define OV_ABI_VERSION (\d+)", header).group(1)) == 212
    assert "int ov_carry_rows_f32(" in header
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below fails validation before a launch
    f = lib.ov_carry_rows_f32
    assert f(None, 1, fake, 8, fake, 8, None) == -1
    assert f(fake, 0, fake, 8, fake, 8, None) == -1
    assert f(fake, 65536, fake, 8, fake, 8, None) == -1
    assert f(fake, 1, None, 8, fake, 8, None) == -1
    assert f(fake, 1, fake, 0, fake, 8, None) == -1
    assert f(fake, 1, fake, 8, None, 8, None) == -1
    assert f(fake, 1, fake, 8, fake, 0, None) == -1


@lib_built
def test_torch_binding_of_the_carry_rejects_cpu_tensors():
    ops = _lib.torch_ops()
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.carry_rows_f32(torch.zeros(1, 6, dtype=torch.long), 1, torch.zeros(8), 8, torch.zeros(8), 8)


def test_bad_chunk_frames_raise():
    for c in (0, -15, 16, 7, 15.0, None, True):
        with pytest.raises(ValueError):
            live.live_latency_samples(CFG, c)
    assert live.check_chunk(CFG, 45) == 45


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


def test_unsupported_engine_modes_raise():
    with pytest.raises(ValueError, match="fp32 generator"):
        live.LivePool(_FakeModel(bf16=True))
    with pytest.raises(ValueError, match="fp32 generator"):
        live.LivePool(_FakeModel(split=True))
    with pytest.raises(ValueError, match="multiple of 15"):
        live.LivePool(_FakeModel(), chunk_frames=20)
    pool = live.LivePool(_FakeModel(), chunk_frames=15)
    assert pool.latency_samples == 32060 and pool.state_bytes_per_stream() > 0
