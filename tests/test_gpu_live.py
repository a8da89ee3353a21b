"""Low-latency live streams on the MI355X (openvoice_amd/live.py): the state-carry kernel against torch slicing through
both bindings, a live stream against convert_long of the same input and noise, push-pattern independence, and a pool
of streams against solo streams."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, live  # noqa: E402

DEV = "cuda:0"
O_HAT_TOL = 1e-4


@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("live")
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


@pytest.fixture
def direct(tcc):
    eng = tcc.model.engine()
    saved = eng.use_winograd
    eng.use_winograd = False
    yield
    eng.use_winograd = saved


def _ses(seed):
    gen = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


def _wave(n, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    phase = 2 * np.pi * torch.cumsum(140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / 22050.0
    y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float().to(DEV)


def _noise(T, seed):
    return torch.randn(1, 192, T, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _frames(n):
    return (n + 2 * 384 - 1024) // 256 + 1


# ---- ov_carry_rows_f32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_carry_rows_matches_torch_slicing(binding, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    gen = torch.Generator().manual_seed(7)
    S, D = 200_003, 150_001
    src = torch.randn(S, generator=gen).to(DEV)
    dst = torch.full((D,), -7.0).to(DEV)
    ref = dst.clone().cpu()
    s_cpu = src.cpu()
    recs, used = [], torch.zeros(D, dtype=torch.bool)
    while len(recs) < 300:
        rows = int(torch.randint(1, 9, (1,), generator=gen))
        cols = int(torch.randint(1, 130, (1,), generator=gen))
        sld = cols + int(torch.randint(0, 9, (1,), generator=gen))
        dld = cols + int(torch.randint(0, 9, (1,), generator=gen))
        so = int(torch.randint(0, S - rows * sld, (1,), generator=gen))
        do = int(torch.randint(0, D - rows * dld, (1,), generator=gen))
        if len(recs) % 3 == 0:                     # aligned: the vector path
            so, do, sld, dld = so // 4 * 4, do // 4 * 4, (sld + 3) // 4 * 4, (dld + 3) // 4 * 4
        idx = torch.tensor([do + i * dld + j for i in range(rows) for j in range(cols)])
        if used[idx].any():
            continue                               # destinations of one launch never overlap
        used[idx] = True
        recs.append((so, do, rows, cols, sld, dld))
        for i in range(rows):
            ref[do + i * dld:do + i * dld + cols] = s_cpu[so + i * sld:so + i * sld + cols]
    # out of range: source past the end (destination in range) -> zeros; destination past the end -> untouched
    free = (~used).nonzero().flatten()
    z = int(free[free < D - 40][0])
    while used[z:z + 4].any():
        z += 1
    recs.append((S - 2, z, 1, 4, 4, 4))
    used[z:z + 4] = True
    ref[z:z + 4] = 0.0
    recs.append((0, D - 3, 1, 4, 4, 4))
    recs.append((-4, 0, 1, 4, 4, 4))              # negative source offset: destination in range but bad record -> nothing
    table = torch.tensor(recs, dtype=torch.int64).to(DEV)
    _lib.call("ov_carry_rows_f32", table, len(recs), src, S, dst, D)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), ref)


def test_carry_rows_rejects_bad_host_arguments():
    t = torch.zeros(4, 6, dtype=torch.int64, device=DEV)
    x = torch.zeros(64, device=DEV)
    for args in [(t, 0, x, 64, x, 64), (t, 65536, x, 64, x, 64), (t, 1, x, 0, x, 64), (t, 1, x, 64, x, 0)]:
        with pytest.raises(_lib.OvError):
            _lib.call("ov_carry_rows_f32", *args)


# ---- a live stream against convert_long -------------------------------------------------------------------------------
def _run_stream(st, wave, pushes):
    outs, i = [], 0
    for n in pushes:
        outs.append(st.push(wave[i:i + n]))
        i += n
    outs.append(st.push(wave[i:]))
    outs.append(st.close())
    return torch.cat(outs)


def _pushes(n, seed, lo=100, hi=9000):
    gen = np.random.default_rng(seed)
    out, acc = [], 0
    while acc < n:
        k = int(gen.integers(lo, hi))
        out.append(k)
        acc += k
    return out


@pytest.mark.parametrize("chunk", [15, 60])
def test_live_stream_equals_convert_long_bitwise_with_direct_kernels(tcc, direct, chunk):
    src, tgt = _ses(1)
    for n in [256 * 9 + 100, 256 * 700 + 13]:
        wave = _wave(n, n)
        noise = _noise(_frames(n), n)
        ref = torch.as_tensor(tcc.convert_long(wave, src, tgt, noise=noise)).to(DEV)
        st = tcc.live_stream(src, tgt, chunk_frames=chunk, noise=noise)
        out = _run_stream(st, wave, _pushes(n, n + chunk))
        assert out.shape == ref.shape
        assert torch.equal(out, ref), (n, chunk, (out - ref).abs().max().item())


@pytest.mark.parametrize("chunk", [15, 60])
def test_live_stream_matches_convert_long_with_default_kernels(tcc, chunk):
    src, tgt = _ses(2)
    lengths = [256 * 9 + 100, 256 * 300 + 77] + ([22050 * 20 + 5] if chunk == 60 else [])
    for n in lengths:
        wave = _wave(n, n)
        noise = _noise(_frames(n), n)
        ref = torch.as_tensor(tcc.convert_long(wave, src, tgt, noise=noise)).to(DEV)
        st = tcc.live_stream(src, tgt, chunk_frames=chunk, noise=noise)
        out = _run_stream(st, wave, [2205] * (n // 2205))
        assert out.shape == ref.shape
        err = (out - ref).abs().max().item()
        assert err <= O_HAT_TOL, (n, chunk, err)


def test_output_does_not_depend_on_the_push_pattern(tcc):
    src, tgt = _ses(3)
    n = 256 * 400 + 31
    wave, noise = _wave(n, 5), _noise(_frames(n), 5)
    outs = []
    for pushes in ([n], [1, 2, 3, 500, 4096] + [2205] * 40, _pushes(n, 9, 1, 30000)):
        st = tcc.live_stream(src, tgt, chunk_frames=15, noise=noise)
        outs.append(_run_stream(st, wave, pushes))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_latency_bound_holds_on_the_device(tcc):
    src, tgt = _ses(4)
    n = 256 * 300
    wave, noise = _wave(n, 6), _noise(_frames(n), 6)
    st = tcc.live_stream(src, tgt, chunk_frames=15, noise=noise)
    emitted = 0
    for i in range(0, n, 1000):
        emitted += st.push(wave[i:i + 1000]).numel()
        arrived = min(n, i + 1000)
        assert emitted >= arrived - st.latency_samples + 1
    assert st.latency_samples <= int(1.5 * 22050)


# ---- the pool ---------------------------------------------------------------------------------------------------------
def _pool_vs_solo(tcc, tol):
    lengths = [256 * 120 + 5, 256 * 50, 256 * 8 + 200, 256 * 200 + 99, 256 * 90 + 1]
    opens = [0, 0, 3, 5, 9]           # tick at which each stream opens
    ses = [_ses(10 + i) for i in range(len(lengths))]
    waves = [_wave(n, 20 + i) for i, n in enumerate(lengths)]
    noises = [_noise(_frames(n), 30 + i) for i, n in enumerate(lengths)]
    pool = tcc.live_pool(chunk_frames=15, max_streams_per_launch=4)
    handles, pos, outs = {}, [0] * len(lengths), {i: [] for i in range(len(lengths))}
    builds = None
    tick = 0
    while True:
        for i, t in enumerate(opens):
            if t == tick:
                handles[i] = pool.open(*ses[i], noise=noises[i])
        for i, h in list(handles.items()):
            if pos[i] < lengths[i]:
                k = 2205 + 37 * i
                pool.push(h, waves[i][pos[i]:pos[i] + k])
                pos[i] += k
                if pos[i] >= lengths[i]:
                    pool.close(h)
        res = pool.step()
        for i, h in handles.items():
            if h in res:
                outs[i].append(res[h])
        tick += 1
        if tick == 14:
            builds = tcc.model.engine().live_ws_builds
        if all(pos[i] >= lengths[i] for i in range(len(lengths))) and not pool.active:
            break
    assert tcc.model.engine().live_ws_builds == builds, "a unit workspace was rebuilt after the ladder was warm"
    for i in range(len(lengths)):
        st = tcc.live_stream(*ses[i], chunk_frames=15, noise=noises[i])
        solo = _run_stream(st, waves[i], [2205 + 37 * i] * (lengths[i] // (2205 + 37 * i)))
        got = torch.cat(outs[i])
        assert got.shape == solo.shape
        err = (got - solo).abs().max().item()
        assert err <= tol, (i, err)


def test_pool_equals_solo_streams_bitwise_with_direct_kernels(tcc, direct):
    _pool_vs_solo(tcc, 0.0)


def test_pool_matches_solo_streams_with_default_kernels(tcc):
    _pool_vs_solo(tcc, O_HAT_TOL)


def test_pool_memory_grows_by_the_documented_state(tcc):
    pool = tcc.live_pool(chunk_frames=15, max_streams_per_launch=4)
    hs = [pool.open(*_ses(i)) for i in range(4)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    hs += [pool.open(*_ses(10 + i)) for i in range(4)]      # 4 -> 8 slots: the arena doubles
    torch.cuda.synchronize()
    grew = torch.cuda.memory_allocated(DEV) - before
    assert grew <= 4 * pool.state_bytes_per_stream() + (2 << 20), grew       # + the allocator's 2 MiB granularity


def test_unsupported_modes_raise(tcc):
    src, tgt = _ses(0)
    with pytest.raises(ValueError):
        tcc.live_stream(src, tgt, chunk_frames=16)
    tcc.enable_split_bf16x3(True)
    try:
        with pytest.raises(ValueError):
            tcc.live_stream(src, tgt)
    finally:
        tcc.enable_split_bf16x3(False)
