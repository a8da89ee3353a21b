"""One ``tau`` per item inside shared launches on the MI355X (``ov_conv1d_params.scale_b``, read by ``OV_EPI_POSTERIOR``).

Kernel level (``launch_conv``, operands inside NaN-filled buffers as in tests/test_gpu_frame_kernels.py):

* every element of a mixed launch within that file's element-wise limit of float64 computed with ITS row's ``tau``;
* row ``b`` of the mixed launch ``torch.equal`` to row ``b`` of the same launch with the scalar ``tau[b]``; a vector of
  equal values ``torch.equal`` to the scalar launch; the other epilogues bit-identical with and without the field.

End to end, all ``torch.equal`` -- one scalar per row is all that changes: ``voice_conversion``, ``LivePool``,
``StreamPool``, ``convert_many``, ``VoiceCloner.speak_ids_many`` and ``convert_batch`` with per-item ``tau`` against the
same work done with one ``tau`` at a time.  Comparisons between launches of DIFFERENT sizes (a pool against a solo stream,
``convert_many`` against ``convert_long``) run the direct kernels, as the existing pool tests do: the Winograd choice
depends on the launch size.

Each kernel test prints ``RATIO <what> <worst err / lim>`` before it asserts.
"""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib  # noqa: E402
from openvoice_amd._lib import EPI_COUPLE, EPI_LINEAR, EPI_POSTERIOR  # noqa: E402
from openvoice_amd.engine import PackedConv, gate_row_order, launch_conv  # noqa: E402
from oracle import fp32_ref as R  # noqa: E402
from oracle.nanbuf import Buf  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
FORCED = dict(tile=1, chunk=32, loaders=4)      # the POSTERIOR instances; the layout picks 16-byte or 4-byte staging
KNOBS = {"forced": FORCED, "dispatcher": {}}
TAUS3 = (0.0, 0.3, 1.7)


# ---- kernel level --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(B, H, T, stress=False):
    """Operands of a q_proj launch: ``fp32_ref.posterior_operands`` itself at its own shape (B = 3, H = 192), the same
    recipe at the others; the ragged lengths of ``fp32_ref.lengths``."""
    if (B, H) == (R.B, R.H):
        o = R.posterior_operands(T, stress=stress)
    else:
        s = 7000 + 10 * H + B
        w, b = R.rand(2 * H, H, 1, seed=s + 3, scale=H ** -0.5), R.rand(2 * H, seed=s + 4, scale=0.1)
        if stress:
            w[H:] *= 0.01
            b[H:] = torch.linspace(-20.0, 20.0, H)
        mask = (torch.arange(T)[None, :] < torch.tensor(R.lengths(T)[:B])[:, None]).float()
        o = dict(h=R.rand(B, H, T, seed=s + 1), noise=R.rand(B, H, T, seed=s + 2), mask=mask, w=w, b=b)
    order = gate_row_order(H)
    return o, PackedConv(o["w"][order], o["b"][order], DEV, K=1, cout=H)


def _mask_rows(mask):
    T = mask.shape[1]
    mld = (T + 3) // 4 * 4 + 4
    m = torch.full((mask.shape[0], mld), NAN)
    m[:, :T] = mask
    return m.to(DEV), mld


def _scale_b(values):
    """The per-item vector inside a NaN-filled buffer, two floats in: ``(tensor, offset)``."""
    v = torch.full((len(values) + 5,), NAN)
    v[2:2 + len(values)] = torch.tensor(values, dtype=torch.float32)
    return v.to(DEV), 2


def _posterior(o, layer, layout, knobs, tau=None, taus=None):
    """One EPI_POSTERIOR launch -> the valid block on the host.  With ``taus`` the launch scalar is NaN: it must be
    ignored."""
    B, H, T = o["h"].shape
    x, noise, z = Buf(o["h"], layout), Buf(o["noise"]), Buf(torch.full((B, H, T), NAN))
    maskd, mld = _mask_rows(o["mask"])
    kw = dict(scale=tau)
    if taus is not None:
        sb, off = _scale_b(taus)
        kw = dict(scale=NAN, scale_b=sb, scale_b_off=off)
    launch_conv(layer, x.flat, x.off, x.bs, z.flat, z.off, z.bs, B, T, epi=EPI_POSTERIOR, res=noise.flat,
                res_off=noise.off, res_bs=noise.bs, mask=maskd, mask_bs=mld, rows=2 * H, x_ld=x.ld, out_ld=z.ld,
                **kw, **knobs)
    return z.get()


def _worst_per_item(got, o, taus):
    """Worst err / lim over the items, each against float64 computed with its own tau (``fp32_ref.posterior``)."""
    worst = 0.0
    for b, tau in enumerate(taus):
        ref = R.posterior(o["h"][b:b + 1], o["w"], o["b"], o["noise"][b:b + 1], tau, o["mask"][b:b + 1])
        worst = max(worst, R.worst(got[b:b + 1], ref))
    return worst


def _check(what, o, layer, layout, knobs, taus):
    got = _posterior(o, layer, layout, knobs, taus=taus)
    assert torch.isfinite(got).all()
    w = _worst_per_item(got, o, taus)
    print(f"RATIO {what} {w:.3f}")
    for b, tau in enumerate(taus):
        scalar = _posterior(o, layer, layout, knobs, tau=tau)
        assert torch.equal(got[b], scalar[b]), f"{what}: row {b} differs from the scalar launch with tau {tau}"
    assert w <= 1.0, f"{what}: worst err / lim = {w:.3f}"
    return got


@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("layout", ["vec", "odd_ld"])
@pytest.mark.parametrize("T", [5, 129])
@pytest.mark.parametrize("H", [32, 192])
def test_mixed_taus_per_row_against_float64_and_the_scalar_launches(H, T, layout, knobs):
    """B = 3, ragged lengths T, 1, T / 2; H = 32 is one pair of 32-row tiles (64 packed rows), H = 192 six; T = 129 two
    time tiles.  And B = 1 with a vector of one element."""
    o, layer = _case(3, H, T)
    got = _check(f"tau items H={H} T={T} {layout} {knobs}", o, layer, layout, KNOBS[knobs], TAUS3)
    assert not torch.equal(got[2], _posterior(o, layer, layout, KNOBS[knobs], tau=TAUS3[0])[2])     # the taus do differ
    o1, layer1 = _case(1, H, T)
    _check(f"tau items B=1 H={H} T={T} {layout} {knobs}", o1, layer1, layout, KNOBS[knobs], (0.3,))


@pytest.mark.parametrize("layout", ["vec", "odd_ld"])
def test_a_vector_of_equal_values_is_the_scalar_launch(layout):
    for H, T in ((32, 5), (192, 129)):
        o, layer = _case(3, H, T)
        assert torch.equal(_posterior(o, layer, layout, FORCED, taus=(0.3, 0.3, 0.3)),
                           _posterior(o, layer, layout, FORCED, tau=0.3))


@pytest.mark.parametrize("layout", ["vec", "odd_ld"])
def test_stress_logs_to_plus_minus_20_with_a_tau_vector(layout):
    """``test_posterior_epilogue_with_logs_to_plus_minus_20``'s weights (logs spread over [-20, 20]) at taus 0, 1, 4."""
    for T in (5, 129):
        o, layer = _case(R.B, R.H, T, stress=True)
        _check(f"tau items stress T={T} {layout}", o, layer, layout, FORCED, (0.0, 1.0, 4.0))


@pytest.mark.parametrize("layout", ["vec", "odd_ld"])
@pytest.mark.parametrize("T", [5, 129])
def test_the_other_epilogues_ignore_scale_b(T, layout):
    """EPI_COUPLE (forward, in place on the upper half) and EPI_LINEAR with a non-NULL vector of wild values: the bits
    of the launch without it."""
    H, B = R.H, R.B
    sb, off = _scale_b((5.0, -3.0, NAN))
    oc = R.couple_operands(T)
    couple = PackedConv(oc["w"], oc["b"], DEV, K=1)
    maskd, mld = _mask_rows(oc["mask"])
    ol = R.linear_operands(1, T)
    linear = PackedConv(ol["w"], ol["bias"], DEV, K=1)
    outs = {}
    for name, extra in (("null", {}), ("vector", dict(scale_b=sb, scale_b_off=off))):
        x, out = Buf(oc["h"], layout), Buf(oc["x"])
        launch_conv(couple, x.flat, x.off, x.bs, out.flat, out.off + (H // 2) * out.ld, out.bs, B, T, epi=EPI_COUPLE,
                    mask=maskd, mask_bs=mld, scale=1.0, x_ld=x.ld, out_ld=out.ld, **extra, **FORCED)
        x2, out2 = Buf(ol["x"], layout), Buf(torch.full((B, ol["w"].shape[0], T), NAN))
        launch_conv(linear, x2.flat, x2.off, x2.bs, out2.flat, out2.off, out2.bs, B, T, epi=EPI_LINEAR, scale=1 / 3,
                    x_ld=x2.ld, out_ld=out2.ld, **extra, **FORCED)
        outs[name] = (out.get(), out2.get())
    assert torch.isfinite(outs["null"][0]).all() and torch.isfinite(outs["null"][1]).all()
    assert torch.equal(outs["vector"][0], outs["null"][0]) and torch.equal(outs["vector"][1], outs["null"][1])
    assert not torch.equal(outs["null"][0], oc["x"])             # the coupling did run


def test_launch_conv_refuses_a_vector_it_cannot_use():
    o, layer = _case(3, 32, 5)
    for bad in (torch.zeros(2, device=DEV), torch.zeros(3, dtype=torch.float64, device=DEV),
                torch.zeros(6, device=DEV)[::2]):
        x, noise, z = Buf(o["h"]), Buf(o["noise"]), Buf(torch.full((3, 32, 5), NAN))
        with pytest.raises(_lib.OvError):
            launch_conv(layer, x.flat, x.off, x.bs, z.flat, z.off, z.bs, 3, 5, epi=EPI_POSTERIOR, res=noise.flat,
                        res_off=noise.off, res_bs=noise.bs, rows=64, x_ld=x.ld, out_ld=z.ld, scale_b=bad)
        assert torch.isnan(z.get()).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("tau_items")
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


def _frames(n):
    return (n + 2 * 384 - 1024) // 256 + 1


VC_TAUS = (0.1, 0.3, 0.9)


@pytest.mark.parametrize("skip_padding,wavenet,as_tensor", [(False, None, False), (True, None, False),
                                                            (False, "bf16", False), (False, None, True)])
def test_voice_conversion_item_b_is_the_batch_with_the_scalar_tau_b(tcc, skip_padding, wavenet, as_tensor):
    """B = 3, T = 65, lengths 65, 17, 40, explicit noise; the tau vector as a list or as a device tensor."""
    gen = torch.Generator().manual_seed(41)
    B, T = 3, 65
    spec = torch.rand(B, 513, T, generator=gen).to(DEV)
    lengths = torch.tensor([65, 17, 40])
    noise = torch.randn(B, 192, T, generator=gen).to(DEV)
    g_src, g_tgt = (0.3 * torch.randn(B, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(B, 256, 1, generator=gen)).to(DEV)
    kw = dict(noise=noise, skip_padding=skip_padding, **_lib.wavenet_kw(wavenet))
    tau = torch.tensor(VC_TAUS, dtype=torch.float32, device=DEV) if as_tensor else list(VC_TAUS)
    o_hat, _, lat = tcc.model.voice_conversion(spec, lengths, g_src, g_tgt, tau=tau, **kw)
    assert torch.isfinite(o_hat).all()
    for b, t in enumerate(VC_TAUS):
        o_ref, _, lat_ref = tcc.model.voice_conversion(spec, lengths, g_src, g_tgt, tau=t, **kw)
        assert torch.equal(o_hat[b], o_ref[b]), ("o_hat", b)
        for name, got, ref in zip(("z", "z_p", "z_hat"), lat, lat_ref):
            assert torch.equal(got[b], ref[b]), (name, b)
        other = (b + 1) % B
        assert not torch.equal(lat[0][other], lat_ref[0][other])        # the other rows did run with another tau


def test_convert_batch_scalar_equals_a_vector_of_that_value(tcc):
    gen = torch.Generator().manual_seed(43)
    B, n = 2, 256 * 20
    waves = (0.3 * torch.randn(B, n, generator=gen)).to(DEV)
    noise = torch.randn(B, 192, _frames(n), generator=gen).to(DEV)
    src, tgt = _ses(44)
    a, la = tcc.convert_batch(waves, src, tgt, tau=0.3, noise=noise)
    b, lb = tcc.convert_batch(waves, src, tgt, tau=[0.3] * B, noise=noise)
    assert torch.equal(a, b) and torch.equal(la, lb) and float(a.abs().max()) > 1e-4
    c, _ = tcc.convert_batch(waves, src, tgt, tau=[0.3, 0.9], noise=noise)
    assert torch.equal(c[0], a[0]) and not torch.equal(c[1], a[1])


POOL_TAUS = (0.1, 0.9)
LIVE_SAMPLES = (256 * 60 + 5, 256 * 57 + 130)
LIVE_PUSHES = (3000, 1, 5000, 777, 2205, 4099)


def _pool_run(pool, handles, waves, pushes):
    """Every tick pushes the same uneven amount into every stream still open, so that the streams advance together and
    their rows meet in the same launches."""
    pos, outs, tick = [0] * len(waves), [[] for _ in waves], 0
    while pool.active:
        for i, h in enumerate(handles):
            if pos[i] < waves[i].numel():
                k = pushes[tick % len(pushes)]
                pool.push(h, waves[i][pos[i]:pos[i] + k])
                pos[i] += k
                if pos[i] >= waves[i].numel():
                    pool.close(h)
        for h, o in pool.step().items():
            outs[handles.index(h)].append(o.clone())
        tick += 1
    return [torch.cat(o) for o in outs]


def _solo_run(st, wave, pushes):
    outs, pos, i = [], 0, 0
    while pos < wave.numel():
        outs.append(st.push(wave[pos:pos + pushes[i % len(pushes)]]))
        pos += pushes[i % len(pushes)]
        i += 1
    outs.append(st.close())
    return torch.cat(outs)


@pytest.mark.parametrize("generator", ["fp32", "bf16"])
def test_live_pool_streams_with_their_own_tau_equal_their_solo_streams(tcc, direct, generator):
    """Two streams of about 60 frames, taus 0.1 and 0.9, uneven pushes, one pool whose posterior-encoder launches carry
    both; the second stream leaves tau to the pool's default."""
    ses = [_ses(50), _ses(51)]
    waves = [_wave(n, 52 + i) for i, n in enumerate(LIVE_SAMPLES)]
    pool = tcc.live_pool(tau=POOL_TAUS[1], chunk_frames=15, max_streams_per_launch=2, generator=generator)
    handles = [pool.open(*ses[0], seed=61, tau=POOL_TAUS[0]), pool.open(*ses[1], seed=62)]
    got = _pool_run(pool, handles, waves, LIVE_PUSHES)
    assert pool._tau_rows, "no launch of the pool carried both taus"
    for i, n in enumerate(LIVE_SAMPLES):
        st = tcc.live_stream(*ses[i], tau=POOL_TAUS[i], chunk_frames=15, seed=61 + i, generator=generator)
        solo = _solo_run(st, waves[i], LIVE_PUSHES)
        assert got[i].numel() == (n // 256) * 256 and torch.equal(got[i], solo), (i, (got[i] - solo).abs().max().item())
        wrong = tcc.live_stream(*ses[i], tau=POOL_TAUS[1 - i], chunk_frames=15, seed=61 + i, generator=generator)
        assert not torch.equal(got[i], _solo_run(wrong, waves[i], LIVE_PUSHES))


WINDOW = 255                    # the smallest window: 2 x 120 frames of context and one 15-frame grid step of core
LONG_SAMPLES = (256 * 300 + 5, 256 * 290 + 130)


def test_stream_pool_streams_with_their_own_tau_equal_their_solo_streams(tcc, direct):
    """Two streams of 300 and 290 frames at 255-frame windows (four and three each), whose windows share launches."""
    ses = [_ses(70), _ses(71)]
    waves = [_wave(n, 72 + i) for i, n in enumerate(LONG_SAMPLES)]
    pushes = (30000, 1, 50000, 7777)
    pool = tcc.stream_pool(tau=POOL_TAUS[1], window_frames=WINDOW, max_windows_per_launch=8)
    handles = [pool.open(*ses[0], seed=81, tau=POOL_TAUS[0]), pool.open(*ses[1], seed=82)]
    got = _pool_run(pool, handles, waves, pushes)
    for i, n in enumerate(LONG_SAMPLES):
        solo = _solo_run(tcc.stream(*ses[i], tau=POOL_TAUS[i], window_frames=WINDOW, seed=81 + i), waves[i], pushes)
        assert got[i].numel() == 256 * _frames(n) and torch.equal(got[i], solo), (i, (got[i] - solo).abs().max().item())


def test_convert_many_with_two_taus_equals_convert_long_per_item(tcc, direct):
    ses = [_ses(90), _ses(91)]
    waves = [_wave(n, 92 + i) for i, n in enumerate(LONG_SAMPLES)]
    kw = dict(window_frames=WINDOW)
    many = tcc.convert_many(waves, [s for s, _ in ses], [t for _, t in ses], tau=list(POOL_TAUS), windows_per_launch=4,
                            seed=[5, 6], **kw)
    for i, n in enumerate(LONG_SAMPLES):
        one = tcc.convert_long(waves[i], *ses[i], tau=POOL_TAUS[i], seed=5 + i, **kw)
        assert many[i].shape == (256 * _frames(n),) and np.array_equal(many[i], one), i
    same = tcc.convert_many(waves, [s for s, _ in ses], [t for _, t in ses], tau=POOL_TAUS[0], windows_per_launch=4,
                            seed=[5, 6], **kw)
    assert np.array_equal(same[0], many[0]) and not np.array_equal(same[1], many[1])


def test_cloner_requests_differing_only_in_tau_equal_their_single_request_calls(tcc, direct, tmp_path, synth_tts_sd):
    """Two requests with the same sentence, speaker, embeddings and noise, taus 0.1 and 0.9 (the second through the
    call's default): one ``convert_many`` for both.  One sentence per ``infer`` launch in every call, so that the TTS
    half sees the same batches."""
    from openvoice_amd import api, clone
    from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG as CFG
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=True),
           "model": dict(CFG), "symbols": [f"s{i}" for i in range(68)], "speakers": {"default": 1}}
    (tmp_path / "tts.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_tts_sd}, tmp_path / "tts.pth")
    tts = api.BaseSpeakerTTS(str(tmp_path / "tts.json"), device=DEV)
    tts.load_ckpt(str(tmp_path / "tts.pth"))
    vc = clone.VoiceCloner(tts, tcc)
    gen = torch.Generator().manual_seed(95)
    ids = [api.intersperse(torch.randint(1, 68, (9,), generator=gen).tolist(), 0)]
    src, tgt = _ses(96)
    nw, nzz = [torch.randn(2, len(ids[0]), generator=gen)], [torch.randn(192, 64 * len(ids[0]), generator=gen)]
    nz = torch.randn(1, 192, 64 * len(ids[0]) + 64, generator=gen)
    requests = [(ids, "default", src, tgt, 1.0, None, POOL_TAUS[0]), dict(ids=ids, speaker="default", src_se=src, tgt_se=tgt)]
    kw = dict(max_sentences_per_launch=1)
    both = vc.speak_ids_many(requests, tau=POOL_TAUS[1], noise_w=[nw, nw], noise_z=[nzz, nzz], noise=[nz, nz], **kw)
    assert not np.array_equal(both[0], both[1]) and len(both[0]) > 4000
    for i, t in enumerate(POOL_TAUS):
        one = vc.speak_ids(ids, "default", src, tgt, tau=t, noise_w=nw, noise_z=nzz, noise=nz, **kw)
        assert both[i].shape == one.shape and np.array_equal(both[i], one), i
