"""Streaming synthesis on the MI355X (openvoice_amd/tts_live.py, csrc/tts_live.hip).

* ``ov_expand_prior_rows_f32`` against ``ov_normal_philox_f32`` + ``ov_expand_prior_items_f32``, ``torch.equal``, through
  both bindings; invalid records and bad host arguments.
* The front half of a padded batch against its batch-1 runs (what lets the pool batch it).
* A stream against the solo one-pass ``infer`` of the sentence: bitwise with direct kernels (fp32, bf16 generator, bf16
  WaveNet layers), within the live bar with the default kernels; a pool against solo streams; the public generators.
"""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, clone, tts_live  # noqa: E402
from openvoice_amd import noise as noise_mod  # noqa: E402
from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG as CFG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
C = 192
O_HAT_TOL = 1e-4            # tests/test_gpu_live.py: a live stream against the one-pass call, default kernels
RATE_TOL = 3e-4             # tests/test_gpu_rates.py LIVE_TOL: the same through the output resampler
SENTINEL = -77.25


# ---- the kernel ------------------------------------------------------------------------------------------------------
DURS = [[1, 9, 1, 1, 12, 2, 1, 10, 3, 5, 5, 5],        # x_len 9 of Tx 12: the last three tokens are padding
        [1, 1, 10, 1, 20, 1, 1]]
X_LEN = [9, 7]
SEEDS = [(1234567, 0), ((1 << 40) + 5, 3)]


def _sentences():
    """Two sentences in one token arena: ([2][2C][cap] stats, [2][cap] cum, y_len)."""
    cap = 16
    gen = torch.Generator().manual_seed(3)
    tok = torch.randn(2, 2 * C, cap, generator=gen)
    tok[:, C:] *= 0.3
    cum = torch.zeros(2, cap, dtype=torch.int32)
    y_len = []
    for b, (d, xl) in enumerate(zip(DURS, X_LEN)):
        d = torch.tensor([v if j < xl else 0 for j, v in enumerate(d)])
        cum[b, :len(d)] = torch.cumsum(d, 0).int()
        y_len.append(int(d.sum()))
    return tok.to(DEV), cum.to(DEV), y_len, cap


def _reference(tok, cum, y_len, cap, b, scale):
    """z_p [C, y_len] of sentence b: ov_normal_philox_f32 then ov_expand_prior_items_f32 at B = 1."""
    Ty, Tx = y_len[b], len(DURS[b])
    nz = noise_mod.normal(SEEDS[b], C, 0, Ty, DEV, purpose=noise_mod.PURPOSE_TTS_Z).contiguous()
    z_p = torch.zeros(1, C, Ty, device=DEV)
    stats = tok[b:b + 1].contiguous()
    _lib.call("ov_expand_prior_items_f32", stats, (stats, C * cap), 2 * C * cap, cap, cum[b:b + 1].contiguous(),
              torch.tensor([X_LEN[b]], device=DEV), torch.tensor([Ty], device=DEV), nz, C * Ty, Ty, z_p, None, None, None,
              1, C, Tx, Ty, Ty, torch.tensor([scale], dtype=torch.float32, device=DEV))
    return z_p[0]


def _record(b, first, count, off, ld, y_len, cap, **kw):
    r = dict(seed=SEEDS[b][0], stream=SEEDS[b][1], f0=first, nf=count, x_len=X_LEN[b], y_len=y_len[b], m_off=b * 2 * C * cap,
             m_ld=cap, logs_off=b * 2 * C * cap + C * cap, logs_ld=cap, cum_off=b * cap, dst_off=off, dst_ld=ld)
    r.update(kw)
    return tuple(r.values())


def _launch(recs, scales, tok, cum, dst):
    _lib.call("ov_expand_prior_rows_f32", torch.tensor(recs, dtype=torch.int64).to(DEV), len(recs), C, tok, tok.numel(),
              cum, cum.numel(), torch.tensor(scales, dtype=torch.float32).to(DEV), dst, dst.numel(),
              max(max(r[3] for r in recs), 0))
    torch.cuda.synchronize()


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_rows_kernel_equals_philox_then_expand_items_bitwise(binding, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    tok, cum, y_len, cap = _sentences()
    assert min(min(d) for d in DURS) == 1 and max(max(d) for d in DURS) > 8 and X_LEN[0] < len(DURS[0])
    y0, y1 = y_len
    # (sentence, f0, nf, dst_ld, noise_scale, offset jitter)
    pieces = [(0, 5, 1, 1, 0.667, 1), (0, 1, 7, 9, 0.667, 2), (1, 2, 9, 37, 0.25, 3), (0, 3, 6, 6, 0.667, 1),
              (1, 0, 30, 31, 0.25, 0), (0, y0 - 11, 11, 13, 0.25, 3), (1, 0, y1, y1 + 2, 0.667, 2),
              (0, 8, 24, 64, 0.667, 0), (1, 4, 15, 16, 0.25, 0), (0, 0, y0, y0, 1.0, 1)]
    assert {p[1] % 4 for p in pieces} == {0, 1, 2, 3} and len({p[4] for p in pieces}) >= 2
    recs, at = [], 5
    for b, f0, nf, ld, scale, jitter in pieces:
        at = (at + 3) // 4 * 4 + jitter                # jitter 0 + f0 % 4 == 0: the vector store's case
        recs.append(_record(b, f0, nf, at, ld, y_len, cap))
        at += C * ld
    assert any(r[11] % 4 and r[12] % 4 for r in recs) and any(r[11] % 4 == 0 and r[2] % 4 == 0 for r in recs)
    dst = torch.full((at + 50,), SENTINEL, device=DEV)
    _launch(recs, [p[4] for p in pieces], tok, cum, dst)
    want = torch.full_like(dst, SENTINEL)
    refs = {}
    for (b, f0, nf, ld, scale, _), r in zip(pieces, recs):
        if (b, scale) not in refs:
            refs[(b, scale)] = _reference(tok, cum, y_len, cap, b, scale)
        want[r[11]:r[11] + C * ld].view(C, ld)[:, :nf] = refs[(b, scale)][:, f0:f0 + nf]
    assert torch.equal(dst, want), (dst - want).abs().max().item()      # the pieces bitwise, everything else the sentinel
    assert not torch.equal(refs[(0, 0.667)], refs[(0, 0.25)])


@pytest.mark.parametrize("bad", [dict(f0=-1), dict(dst_off=-4), dict(f0=30, nf=12), dict(nf=9, dst_ld=8),
                                 dict(dst_off=10 ** 7), dict(m_off=10 ** 9), dict(cum_off=31), dict(stream=1 << 32)])
def test_rows_kernel_invalid_record_writes_nothing_and_its_neighbour_still_writes(bad):
    tok, cum, y_len, cap = _sentences()
    good = _record(1, 3, 10, 8, 12, y_len, cap)
    invalid = _record(0, 4, 8, 8 + C * 12 + 4, 16, y_len, cap, **bad)
    dst = torch.full((8 + C * 12 + 4 + C * 16 + 40,), SENTINEL, device=DEV)
    _launch([invalid, good], [0.667, 0.667], tok, cum, dst)
    want = torch.full_like(dst, SENTINEL)
    want[8:8 + C * 12].view(C, 12)[:, :10] = _reference(tok, cum, y_len, cap, 1, 0.667)[:, 3:13]
    assert torch.equal(dst, want)


def test_rows_kernel_rejects_bad_host_arguments():
    tok, cum, y_len, cap = _sentences()
    recs = torch.tensor([_record(0, 0, 4, 0, 4, y_len, cap)], dtype=torch.int64).to(DEV)
    sc = torch.ones(1, device=DEV)
    dst = torch.zeros(C * 4, device=DEV)
    ok = [recs, 1, C, tok, tok.numel(), cum, cum.numel(), sc, dst, dst.numel(), 4]
    _lib.call("ov_expand_prior_rows_f32", *ok)
    for i, v in ((1, 0), (1, 65536), (2, 0), (4, 0), (6, 0), (9, 0), (10, -1), (0, None), (3, None), (5, None), (7, None),
                 (8, None)):
        args = list(ok)
        args[i] = v
        with pytest.raises(_lib.OvError):
            _lib.call("ov_expand_prior_rows_f32", *args)
    torch.cuda.synchronize()


# ---- models ----------------------------------------------------------------------------------------------------------
def _converter(d, synth_sd, sr=22050):
    hps = default_converter_hparams("v2")
    (d / "conv.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items(), sampling_rate=sr),
                                             "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "converter.pth")
    t = api.ToneColorConverter(str(d / "conv.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "converter.pth"))
    return t


@pytest.fixture(scope="module")
def models(tmp_path_factory, synth_sd, synth_tts_sd):
    d = tmp_path_factory.mktemp("tts_live")
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=True),
           "model": dict(CFG), "symbols": [f"s{i}" for i in range(68)], "speakers": {"default": 1, "whispering": 2}}
    (d / "tts.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_tts_sd}, d / "tts.pth")
    tts = api.BaseSpeakerTTS(str(d / "tts.json"), device=DEV)
    tts.load_ckpt(str(d / "tts.pth"))
    return tts, _converter(d, synth_sd)


@pytest.fixture
def direct(models):
    engines = [models[0].model.engine().core, models[1].model.engine()]
    saved = [e.use_winograd for e in engines]
    for e in engines:
        e.use_winograd = False
    yield
    for e, s in zip(engines, saved):
        e.use_winograd = s


def _ids(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.tensor(api.intersperse(torch.randint(1, 68, (n,), generator=gen).tolist(), 0))


def _frames(tts, ids, speed, seed):
    eng = tts.model.engine()
    fh = eng.front(ids[None], torch.tensor([ids.numel()]), torch.tensor([1]), noise_scale=0.667,
                   length_scale=1.0 / speed, noise_scale_w=0.6, seed=seed)
    return int(fh["y_len"][0])


_speeds = {}


def _speed_for(tts, ids, seed, lo, hi):
    """A speed at which the sentence has between lo and hi frames (the frame count falls as the speed rises)."""
    key = (tuple(ids.tolist()), seed, lo, hi)
    if key not in _speeds:
        a, b = 0.02, 60.0
        for _ in range(40):
            mid = (a * b) ** 0.5
            T = _frames(tts, ids, mid, seed)
            if lo <= T <= hi:
                _speeds[key] = (mid, T)
                break
            a, b = (mid, b) if T > hi else (a, mid)
        assert key in _speeds, f"no speed gives [{lo}, {hi}] frames"
    return _speeds[key]


def _solo(tts, ids, speaker, speed, seed, noise_scale=0.667, **kw):
    o = tts.model.infer(ids[None].to(DEV), torch.tensor([ids.numel()]).to(DEV), sid=torch.tensor([speaker]).to(DEV),
                        noise_scale=noise_scale, noise_scale_w=0.6, length_scale=1.0 / speed, seed=seed, **kw)[0]
    return o[0, 0]


def _stream(tts, ids, speaker, speed, seed, chunk, noise_scale=0.667, **kw):
    st = tts_live.TtsLiveStream(tts.model, ids, speaker, speed=speed, noise_scale=noise_scale, seed=seed,
                                chunk_frames=chunk, **kw)
    outs = list(st)
    assert st.done and all(o.numel() for o in outs)
    return torch.cat(outs), outs


# ---- the front half of a padded batch --------------------------------------------------------------------------------
def test_front_half_of_a_padded_batch_has_the_bits_of_its_batch_1_runs(models):
    tts = models[0]
    seqs = [_ids(11, 1), torch.tensor([5]), _ids(4, 2)]
    assert [s.numel() for s in seqs] == [23, 1, 9]          # 1 token: the smallest check_token_count admits
    lengths = torch.tensor([s.numel() for s in seqs])
    x = torch.zeros(3, 23, dtype=torch.long)
    for i, s in enumerate(seqs):
        x[i, :s.numel()] = s
    sid = torch.tensor([1, 2, 3])
    kw = dict(noise_scale=0.667, noise_scale_w=0.6, length_scale=0.9)
    _, attn, y_mask, (_, z_p, _, _) = tts.model.infer(x.to(DEV), lengths.to(DEV), sid=sid.to(DEV), seed=77, **kw)
    Ty = y_mask[:, 0].sum(1).long().tolist()
    for b, s in enumerate(seqs):
        _, a1, m1, (_, z1, _, _) = tts.model.infer(s[None].to(DEV), lengths[b:b + 1].to(DEV), sid=sid[b:b + 1].to(DEV),
                                                   seed=(77, b), **kw)
        assert m1.shape[-1] == Ty[b]
        assert torch.equal(attn[b, 0, :Ty[b], :s.numel()], a1[0, 0]), b
        assert not attn[b, 0, :Ty[b], s.numel():].any()
        assert torch.equal(z_p[b, :, :Ty[b]], z1[0]), (b, (z_p[b, :, :Ty[b]] - z1[0]).abs().max().item())


# ---- a stream against the solo one-pass infer ------------------------------------------------------------------------
def _ranges(chunk):
    faf = tts_live.first_audio_frames(CFG, chunk)
    return {"short": (8, 14), "ragged": (100, 104), "below": (faf - 4, faf - 1), "above": (faf + 1, faf + 4),
            "long": (295, 310)}


@pytest.mark.parametrize("chunk", [15, 60])
def test_stream_equals_solo_infer_bitwise_with_direct_kernels(models, direct, chunk):
    tts = models[0]
    assert tts_live.first_audio_frames(CFG, chunk) == {15: 45, 60: 60}[chunk]
    for name, (lo, hi) in _ranges(chunk).items():
        ids = _ids(3, 11) if name == "short" else _ids(12, 10)      # a token takes at least one frame
        seed = (4242, 3)
        speed, T = _speed_for(tts, ids, seed, lo, hi)
        assert name != "ragged" or T % chunk
        ref = _solo(tts, ids, 1, speed, seed)
        out, outs = _stream(tts, ids, 1, speed, seed, chunk)
        assert ref.numel() == T * 256 and out.shape == ref.shape, (name, T)
        assert torch.equal(out, ref), (name, T, (out - ref).abs().max().item())
        if T > tts_live.first_audio_frames(CFG, chunk) + chunk:
            assert len(outs) > 1                     # audio left before the sentence had been fed whole


@pytest.mark.parametrize("kw", [dict(generator="bf16"), dict(wavenet="bf16")])
def test_stream_equals_solo_infer_on_the_bf16_kernels(models, direct, kw):
    tts, ids, seed = models[0], _ids(12, 10), (99, 1)
    speed, T = _speed_for(tts, ids, seed, 100, 104)
    ref = _solo(tts, ids, 2, speed, seed, **kw)
    out, _ = _stream(tts, ids, 2, speed, seed, 15, **kw)
    assert out.shape == ref.shape and torch.equal(out, ref), (out - ref).abs().max().item()
    assert not torch.equal(ref, _solo(tts, ids, 2, speed, seed))       # genuinely the other kernels


def test_stream_matches_solo_infer_with_default_kernels(models):
    """The bar is tests/test_gpu_live.py's 1e-4 for this same algorithm switch (Winograd tiles line up differently in a
    live buffer), unless a third of it does not cover what the switch itself does to the one-pass call on these
    inputs: then three times that."""
    tts, ids, seed = models[0], _ids(12, 10), (4242, 3)
    core = tts.model.engine().core
    for lo, hi in ((100, 104), (295, 310)):
        speed, T = _speed_for(tts, ids, seed, lo, hi)
        ref = _solo(tts, ids, 1, speed, seed)
        core.use_winograd = False
        try:
            ref_direct = _solo(tts, ids, 1, speed, seed)
        finally:
            core.use_winograd = True
        switch = (ref - ref_direct).abs().max().item()
        tol = O_HAT_TOL if switch <= O_HAT_TOL / 3 else 3 * switch
        out, _ = _stream(tts, ids, 1, speed, seed, 15)
        err = (out - ref).abs().max().item()
        print(f"T = {T}: one-pass default vs direct {switch:.3e}, stream vs one-pass {err:.3e}, bar {tol:.3e}")
        assert out.shape == ref.shape and err <= tol, (T, err, switch)


# ---- a pool ----------------------------------------------------------------------------------------------------------
def _run_pool(tts, plan):
    """``plan``: [(open at step, ids, speaker, speed, noise_scale, seed)] -> one waveform per sentence."""
    pool = tts_live.TtsLivePool(tts.model, chunk_frames=15, max_streams_per_launch=4)
    outs, handles, step = {}, {}, 0
    while step <= max(p[0] for p in plan) or pool.active:
        for i, (at, ids, speaker, speed, scale, seed) in enumerate(plan):
            if at == step:
                handles[pool.open(ids, speaker, speed=speed, noise_scale=scale, seed=seed)] = i
        for h, o in pool.step().items():
            outs.setdefault(handles[h], []).append(o)
        step += 1
    return [torch.cat(outs[i]) for i in range(len(plan))]


def test_pool_of_five_equals_solo_streams_bitwise(models, direct):
    tts = models[0]
    plan = [(0, _ids(30, 20), 1, 1.0, 0.667, (5, 0)), (0, _ids(7, 21), 2, 1.3, 0.5, (5, 1)),
            (1, _ids(18, 22), 3, 0.8, 0.667, (6, 0)), (4, _ids(3, 23), 1, 1.0, 0.9, 8), (4, _ids(25, 24), 4, 1.1, 0.3, (5, 2))]
    solos = [_stream(tts, ids, spk, speed, seed, 15, noise_scale=scale)[0] for _, ids, spk, speed, scale, seed in plan]
    got = _run_pool(tts, plan)
    for i, (g, s) in enumerate(zip(got, solos)):
        assert g.shape == s.shape and torch.equal(g, s), (i, (g - s).abs().max().item())
    core = tts.model.engine().core
    builds = core.live_ws_builds                          # the ladder is warm: a second run allocates no workspace
    again = _run_pool(tts, plan)
    assert core.live_ws_builds == builds
    assert all(torch.equal(a, g) for a, g in zip(again, got))


# ---- the public generators -------------------------------------------------------------------------------------------
SENTENCES = [(36, 30), (6, 31), (20, 32)]


def test_tts_stream_from_ids_equals_the_joined_solo_sentences(models, direct):
    tts = models[0]
    seqs = [_ids(n, s) for n, s in SENTENCES]
    want = tts.audio_numpy_concat(tts.tts_from_ids(seqs, 1, speed=1.2, seed=(31, 4)), sr=22050, speed=1.2)
    chunks = list(tts.tts_stream_from_ids(seqs, 1, speed=1.2, seed=(31, 4), chunk_frames=15))
    got = torch.cat(chunks).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    # the first chunk leaves once ONE sentence has been fed first_audio_frames (+ at most one more chunk), by the books
    pool = tts_live.TtsLivePool(tts.model, chunk_frames=15, max_streams_per_launch=2)
    gen = tts_live.stream_sentences(pool, seqs, 1, 1.2, 0.667, 0.6, (31, 4), 22050)
    first = next(gen)
    assert pool._next == 1 and list(pool.frames) == [0] and pool.frames[0] > 4 * 15
    assert pool.first_audio_frames <= pool.frames_fed[0] <= pool.first_audio_frames + 15
    assert torch.equal(first, chunks[0])
    rest = list(gen)
    assert np.array_equal(torch.cat([first] + rest).cpu().numpy(), want)


@pytest.mark.parametrize("out_sr", [None, 16000])
def test_speak_stream_ids_equals_convert_long_of_the_streamed_speech(models, direct, out_sr):
    tts, conv = models
    cloner = clone.VoiceCloner(tts, conv)
    seqs = [_ids(n, s) for n, s in SENTENCES]
    gen = torch.Generator().manual_seed(40)
    src, tgt = (0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV) for _ in range(2))
    joined = torch.cat(list(tts.tts_stream_from_ids(seqs, 1, speed=1.0, seed=17)))
    want = conv.convert_long(joined, src, tgt, seed=17, tau=0.4, out_sr=out_sr)
    got = torch.cat(list(cloner.speak_stream_ids(seqs, 1, src, tgt, speed=1.0, seed=17, tau=0.4, out_sr=out_sr)))
    got = got.cpu().numpy()
    assert got.shape == want.shape
    if out_sr is None:
        assert np.array_equal(got, want), np.abs(got - want).max()
    else:
        assert np.abs(got - want).max() <= RATE_TOL


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_errors(models):
    tts = models[0]
    for chunk in (16, 0, 15.0):
        with pytest.raises(ValueError):
            tts.tts_live_pool(chunk_frames=chunk)
        with pytest.raises(ValueError):
            tts.tts_stream_from_ids([[1, 2]], 1, chunk_frames=chunk)
    pool = tts.tts_live_pool()
    with pytest.raises(IndexError):
        pool.open([1, 2, 3], 10)
    with pytest.raises(IndexError):
        pool.open([1, 68], 1)
    with pytest.raises(IndexError):
        pool.open([-1], 1)
    with pytest.raises(ValueError):
        pool.open([], 1)
    with pytest.raises(ValueError):
        pool.open([1], 1, speed=0)
    assert pool.active == []
    core = tts.model.engine().core
    for flag in ("_bf16_on", "_split3_on"):
        setattr(core, flag, True)
        try:
            with pytest.raises(ValueError):
                pool.open([1, 2, 3], 1)
            with pytest.raises(ValueError):
                tts.tts_live_pool()
        finally:
            setattr(core, flag, False)
    h = pool.open([1, 2, 3], 1, seed=3)
    assert pool.active == [h]
