"""Per-item synthesis controls on the MI355X: ``ov_duration_items_f32`` / ``ov_expand_prior_items_f32`` against the
scalar kernels they generalise (bit for bit: the scalar kernels are pinned to the oracle by tests/test_gpu_tts*.py, so
no ceil-boundary tolerance enters here), ``infer`` with per-item ``noise_scale`` / ``length_scale`` / ``noise_scale_w``
/ ``sdp_ratio`` against scalar calls and the CPU oracle, ``tts_from_ids`` / ``infer_padded`` with per-sentence
speakers and speeds, and ``VoiceCloner.speak_ids_many(mixed=True)`` against the chain of the public pieces.

Bars.  Kernel level and everything that runs the same launches on the same shapes: equal bits.  ``o`` of item b in a
mixed batch against the same batch run with item b's scalars: 1e-4 (the batch-independence bar of tests/test_gpu_e2e.py:
another row width, other launch shapes).  Against the oracle: ``attn`` equal, ``o`` within 1e-3 (tests/test_gpu_tts.py)."""
import ctypes
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, clone  # noqa: E402
from openvoice_amd.engine import _ptr, padded_frames  # noqa: E402
from openvoice_amd.models import SynthesizerTrn  # noqa: E402
from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG as CFG, default_converter_hparams  # noqa: E402

DEV = "cuda:0"
HOP = 256


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(t):
    """Bit patterns, so that NaN sentinels in never-written padding compare equal."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rand(*shape, seed, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- ov_duration_items_f32 ------------------------------------------------------------------------------------------------
DUR_EA = (0.1, -0.2)


def _dur_inputs(T):
    """B = 3, ragged: a full row, a half row, a row of one token.  Row 1's dp is ~ -20, so that with sdp_ratio = 0 and a
    length_scale of 2e-38 every exp(logw) * length_scale rounds to zero: a total of 0, the y_len = max(1, .) branch."""
    B, ld = 3, padded_frames(T)
    lens = [T, max(1, T // 2), 1]
    mask = (torch.arange(ld)[None] < torch.tensor(lens)[:, None]).float()
    z = torch.full((B, 2, ld), float("nan"))
    z[:, :, :T] = _rand(B, 2, T, seed=10 + T)
    dp = torch.full((B, 32, ld), float("nan"))
    dp[:, :, :T] = _rand(B, 32, T, seed=20 + T) * mask[:, None, :T]
    dp[1, 0, :T] = -20.0 + 0.1 * _rand(T, seed=30 + T)
    return B, ld, z.to(DEV), dp.to(DEV), mask.to(DEV)


def _dur_outputs(B, ld):
    return (torch.full((B, ld), float("nan"), device=DEV), torch.full((B, ld), -7, dtype=torch.int32, device=DEV),
            torch.full((B,), -7, dtype=torch.int64, device=DEV))


def _dur_scalar(T, inp, ratio, scale):
    B, ld, z, dp, mask = inp
    logw, cum, ylen = _dur_outputs(B, ld)
    rc = _lib.load().ov_duration_f32(_ptr(z), 2 * ld, *DUR_EA, _ptr(dp), 32 * ld, _ptr(mask), _ptr(logw), _vp(cum),
                                     _vp(ylen), B, T, ld, ratio, scale, _st())
    assert rc == 0
    return logw.cpu(), cum.cpu(), ylen.cpu()


def _dur_items(T, inp, ratios, scales):
    B, ld, z, dp, mask = inp
    logw, cum, ylen = _dur_outputs(B, ld)
    rb, sb = torch.tensor(ratios, dtype=torch.float32, device=DEV), torch.tensor(scales, dtype=torch.float32, device=DEV)
    rc = _lib.load().ov_duration_items_f32(_ptr(z), 2 * ld, *DUR_EA, _ptr(dp), 32 * ld, _ptr(mask), _ptr(logw),
                                           _vp(cum), _vp(ylen), B, T, ld, _ptr(rb), _ptr(sb), _st())
    assert rc == 0
    return logw.cpu(), cum.cpu(), ylen.cpu()


@pytest.mark.parametrize("T", [1, 7, 64, 65, 300])       # 64 / 65: one wave and one more lane; 300: a second chunk of 256
def test_duration_items_equals_the_scalar_kernel_bitwise(T):
    inp = _dur_inputs(T)
    # constant vectors: the scalar launch, every word of every buffer (the padding columns stay untouched in both)
    want = _dur_scalar(T, inp, 0.2, 1.1)
    got = _dur_items(T, inp, [0.2] * 3, [1.1] * 3)
    for g, w, name in zip(got, want, ("logw", "cum", "y_len")):
        assert _same_bits(g, w), f"T={T} constant vectors: {name} differs"
    assert (want[1][0, :T].diff() >= 0).all() and want[2][0] == want[1][0, T - 1]       # a real prefix sum was compared
    # three pairs: row b is row b of the scalar kernel run with row b's pair
    pairs = [(0.2, 1.0), (0.0, 2e-38), (1.0, 1.7)]
    got = _dur_items(T, inp, [p[0] for p in pairs], [p[1] for p in pairs])
    for b, (ratio, scale) in enumerate(pairs):
        want = _dur_scalar(T, inp, ratio, scale)
        for g, w, name in zip(got, want, ("logw", "cum", "y_len")):
            assert _same_bits(g[b], w[b]), f"T={T} item {b} ({ratio}, {scale}): {name} differs"
    assert got[2][1] == 1 and (got[1][1, :T] == 0).all(), "item 1 was built to total 0 frames"
    assert got[2][0] > 1 or T == 1


# ---- ov_expand_prior_items_f32 --------------------------------------------------------------------------------------------
def _partition(total, parts, seed):
    """``parts`` non-negative durations summing to ``total``, zeros among them when there is room."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, total + 1, parts - 1))
    return np.diff(np.concatenate([[0], cuts, [total]])).tolist()


def _ep_inputs(Tx, Ty):
    """Item 0 is full (x_len = Tx, y_len = Ty); item 1 is shorter in both; item 2 has one token of duration 0, so
    y_len = 1 = max(1, 0) and its frame 0 belongs to no token."""
    B, C = 3, 192
    ldx, ldy = padded_frames(Tx), padded_frames(Ty)
    x_len = [Tx, max(1, Tx - 2), 1]
    y_len = [Ty, max(1, Ty // 2), 1]
    cum = torch.zeros(B, ldx, dtype=torch.int32)
    for b in (0, 1):
        d = _partition(y_len[b], x_len[b], seed=100 * Tx + Ty + b)
        cum[b, :x_len[b]] = torch.tensor(d).cumsum(0)
    mask = (torch.arange(ldx)[None] < torch.tensor(x_len)[:, None]).float()
    stats = torch.full((B, 2 * C, ldx), float("nan"))
    stats[:, :, :Tx] = _rand(B, 2 * C, Tx, seed=Tx + Ty) * mask[:, None, :Tx]
    noise = torch.full((B, C, ldy), float("nan"))
    noise[:, :, :Ty] = _rand(B, C, Ty, seed=Tx + Ty + 1)
    dev = lambda t: t.to(DEV)
    return dict(B=B, C=C, Tx=Tx, Ty=Ty, ldx=ldx, ldy=ldy, y_len=y_len, stats=dev(stats), noise=dev(noise), cum=dev(cum),
                x_lend=dev(torch.tensor(x_len)), y_lend=dev(torch.tensor(y_len)))


def _ep_run(p, config, noise_scale):
    """One launch: the scalar entry for a float ``noise_scale``, the items entry for a list.  Returns (z_p, m_p,
    logs_p, attn) on the host, None where ``config`` leaves an output out."""
    B, C, Tx, Ty, ldx, ldy = (p[k] for k in ("B", "C", "Tx", "Ty", "ldx", "ldy"))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    zp = nan(B, C, ldy)
    mp, lp = (nan(B, C, ldy), nan(B, C, ldy)) if config != "no_stats" else (None, None)
    attn = nan(B, Ty, Tx) if config != "no_attn" else None
    opt = lambda t: _ptr(t) if t is not None else None
    head = (_ptr(p["stats"]), _ptr(p["stats"], C * ldx), 2 * C * ldx, ldx, _vp(p["cum"]), _vp(p["x_lend"]),
            _vp(p["y_lend"]), _ptr(p["noise"]), C * ldy, ldy, _ptr(zp), opt(mp), opt(lp), opt(attn), B, C, Tx, Ty, ldy)
    lib = _lib.load()
    if isinstance(noise_scale, float):
        rc = lib.ov_expand_prior_f32(*head, noise_scale, _st())
    else:
        nsb = torch.tensor(noise_scale, dtype=torch.float32, device=DEV)
        rc = lib.ov_expand_prior_items_f32(*head, _ptr(nsb), _st())
    assert rc == 0
    return tuple(None if t is None else t.cpu() for t in (zp, mp, lp, attn))


@pytest.mark.parametrize("config", ["all", "no_attn", "no_stats"])
@pytest.mark.parametrize("Tx,Ty", [(1, 1), (9, 1), (1, 257), (9, 257)])      # 257 frames: five 64-frame tiles, one of 1
def test_expand_prior_items_equals_the_scalar_kernel_bitwise(Tx, Ty, config):
    p = _ep_inputs(Tx, Ty)
    scales = [0.0, 0.667, 1.0]
    got = _ep_run(p, config, scales)
    names = ("z_p", "m_p", "logs_p", "attn")
    for b, ns in enumerate(scales):
        want = _ep_run(p, config, ns)
        for g, w, name in zip(got, want, names):
            assert (g is None) == (w is None)
            if g is not None:       # whole rows: valid frames, the frames in [y_len, Ty) and the untouched padding
                assert _same_bits(g[b], w[b]), f"Tx={Tx} Ty={Ty} {config} item {b}: {name} differs"
    # what lies in [y_len[b], Ty) of a short item, stated on its own: no prior there, noise alone in z_p
    noise = p["noise"].cpu()
    for b, ns in enumerate(scales):
        n = p["y_len"][b]
        assert torch.equal(got[0][b, :, n:Ty], noise[b, :, n:Ty] * torch.tensor(ns, dtype=torch.float32))
        for t in got[1:3]:
            if t is not None:
                assert (t[b, :, n:Ty] == 0).all()
        if got[3] is not None:
            assert (got[3][b, n:] == 0).all() and set(got[3][b].unique().tolist()) <= {0.0, 1.0}
    if got[3] is not None:
        assert (got[3][0].sum(1) == 1).all(), "every frame of the full item belongs to exactly one token"
        assert (got[3][2] == 0).all(), "the item whose durations total 0 aligns nothing"


def test_constant_vector_equals_the_scalar_launch_bitwise():
    p = _ep_inputs(9, 257)
    for g, w in zip(_ep_run(p, "all", [0.667] * 3), _ep_run(p, "all", 0.667)):
        assert _same_bits(g, w)


# ---- TtsEngine.infer ------------------------------------------------------------------------------------------------------
LENGTHS = (5, 12, 9)
SPEAKERS = (0, 3, 7)
SPEEDS = (0.8, 1.0, 1.3)
ITEM = dict(noise_scale=(0.5, 0.667, 1.0), length_scale=tuple(1.0 / s for s in SPEEDS), noise_scale_w=(0.4, 0.6, 0.8),
            sdp_ratio=(0.0, 0.2, 1.0))
FRAMES_PER_ID = 64          # columns of explicit noise per symbol id: far more than the duration predictor gives


@pytest.fixture(scope="module")
def model(synth_tts_sd):
    m = SynthesizerTrn(68, 513, n_speakers=10, **CFG)
    m.load_state_dict(synth_tts_sd, strict=True)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def batch():
    gen = torch.Generator().manual_seed(21)
    B, Tx = len(LENGTHS), max(LENGTHS)
    tokens = torch.zeros(B, Tx, dtype=torch.long)
    for b, n in enumerate(LENGTHS):
        tokens[b, :n] = torch.randint(1, 68, (n,), generator=gen)
    return dict(tokens=tokens, lengths=torch.tensor(LENGTHS), sid=torch.tensor(SPEAKERS),
                noise_w=torch.randn(B, 2, Tx, generator=gen), noise_z=torch.randn(B, 192, FRAMES_PER_ID * Tx, generator=gen))


def _infer(model, batch, controls, **kw):
    noise = {} if "seed" in kw else dict(noise_w=batch["noise_w"], noise_z=batch["noise_z"])
    o, attn, y_mask, lat = model.infer(batch["tokens"], batch["lengths"], sid=batch["sid"], **controls, **noise, **kw)
    torch.cuda.synchronize()
    return dict(o=o.cpu(), attn=attn.cpu(), y_mask=y_mask.cpu(), z=lat[0].cpu(), z_p=lat[1].cpu(), m_p=lat[2].cpu(),
                logs_p=lat[3].cpu())


@pytest.fixture(scope="module")
def mixed(model, batch):
    """The per-item call every engine-level test looks at: computed once."""
    return _infer(model, batch, ITEM)


def _frames(run):
    return run["y_mask"][:, 0].sum(1).long().tolist()


def test_infer_constant_vectors_equal_the_scalar_call_bitwise(model, batch):
    scalars = dict(noise_scale=0.667, length_scale=1.1, noise_scale_w=0.6, sdp_ratio=0.2)
    want = _infer(model, batch, scalars)
    forms = [{k: [v] * 3 for k, v in scalars.items()},
             dict(scalars, length_scale=torch.full((3,), 1.1, dtype=torch.float64)),        # one per-item control suffices
             dict(scalars, noise_scale=np.full(3, 0.667))]
    for controls in forms:
        got = _infer(model, batch, controls)
        for name in want:
            assert _same_bits(got[name], want[name]), f"{name} differs from the scalar call"


def test_infer_per_item_equals_the_batch_run_with_that_items_scalars(model, batch, mixed):
    frames = _frames(mixed)
    assert len(set(frames)) == 3, frames
    for b in range(3):
        ref = _infer(model, batch, {k: v[b] for k, v in ITEM.items()})
        n = frames[b]
        assert _frames(ref)[b] == n
        assert torch.equal(mixed["y_mask"][b, :, :n], ref["y_mask"][b, :, :n])
        assert not mixed["y_mask"][b, :, n:].any() and not ref["y_mask"][b, :, n:].any()
        assert torch.equal(mixed["attn"][b, :, :n], ref["attn"][b, :, :n])
        assert not mixed["attn"][b, :, n:].any() and not ref["attn"][b, :, n:].any()
        for name in ("m_p", "logs_p", "z_p"):
            assert _same_bits(mixed[name][b, :, :n], ref[name][b, :, :n]), f"item {b}: {name} differs over its own frames"
        err = (mixed["o"][b, :, :n * HOP] - ref["o"][b, :, :n * HOP]).abs().max().item()
        print(f"item {b}: {n} frames of {mixed['o'].shape[2] // HOP} / {ref['o'].shape[2] // HOP}, |o - o_scalar|max {err:.3e}")
        assert err <= 1e-4, (b, err)


def test_infer_per_item_matches_the_oracle_item_by_item(model, batch, mixed, synth_tts_sd):
    """Each item alone (B = 1) through the CPU oracle with its own four scalars, as tests/test_gpu_tts.py drives it:
    ``attn`` equal, ``o`` within 1e-3 over every valid sample.

    The generator is unmasked (the reference's too): behind a short item's last frame the padded batch holds frames of
    z = 0, whose activations are the biases', where a B = 1 run has the convs' zero padding, so a sentence alone and
    the same sentence in a padded batch differ over its last ~13 frames in the reference as well (``tts_from_ids`` says
    so; measured here: 0.41 on the 15-frame item).  The oracle's waveform of a short item is therefore its generator on
    the item's own B = 1 latent ``z * y_mask`` zero-extended to the batch's frame count -- what the padded row holds.
    For the longest item nothing is extended, and the oracle's own ``o`` is compared as it is."""
    import torch.nn.functional as F
    from oracle import tts_oracle, vc_oracle
    from openvoice_amd.hostinfo import usable_cpus
    torch.set_num_threads(usable_cpus(32))
    frames = _frames(mixed)
    Ty = mixed["o"].shape[2] // HOP
    assert Ty == max(frames)
    for b, tx in enumerate(LENGTHS):
        with torch.no_grad():
            o_r, attn_r, ym_r, (z_r, _, _, _), _ = tts_oracle.infer(
                synth_tts_sd, CFG, batch["tokens"][b:b + 1, :tx], batch["lengths"][b:b + 1], batch["sid"][b:b + 1],
                batch["noise_w"][b:b + 1, :, :tx], batch["noise_z"][b:b + 1], ITEM["noise_scale"][b],
                ITEM["length_scale"][b], ITEM["noise_scale_w"][b], ITEM["sdp_ratio"][b])
            n = frames[b]
            assert int(ym_r.sum()) == n and attn_r.shape[2] == n
            if n < Ty:
                g = F.embedding(batch["sid"][b:b + 1], synth_tts_sd["emb_g.weight"]).unsqueeze(-1)
                o_r = vc_oracle.generator(synth_tts_sd, F.pad(z_r * ym_r, (0, Ty - n)), g, CFG)
        assert torch.equal(mixed["attn"][b, :, :n, :tx], attn_r[0]), f"item {b}: alignment differs from the oracle"
        assert not mixed["attn"][b, :, :, tx:].any()
        err = (mixed["o"][b, :, :n * HOP] - o_r[0, :, :n * HOP]).abs().max().item()
        print(f"item {b}: {n} frames of {Ty}, |o - o_oracle|max {err:.3e}")
        assert err <= 1e-3, (b, err)


@pytest.mark.parametrize("kw", [dict(generator="bf16"), dict(seed=5), dict(seed=5, generator="bf16", skip_padding=True)],
                         ids=["bf16", "seed5", "seed5_bf16_skip"])
def test_infer_per_item_runs_and_repeats_on_the_other_paths(model, batch, mixed, kw):
    first, second = _infer(model, batch, ITEM, **kw), _infer(model, batch, ITEM, **kw)
    for name in first:
        assert _same_bits(first[name], second[name]), f"{name} differs between two calls"
    assert torch.isfinite(first["o"]).all() and first["o"].abs().max() > 0
    if "seed" not in kw:        # the generator alone changes: everything before it is the fp32 call's bits
        for name in ("attn", "y_mask", "z", "z_p", "m_p", "logs_p"):
            assert _same_bits(first[name], mixed[name])


def test_infer_rejects_bad_per_item_controls(model, batch):
    for bad in (dict(length_scale=[1.0, 1.0]), dict(length_scale=[1.0, 0.0, 1.0]), dict(noise_scale=[0.1, float("nan"), 1.0])):
        with pytest.raises(ValueError):
            model.infer(batch["tokens"], batch["lengths"], sid=batch["sid"], **bad)


# ---- BaseSpeakerTTS and VoiceCloner -------------------------------------------------------------------------------------------
def _converter(d, synth_sd, sr):
    hps = default_converter_hparams("v2")
    data = dict(hps.data.items(), sampling_rate=sr)
    (d / f"conv{sr}.json").write_text(json.dumps({"_version_": "v2", "data": data, "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "converter.pth")
    t = api.ToneColorConverter(str(d / f"conv{sr}.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "converter.pth"))
    return t


@pytest.fixture(scope="module")
def models(tmp_path_factory, synth_sd, synth_tts_sd):
    d = tmp_path_factory.mktemp("tts_items")
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=True),
           "model": dict(CFG), "symbols": [f"s{i}" for i in range(68)], "speakers": {"default": 1, "whispering": 2}}
    (d / "tts.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_tts_sd}, d / "tts.pth")
    tts = api.BaseSpeakerTTS(str(d / "tts.json"), device=DEV)
    tts.load_ckpt(str(d / "tts.pth"))
    return tts, _converter(d, synth_sd, 22050)


def _sentences(counts, gen):
    return [api.intersperse(torch.randint(1, 68, (n,), generator=gen).tolist(), 0) for n in counts]


def test_tts_from_ids_with_one_speaker_and_speed_per_sentence(models):
    tts, _ = models
    gen = torch.Generator().manual_seed(31)
    ids = _sentences((2, 6, 4), gen)                              # 5, 13 and 9 ids with the blanks
    noise_w = [torch.randn(2, len(s), generator=gen) for s in ids]
    noise_z = [torch.randn(192, FRAMES_PER_ID * len(s), generator=gen) for s in ids]
    speakers, speeds, scales = [0, 3, 7], [0.8, 1.0, 1.3], [0.5, 0.667, 1.0]
    # the per-sentence loop: three single-sentence calls
    loop = tts.tts_from_ids(ids, speakers, speed=speeds, noise_scale=scales, noise_w=noise_w, noise_z=noise_z)
    for i in range(3):
        one = tts.tts_from_ids(ids[i:i + 1], speakers[i], speed=speeds[i], noise_scale=scales[i], noise_w=noise_w[i:i + 1],
                               noise_z=noise_z[i:i + 1])
        assert len(one) == 1 and np.array_equal(loop[i], one[0]), i
    # the batch: infer_padded with the same lists
    batched = tts.tts_from_ids(ids, speakers, speed=speeds, noise_scale=scales, batched=True, noise_w=noise_w,
                               noise_z=noise_z)
    o, frames = tts.infer_padded(ids, speakers, speed=speeds, noise_scale=scales, noise_w=noise_w, noise_z=noise_z)
    frames, o = frames.cpu().tolist(), o[:, 0].cpu().numpy()
    assert len(set(frames)) == 3
    for i in range(3):
        assert np.array_equal(batched[i], o[i, :frames[i] * HOP]) and len(batched[i]) == len(loop[i]), i
        assert np.isfinite(batched[i]).all()
    # lists that say the same as one value give the one value's bits (other kernels, same numbers)
    same = tts.tts_from_ids(ids, [3] * 3, speed=[1.3] * 3, batched=True, noise_w=noise_w, noise_z=noise_z)
    want = tts.tts_from_ids(ids, 3, speed=1.3, batched=True, noise_w=noise_w, noise_z=noise_z)
    assert all(np.array_equal(a, b) for a, b in zip(same, want))
    # seed= works unchanged: sentence i on stream (5, i) in both loops, so both draw the same durations
    seeded = tts.tts_from_ids(ids, speakers, speed=speeds, batched=True, seed=5)
    again = tts.tts_from_ids(ids, speakers, speed=speeds, batched=True, seed=5)
    per = tts.tts_from_ids(ids, speakers, speed=speeds, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(seeded, again))
    assert [len(a) for a in seeded] == [len(a) for a in per]
    with pytest.raises(ValueError, match="speed"):
        tts.tts_from_ids(ids, speakers, speed=[1.0, 1.0], batched=True)
    with pytest.raises(ValueError, match="speed"):
        tts.tts_from_ids(ids, speakers, speed=[1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match="speaker_id"):
        tts.infer_padded(ids, [0, 1], speed=speeds)


def _clone_requests():
    """Four requests of two sentences over three (speed, speaker) keys: requests 0 and 3 share one."""
    gen = torch.Generator().manual_seed(41)
    ids = [_sentences(ns, gen) for ns in ((5, 9), (12, 3), (7, 7), (4, 10))]
    ses = [(0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV), 0.3 * torch.randn(1, 256, 1, generator=gen).to(DEV))
           for _ in ids]
    speakers, speeds = ["default", "whispering", 7, 1], [1.0, 1.3, 0.8, 1.0]
    requests = [(i, spk, s, t, spd) for i, spk, (s, t), spd in zip(ids, speakers, ses, speeds)]
    nz = dict(noise_w=[[torch.randn(2, len(s), generator=gen) for s in req] for req in ids],
              noise_z=[[torch.randn(192, FRAMES_PER_ID * len(s), generator=gen) for s in req] for req in ids],
              noise=[torch.randn(1, 192, FRAMES_PER_ID * sum(len(s) for s in req) + 64, generator=gen) for req in ids])
    return requests, nz


def _chain(tts, conv, requests, nz, mixed):
    """The public pieces: ``infer_padded`` per batch (per-sentence lists for a mixed batch, one speaker and speed for a
    keyed one), ``ov_join_segments_f32`` per request (``clone.join_segments``), ``convert_many``."""
    ids = [q[0] for q in requests]
    sid = lambda spk: tts.hps.speakers[spk] if isinstance(spk, str) else spk
    batches = clone.sentence_batches([[len(s) for s in req] for req in ids], [(q[4], sid(q[1])) for q in requests], 32,
                                     mixed=mixed)
    sr = tts.hps.data.sampling_rate
    seg = {}
    for key, items in batches:
        if key is None:
            speaker, speed = [sid(requests[r][1]) for r, _ in items], [requests[r][4] for r, _ in items]
        else:
            speed, speaker = key
        o, frames = tts.infer_padded([ids[r][s] for r, s in items], speaker, speed=speed,
                                     noise_w=[nz["noise_w"][r][s] for r, s in items],
                                     noise_z=[nz["noise_z"][r][s] for r, s in items])
        frames = frames.cpu().tolist()
        for row, item in enumerate(items):
            seg[item] = o[row, 0, :frames[row] * HOP].contiguous()
    joined = []
    for r, q in enumerate(requests):                                # one request: its sentences as rows of one buffer
        rows = [seg[(r, s)] for s in range(len(q[0]))]
        ld = max(x.numel() for x in rows)
        buf = torch.zeros(len(rows), ld, device=DEV)
        for i, x in enumerate(rows):
            buf[i, :x.numel()] = x
        joined += clone.join_segments(buf, [x.numel() for x in rows], [list(range(len(rows)))], clone.gap_samples(sr, q[4]))
    out = conv.convert_many([w.cpu().numpy() for w in joined], [q[2] for q in requests], [q[3] for q in requests],
                            noise=nz["noise"], sr=sr)
    return out, batches


def test_speak_ids_many_mixed_is_one_launch_and_equals_the_public_chain(models):
    tts, conv = models
    requests, nz = _clone_requests()
    vc = clone.VoiceCloner(tts, conv)
    got = vc.speak_ids_many(requests, mixed=True, **nz)
    assert vc.last_launches == {"infer": 1, "join": 1}
    assert [key for key, _ in vc.last_batches] == [None] and len(vc.last_batches[0][1]) == 8
    want, batches = _chain(tts, conv, requests, nz, mixed=True)
    assert vc.last_batches == batches
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.ndim == 1 and len(g) > 4000 and np.isfinite(g).all(), r
        assert g.shape == w.shape and np.array_equal(g, w), r
    # keyed, said or unsaid: three launch sequences, the chain of the keyed pieces (scalar speed and speaker: the path
    # every caller had before mixed= existed), bit for bit
    keyed = vc.speak_ids_many(requests, mixed=False, **nz)
    assert vc.last_launches == {"infer": 3, "join": 3}
    default = vc.speak_ids_many(requests, **nz)
    assert vc.last_launches == {"infer": 3, "join": 3} and all(key is not None for key, _ in vc.last_batches)
    want_keyed, _ = _chain(tts, conv, requests, nz, mixed=False)
    for r, (d, k, w) in enumerate(zip(default, keyed, want_keyed)):
        assert np.array_equal(d, k) and np.array_equal(d, w), r
    # the same sentences, other batch neighbours: the same lengths
    assert [len(a) for a in got] == [len(a) for a in default]


def test_speak_ids_mixed_is_the_one_request_form(models):
    tts, conv = models
    requests, nz = _clone_requests()
    vc = clone.VoiceCloner(tts, conv)
    ids, spk, s, t, spd = requests[1]
    one = vc.speak_ids(ids, spk, s, t, speed=spd, mixed=True, noise_w=nz["noise_w"][1], noise_z=nz["noise_z"][1],
                       noise=nz["noise"][1])
    assert vc.last_launches == {"infer": 1, "join": 1} and vc.last_batches[0][0] is None
    many = vc.speak_ids_many(requests[1:2], mixed=True, noise_w=nz["noise_w"][1:2], noise_z=nz["noise_z"][1:2],
                             noise=nz["noise"][1:2])
    keyed = vc.speak_ids(ids, spk, s, t, speed=spd, noise_w=nz["noise_w"][1], noise_z=nz["noise_z"][1], noise=nz["noise"][1])
    # one request has one key: per-item kernels fed constant vectors give the scalar kernels' bits
    assert np.array_equal(one, many[0]) and np.array_equal(one, keyed)
