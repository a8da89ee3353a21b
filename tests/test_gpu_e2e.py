"""End-to-end parity of the HIP converter path (through SynthesizerTrn / the C ABI) against
(a) the committed reference outputs (tests/golden, produced by the unmodified reference) and
(b) the oracle on the same seeded inputs at other shapes.  Tolerance from BASELINE.json's
north_star: waveform within 1e-3 max-abs of the fp32 reference; latents are checked at 2e-4."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd.hostinfo import usable_cpus  # noqa: E402
from openvoice_amd.models import SynthesizerTrn  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG  # noqa: E402

DEV = "cuda:0"
VC_CASES = ["vc_b2_t17", "vc_b3_t65_ragged_zero_g", "vc_b1_t40_tau0", "vc_b2_t64_stress_gain4"]
O_HAT_TOL = 1e-3
LATENT_TOL = 2e-4


def _model(sd, zero_g):
    m = SynthesizerTrn(0, 513, n_speakers=0, zero_g=zero_g, **CONVERTER_MODEL_CONFIG)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("name", VC_CASES)
def test_voice_conversion_matches_reference_golden(golden_dir, synth_sd, name):
    rec = torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)
    from test_oracle_golden import case_state_dict
    case = rec["case"]
    model = _model(case_state_dict(rec, synth_sd), case["zero_g"])
    o_hat, y_mask, (z, z_p, z_hat) = model.voice_conversion(
        rec["spec"].to(DEV), rec["lengths"].to(DEV), rec["g_src"].to(DEV), rec["g_tgt"].to(DEV),
        tau=case["tau"], noise=rec["noise"].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y_mask.cpu(), rec["y_mask"])
    errs = {k: (v.cpu() - rec[k]).abs().max().item() for k, v in
            dict(z=z, z_p=z_p, z_hat=z_hat, o_hat=o_hat).items()}
    # the latent bar is relative to the latents' magnitude: |z| <= ~4 in the calibrated cases, ~17 in the
    # high-dynamic-range case (params.stress_state_dict), where fp32 summation-order noise grows in proportion
    lat_tol = LATENT_TOL * max(1.0, rec["z"].abs().max().item() / 4.0)
    print(name, errs, "| |z|max", rec["z"].abs().max().item(), "latent bar", lat_tol)
    assert errs["z"] <= lat_tol and errs["z_p"] <= lat_tol and errs["z_hat"] <= lat_tol, errs
    assert errs["o_hat"] <= O_HAT_TOL, errs
    assert o_hat.shape == rec["o_hat"].shape


@pytest.mark.parametrize("B,T,zero_g,per_item", [(1, 1, True, False), (2, 64, False, True), (3, 127, True, False),
                                                 (1, 861, True, False), (1, 1000, False, False),
                                                 (9, 65, False, True)])
def test_voice_conversion_matches_oracle(synth_sd, B, T, zero_g, per_item):
    """Tile/halo edge shapes, the benchmark frame count (T = 861), T = 1000 (SURVEY.md section 8c's shape list) and a
    ragged batch of 9 with per-item embeddings, vs the CPU oracle."""
    from oracle import vc_oracle
    gen = torch.Generator().manual_seed(B * 1000 + T)
    spec = torch.rand(B, 513, T, generator=gen).abs() * torch.linspace(3, 0.05, 513)[None, :, None]
    gshape = (B if per_item else 1, 256, 1)
    g_src, g_tgt = 0.3 * torch.randn(gshape, generator=gen), 0.3 * torch.randn(gshape, generator=gen)
    noise = torch.randn(B, 192, T, generator=gen)
    lengths = torch.tensor([max(1, T - 7 * b) for b in range(B)], dtype=torch.long)
    torch.set_num_threads(usable_cpus(32))
    with torch.no_grad():
        o_ref, mask_ref, (z_r, zp_r, zh_r) = vc_oracle.voice_conversion(
            synth_sd, CONVERTER_MODEL_CONFIG, spec, lengths, g_src, g_tgt, 0.3, noise, zero_g=zero_g)
    model = _model(synth_sd, zero_g)
    o_hat, y_mask, (z, z_p, z_hat) = model.voice_conversion(spec.to(DEV), lengths.to(DEV), g_src.to(DEV),
                                                            g_tgt.to(DEV), tau=0.3, noise=noise.to(DEV))
    torch.cuda.synchronize()
    errs = dict(z=(z.cpu() - z_r).abs().max().item(), z_p=(z_p.cpu() - zp_r).abs().max().item(),
                z_hat=(z_hat.cpu() - zh_r).abs().max().item(), o_hat=(o_hat.cpu() - o_ref).abs().max().item())
    print((B, T), errs)
    assert torch.equal(y_mask.cpu(), mask_ref)
    assert max(errs["z"], errs["z_p"], errs["z_hat"]) <= LATENT_TOL, errs
    assert errs["o_hat"] <= O_HAT_TOL, errs


@pytest.mark.parametrize("name", VC_CASES + ["ref_enc_b2_t200"])
def test_reference_encoder_matches_reference_golden(golden_dir, synth_sd, name):
    """extract_se's model half: model.ref_enc(spec.transpose(1, 2)) as openvoice/api.py:131 calls it,
    against the unmodified reference's output.  Tolerance 1e-4 max-abs on |se| ~ 0.1-0.3."""
    rec = torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)
    model = _model(synth_sd, False)
    se = model.ref_enc(rec["spec"].to(DEV).transpose(1, 2))
    torch.cuda.synchronize()
    assert se.shape == rec["ref_enc"].shape
    err = (se.cpu() - rec["ref_enc"]).abs().max().item()
    print(name, "ref_enc err", err, "scale", rec["ref_enc"].abs().max().item())
    assert err <= 1e-4, err


def test_reference_encoder_matches_oracle_at_benchmark_length(synth_sd):
    """T = 861 frames (10 s): 14 GRU steps, all six conv2d layers with odd sizes."""
    from oracle import vc_oracle
    gen = torch.Generator().manual_seed(5)
    spec = torch.rand(3, 513, 861, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]
    with torch.no_grad():
        ref = vc_oracle.reference_encoder(synth_sd, spec.transpose(1, 2))
    model = _model(synth_sd, False)
    se = model.ref_enc(spec.to(DEV).transpose(1, 2))
    torch.cuda.synchronize()
    err = (se.cpu() - ref).abs().max().item()
    print("ref_enc T=861 err", err)
    assert err <= 1e-4, err


def test_benchmark_size_properties_round_trip_and_batch_independence(synth_sd):
    """BASELINE.json configs[1] at full size (B = 32, T = 861 frames) -- too big for the CPU oracle in a test,
    so checked through properties that do not depend on size:
      * the flow is a bijection: with sid_src == sid_tgt, forward then reverse must return z (z_hat == z);
      * utterances are independent (the sharding argument of the multi-GPU path): item b of the batch-32 run
        equals a batch-1 run of the same item -- bit for bit within one kernel family (``use_winograd = False``: the
        direct convs), and within 1e-4 (measured ~1e-5) under the default launch policy, which picks the conv ALGORITHM
        by launch size (engine.WINO_MIN_ITEMS: generator stage 0 runs the direct kernel at batch 1-2, the Winograd-domain
        kernel from batch 3 on), as the reference's own backend does;
      * re-running the same batch is bit-identical (no races, no uninitialised reads);
      * masks: positions >= length are exactly zero in z and z_hat."""
    B, T = 32, 861
    gen = torch.Generator().manual_seed(77)
    spec = (torch.rand(B, 513, T, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]).to(DEV)
    lengths = torch.full((B,), T, dtype=torch.long)
    lengths[5], lengths[17] = 400, 1
    g = (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)
    noise = torch.randn(B, 192, T, generator=gen).to(DEV)
    model = _model(synth_sd, True)
    o1, _, (z, z_p, z_hat) = model.voice_conversion(spec, lengths.to(DEV), g, g, tau=0.3, noise=noise)
    err = (z_hat - z).abs().max().item()
    print("flow round trip at B=32, T=861: max |z_hat - z| =", err, "| |z|max =", z.abs().max().item(),
          "| |z_p - z|max =", (z_p - z).abs().max().item())
    assert (z_p - z).abs().max().item() > 0.5, "flow must be non-trivial for the round trip to mean anything"
    assert err <= 2e-4, err
    assert z[5, :, 400:].abs().max().item() == 0.0 and z_hat[17, :, 1:].abs().max().item() == 0.0
    assert bool(torch.isfinite(o1).all()) and o1.shape == (B, 1, 256 * T)
    o2 = model.voice_conversion(spec, lengths.to(DEV), g, g, tau=0.3, noise=noise)[0]
    assert torch.equal(o1, o2), "same batch twice must be bit-identical"
    for b in (0, 5, 31):
        ob = model.voice_conversion(spec[b:b + 1], lengths[b:b + 1].to(DEV), g, g, tau=0.3, noise=noise[b:b + 1])[0]
        err_b = (ob[0] - o1[b]).abs().max().item()
        assert err_b <= 1e-4, f"item {b}: batch-32 and batch-1 results differ by {err_b}"
    eng = model.engine()
    eng.use_winograd = False
    try:
        od = model.voice_conversion(spec, lengths.to(DEV), g, g, tau=0.3, noise=noise)[0]
        assert (od - o1).abs().max().item() <= 1e-4        # the two conv algorithms agree far inside the path's 1e-3
        for b in (0, 31):
            ob = model.voice_conversion(spec[b:b + 1], lengths[b:b + 1].to(DEV), g, g, tau=0.3, noise=noise[b:b + 1])[0]
            assert torch.equal(ob[0], od[b]), f"item {b}: batch-32 and batch-1 results of the direct kernels differ"
    finally:
        eng.use_winograd = True


def test_tone_color_converter_api_end_to_end_from_files(tmp_path, synth_sd):
    """BASELINE.json configs[0] plumbing (the reference demo flow, openvoice/api.py:114-160,
    se_extractor.py:129-152) with WAV files standing in for the MP3 resources (no MP3 decoder in the image):
    config.json + checkpoint.pth on disk -> ToneColorConverter -> get_se / extract_se -> convert -> WAV on disk,
    checked against the CPU oracle run on the same samples (tau = 0 makes the conversion deterministic)."""
    import json
    import numpy as np
    from openvoice_amd import api, audio_io, se_extractor
    from openvoice_amd.utils import default_converter_hparams
    from oracle import vc_oracle
    hps = default_converter_hparams("v2")
    cfg = {"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_sd}, tmp_path / "checkpoint.pth")
    sr = 22050
    t = np.arange(int(2.3 * sr)) / sr
    src = (0.4 * np.sin(2 * np.pi * 220 * t) + 0.2 * np.sin(2 * np.pi * 1370 * t + 1.0)).astype(np.float32)
    ref = (0.5 * np.sin(2 * np.pi * 330 * np.arange(int(21 * sr)) / sr) *
           (1 + 0.3 * np.sin(2 * np.pi * 3 * np.arange(int(21 * sr)) / sr))).astype(np.float32)
    audio_io.write(str(tmp_path / "src.wav"), src, sr)
    audio_io.write(str(tmp_path / "ref.wav"), ref, sr)
    tcc = api.ToneColorConverter(str(tmp_path / "config.json"), device=DEV, enable_watermark=False)
    tcc.load_ckpt(str(tmp_path / "checkpoint.pth"))
    assert tcc.version == "v2" and tcc.model.zero_g is True
    tgt_se, name = se_extractor.get_se(str(tmp_path / "ref.wav"), tcc, target_dir=str(tmp_path / "processed"), vad=True)
    src_se = tcc.extract_se(str(tmp_path / "src.wav"), se_save_path=str(tmp_path / "se" / "src.pth"))
    assert tgt_se.shape == src_se.shape == (1, 256, 1) and os.path.exists(tmp_path / "se" / "src.pth")
    assert os.path.exists(tmp_path / "processed" / name / "se.pth")
    # oracle: same decoded samples (16-bit WAV round trip), same embeddings, tau = 0
    wav16, _ = audio_io.load(str(tmp_path / "src.wav"), sr)
    with torch.no_grad():
        spec = vc_oracle.spectrogram(torch.from_numpy(wav16)[None])
        segs = sorted((tmp_path / "processed" / name / "wavs").glob("*.wav"))
        ses = []
        for seg in segs:
            w, _ = audio_io.load(str(seg), sr)
            ses.append(vc_oracle.reference_encoder(synth_sd, vc_oracle.spectrogram(torch.from_numpy(w)[None]).transpose(1, 2)))
        se_ref = torch.stack(ses).mean(0).unsqueeze(-1)
        o_ref = vc_oracle.voice_conversion(synth_sd, dict(hps.model.items()), spec, torch.tensor([spec.shape[2]]),
                                           src_se.cpu(), tgt_se.cpu(), 0.0, torch.zeros(1, 192, spec.shape[2]),
                                           zero_g=True)[0]
    assert len(segs) == 2 and (tgt_se.cpu() - se_ref).abs().max().item() <= 1e-4
    assert tcc.last_extract_se_batches == [1]       # (the src.wav call above; get_se ran the two pieces as one batch)
    audio = tcc.convert(str(tmp_path / "src.wav"), src_se, tgt_se, output_path=None, tau=0.0)
    assert audio.dtype == np.float32 and audio.shape == (spec.shape[2] * 256,)
    err = np.abs(audio - o_ref[0, 0].numpy()).max()
    print("api convert vs oracle:", err)
    assert err <= 1e-3
    tcc.convert(str(tmp_path / "src.wav"), src_se, tgt_se, output_path=str(tmp_path / "out.wav"), tau=0.0)
    back, _ = audio_io.load(str(tmp_path / "out.wav"), sr)
    assert np.abs(back - audio).max() <= 1.0 / 32768 + 1e-6
    # batched entry: ragged list == per-item convert away from the unmasked-decoder tails
    o_b, n_b = tcc.convert_batch([src, src[: sr]], src_se, tgt_se, tau=0.0)
    assert n_b.tolist() == [spec.shape[2] * 256, ((sr - 256) // 256 + 1) * 256]
    assert np.abs(o_b[0, 0].cpu().numpy()[: len(audio)] - audio).max() <= 1e-3


def test_ragged_batch_at_benchmark_length_matches_oracle_on_the_same_padded_batch(synth_sd):
    """B = 3 x T = 861 with lengths 861 / 600 / 100: the generator is unmasked, so a padded batch
    differs from per-utterance runs near each utterance's end (hard part 6) -- the oracle therefore
    converts the SAME padded batch.  Every time tile of the short utterances beyond their length is exercised."""
    from oracle import vc_oracle
    B, T = 3, 861
    gen = torch.Generator().manual_seed(861600100)
    spec = torch.rand(B, 513, T, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]
    lengths = torch.tensor([861, 600, 100])
    g_src, g_tgt = 0.3 * torch.randn(1, 256, 1, generator=gen), 0.3 * torch.randn(B, 256, 1, generator=gen)
    noise = torch.randn(B, 192, T, generator=gen)
    torch.set_num_threads(usable_cpus(32))
    with torch.no_grad():
        o_ref, mask_ref, (z_r, zp_r, zh_r) = vc_oracle.voice_conversion(
            synth_sd, CONVERTER_MODEL_CONFIG, spec, lengths, g_src, g_tgt, 0.3, noise, zero_g=True)
    model = _model(synth_sd, True)
    o_hat, y_mask, (z, z_p, z_hat) = model.voice_conversion(spec.to(DEV), lengths.to(DEV), g_src.to(DEV),
                                                            g_tgt.to(DEV), tau=0.3, noise=noise.to(DEV))
    torch.cuda.synchronize()
    errs = dict(z=(z.cpu() - z_r).abs().max().item(), z_p=(z_p.cpu() - zp_r).abs().max().item(),
                z_hat=(z_hat.cpu() - zh_r).abs().max().item(), o_hat=(o_hat.cpu() - o_ref).abs().max().item())
    print("ragged 861/600/100:", errs)
    assert torch.equal(y_mask.cpu(), mask_ref)
    assert max(errs["z"], errs["z_p"], errs["z_hat"]) <= LATENT_TOL and errs["o_hat"] <= O_HAT_TOL, errs
    assert z_hat[2, :, 100:].abs().max().item() == 0.0 and z_hat[1, :, 600:].abs().max().item() == 0.0
    # the padded tail of a short utterance is NOT silence (unmasked generator: biases propagate) -- and matches
    tail = o_hat[2, 0, 256 * 200:].cpu()
    assert tail.abs().max().item() > 0 and (tail - o_ref[2, 0, 256 * 200:]).abs().max().item() <= O_HAT_TOL


def test_device_rng_path_is_deterministic_under_a_seed(synth_sd):
    """What bench.py times: waveform -> spectrogram_torch -> voice_conversion with ``noise=None`` (drawn on the device
    from torch's generator).  Under the same ``torch.manual_seed`` two runs at B = 32 are bit-identical; another seed
    changes the waveform (tau > 0), and an explicit draw from the same seed reproduces the implicit one."""
    from openvoice_amd.mel_processing import spectrogram_torch
    model = _model(synth_sd, True)
    B, N = 32, 256 * 120
    gen = torch.Generator().manual_seed(12)
    wave = (0.5 * torch.rand(B, N, generator=gen) - 0.25).to(DEV)
    g = (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)

    def run(seed, explicit=False):
        torch.manual_seed(seed)
        spec = spectrogram_torch(wave, 1024, 22050, 256, 1024, center=False)
        lengths = torch.full((B,), spec.shape[2], dtype=torch.int64, device=DEV)
        noise = torch.randn(B, 192, spec.shape[2], dtype=torch.float32, device=DEV) if explicit else None
        return model.voice_conversion(spec, lengths, g, g, tau=0.3, noise=noise)[0].clone()

    a, b, c, d = run(7), run(7), run(8), run(7, explicit=True)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b), "same seed, same batch: must be bit-identical"
    assert not torch.equal(a, c), "another seed must change the posterior sample"
    assert torch.equal(a, d), "the implicit draw is torch.randn(B, 192, T) on the device from the global generator"


def test_extract_se_batches_equal_length_pieces(tmp_path, synth_sd):
    """SURVEY.md section 8f item 2, second half: ``get_se`` on a 60 s recording cuts six equal pieces and
    ``extract_se`` runs them as ONE [6, samples] spectrogram + ONE ``ref_enc`` launch sequence (the reference loops
    over the files, openvoice/api.py:121-133); the mean equals the per-file mean within 1e-5.  Files of other lengths
    keep their own call, and the result is the mean over files in the caller's order."""
    import json
    import numpy as np
    from openvoice_amd import api, audio_io, se_extractor
    from openvoice_amd.utils import default_converter_hparams
    hps = default_converter_hparams("v2")
    cfg = {"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_sd}, tmp_path / "checkpoint.pth")
    sr = 22050
    n = np.arange(60 * sr)
    rng = np.random.default_rng(3)
    ref = (0.4 * np.sin(2 * np.pi * (200 + 30 * np.sin(2 * np.pi * n / (7.3 * sr))) * n / sr)
           + 0.05 * rng.standard_normal(len(n))).astype(np.float32)
    audio_io.write(str(tmp_path / "ref60.wav"), ref, sr)
    tcc = api.ToneColorConverter(str(tmp_path / "config.json"), device=DEV, enable_watermark=False)
    tcc.load_ckpt(str(tmp_path / "checkpoint.pth"))
    se, name = se_extractor.get_se(str(tmp_path / "ref60.wav"), tcc, target_dir=str(tmp_path / "processed"))
    assert tcc.last_extract_se_batches == [6], tcc.last_extract_se_batches
    segs = sorted(str(p) for p in (tmp_path / "processed" / name / "wavs").glob("*.wav"))
    per_file = torch.stack([tcc.extract_se(s) for s in segs]).mean(0)
    assert tcc.last_extract_se_batches == [1]
    err = (se - per_file).abs().max().item()
    print("batched extract_se vs per-file mean:", err)
    assert se.shape == (1, 256, 1) and err <= 1e-5
    # mixed lengths: two equal files + one shorter -> two ref_enc calls, mean over the three files
    audio_io.write(str(tmp_path / "short.wav"), ref[: 4 * sr], sr)
    mixed = [segs[0], str(tmp_path / "short.wav"), segs[1]]
    se_mixed = tcc.extract_se(mixed)
    assert sorted(tcc.last_extract_se_batches) == [1, 2]
    want = torch.stack([tcc.extract_se(f) for f in mixed]).mean(0)
    assert (se_mixed - want).abs().max().item() <= 1e-5


def test_voice_conversion_matches_reference_at_benchmark_length(golden_dir, synth_sd):
    """The waveform -> spectrogram -> voice_conversion path at T = 861 frames against the unmodified reference's
    own output (fixture tests/golden/vc_b1_t861_benchmark_length.pt)."""
    from openvoice_amd.mel_processing import spectrogram_torch
    from test_oracle_golden import benchmark_length_inputs
    rec = torch.load(os.path.join(golden_dir, "vc_b1_t861_benchmark_length.pt"), weights_only=False)
    wave, g_src, g_tgt, noise = benchmark_length_inputs(rec)
    model = _model(synth_sd, rec["case"]["zero_g"])
    spec = spectrogram_torch(wave.to(DEV), 1024, 22050, 256, 1024, center=False)
    o_hat, _, (z, z_p, z_hat) = model.voice_conversion(spec, torch.tensor([861]).to(DEV), g_src.to(DEV), g_tgt.to(DEV),
                                                       tau=rec["case"]["tau"], noise=noise.to(DEV))
    torch.cuda.synchronize()
    err = (o_hat.cpu() - rec["o_hat"]).abs().max().item()
    print("T=861 vs reference: o_hat err", err)
    assert (z_hat.cpu().sum(2) - rec["z_hat_sum"]).abs().max().item() <= 5e-3
    assert err <= O_HAT_TOL


def test_benchmark_batch_items_match_the_oracle_directly(synth_sd):
    """BASELINE.json configs[1] itself -- B = 32 x T = 861 in ONE call --
    compared with the oracle, not only through properties: the oracle converts items 3 and 20 of the same inputs one
    at a time (utterances are independent at full length: no padding)."""
    from oracle import vc_oracle
    B, T = 32, 861
    gen = torch.Generator().manual_seed(4242)
    spec = torch.rand(B, 513, T, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]
    lengths = torch.full((B,), T, dtype=torch.long)
    g_src, g_tgt = 0.3 * torch.randn(1, 256, 1, generator=gen), 0.3 * torch.randn(1, 256, 1, generator=gen)
    noise = torch.randn(B, 192, T, generator=gen)
    model = _model(synth_sd, True)
    o_hat, _, (z, z_p, z_hat) = model.voice_conversion(spec.to(DEV), lengths.to(DEV), g_src.to(DEV), g_tgt.to(DEV),
                                                       tau=0.3, noise=noise.to(DEV))
    torch.cuda.synchronize()
    torch.set_num_threads(usable_cpus(32))
    for b in (3, 20):
        with torch.no_grad():
            o_r, _, (z_r, zp_r, zh_r) = vc_oracle.voice_conversion(
                synth_sd, CONVERTER_MODEL_CONFIG, spec[b:b + 1], lengths[b:b + 1], g_src, g_tgt, 0.3, noise[b:b + 1],
                zero_g=True)
        errs = dict(z=(z[b:b + 1].cpu() - z_r).abs().max().item(), z_p=(z_p[b:b + 1].cpu() - zp_r).abs().max().item(),
                    z_hat=(z_hat[b:b + 1].cpu() - zh_r).abs().max().item(),
                    o_hat=(o_hat[b:b + 1].cpu() - o_r).abs().max().item())
        print("B=32 x T=861, item", b, errs)
        assert max(errs["z"], errs["z_p"], errs["z_hat"]) <= LATENT_TOL, errs
        assert errs["o_hat"] <= O_HAT_TOL, errs


@pytest.mark.gpu
def test_graph_replay_is_bit_identical_to_eager_launches(synth_sd):
    """HIP-graph replay of the conversion (engine.GraphedConversion) = the same kernels with the same arguments:
    outputs must equal the eager path's bit for bit, on a second set of inputs too (static buffers refreshed),
    with ragged lengths and per-item speaker embeddings, and after the engine has moved on to another shape."""
    model = _model(synth_sd, zero_g=False)
    B, T = 3, 70
    gen = torch.Generator().manual_seed(77)

    def inputs(seed_shift):
        spec = (torch.rand(B, 513, T, generator=gen) * torch.linspace(3, 0.05, 513)[None, :, None]).to(DEV)
        lengths = torch.tensor([T, T - 9 - seed_shift, T - 30], dtype=torch.long, device=DEV)
        g_src, g_tgt = (0.3 * torch.randn(B, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)
        return spec, lengths, g_src, g_tgt, torch.randn(B, 192, T, generator=gen).to(DEV)

    a, b = inputs(0), inputs(4)
    eager = [model.voice_conversion(*x[:4], tau=0.3, noise=x[4]) for x in (a, b)]
    eager = [(o.clone(), m.clone(), [t.clone() for t in lat]) for o, m, lat in eager]
    for x, (o_e, m_e, lat_e) in zip((a, b, a), eager + eager[:1]):
        o_g, m_g, lat_g = model.voice_conversion(*x[:4], tau=0.3, noise=x[4], graph=True)
        torch.cuda.synchronize()
        assert torch.equal(o_g, o_e) and torch.equal(m_g, m_e)
        assert all(torch.equal(g, e) for g, e in zip(lat_g, lat_e))
    # another shape evicts the engine's workspace of (B, T); the captured graph keeps its own alive
    model.voice_conversion(a[0][:1, :, :33].contiguous(), torch.tensor([33], device=DEV), a[2][:1], a[3], tau=0.3,
                           noise=a[4][:1, :, :33].contiguous())
    o_g = model.voice_conversion(*b[:4], tau=0.3, noise=b[4], graph=True)[0]
    torch.cuda.synchronize()
    assert torch.equal(o_g, eager[1][0])
    eng = model.engine()
    assert len(eng._graphs) == 1
    with pytest.raises(RuntimeError):
        eng.graphed(B, T, 0.3, B, 1)(a[0][:, :, :T - 1], a[1], a[2], a[3])


def test_concurrent_resblock_chains_of_the_fp32_generator_are_bit_identical_to_the_serial_order(synth_sd):
    """``ConverterEngine.chain_streams``: at small batches (what ``ToneColorConverter.convert`` issues: batch 1,
    openvoice/api.py:141-160) the three ResBlock chains of a generator stage run on three HIP streams; the MRF sum
    (openvoice/models.py:280-286) keeps its order through events, so ``o_hat`` equals the one-stream order bit for bit
    -- fused and unfused pairs, twice in a row (scratch buffers are reused), under a non-default current stream, and
    from a captured graph."""
    from openvoice_amd.engine import ConverterEngine
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    gen = torch.Generator().manual_seed(11)
    for B, T in ((1, 120), (3, 65)):
        spec = (torch.randn(B, 513, T, generator=gen).abs() * torch.linspace(3, 0.05, 513)[None, :, None]).to(DEV)
        lengths = torch.full((B,), T, dtype=torch.int64, device=DEV)
        g1, g2 = (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)
        noise = torch.randn(B, 192, T, generator=gen).to(DEV)
        eng = ConverterEngine(synth_sd, CFG, 513, DEV, zero_g=True)
        run = lambda: eng.voice_conversion(spec, lengths, g1, g2, tau=0.3, noise=noise)[0].clone()
        for fuse in (True, False):
            eng.fuse_pairs = fuse
            eng.chain_streams = 1
            serial = run()
            eng.chain_streams = 3
            assert B <= eng.chain_streams_max_batch
            a, b = run(), run()
            side = torch.cuda.Stream(DEV)
            side.wait_stream(torch.cuda.current_stream(DEV))
            with torch.cuda.stream(side):
                c = run()
            side.synchronize()
            torch.cuda.synchronize()
            assert torch.isfinite(serial).all()
            assert torch.equal(a, serial) and torch.equal(b, serial) and torch.equal(c, serial), (B, fuse)
            if fuse:
                serial_fused = serial
        eng.fuse_pairs = True
        graphed = eng.graphed(B, T, 0.3)(spec, lengths, g1, g2, noise=noise)[0].clone()
        assert torch.equal(graphed, serial_fused)
        assert "dec_extra" in eng._workspace(B, T)             # the concurrent chains really had their own scratch


def test_non_released_config_matches_oracle():
    """The engine is shape-driven, not constant-driven (reference: openvoice/models.py:225-270 builds the generator from
    the JSON): a configuration no released checkpoint uses -- three upsampling stages 8 x 8 x 4 from 256 channels, two
    ResBlock kernels with two dilations each, inter = hidden = 128 -- against the oracle on the same weights."""
    from openvoice_amd.params import synthetic_state_dict
    from oracle import vc_oracle
    cfg = dict(CONVERTER_MODEL_CONFIG, upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8],
               upsample_initial_channel=256, inter_channels=128, hidden_channels=128, resblock_kernel_sizes=[3, 7],
               resblock_dilation_sizes=[[1, 3], [1, 5]])
    sd = synthetic_state_dict(cfg, 513, seed=11)
    B, T = 2, 70
    gen = torch.Generator().manual_seed(77)
    spec = torch.rand(B, 513, T, generator=gen).abs() * torch.linspace(3, 0.05, 513)[None, :, None]
    g_src, g_tgt = 0.3 * torch.randn(1, 256, 1, generator=gen), 0.3 * torch.randn(1, 256, 1, generator=gen)
    noise = torch.randn(B, cfg["inter_channels"], T, generator=gen)
    lengths = torch.tensor([T, T - 9], dtype=torch.long)
    with torch.no_grad():
        o_ref, mask_ref, (z_r, zp_r, zh_r) = vc_oracle.voice_conversion(sd, cfg, spec, lengths, g_src, g_tgt, 0.3, noise)
    model = SynthesizerTrn(0, 513, n_speakers=0, **cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    o_hat, y_mask, (z, z_p, z_hat) = model.voice_conversion(spec.to(DEV), lengths.to(DEV), g_src.to(DEV), g_tgt.to(DEV),
                                                            tau=0.3, noise=noise.to(DEV))
    torch.cuda.synchronize()
    assert o_hat.shape == o_ref.shape == (B, 1, 256 * T) and torch.equal(y_mask.cpu(), mask_ref)
    errs = dict(z=(z.cpu() - z_r).abs().max().item(), z_p=(z_p.cpu() - zp_r).abs().max().item(),
                z_hat=(z_hat.cpu() - zh_r).abs().max().item(), o_hat=(o_hat.cpu() - o_ref).abs().max().item())
    print(errs, "|o|max", o_ref.abs().max().item())
    assert max(errs["z"], errs["z_p"], errs["z_hat"]) <= LATENT_TOL and errs["o_hat"] <= O_HAT_TOL, errs
    # and the unsupported neighbours are named, not discovered as launch failures
    from openvoice_amd._lib import OvError
    with pytest.raises(OvError, match="resblock"):
        SynthesizerTrn(0, 513, n_speakers=0, **dict(cfg, resblock="2"))


def test_convert_and_extract_se_from_an_mp3_file(tmp_path, golden_dir, synth_sd):
    """BASELINE.json configs[0] AS WRITTEN -- ``ToneColorConverter.convert`` / ``extract_se`` on an MP3 file (reference:
    openvoice/api.py:123,144 ``librosa.load``): kaleido's invalid_keypress.mp3 (tests/golden/mp3_invalid_keypress.mp3, 0.52 s
    of joint stereo at 44.1 kHz) goes through ``openvoice_amd.mp3`` (pinned against FFmpeg, tests/test_mp3_cpu.py), the
    channel mean and the kaiser_best resampler to the model rate, then through the HIP path; checked against the CPU
    oracle on the same decoded samples."""
    import json
    import numpy as np
    from openvoice_amd import api, audio_io
    from openvoice_amd.utils import default_converter_hparams
    from oracle import vc_oracle
    mp3_path = os.path.join(golden_dir, "mp3_invalid_keypress.mp3")
    hps = default_converter_hparams("v2")
    cfg = {"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_sd}, tmp_path / "checkpoint.pth")
    tcc = api.ToneColorConverter(str(tmp_path / "config.json"), device=DEV, enable_watermark=False)
    tcc.load_ckpt(str(tmp_path / "checkpoint.pth"))
    wave, sr = audio_io.load(mp3_path, 22050)
    assert sr == 22050 and 0.4 < len(wave) / sr < 0.6 and np.abs(wave).max() > 0.1
    se = tcc.extract_se(mp3_path)
    assert se.shape == (1, 256, 1) and torch.isfinite(se).all()
    tgt = 0.3 * torch.randn(1, 256, 1, generator=torch.Generator().manual_seed(3))
    audio = tcc.convert(mp3_path, se, tgt.to(DEV), output_path=None, tau=0.0)
    with torch.no_grad():
        spec = vc_oracle.spectrogram(torch.from_numpy(wave)[None])
        se_ref = vc_oracle.reference_encoder(synth_sd, spec.transpose(1, 2)).unsqueeze(-1)
        o_ref = vc_oracle.voice_conversion(synth_sd, dict(hps.model.items()), spec, torch.tensor([spec.shape[2]]), se.cpu(),
                                           tgt, 0.0, torch.zeros(1, 192, spec.shape[2]), zero_g=True)[0]
    assert (se.cpu() - se_ref).abs().max().item() <= 1e-4
    assert audio.shape == (spec.shape[2] * 256,) and np.abs(audio - o_ref[0, 0].numpy()).max() <= 1e-3
    # the same call with the opt-in split-precision generator stages (API switch): fp32-level agreement
    audio_split = tcc.enable_split_bf16x3().convert(mp3_path, se, tgt.to(DEV), output_path=None, tau=0.0)
    tcc.enable_split_bf16x3(False)
    assert np.abs(audio_split - o_ref[0, 0].numpy()).max() <= 1e-4 and np.abs(audio_split - audio).max() <= 1e-4
