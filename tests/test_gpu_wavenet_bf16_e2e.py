"""``wavenet="bf16"`` end to end on the MI355X: the posterior encoder's and the flow's WaveNet layers on
``ov_wn_layer_bf16`` (bf16 matrix operands, fp32 state) through ``voice_conversion``, the captured graph, ``convert``,
``convert_long``, a live stream and ``infer``.  Synthetic weights, B = 2, T = 40 and 64.

The bar on z, z_p, z_hat and (fp32 generator) o_hat against the fp32 oracle is MEASURED, not chosen: on the CPU,
``wn_bf16_ref.measure_e2e`` runs the fp32 oracle (oracle/vc_oracle.py) with the kernel's operand roundings hooked into
its WaveNet layers and compares it with the unmodified oracle on the inputs below, five seeds; the largest deviations
were z 1.561e-02, z_p 2.053e-02, z_hat 1.883e-02, o_hat 5.337e-03, and the bar is 3 x each (the project's practice for
chained roundings).  The fp32 path's 1e-3 parity bar is not claimed for this mode."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wn_bf16_ref as R  # noqa: E402
from openvoice_amd import _lib  # noqa: E402
from openvoice_amd.models import SynthesizerTrn  # noqa: E402
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU = 0.3
MEASURED = R.E2E_MEASURED            # recomputed on the CPU by tests/test_wn_bf16_criterion_cpu.py
BAR = {k: 3 * v for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def model(synth_sd):
    m = SynthesizerTrn(0, 513, n_speakers=0, **CFG)
    m.load_state_dict(synth_sd, strict=False)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def oracle_out(synth_sd):
    """The unmodified fp32 oracle on the test's inputs (seed 0), computed once."""
    from oracle import vc_oracle
    out = {}
    for T in R.E2E_LENGTHS:
        spec, lengths, g_src, g_tgt, noise = R.e2e_inputs(T, 0)
        with torch.no_grad():
            o, _, lat = vc_oracle.voice_conversion(synth_sd, CFG, spec, lengths, g_src, g_tgt, TAU, noise)
        out[T] = dict(zip(("z", "z_p", "z_hat", "o_hat"), lat + (o,)))
    return out


def _vc(model, T, **kw):
    spec, lengths, g_src, g_tgt, noise = (t.to(DEV) for t in R.e2e_inputs(T, 0))
    o, mask, lat = model.voice_conversion(spec, lengths, g_src, g_tgt, tau=TAU, noise=noise, **kw)
    return dict(zip(("z", "z_p", "z_hat", "o_hat"), tuple(t.clone() for t in lat) + (o.clone(),)))


@pytest.mark.parametrize("T", R.E2E_LENGTHS)
def test_voice_conversion_within_the_measured_bar(model, oracle_out, T):
    eng = model.engine()
    default, fp32 = _vc(model, T), _vc(model, T, wavenet="fp32")
    for generator in ("fp32", "bf16"):
        got = _vc(model, T, wavenet="bf16", generator=generator)
        assert eng._wn_bf16_on is False and eng._wn_choice is None
        for name in ("z", "z_p", "z_hat", "o_hat"):
            assert got[name].shape == oracle_out[T][name].shape and torch.isfinite(got[name]).all(), (name, generator)
            if name == "o_hat" and generator == "bf16":
                continue
            dev = (got[name].cpu() - oracle_out[T][name]).abs().max().item()
            print(f"[wavenet bf16 e2e] T={T} generator={generator} {name}: max-abs against the fp32 oracle {dev:.3e} "
                  f"(bar {BAR[name]:.3e})")
            assert dev <= BAR[name], (name, dev)
        assert not torch.equal(got["z"], fp32["z"]), "wavenet='bf16' ran the fp32 layers"
    for name in default:
        assert torch.equal(default[name], fp32[name]), name       # the default is the fp32 path, bit for bit


def test_switch_keyword_and_graph_agree(model):
    T = 40
    eng = model.engine()
    kw = _vc(model, T, wavenet="bf16")
    graphed = _vc(model, T, wavenet="bf16", graph=True)
    eng.use_bf16_wavenet(True)
    try:
        switch = _vc(model, T)
        over = _vc(model, T, wavenet="fp32")           # the keyword wins over the switch, without touching it
        assert eng._wn_bf16_on is True
    finally:
        eng.use_bf16_wavenet(False)
    back = _vc(model, T)
    for name in kw:
        assert torch.equal(kw[name], switch[name]), name
        assert torch.equal(kw[name], graphed[name]), name
        assert torch.equal(over[name], back[name]), name
    assert not torch.equal(kw["z"], back["z"])
    for junk in ("half", 16, "BF16"):
        with pytest.raises(_lib.OvError):
            _vc(model, T, wavenet=junk)


# ---- the converter's public pieces --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("wavenet_bf16")
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


def _wave(n, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050
    return (0.3 * torch.sin(2 * torch.pi * 170.0 * t) + 0.02 * torch.randn(n, generator=gen, dtype=torch.float64)).float().to(DEV)


def test_live_stream_and_convert_long_equal_the_one_pass_conversion(tcc):
    """As tests/test_gpu_live_bf16.py does for the generator: at one seed, a live stream at chunk 15 and ``convert_long``
    with ``wavenet="bf16"`` ARE the one-pass ``convert_batch`` with ``wavenet="bf16"`` -- the layer's results do not
    depend on tile, row or batch."""
    gen = torch.Generator().manual_seed(3)
    src, tgt = ((0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV) for _ in range(2))
    n = 256 * 64 + 100
    wave, seed = _wave(n, 11), 5
    one = tcc.convert_batch(wave[None], src, tgt, seed=[seed], wavenet="bf16")[0][0, 0]
    fp32 = tcc.convert_batch(wave[None], src, tgt, seed=[seed])[0][0, 0]
    assert torch.isfinite(one).all() and not torch.equal(one, fp32)
    long_ = torch.as_tensor(tcc.convert_long(wave, src, tgt, seed=seed, wavenet="bf16")).to(DEV)
    m = min(long_.numel(), one.numel())
    assert m >= (n // 256) * 256 and torch.equal(long_[:m], one[:m])
    st = tcc.live_stream(src, tgt, chunk_frames=15, seed=seed, wavenet="bf16")
    outs, i = [], 0
    while i < n:
        outs.append(st.push(wave[i:i + 2205]))
        i += 2205
    outs.append(st.close())
    live = torch.cat(outs)
    m = min(live.numel(), one.numel())
    assert m >= (n // 256) * 256 and torch.equal(live[:m], one[:m])
    assert tcc.model.engine()._wn_bf16_on is False


# ---- TTS ---------------------------------------------------------------------------------------------------------------
def test_infer_runs_and_a_padded_batch_equals_the_item_alone(synth_tts_sd):
    m = SynthesizerTrn(68, 513, n_speakers=10, **CFG)
    m.load_state_dict(synth_tts_sd, strict=True)
    m = m.to(DEV).eval()
    gen = torch.Generator().manual_seed(21)
    B, Tx = 2, 10
    lengths = torch.tensor([10, 6])
    tokens = torch.randint(1, 68, (B, Tx), generator=gen)
    tokens[1, 6:] = 0
    sid = torch.tensor([3, 7])
    seeds = [(9, b) for b in range(B)]
    run = lambda sl, n, **kw: m.infer(tokens[sl, :n].to(DEV), lengths[sl].to(DEV), sid=sid[sl].to(DEV), seed=seeds[sl],
                                      length_scale=3.0, skip_padding=True, **kw)
    both = slice(0, 2)
    o, _, y_mask, lat = run(both, Tx, wavenet="bf16")
    o32, _, _, lat32 = run(both, Tx)
    assert torch.isfinite(o).all() and torch.equal(lat[1], lat32[1]) and not torch.equal(lat[0], lat32[0])   # z_p same, z differs
    frames = y_mask[:, 0].sum(1).long().tolist()
    n = frames[1]
    # The flow's output of the short item is the same bits in the padded batch and alone: the bf16 layer's results do not
    # depend on batch, row or tile.
    o1, _, _, lat1 = run(slice(1, 2), 6, wavenet="bf16")
    assert n > 0 and o1.shape[-1] >= n * 256 and torch.isfinite(o1).all()
    assert torch.equal(lat[0][1, :, :n], lat1[0][0, :, :n])
    # The waveform: the generator is unmasked (the reference's too), so behind the short item's last frame the padded batch
    # holds the activations of z = 0 where the item alone has the convs' zero padding, and the last ~13 frames differ on
    # every path (tests/test_gpu_tts_items.py); and the fp32 generator chooses its kernels by launch size.  On the bf16
    # generator, whose direct convolutions do not depend on the launch, every sample further than the generator's margin
    # from the item's end is the same bits in the padded batch and alone.
    margin = m.engine().core.generator_margin
    keep = (n - margin) * 256
    assert keep > 0, (n, margin)
    ob = run(both, Tx, wavenet="bf16", generator="bf16")[0]
    o1b = run(slice(1, 2), 6, wavenet="bf16", generator="bf16")[0]
    d = (ob[1, 0, :keep] - o1b[0, 0, :keep]).abs().max().item()
    print(f"[wavenet bf16 e2e] infer: item alone against row 2 of the padded batch over {keep} samples ({n} frames, margin "
          f"{margin}): max-abs {d:.3e}")
    assert torch.equal(ob[1, 0, :keep], o1b[0, 0, :keep])
