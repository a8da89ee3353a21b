"""Many-voice enrolment on the device: the ragged ReferenceEncoder kernels of csrc/ref_enc_ragged.hip
(``ov_layernorm_freq_ragged_f32``, ``ov_conv2d_s2_relu_ragged_f32``, ``ov_gru_ragged_f32``), then
``ConverterEngine.reference_encoder_ragged``, ``ToneColorConverter.extract_se_many`` and ``se_extractor.get_se_many``.

Two references per kernel:

* its DENSE twin (csrc/ref_enc.hip) run on each item's own unpadded tensor -- ``torch.equal`` over the item's columns,
  because the ragged kernel is specified to perform the twin's operations in the twin's order;
* PyTorch's own operator in float64 per item, at the tolerance of tests/test_gpu_ref_enc.py (max-abs err <=
  2e-5 * max(1, |ref|max)), with that file's inputs and conditioning checks.

Lengths: T in {1, 2, 3, 5, 64, 65, 127, 128, 129, 255, 257} -- odd and even at different halvings, both sides of the
256-column block edge of the LayerNorm grid -- in batches with the shortest item first, last and alone.  An input's
columns beyond its item's length are NaN and every output buffer starts as NaN: the item's columns must come out
finite, the columns from its end to the row stride exactly 0, and the surplus behind the buffer still NaN."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib  # noqa: E402
from openvoice_amd.engine import ref_enc_lengths  # noqa: E402
from test_gpu_ref_enc import (H, TAIL, _bar, _conv_inputs, _conv_pre64, _dev_in, _dev_out, _err,  # noqa: E402
                              _gru_conditioning, _gru_setup, _ln_fp32_two_pass, _ln_inputs, _ln_ref, _spec,
                              _trained_looking_sd)

DEV = "cuda:0"
NAN = float("nan")
# every length of the issue's list is in one of these; the shortest item first, last, and alone
BATCHES = {"shortest_first": [1, 257, 64, 129, 5, 128],
           "shortest_last": [255, 65, 2, 127, 3, 257, 1],
           "alone": [1],
           "alone_long": [257]}
assert {t for b in BATCHES.values() for t in b} == {1, 2, 3, 5, 64, 65, 127, 128, 129, 255, 257}
BATCH_IDS = list(BATCHES)


def _ld_of(lens, extra=0):
    """Row stride of a batch: the longest item rounded up to 4 floats (257 -> 260: the LayerNorm grid's second block
    then holds valid columns and tail columns), plus ``extra``."""
    return (max(lens) + 3) // 4 * 4 + extra


def _ragged(items, ld):
    """Items ``[C.., T_n]`` (time last) -> one ``[N, C.., ld]`` tensor whose columns beyond each item are NaN."""
    out = torch.full((len(items),) + tuple(items[0].shape[:-1]) + (ld,), NAN)
    for n, it in enumerate(items):
        out[n, ..., :it.shape[-1]] = it
    return out


def _lens_dev(lens):
    return torch.tensor(lens, dtype=torch.int32).to(DEV)


def _split(buf, shape, what):
    """The device buffer -> its ``shape`` part on the host, after checking that the TAIL behind it is still NaN."""
    torch.cuda.synchronize()
    flat = buf.cpu()
    n = int(np.prod(shape))
    assert torch.isnan(flat[n:]).all(), f"{what}: the kernel wrote past the end of its output"
    return flat[:n].view(shape)


def _check_item(got_item, got_tail, dense, ref64, what):
    """One item of a ragged output: finite, bit-identical to the dense kernel's output for the item alone, within the
    float64 bar, and an all-zero tail."""
    assert torch.isfinite(got_item).all(), f"{what}: non-finite output (a read past the item's end, or unwritten)"
    assert got_tail.numel() == 0 or (got_tail == 0).all(), f"{what}: columns past the item's end must be exactly 0"
    assert not torch.isnan(got_tail).any()
    err, bar = _err(got_item, ref64), _bar(ref64)
    print(f"{what}: max-abs err vs float64 {err:.3e} (bar {bar:.3e}); equal to the dense kernel: "
          f"{torch.equal(got_item, dense)}")
    assert torch.equal(got_item, dense), f"{what}: differs from the dense kernel on the item alone"
    assert err <= bar, f"{what}: max-abs err {err:.3e} > {bar:.3e}"


# ---- 1. ov_layernorm_freq_ragged_f32 ---------------------------------------------------------------------------------
def _ln_case(lens, Fq, kind, extra=0, table=None):
    N, ld = len(lens), _ld_of(lens, extra)
    items, refs = [], []
    gamma = beta = None
    for n, T in enumerate(lens):
        x, g, b = _ln_inputs(kind, "random", 1, Fq, T)
        if gamma is None:
            gamma, beta = g, b                       # one affine per launch
        ref = _ln_ref(x, gamma, beta, 1e-5)
        e32 = _err(_ln_fp32_two_pass(x, gamma, beta, 1e-5), ref)
        assert e32 <= _bar(ref) / 4, f"ill-conditioned input: fp32 on the CPU is {e32:.3e} from float64"
        items.append(x[0])
        refs.append(ref[0])
    xd, gd, bd = _dev_in(_ragged(items, ld)), _dev_in(gamma), _dev_in(beta)
    yd = _dev_out(N * Fq * ld)
    _lib.call("ov_layernorm_freq_ragged_f32", xd, gd, bd, _lens_dev(lens if table is None else table), yd, N, Fq, ld,
              1e-5)
    got = _split(yd, (N, Fq, ld), "layernorm")
    for n, T in enumerate(lens):
        dd = _dev_out(Fq * T)
        _lib.call("ov_layernorm_freq_f32", _dev_in(items[n]), gd, bd, dd, 1, Fq, T, 1e-5)
        dense = _split(dd, (Fq, T), "dense layernorm")
        _check_item(got[n, :, :T], got[n, :, T:], dense, refs[n], f"layernorm F{Fq} item {n} T{T} ld{ld}")


@pytest.mark.parametrize("batch", BATCH_IDS)
@pytest.mark.parametrize("Fq,kind", [(513, "spec"), (513, "randn"), (7, "randn")])
def test_layernorm_freq_ragged(Fq, kind, batch):
    _ln_case(BATCHES[batch], Fq, kind, extra=4 if batch == "alone" else 0)


# ---- 2. ov_conv2d_s2_relu_ragged_f32 ---------------------------------------------------------------------------------
# (Cin, Cout, Fi): layers 0, 2 and 5 of the stack at their real sizes, and an even / odd pair of small images
CONV_CFGS = [(1, 32, 513), (32, 64, 129), (128, 128, 17), (16, 16, 6), (16, 16, 5)]


def _conv_case(lens, Cin, Cout, Fi, extra_in=0, extra_out=0, table=None, ld_in=None):
    N, ld_in = len(lens), _ld_of(lens, extra_in) if ld_in is None else ld_in
    ld_out = (ld_in - 1) // 2 + 1 + extra_out
    Fo = (Fi - 1) // 2 + 1
    _, w, b = _conv_inputs(N, Cin, Cout, Fi, max(lens))
    items = [_conv_inputs(1, Cin, Cout, Fi, T)[0][0] * (1 + 0.1 * n) for n, T in enumerate(lens)]
    xd, wd, bd = _dev_in(_ragged(items, ld_in)), _dev_in(w), _dev_in(b)
    yd = _dev_out(N * Cout * Fo * ld_out)
    _lib.call("ov_conv2d_s2_relu_ragged_f32", xd, wd, bd, _lens_dev(lens if table is None else table), yd, N, Cin,
              Cout, Fi, ld_in, ld_out)
    got = _split(yd, (N, Cout, Fo, ld_out), "conv")
    for n, T in enumerate(lens):
        To = ref_enc_lengths(T, 1)[1]
        dd = _dev_out(Cout * Fo * To)
        _lib.call("ov_conv2d_s2_relu_f32", _dev_in(items[n]), wd, bd, dd, 1, Cin, Cout, Fi, T)
        dense = _split(dd, (Cout, Fo, To), "dense conv")
        ref = _conv_pre64(items[n][None], w, b).relu()[0]
        assert ref.shape == (Cout, Fo, To)
        _check_item(got[n, :, :, :To], got[n, :, :, To:], dense, ref,
                    f"conv {Cin}->{Cout} F{Fi} item {n} T{T} ld {ld_in}->{ld_out}")


@pytest.mark.parametrize("batch", BATCH_IDS)
@pytest.mark.parametrize("Cin,Cout,Fi", CONV_CFGS)
def test_conv2d_s2_relu_ragged(Cin, Cout, Fi, batch):
    """Row strides are ld_in / ld_out, not the item's length: ``shortest_last`` and ``alone`` run with an output row
    wider than the longest item needs, ``alone_long`` with a wider input row too."""
    _conv_case(BATCHES[batch], Cin, Cout, Fi, extra_in=8 if batch == "alone_long" else 0,
               extra_out=0 if batch == "shortest_first" else 3)


# ---- 3. ov_gru_ragged_f32 --------------------------------------------------------------------------------------------
def _gru_case(lens, gain, extra=0, table=None):
    N, ld = len(lens), _ld_of(lens, extra)
    gru, x = _gru_setup(N, max(lens), gain)
    items, refs = [], []
    whh = bhh = None
    for n, T in enumerate(lens):
        gi, whh, bhh, ref, _ = _gru_conditioning(gru, x[n:n + 1, :T].contiguous())
        items.append(gi[0])
        refs.append(ref[0])
    gid, wd, bd = _dev_in(_ragged(items, ld)), _dev_in(whh.t().contiguous()), _dev_in(bhh)
    hd = _dev_out(N * H)
    _lib.call("ov_gru_ragged_f32", gid, wd, bd, _lens_dev(lens if table is None else table), hd, N, H, ld)
    got = _split(hd, (N, H), "gru")
    for n, T in enumerate(lens):
        dd = _dev_out(H)
        _lib.call("ov_gru_f32", _dev_in(items[n]), wd, bd, dd, 1, H, T)
        dense = _split(dd, (H,), "dense gru")
        _check_item(got[n], got[n, :0], dense, refs[n], f"gru gain{gain} item {n} T{T} ld{ld}")


@pytest.mark.parametrize("batch", BATCH_IDS)
@pytest.mark.parametrize("gain", [1, 2])
def test_gru_ragged_final_state(gain, batch):
    """The state after each item's own last step: a padded step (its gi is NaN here) would show at once."""
    _gru_case(BATCHES[batch], gain, extra=4 if batch == "alone" else 0)


# ---- a length table the host wrapper would refuse: clamped in the kernel -----------------------------------------------
def test_lengths_outside_the_row_are_clamped():
    """``lens[n] > ld`` behaves as ``ld`` and ``lens[n] < 0`` as 0 (all-zero rows, h = h0 = 0): nothing outside the rows
    is read or written.  Every input is TAIL floats longer than its rows, so even an unclamped kernel would stay inside
    the test's own allocations -- it would show as a NaN or as a written surplus, not as a fault.  Where a missing clamp
    would show: the conv at an ODD row stride (ld_in = 7: the last output column's third tap is ti = 7 = ld_in, the
    next row's first element, valid only for an unclamped Ti) and the GRU (steps past the row).  The LayerNorm returns
    on t >= ld before it looks at the length, and a negative length gives no column and no step with or without the
    clamp: those parts pin the stated behaviour only."""
    lens, ld = [8, 8, 8], 8
    bad = [8 + 50, -3, 8]
    _ln_case(lens[:1] + lens[2:], 7, "randn", table=[bad[0], bad[2]])
    _conv_case(lens[:1] + lens[2:], 16, 16, 5, table=[bad[0], bad[2]])
    _conv_case([7, 7], 16, 16, 5, table=[7 + 50, 7], ld_in=7)
    _conv_case([7, 5, 7], 16, 16, 6, table=[7 + 1, 5, 7 + 50], ld_in=7)
    _gru_case(lens[:1] + lens[2:], 1, table=[bad[0], bad[2]])
    x = torch.randn(3, 7, ld, generator=torch.Generator().manual_seed(5))
    yd = _dev_out(3 * 7 * ld)
    _lib.call("ov_layernorm_freq_ragged_f32", _dev_in(x), _dev_in(torch.ones(7)), _dev_in(torch.zeros(7)),
              _lens_dev(bad), yd, 3, 7, ld, 1e-5)
    y = _split(yd, (3, 7, ld), "layernorm, bad table")
    assert torch.isfinite(y).all() and (y[1] == 0).all() and y[0].abs().max() > 0 and y[2].abs().max() > 0
    xc = torch.randn(3, 16, 5, ld, generator=torch.Generator().manual_seed(6))
    w, b = torch.randn(16, 16, 3, 3) / 12, torch.ones(16)
    yd = _dev_out(3 * 16 * 3 * 4)
    _lib.call("ov_conv2d_s2_relu_ragged_f32", _dev_in(xc), _dev_in(w), _dev_in(b), _lens_dev(bad), yd, 3, 16, 16, 5,
              ld, 4)
    y = _split(yd, (3, 16, 3, 4), "conv, bad table")
    assert torch.isfinite(y).all() and (y[1] == 0).all() and y[0].abs().max() > 0
    hd = _dev_out(3 * H)
    _lib.call("ov_gru_ragged_f32", _dev_in(torch.randn(3, 3 * H, ld)), _dev_in(torch.randn(H, 3 * H) / 11),
              _dev_in(torch.zeros(3 * H)), _lens_dev(bad), hd, 3, H, ld)
    h = _split(hd, (3, H), "gru, bad table")
    assert torch.isfinite(h).all() and (h[1] == 0).all() and h[0].abs().max() > 0


# ---- 4. the encoder: reference_encoder_ragged against reference_encoder per item ------------------------------------
@pytest.fixture(scope="module")
def trained_looking(synth_sd):
    """tests/test_gpu_ref_enc.py's model: the synthetic converter weights with a LayerNorm affine that differs for
    every f and conv / GRU biases of std 0.3."""
    from openvoice_amd.models import SynthesizerTrn
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG
    sd = _trained_looking_sd(synth_sd)
    model = SynthesizerTrn(0, 513, n_speakers=0, zero_g=False, **CONVERTER_MODEL_CONFIG)
    model.load_state_dict(sd, strict=True)
    return sd, model.to(DEV).eval()


def _dense_stack(eng, x):
    """LayerNorm + the six convs of ``ConverterEngine.reference_encoder`` on one dense ``[N, F, T]`` input, through
    the dense entry points with the engine's own weights."""
    re = eng.ref_enc
    N, F, T = x.shape
    cur = torch.empty_like(x)
    _lib.call("ov_layernorm_freq_f32", x, re["ln_w"], re["ln_b"], cur, N, F, T, 1e-5)
    cin = 1
    for w, b in re["convs"]:
        cout, Fo, To = w.shape[0], (F - 1) // 2 + 1, (T - 1) // 2 + 1
        nxt = torch.empty(N, cout, Fo, To, dtype=torch.float32, device=x.device)
        _lib.call("ov_conv2d_s2_relu_f32", cur, w, b, nxt, N, cin, cout, F, T)
        cur, cin, F, T = nxt, cout, Fo, To
    return cur


@pytest.mark.parametrize("batch", BATCH_IDS)
def test_reference_encoder_ragged_equals_reference_encoder_per_item(trained_looking, batch):
    """Row p of the ragged call against ``reference_encoder`` on item p alone, with the input's tail NaN: the conv stack
    output and the embedding bit for bit.  ``shortest_last`` hands the spectrogram over as a ``[:, :, :W]`` view of
    a wider buffer (the form ``_NativeSpectrogram.windows_multi`` returns)."""
    _, model = trained_looking
    eng = model.engine()
    lens = BATCHES[batch]
    W = max(lens)
    items = [_spec(1, T, 7000 + 10 * n + T)[0] for n, T in enumerate(lens)]
    if batch == "shortest_last":
        spec = _ragged(items, _ld_of(lens)).to(DEV)[:, :, :W]
        assert not spec.is_contiguous()
    else:
        spec = _ragged(items, W).to(DEV)
    got = eng.reference_encoder_ragged(spec, lens).clone()
    stack, steps, L = eng._reference_encoder_ragged_stack(spec, lens)
    torch.cuda.synchronize()
    assert got.shape == (len(lens), 256) and torch.isfinite(got).all()
    assert steps.tolist() == [ref_enc_lengths(T)[-1] for T in lens] and L == stack.shape[3]
    assert torch.isfinite(stack).all()
    for p, T in enumerate(lens):
        alone = items[p][None].to(DEV)
        dense_stack = _dense_stack(eng, alone)
        To = dense_stack.shape[3]
        assert torch.equal(stack[p, :, :, :To], dense_stack[0]), f"item {p} T{T}: conv stack output differs"
        assert (stack[p, :, :, To:] == 0).all(), f"item {p} T{T}: conv stack tail must be 0"
        dense = eng.reference_encoder(alone.transpose(1, 2))
        err = (got[p] - dense[0]).abs().max().item()
        print(f"ragged ref_enc item {p} T{T}: max-abs diff to the dense path {err:.3e}")
        assert torch.equal(got[p], dense[0]), f"item {p} T{T}: embedding differs from the dense path by {err:.3e}"


def test_reference_encoder_ragged_rejects_bad_lengths(trained_looking):
    _, model = trained_looking
    eng = model.engine()
    spec = _spec(2, 9, 1).to(DEV)
    for frames in ([9], [9, 0], [9, 10], [9, 9, 9]):
        with pytest.raises(ValueError):
            eng.reference_encoder_ragged(spec, frames)


# ---- 5. extract_se_many against extract_se_from_audio per voice -----------------------------------------------------
SR = 22050


@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("enrol")
    hps = default_converter_hparams("v2")
    cfg = {"_version_": "v2", "data": dict(hps.data.items()), "model": dict(hps.model.items())}
    (d / "config.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    conv = api.ToneColorConverter(str(d / "config.json"), device=DEV, enable_watermark=False)
    conv.load_ckpt(str(d / "checkpoint.pth"))
    return conv


def _voice_audio(n, seed, lead=0):
    """``n`` samples of a wandering tone in noise (every frame active), after ``lead`` samples of digital silence
    (leading silence is what the detector always removes)."""
    t = np.arange(n)
    rng = np.random.default_rng(seed)
    f0 = 150 + 40 * seed
    x = (0.4 * np.sin(2 * np.pi * (f0 + 30 * np.sin(2 * np.pi * t / (0.73 * SR))) * t / SR)
         + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return np.concatenate([np.zeros(lead, dtype=np.float32), x])


# 4 voices of 1, 2, 3 and 3 pieces of about 1 s whose lengths differ by 1 to 500 samples
PIECE_SAMPLES = [[SR], [SR + 1, SR + 500], [SR + 257, SR + 256, SR + 2], [SR + 130, SR + 499, SR + 31]]


def _voices(vad):
    lead = int(0.25 * SR) if vad else 0          # with the detector on, every other piece starts with silence
    return [[_voice_audio(n, 10 * v + i, lead=lead * ((v + i) % 2)) for i, n in enumerate(ns)]
            for v, ns in enumerate(PIECE_SAMPLES)]


@pytest.mark.parametrize("vad", [False, True])
def test_extract_se_many_equals_extract_se_from_audio_per_voice(tcc, vad):
    voices = _voices(vad)
    counts = [len(v) for v in voices]
    se, pieces = tcc.extract_se_many(voices, vad=vad, return_pieces=True)
    assert tcc.last_extract_se_batches == [sum(counts)]
    assert se.shape == (4, 256, 1) and pieces.shape == (sum(counts), 256)
    assert torch.isfinite(se).all() and torch.isfinite(pieces).all()
    p = 0
    for v, voice in enumerate(voices):
        solo = [tcc.extract_se_from_audio([a], vad=vad).reshape(-1) for a in voice]
        for i, g in enumerate(solo):
            diff = (pieces[p + i] - g).abs().max().item()
            print(f"vad={vad} voice {v} piece {i}: max-abs diff to extract_se_from_audio {diff:.3e}")
            assert torch.equal(pieces[p + i], g), f"voice {v} piece {i}: piece embedding differs by {diff:.3e}"
        want = tcc.extract_se_from_audio(voice, vad=vad)
        n = len(voice)
        bound = n * 2.0 ** -23 * max(g.abs().max().item() for g in solo)
        err = (se[v:v + 1] - want).abs().max().item()
        print(f"vad={vad} voice {v}: mean differs by {err:.3e} (bound {bound:.3e})")
        assert want.shape == (1, 256, 1) and err <= bound, (v, err, bound)
        p += n
    if vad:       # the detector did remove something: the pieces that start with silence are shorter afterwards
        plain = tcc.extract_se_many(voices, vad=False)
        assert not torch.equal(plain, se)
    for cap, sizes in ((1, [1] * 9), (2, [2, 2, 2, 2, 1])):
        se_c, pieces_c = tcc.extract_se_many(voices, vad=vad, max_pieces_per_launch=cap, return_pieces=True)
        assert tcc.last_extract_se_batches == sizes
        assert torch.equal(pieces_c, pieces) and torch.equal(se_c, se), f"results depend on the cap ({cap})"
    assert torch.equal(tcc.extract_se_many(voices, vad=vad), se), "return_pieces must not change the result"


def test_extract_se_many_refuses_what_extract_se_from_audio_refuses(tcc):
    quiet = np.zeros(SR, dtype=np.float32)
    with pytest.raises(ValueError, match="no frame above"):
        tcc.extract_se_many([[_voice_audio(SR, 1)], [quiet]], vad=True)
    with pytest.raises(ValueError, match="shorter than the reflect padding"):
        tcc.extract_se_many([[_voice_audio(SR, 1), _voice_audio(300, 2)]])


# ---- 6. get_se_many against get_se per path ------------------------------------------------------------------------------
def test_get_se_many_equals_get_se_per_path(tcc, tmp_path):
    from openvoice_amd import audio_io, se_extractor
    # 1, 2 and 3 pieces; the second starts with 2 s of silence, the third's pieces differ by one sample
    specs = [("a.wav", 6 * SR, 0), ("b.wav", 16 * SR, 2 * SR), ("c.wav", 27 * SR + 100, 0)]
    paths = []
    for name, n, lead in specs:
        audio_io.write(str(tmp_path / name), _voice_audio(n, len(paths) + 3, lead=lead), SR)
        paths.append(str(tmp_path / name))
    one = [se_extractor.get_se(p, tcc, target_dir=str(tmp_path / "one")) for p in paths]
    many = se_extractor.get_se_many(paths, tcc, target_dir=str(tmp_path / "many"))
    assert tcc.last_extract_se_batches == [6]
    assert len(many) == 3
    for (se1, name1), (se2, name2), n_pieces in zip(one, many, (1, 2, 3)):
        assert name1 == name2
        files1 = sorted(os.listdir(tmp_path / "one" / name1 / "wavs"))
        files2 = sorted(os.listdir(tmp_path / "many" / name2 / "wavs"))
        assert files1 == files2 and len(files1) == n_pieces
        segs = []
        for f in files1:
            a, b = tmp_path / "one" / name1 / "wavs" / f, tmp_path / "many" / name2 / "wavs" / f
            assert a.read_bytes() == b.read_bytes(), f"{f}: piece files differ"
            segs.append(str(a))
        biggest = max(tcc.extract_se(s).abs().max().item() for s in segs)
        bound = n_pieces * 2.0 ** -23 * biggest
        err = (se1 - se2).abs().max().item()
        print(f"{name1}: {n_pieces} pieces, se differs by {err:.3e} (bound {bound:.3e})")
        assert se2.shape == (1, 256, 1) and err <= bound, (name1, err, bound)
        saved = torch.load(tmp_path / "many" / name2 / "se.pth")
        assert torch.equal(saved, se2.cpu())
    lens = [len(audio_io.load(str(tmp_path / "many" / many[2][1] / "wavs" / f), SR)[0])
            for f in sorted(os.listdir(tmp_path / "many" / many[2][1] / "wavs"))]
    assert len(set(lens)) > 1, "the three pieces of c.wav are meant to differ in length"
