"""The native watermark on the MI355X (openvoice_amd/watermark.py, csrc/watermark.hip): the embed kernel against the
float64 mirror under a derived per-sample bound, its own mark read back by the detect kernel and by the mirror, batch /
position / alignment independence, the silent window, rejected records, and the converter's output paths end to end.

The per-sample bound (u = 2^-24, one fp32 rounding; x is the same fp32 input on both sides, exact in float64):

* p_j: a thread adds its ceil(L / 256) products in order (c x is exact), three more additions join the eight partials of
  a bit and one division by |S_j| follows: at most L / 256 + 5 <= L / 32 + 3 roundings (L >= 512), each relative to a
  partial sum that is at most sum_{S_j} |x|.  So |dp_j| <= (L / 32 + 3) u mean_{S_j} |x|.
* a: x^2 is fused into the sum; ceil(L / 256) additions per thread, eight through the tree, one division by L: the mean
  square carries at most (L / 256 + 10) u relative, its root half of that plus one rounding, the product with strength
  one more, and fp32(strength) differs from the mirror's double by at most u: |da| <= (L / 512 + 9) u a.  max(., floor)
  does not enlarge an error.
* d_j = b max(a - b p_j, 0): |dd_j| <= |dp_j| + |da| + u |d_j|  (the subtraction rounds once; max and the signs are
  exact and 1-Lipschitz).
* y_i = x_i +- d_j, one rounding: |dy_i| <= |dd_j| + u (|x_i| + |d_j| + |dd_j|).

A factor 1 + 2^-10 covers the second-order terms dropped above."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, audio_io, watermark  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
KEY, STRENGTH, FLOOR = 0x1234ABCD5678, watermark.DEFAULT_STRENGTH, watermark.DEFAULT_FLOOR
PAYLOADS = [0xA5A5A5A5, 0x00000000, 0xFFFFFFFF, 0x0F0F1234, 0x80000001]
GAPS = [0, 1, 2, 3, 4]          # sentinel samples in front of window k: the window starts run through every alignment


def _bits(word):
    return np.array([(word >> j) & 1 for j in range(32)], dtype=np.float64)


def _content(kind, L, gen):
    t = torch.arange(L, dtype=torch.float64) / 22050.0
    if kind == 0:
        return (0.1 * torch.randn(L, generator=gen, dtype=torch.float64)).float()
    if kind == 1:
        return (0.3 * torch.sin(2 * np.pi * 220.0 * t)).float()
    if kind == 2:
        return torch.zeros(L)
    if kind == 3:
        return (1e-5 * torch.randn(L, generator=gen, dtype=torch.float64)).float()
    return torch.randn(L, generator=gen, dtype=torch.float64).float()


def _layout(L, W):
    """W windows of L samples in one NaN-filled buffer: offsets, contents, payload words."""
    gen = torch.Generator().manual_seed(1000 * W + L)
    offs, acc = [], 0
    for k in range(W):
        acc += GAPS[k % 5]
        offs.append(acc)
        acc += L
    buf = torch.full((acc + 5,), float("nan"))
    xs = [_content(k % 5, L, gen) for k in range(W)]
    for o, x in zip(offs, xs):
        buf[o:o + L] = x
    return offs, xs, buf, PAYLOADS[:W]


def _embed(src, dst, recs):
    _lib.call("ov_wm_embed_windows_f32", src, src.numel(), dst, dst.numel(), torch.tensor(recs, dtype=torch.int64).to(DEV),
              len(recs), KEY, STRENGTH, FLOOR)


def _detect(src, recs):
    q = torch.full((len(recs), 32), float("nan"), device=DEV)
    level = torch.full((len(recs),), float("nan"), device=DEV)
    _lib.call("ov_wm_detect_windows_f32", src, src.numel(), torch.tensor(recs, dtype=torch.int64).to(DEV), len(recs), KEY,
              STRENGTH, FLOOR, q, level)
    return q, level


def _bound(x, bits):
    """(reference y, per-sample bound) of one window, both float64: the module docstring's derivation."""
    x = x.astype(np.float64)
    L = len(x)
    p, a = watermark.read_host(x, KEY, STRENGTH, FLOOR)
    b = 2.0 * bits - 1.0
    d = b * np.maximum(a[0] - b * p[0], 0.0)
    mabs = np.array([np.abs(x[j::32]).mean() for j in range(32)])
    dd = (L / 32 + 3) * U * mabs + (L / 512 + 9) * U * a[0] + U * np.abs(d)
    j = np.arange(L) % 32
    y = watermark.encode_host(x, bits[None], KEY, STRENGTH, FLOOR)
    return y, (dd[j] + U * (np.abs(x) + np.abs(d[j]) + dd[j])) * (1.0 + 2.0 ** -10), a[0]


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("L,W", [(16000, 1), (16000, 5), (512, 1), (512, 5), (16001, 1), (16001, 5)])
def test_embed_against_the_float64_mirror(L, W, binding, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    offs, xs, buf, words = _layout(L, W)
    assert W == 1 or len({o % 4 for o in offs}) >= 3          # aligned and unaligned window starts in one launch
    src = buf.to(DEV)
    # out of place, to destinations of yet another alignment
    d_offs = [o + 3 for o in offs]
    dst = torch.full((buf.numel() + 8,), float("nan"), device=DEV)
    _embed(src, dst, [(so, do, L, w) for so, do, w in zip(offs, d_offs, words)])
    # in place
    inp = src.clone()
    _embed(inp, inp, [(o, o, L, w) for o, w in zip(offs, words)])
    torch.cuda.synchronize()
    assert torch.equal(src.cpu().nan_to_num(nan=7.0), buf.nan_to_num(nan=7.0))           # the source is only read
    out, inp = dst.cpu(), inp.cpu()
    worst = 0.0
    touched_out, touched_in = torch.zeros(out.numel(), dtype=torch.bool), torch.zeros(inp.numel(), dtype=torch.bool)
    for o, do, x, w in zip(offs, d_offs, xs, words):
        y_ref, bound, _ = _bound(x.numpy(), _bits(w))
        y = out[do:do + L]
        assert torch.isfinite(y).all()
        assert torch.equal(y, inp[o:o + L])                                               # in place = out of place
        err = np.abs(y.numpy().astype(np.float64) - y_ref)
        worst = max(worst, float((err / bound).max()))
        touched_out[do:do + L] = True
        touched_in[o:o + L] = True
    print(f"L = {L}, W = {W}, {binding}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.isnan(out[~touched_out]).all() and torch.isnan(inp[~touched_in]).all()  # the sentinels stand


def test_src_offsets_0_1_3_and_16000_in_one_launch():
    """Windows at src_off 0, 1, 3 and 16000 of one source (they overlap: a source is only read), written to four
    differently aligned destinations by one launch: each is ``torch.equal`` to its own launch from offset 0."""
    L = 16000
    src = _content(0, 2 * L, torch.Generator().manual_seed(5)).to(DEV)
    s_offs, d_offs = [0, 1, 3, 16000], [2, L + 5, 2 * L + 9, 3 * L + 16]
    dst = torch.full((4 * L + 32,), float("nan"), device=DEV)
    _embed(src, dst, [(so, do, L, PAYLOADS[0]) for so, do in zip(s_offs, d_offs)])
    for so, do in zip(s_offs, d_offs):
        solo = src[so:so + L].clone()
        y1 = torch.empty_like(solo)
        _embed(solo, y1, [(0, 0, L, PAYLOADS[0])])
        assert torch.equal(y1, dst[do:do + L])
    dst = dst.cpu()
    mask = torch.ones(dst.numel(), dtype=torch.bool)
    for do in d_offs:
        mask[do:do + L] = False
    assert torch.isnan(dst[mask]).all()


@pytest.mark.parametrize("L", [16000, 512, 16001])
def test_own_mark_reads_back_and_a_window_does_not_depend_on_its_batch(L):
    """Device output decoded by the detect kernel and by the mirror: bits = payload and b_j q_j >= 0.99 a (the fp32
    rounding of y moves a projection by at most 2^-24 mean |y|, four orders below a).  Window w of the W = 5 launch is
    ``torch.equal`` to its own W = 1 launch, for the marked samples and for q_out / level_out."""
    W = 5
    offs, xs, buf, words = _layout(L, W)
    src = buf.to(DEV)
    recs = [(o, o, L, w) for o, w in zip(offs, words)]
    y5 = src.clone()
    _embed(y5, y5, recs)
    q5, a5 = _detect(y5, recs)
    for k, (o, x, w) in enumerate(zip(offs, xs, words)):
        solo = x.to(DEV)
        y1 = torch.empty_like(solo)
        _embed(solo, y1, [(0, 0, L, w)])
        assert torch.equal(y1, y5[o:o + L])
        q1, a1 = _detect(y1, [(0, 0, L, 0)])
        assert torch.equal(q1[0], q5[k]) and torch.equal(a1[0], a5[k])
        _, a = watermark.read_host(x.numpy(), KEY, STRENGTH, FLOOR)
        q_ref, _ = watermark.read_host(y1.cpu().numpy(), KEY, STRENGTH, FLOOR)
        b = 2.0 * _bits(w) - 1.0
        for q in (q1[0].cpu().numpy().astype(np.float64), q_ref[0]):
            assert np.all(b * q >= 0.99 * a[0]), (b * q / a[0]).min()
            assert np.array_equal(q >= 0, _bits(w) == 1)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_model_interface_and_the_silent_window(binding, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    wm = watermark.NativeWatermark(key=KEY).to(DEV)
    gen = torch.Generator().manual_seed(3)
    carrier = torch.stack([_content(k, 16000, gen) for k in (2, 0, 4)]).to(DEV)       # row 0: silence
    bits = torch.tensor(np.stack([_bits(w) for w in PAYLOADS[:3]]), dtype=torch.float32)
    y = wm.encode(carrier, bits.to(DEV))
    assert wm.launches == 1 and y.shape == carrier.shape and torch.isfinite(y).all()
    assert torch.equal(y, wm.encode(carrier, bits))                                    # host bits: the same records
    scores = wm.decode(y)
    assert wm.launches == 3 and scores.shape == (3, 32)
    assert torch.equal(scores >= 0.5, bits.to(DEV) == 1)
    _, level = wm.read(carrier)
    assert float(level[0]) == FLOOR                                                    # a == floor for the silent window
    assert torch.equal(y[0].abs(), torch.full((16000,), FLOOR, device=DEV))           # +- floor along the chips
    assert torch.equal(wm.decode(torch.zeros(1, 16000, device=DEV)), torch.full((1, 32), 0.5, device=DEV))
    # against the mirror's scores
    ref = watermark.decode_host(y.cpu().numpy(), KEY)
    assert np.abs(scores.cpu().numpy() - ref).max() <= 1e-5
    with pytest.raises(ValueError, match="512"):
        wm.encode(torch.zeros(1, 511, device=DEV), bits[:1])


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_rejected_records_write_nothing(binding, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    n = 20000
    src = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    dst = torch.full((n,), -7.0, device=DEV)
    bad = [(0, 0, 511, 1), (n - 15999, 0, 16000, 1), (0, n - 15999, 16000, 1), (-1, 0, 16000, 1), (0, -4, 16000, 1),
           (0, 0, 0, 1), (0, 0, 1 << 40, 1)]
    for rec in bad:                                       # the Python layer refuses them before any launch
        with pytest.raises(ValueError):
            watermark.embed_windows(src, dst, [rec], KEY)
    _embed(src, dst, bad + [(100, 2000, 512, 5)])         # the kernel's own checks: only the good record writes
    q, level = _detect(src, bad[:2] + [(0, 0, 512, 0)])
    torch.cuda.synchronize()
    out = dst.cpu()
    assert (out[:2000] == -7.0).all() and (out[2512:] == -7.0).all() and (out[2000:2512] != -7.0).all()
    assert torch.isnan(q[:2]).all() and torch.isnan(level[:2]).all() and torch.isfinite(q[2]).all()
    recs = torch.zeros(1, 4, dtype=torch.int64, device=DEV)
    for args in [(src, n, dst, n, recs, 0, KEY, STRENGTH, FLOOR), (src, n, dst, n, recs, 65536, KEY, STRENGTH, FLOOR),
                 (src, 0, dst, n, recs, 1, KEY, STRENGTH, FLOOR), (src, n, dst, 0, recs, 1, KEY, STRENGTH, FLOOR),
                 (src, n, dst, n, recs, 1, -1, STRENGTH, FLOOR), (src, n, dst, n, recs, 1, KEY, -0.5, FLOOR),
                 (src, n, dst, n, recs, 1, KEY, STRENGTH, 0.0), (src, n, dst, n, recs, 1, KEY, float("nan"), FLOOR)]:
        with pytest.raises(_lib.OvError):
            _lib.call("ov_wm_embed_windows_f32", *args)
    assert (dst.cpu() == out).all()


# ---- end to end: the converter's output paths -------------------------------------------------------------------------
MESSAGE = "@MyShell"


def _make(tmp_path_factory, synth_sd, name, **kw):
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp(name)
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, **kw)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


@pytest.fixture(scope="module")
def native(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "wm_native", watermark="native", watermark_key=KEY)


@pytest.fixture(scope="module")
def plain(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "wm_plain", enable_watermark=False)


@pytest.fixture(scope="module")
def ses():
    gen = torch.Generator().manual_seed(11)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


def _wave(n, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    phase = 2 * np.pi * torch.cumsum(140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / 22050.0
    y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float()


def test_constructor_keyword(native, plain, tmp_path_factory, synth_sd, capsys):
    assert isinstance(native.watermark_model, watermark.NativeWatermark) and native.watermark_model.key == KEY
    assert plain.watermark_model is None
    cfg = str(tmp_path_factory.getbasetemp() / "wm_native0" / "config.json")
    assert api.ToneColorConverter(cfg, device=DEV, watermark="native", enable_watermark=False).watermark_model is None
    capsys.readouterr()
    default = api.ToneColorConverter(cfg, device=DEV)        # watermark=None: the wavmark attempt and its print, as before
    try:
        import wavmark  # noqa: F401
        assert default.watermark_model is not None
    except ImportError:
        assert default.watermark_model is None and "wavmark is not installed: watermarking disabled" in capsys.readouterr().out
    with pytest.raises(ValueError, match="native"):
        api.ToneColorConverter(cfg, device=DEV, watermark="wavmark")


def test_convert_marks_on_the_device_what_the_host_loop_marks(native, plain, ses, tmp_path):
    path = str(tmp_path / "four_seconds.wav")
    audio_io.write(path, _wave(4 * 22050, 4).numpy(), 22050)
    wm = native.watermark_model
    before = wm.launches
    audio = native.convert(path, *ses, message=MESSAGE, seed=5)
    assert wm.launches == before + 1                                        # both windows, one launch
    assert native.detect_watermark(audio, 2) == MESSAGE
    unmarked = plain.convert(path, *ses, seed=5)                            # watermark off: today's output
    looped = native.add_watermark(unmarked.copy(), MESSAGE)                 # the host loop with the same model
    assert np.array_equal(audio, looped)
    outside = np.ones(len(audio), bool)
    outside[0:16000] = outside[32000:48000] = False
    assert np.array_equal(audio[outside], unmarked[outside]) and not np.array_equal(audio[~outside], unmarked[~outside])
    # through a file: the 16-bit WAV still reads
    out_path = str(tmp_path / "out.wav")
    native.convert(path, *ses, output_path=out_path, message=MESSAGE, seed=5)
    assert native.detect_watermark(audio_io.load(out_path, None)[0], 2) == MESSAGE
    # convert_long (one window plan or many) goes through _finish: the same marked audio at the model rate
    long_audio = native.convert_long(path, *ses, message=MESSAGE, seed=5)
    assert native.detect_watermark(long_audio, 2) == MESSAGE
    assert np.array_equal(long_audio, native.add_watermark(plain.convert_long(path, *ses, seed=5), MESSAGE))


@pytest.fixture
def direct(native, plain):
    """The direct conv kernels, whose results do not depend on what shares a launch: ``convert_many`` then equals the
    solo calls bit for bit (the other suites' pattern)."""
    engines = [t.model.engine() for t in (native, plain)]
    saved = [e.use_winograd for e in engines]
    for e in engines:
        e.use_winograd = False
    yield
    for e, s in zip(engines, saved):
        e.use_winograd = s


def test_convert_many_marks_every_item_in_one_launch(native, plain, ses, direct, capsys):
    waves = [_wave(4 * 22050, 21), _wave(11025, 22), _wave(35280, 23)]      # two windows, none (too short), one
    wm = native.watermark_model
    before = wm.launches
    capsys.readouterr()
    many = native.convert_many(waves, *ses, message=MESSAGE, seed=9)
    assert wm.launches == before + 1
    assert capsys.readouterr().out.count("Audio too short, fail to add watermark") == 2
    unmarked = plain.convert_many(waves, *ses, seed=9)
    for i, (got, raw) in enumerate(zip(many, unmarked)):
        solo = native.convert_long(waves[i], *ses, message=MESSAGE, seed=(9, i))
        assert np.array_equal(got, solo)
        assert np.array_equal(got, native.add_watermark(raw.copy(), MESSAGE))
    assert native.detect_watermark(many[0], 2) == MESSAGE
    assert np.array_equal(many[1], unmarked[1])                             # shorter than one window: untouched
    assert native.detect_watermark(many[2], 1) == MESSAGE[:4]
    # at another output rate the mark is applied at the model rate, before the resampler
    r16 = native.convert_many(waves[:1], *ses, message=MESSAGE, seed=9, out_sr=16000)[0]
    ref = audio_io.resample_on_device(torch.from_numpy(many[0]).to(DEV), 22050, 16000).cpu().numpy()
    assert np.array_equal(r16, ref)


def test_mark_many_on_separate_tensors(native):
    wm = native.watermark_model
    a, b = _wave(50000, 31).to(DEV), _wave(16000, 32).to(DEV)
    packed = torch.cat([a, b])
    views = [packed[:50000], packed[50000:]]
    wm.mark_many(views, [MESSAGE, "other"])
    before = wm.launches
    wm.mark_many([a, b], [MESSAGE, "other"])                                 # separate allocations: gathered, copied back
    assert wm.launches == before + 1
    assert torch.equal(a, views[0]) and torch.equal(b, views[1])
    assert native.detect_watermark(a.cpu().numpy(), 2) == MESSAGE
    assert native.detect_watermark(b.cpu().numpy(), 1) == "othe"
