"""``speed=`` / ``duration=`` on the MI355X: ``ov_stretch_rows_f32`` against the mirror of ``openvoice_amd/stretch.py``, its
bit identities and record checks, and the stretched conversion end to end -- one pass, per item, bf16, long-form, marked
and resampled.  Small shapes throughout; the definition is the project's own (nothing in the reference stretches)."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, audio_io, longform, stretch  # noqa: E402
from openvoice_amd.engine import stretch_rows  # noqa: E402
from openvoice_amd.generator import GENERATOR_MARGIN  # noqa: E402
from openvoice_amd.mel_processing import spectrogram_torch  # noqa: E402

DEV = "cuda:0"
HOP, NFFT = 256, 1024
ONE = stretch.ONE
SENTINEL = -7.5
O_HAT_TOL = 1e-4          # across kernel families, the bar of tests/test_gpu_longform.py and of batch independence
SPEEDS = [0.5, 0.75, 1.0, 1.37, 2.0]
U = 2.0 ** -24


def _launch(recs, src, dst, device_recs=None):
    host = torch.tensor([v for r in recs for v in r], dtype=torch.int64)
    table = host.to(DEV) if device_recs is None else torch.tensor([v for r in device_recs for v in r], dtype=torch.int64).to(DEV)
    stretch_rows(table, host, len(recs), src, dst)


def _case(rows, T_in, step, src_off=5, dst_off=3, pad_src=3, pad_dst=5):
    """(record, source elements, destination elements) of one item with unaligned offsets and ld > T."""
    n = stretch.t_out(T_in, step)
    sld, dld = T_in + pad_src, n + pad_dst
    rec = stretch.record(src_off, dst_off, rows, sld, dld, T_in, 0, 0, n, step)
    return rec, src_off + rows * sld + 2, dst_off + rows * dld + 2, n


def _rows_of(buf, off, rows, ld, n):
    return buf[off:off + rows * ld].view(rows, ld)[:, :n]


# ---- the kernel against the mirror ----------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_kernel_matches_the_mirror_and_the_three_rounding_bound(binding, monkeypatch, capsys):
    """out = fl(a + fl(f * fl(b - a))) with |eps_k| <= u = 2^-24 each and f in [0, 1) exact:
    fl(b - a) = d (1 + e1), the product f d (1 + e1)(1 + e2) differs from f d by at most |d| (2u + u^2), and the sum is
    (a + m)(1 + e3) = out, so its rounding is at most u |out| / (1 - u).  Against the exact a + f (b - a):
        |out - exact| <= u (2 |b - a| + |out|) + u^2 (|b - a| + 2 |out|) <= u (2 |b - a| + |out|) (1 + 2u),
    element by element; the float64 reference adds 2^-53 relative, far below the u^2 term.  The integer ramp has b - a = 1,
    so f * 1 is exact and out = fl(i + f) is ONE rounding of an exactly known number: equality reads i (and f) back."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for rows in (1, 3, 192):
        for T_in in (1, 2, 17, 65):
            for speed in SPEEDS:
                step = stretch.step_of(speed)
                rec, S, D, n = _case(rows, T_in, step)
                sld = rec[3]
                i, f = stretch.positions(0, n, step)
                # the ramp: row r holds t + 128 r
                ramp = (torch.arange(sld, dtype=torch.float32)[None] + 128.0 * torch.arange(rows, dtype=torch.float32)[:, None])
                normal = torch.randn(rows, sld, generator=gen)
                for kind, x in (("ramp", ramp), ("normal", normal)):
                    src = torch.full((S,), float("nan"))
                    src[5:5 + rows * sld] = x.reshape(-1)
                    dst = torch.full((D,), SENTINEL, device=DEV)
                    _launch([rec], src.to(DEV), dst)
                    got = _rows_of(dst, 3, rows, rec[4], n).cpu().numpy()
                    untouched = dst.clone()
                    _rows_of(untouched, 3, rows, rec[4], n).fill_(SENTINEL)
                    assert bool((untouched == SENTINEL).all()), "wrote outside its rows"
                    z = x[:, :T_in].numpy()
                    assert np.array_equal(got, stretch.stretch_rows(z, step)), (kind, rows, T_in, speed)
                    a = z[:, i].astype(np.float64)
                    b = z[:, np.minimum(i + 1, T_in - 1)].astype(np.float64)
                    exact = a + f.astype(np.float64)[None] * (b - a)
                    if kind == "ramp":
                        assert np.array_equal(got, exact.astype(np.float32))
                        # where i + f is representable (f a multiple of the spacing) the integer part IS i
                        assert np.array_equal(np.floor(got[0, f < 1 - 2.0 ** -8]), i[f < 1 - 2.0 ** -8].astype(np.float32))
                    else:
                        bound = U * (2 * np.abs(b - a) + np.abs(got)) * (1 + 2 * U)
                        err = np.abs(got.astype(np.float64) - exact)
                        assert np.all(err <= bound), (rows, T_in, speed, (err / np.maximum(bound, 1e-300)).max())
                        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    with capsys.disabled():
        print(f"\nov_stretch_rows_f32 [{binding}]: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


# ---- bit identity ----------------------------------------------------------------------------------------------------
def test_speed_one_copies_and_items_do_not_depend_on_the_launch():
    gen = torch.Generator().manual_seed(9)
    rec, S, D, n = _case(192, 65, ONE)
    src = torch.randn(S, generator=gen).to(DEV)
    dst = torch.full((D,), SENTINEL, device=DEV)
    _launch([rec], src, dst)
    assert torch.equal(_rows_of(dst, 3, 192, rec[4], 65), _rows_of(src, 5, 192, rec[3], 65))
    # five records of different rows, lengths and speeds in one launch: each the bits of its solo launch
    shapes = [(192, 65, 0.75), (3, 17, 2.0), (1, 1, 0.5), (192, 17, 1.37), (5, 300, 1.0)]
    recs, so, do = [], 1, 2
    for rows, T_in, speed in shapes:
        step = stretch.step_of(speed)
        n = stretch.t_out(T_in, step)
        recs.append(stretch.record(so, do, rows, T_in + 1, n + 2, T_in, 0, 0, n, step))
        so, do = so + rows * (T_in + 1) + 3, do + rows * (n + 2) + 1
    src = torch.randn(so, generator=gen).to(DEV)
    together = torch.full((do,), SENTINEL, device=DEV)
    _launch(recs, src, together)
    for rec in recs:
        solo = torch.full((do,), SENTINEL, device=DEV)
        _launch([rec], src, solo)
        mine = lambda t: _rows_of(t, rec[1], rec[2], rec[4], rec[8])
        assert torch.equal(mine(together), mine(solo)) and bool((mine(solo) != SENTINEL).any())


@pytest.mark.parametrize("speed", [0.75, 1.37])
def test_a_window_record_holds_the_bits_of_the_whole_row_stretch(speed):
    """T_in = 65, window core [20, 45): a slice with context, column 0 being global frame i0, writes the output frames from
    j0 on -- torch.equal to the slice of the whole-row stretch."""
    T, rows, lo, hi = 65, 192, 20, 45
    step = stretch.step_of(speed)
    z = torch.randn(rows, T, generator=torch.Generator().manual_seed(3)).to(DEV)
    n = stretch.t_out(T, step)
    whole = torch.empty(rows, n, device=DEV)
    _launch([stretch.record(0, 0, rows, T, n, T, 0, 0, n, step)], z, whole)
    j_lo, j_hi = stretch.first_output_at(lo, step), stretch.first_output_at(hi, step)
    a, b = lo - 4, hi + 4
    piece = z[:, a:b].contiguous()
    out = torch.full((rows, j_hi - j_lo), SENTINEL, device=DEV)
    _launch([stretch.record(0, 0, rows, b - a, j_hi - j_lo, b - a, a, j_lo, j_hi - j_lo, step)], piece, out)
    assert torch.equal(out, whole[:, j_lo:j_hi])
    i, _ = stretch.positions(j_lo, j_hi - j_lo, step)
    assert lo <= i[0] and i[-1] < hi


# ---- bad records -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_bad_records_are_refused_and_never_executed(binding, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    step = stretch.step_of(0.75)
    T, rows = 17, 3
    n = stretch.t_out(T, step)
    src = torch.randn(rows * T, generator=torch.Generator().manual_seed(1)).to(DEV)
    good = stretch.record(0, 0, rows, T, n, T, 0, 0, n, step)
    bad = {
        "beyond the source extent": stretch.record(1, 0, rows, T, n, T, 0, 0, n, step),
        "beyond the destination extent": stretch.record(0, 1, rows, T, n, T, 0, 0, n, step),
        "i past the slice": stretch.record(0, 0, rows, T, n, T - 1, 0, 0, n, step),
        "negative reach": stretch.record(0, 0, rows, T, n, T, 1, 0, n, step),
        "negative offset": stretch.record(-4, 0, rows, T, n, T, 0, 0, n, step),
        "step out of range": stretch.record(0, 0, rows, T, n, T, 0, 0, n, 3 * ONE),
    }
    for why, rec in bad.items():
        assert not stretch.check_record(rec, src.numel(), rows * n), why
        # in the host table: the call returns OV_E_BADARG and launches nothing, the good record next to it included
        for recs in ([rec], [good, rec]):
            dst = torch.full((rows * n,), SENTINEL, device=DEV)
            with pytest.raises(_lib.OvError, match="OV_E_BADARG"):
                _launch(recs, src, dst)
            torch.cuda.synchronize()
            assert bool((dst == SENTINEL).all()), why
        # in the DEVICE table only (the host copy says otherwise): the kernel's own check refuses to execute it
        dst = torch.full((rows * n,), SENTINEL, device=DEV)
        _launch([good], src, dst, device_recs=[rec])
        torch.cuda.synchronize()
        assert bool((dst == SENTINEL).all()), why
    # ... and only it: the good record next to it in the same launch is written
    dst = torch.full((2 * rows * n,), SENTINEL, device=DEV)
    second = stretch.record(0, rows * n, rows, T, n, T, 0, 0, n, step)
    _launch([good, second], src, dst, device_recs=[bad["negative reach"], second])
    torch.cuda.synchronize()
    assert bool((dst[:rows * n] == SENTINEL).all()) and bool((dst[rows * n:] != SENTINEL).all())
    assert stretch.check_record(good, src.numel(), rows * n)
    for args in [(None, torch.zeros(10, dtype=torch.int64), 1, src, src.numel(), src, src.numel()),
                 (torch.zeros(10, dtype=torch.int64, device=DEV), None, 1, src, src.numel(), src, src.numel()),
                 (torch.zeros(10, dtype=torch.int64, device=DEV), torch.zeros(10, dtype=torch.int64), 0, src, src.numel(), src,
                  src.numel())]:
        with pytest.raises(_lib.OvError):
            _lib.call("ov_stretch_rows_f32", *args)


# ---- end to end --------------------------------------------------------------------------------------------------------
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
def tcc(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "stretch_plain", enable_watermark=False)


@pytest.fixture(scope="module")
def native(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "stretch_native", watermark="native", watermark_key=77)


@pytest.fixture(scope="module")
def ses():
    gen = torch.Generator().manual_seed(31)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


@pytest.fixture
def direct(tcc, native):
    """The direct conv kernels, whose results do not depend on what shares a launch or where a tile starts."""
    engines = [t.model.engine() for t in (tcc, native)]
    saved = [e.use_winograd for e in engines]
    for e in engines:
        e.use_winograd = False
    yield
    for e, s in zip(engines, saved):
        e.use_winograd = s


def _wave(n, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    phase = 2 * np.pi * torch.cumsum(140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / 22050.0
    y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float().to(DEV)


FRAMES = (33, 17)


@pytest.fixture(scope="module")
def pair():
    return [_wave(HOP * T, T) for T in FRAMES]


def _composed(tcc, waves, ses, steps, seed, generator=None):
    """What the issue defines: (the stretched call's o_hat, the generator run on the stretched masked z_hat), the second
    built from the call's OWN returned z_hat by the mirror and handed to the engine's public generator step."""
    g_src, g_tgt = ses
    eng = tcc.model.engine()
    specs = [spectrogram_torch(w[None], NFFT, 22050, HOP, NFFT, center=False)[0] for w in waves]
    frames = [s.shape[1] for s in specs]
    assert tuple(frames) == FRAMES[:len(waves)] or len(waves) == 1
    B, T = len(specs), max(frames)
    spec = torch.zeros(B, 513, T, device=DEV)
    for b, s in enumerate(specs):
        spec[b, :, :s.shape[1]] = s
    kw = {} if generator is None else {"generator": generator}
    o, y_mask, (z, z_p, z_hat) = tcc.model.voice_conversion(spec, torch.tensor(frames), g_src, g_tgt, tau=0.3,
                                                            seed=[(seed, b) for b in range(B)], stretch=steps, **kw)
    n_out = [stretch.t_out(t, s) for t, s in zip(frames, steps)]
    T2 = max(n_out)
    assert z_hat.shape == (B, 192, T) and o.shape == (B, 1, HOP * T2) and y_mask.shape == (B, 1, T2)
    assert y_mask[:, 0].sum(1).long().tolist() == n_out
    gws = eng.generator_workspace(B, T2)
    zs = torch.zeros(B, 192, gws["Tp"], device=DEV)
    for b in range(B):
        assert float(z_hat[b, :, frames[b]:].abs().max()) == 0.0 if frames[b] < T else True
        zs[b, :, :n_out[b]] = torch.from_numpy(stretch.stretch_rows(z_hat[b, :, :frames[b]].cpu().numpy(), steps[b])).to(DEV)
    g = g_tgt.reshape(1, -1).contiguous()
    ref = eng.generate(zs, T2, torch.tensor(n_out, device=DEV), eng.generator.cond(eng._g(g)), g, gws,
                       skip_padding=any(n != T2 for n in n_out), use_bf16=generator == "bf16")
    return o, ref, n_out


@pytest.mark.parametrize("speed", [0.75, 1.37, 2.0])
def test_convert_batch_speed_is_the_generator_on_the_stretched_latent(tcc, ses, pair, direct, speed):
    steps = [stretch.step_of(speed)] * 2
    o, ref, n_out = _composed(tcc, pair, ses, steps, 7)
    assert torch.equal(o, ref)
    got, lens = tcc.convert_batch(pair, *ses, tau=0.3, seed=7, speed=speed)
    assert torch.equal(got, o)
    assert lens.tolist() == [n * HOP for n in n_out]
    # a stretched call holds frame-rate tensors for T and generator scratch for T_out only
    eng = tcc.model.engine()
    frames_ws = [w for k, w in eng._ws.items() if len(k) == 3]
    assert frames_ws and all("dec" not in w and "pre" not in w for w in frames_ws)
    assert eng._stretch_ws[0] == (2, max(n_out))
    short = min(range(2), key=lambda b: n_out[b])
    assert float(got[short, 0, n_out[short] * HOP:].abs().max()) == 0.0          # the padded tail is zero
    assert float(got[short, 0, :n_out[short] * HOP].abs().max()) > 0.0


def test_speed_none_and_one_are_todays_call(tcc, ses, pair):
    today, lens = tcc.convert_batch(pair, *ses, tau=0.3, seed=7)
    for speed in (None, 1.0, [1.0, None]):
        got, n = tcc.convert_batch(pair, *ses, tau=0.3, seed=7, speed=speed)
        assert torch.equal(got, today) and torch.equal(n, lens)
    dense = torch.stack([pair[0], pair[0]])
    assert torch.equal(tcc.convert_batch(dense, *ses, seed=3, speed=1.0)[0], tcc.convert_batch(dense, *ses, seed=3)[0])
    with pytest.raises(ValueError):
        tcc.convert_batch(pair, *ses, speed=2.5)
    with pytest.raises(ValueError, match="one per item"):
        tcc.convert_batch(pair, *ses, speed=[1.0, 1.2, 1.3])


def test_a_per_item_speed_list_gives_each_item_its_solo_call(tcc, ses, pair, direct):
    """33 frames at 1.5 and 17 at 17 / 21.5 both make 22 frames: the stretched batch is dense, and item b equals its solo call
    everywhere, bit for bit with the direct kernels.  With output lengths that differ, the shorter item sits in a padded
    row; the reference generator is unmasked, so -- as for any ragged ``convert_batch`` -- its last frames see what lies
    beyond its end: there the items are compared up to the generator's reach before the end."""
    speeds = [1.5, 17 / 21.5]
    n_out = [stretch.t_out(T, stretch.step_of(s)) for T, s in zip(FRAMES, speeds)]
    assert n_out == [22, 22]
    both, lens = tcc.convert_batch(pair, *ses, tau=0.3, seed=[(5, 0), (5, 1)], speed=speeds)
    for b in range(2):
        solo, n = tcc.convert_batch([pair[b]], *ses, tau=0.3, seed=[(5, b)], speed=speeds[b])
        assert int(n[0]) == int(lens[b]) == 22 * HOP and torch.equal(solo[0], both[b])
    speeds = [0.75, 0.5]
    n_out = [stretch.t_out(T, stretch.step_of(s)) for T, s in zip(FRAMES, speeds)]
    both, lens = tcc.convert_batch(pair, *ses, tau=0.3, seed=[(5, 0), (5, 1)], speed=speeds)
    assert lens.tolist() == [n * HOP for n in n_out] and n_out[1] < n_out[0]
    for b in range(2):
        solo, n = tcc.convert_batch([pair[b]], *ses, tau=0.3, seed=[(5, b)], speed=speeds[b])
        keep = (n_out[b] if n_out[b] == max(n_out) else max(1, n_out[b] - GENERATOR_MARGIN)) * HOP
        assert int(n[0]) == n_out[b] * HOP and torch.equal(solo[0, :, :keep], both[b, :, :keep])


def test_default_kernels_hold_the_batch_independence_bar(tcc, ses, pair):
    speeds = [1.5, 17 / 21.5]
    both, _ = tcc.convert_batch(pair, *ses, tau=0.3, seed=[(5, 0), (5, 1)], speed=speeds)
    for b in range(2):
        solo, _ = tcc.convert_batch([pair[b]], *ses, tau=0.3, seed=[(5, b)], speed=speeds[b])
        assert float((solo[0] - both[b]).abs().max()) <= O_HAT_TOL


def test_the_bf16_generator_runs_on_the_stretched_latent(tcc, ses, pair):
    steps = [stretch.step_of(0.75), stretch.step_of(1.37)]
    o, ref, n_out = _composed(tcc, pair, ses, steps, 11, generator="bf16")
    assert bool(torch.isfinite(o).all()) and torch.equal(o, ref)
    fp32 = _composed(tcc, pair, ses, steps, 11)[0]
    assert 0.0 < float((o - fp32).abs().max()) < 0.1                        # another generator, the same audio


def test_convert_takes_speed_and_duration(tcc, ses, tmp_path):
    path = str(tmp_path / "one_second.wav")
    audio_io.write(path, _wave(22050, 4).cpu().numpy(), 22050)
    plain = tcc.convert(path, *ses, seed=5)
    T = longform.frames_of(22050, NFFT, HOP)
    fast = tcc.convert(path, *ses, seed=5, speed=1.25)
    assert len(plain) == T * HOP and len(fast) == stretch.t_out(T, stretch.step_of(1.25)) * HOP
    slow = tcc.convert(path, *ses, seed=5, duration=1.4)
    assert abs(len(slow) - 1.4 * 22050) <= HOP
    assert np.array_equal(slow, tcc.convert_long(path, *ses, seed=5, duration=1.4))      # one window: the same call
    with pytest.raises(ValueError):
        tcc.convert(path, *ses, speed=1.2, duration=1.0)
    with pytest.raises(ValueError):
        tcc.convert(path, *ses, duration=0.3)                                # would need speed 3.3


# ---- long-form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed,window_frames,windows", [(0.75, 255, 5), (1.5, 285, 3)])
def test_convert_long_speed_matches_the_one_pass_stretched_conversion(tcc, ses, speed, window_frames, windows):
    """T = 310 frames in windows of 2 x context + 15 frames (the smallest the context of the speed allows): direct kernels
    bit for bit, default kernels within the cross-family bar -- what tests/test_gpu_longform.py holds the unstretched pair
    to."""
    T = 310
    wave = _wave(HOP * T, 60)
    noise = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(60)).to(DEV)
    step = stretch.step_of(speed)
    ctx = longform.stretch_context_frames(tcc.model.model_cfg, step)
    assert window_frames == 2 * ctx + 15 and len(longform.plan_windows(T, window_frames, ctx, 15)) == windows >= 3
    eng = tcc.model.engine()
    try:
        eng.use_winograd = False
        a = tcc.convert_batch(wave[None], *ses, tau=0.3, noise=noise, speed=speed)[0][0, 0].clone()
        b = tcc.convert_long(wave, *ses, tau=0.3, window_frames=window_frames, windows_per_launch=2, noise=noise, speed=speed)
        err_direct = float(np.abs(a.cpu().numpy() - b).max())
    finally:
        eng.use_winograd = True
    c = tcc.convert_batch(wave[None], *ses, tau=0.3, noise=noise, speed=speed)[0][0, 0].clone()
    d = tcc.convert_long(wave, *ses, tau=0.3, window_frames=window_frames, windows_per_launch=2, noise=noise, speed=speed)
    err_default = float(np.abs(c.cpu().numpy() - d).max())
    print(f"convert_long(speed={speed}) vs one pass, T = {T}: direct {err_direct:.3e}, default {err_default:.3e}")
    assert b.shape == d.shape == (stretch.t_out(T, step) * HOP,)
    assert err_direct == 0.0
    assert err_default <= O_HAT_TOL


# ---- marked and resampled ----------------------------------------------------------------------------------------------
def test_convert_many_marks_and_resamples_the_stretched_waveform(native, tcc, ses, direct):
    """The marked, resampled, stretched ``convert_many`` against its composition: the UNMARKED stretched conversion, marked,
    then resampled.  The expectation is marked by the host loop ``add_watermark`` with the same model, not by
    ``mark_many`` -- the call under test runs ``mark_many`` itself, so the host loop is the independent reference (the two
    are held equal bit for bit in tests/test_gpu_watermark.py)."""
    message = "@MyShell"
    waves = [_wave(4 * 22050, 21), _wave(35280, 23)]
    speeds = [0.75, 1.5]
    many = native.convert_many(waves, *ses, message=message, seed=9, speed=speeds, out_sr=16000)
    unmarked = tcc.convert_many(waves, *ses, seed=9, speed=speeds)
    d = tcc.hps.data
    for i, (got, raw) in enumerate(zip(many, unmarked)):
        T = longform.frames_of(waves[i].numel(), d.filter_length, d.hop_length)
        assert len(raw) == stretch.t_out(T, stretch.step_of(speeds[i])) * HOP
        marked = native.add_watermark(raw.copy(), message)                     # the host loop with the same model
        ref = audio_io.resample_on_device(torch.from_numpy(marked).to(DEV), 22050, 16000).cpu().numpy()
        assert np.array_equal(got, ref), i
    assert native.detect_watermark(native.convert_many(waves[:1], *ses, message=message, seed=9, speed=0.75)[0], 2) == message
    # an item left alone in a stretched call is today's conversion of it
    mixed = tcc.convert_many(waves, *ses, seed=9, speed=[None, 1.5])
    assert np.array_equal(mixed[0], tcc.convert_many(waves, *ses, seed=9)[0]) and np.array_equal(mixed[1], unmarked[1])
