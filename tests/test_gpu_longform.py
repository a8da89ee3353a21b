"""Recordings of any length on the MI355X (openvoice_amd/longform.py): the windowed framing kernel against the whole-file
planes, windowed conversion against the one-pass path and the oracle, the 55-minute file that one pass refuses, bounded
memory, and the streaming converter."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, longform  # noqa: E402
from openvoice_amd.hostinfo import usable_cpus  # noqa: E402
from openvoice_amd.mel_processing import native_spectrogram, spectrogram_torch  # noqa: E402

DEV = "cuda:0"
HOP, NFFT, PAD = 256, 1024, 384
O_HAT_TOL = 1e-4          # across kernel families (Winograd phase of a shifted window), as in test_gpu_e2e.py
ORACLE_TOL = 1e-3


@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("longform")
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


@pytest.fixture(scope="module")
def ses():
    gen = torch.Generator().manual_seed(31)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


def _wave(n, seed, device=DEV):
    """Speech-like test signal: a few drifting partials under a syllable-rate envelope, plus a little noise."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    f = 140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t)
    phase = 2 * np.pi * torch.cumsum(f, 0) / 22050.0
    y = 0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5) + 0.05 * torch.sin(7.3 * phase)
    y = y * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t)) + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)
    return y.float().to(device)


def _one_pass(model, wave, g_src, g_tgt, tau, noise):
    spec = spectrogram_torch(wave[None], NFFT, 22050, HOP, NFFT, center=False)
    T = spec.shape[2]
    o = model.voice_conversion(spec, torch.tensor([T], device=DEV), g_src, g_tgt, tau=tau, noise=noise)[0]
    return o[0, 0]


def _windowed(model, wave, g_src, g_tgt, tau, noise, Tw, wpl):
    conv = longform.WindowedConverter(model, NFFT, HOP, window_frames=Tw, windows_per_launch=wpl)
    return conv.convert(wave, g_src, g_tgt, tau=tau, noise=noise)


# ---- the framing kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Tw,firsts", [
    (256 * 300 + 77, 64, "edges"),        # N not a multiple of hop; windows touching the start, the end, the middle
    (256 * 40, 40, "whole"),              # one window = the whole file: touches both ends
    (256 * 1000 + 255, 997, "edges"),
    (1000, 1, "edges"),                   # two frames in all
])
def test_windowed_framing_matches_the_whole_file_planes_and_spectrogram(n, Tw, firsts):
    wave = _wave(n, n)
    T = longform.frames_of(n, NFFT, HOP)
    if firsts == "whole":
        starts = [0]
        Tw = T
    else:
        starts = sorted(set([0, T - Tw, max(0, T // 2 - Tw // 2), 1 if T - Tw >= 1 else 0, max(0, T - Tw - 1)]))
    U = T + 3
    ld = (U + 3) // 4 * 4
    whole = torch.full((1, HOP, ld), float("nan"), device=DEV)
    _lib.call("ov_frame_hops_f32", wave[None], whole, 1, n, HOP, PAD, U, ld)
    Uw = Tw + 3
    ldw = (Uw + 3) // 4 * 4
    firsts_dev = torch.tensor(starts, dtype=torch.int64, device=DEV)
    win = torch.full((len(starts), HOP, ldw), float("nan"), device=DEV)
    _lib.call("ov_frame_hops_windows_f32", wave, n, firsts_dev, len(starts), HOP, PAD, Uw, ldw, win)
    spec_whole = spectrogram_torch(wave[None], NFFT, 22050, HOP, NFFT, center=False)
    spec_win = native_spectrogram(DEV, NFFT, HOP).windows(wave, n, firsts_dev, Tw)
    torch.cuda.synchronize()
    for w, f0 in enumerate(starts):
        assert torch.equal(win[w, :, :Uw], whole[0, :, f0:f0 + Uw]), (n, Tw, f0)
        assert torch.all(win[w, :, Uw:] == 0)
        assert torch.equal(spec_win[w], spec_whole[0, :, f0:f0 + Tw]), (n, Tw, f0)


# ---- windowed conversion against one pass -----------------------------------------------------------------------------
def test_convert_long_matches_one_pass_at_60_s(tcc, ses):
    """T = 5168 frames, windows of 1024 (core 780): 7 windows in launches of 2 (4 launches), the last one shifted off the
    grid to end at T.  Direct kernels only: bit-identical.  Default (Winograd) kernels: within the cross-family bar."""
    model, (g_src, g_tgt) = tcc.model, ses
    n = 256 * 5168
    wave = _wave(n, 60)
    noise = torch.randn(1, 192, 5168, generator=torch.Generator().manual_seed(60)).to(DEV)
    plan = longform.plan_windows(5168, 1024, 120, 15)
    assert len(plan) == 7 and plan[-1][0] % 15 != 0
    eng = model.engine()
    try:
        eng.use_winograd = False
        a = _one_pass(model, wave, g_src, g_tgt, 0.3, noise).clone()
        b = _windowed(model, wave, g_src, g_tgt, 0.3, noise, 1024, 2)
        torch.cuda.synchronize()
        err_direct = (a - b).abs().max().item()
    finally:
        eng.use_winograd = True
    c = _one_pass(model, wave, g_src, g_tgt, 0.3, noise).clone()
    d = tcc.convert_long(wave, g_src, g_tgt, tau=0.3, window_frames=1024, windows_per_launch=2, noise=noise)
    err_default = np.abs(c.cpu().numpy() - d).max()
    print(f"convert_long vs one pass, T = 5168: direct kernels {err_direct:.3e}, default kernels {err_default:.3e}")
    assert b.shape == a.shape == (256 * 5168,) and d.shape == (256 * 5168,)
    assert err_direct == 0.0
    assert err_default <= O_HAT_TOL


def test_seeded_device_noise_reproduces_a_seeded_convert_batch(tcc, ses):
    g_src, g_tgt = ses
    wave = _wave(256 * 2100 + 100, 21)
    torch.manual_seed(1234)
    a = tcc.convert_batch(wave[None], g_src, g_tgt, tau=0.3)[0][0, 0].clone()
    torch.manual_seed(1234)
    b = tcc.convert_long(wave, g_src, g_tgt, tau=0.3, window_frames=1024, windows_per_launch=2)
    err = np.abs(a.cpu().numpy() - b).max()
    print("seeded convert_long vs seeded convert_batch:", err)
    assert err <= O_HAT_TOL
    torch.manual_seed(1235)
    c = tcc.convert_long(wave, g_src, g_tgt, tau=0.3, window_frames=1024, windows_per_launch=2)
    assert np.abs(c - b).max() > 1e-3               # another seed changes the posterior sample


@pytest.mark.parametrize("T,extra", [(300, 0), (512, 37), (513, 0), (513, 255), (1023, 100), (1537, 1)])
def test_edge_lengths_match_one_pass(tcc, ses, T, extra):
    """T < Tw (one window), T == Tw, Tw + 1, 2 Tw - 1, 3 Tw + 1, sample counts that are not multiples of hop."""
    model, (g_src, g_tgt) = tcc.model, ses
    n = 256 * T + extra
    assert longform.frames_of(n, NFFT, HOP) == T
    wave = _wave(n, T + extra)
    noise = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(T)).to(DEV)
    a = _one_pass(model, wave, g_src, g_tgt, 0.3, noise)
    b = _windowed(model, wave, g_src, g_tgt, 0.3, noise, 512, 4)
    err = (a - b).abs().max().item()
    print((T, extra), "windowed vs one pass:", err)
    assert b.shape == (256 * T,) and err <= O_HAT_TOL
    if T <= 512:
        assert err == 0.0                            # one window is the one-pass conversion


def test_windowed_conversion_matches_the_oracle(tcc, ses, synth_sd):
    from oracle import vc_oracle
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG
    g_src, g_tgt = ses
    T = 1200
    n = 256 * T + 11
    wave = _wave(n, 1200)
    noise = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(1200))
    b = _windowed(tcc.model, wave, g_src, g_tgt, 0.3, noise.to(DEV), 400, 4).cpu()
    torch.set_num_threads(usable_cpus(16))
    with torch.no_grad():
        spec = vc_oracle.spectrogram(wave.cpu()[None])
        o_ref = vc_oracle.voice_conversion(synth_sd, CONVERTER_MODEL_CONFIG, spec, torch.tensor([T]), g_src.cpu(),
                                           g_tgt.cpu(), 0.3, noise, zero_g=True)[0][0, 0]
    err = (b - o_ref).abs().max().item()
    print("windowed (400-frame windows) vs oracle, T = 1200:", err)
    assert err <= ORACLE_TOL


def test_graph_replay_composes_with_windows(tcc, ses):
    g_src, g_tgt = ses
    wave = _wave(256 * 1500 + 3, 15)
    noise = torch.randn(1, 192, 1500, generator=torch.Generator().manual_seed(15)).to(DEV)
    a = tcc.convert_long(wave, g_src, g_tgt, window_frames=512, windows_per_launch=2, noise=noise)
    try:
        tcc.enable_graphs(True)
        b = tcc.convert_long(wave, g_src, g_tgt, window_frames=512, windows_per_launch=2, noise=noise)
    finally:
        tcc.enable_graphs(False)
    assert np.array_equal(a, b)


# ---- the file one pass refuses ----------------------------------------------------------------------------------------
def test_convert_of_a_55_minute_file_returns_audio(tcc, ses, tmp_path):
    """55 min = 284 238 frames: beyond the one-pass launch limit (63 551 frames), where ``convert`` raised OvError
    before; it now converts through the windows.  At the start, middle and end, output frames [a, b) match a one-pass
    conversion of the frames [a - context, b + context) of the same spectrogram with the same noise."""
    from openvoice_amd import audio_io
    g_src, g_tgt = ses
    n = 55 * 60 * 22050
    T = longform.frames_of(n, NFFT, HOP)
    assert T >= longform.one_pass_limit_frames(tcc.model.model_cfg)
    audio_io.write(str(tmp_path / "long.wav"), _wave(n, 55, device="cpu").numpy(), 22050)
    torch.manual_seed(55)
    audio = tcc.convert(str(tmp_path / "long.wav"), g_src, g_tgt, tau=0.3)
    assert isinstance(audio, np.ndarray) and audio.shape == (256 * T,) and np.isfinite(audio).all()
    torch.manual_seed(55)
    noise = torch.randn(1, 192, T, device=DEV)           # the draw convert() made
    wave = audio_io.load_to_device(str(tmp_path / "long.wav"), 22050, DEV)
    spec = spectrogram_torch(wave[None], NFFT, 22050, HOP, NFFT, center=False)
    ctx = longform.context_frames(tcc.model.model_cfg)
    errs = []
    for a, b in [(0, 300), (T // 2 - 150, T // 2 + 150), (T - 300, T)]:
        lo, hi = max(0, a - ctx), min(T, b + ctx)
        o = tcc.model.voice_conversion(spec[:, :, lo:hi].contiguous(), torch.tensor([hi - lo], device=DEV), g_src, g_tgt,
                                       tau=0.3, noise=noise[:, :, lo:hi])[0][0, 0]
        ref = o[(a - lo) * 256:(b - lo) * 256].cpu().numpy()
        errs.append(float(np.abs(audio[a * 256:b * 256] - ref).max()))
    print("55 min file: start / middle / end vs one-pass excerpts:", errs)
    assert max(errs) <= O_HAT_TOL


def test_one_pass_limit_is_where_the_launchers_refuse(tcc, ses):
    """``one_pass_limit_frames`` (where ``convert`` hands over to the windows) is exactly where one pass starts to fail:
    T - 1 frames convert, T frames raise OvError (OV_E_BADARG, nothing launched past the refusal)."""
    g_src, g_tgt = ses
    model, eng = tcc.model, tcc.model.engine()
    T = longform.one_pass_limit_frames(model.model_cfg)
    spec = torch.rand(1, 513, T, generator=torch.Generator().manual_seed(3)).to(DEV)
    try:
        o = model.voice_conversion(spec[:, :, :T - 1], torch.tensor([T - 1], device=DEV), g_src, g_tgt, tau=0.0)[0]
        assert o.shape == (1, 1, 256 * (T - 1)) and torch.isfinite(o).all()
        del o
        with pytest.raises(_lib.OvError, match="OV_E_BADARG"):
            model.voice_conversion(spec, torch.tensor([T], device=DEV), g_src, g_tgt, tau=0.0)
        torch.cuda.synchronize()
    finally:
        eng._ws.clear()
        torch.cuda.empty_cache()


def test_peak_memory_is_flat_in_file_length(tcc, ses):
    g_src, g_tgt = ses
    eng = tcc.model.engine()
    peaks = {}
    for minutes in (10, 20):
        n = minutes * 60 * 22050
        wave = _wave(n, minutes)
        eng._ws.clear()                                  # no workspace of an earlier one-pass shape in the figure
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        tcc.convert_long(wave, g_src, g_tgt, tau=0.3)
        torch.cuda.synchronize()
        peaks[longform.frames_of(n, NFFT, HOP)] = torch.cuda.max_memory_allocated(DEV)
        del wave
    (t1, p1), (t2, p2) = sorted(peaks.items())
    per_frame = (p2 - p1) / (t2 - t1)
    print(f"peak allocation: {p1 / 2**30:.2f} GiB at {t1} frames, {p2 / 2**30:.2f} GiB at {t2} frames: "
          f"{per_frame:.0f} bytes per extra frame")
    assert per_frame <= 16 * 1024


# ---- streaming --------------------------------------------------------------------------------------------------------
def _push_all(stream, wave, sizes):
    """Push ``wave`` in blocks of the cycled ``sizes``; returns (the concatenated output, samples pushed before the push
    that returned the first output)."""
    outs, pos, before_first, i = [], 0, None, 0
    while pos < wave.numel():
        k = sizes[i % len(sizes)]
        i += 1
        o = stream.push(wave[pos:pos + k])
        if o.numel() and before_first is None:
            before_first = pos
        pos += min(k, wave.numel() - pos)
        outs.append(o)
    outs.append(stream.close())
    return torch.cat(outs), before_first


@pytest.mark.parametrize("on_host", [False, True])
def test_stream_concatenates_to_convert_long_with_one_window_per_launch(tcc, ses, on_host):
    g_src, g_tgt = ses
    T = 2100
    n = 256 * T + 99
    wave = _wave(n, 2100)
    noise = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(2100)).to(DEV)
    want = tcc.convert_long(wave, g_src, g_tgt, tau=0.3, window_frames=512, windows_per_launch=1, noise=noise)
    st = tcc.stream(g_src, g_tgt, tau=0.3, window_frames=512, noise=noise)
    src = wave.cpu() if on_host else wave
    got, before_first = _push_all(st, src, [1, 3, 44100, 1001, 7, 30000, 257])
    assert got.shape == (256 * T,) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert st.latency_samples == 511 * 256 + NFFT - PAD
    assert before_first is not None and before_first < st.latency_samples     # out with the push that reached it
    with pytest.raises(RuntimeError):
        st.push(wave[:10])


def test_stream_at_tau_0_matches_one_pass_convert(tcc, ses):
    g_src, g_tgt = ses
    n = 256 * 1800 + 5
    wave = _wave(n, 1800)
    a = _one_pass(tcc.model, wave, g_src, g_tgt, 0.0, None)
    st = tcc.stream(g_src, g_tgt, tau=0.0, window_frames=600)
    b, _ = _push_all(st, wave, [22050])
    err = (a - b).abs().max().item()
    print("stream (tau = 0) vs one-pass convert:", err)
    assert b.shape == a.shape and err <= O_HAT_TOL
    # the first output leaves exactly when latency_samples samples have arrived
    st = tcc.stream(g_src, g_tgt, tau=0.0, window_frames=600)
    assert st.latency_samples == 599 * 256 + NFFT - PAD
    assert st.push(wave[:st.latency_samples - 1]).numel() == 0
    first = st.push(wave[st.latency_samples - 1:st.latency_samples])
    assert first.numel() > 0 and torch.equal(first, b[:first.numel()])


def test_stream_close_on_input_shorter_than_one_frame_raises(tcc, ses):
    g_src, g_tgt = ses
    st = tcc.stream(g_src, g_tgt, window_frames=512)
    assert st.push(_wave(200, 1)).numel() == 0
    with pytest.raises(ValueError):
        st.close()
    with pytest.raises(ValueError):
        spectrogram_torch(_wave(200, 1)[None], NFFT, 22050, HOP, NFFT, center=False)
