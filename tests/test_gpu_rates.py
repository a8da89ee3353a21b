"""Rate conversion inside streams on the MI355X (openvoice_amd/rates.py): the record-driven resampler against the
whole-waveform kernel through both bindings, live and windowed streams at 8 - 48 kHz against the whole-file conversion
composed with the whole-file resampler, pools of mixed rates against solo streams, the defaults, the latency bound and
the whole-recording entry points."""
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, audio_io, longform, rates  # noqa: E402

DEV = "cuda:0"
SR = 22050
PAIRS = [(48000, 22050), (44100, 22050), (16000, 22050), (8000, 22050), (22050, 48000), (22050, 16000), (22050, 44100)]
LIVE_TOL = 3e-4           # 1e-4 (live vs convert_long, default kernels) x the largest sum |h| of a phase (~2.6)


@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("rates")
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


@pytest.fixture
def launches(monkeypatch):
    """Counts resampler launches (either entry point) issued through _lib.call."""
    log = []
    real = _lib.call

    def call(name, *args):
        if name in ("ov_polyphase_fir_rows_f32", "ov_polyphase_fir_f32"):
            log.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return log


def _ses(seed):
    gen = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


def _wave(n, seed, sr=SR):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / sr
    phase = 2 * np.pi * torch.cumsum(140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / sr
    y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float().to(DEV)


def _frames(n):
    return (n + 2 * 384 - 1024) // 256 + 1


def _noise(T, seed):
    return torch.randn(1, 192, T, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _to22(x, sr):
    return x if sr in (None, SR) else audio_io.resample_on_device(x, sr, SR)


def _from22(y, sr):
    y = torch.as_tensor(y).to(DEV)
    return y if sr in (None, SR) else audio_io.resample_on_device(y, SR, sr)


def _pushes(n, seed, lo=1, hi=9000):
    gen = np.random.default_rng(seed)
    out, acc = [], 0
    while acc < n:
        k = int(gen.integers(lo, hi))
        out.append(k)
        acc += k
    return out


def _run_stream(st, wave, pushes):
    outs, i = [], 0
    for n in pushes:
        outs.append(st.push(wave[i:i + n]))
        i += n
    outs.append(st.push(wave[i:]))
    outs.append(st.close())
    return torch.cat(outs)


# ---- ov_polyphase_fir_rows_f32 against ov_polyphase_fir_f32 ------------------------------------------------------------
@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_rows_kernel_split_into_arbitrary_records_equals_the_whole_file_kernel(binding, monkeypatch):
    """Every pair's output range cut into random records (some of one sample), each reading only its own window of an
    arena that packs the inputs, all in ONE launch that mixes the pairs; bit for bit against the whole-waveform kernel."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    rng = np.random.default_rng(11)
    xs = [_wave(20000 + 777 * i, 40 + i, a) for i, (a, b) in enumerate(PAIRS)]
    refs = [audio_io.resample_on_device(x, a, b) for x, (a, b) in zip(xs, PAIRS)]
    tables, offs, acc = [], {}, 0
    for a, b in PAIRS:
        h = audio_io.device_phases(a, b, DEV)[0].reshape(-1)
        offs[(a, b)] = acc
        tables.append(h)
        acc += h.numel()
    h_all = torch.cat(tables)
    pieces, recs, src_acc, dst_acc, spans = [], [], 0, 0, []
    for x, (a, b), ref in zip(xs, PAIRS, refs):
        P, Q, taps = rates.pair(a, b)
        n, n_fix = x.numel(), ref.numel()
        t = 0
        spans.append(dst_acc)
        while t < n_fix:
            k = min(n_fix - t, int(rng.choice([1, 2, 37, 500, 4000])))
            lo = max(0, (t * Q) // P - taps + 1)
            hi = min(n, ((t + k - 1) * Q) // P + taps + 1)
            hi = max(hi, lo)
            pieces.append(x[lo:hi])                      # this record's own window, packed
            recs.append((src_acc, lo, hi, n, t, k, dst_acc, offs[(a, b)], P, Q, taps))
            src_acc += hi - lo
            dst_acc += k
            t += k
    arena = torch.cat(pieces)
    out = torch.full((dst_acc,), float("nan"), device=DEV)
    table = torch.tensor(recs, dtype=torch.int64).to(DEV)
    assert len(recs) <= 65535
    _lib.call("ov_polyphase_fir_rows_f32", table, len(recs), arena, arena.numel(), h_all, h_all.numel(), out, out.numel(),
              max(r[5] for r in recs))
    torch.cuda.synchronize()
    for d0, ref in zip(spans, refs):
        assert torch.equal(out[d0:d0 + ref.numel()], ref)


def test_rows_kernel_checks_every_record_on_the_device():
    x = _wave(5000, 3, 48000)
    h = audio_io.device_phases(48000, 22050, DEV)[0].reshape(-1)
    P, Q, taps = rates.pair(48000, 22050)
    ref = audio_io.resample_on_device(x, 48000, 22050)
    out = torch.full((3000,), -7.0, device=DEV)
    recs = [(0, 0, 5000, 5000, 0, 1000, 0, 0, P, Q, taps),             # good
            (0, 0, 5000, 5000, 1000, 100, 2950, 0, P, Q, taps),         # destination past the end: nothing
            (0, 0, 5000, 5000, 1000, 100, 1000, 1, P, Q, taps),         # phase table past the end: nothing
            (0, 4000, 5000, 5000, 1500, 100, 1200, 0, P, Q, taps),      # reads before the valid window: zeros
            (0, 0, 2000, -1, 1000, 100, 1400, 0, P, Q, taps),           # reads past an unfinished window: zeros
            (0, 0, 5000, 5000, 0, 100, 1600, 0, -1, Q, taps)]           # bad P: nothing
    table = torch.tensor(recs, dtype=torch.int64).to(DEV)
    _lib.call("ov_polyphase_fir_rows_f32", table, len(recs), x, x.numel(), h, h.numel(), out, out.numel(), 1000)
    torch.cuda.synchronize()
    want = torch.full((3000,), -7.0, device=DEV)
    want[:1000] = ref[:1000]
    want[1200:1300] = 0.0
    want[1400:1500] = 0.0
    assert torch.equal(out, want)
    for args in [(table, 0), (table, 65536)]:
        with pytest.raises(_lib.OvError):
            _lib.call("ov_polyphase_fir_rows_f32", *args, x, x.numel(), h, h.numel(), out, out.numel(), 1000)
    with pytest.raises(_lib.OvError):
        _lib.call("ov_polyphase_fir_rows_f32", table, 1, x, x.numel(), h, h.numel(), out, out.numel(), 0)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_bank_streams_of_mixed_pairs_equal_the_whole_file_kernel(binding, monkeypatch, launches):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    xs = [_wave(30000 + 1234 * i, 60 + i, a) for i, (a, b) in enumerate(PAIRS * 2)]
    refs = [audio_io.resample_on_device(x, a, b) for x, (a, b) in zip(xs, PAIRS * 2)]
    launches.clear()
    bank = rates.ResamplerBank(DEV)
    keys = [bank.open(a, b) for a, b in PAIRS * 2]
    pushes = [_pushes(x.numel(), i, 1, 5000) for i, x in enumerate(xs)]
    pos, outs, steps = [0] * len(xs), [[] for _ in xs], 0
    while len(bank):
        for i, k in enumerate(keys):
            if k in bank and pos[i] <= xs[i].numel():
                n = pushes[i][steps] if steps < len(pushes[i]) else 0
                bank.push(k, xs[i][pos[i]:pos[i] + n].clone())
                pos[i] += n
                if pos[i] >= xs[i].numel():
                    bank.end(k)
                    pos[i] = xs[i].numel() + 1
        res = bank.step()
        for i, k in enumerate(keys):
            if k in res:
                outs[i].append(res[k])
        steps += 1
    assert len(launches) <= steps
    for o, ref in zip(outs, refs):
        got = torch.cat(o)
        assert got.shape == ref.shape and torch.equal(got, ref)


# ---- streams against the composed whole file --------------------------------------------------------------------------
def _composed(tcc, x, sr_in, sr_out, noise, **kw):
    x22 = _to22(x, sr_in)
    return _from22(tcc.convert_long(x22, *kw.pop("ses"), noise=noise, **kw), sr_out)


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 48000), (16000, 44100), (8000, 22050), (22050, 16000)])
def test_live_stream_equals_the_composed_whole_file_bitwise_with_direct_kernels(tcc, direct, sr_in, sr_out):
    ses = _ses(1)
    n = (sr_in * 256 * 400) // SR + 77
    x = _wave(n, 5, sr_in)
    noise = _noise(_frames(_to22(x, sr_in).numel()), 7)
    ref = _composed(tcc, x, sr_in, sr_out, noise, ses=ses)
    st = tcc.live_stream(*ses, chunk_frames=15, noise=noise, sr_in=sr_in, sr_out=sr_out)
    out = _run_stream(st, x, _pushes(n, sr_in + sr_out, 1, 7000))
    assert out.shape == ref.shape
    assert torch.equal(out, ref), (out - ref).abs().max().item()


def test_live_stream_matches_the_composed_whole_file_with_default_kernels(tcc):
    ses = _ses(2)
    n = 48000 * 6 + 11
    x = _wave(n, 8, 48000)
    noise = _noise(_frames(_to22(x, 48000).numel()), 9)
    ref = _composed(tcc, x, 48000, 48000, noise, ses=ses)
    st = tcc.live_stream(*ses, chunk_frames=15, noise=noise, sr_in=48000, sr_out=48000)
    out = _run_stream(st, x, [4800] * (n // 4800))
    assert out.shape == ref.shape
    assert (out - ref).abs().max().item() <= LIVE_TOL


def test_windowed_stream_equals_the_composed_whole_file_bitwise(tcc, direct):
    ses = _ses(3)
    n = 48000 * 9 + 5
    x = _wave(n, 10, 48000)
    noise = _noise(_frames(_to22(x, 48000).numel()), 11)
    ref = _composed(tcc, x, 48000, 48000, noise, ses=ses, window_frames=300, windows_per_launch=1)
    st = tcc.stream(*ses, window_frames=300, noise=noise, sr_in=48000, sr_out=48000)
    out = _run_stream(st, x, _pushes(n, 12, 1, 20000))
    assert out.shape == ref.shape and torch.equal(out, ref)


def test_output_does_not_depend_on_the_push_pattern(tcc):
    ses = _ses(4)
    n = 44100 * 4 + 3
    x = _wave(n, 13, 44100)
    noise = _noise(_frames(_to22(x, 44100).numel()), 14)
    outs = []
    for pushes in ([n], [1, 2, 3, 500, 4096] + [4410] * 30, _pushes(n, 15, 1, 30000)):
        st = tcc.live_stream(*ses, chunk_frames=15, noise=noise, sr_in=44100, sr_out=16000)
        outs.append(_run_stream(st, x, pushes))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ---- pools of mixed rates ----------------------------------------------------------------------------------------------
POOL_RATES = [(8000, 8000), (16000, 44100), (44100, 16000), (48000, 48000), (22050, 22050), (None, 48000)]


def _pool_run(pool, xs, ses, noises, launches):
    hs = [pool.open(*ses[i], noise=noises[i], sr_in=a, sr_out=b) for i, (a, b) in enumerate(POOL_RATES)]
    pos, outs = [0] * len(xs), [[] for _ in xs]
    while pool.active:
        for i, h in enumerate(hs):
            if pos[i] < xs[i].numel():
                k = 2205 * (1 + i % 3) + 37 * i
                pool.push(h, xs[i][pos[i]:pos[i] + k])
                pos[i] += k
                if pos[i] >= xs[i].numel():
                    pool.close(h)
        before = len(launches)
        for h, o in pool.step().items():
            outs[hs.index(h)].append(o.clone())
        assert len(launches) - before <= 2, "more than one resampler launch per direction in a step"
    return [torch.cat(o) for o in outs]


def _mixed_inputs():
    xs = [_wave(((a or SR) * 256 * (90 + 20 * i)) // SR + 3 * i, 70 + i, a or SR) for i, (a, _) in enumerate(POOL_RATES)]
    noises = [_noise(_frames(_to22(x, a).numel()), 80 + i) for i, (x, (a, _)) in enumerate(zip(xs, POOL_RATES))]
    return xs, [_ses(90 + i) for i in range(len(xs))], noises


def test_live_pool_of_mixed_rates_equals_solo_streams_bitwise(tcc, direct, launches):
    xs, ses, noises = _mixed_inputs()
    got = _pool_run(tcc.live_pool(chunk_frames=15, max_streams_per_launch=4), xs, ses, noises, launches)
    for i, (a, b) in enumerate(POOL_RATES):
        st = tcc.live_stream(*ses[i], chunk_frames=15, noise=noises[i], sr_in=a, sr_out=b)
        solo = _run_stream(st, xs[i], [2205 * (1 + i % 3) + 37 * i] * (xs[i].numel() // (2205 * (1 + i % 3) + 37 * i)))
        assert got[i].shape == solo.shape and torch.equal(got[i], solo), (a, b)


def test_stream_pool_of_mixed_rates_equals_solo_streams_bitwise(tcc, direct, launches):
    xs, ses, noises = _mixed_inputs()
    got = _pool_run(tcc.stream_pool(window_frames=300, max_windows_per_launch=4), xs, ses, noises, launches)
    for i, (a, b) in enumerate(POOL_RATES):
        st = tcc.stream(*ses[i], window_frames=300, noise=noises[i], sr_in=a, sr_out=b)
        solo = _run_stream(st, xs[i], [3000 + 11 * i] * (xs[i].numel() // (3000 + 11 * i)))
        assert got[i].shape == solo.shape and torch.equal(got[i], solo), (a, b)


# ---- defaults --------------------------------------------------------------------------------------------------------
def test_model_rate_and_no_rate_give_todays_output_without_a_resampler_launch(tcc, launches):
    ses = _ses(5)
    n = 256 * 200 + 9
    x = _wave(n, 16)
    noise = _noise(_frames(n), 17)
    launches.clear()
    live = [_run_stream(tcc.live_stream(*ses, noise=noise, **kw), x, [2205] * 20)
            for kw in ({}, dict(sr_in=None, sr_out=None), dict(sr_in=SR, sr_out=SR))]
    win = [_run_stream(tcc.stream(*ses, window_frames=300, noise=noise, **kw), x, [2205] * 20)
           for kw in ({}, dict(sr_in=None, sr_out=None), dict(sr_in=SR, sr_out=SR))]
    st = tcc.live_stream(*ses, sr_in=SR, sr_out=SR)
    assert st.latency_samples == tcc.live_stream(*ses).latency_samples == 32060
    assert launches == []
    assert torch.equal(live[0], live[1]) and torch.equal(live[0], live[2])
    assert torch.equal(win[0], win[1]) and torch.equal(win[0], win[2])


# ---- latency -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 16000])
def test_latency_bound_holds_on_the_device(tcc, sr):
    ses = _ses(6)
    n = sr * 5
    x = _wave(n, 18, sr)
    st = tcc.live_stream(*ses, chunk_frames=15, noise=_noise(_frames(_to22(x, sr).numel()), 19), sr_in=sr, sr_out=sr)
    lat = st.latency_seconds
    assert st.latency_samples == -(-lat * sr // 1)
    assert lat == Fraction(rates.pair(sr, SR)[2], sr) + Fraction(32060 + rates.pair(SR, sr)[2], SR)
    emitted, step = 0, 1000
    for i in range(0, n, step):
        emitted += st.push(x[i:i + step]).numel()
        arrived = min(n, i + step)
        due = Fraction(arrived - 1, sr) - lat          # every output at or before this instant has left
        if due >= 0:
            assert emitted >= int(due * sr) + 1, (arrived, emitted)


# ---- whole recordings ---------------------------------------------------------------------------------------------------
def test_convert_long_and_convert_many_at_other_rates_equal_the_composition(tcc, direct, launches, tmp_path):
    ses = _ses(7)
    kw = dict(tau=0.3, window_frames=512)
    x48 = _wave(48000 * 8 + 1, 20, 48000)
    noise = _noise(_frames(_to22(x48, 48000).numel()), 21)
    got = tcc.convert_long(x48, *ses, noise=noise, sr=48000, out_sr=16000, **kw)
    want = _composed(tcc, x48, 48000, 16000, noise, ses=ses, **kw)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want.cpu().numpy())
    items = [_wave(8000 * 5 + 7, 22, 8000), x48.cpu(), _wave(SR * 4, 23), _wave(44100 * 6, 24, 44100)]
    srs = [8000, 48000, None, 44100]
    out_srs = [48000, 16000, None, 22050]
    noises = [_noise(_frames(_to22(torch.as_tensor(x).to(DEV), a).numel()), 30 + i) for i, (x, a) in
              enumerate(zip(items, srs))]
    launches.clear()
    many = tcc.convert_many(items, ses[0], ses[1], noise=noises, sr=srs, out_sr=out_srs, windows_per_launch=4, **kw)
    assert launches == ["ov_polyphase_fir_rows_f32"] * 2             # one launch per direction for all items
    for i, (x, a, b) in enumerate(zip(items, srs, out_srs)):
        want = _composed(tcc, torch.as_tensor(x).to(DEV), a, b, noises[i], ses=ses, **kw).cpu().numpy()
        assert many[i].shape == want.shape and np.array_equal(many[i], want), i
    paths = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    assert tcc.convert_many(items[:2], ses[0], ses[1], noise=noises[:2], sr=srs[:2], out_sr=16000, output_paths=paths,
                            **kw) is None
    for p, x, a in zip(paths, items, srs):
        y, rate = audio_io.load(p, None)
        assert rate == 16000
        T = _frames(_to22(torch.as_tensor(x).to(DEV), a).numel())
        assert y.size == -(-T * 256 * 16000 // SR)
