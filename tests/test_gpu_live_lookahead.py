"""Live streams with bounded look-ahead on the MI355X (``lookahead_frames=``, openvoice_amd/live.py): every emitted piece
against the one-pass conversion of the frames received so far, the bf16 generator, exactness past the reach, pools
against solo streams, push patterns, the latency bound, ``ov_crossfade_rows_f32`` alone and in the stream, ``sr_out``."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, audio_io, live, rates  # noqa: E402
from openvoice_amd.mel_processing import spectrogram_torch  # noqa: E402

DEV = "cuda:0"
O_HAT_TOL = 1e-4
HOP, NFFT, SEED = 256, 1024, 1234


@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("live_ahead")
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


def _pushes(n, seed, lo=100, hi=9000):
    gen = np.random.default_rng(seed)
    out, acc = [], 0
    while acc < n:
        k = int(gen.integers(lo, hi))
        out.append(k)
        acc += k
    return out


def _run_stream(st, wave, pushes):
    """-> (what every push returned, what close returned)."""
    outs, i = [], 0
    for n in list(pushes) + [wave.numel()]:
        outs.append(st.push(wave[i:i + n]))
        i += n
    return outs, st.close()


class _OnePass:
    """One-pass conversions of the first F frames of a wave's spectrogram, one per F, made once and shared."""

    def __init__(self, tcc, wave, ses, generator=None):
        self.tcc, self.ses, self.generator, self.cache = tcc, ses, generator, {}
        self.spec = spectrogram_torch(wave[None], NFFT, 22050, HOP, NFFT, center=False)
        self.T = self.spec.shape[2]

    def __call__(self, F):
        if F not in self.cache:
            o = self.tcc.model.voice_conversion(self.spec[:, :, :F].contiguous(), torch.tensor([F], device=DEV), *self.ses,
                                                tau=0.3, seed=SEED, generator=self.generator)[0]
            self.cache[F] = o[0, 0].clone()
        return self.cache[F]


def _check_pieces(ref, wave, outs, rest, chunk, A, tol):
    """Every round's piece [E_{n-1}, E_n) against the one-pass conversion of the first F_n = n x chunk frames, and the
    rest against the whole file's."""
    got, E, F, pos = torch.cat(outs), 0, 0, 0
    while True:
        F += chunk
        En = HOP * max(0, F - A)
        if pos + En - E > got.numel() or F > ref.T:
            break
        if En > E:
            piece, want = got[pos:pos + En - E], ref(F)[E:En]
            if tol == 0:
                assert torch.equal(piece, want), (A, chunk, F, (piece - want).abs().max().item())
            else:
                assert (piece - want).abs().max().item() <= tol, (A, chunk, F)
            pos, E = pos + En - E, En
    assert pos == got.numel(), "pushes returned samples that belong to no round"
    rounds = live.interior_frames(wave.numel(), NFFT, HOP) // chunk
    assert E == HOP * max(0, rounds * chunk - A)
    want = ref(ref.T)[E:]
    assert rest.shape == want.shape
    assert torch.equal(rest, want) if tol == 0 else (rest - want).abs().max().item() <= tol


CASES = [(300, 15, 0), (300, 15, 15), (300, 15, 45), (9, 15, 0), (9, 15, 15), (9, 15, 45), (300, 60, 0)]
_refs = {}


def _ref(tcc, frames, tag, generator=None):
    key = (frames, tag, generator, tcc.model.engine().use_winograd)
    if key not in _refs:
        wave = _wave(HOP * frames + 77, frames)
        _refs[key] = (wave, _OnePass(tcc, wave, _ses(1), generator))
    return _refs[key]


@pytest.mark.parametrize("frames,chunk,A", CASES)
def test_pieces_equal_the_one_pass_conversion_of_the_frames_so_far_bitwise(tcc, direct, frames, chunk, A):
    wave, ref = _ref(tcc, frames, "direct")
    st = tcc.live_stream(*_ses(1), chunk_frames=chunk, seed=SEED, lookahead_frames=A, crossfade_samples=0)
    outs, rest = _run_stream(st, wave, _pushes(wave.numel(), frames + A))
    _check_pieces(ref, wave, outs, rest, chunk, A, 0)


@pytest.mark.parametrize("frames,chunk,A", CASES)
def test_pieces_match_the_one_pass_conversion_with_default_kernels(tcc, frames, chunk, A):
    wave, ref = _ref(tcc, frames, "default")
    st = tcc.live_stream(*_ses(1), chunk_frames=chunk, seed=SEED, lookahead_frames=A, crossfade_samples=0)
    outs, rest = _run_stream(st, wave, _pushes(wave.numel(), frames + A))
    _check_pieces(ref, wave, outs, rest, chunk, A, O_HAT_TOL)


@pytest.mark.parametrize("frames,chunk,A", CASES)
def test_bf16_generator_pieces_equal_the_one_pass_bf16_conversion(tcc, frames, chunk, A):
    wave, ref = _ref(tcc, frames, "default", "bf16")
    st = tcc.live_stream(*_ses(1), chunk_frames=chunk, seed=SEED, generator="bf16", lookahead_frames=A,
                         crossfade_samples=0)
    outs, rest = _run_stream(st, wave, _pushes(wave.numel(), frames + A + 3))
    _check_pieces(ref, wave, outs, rest, chunk, A, 0)


def test_past_the_reach_the_stream_is_the_plain_stream_and_previews_nothing(tcc):
    wave = _wave(HOP * 300 + 77, 2)
    eng = tcc.model.engine()
    outs, rest = _run_stream(tcc.live_stream(*_ses(2), seed=SEED), wave, [2205] * 30)
    plain = torch.cat(outs + [rest])
    before, builds = set(eng._live_ws), eng.live_ws_builds      # the plain stream's workspaces (and earlier tests')
    st = tcc.live_stream(*_ses(2), seed=SEED, lookahead_frames=110)
    outs, rest = _run_stream(st, wave, [2205] * 30)
    assert torch.equal(torch.cat(outs + [rest]), plain)
    assert set(eng._live_ws) == before and eng.live_ws_builds == builds, "a preview workspace was built"
    assert st._pool._pv is None and st._pool._fade is None
    assert st.latency_samples == HOP * 125 + 384


def _pool_run(tcc, lengths, taus, opens, waves):
    pool = tcc.live_pool(chunk_frames=15, max_streams_per_launch=2, lookahead_frames=15, crossfade_samples=0)
    handles, pos, outs = {}, [0] * len(lengths), {i: [] for i in range(len(lengths))}
    tick = 0
    while True:
        for i, t in enumerate(opens):
            if t == tick:
                handles[i] = pool.open(*_ses(10 + i), seed=(SEED, i), tau=taus[i])
        for i, h in list(handles.items()):
            if pos[i] < lengths[i]:
                k = 2205 + 37 * i
                pool.push(h, waves[i][pos[i]:pos[i] + k])
                pos[i] += k
                if pos[i] >= lengths[i]:
                    pool.close(h)
        res = pool.step()
        for i, h in handles.items():
            if h in res:
                outs[i].append(res[h])
        tick += 1
        if all(p >= n for p, n in zip(pos, lengths)) and not pool.active:
            return [torch.cat(outs[i]) for i in range(len(lengths))]


def test_pool_streams_equal_their_solo_streams_bitwise(tcc, direct):
    lengths, taus, opens = [HOP * 150 + 5, HOP * 60, HOP * 8 + 200, HOP * 200 + 99], [0.3, 0.1, 0.5, 0.3], [0, 0, 3, 5]
    waves = [_wave(n, 20 + i) for i, n in enumerate(lengths)]
    got = _pool_run(tcc, lengths, taus, opens, waves)
    builds = tcc.model.engine().live_ws_builds
    again = _pool_run(tcc, lengths, taus, opens, waves)
    assert tcc.model.engine().live_ws_builds == builds, "a second run built a workspace"
    for i, n in enumerate(lengths):
        st = tcc.live_stream(*_ses(10 + i), tau=taus[i], seed=(SEED, i), lookahead_frames=15, crossfade_samples=0)
        k = 2205 + 37 * i
        outs, rest = _run_stream(st, waves[i], [k] * (n // k))
        solo = torch.cat(outs + [rest])
        assert got[i].shape == solo.shape == (HOP * ((n + 768 - NFFT) // HOP + 1),)
        assert torch.equal(got[i], solo) and torch.equal(again[i], solo), i


def test_output_does_not_depend_on_the_push_pattern(tcc):
    src, tgt = _ses(3)
    n = 256 * 400 + 31
    wave = _wave(n, 5)
    outs = []
    for pushes in ([n], [1, 2, 3, 500, 4096] + [2205] * 40, _pushes(n, 9, 1, 30000)):
        st = tcc.live_stream(src, tgt, chunk_frames=15, seed=SEED, lookahead_frames=15)
        o, rest = _run_stream(st, wave, pushes)
        outs.append(torch.cat(o + [rest]))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("A", [0, 15])
def test_latency_bound_holds_on_the_device(tcc, A):
    src, tgt = _ses(4)
    n = 256 * 300
    wave = _wave(n, 6)
    st = tcc.live_stream(src, tgt, chunk_frames=15, seed=SEED, lookahead_frames=A)
    assert st.latency_samples == live.live_latency_samples(tcc.model.model_cfg, 15, lookahead_frames=A)
    emitted = 0
    for i in range(0, n, 1000):
        emitted += st.push(wave[i:i + 1000]).numel()
        arrived = min(n, i + 1000)
        assert emitted >= arrived - st.latency_samples + 1
    if A == 0:
        assert 4 * st.latency_samples < live.live_latency_samples(tcc.model.model_cfg, 15)
        assert st.latency_seconds <= 0.2


# ---- ov_crossfade_rows_f32 alone ----------------------------------------------------------------------------------------
def _fade64(w, old, new):
    w, old, new = w.double(), old.double(), new.double()
    return old + w * (new - old)


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_crossfade_rows_against_the_float64_blend(binding, monkeypatch):
    """|out - exact| <= 2^-23 (|old| + |new|): the difference new - old is rounded once (error <= 2^-24 |new - old|, and
    |w| <= 1), the fused multiply-add once more (<= 2^-24 |out|, |out| <= max(|old|, |new|) for 0 <= w <= 1)."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    gen = torch.Generator().manual_seed(11)
    S, D = 200_000, 60_000
    src = torch.randn(S, generator=gen)
    w = live.crossfade_weights(256)
    recs, expect, o, d = [], [], 0, 8
    for x in (0, 1, 255, 256):
        for n in (1, 3, 257, 4099):
            for mis in ((0, 0, 0), (1, 2, 3)) if n == 257 else ((0, 0, 0),) if x != 255 else ((3, 0, 1),):
                oo, no, do = o + mis[0], o + 4400 + mis[1], d + mis[2]
                recs.append((oo, no, do, n, x))
                expect.append((do, n, min(x, n), oo, no))
                o, d = o + 2 * 4400 + 8, d + (n + 3) // 4 * 4 + 16
    assert o < S and d < D
    bad = (0, 4, D - 2, 4, 2)                     # destination leaves the buffer: nothing is written
    recs.append(bad)
    recs.append((S - 1, 0, d, 4, 2))              # old span leaves the source: nothing is written
    recs.append((0, 0, d, 4, 257))                # x past the weights: nothing is written
    dst = torch.full((D,), -7.0)
    ref = dst.clone().double()
    bound = torch.zeros(D, dtype=torch.float64)
    exact = torch.zeros(D, dtype=torch.bool)
    for do, n, xb, oo, no in expect:
        ref[do:do + n] = src[no:no + n].double()
        ref[do:do + xb] = _fade64(w[:xb], src[oo:oo + xb], src[no:no + xb])
        bound[do:do + xb] = 2.0 ** -23 * (src[oo:oo + xb].abs().double() + src[no:no + xb].abs().double())
        exact[do + xb:do + n] = True
    out = dst.to(DEV)
    _lib.call("ov_crossfade_rows_f32", torch.tensor(recs, dtype=torch.int64).to(DEV), len(recs), w.to(DEV), w.numel(),
              src.to(DEV), S, out, D)
    torch.cuda.synchronize()
    out = out.cpu()
    touched = bound > 0
    assert ((out.double() - ref).abs() <= bound)[touched].all()
    assert torch.equal(out[exact], ref[exact].float())                     # samples past x: the bits of ``new``
    rest = ~(touched | exact)
    assert (out[rest] == -7.0).all(), "a sentinel around a destination or an out-of-range record was written"
    assert rest.sum() >= 16 * len(expect)


def test_crossfade_rows_rejects_bad_host_arguments():
    t = torch.zeros(4, 5, dtype=torch.int64, device=DEV)
    x = torch.zeros(64, device=DEV)
    for args in [(t, 0, x, 64, x, 64, x, 64), (t, 65536, x, 64, x, 64, x, 64), (t, 1, x, 0, x, 64, x, 64),
                 (t, 1, x, 64, x, 0, x, 64), (t, 1, x, 64, x, 64, x, 0), (t, 1, None, 64, x, 64, x, 64)]:
        with pytest.raises(_lib.OvError):
            _lib.call("ov_crossfade_rows_f32", *args)


# ---- the seam in the stream ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [15, 100])
def test_crossfade_in_the_stream_is_the_float64_blend_of_the_unblended_pieces(tcc, direct, A):
    """X = 256.  A piece that begins past the committed samples while the previous round previewed is the X = 0 piece
    with its first 256 samples blended with ``old`` = the 256 samples after piece n - 1 in the one-pass conversion of
    F_{n-1} frames (what that round's preview held), the rest of it bit for bit; so is the rest at close.  A piece that
    begins inside committed samples is the X = 0 piece bit for bit: at A = 15 no piece does, at A = 100 every piece of
    a regular round does (E_{n-1} = hop (F_n - 115) < C_n = hop F_n - 27 836) although each round before it previewed."""
    wave, ref = _ref(tcc, 300, "direct")
    X, chunk, R = 256, 15, live.live_right_samples(tcc.model.model_cfg)
    st = tcc.live_stream(*_ses(1), chunk_frames=chunk, seed=SEED, lookahead_frames=A, crossfade_samples=X)
    outs, rest = _run_stream(st, wave, [2205] * 34)
    got = torch.cat(outs + [rest]).cpu()
    w = live.crossfade_weights(X)
    rounds = live.interior_frames(wave.numel(), NFFT, HOP) // chunk
    assert got.numel() == HOP * ref.T
    E0, tail_F, blended, exact = 0, None, 0, 0
    for r in range(1, rounds + 2):
        last = r > rounds
        F = ref.T if last else r * chunk
        E1 = HOP * ref.T if last else HOP * max(0, F - A)
        C = HOP * ref.T if last else max(0, HOP * F - R)
        if E1 <= E0:
            continue
        new, piece = ref(F)[E0:E1].cpu(), got[E0:E1]
        if tail_F is not None and (last or E0 >= C):
            old = ref(tail_F)[E0:E0 + X].cpu()
            want = _fade64(w, old, new[:X])
            bound = 2.0 ** -23 * (old.abs().double() + new[:X].abs().double())
            assert ((piece[:X].double() - want).abs() <= bound).all(), (E0, F)
            assert not torch.equal(piece[:X], new[:X])
            assert torch.equal(piece[X:], new[X:]), (E0, F)
            blended += 1
        else:
            assert torch.equal(piece, new), (E0, F)
            exact += 1
        tail_F = F if E1 > max(C, E0) else None        # this round previewed: its tail is kept
        E0 = E1
    assert (blended, exact) == ((rounds - 1, 1) if A == 15 else (1, rounds - 6))


def test_sr_out_resamples_the_emitted_sequence(tcc, direct):
    """48 kHz in, 16 kHz out, A = 15: the output is the model-rate emitted sequence (the stream with the same input at the
    model rate and no output rate) through the ``rates`` resampler in one go."""
    n = 48000 * 3 + 11
    wave48 = _wave(n, 8)
    kw = dict(chunk_frames=15, seed=SEED, lookahead_frames=15)
    outs, rest = _run_stream(tcc.live_stream(*_ses(5), sr_in=48000, **kw), wave48, [4800] * 29)
    model_rate = torch.cat(outs + [rest])
    outs, rest = _run_stream(tcc.live_stream(*_ses(5), sr_in=48000, sr_out=16000, **kw), wave48, [4800] * 29)
    got = torch.cat(outs + [rest])
    want = audio_io.resample_on_device(model_rate, rates.MODEL_RATE, 16000)
    assert got.shape == want.shape and torch.equal(got, want)


def test_bad_arguments_raise(tcc):
    src, tgt = _ses(0)
    for kw in (dict(lookahead_frames=-1), dict(lookahead_frames=1.5), dict(lookahead_frames=True),
               dict(lookahead_frames=0, crossfade_samples=1), dict(crossfade_samples=4),
               dict(lookahead_frames=45, crossfade_samples=15 * HOP + 1)):
        with pytest.raises(ValueError):
            tcc.live_stream(src, tgt, **kw)
        with pytest.raises(ValueError):
            tcc.live_pool(**kw)
