"""Live streams on the bf16 generator on the MI355X (``live_stream`` / ``live_pool`` with ``generator="bf16"``): the two
layout hand-over kernels against torch through both bindings, ``GeneratorBf16.decode`` against its own stages chained
by hand, a live bf16 stream against the one-pass bf16 conversion, push-pattern independence, a pool against solo
streams, fp32 and bf16 pools side by side, and a stream at rates of its own."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, audio_io  # noqa: E402

DEV = "cuda:0"
# the bf16 generator's stated waveform tolerance against fp32 (tests/test_gpu_bf16.py:
# test_generator_bf16_against_fp32_oracle, test_voice_conversion_with_the_opt_in_bf16_generator: max-abs 3e-2)
BF16_O_HAT_TOL = 3e-2


@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("live_bf16")
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


@pytest.fixture(scope="module", autouse=True)
def fp32_before_bf16(tcc):
    """The fp32 live conversion of ``_side_inputs``, made when the module starts: before this converter has opened a
    bf16 pool or built its bf16 generator."""
    assert tcc.model.engine().generator_bf16 is None
    return _run_pools(tcc, [tcc.live_pool(chunk_frames=15, max_streams_per_launch=2)])[0]


def _bf16_on(tcc):
    """The engine-wide switch (``use_bf16_generator``); an engine that never saw it has no such attribute."""
    return getattr(tcc.model.engine(), "_bf16_on", False)


def _ses(seed):
    gen = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


def _wave(n, seed, sr=22050):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / sr
    phase = 2 * np.pi * torch.cumsum(140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / sr
    y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float().to(DEV)


def _noise(T, seed):
    return torch.randn(1, 192, T, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _frames(n):
    return (n + 2 * 384 - 1024) // 256 + 1


def _run_stream(st, wave, pushes):
    outs, i = [], 0
    for n in pushes:
        outs.append(st.push(wave[i:i + n]))
        i += n
    outs.append(st.push(wave[i:]))
    outs.append(st.close())
    return torch.cat(outs)


def _pushes(n, seed, lo=100, hi=9000):
    gen = np.random.default_rng(seed)
    out, acc = [], 0
    while acc < n:
        k = int(gen.integers(lo, hi))
        out.append(k)
        acc += k
    return out


# ---- ov_rows_f32_to_cl_bf16 / ov_cl_bf16_to_rows_f32 ------------------------------------------------------------------
SPECIAL_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # exact ties: to even, down and up, both signs
                0x3F808001, 0x3F807FFF,                              # one ulp past / short of a tie
                0x7F7FFFFF, 0x7F7F8000,                              # the largest float, a tie at the top: both -> inf
                0x00000001, 0x80000000,                              # a subnormal, -0
                0x7F800000, 0xFF800000, 0x7FC00001, 0xFF800001]      # +-inf, a quiet and a signalling NaN


def _special_values(rows, L):
    """Plant the special values in valid columns of ``rows`` [B, C, ld], spread over rows, channels and columns."""
    vals = torch.from_numpy(np.array(SPECIAL_BITS, dtype=np.uint32).view(np.float32).copy())
    B, C, _ = rows.shape
    for i in range(3 * len(SPECIAL_BITS)):
        rows[i % B, (7 * i + 3) % C, (5 * i) % L] = vals[i % len(SPECIAL_BITS)]


HANDOVER_CASES = [(C, L, ld, misalign) for C in (32, 192) for L, ld, misalign in
                  [(1, 4, 0), (7, 8, 0), (64, 64, 0), (65, 68, 0), (130, 132, 0), (130, 135, 0), (65, 68, 1), (7, 7, 0)]]


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_hand_over_kernels_match_torch_exactly(binding, monkeypatch):
    """B = 3; ld > L (a multiple of 4: the vector path with a scalar tail, and 135: the scalar path); a row stride larger
    than C * ld; the base offset by one element (scalar path on 16-byte-aligned strides)."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    B = 3
    gen = torch.Generator().manual_seed(17)
    for C, L, ld, misalign in HANDOVER_CASES:
        bs = C * ld + 8                                            # a gap of 8 floats between the rows
        x = torch.randn(B, bs, generator=gen) * 3.0
        _special_values(x[:, :C * ld].view(B, C, ld), L)
        store = torch.zeros(B * bs + misalign)
        store[misalign:] = x.view(-1)
        store = store.to(DEV)
        src = store[misalign:]
        rows = src.view(B, bs)[:, :C * ld].view(B, C, ld)
        want = rows[..., :L].transpose(1, 2).to(torch.bfloat16).contiguous()
        got = torch.full((B, L, C), -5.0, dtype=torch.bfloat16, device=DEV)
        _lib.call("ov_rows_f32_to_cl_bf16", src, bs, ld, got, B, C, L)
        torch.cuda.synchronize()
        nan = torch.isnan(want)
        assert nan.any() and torch.isinf(want).any()
        assert torch.equal(torch.isnan(got), nan), (C, L, ld, misalign)
        assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), (C, L, ld, misalign)
        # and back: exact widening; columns >= L, the gaps between the rows and everything before the base stay
        SENT = -7.0
        back = torch.full((B * bs + misalign,), SENT, device=DEV)
        _lib.call("ov_cl_bf16_to_rows_f32", want, back[misalign:], bs, ld, B, C, L)
        torch.cuda.synchronize()
        ref = torch.full((B, bs), SENT, device=DEV)
        ref[:, :C * ld].view(B, C, ld)[..., :L] = want.float().transpose(1, 2)
        out = back[misalign:].view(B, bs)
        assert torch.equal(torch.isnan(out), torch.isnan(ref)), (C, L, ld, misalign)
        assert torch.equal(torch.nan_to_num(out, nan=0.5), torch.nan_to_num(ref, nan=0.5)), (C, L, ld, misalign)
        assert (back[:misalign] == SENT).all()


def test_hand_over_kernels_reject_bad_arguments():
    x = torch.zeros(3 * 64 * 16, device=DEV)
    y = torch.zeros(3 * 16 * 64, dtype=torch.bfloat16, device=DEV)
    # (bs, ld, B, C, L): C = 40; L = 0; ld < L; B = 0; rows that overlap
    for bs, ld, B, C, L in [(40 * 16, 16, 3, 40, 8), (64 * 16, 16, 3, 64, 0), (64 * 16, 7, 3, 64, 8), (64 * 16, 16, 0, 64, 8),
                            (64 * 16 - 1, 16, 3, 64, 8)]:
        with pytest.raises(_lib.OvError):
            _lib.call("ov_rows_f32_to_cl_bf16", x, bs, ld, y, B, C, L)
        with pytest.raises(_lib.OvError):
            _lib.call("ov_cl_bf16_to_rows_f32", y, x, bs, ld, B, C, L)


# ---- GeneratorBf16.stage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse_pairs", [True, False])
def test_decode_equals_its_stages_chained_by_hand(synth_sd, fuse_pairs):
    from openvoice_amd.bf16 import GeneratorBf16
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG
    gen = torch.Generator().manual_seed(23)
    B, T = 2, 20
    z = torch.randn(B, 192, T, generator=gen).to(DEV)
    g = (0.3 * torch.randn(B, 256, 1, generator=gen)).to(DEV)
    dec = GeneratorBf16(synth_sd, CFG, DEV)
    dec.fuse_pairs = fuse_pairs
    ref = dec.decode(z, g).clone()
    bf = lambda n: torch.empty(n, dtype=torch.bfloat16, device=DEV)
    x = z.transpose(1, 2).to(torch.bfloat16).contiguous()
    cond = dec.cond_rows(g)
    ch, L = CFG["upsample_initial_channel"], T
    for i, s in enumerate(CFG["upsample_rates"]):
        n = dec.stage_scratch_elems(i, B, L)
        assert n == B * L * s * (ch // 2)
        last = i == len(CFG["upsample_rates"]) - 1
        out = torch.empty(B, 1, L * s, device=DEV) if last else bf(n).view(B, L * s, ch // 2)
        bufs = [bf(n) for _ in range(4 if last else 3)]
        dec.stage(i, x, out, B, L, cond=cond if i == 0 else None, bufs=bufs, pre=bf(B * L * ch) if i == 0 else None)
        x, ch, L = out, ch // 2, L * s
    torch.cuda.synchronize()
    assert x.shape == ref.shape and torch.isfinite(ref).all()
    assert torch.equal(x, ref)


# ---- a live bf16 stream is the bf16 conversion ------------------------------------------------------------------------
def _bf16_reference(tcc, wave, src, tgt, noise, **kw):
    eng = tcc.model.engine()
    eng.use_bf16_generator(True)
    try:
        return torch.as_tensor(tcc.convert_long(wave, src, tgt, noise=noise, **kw)).to(DEV)
    finally:
        eng.use_bf16_generator(False)


def _check_against_the_bf16_conversion(tcc, out, wave, src, tgt, noise, tag, **kw):
    """The condition of a live bf16 stream: it IS the one-pass bf16 conversion (the bf16 kernels are direct convolutions
    whose result for a column does not depend on where the column lies in the launch, and the fp32 arena between two
    stages holds bf16 values exactly), so ``torch.equal``; and it is within the bf16 generator's stated tolerance of
    the fp32 conversion.  Measured on the MI355X: max|live_bf16 - bf16_ref| = 0 in every case of this file."""
    ref16 = _bf16_reference(tcc, wave, src, tgt, noise, **kw)
    ref32 = torch.as_tensor(tcc.convert_long(wave, src, tgt, noise=noise, **kw)).to(DEV)
    assert out.shape == ref16.shape == ref32.shape
    d_live = (out - ref16).abs().max().item()
    d_prec = (ref16 - ref32).abs().max().item()
    d_fp32 = (out - ref32).abs().max().item()
    print(f"live bf16 {tag}: max|live - bf16_ref| {d_live:.3e}, max|bf16_ref - fp32_ref| {d_prec:.3e}, "
          f"max|live - fp32_ref| {d_fp32:.3e}")
    assert d_prec > 1e-5, "the reference did not run the bf16 generator"
    assert torch.equal(out, ref16), (tag, d_live, d_prec)
    assert d_fp32 <= BF16_O_HAT_TOL, (tag, d_fp32)


@pytest.mark.parametrize("chunk", [15, 60])
def test_live_bf16_stream_equals_the_bf16_conversion(tcc, chunk):
    src, tgt = _ses(2)
    for n in [256 * 9 + 100, 256 * 300 + 77]:       # start and end inside one round; steady state
        wave = _wave(n, n)
        noise = _noise(_frames(n), n)
        st = tcc.live_stream(src, tgt, chunk_frames=chunk, noise=noise, generator="bf16")
        out = _run_stream(st, wave, [2205] * (n // 2205))
        assert not _bf16_on(tcc)
        _check_against_the_bf16_conversion(tcc, out, wave, src, tgt, noise, f"n={n} chunk={chunk}")


def test_live_bf16_output_does_not_depend_on_the_push_pattern(tcc):
    src, tgt = _ses(3)
    n = 256 * 200 + 31
    wave, noise = _wave(n, 5), _noise(_frames(n), 5)
    outs = []
    for pushes in ([2205] * (n // 2205), _pushes(n, 9, 1, 30000)):
        st = tcc.live_stream(src, tgt, chunk_frames=15, noise=noise, generator="bf16")
        outs.append(_run_stream(st, wave, pushes))
    assert outs[0].numel() == (n // 256) * 256 and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def _step_pool(pool, handles, waves, pos, outs, k=2205):
    """One tick: push the next ``k`` samples of every open stream (closing it at its end), then ``step``."""
    for i, h in handles.items():
        if pos[i] < waves[i].numel():
            pool.push(h, waves[i][pos[i]:pos[i] + k])
            pos[i] += k
            if pos[i] >= waves[i].numel():
                pool.close(h)
    for h, o in pool.step().items():
        outs[next(i for i, hh in handles.items() if hh == h)].append(o.clone())


def test_live_bf16_pool_equals_solo_streams(tcc):
    lengths = [256 * 70 + 5, 256 * 8 + 200, 256 * 40 + 99]          # the second: shorter than one chunk of frames
    ses = [_ses(10 + i) for i in range(3)]
    waves = [_wave(n, 20 + i) for i, n in enumerate(lengths)]
    noises = [_noise(_frames(n), 30 + i) for i, n in enumerate(lengths)]
    pool = tcc.live_pool(chunk_frames=15, max_streams_per_launch=2, generator="bf16")
    handles = {i: pool.open(*ses[i], noise=noises[i]) for i in range(3)}
    pos, outs = [0] * 3, {i: [] for i in range(3)}
    while pool.active:
        _step_pool(pool, handles, waves, pos, outs)
    for i, n in enumerate(lengths):
        st = tcc.live_stream(*ses[i], chunk_frames=15, noise=noises[i], generator="bf16")
        solo = _run_stream(st, waves[i], [2205] * (n // 2205))
        got = torch.cat(outs[i])
        assert got.shape == solo.shape and got.numel() == (n // 256) * 256
        assert torch.equal(got, solo), (i, (got - solo).abs().max().item())


def _side_inputs():
    lengths = [256 * 60 + 5, 256 * 33 + 120]
    return ([_ses(40 + i) for i in range(2)], [_wave(n, 50 + i) for i, n in enumerate(lengths)],
            [_noise(_frames(n), 60 + i) for i, n in enumerate(lengths)])


def _run_pools(tcc, pools):
    """Every pool converts both ``_side_inputs``; the pools are stepped alternately, tick by tick."""
    ses, waves, noises = _side_inputs()
    state = []
    for pool in pools:
        handles = {i: pool.open(*ses[i], noise=noises[i]) for i in range(2)}
        state.append((pool, handles, [0, 0], {0: [], 1: []}))
    while any(pool.active for pool in pools):
        for pool, handles, pos, outs in state:
            if pool.active:
                _step_pool(pool, handles, waves, pos, outs)
            assert not _bf16_on(tcc)
    return [[torch.cat(outs[i]) for i in range(2)] for _, _, _, outs in state]


def test_fp32_and_bf16_pools_side_by_side(tcc, fp32_before_bf16):
    eng = tcc.model.engine()
    alone = fp32_before_bf16
    both = _run_pools(tcc, [tcc.live_pool(chunk_frames=15, max_streams_per_launch=2),
                            tcc.live_pool(chunk_frames=15, max_streams_per_launch=2, generator="bf16")])
    builds = eng.live_ws_builds
    again = _run_pools(tcc, [tcc.live_pool(chunk_frames=15, max_streams_per_launch=2),
                             tcc.live_pool(chunk_frames=15, max_streams_per_launch=2, generator="bf16")])
    assert eng.live_ws_builds == builds, "a unit workspace was rebuilt for a shape both generators had run already"
    assert not _bf16_on(tcc)
    for i in range(2):
        assert torch.equal(both[0][i], alone[i]) and torch.equal(again[0][i], alone[i])      # fp32 untouched
        assert torch.equal(again[1][i], both[1][i])
        d = (both[1][i] - alone[i]).abs().max().item()
        assert 1e-5 < d <= BF16_O_HAT_TOL, d                     # genuinely the bf16 generator, within its tolerance


def test_live_bf16_stream_at_rates_of_its_own(tcc):
    src, tgt = _ses(4)
    n = 48000 * 2 + 11
    x = _wave(n, 8, 48000)
    noise = _noise(_frames(audio_io.resample_on_device(x, 48000, 22050).numel()), 9)
    st = tcc.live_stream(src, tgt, chunk_frames=15, noise=noise, sr_in=48000, sr_out=16000, generator="bf16")
    out = _run_stream(st, x, [4800] * (n // 4800))
    _check_against_the_bf16_conversion(tcc, out, x, src, tgt, noise, "48000 -> 16000", sr=48000, out_sr=16000)
