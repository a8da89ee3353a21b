"""Counter-based noise on the MI355X (openvoice_amd/noise.py, csrc/noise.hip): the kernel against the float64
restatement, its purity bit for bit, records it must refuse, and ``seed=`` through every layer -- a seeded call equals
the call with the explicit tensor ``noise.normal`` makes, and live streams, windowed streams, ``convert_long`` and
``convert_many`` are one function of the audio."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, longform, noise  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")
# A plain fp32 evaluation of the definition with the angle rounded as 2 pi u2 (worse than what the kernel does) reaches
# 1.0e-5 on 768 000 values; the bar is twice that.
KERNEL_TOL = 2e-5
SEED = 20261018


# ---- the kernel -------------------------------------------------------------------------------------------------------
def _launch(records, C, dst):
    table = torch.tensor(records, dtype=torch.int64).to(DEV)
    _lib.call("ov_normal_philox_f32", table, len(records), C, dst, dst.numel(), max(max(r[4] for r in records), 0))


def _canvas(n):
    return torch.full((n,), NAN, dtype=torch.float32, device=DEV)


def _expected(records, C, n):
    want = np.full(n, np.nan)
    for s, k, purpose, f0, nf, off, ld in records:
        ref = noise.normal_host((s, k), C, f0, nf, purpose=purpose)
        for c in range(C):
            want[off + c * ld:off + c * ld + nf] = ref[c]
    return want


@pytest.mark.parametrize("C", [1, 2, 192])
def test_kernel_matches_the_float64_restatement(C):
    records, off = [], 0
    for f0 in (0, 1, 2, 3, 5, (1 << 34) - 8):
        for nf in (1, 2, 3, 4, 5, 7, 8, 64, 65):
            if f0 + nf > 1 << 34:
                continue
            ld = nf | 1                                     # odd: the rows of a slab take every alignment in turn
            off += (len(records) - off) % 4                 # dst_off = 0, 1, 2, 3 (mod 4) in turn
            records.append((SEED + len(records), len(records) % 3, len(records) % 2, f0, nf, off, ld))
            off += C * ld + 3
    assert len(records) >= 40 and {r[5] % 4 for r in records} == {0, 1, 2, 3}
    dst = _canvas(off + 5)
    _launch(records, C, dst)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().astype(np.float64)
    want = _expected(records, C, dst.numel())
    inside = ~np.isnan(want)
    assert np.isnan(got[~inside]).all(), "an element outside every slab was written"
    assert not np.isnan(got[inside]).any(), "an element of a slab was not written"
    err = float(np.abs(got[inside] - want[inside]).max())
    print(f"C = {C}: {len(records)} records, {int(inside.sum())} values, max |kernel - float64| = {err:.3e}")
    assert err <= KERNEL_TOL
    assert np.abs(got[inside]).max() <= np.sqrt(50 * np.log(2)) + KERNEL_TOL


def test_kernel_is_pure_bit_for_bit():
    C, f0, nf = 192, 5, 16
    rec = lambda f, n, off, ld, seed=SEED, stream=3: (seed, stream, 0, f, n, off, ld)
    one = _canvas(C * nf)
    _launch([rec(f0, nf, 0, nf)], C, one)
    slab = one.view(C, nf).clone()
    assert not torch.isnan(slab).any()
    # two records cut at each interior point, every cut in its own region of one canvas: one launch of 30 records
    cuts = _canvas(15 * C * nf)
    records = []
    for k in range(1, nf):
        base = (k - 1) * C * nf
        records += [rec(f0, k, base, nf), rec(f0 + k, nf - k, base + k, nf)]
    _launch(records, C, cuts)
    for k in range(1, nf):
        assert torch.equal(cuts.view(15, C, nf)[k - 1], slab), f"cut at {k}"
    # the four destination alignments (ld = 17: the rows shift through the alignments too)
    for a in range(4):
        for ld in (16, 17):
            dst = _canvas(a + C * ld + 4)
            _launch([rec(f0, nf, a, ld)], C, dst)
            assert torch.equal(dst[a:a + C * ld].view(C, ld)[:, :nf], slab), (a, ld)
            assert torch.isnan(dst[:a]).all() and torch.isnan(dst[a + (C - 1) * ld + nf:]).all()
    # alone (R = 1) against among 63 other records
    many = _canvas(64 * C * 24)
    records = [rec(7 * i, 1 + i % 24, i * C * 24, 24, seed=SEED + i, stream=i) for i in range(64)]
    records[40] = rec(f0, nf, 40 * C * 24, 24)
    _launch(records, C, many)
    assert torch.equal(many[40 * C * 24:41 * C * 24].view(C, 24)[:, :nf], slab)
    # two runs
    again = _canvas(C * nf)
    _launch([rec(f0, nf, 0, nf)], C, again)
    assert torch.equal(again.view(C, nf), slab)
    # and the public one-launch form is the same function
    assert torch.equal(noise.normal((SEED, 3), C, f0, nf, DEV), slab)


def test_bad_records_write_nothing_and_good_ones_are_still_written():
    C, n = 4, 4096
    good = [(SEED, 0, 0, 10, 8, 0, 8), (SEED, 1, 0, 0, 5, 3000, 7)]
    bad = [
        (SEED, 0, 0, 0, -3, 100, 8),                    # negative nf
        (SEED, 0, 0, 0, 9, 200, 8),                     # nf > dst_ld
        (SEED, 0, 0, 0, 8, n - 4 * 8 + 1, 8),           # the slab ends one element beyond dst_elems
        (SEED, 0, 0, 0, 8, n - 8, 8),                   # first row in range, later rows beyond
        (SEED, 0, 0, (1 << 34) - 7, 8, 300, 8),         # f0 + nf > 2^34
        (SEED, 0, 0, -1, 8, 400, 8),                    # negative f0
        (SEED, 0, 0, 0, 8, -4, 8),                      # negative dst_off
        (-1, 0, 0, 0, 8, 500, 8),                       # negative seed
        (SEED, 1 << 32, 0, 0, 8, 600, 8),               # stream beyond 32 bits
        (SEED, 0, 1 << 32, 0, 8, 700, 8),               # purpose beyond 32 bits
    ]
    dst = _canvas(n)
    _launch(bad[:5] + good[:1] + bad[5:] + good[1:], C, dst)        # OV_OK: _lib.call raises on any other code
    torch.cuda.synchronize()
    got = dst.cpu().numpy().astype(np.float64)
    want = _expected(good, C, n)
    inside = ~np.isnan(want)
    assert np.isnan(got[~inside]).all(), "a bad record wrote something"
    assert np.abs(got[inside] - want[inside]).max() <= KERNEL_TOL
    only_bad = _canvas(n)
    _launch(bad, C, only_bad)
    assert torch.isnan(only_bad).all()


def test_fill_validates_on_the_host():
    dst = torch.zeros(2, 16, device=DEV)
    for rec in [(1, 0, 0, 0, 17, 0, 17), (1, 0, 0, 0, 8, 9, 16), (1, 0, 0, 0, 8, 0, 4), (-1, 0, 0, 0, 8, 0, 16),
                (1, 0, 0, (1 << 34) - 4, 8, 0, 16), (1, 0, 0, 0, 8, 0)]:
        with pytest.raises(ValueError):
            noise.fill([rec], 2, dst)
    assert torch.all(dst == 0)
    with pytest.raises(ValueError):
        noise.fill([(1, 0, 0, 0, 8, 0, 16)], 2, dst.cpu())
    noise.fill([], 2, dst)
    assert noise.normal(5, 3, 7, 0, DEV).shape == (3, 0)


# ---- through the layers -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("noise")
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


@pytest.fixture
def direct(tcc):
    """The existing bit-for-bit contracts between launches of different sizes hold with the direct kernels."""
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


def _frames(n):
    return (n + 2 * 384 - 1024) // 256 + 1


def _N(stream, T, seed=SEED):
    return noise.normal((seed, stream), 192, 0, T, DEV)[None]


def _run_stream(st, wave, pushes):
    outs, i = [], 0
    for n in pushes:
        outs.append(st.push(wave[i:i + n]))
        i += n
    outs.append(st.push(wave[i:]))
    outs.append(st.close())
    return torch.cat(outs)


def _dev(x):
    return torch.as_tensor(x).to(DEV)


def test_convert_batch_seed_equals_the_explicit_tensor(tcc):
    src, tgt = _ses(1)
    n = 256 * 40 + 90
    T = _frames(n)
    waves = torch.stack([_wave(n, 10 + b) for b in range(3)])
    N = torch.cat([_N(b, T) for b in range(3)])
    a, la = tcc.convert_batch(waves, src, tgt, seed=SEED)
    b, lb = tcc.convert_batch(waves, src, tgt, noise=N)
    assert a.shape == (3, 1, 256 * T) and torch.equal(a, b) and torch.equal(la, lb)
    # an item's noise is its own: item 1 alone, on stream 1
    solo = tcc.convert_batch(waves[1:2], src, tgt, seed=[(SEED, 1)])[0]
    assert torch.equal(solo, tcc.convert_batch(waves[1:2], src, tgt, noise=N[1:2])[0])
    assert not torch.equal(a, tcc.convert_batch(waves, src, tgt, seed=SEED + 1)[0])
    tcc.enable_graphs()
    try:
        ga = tcc.convert_batch(waves, src, tgt, seed=SEED)[0]
        gb = tcc.convert_batch(waves, src, tgt, noise=N)[0]
        ga2 = tcc.convert_batch(waves, src, tgt, seed=SEED)[0]             # a replay of the captured graph
    finally:
        tcc.enable_graphs(False)
    assert torch.equal(ga, gb) and torch.equal(ga, ga2)


def test_convert_batch_seed_on_a_ragged_list(tcc):
    src, tgt = _ses(2)
    lengths = [256 * 40 + 90, 256 * 23, 256 * 31 + 7]
    waves = [_wave(n, 20 + i) for i, n in enumerate(lengths)]
    Ts = [_frames(n) for n in lengths]
    full = torch.cat([_N(b, max(Ts)) for b in range(3)])
    a, la = tcc.convert_batch(waves, src, tgt, seed=SEED)
    b, lb = tcc.convert_batch(waves, src, tgt, noise=full)
    assert torch.equal(a, b) and la.tolist() == [256 * t for t in Ts] == lb.tolist()
    with pytest.raises(ValueError):
        tcc.convert_batch(waves, src, tgt, seed=[1, 2])                    # a list of the wrong length


def test_convert_long_seed_equals_the_explicit_tensor(tcc):
    src, tgt = _ses(3)
    n = 256 * 500 + 17
    T = _frames(n)
    wave = _wave(n, 30)
    assert len(longform.plan_windows(T, 300, 120, 15)) >= 3
    kw = dict(tau=0.3, window_frames=300, windows_per_launch=2)
    a = tcc.convert_long(wave, src, tgt, seed=SEED, **kw)
    b = tcc.convert_long(wave, src, tgt, noise=_N(0, T), **kw)
    assert a.shape == (256 * T,) and np.array_equal(a, b)
    c = tcc.convert_long(wave, src, tgt, seed=(SEED, 4), **kw)
    assert np.array_equal(c, tcc.convert_long(wave, src, tgt, noise=_N(4, T), **kw)) and not np.array_equal(a, c)
    # the model seam
    o = tcc.model.voice_conversion_windowed(wave, src, tgt, tau=0.3, seed=SEED, window_frames=300, windows_per_launch=2)
    assert np.array_equal(o[0, 0].cpu().numpy(), a)


def test_windowed_stream_seed_equals_convert_long(tcc):
    src, tgt = _ses(4)
    n = 256 * 500 + 17
    wave = _wave(n, 40)
    want = _dev(tcc.convert_long(wave, src, tgt, tau=0.3, window_frames=300, windows_per_launch=1, seed=SEED))
    st = tcc.stream(src, tgt, tau=0.3, window_frames=300, seed=SEED)
    got = _run_stream(st, wave, [1, 1000])
    assert torch.equal(got, want)
    st = tcc.stream(src, tgt, tau=0.3, window_frames=300, seed=SEED)
    assert torch.equal(_run_stream(st, wave, [30000] * 4), want)


def test_live_stream_seed(tcc, direct):
    src, tgt = _ses(5)
    n = 256 * 100 + 31
    T = _frames(n)
    wave = _wave(n, 50)
    pushes = [2205] * (n // 2205)
    explicit = _run_stream(tcc.live_stream(src, tgt, chunk_frames=15, noise=_N(0, T)), wave, pushes)
    seeded = _run_stream(tcc.live_stream(src, tgt, chunk_frames=15, seed=SEED), wave, pushes)
    assert seeded.shape == (256 * T,) and torch.equal(seeded, explicit)
    other = _run_stream(tcc.live_stream(src, tgt, chunk_frames=15, seed=SEED), wave, [1, 2, 3, 500, 4096, 9000])
    assert torch.equal(other, seeded)
    # the same function of the audio as the offline conversion
    assert torch.equal(seeded, _dev(tcc.convert_long(wave, src, tgt, seed=SEED)))
    # inside a pool of three, other seeds (one unseeded, one with a tensor) and other push sizes, stepped together
    pool = tcc.live_pool(chunk_frames=15, max_streams_per_launch=4)
    lengths = [n, 256 * 60 + 5, 256 * 130]
    waves = [wave, _wave(lengths[1], 51), _wave(lengths[2], 52)]
    hs = [pool.open(src, tgt, seed=SEED), pool.open(*_ses(6), seed=(SEED + 1, 9)),
          pool.open(*_ses(7), noise=_N(5, _frames(lengths[2])))]
    steps, pos, outs = [3001, 2205, 4444], [0, 0, 0], [[], [], []]
    while pool.active:
        for i, h in enumerate(hs):
            if pos[i] < lengths[i]:
                pool.push(h, waves[i][pos[i]:pos[i] + steps[i]])
                pos[i] += steps[i]
                if pos[i] >= lengths[i]:
                    pool.close(h)
        for h, o in pool.step().items():
            outs[hs.index(h)].append(o)
    assert torch.equal(torch.cat(outs[0]), seeded)
    solo1 = _run_stream(tcc.live_stream(*_ses(6), chunk_frames=15, seed=(SEED + 1, 9)), waves[1], [7000])
    assert torch.equal(torch.cat(outs[1]), solo1)


def test_live_stream_seed_on_the_bf16_generator(tcc):
    src, tgt = _ses(8)
    n = 256 * 60 + 31
    wave = _wave(n, 60)
    pushes = [2205] * (n // 2205)
    explicit = _run_stream(tcc.live_stream(src, tgt, chunk_frames=15, noise=_N(0, _frames(n)), generator="bf16"), wave,
                           pushes)
    seeded = _run_stream(tcc.live_stream(src, tgt, chunk_frames=15, seed=SEED, generator="bf16"), wave, pushes)
    assert torch.equal(seeded, explicit)


def test_stream_pool_seeded_member_equals_its_solo_stream(tcc, direct):
    n = [256 * 500 + 17, 256 * 350]
    waves = [_wave(n[0], 70), _wave(n[1], 71)]
    ses = [_ses(70), _ses(71)]
    pool = tcc.stream_pool(tau=0.3, window_frames=300, max_windows_per_launch=4)
    hs = [pool.open(*ses[0], seed=SEED), pool.open(*ses[1], noise=_N(2, _frames(n[1])))]
    pos, outs, step = [0, 0], [[], []], [40000, 33333]
    while pool.active:
        for i, h in enumerate(hs):
            if pos[i] < n[i]:
                pool.push(h, waves[i][pos[i]:pos[i] + step[i]])
                pos[i] += step[i]
                if pos[i] >= n[i]:
                    pool.close(h)
        for h, o in pool.step().items():
            outs[hs.index(h)].append(o)
    solo = _run_stream(tcc.stream(*ses[0], tau=0.3, window_frames=300, seed=SEED), waves[0], [50000])
    assert torch.equal(torch.cat(outs[0]), solo)
    # the member with a tensor, in launches shared with the seeded one (the mixed-launch path)
    solo1 = _run_stream(tcc.stream(*ses[1], tau=0.3, window_frames=300, noise=_N(2, _frames(n[1]))), waves[1], [50000])
    assert torch.equal(torch.cat(outs[1]), solo1)


def test_convert_many_seed_equals_convert_long_per_item(tcc, direct):
    lengths = [256 * 500 + 17, 256 * 200 + 5, 256 * 330]
    waves = [_wave(n, 80 + i) for i, n in enumerate(lengths)]
    ses = [_ses(80 + i) for i in range(3)]
    src, tgt = [s for s, _ in ses], [t for _, t in ses]
    kw = dict(tau=0.3, window_frames=300)
    many = tcc.convert_many(waves, src, tgt, windows_per_launch=4, seed=SEED, **kw)
    for i, x in enumerate(waves):
        one = tcc.convert_long(x, src[i], tgt[i], seed=(SEED, i), **kw)
        assert np.array_equal(many[i], one), i
    listed = tcc.convert_many(waves[:2], src[:2], tgt[:2], windows_per_launch=4, seed=[(SEED, 0), (SEED, 1)], **kw)
    assert np.array_equal(listed[0], many[0]) and np.array_equal(listed[1], many[1])


def test_seeded_streams_hold_no_noise_tensor(tcc):
    src, tgt = _ses(9)
    wave = _wave(256 * 400, 90)
    st = tcc.stream(src, tgt, window_frames=300, seed=SEED)
    for i in range(3):
        st.push(wave[i * 34000:(i + 1) * 34000])
    assert st._k >= 1 and st._noise is None and st._nz is None
    ls = tcc.live_stream(src, tgt, chunk_frames=15, seed=SEED)
    for i in range(3):
        ls.push(wave[i * 9000:(i + 1) * 9000])
    live = ls._pool._streams[ls._h]
    assert live.cas.n[0] >= 15 and live.noise is None and live.seed == (SEED, 0)
    tensors = [k for k, v in {**vars(live), **vars(live.wave)}.items() if torch.is_tensor(v) and k != "buf"]
    assert tensors == [], tensors


def test_seed_and_noise_together_raise_on_every_entry_point(tcc):
    src, tgt = _ses(0)
    nz = _N(0, 64)
    wave = _wave(256 * 40, 1)
    spec = torch.rand(1, 513, 20, device=DEV)
    lens = torch.tensor([20], device=DEV)
    calls = [
        lambda: tcc.convert_batch(wave[None], src, tgt, noise=nz, seed=1),
        lambda: tcc.convert_long(wave, src, tgt, noise=nz, seed=1),
        lambda: tcc.convert_many([wave], src, tgt, noise=[nz], seed=1),
        lambda: tcc.stream(src, tgt, noise=nz, seed=1),
        lambda: tcc.live_stream(src, tgt, noise=nz, seed=1),
        lambda: tcc.stream_pool().open(src, tgt, noise=nz, seed=1),
        lambda: tcc.live_pool().open(src, tgt, noise=nz, seed=1),
        lambda: tcc.model.voice_conversion(spec, lens, src, tgt, noise=nz[:, :, :20], seed=1),
        lambda: tcc.model.voice_conversion(spec, lens, src, tgt, noise=nz[:, :, :20], seed=1, graph=True),
        lambda: tcc.model.voice_conversion_windowed(wave, src, tgt, noise=nz, seed=1),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="mutually exclusive"):
            call()
    for bad in (True, -1, 1 << 63, (1, 1 << 32)):
        with pytest.raises(ValueError):
            tcc.convert_long(wave, src, tgt, seed=bad)


# ---- TTS --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tts(tmp_path_factory, synth_tts_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import CONVERTER_DATA_CONFIG, CONVERTER_MODEL_CONFIG
    d = tmp_path_factory.mktemp("noise_tts")
    cfg = {"data": dict(CONVERTER_DATA_CONFIG, n_speakers=10, text_cleaners=["cjke_cleaners2"], add_blank=True),
           "model": dict(CONVERTER_MODEL_CONFIG), "symbols": [f"s{i}" for i in range(68)],
           "speakers": {"default": 1, "whispering": 2}}
    (d / "config.json").write_text(json.dumps(cfg))
    torch.save({"model": synth_tts_sd}, d / "checkpoint.pth")
    t = api.BaseSpeakerTTS(str(d / "config.json"), device=DEV)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


def _ids(lengths, seed=1):
    from openvoice_amd import api
    gen = torch.Generator().manual_seed(seed)
    return [api.intersperse(torch.randint(1, 68, (n,), generator=gen).tolist(), 0) for n in lengths]


def test_infer_seed_equals_the_explicit_tensors(tts):
    ids = _ids((12, 7))
    lens = torch.tensor([len(s) for s in ids])
    Tx = int(lens.max())
    x = torch.zeros(2, Tx, dtype=torch.long)
    for b, s in enumerate(ids):
        x[b, :len(s)] = torch.tensor(s)
    sid = torch.tensor([1, 2])
    kw = dict(sid=sid.to(DEV), noise_scale=0.667, noise_scale_w=0.6, length_scale=1.0)
    o, attn, y_mask, _ = tts.model.infer(x.to(DEV), lens.to(DEV), seed=SEED, **kw)
    Ty = y_mask.shape[2]
    W = torch.stack([noise.normal((SEED, b), 2, 0, Tx, DEV, purpose=1) for b in range(2)])
    Z = torch.stack([noise.normal((SEED, b), 192, 0, Ty, DEV, purpose=2) for b in range(2)])
    o2, attn2, y_mask2, _ = tts.model.infer(x.to(DEV), lens.to(DEV), noise_w=W, noise_z=Z, **kw)
    assert Ty > 0 and torch.equal(y_mask, y_mask2) and torch.equal(attn, attn2) and torch.equal(o, o2)
    with pytest.raises(ValueError, match="mutually exclusive"):
        tts.model.infer(x.to(DEV), lens.to(DEV), noise_w=W, seed=SEED, **kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        tts.model.infer(x.to(DEV), lens.to(DEV), noise_z=Z, seed=SEED, **kw)
    # the padded form behind tts_from_ids(batched=True) and VoiceCloner
    frames = y_mask[:, 0].sum(1).long().tolist()
    op, fp = tts.infer_padded(ids, 1, seed=SEED)
    oq, fq = tts.infer_padded(ids, 1, noise_w=[W[b] for b in range(2)],
                              noise_z=[noise.normal((SEED, b), 192, 0, max(fp.tolist()), DEV, purpose=2) for b in range(2)])
    assert torch.equal(fp, fq) and torch.equal(op, oq) and len(frames) == 2


def test_tts_from_ids_seed_is_reproducible_and_batching_keeps_the_lengths(tts):
    ids = _ids((12, 7, 20), seed=2)
    spk = tts.hps.speakers["default"]
    a = tts.tts_from_ids(ids, spk, seed=SEED)
    torch.manual_seed(123)                                   # torch's generator is not involved
    b = tts.tts_from_ids(ids, spk, seed=SEED)
    assert len(a) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    batched = tts.tts_from_ids(ids, spk, seed=SEED, batched=True)
    assert [len(x) for x in batched] == [len(x) for x in a]
    assert all(np.array_equal(x, y) for x, y in zip(batched, tts.tts_from_ids(ids, spk, seed=SEED, batched=True)))
    other = tts.tts_from_ids(ids, spk, seed=SEED + 1)
    assert any(len(x) != len(y) or not np.array_equal(x, y) for x, y in zip(a, other))
    for kw in (dict(noise_w=[None] * 3), dict(noise_z=[None] * 3)):
        with pytest.raises(ValueError, match="mutually exclusive"):
            tts.tts_from_ids(ids, spk, seed=SEED, **kw)
