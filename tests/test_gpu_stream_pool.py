"""Many streams and recordings in shared launches on the MI355X (openvoice_amd/longform.py StreamPool, convert_many): the
multi-source framing kernel against the single-source one, a pool of streams against solo streams and the oracle, fault
isolation, convert_many against convert_long, and the resident workspaces of a pool whose ready count varies."""
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
O_HAT_TOL = 1e-4          # across kernel families (the Winograd choice depends on the launch size)
ORACLE_TOL = 1e-3


@pytest.fixture(scope="module")
def tcc(tmp_path_factory, synth_sd):
    from openvoice_amd import api
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp("stream_pool")
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, enable_watermark=False)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


def _ses(seed):
    gen = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


def _wave(n, seed, device=DEV):
    """Speech-like test signal: a few drifting partials under a syllable-rate envelope, plus a little noise."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    f = 140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t) + 7.0 * (seed % 5)
    phase = 2 * np.pi * torch.cumsum(f, 0) / 22050.0
    y = 0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5) + 0.05 * torch.sin(7.3 * phase)
    y = y * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t)) + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)
    return y.float().to(device)


def _noise(T, seed):
    return torch.randn(1, 192, T, generator=torch.Generator().manual_seed(seed)).to(DEV)


# ---- the multi-source framing kernel ----------------------------------------------------------------------------------
def test_multi_framing_matches_the_single_source_kernel_per_source():
    lengths = [256 * 300 + 77, 256 * 40, 1000, 256 * 1000 + 255, 256 * 77 + 1, 256 * 523 + 128]
    Tw = 37
    U = Tw + 3
    ld = (U + 3) // 4 * 4
    gen = torch.Generator().manual_seed(3)
    sources = [_wave(n, i) for i, n in enumerate(lengths)]
    pool = torch.cat(sources)
    bases = np.cumsum([0] + lengths[:-1]).tolist()
    recs, per_source = [], []
    for i, n in enumerate(lengths):
        T = longform.frames_of(n, NFFT, HOP)
        top = max(0, T - Tw)
        firsts = sorted(set([0, top, top // 2] + torch.randint(0, top + 1, (min(80, top + 1),), generator=gen).tolist()))
        per_source.append(firsts)
        recs += [(bases[i], n, f0) for f0 in firsts]
    bad = len(recs) // 2
    recs.insert(bad, (bases[3], PAD, 0))                  # n_samples <= pad: the kernel writes zeros, reads nothing
    recs.insert(bad + 1, (-256, 5000, 0))                 # base < 0
    recs.insert(bad + 2, (bases[5], lengths[5] + 1, 0))   # past the pool's end
    W = len(recs)
    assert W > 200
    recs_dev = torch.tensor(recs, dtype=torch.int64, device=DEV)
    multi = torch.full((W, HOP, ld), float("nan"), device=DEV)
    _lib.call("ov_frame_hops_multi_f32", pool, pool.numel(), recs_dev, W, HOP, PAD, U, ld, multi)
    spec_multi = native_spectrogram(DEV, NFFT, HOP).windows_multi(pool, recs_dev, Tw)
    torch.cuda.synchronize()
    for w in (bad, bad + 1, bad + 2):
        assert torch.all(multi[w] == 0)
    good = [w for w in range(W) if w not in (bad, bad + 1, bad + 2)]
    w_at = iter(good)
    for i, (n, firsts) in enumerate(zip(lengths, per_source)):
        fd = torch.tensor(firsts, dtype=torch.int64, device=DEV)
        one = torch.full((len(firsts), HOP, ld), float("nan"), device=DEV)
        _lib.call("ov_frame_hops_windows_f32", sources[i], n, fd, len(firsts), HOP, PAD, U, ld, one)
        spec_whole = spectrogram_torch(sources[i][None], NFFT, 22050, HOP, NFFT, center=False)
        T = spec_whole.shape[2]
        for j, f0 in enumerate(firsts):
            w = next(w_at)
            assert torch.equal(multi[w], one[j]), (i, f0)
            if f0 + Tw <= T:
                assert torch.equal(spec_multi[w], spec_whole[0, :, f0:f0 + Tw]), (i, f0)


# ---- the pool against solo streams ------------------------------------------------------------------------------------
POOL_LENGTHS = [256 * 1400 + 99, 256 * 900 + 3, 256 * 300 + 17, 256 * 2000, 256 * 450 + 200, 256 * 700 + 255]
PUSHES = [22050, 1, 44100, 3001, 70000, 257, 11025]


def _run_pool(tcc, lengths, waves, ses, noises, tau=0.3, Tw=512, M=32, short=None):
    """Interleaved pushes into one pool; stream i closes once all its samples are in.  Returns the outputs per stream
    (``short``: index of a stream to close after 200 samples; it must raise and leave the others alone)."""
    pool = tcc.stream_pool(tau=tau, window_frames=Tw, max_windows_per_launch=M)
    hs = [pool.open(ses[i][0], ses[i][1], noise=noises[i]) for i in range(len(lengths))]
    pos, outs, step = [0] * len(lengths), [[] for _ in lengths], 0
    while pool.active:
        for i, h in enumerate(hs):
            if h not in pool.active or pos[i] < 0:
                continue
            if i == short and pos[i] >= 200:
                with pytest.raises(ValueError):
                    pool.close(h)
                pos[i] = -1
                continue
            k = min(PUSHES[(step + i) % len(PUSHES)], lengths[i] - pos[i], 200 if i == short else 1 << 30)
            pool.push(h, waves[i][pos[i]:pos[i] + k])
            pos[i] += k
            if pos[i] == lengths[i]:
                pool.close(h)
                pos[i] = -1
        for h, o in pool.step().items():
            outs[hs.index(h)].append(o.clone())
        step += 1
    return [torch.cat(o) if o else None for o in outs]


def _run_solo(tcc, n, wave, se, noise, tau=0.3, Tw=512):
    st = tcc.stream(se[0], se[1], tau=tau, window_frames=Tw, noise=noise)
    outs, pos, i = [], 0, 0
    while pos < n:
        k = PUSHES[i % len(PUSHES)]
        i += 1
        outs.append(st.push(wave[pos:pos + k]))
        pos += min(k, n - pos)
    outs.append(st.close())
    return torch.cat(outs)


def test_pool_of_six_streams_equals_solo_streams(tcc):
    lengths = POOL_LENGTHS
    waves = [_wave(n, 10 + i) for i, n in enumerate(lengths)]
    ses = [_ses(100 + i) for i in range(len(lengths))]
    Ts = [longform.frames_of(n, NFFT, HOP) for n in lengths]
    assert sum(T < 512 for T in Ts) == 2
    noises = [_noise(T, 200 + i) for i, T in enumerate(Ts)]
    eng = tcc.model.engine()
    try:
        eng.use_winograd = False
        pool_direct = _run_pool(tcc, lengths, waves, ses, noises)
        solo_direct = [_run_solo(tcc, n, waves[i], ses[i], noises[i]) for i, n in enumerate(lengths)]
    finally:
        eng.use_winograd = True
    pool_default = _run_pool(tcc, lengths, waves, ses, noises)
    solo_default = [_run_solo(tcc, n, waves[i], ses[i], noises[i]) for i, n in enumerate(lengths)]
    errs = []
    for i, T in enumerate(Ts):
        assert pool_direct[i].shape == (256 * T,) and pool_default[i].shape == (256 * T,)
        assert torch.equal(pool_direct[i], solo_direct[i]), i
        errs.append((pool_default[i] - solo_default[i]).abs().max().item())
    print("pool vs solo streams, default kernels:", errs)
    assert max(errs) <= O_HAT_TOL


def test_pool_stream_at_tau_0_matches_the_oracle(tcc, synth_sd):
    from oracle import vc_oracle
    from openvoice_amd.utils import CONVERTER_MODEL_CONFIG
    n = 256 * 900 + 11
    T = longform.frames_of(n, NFFT, HOP)
    wave, se = _wave(n, 900), _ses(900)
    noise = _noise(T, 900)
    other = _wave(256 * 700, 901)
    outs = _run_pool(tcc, [n, other.numel()], [wave, other], [se, _ses(901)],
                     [noise, _noise(longform.frames_of(other.numel(), NFFT, HOP), 901)], tau=0.0, Tw=400)
    torch.set_num_threads(usable_cpus(16))
    with torch.no_grad():
        spec = vc_oracle.spectrogram(wave.cpu()[None])
        o_ref = vc_oracle.voice_conversion(synth_sd, CONVERTER_MODEL_CONFIG, spec, torch.tensor([T]), se[0].cpu(),
                                           se[1].cpu(), 0.0, noise.cpu(), zero_g=True)[0][0, 0]
    err = (outs[0].cpu() - o_ref).abs().max().item()
    print("pool stream (tau = 0, 400-frame windows) vs oracle:", err)
    assert err <= ORACLE_TOL


def test_a_too_short_stream_leaves_the_others_unchanged(tcc):
    lengths = POOL_LENGTHS[:3]
    waves = [_wave(n, 30 + i) for i, n in enumerate(lengths)]
    ses = [_ses(300 + i) for i in range(3)]
    noises = [_noise(longform.frames_of(n, NFFT, HOP), 400 + i) for i, n in enumerate(lengths)]
    clean = _run_pool(tcc, lengths, waves, ses, noises)
    faulty = _run_pool(tcc, lengths + [256 * 100], waves + [_wave(256 * 100, 33)], ses + [_ses(303)],
                       noises + [_noise(100, 403)], short=3)
    assert faulty[3] is None
    for i in range(3):
        assert torch.equal(faulty[i], clean[i]), i


# ---- convert_many against convert_long --------------------------------------------------------------------------------
def test_convert_many_equals_convert_long_per_item(tcc, tmp_path):
    from openvoice_amd import audio_io
    lengths = [256 * 1300 + 5, 256 * 900, 256 * 700 + 100, 256 * 300 + 11, 256 * 300 + 200]
    waves = [_wave(n, 50 + i) for i, n in enumerate(lengths)]
    path = str(tmp_path / "item1.wav")
    audio_io.write(path, waves[1].cpu().numpy(), 22050)
    items = [waves[0], path, waves[2].cpu(), waves[3], waves[4]]
    decoded = audio_io.load_to_device(path, 22050, DEV)
    Ts = [longform.frames_of(n if i != 1 else decoded.numel(), NFFT, HOP) for i, n in enumerate(lengths)]
    noises = [_noise(T, 500 + i) for i, T in enumerate(Ts)]
    ses = [_ses(600 + i) for i in range(5)]
    src, tgt = [s for s, _ in ses], [t for _, t in ses]
    eng = tcc.model.engine()
    kw = dict(tau=0.3, window_frames=512)
    try:
        eng.use_winograd = False
        many_direct = tcc.convert_many(items, src, tgt, windows_per_launch=4, noise=noises, **kw)
        long_direct = [tcc.convert_long(x, src[i], tgt[i], noise=noises[i], **kw) for i, x in enumerate(items)]
    finally:
        eng.use_winograd = True
    many_default = tcc.convert_many(items, src, tgt, windows_per_launch=4, noise=noises, **kw)
    long_default = [tcc.convert_long(x, src[i], tgt[i], noise=noises[i], **kw) for i, x in enumerate(items)]
    errs = []
    for i, T in enumerate(Ts):
        assert isinstance(many_direct[i], np.ndarray) and many_direct[i].shape == (256 * T,)
        assert np.array_equal(many_direct[i], long_direct[i]), i
        errs.append(float(np.abs(many_default[i] - long_default[i]).max()))
    print("convert_many vs convert_long, default kernels:", errs)
    assert max(errs) <= O_HAT_TOL
    # one embedding pair for all items, written to files
    outs = [str(tmp_path / f"out{i}.wav") for i in range(2)]
    assert tcc.convert_many(items[3:], src[0], tgt[0], output_paths=outs, noise=noises[3:], **kw) is None
    for i, p in enumerate(outs):
        assert audio_io.load_to_device(p, 22050, "cpu").numel() == 256 * Ts[3 + i]


# ---- resident workspaces ----------------------------------------------------------------------------------------------
def test_a_varying_ready_count_does_not_rebuild_workspaces(tcc):
    """A pool of 8 streams whose pushes make 0 .. 8+ windows ready per step over 20 steps: every launch is a ladder
    size, each size's workspace stays resident once built, and the peak allocation stays within the resident
    workspaces plus one step's transients."""
    Tw, M = 512, 8
    eng = tcc.model.engine()
    pool = tcc.stream_pool(tau=0.3, window_frames=Tw, max_windows_per_launch=M)
    ladder = pool.ladder
    assert ladder == [1, 2, 4, 8] and eng.resident_workspaces >= len(ladder) + 1
    eng._ws.clear()
    torch.cuda.empty_cache()
    for B in ladder:
        eng._workspace(B, Tw)
    resident = {k: id(v) for k, v in eng._ws.items()}
    budget = sum(eng.workspace_bytes(B, Tw) for B in ladder)
    print(f"ladder {ladder} at Tw = {Tw}: resident workspaces {budget / 2**30:.2f} GiB")
    gen = torch.Generator().manual_seed(8)
    hs = [pool.open(*_ses(800 + i)) for i in range(8)]
    waves = [_wave(256 * 4000, 800 + i) for i in range(8)]
    pos = [0] * 8
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    counts = []
    for step in range(20):
        for i, h in enumerate(hs):
            k = int(torch.randint(0, 3 * 255 * 256, (1,), generator=gen)) if (step + i) % 3 else 0
            pool.push(h, waves[i][pos[i]:pos[i] + k])
            pos[i] += k
        counts.append(sum(o.numel() for o in pool.step().values()))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    print("samples out per step:", counts, f"peak above the resident set: {peak / 2**20:.1f} MiB")
    assert len(set(counts)) > 3
    assert {k: id(v) for k, v in eng._ws.items()} == resident           # nothing rebuilt, nothing evicted
    assert peak <= eng.workspace_bytes(1, Tw)                            # less than one more workspace of the ladder
    eng.resident_workspaces = 1
