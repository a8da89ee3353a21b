"""The block-wise watermark of streams on the MI355X (``ov_wm_embed_blocks_f32``, ``watermark.MarkBank``): the kernel
against the float64 mirror under a derived per-sample bound inside NaN-filled buffers, its independence of how a window is
cut into runs and launches, of what shares a launch and of the alignment of its offsets, a hold of one window against
``ov_wm_embed_windows_f32``, rejected records, and marked live and windowed streams end to end.

The per-sample bound (u = 2^-24, one fp32 rounding; x is the same fp32 input on both sides, exact in float64).  For one
block of H samples the kernel reduces as ``ov_wm_embed_windows_f32`` reduces a window of L = H, so the first two lines are
those of ``tests/test_gpu_watermark.py``:

* p_j: |dp_j| <= (H / 32 + 3) u mean_{S_j in block} |x|.
* a_m: |da| <= (H / 512 + 9) u a_m.
* u_j = b p_j + R_j is one fused operation (b p_j is exact), so one rounding, and it inherits the error dR of the R that
  came in: |du_j| <= |dp_j| + |dR_j| + u |u_j|.
* d_j = b max(a_m - u_j, 0): |dd_j| <= |da| + |du_j| + u |d_j|  (the subtraction rounds once; max and the signs are
  exact and 1-Lipschitz).
* R_j <- max(u_j - a_m, 0): |dR_j| <= |da| + |du_j| + u |R_j| -- the error of R grows by one such term per block, and
  this is what the next block takes as dR.  It is zero at a window's start; a state row holds R as the fp32 it is.
* y_i = x_i +- d_j, one rounding: |dy_i| <= |dd_j| + u (|x_i| + |d_j| + |dd_j|).

A factor 1 + 2^-10 covers the second-order terms dropped above.  The state row is checked against the mirror's R under
its own line.  Measured on the MI355X: worst error / bound 0.090 (H = 640), 0.035 (H = 3200), 0.010 (H = 16000) on the
samples and 0.012 / 0.001 / 0.001 on the state row, the same through both bindings."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, watermark  # noqa: E402
from oracle.nanbuf import Buf  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
KEY, STRENGTH, FLOOR = 0x1234ABCD5678, watermark.DEFAULT_STRENGTH, watermark.DEFAULT_FLOOR
W = watermark.WINDOW
HOLDS = [640, 3200, 16000]
PAYLOAD = 0xA5A50F35
STATE_ROWS, ROW = 5, 3


def _window(seed=1):
    """One carrier window: loud audio with a silent stretch and a 1e-5 stretch (whole blocks of them at H <= 3200)."""
    gen = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(W, generator=gen, dtype=torch.float64)
    x[3200:6400] = 0.0
    x[6400:9600] = 1e-5 * torch.randn(3200, generator=gen, dtype=torch.float64)
    return x.float()


def _walk(x, H, word):
    """The mirror of one window with the docstring's bound next to it: (y, bound of y, R after the last block, bound of
    it), float64."""
    x = x.astype(np.float64)
    c = watermark.chips_host(KEY, W)
    b = np.array([1.0 if (word >> j) & 1 else -1.0 for j in range(32)])
    y, by = x.copy(), np.zeros(W)
    R, dR = np.zeros(32), np.zeros(32)
    for m in range(0, W, H):
        blk, cm = x[m:m + H], c[m:m + H]
        p = (blk * cm).reshape(-1, 32).mean(axis=0)
        a = max(STRENGTH * np.sqrt(np.mean(blk * blk)), FLOOR)
        mabs = np.abs(blk).reshape(-1, 32).mean(axis=0)
        u = b * p + R
        d = b * np.maximum(a - u, 0.0)
        R = np.maximum(u - a, 0.0)
        dp, da = (H / 32 + 3) * U * mabs, (H / 512 + 9) * U * a
        du = dp + dR + U * np.abs(u)
        dd = da + du + U * np.abs(d)
        dR = da + du + U * R
        j = np.arange(H) % 32
        y[m:m + H] = blk + d[j] * cm
        by[m:m + H] = dd[j] + U * (np.abs(blk) + np.abs(d[j]) + dd[j])
    s = 1.0 + 2.0 ** -10
    return y, by * s, R, dR * s


def _launch(src, dst, recs, state):
    _lib.call("ov_wm_embed_blocks_f32", src, src.numel(), dst, dst.numel(), torch.tensor(recs, dtype=torch.int64).to(DEV),
              len(recs), state, state.shape[0], KEY, STRENGTH, FLOOR)


def _cut(H, run):
    """Records' (first block, blocks) of one window cut into runs of ``run`` blocks (None: all)."""
    M = W // H
    run = M if run is None else run
    return [(m, min(run, M - m)) for m in range(0, M, run)]


def _mark_window(x, H, run, layout="shift1", in_place=False):
    """One window marked in launches of one run each, inside NaN-filled buffers -> (marked samples, state row)."""
    src = Buf(x.reshape(1, 1, W), layout)
    dst = src if in_place else Buf(torch.full((1, 1, W), float("nan")), "out")
    state = torch.full((STATE_ROWS, 32), float("nan"), device=DEV)
    for m0, k in _cut(H, run):
        _launch(src.flat, dst.flat, [(src.off + m0 * H, dst.off + m0 * H, H, k, PAYLOAD, m0 * H, ROW, int(m0 == 0))], state)
    y = dst.get()[0, 0]                                   # nothing outside the window was written
    if not in_place:
        assert torch.equal(src.get()[0, 0], x)            # the source is only read
    state = state.cpu()
    assert torch.isnan(state[[0, 1, 2, 4]]).all()         # the other state rows stand
    return y, state[ROW]


@pytest.fixture(scope="module")
def window():
    return _window()


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("H", HOLDS)
def test_blocks_against_the_float64_mirror_whatever_the_cut(H, binding, window, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    y_ref, bound, R_ref, R_bound = _walk(window.numpy(), H, PAYLOAD)
    ys = [_mark_window(window, H, run) for run in (None, 1, 2)]
    ys.append(_mark_window(window, H, 2, layout="out", in_place=True))           # aligned, in place
    for y, R in ys[1:]:
        assert torch.equal(y, ys[0][0]) and torch.equal(R, ys[0][1])             # across the run cuts and alignments
    y, R = ys[0]
    assert torch.isfinite(y).all() and torch.isfinite(R).all() and (R >= 0).all()
    worst = float((np.abs(y.numpy().astype(np.float64) - y_ref) / bound).max())
    worst_R = float((np.abs(R.numpy().astype(np.float64) - R_ref) / np.maximum(R_bound, 1e-300)).max())
    print(f"H = {H}, {binding}: worst error / bound = {worst:.3f} (samples), {worst_R:.3f} (state row)")
    assert worst <= 1.0 and worst_R <= 1.0
    # the unchanged reader on the device output
    bits = np.array([(PAYLOAD >> j) & 1 for j in range(32)])
    assert np.array_equal(watermark.decode_host(y.numpy(), KEY)[0] >= 0.5, bits == 1)
    q, _ = watermark.detect_windows(y.to(DEV), [(0, 0, W, 0)], KEY)
    assert np.array_equal(q[0].cpu().numpy() >= 0, bits == 1)


def test_the_mirror_of_the_test_is_the_modules(window):
    """``_walk`` (which carries the bound) and ``watermark.mark_stream_host`` agree to float64 rounding."""
    word = watermark.groups_of("@MyS")[0]
    for H in HOLDS:
        y, _, _, _ = _walk(window.numpy(), H, word)
        ref = watermark.mark_stream_host(window.numpy(), "@MyS", KEY, hold=H)
        assert np.abs(y - ref).max() <= 1e-15


def test_three_records_in_one_launch_against_one_launch_each(window):
    """Three windows of three streams (holds 640, 3200, 16000; the middle one a continued run that reads its row) in one
    launch, at source offsets of three alignments: each equals its own launch, samples and state row."""
    xs = [_window(s) for s in (1, 2, 3)]
    gaps, H3 = [1, 2, 3], [640, 3200, 16000]
    offs, acc = [], 0
    for g in gaps:
        acc += g
        offs.append(acc)
        acc += W
    buf = torch.full((acc + 4,), float("nan"))
    for o, x in zip(offs, xs):
        buf[o:o + W] = x
    src = buf.to(DEV)
    recs = [(offs[0], offs[0], 640, 25, 1, 0, 0, 1), (offs[1] + 3200, offs[1] + 3200, 3200, 4, 2, 3200, 2, 0),
            (offs[2], offs[2], 16000, 1, 3, 0, 4, 1)]
    state0 = torch.full((STATE_ROWS, 32), float("nan"), device=DEV)
    state0[2] = torch.rand(32, generator=torch.Generator().manual_seed(9)).to(DEV) * 1e-3   # the continued run's R
    together, st_together = src.clone(), state0.clone()
    _launch(together, together, recs, st_together)
    alone, st_alone = src.clone(), state0.clone()
    for rec in recs:
        _launch(alone, alone, [rec], st_alone)
    torch.cuda.synchronize()
    nn = lambda t: t.cpu().nan_to_num(nan=7.0)
    assert torch.equal(nn(together), nn(alone)) and torch.equal(nn(st_together), nn(st_alone))
    out = together.cpu()
    touched = torch.zeros(out.numel(), dtype=torch.bool)
    touched[offs[0]:offs[0] + W] = touched[offs[1] + 3200:offs[1] + W] = touched[offs[2]:offs[2] + W] = True
    assert torch.isnan(out[~touched]).sum() == sum(gaps) + 4                      # the sentinels stand
    assert torch.equal(out[offs[1]:offs[1] + 3200], xs[1][:3200])                 # blocks outside the run too
    assert torch.isfinite(out[touched]).all() and not torch.equal(out[offs[1] + 3200:offs[1] + W], xs[1][3200:])
    assert torch.isnan(st_together.cpu()[[1, 3]]).all() and torch.isfinite(st_together.cpu()[[0, 2, 4]]).all()
    # an unaligned offset against an aligned one
    aligned = xs[1].to(DEV).clone()
    st = state0.clone()
    _launch(aligned, aligned, [(3200, 3200, 3200, 4, 2, 3200, 2, 0)], st)
    assert torch.equal(aligned[3200:].cpu(), out[offs[1] + 3200:offs[1] + W]) and torch.equal(st[2], st_together[2])


def test_a_hold_of_one_window_is_the_window_kernel_bit_for_bit(window):
    for off in (0, 1):
        src = torch.cat([torch.zeros(off), window]).to(DEV)
        a, b = torch.empty_like(src), torch.empty_like(src)
        state = torch.zeros(1, 32, device=DEV)
        _launch(src, a, [(off, off, W, 1, PAYLOAD, 0, 0, 1)], state)
        _lib.call("ov_wm_embed_windows_f32", src, src.numel(), b, b.numel(),
                  torch.tensor([(off, off, W, PAYLOAD)], dtype=torch.int64).to(DEV), 1, KEY, STRENGTH, FLOOR)
        assert torch.equal(a[off:], b[off:])


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_bad_records_write_nothing(binding, window, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    n = 20000
    src = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    dst = torch.full((n,), -7.0, device=DEV)
    state = torch.full((STATE_ROWS, 32), -3.0, device=DEV)
    bad = [(0, 0, 640, 0, 1, 0, 0, 1),                    # short: no block at all
           (n - 639, 0, 640, 1, 1, 0, 0, 1),              # past src
           (0, n - 1279, 640, 2, 1, 0, 0, 1),             # past dst
           (0, 0, 1000, 1, 1, 0, 0, 1),                   # a hold that is not in the list
           (0, 0, 640, 1, 1, 0, STATE_ROWS, 1),           # a state row out of range
           (0, 0, 640, 1, 1, 0, -1, 1), (0, 0, 640, 1, 1, 320, 0, 1), (0, 0, 640, 2, 1, 15360, 0, 1),
           (-1, 0, 640, 1, 1, 0, 0, 1), (0, 0, 640, 1, 1, 0, 0, 2), (0, 0, 512, 1, 1, 0, 0, 1), (0, 0, 640, 26, 1, 0, 0, 1)]
    _launch(src, dst, bad + [(100, 2000, 640, 1, 5, 640, 1, 1)], state)      # only the good record writes
    torch.cuda.synchronize()
    out, st = dst.cpu(), state.cpu()
    assert (out[:2000] == -7.0).all() and (out[2640:] == -7.0).all() and (out[2000:2640] != -7.0).all()
    assert (st[[0, 2, 3, 4]] == -3.0).all() and (st[1] >= 0).all()
    recs = torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    for args in [(src, n, dst, n, recs, 0, state, 5, KEY, STRENGTH, FLOOR), (src, n, dst, n, recs, 65536, state, 5, KEY, STRENGTH, FLOOR),
                 (src, 0, dst, n, recs, 1, state, 5, KEY, STRENGTH, FLOOR), (src, n, dst, 0, recs, 1, state, 5, KEY, STRENGTH, FLOOR),
                 (src, n, dst, n, recs, 1, state, 0, KEY, STRENGTH, FLOOR), (src, n, dst, n, recs, 1, None, 5, KEY, STRENGTH, FLOOR),
                 (src, n, dst, n, recs, 1, state, 5, -1, STRENGTH, FLOOR), (src, n, dst, n, recs, 1, state, 5, KEY, STRENGTH, 0.0)]:
        with pytest.raises(_lib.OvError):
            _lib.call("ov_wm_embed_blocks_f32", *args)
    assert torch.equal(dst.cpu(), out) and torch.equal(state.cpu(), st)


# ---- end to end: marked streams on the synthetic weights ---------------------------------------------------------------
MESSAGE = "@MyShell"
N_IN = 50000


def _make(tmp_path_factory, synth_sd, name, **kw):
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp(name)
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, **kw)
    t.load_ckpt(str(d / "checkpoint.pth"))
    t.model.engine().use_winograd = False       # direct kernels: a stream's bits do not depend on what shares a launch
    return t


@pytest.fixture(scope="module")
def native(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "wms_native", watermark="native", watermark_key=KEY)


@pytest.fixture(scope="module")
def plain(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "wms_plain", enable_watermark=False)


@pytest.fixture(scope="module")
def ses():
    gen = torch.Generator().manual_seed(11)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


@pytest.fixture(scope="module")
def wave():
    gen = torch.Generator().manual_seed(4)
    t = torch.arange(N_IN, dtype=torch.float64) / 22050.0
    phase = 2 * np.pi * torch.cumsum(140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / 22050.0
    y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(N_IN, generator=gen, dtype=torch.float64)).float()


def _run(stream, wave, push):
    outs = [stream.push(wave[i:i + push]) for i in range(0, wave.numel(), push)]
    outs.append(stream.close())
    return torch.cat([o for o in outs if o.numel()])


def _run_pool(pool, handles, wave, push):
    got = {h: [] for h in handles}
    for i in range(0, wave.numel(), push):
        for h in handles:
            pool.push(h, wave[i:i + push])
        for h, o in pool.step().items():
            got[h].append(o.clone())
    for h in handles:
        pool.close(h)
    for h, o in pool.step().items():
        got[h].append(o.clone())
    return {h: torch.cat(v) for h, v in got.items()}


@pytest.fixture(scope="module")
def live_unmarked(native, ses, wave):
    return _run(native.live_stream(*ses, seed=5), wave, 4000)


@pytest.fixture(scope="module")
def windowed_unmarked(native, ses, wave):
    return _run(native.stream(*ses, window_frames=255, seed=5), wave, 4000)


def test_marked_live_stream_whatever_the_chunking_and_the_pool(native, ses, wave, live_unmarked):
    kw = dict(seed=5, message=MESSAGE, watermark_hold=3200)
    a = _run(native.live_stream(*ses, **kw), wave, 4000)
    b = _run(native.live_stream(*ses, **kw), wave, 12345)
    assert torch.equal(a, b) and a.numel() == live_unmarked.numel() >= 48000
    pool = native.live_pool(max_streams_per_launch=4)
    hs = [pool.open(*ses, seed=5, message="other", watermark_hold=640, message_repeat=True), pool.open(*ses, **kw),
          pool.open(*ses, seed=5)]
    assert pool.latency_of(hs[1])[1] == pool.latency_of(hs[2])[1] + 3199 and pool.latency_samples == pool.latency_of(hs[1])[1]
    got = _run_pool(pool, hs, wave, 7000)
    assert torch.equal(got[hs[1]], a)
    assert torch.equal(got[hs[2]], live_unmarked)                                # message=None next to marked streams
    assert native.detect_watermark(a.cpu().numpy(), 2) == MESSAGE
    assert native.detect_watermark(got[hs[0]].cpu().numpy(), 1) == "othe"
    outside = torch.ones(a.numel(), dtype=torch.bool)
    outside[:16000] = outside[32000:48000] = False
    assert torch.equal(a[outside], live_unmarked[outside]) and not torch.equal(a[~outside], live_unmarked[~outside])


def test_live_stream_at_a_hold_of_one_window_is_mark_many(native, ses, wave, live_unmarked):
    s = native.live_stream(*ses, seed=5, message=MESSAGE)
    plain_s = native.live_stream(*ses, seed=5)
    assert s.latency_samples == plain_s.latency_samples + 15999
    got = _run(s, wave, 4000)
    want = native.watermark_model.mark_many([live_unmarked.clone()], MESSAGE)[0]
    assert torch.equal(got, want) and native.detect_watermark(got.cpu().numpy(), 2) == MESSAGE
    ahead = _run(native.live_stream(*ses, seed=5, message=MESSAGE, watermark_hold=640, lookahead_frames=0), wave, 4000)
    assert native.detect_watermark(ahead.cpu().numpy(), 2) == MESSAGE           # look-ahead streams mark what they emit


def test_windowed_stream_and_pool(native, ses, wave, windowed_unmarked):
    kw = dict(seed=5, message=MESSAGE, watermark_hold=3200)
    a = _run(native.stream(*ses, window_frames=255, **kw), wave, 4000)
    b = _run(native.stream(*ses, window_frames=255, **kw), wave, 12345)
    assert torch.equal(a, b)
    pool = native.stream_pool(window_frames=255)
    hs = [pool.open(*ses, seed=5, message="other", watermark_hold=640), pool.open(*ses, **kw), pool.open(*ses, seed=5)]
    got = _run_pool(pool, hs, wave, 7000)
    assert torch.equal(got[hs[1]], a) and torch.equal(got[hs[2]], windowed_unmarked)
    assert native.detect_watermark(a.cpu().numpy(), 2) == MESSAGE
    full = _run(native.stream(*ses, window_frames=255, seed=5, message=MESSAGE), wave, 4000)
    assert torch.equal(full, native.watermark_model.mark_many([windowed_unmarked.clone()], MESSAGE)[0])


def test_message_none_is_todays_output_and_the_keywords_are_checked(native, plain, ses, wave, live_unmarked,
                                                                      windowed_unmarked, capsys):
    wm = native.watermark_model
    before = wm.launches
    assert torch.equal(_run(plain.live_stream(*ses, seed=5), wave, 4000), live_unmarked)
    assert torch.equal(_run(plain.stream(*ses, window_frames=255, seed=5), wave, 4000), windowed_unmarked)
    assert wm.launches == before
    for call in (lambda **kw: plain.live_stream(*ses, **kw), lambda **kw: plain.stream(*ses, **kw),
                 lambda **kw: plain.live_pool().open(*ses, **kw), lambda **kw: plain.stream_pool().open(*ses, **kw)):
        with pytest.raises(ValueError, match="native"):
            call(message=MESSAGE)
    for call in (lambda **kw: native.live_stream(*ses, **kw), lambda **kw: native.stream(*ses, **kw)):
        with pytest.raises(ValueError, match="watermark_hold"):
            call(message=MESSAGE, watermark_hold=1000)
    # a stream too short for the message: the upstream notice, once
    capsys.readouterr()
    short = _run(native.live_stream(*ses, seed=5, message=MESSAGE, watermark_hold=640), wave[:30000], 30000)
    assert capsys.readouterr().out.count("Audio too short, fail to add watermark") == 1
    assert native.detect_watermark(short.cpu().numpy(), 1) == MESSAGE[:4]
