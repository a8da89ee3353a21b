"""Host side of many streams / recordings in shared launches (openvoice_amd/longform.py StreamPool, convert_many):
argument validation of ov_frame_hops_multi_f32, and the scheduling of the pool and of convert_many against the window
plans, with a fake model and a recording launch.  No GPU."""
import ctypes
import math
import os

import pytest
import torch

from openvoice_amd import _lib, longform
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG

HOP, NFFT, PAD, SPF = 256, 1024, 384, 256
OFF = 1 << 21          # stream s's waveform is s * OFF + arange(N): every buffered sample tells its stream and index

lib_built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built")


@lib_built
def test_multi_framing_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)         # never dereferenced: every call below fails validation before a launch
    f = lib.ov_frame_hops_multi_f32
    assert f(None, 1000, fake, 1, 256, 384, 8, 8, fake, None) == -1
    assert f(fake, 1000, None, 1, 256, 384, 8, 8, fake, None) == -1
    assert f(fake, 1000, fake, 1, 256, 384, 8, 8, None, None) == -1
    assert f(fake, 0, fake, 1, 256, 384, 8, 8, fake, None) == -1          # empty pool
    assert f(fake, 1000, fake, 0, 256, 384, 8, 8, fake, None) == -1       # no windows
    assert f(fake, 1000, fake, 65536, 256, 384, 8, 8, fake, None) == -1   # grid.z
    assert f(fake, 1000, fake, 1, 0, 384, 8, 8, fake, None) == -1         # hop
    assert f(fake, 1000, fake, 1, 2048, 384, 8, 8, fake, None) == -1
    assert f(fake, 1000, fake, 1, 256, -1, 8, 8, fake, None) == -1        # pad
    assert f(fake, 1000, fake, 1, 256, 384, 0, 8, fake, None) == -1       # U
    assert f(fake, 1000, fake, 1, 256, 384, 8, 7, fake, None) == -1       # ld < U
    assert f(fake, 1000, fake, 1, 256, 384, 7, 10, fake, None) == -3      # rows not 16-byte multiples
    assert f(fake, 1000, fake, 1, 256, 384, 7, 8, ctypes.c_void_p(4100), None) == -3
    assert lib.ov_version() >= 211


@lib_built
def test_torch_binding_of_the_multi_framing_rejects_cpu_tensors():
    ops = _lib.torch_ops()
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.frame_hops_multi_f32(torch.zeros(4096), 4096, torch.zeros(1, 3, dtype=torch.long), 1, 256, 384, 8, 8,
                                 torch.zeros(1, 256, 8))


def test_launch_ladder():
    assert longform.launch_ladder(1) == [1]
    assert longform.launch_ladder(32) == [1, 2, 4, 8, 16, 32]
    assert longform.launch_ladder(12) == [1, 2, 4, 8, 12]
    with pytest.raises(ValueError):
        longform.launch_ladder(0)


class _FakeModel(torch.nn.Module):
    """What WindowedConverter reads of a SynthesizerTrn: the config and the device of its parameters (CPU here)."""

    def __init__(self):
        super().__init__()
        self.model_cfg = dict(CONVERTER_MODEL_CONFIG)
        self.p = torch.nn.Parameter(torch.zeros(1))


def _recording_multi_launch(log):
    """Stands in for WindowedConverter._launch_multi on the CPU.  Each window's stream comes from its src embedding row
    (s), its absolute first frame from the pool sample at its span's base; its reads are checked against the span, its
    noise and tgt row against the stream's, and its core is written as s * OFF + absolute sample indices."""

    def launch(self, pool, records_dev, Tw, src_se, tgt_se, tau, nz, out, stitch_dev, n_out):
        W = records_dev.shape[0]
        recs, stitch = records_dev.tolist(), stitch_dev.tolist()
        assert len(stitch) == n_out <= W
        log["launches"].append((Tw, W, n_out))
        for w in range(W):
            if w >= n_out:                                           # padding: a copy of a real window
                assert recs[w] == recs[n_out - 1] and torch.equal(nz[w], nz[n_out - 1])
                assert torch.equal(src_se[w], src_se[n_out - 1]) and torch.equal(tgt_se[w], tgt_se[n_out - 1])
                continue
            base, n, f0 = recs[w]
            s = int(src_se[w, 0, 0].item())
            assert torch.all(src_se[w] == s) and torch.all(tgt_se[w] == -1 - s)
            assert 0 <= base and base + n <= pool.numel() and n > PAD
            span = pool[base:base + n]
            start = int(span[0].item()) - s * OFF                     # absolute index of the span's first sample
            assert torch.equal(span, s * OFF + torch.arange(start, start + n, dtype=torch.float32))
            assert start % HOP == 0
            fa = f0 + start // HOP
            first, last = f0 * HOP - PAD, (f0 + Tw - 1) * HOP + NFFT - PAD   # span samples the window reads
            st = log["streams"][s]
            assert first >= 0 or start == 0, "a window reads samples trimmed off the buffer"
            assert last <= n or st["closed"], "a window reads past the buffered samples before the end is known"
            assert torch.equal(nz[w], st["noise"][0, :, fa:fa + Tw])
            P, lo_off, length = stitch[w][1], stitch[w][1] - stitch[w][0], stitch[w][2] - stitch[w][1]
            lo = fa + lo_off
            st["ran"].append((fa, lo, lo + length))
            out[P * SPF:(P + length) * SPF] = s * OFF + torch.arange(lo * SPF, (lo + length) * SPF, dtype=out.dtype)
    return launch


def _need(k, Tw, core):
    end = k * core + Tw
    return max((end - 1) * HOP + NFFT - PAD, end * HOP + NFFT - 2 * PAD)


@pytest.mark.parametrize("Tw,M", [(512, 3), (512, 4), (300, 8)])
def test_pool_schedules_every_stream_like_its_solo_stream(monkeypatch, Tw, M):
    """S = 5 streams with interleaved pushes of random sizes (some longer than a window), opened and closed mid-way, one
    shorter than a window and one shorter than one frame.  Each stream runs exactly the windows of plan_windows(T) in
    order, each in the first step() after it is ready, with its own noise and embedding rows; every step runs
    ceil(R / M) launches of ladder sizes per window length; the outputs concatenate to each whole output; buffers stay
    bounded."""
    log = {"launches": [], "streams": {}}
    monkeypatch.setattr(longform.WindowedConverter, "_launch_multi", _recording_multi_launch(log))
    conv = longform.WindowedConverter(_FakeModel(), window_frames=Tw, windows_per_launch=1)
    pool = conv.stream_pool(tau=0.3, max_windows_per_launch=M)
    ladder = longform.launch_ladder(M)
    assert pool.ladder == ladder and pool.latency_samples == (Tw - 1) * HOP + NFFT - PAD
    gen = torch.Generator().manual_seed(Tw + M)
    # (samples, step at which it opens)
    spec = [(HOP * 2100 + 99, 0), (HOP * 1300 + 7, 0), (HOP * (Tw // 2) + 50, 3), (HOP * 3000, 5), (200, 2)]
    streams, outs = {}, {}
    for s, (N, _) in enumerate(spec):
        T = longform.frames_of(N, NFFT, HOP) if N > PAD else 0
        log["streams"][s] = dict(noise=torch.randn(1, 192, max(T, 1), generator=gen), ran=[], closed=False)
        streams[s] = dict(N=N, T=T, pos=0, h=None)
    step, biggest = 0, {}
    while True:
        for s, (N, at) in enumerate(spec):
            st = streams[s]
            if st["h"] is None and step >= at:
                st["h"] = pool.open(torch.full((1, 256, 1), float(s)), torch.full((1, 256, 1), -1.0 - s),
                                    noise=log["streams"][s]["noise"])
                outs[st["h"]] = []
            if st["h"] is None or log["streams"][s]["closed"]:
                continue
            if st["pos"] < N:
                k = int(torch.randint(1, 60000, (1,), generator=gen)) if s != 0 else [1, 44100, 7, 30000][step % 4]
                k = min(k, N - st["pos"])
                pool.push(st["h"], s * OFF + torch.arange(st["pos"], st["pos"] + k, dtype=torch.float32))
                st["pos"] += k
            if st["pos"] == N and step % 2 == s % 2:         # closed at a step of its own parity
                if st["T"] < 1:
                    with pytest.raises(ValueError):
                        pool.close(st["h"])
                    with pytest.raises(RuntimeError):
                        pool.push(st["h"], torch.zeros(10))
                    assert st["h"] not in pool.active
                    log["streams"][s]["closed"] = "failed"
                else:
                    pool.close(st["h"])
                    log["streams"][s]["closed"] = True
                    st["closed_at"] = step
        n_launches = len(log["launches"])
        got = pool.step()
        launches = log["launches"][n_launches:]
        for h, o in got.items():
            outs[h].append(o)
        # launches: ceil(R / M) per window length, each of the smallest ladder size that holds it
        per_len = {}
        for Tl, W, r in launches:
            per_len.setdefault(Tl, []).append((W, r))
        for Tl, ls in per_len.items():
            R = sum(r for _, r in ls)
            assert len(ls) == math.ceil(R / M)
            assert all(W == min(b for b in ladder if b >= r) for W, r in ls)
            assert all(r == M for _, r in ls[:-1])
        # every window ran in the first step after it was ready, in plan order
        core = conv.core
        for s, st in streams.items():
            if st["h"] is None or log["streams"][s]["closed"] == "failed":
                continue
            ran = log["streams"][s]["ran"]
            plan = longform.plan_windows(st["T"], Tw, conv.context, conv.grid)
            if log["streams"][s]["closed"]:
                assert ran == plan, (s, step)
                assert st["h"] not in pool.active
            else:
                ready = 0
                while _need(ready, Tw, core) <= st["pos"]:
                    ready += 1
                assert ran == plan[:ready], (s, step)
                biggest[s] = max(biggest.get(s, 0), pool._streams[st["h"]]._len)
        step += 1
        if all(st["h"] is not None for st in streams.values()) and not pool.active:
            break
        assert step < 1000
    for s, st in streams.items():
        if st["T"] < 1:
            assert outs[st["h"]] == []
            continue
        out = torch.cat(outs[st["h"]])
        assert torch.equal(out, s * OFF + torch.arange(st["T"] * SPF, dtype=torch.float32)), s
        with pytest.raises(RuntimeError):
            pool.push(st["h"], torch.zeros(10))
        if s in biggest:
            assert biggest[s] <= (Tw + conv.core + 4) * HOP + 60000     # bounded by the window and one push
    assert any(W > 1 for _, W, _ in log["launches"])      # windows of different streams did share launches
    assert any(Tl < Tw for Tl, _, _ in log["launches"])   # the short stream's T-frame window


def test_pool_steps_without_ready_windows_launch_nothing(monkeypatch):
    log = {"launches": [], "streams": {}}
    monkeypatch.setattr(longform.WindowedConverter, "_launch_multi", _recording_multi_launch(log))
    pool = longform.WindowedConverter(_FakeModel(), window_frames=512).stream_pool()
    h = pool.open(torch.zeros(1, 256, 1), torch.full((1, 256, 1), -1.0))
    pool.push(h, torch.zeros(1000))
    assert pool.step() == {} and log["launches"] == []
    assert pool.active == [h]
    with pytest.raises(RuntimeError):
        pool.push(12345, torch.zeros(3))


def test_convert_many_runs_each_items_plan_in_shared_launches(monkeypatch):
    """3 items longer than the window and 2 shorter ones of equal length: every item runs the windows of its own
    plan (the ones convert runs), full-length windows of different items share launches of windows_per_launch, the
    two short items share one launch, and each item's output is its whole output."""
    log = {"launches": [], "streams": {}}
    monkeypatch.setattr(longform.WindowedConverter, "_launch_multi", _recording_multi_launch(log))
    Tw, wpl = 512, 4
    conv = longform.WindowedConverter(_FakeModel(), window_frames=Tw, windows_per_launch=wpl)
    lengths = [HOP * 2100 + 99, HOP * 700 + 3, HOP * 1500, HOP * 300 + 11, HOP * 300 + 200]
    gen = torch.Generator().manual_seed(5)
    waves, noises = [], []
    for s, N in enumerate(lengths):
        T = longform.frames_of(N, NFFT, HOP)
        noises.append(torch.randn(1, 192, T, generator=gen))
        log["streams"][s] = dict(noise=noises[-1], ran=[], closed=True)
        waves.append(s * OFF + torch.arange(N, dtype=torch.float32))
    srcs = [torch.full((1, 256, 1), float(s)) for s in range(5)]
    tgts = [torch.full((1, 256, 1), -1.0 - s) for s in range(5)]
    outs = conv.convert_many(waves, srcs, tgts, tau=0.3, noises=noises)
    regular = 0
    for s, N in enumerate(lengths):
        T = longform.frames_of(N, NFFT, HOP)
        plan = longform.plan_windows(T, Tw, conv.context, conv.grid)
        assert log["streams"][s]["ran"] == plan
        assert torch.equal(outs[s], s * OFF + torch.arange(T * SPF, dtype=torch.float32))
        regular += len(plan) if T > Tw else 0
        # the windows convert (convert_long) runs for the item alone
        ran = []
        monkeypatch.setattr(longform.WindowedConverter, "_launch",
                            lambda self, wave, n, plan_dev, firsts, Tw_, *a: ran.extend(map(tuple, plan_dev.tolist())))
        conv.convert(waves[s], None, None, noise=noises[s])
        assert ran == plan
    full = [(W, r) for Tl, W, r in log["launches"] if Tl == Tw]
    assert len(full) == math.ceil(regular / wpl) and all(r == wpl for _, r in full[:-1])
    assert [(Tl, r) for Tl, _, r in log["launches"] if Tl != Tw] == [(300, 2)]
    with pytest.raises(ValueError):
        conv.convert_many(waves[:2], srcs, tgts)
    with pytest.raises(ValueError):
        conv.convert_many([torch.zeros(100)], srcs[:1], tgts[:1])
