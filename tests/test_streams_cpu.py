"""openvoice_amd/streams.py, the front end StreamPool and LivePool share: the waveform buffer against a plain reference,
the handle table and the per-stream resamplers through a minimal pool, and that a failed open() leaves the real pools
as they were.  No GPU."""
import random
import types

import numpy as np
import pytest
import torch

from openvoice_amd import _lib, audio_io, live, longform, streams
from test_rates_cpu import _emulating_call, _FakeEngine, _FakeLiveModel, _FakeModel

HOP = 256


@pytest.mark.parametrize("pad", [384, 0])
def test_wave_buffer_equals_the_concatenated_pushes(pad):
    """200 pushes of 1 to 70 000 samples (runs of 1-sample pushes among them) with trims at increasing frames between
    them: the buffer always holds the pushed samples from ``base`` on, ``base`` on the hop grid, and never more than
    twice what it needs (or the 64 Ki floor)."""
    rng = random.Random(pad)
    sizes = []
    while len(sizes) < 200:
        sizes += [1] * rng.randint(5, 15) if rng.random() < 0.1 else [rng.randint(1, 70000)]
    sizes = sizes[:200]
    whole = torch.cat([torch.arange(a, a + k, dtype=torch.float32) for a, k in zip(np.cumsum([0] + sizes), sizes)])
    wave, pos, frame, caps = streams.WaveBuffer("cpu"), 0, 0, set()

    def check():
        assert wave.n == pos and wave.base % HOP == 0 and wave.len == pos - wave.base
        assert torch.equal(wave.valid(), whole[wave.base:pos])
        assert wave.len <= wave.buf.numel() <= max(2 * wave.len, 1 << 16)
        caps.add(wave.buf.numel())

    check()
    for k in sizes:
        wave.append(whole[pos:pos + k])
        pos += k
        check()
        if rng.random() < 0.3:
            frame = rng.randint(frame, pos // HOP)              # never past the samples received; sometimes no advance
            before = wave.base
            wave.trim(frame, HOP, pad)
            assert wave.base == max(before, frame * HOP - -(-pad // HOP) * HOP, 0)
            check()
    assert pos == sum(sizes) and wave.base > 0 and len(caps) > 10
    wave.release()
    assert wave.len == 0 and wave.valid().numel() == 0 and wave.n == pos


class _EchoPool(streams.PushedPool):
    """The smallest pool of pushed streams: its "conversion" returns each stream's new model-rate samples unchanged; a
    closed stream retires with its last sample, one shorter than 10 samples at ``close`` like the real pools' too short
    ones."""
    tau = 0.3

    def __init__(self):
        self._init_streams("cpu", 22050)

    def open(self, sr_in=None, sr_out=None, tau=None):
        st = types.SimpleNamespace(wave=streams.WaveBuffer("cpu"), closed=False, sent=0, total=None)
        st.tau = self._stream_tau(tau, "_EchoPool.open")
        return self._register(st, sr_in, sr_out)

    def close(self, h):
        self._streams[h].total = self._end_input(h)
        if self._streams[h].total < 10:
            self._retire(h)
            raise ValueError("too short")

    def step(self):
        self._take_input()
        routs, outs = self._output_rates(), {}
        for h, st in list(self._streams.items()):
            if st.wave.n > st.sent:
                outs[h] = st.wave.valid()[st.sent - st.wave.base:].clone()
                st.sent = st.wave.n
            if st.closed and st.sent == st.total:
                self._retire(h, finished=True)
        return self._deliver(outs, routs)


def test_pushed_pool_handles_and_their_errors():
    pool = _EchoPool()
    a, b = pool.open(), pool.open(tau=0.5)
    assert (a, b) == (0, 1) and pool.active == [0, 1] and pool._streams[b].tau == 0.5 and pool._streams[a].tau == 0.3
    with pytest.raises(_lib.OvError, match=r"^_EchoPool\.open: tau is one number per stream$"):
        pool.open(tau=[0.1])
    with pytest.raises(_lib.OvError):
        pool.open(tau=[0.1, 0.2])
    assert pool._next == 2
    pool.push(a, torch.arange(100.0))
    pool.push(b, [1.0, 2.0])
    out = pool.step()
    assert torch.equal(out[a], torch.arange(100.0)) and torch.equal(out[b], torch.tensor([1.0, 2.0]))
    with pytest.raises(RuntimeError, match=r"^no stream 7 in this pool$"):
        pool.push(7, torch.zeros(3))
    pool.close(a)
    with pytest.raises(RuntimeError, match=r"^push\(\) after close\(\) on stream 0$"):
        pool.push(a, torch.zeros(3))
    with pytest.raises(RuntimeError, match=r"^close\(\) called twice on stream 0$"):
        pool.close(a)
    assert pool.active == [0, 1]                 # closed, its tail still to run
    assert pool.step() == {} and pool.active == [1]
    with pytest.raises(ValueError):              # too short: retired at once, the other stream untouched
        pool.close(b)
    assert pool.active == []
    for call in (lambda: pool.push(a, torch.zeros(3)), lambda: pool.close(b), lambda: pool._stream(a)):
        with pytest.raises(RuntimeError, match=r"^stream [01] is closed$"):
            call()
    with pytest.raises(RuntimeError, match=r"^no stream 2 in this pool$"):
        pool.close(2)
    assert pool.open() == 2                      # handles are never reused


def test_pushed_pool_resamples_each_direction_in_one_launch_and_drops_its_keys(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, "call", _emulating_call(log))
    pool = _EchoPool()
    rng = np.random.default_rng(11)
    x = {n: (rng.standard_normal(k) * 0.3).astype(np.float32) for n, k in [("in", 9000), ("out", 7000), ("none", 5000)]}
    h = {"in": pool.open(sr_in=16000), "out": pool.open(sr_out=48000), "none": pool.open(sr_in=22050, sr_out=None),
         "short": pool.open(sr_in=8000, sr_out=44100)}
    st = {n: pool._streams[v] for n, v in h.items()}
    assert st["in"].rout is None and st["out"].rin is None and st["none"].rin is None and st["none"].rout is None
    assert len(pool._rin) == 2 and len(pool._rout) == 2 and pool._rin_owner == {st["in"].rin: st["in"],
                                                                               st["short"].rin: st["short"]}
    pool.push(h["short"], torch.zeros(3))
    with pytest.raises(ValueError):              # retired without finishing: both of its keys go at once
        pool.close(h["short"])
    assert st["short"].rin not in pool._rin and st["short"].rout not in pool._rout and len(pool._rin_owner) == 1
    pos, outs, steps = dict.fromkeys(x, 0), {n: [] for n in x}, 0
    while pool.active:
        for n, v in x.items():
            if pos[n] < v.size:
                k = int(rng.choice([1, 37, 441, 2205]))
                pool.push(h[n], torch.from_numpy(v[pos[n]:pos[n] + k]))
                pos[n] += k
                if pos[n] >= v.size:
                    pool.close(h[n])
        before = (pool._rin.launches, pool._rout.launches, len(log))
        res = pool.step()
        steps += 1
        after = (pool._rin.launches, pool._rout.launches, len(log))
        assert after[0] - before[0] <= 1 and after[1] - before[1] <= 1
        assert after[2] - before[2] == after[0] - before[0] + after[1] - before[1]
        for n in x:
            if h[n] in res:
                outs[n].append(res[h[n]].numpy().copy())
        if h["out"] not in pool.active:          # finished: its key was ended in that very step and is gone after it
            assert st["out"].rout not in pool._rout and pool._rout_ending == []
            assert sum(o.size for o in outs["out"]) == -(-x["out"].size * 48000 // 22050)
    assert steps > 5 and len(pool._rin) == len(pool._rout) == 0 and pool._rin_owner == {}
    assert np.array_equal(np.concatenate(outs["none"]), x["none"])
    for n, pair in [("in", (16000, 22050)), ("out", (22050, 48000))]:
        got, ref = np.concatenate(outs[n]), audio_io.resample_kaiser_best(x[n], *pair)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 2 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max())


def _state(pool):
    return (pool._next, getattr(pool, "_slots", None), list(getattr(pool, "_free_slots", [])), pool.active,
            len(pool._rin), len(pool._rout), dict(pool._rin_owner))


class _CondEngine(_FakeEngine):
    def live_conds(self, g_src, g_tgt):
        return {}


class _OpeningLiveModel(_FakeLiveModel):
    def engine(self):
        return _CondEngine()


def test_failed_open_leaves_a_live_pool_as_it_was():
    se = torch.zeros(1, 256, 1)
    bad = [(dict(noise=torch.zeros(1, 3, 10)), ValueError), (dict(noise=torch.zeros(1, 192, 10), seed=1), ValueError),
           (dict(sr_in=-8000, sr_out=48000), ValueError), (dict(sr_in=16000, sr_out=48000, seed=-1), ValueError),
           (dict(sr_in=16000, tau=[0.1, 0.2]), _lib.OvError)]
    pool = live.LivePool(_FakeLiveModel(), chunk_frames=15)
    before = _state(pool)
    assert before[:3] == (0, 0, [])
    for kw, err in bad:
        with pytest.raises(err):
            pool.open(se, se, **kw)
        assert _state(pool) == before and pool.mem is None
    # a pool that holds a stream: its arena is full, so a leaked slot would double it
    pool = live.LivePool(_OpeningLiveModel(), chunk_frames=15, max_streams_per_launch=1)
    assert pool.open(se, se, sr_in=16000, sr_out=48000, seed=3) == 0
    before = _state(pool)
    assert before[:2] == (1, 1) and before[2] == [] and before[4:6] == (1, 1)
    for kw, err in bad:
        with pytest.raises(err):
            pool.open(se, se, **kw)
        assert _state(pool) == before
    assert pool.open(se, se) == 1 and pool._streams[1].slot == 1 and pool._slots == 2


def test_failed_open_leaves_a_stream_pool_as_it_was():
    se = torch.zeros(1, 256, 1)
    pool = longform.WindowedConverter(_FakeModel(), window_frames=300).stream_pool()
    assert pool.open(se, se, sr_in=16000, sr_out=48000) == 0
    before = _state(pool)
    for kw, err in [(dict(sr_in=16000, sr_out=0), ValueError), (dict(sr_in=16000, tau=[0.1, 0.2]), _lib.OvError),
                    (dict(sr_out=48000, noise=torch.zeros(1, 192, 10), seed=1), ValueError)]:
        with pytest.raises(err):
            pool.open(se, se, **kw)
        assert _state(pool) == before
    with pytest.raises(_lib.OvError, match=r"^StreamPool\.open: tau is one number per stream$"):
        pool.open(se, se, tau=torch.tensor([0.1]))
    assert pool.open(se, se) == 1
