"""Host side of rate conversion inside streams (openvoice_amd/rates.py): the resampler schedule and the record semantics
of ov_polyphase_fir_rows_f32 emulated in float64 against the whole-file resampler, the latency bound, one launch per
direction per pool step, the entry point's host checks and the argument checks.  No GPU."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from openvoice_amd import _lib, audio_io, longform, rates
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG

PAIRS = [(48000, 22050), (44100, 22050), (16000, 22050), (8000, 22050), (22050, 48000), (22050, 16000), (22050, 44100)]
lib_built = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libopenvoice_amd.so not built")


def _run_records(recs, src, h, dst):
    """float64 emulation of ov_polyphase_fir_rows_f32 (include/openvoice_amd.h) on numpy arrays, records as tuples;
    writes float64 into ``dst``."""
    for so, base, end, total, t0, n_out, do, h_off, P, Q, taps in recs:
        if n_out <= 0 or do + n_out > dst.size:
            continue
        w = h[h_off:h_off + P * 2 * taps].reshape(P, 2 * taps)
        n_in = np.iinfo(np.int64).max // 4 if total < 0 else total
        n_res = n_in if total < 0 else total * P // Q
        t = np.arange(t0, t0 + n_out)
        live = t[t < n_res]
        y = np.zeros(n_out)
        if live.size:
            lo = max(0, int(live[0]) * Q // P - taps + 1)
            hi = min(n_in, int(live[-1]) * Q // P + taps + 1)
            if lo < hi and not (lo >= base and hi <= end and so + hi - base <= src.size):
                dst[do:do + n_out] = 0.0            # reads outside the valid window: zeros
                continue
            idx = (live * Q // P - taps + 1)[:, None] + np.arange(2 * taps)[None, :]
            ok = (idx >= 0) & (idx < n_in)
            xv = np.where(ok, src[np.clip(so + idx - base, 0, src.size - 1)], 0.0)
            y[:live.size] = (w[live % P] * xv).sum(axis=1)
        dst[do:do + n_out] = y


def _stream(x, sr_in, sr_out, pushes):
    """Drive one Schedule with ``pushes`` (sizes) and an end, keeping only its window between steps like the bank;
    returns the concatenated float64 output and the largest kept window."""
    h, P, Q, taps = audio_io.kaiser_best_phases(sr_in, sr_out)
    sch = rates.Schedule(sr_in, sr_out)
    win, outs, pos, biggest = np.zeros(0), [], 0, 0
    sizes = list(pushes) + [None]
    for n in sizes:
        new = x[pos:] if n is None else x[pos:pos + n]
        pos += new.size
        arena = np.concatenate([win, new])
        base, end, total, t0, n_out = sch.advance(new.size, end=n is None)
        assert end - base == arena.size
        y = np.full(n_out, np.nan)
        _run_records([(0, base, end, total, t0, n_out, 0, 0, P, Q, taps)], arena, h.reshape(-1), y)
        outs.append(y)
        win = arena[sch.base - base:]
        biggest = max(biggest, win.size)
    return np.concatenate(outs), biggest, taps


def _whole64(x, sr_in, sr_out):
    """The per-sample definition of the whole-file resampler in float64 (what ov_polyphase_fir_f32 computes)."""
    h, P, Q, taps = audio_io.kaiser_best_phases(sr_in, sr_out)
    n = -(-x.size * P // Q)
    y = np.full(n, np.nan)
    _run_records([(0, 0, x.size, x.size, 0, n, 0, 0, P, Q, taps)], x, h.reshape(-1), y)
    return y


def _push_sizes(rng, n, hi):
    out, acc = [], 0
    while acc < n:
        k = int(rng.choice([0, 1, 1, 2, int(rng.integers(0, hi))]))
        out.append(k)
        acc += k
    return out


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_streamed_schedule_equals_the_whole_file_resampler(sr_in, sr_out):
    rng = np.random.default_rng(sr_in + 7 * sr_out)
    n = 6000 + int(rng.integers(0, 500))
    x = rng.standard_normal(n) * 0.3
    ref = audio_io.resample_kaiser_best(x, sr_in, sr_out)
    whole = _whole64(x, sr_in, sr_out)
    assert whole.size == ref.size
    # float64 definition vs the vectorised host restatement (float32 result): one rounding apart
    assert np.abs(whole.astype(np.float32) - ref).max() <= 2 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max())
    for pushes in ([n], [1] * 300 + [n], _push_sizes(rng, n, 900), _push_sizes(rng, n, 40)):
        y, biggest, taps = _stream(x, sr_in, sr_out, pushes)
        assert y.shape == whole.shape and not np.isnan(y).any()
        assert np.abs(y - whole).max() <= 1e-12
        assert np.abs(y.astype(np.float32) - ref).max() <= 2 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max())
        assert biggest < 2 * taps          # kept between steps: from the next output's first tap on


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_latency_bound_holds_and_is_tight_for_one_sample_pushes(sr_in, sr_out):
    sch = rates.Schedule(sr_in, sr_out)
    bound = rates.latency_seconds(sr_in, sr_out)
    assert bound == Fraction(sch.taps, sr_in)
    worst = Fraction(-1)
    for a in range(4000):                      # input sample a arrives: the outputs it completes leave with it
        _, _, _, t0, n_out = sch.advance(1)
        for t in range(t0, t0 + n_out):
            delay = Fraction(a, sr_in) - Fraction(t, sr_out)
            assert delay <= bound
            worst = max(worst, delay)
    assert worst > bound - Fraction(1, sr_in)
    assert float(rates.latency_seconds(48000, 22050)) == pytest.approx(140 / 48000)
    assert float(rates.latency_seconds(22050, 48000)) == pytest.approx(65 / 22050)


def test_stream_latency_composition():
    core = 32060
    assert rates.stream_latency(core) == (Fraction(core, 22050), core)
    assert rates.stream_latency(core, 22050, 22050, 22050) == (Fraction(core, 22050), core)
    sec, n = rates.stream_latency(core, 22050, 48000, 48000)
    assert sec == Fraction(140, 48000) + Fraction(core + 65, 22050)
    assert n == -(-sec * 48000 // 1)
    sec, n = rates.stream_latency(core, 22050, 48000, None)
    assert sec == Fraction(140, 48000) + Fraction(core, 22050) and n == -(-sec * 22050 // 1)


def _emulating_call(log):
    """Stands in for _lib.call on the CPU: ov_polyphase_fir_rows_f32 by the float64 emulation, rounded to float32."""
    def call(name, *args):
        assert name == "ov_polyphase_fir_rows_f32", name
        table, n, src, src_elems, h, h_elems, dst, dst_elems, max_out = args
        recs = [tuple(r) for r in table.tolist()]
        assert len(recs) == n and src.numel() == src_elems and h.numel() == h_elems and dst.numel() == dst_elems
        assert max_out == max(r[5] for r in recs) and all(len(r) == rates.RECORD_FIELDS for r in recs)
        y = np.full(dst.numel(), np.nan)
        _run_records(recs, src.numpy().astype(np.float64), h.numpy(), y)
        written = np.zeros(dst.numel(), dtype=bool)
        for r in recs:
            assert not written[r[6]:r[6] + r[5]].any()       # destinations of one launch never overlap
            written[r[6]:r[6] + r[5]] = True
        dst[torch.from_numpy(written)] = torch.from_numpy(y[written]).float()
        log.append(len(recs))
    return call


def test_bank_issues_one_launch_per_step_for_any_mix_of_streams_and_pairs(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, "call", _emulating_call(log))
    bank = rates.ResamplerBank("cpu")
    rng = np.random.default_rng(3)
    streams = []
    for i in range(23):
        a, b = PAIRS[i % len(PAIRS)]
        x = (rng.standard_normal(3000 + 97 * i) * 0.3).astype(np.float32)
        streams.append(dict(key=bank.open(a, b), x=x, pos=0, out=[], pair=(a, b)))
    steps = 0
    while len(bank):
        for s in streams:
            if s["key"] not in bank or s["pos"] > s["x"].size:
                continue
            k = int(rng.choice([0, 1, 37, 441, 2205]))
            bank.push(s["key"], torch.from_numpy(s["x"][s["pos"]:s["pos"] + k]))
            s["pos"] += k
            if s["pos"] >= s["x"].size:
                bank.end(s["key"])
                s["pos"] = s["x"].size + 1
        before = len(log)
        res = bank.step()
        steps += 1
        assert len(log) - before <= 1
        for s in streams:
            if s["key"] in res:
                s["out"].append(res[s["key"]].numpy().copy())
    assert steps > 5 and len(log) <= steps
    for s in streams:
        got = np.concatenate(s["out"])
        ref = audio_io.resample_kaiser_best(s["x"], *s["pair"])
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 2 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max())


def test_resample_many_is_one_launch(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, "call", _emulating_call(log))
    rng = np.random.default_rng(4)
    xs = [torch.from_numpy((rng.standard_normal(2000 + 31 * i) * 0.3).astype(np.float32)) for i in range(len(PAIRS) + 1)]
    pairs = PAIRS + [(None, None)]
    outs = rates.resample_many(xs, pairs, "cpu")
    assert log == [len(PAIRS)]
    assert outs[-1] is xs[-1]
    for x, (a, b), y in zip(xs, PAIRS, outs):
        ref = audio_io.resample_kaiser_best(x.numpy(), a, b)
        assert y.shape == ref.shape and np.abs(y.numpy() - ref).max() <= 1e-6


# ---- a StreamPool with a fake model: one resampler launch per direction and step -------------------------------------
class _FakeModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.model_cfg = dict(CONVERTER_MODEL_CONFIG)
        self.p = torch.nn.Parameter(torch.zeros(1))


def test_stream_pool_step_issues_at_most_one_resampler_launch_per_direction(monkeypatch):
    log = []
    monkeypatch.setattr(_lib, "call", _emulating_call(log))
    monkeypatch.setattr(longform.WindowedConverter, "_launch_multi",
                        lambda self, pool, recs, Tw, s, t, tau, nz, out, stitch, n_out: out.zero_())
    conv = longform.WindowedConverter(_FakeModel(), window_frames=300, windows_per_launch=1)
    pool = conv.stream_pool(max_windows_per_launch=4)
    rng = np.random.default_rng(5)
    rates_ = [(48000, 48000), (8000, 16000), (44100, None), (None, 44100), (22050, 22050), (16000, 8000), (None, None)]
    hs, lens, pos, total = [], [], [], {}
    for i, (a, b) in enumerate(rates_ * 2):
        hs.append(pool.open(torch.zeros(1, 256, 1), torch.zeros(1, 256, 1), sr_in=a, sr_out=b))
        lens.append(int((a or 22050) * (4 + i % 5)))
        pos.append(0)
    steps = 0
    while pool.active:
        for i, h in enumerate(hs):
            if pos[i] < lens[i]:
                k = int(rng.integers(1, 6000))
                pool.push(h, torch.zeros(min(k, lens[i] - pos[i])))
                pos[i] += k
                if pos[i] >= lens[i]:
                    pool.close(h)
        before = len(log)
        for h, y in pool.step().items():
            total[h] = total.get(h, 0) + y.numel()
        steps += 1
        assert len(log) - before <= 2          # one launch for the input side, one for the output side
    assert steps > 10 and log
    for i, (a, b) in enumerate(rates_ * 2):
        # whole-file lengths: input resampled to the model rate, T frames converted, output resampled
        n22 = lens[i] if a in (None, 22050) else -(-lens[i] * 22050 // a)
        T = longform.stream_end_frames(n22, 1024, 256)
        n_out = T * 256 if b in (None, 22050) else -(-T * 256 * b // 22050)
        assert total[hs[i]] == n_out, (a, b)
    for a, b in [(None, None), (22050, 22050), (None, 22050)]:
        log.clear()
        p2 = conv.stream_pool(max_windows_per_launch=4)
        h = p2.open(torch.zeros(1, 256, 1), torch.zeros(1, 256, 1), sr_in=a, sr_out=b)
        p2.push(h, torch.zeros(22050 * 3))
        p2.close(h)
        p2.step()
        assert log == [] and not p2.active       # the model rate: no resampler runs


# ---- the entry point's host checks -----------------------------------------------------------------------------------
@lib_built
def test_rows_entry_point_is_exported_and_rejects_bad_host_arguments():
    lib = _lib.load()
    assert lib.ov_version() == 212 == _lib.MIN_VERSION        # an additive symbol of 2.12
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "openvoice_amd.h")).read()
    assert "int ov_polyphase_fir_rows_f32(" in header
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below fails validation before a launch
    f = lib.ov_polyphase_fir_rows_f32
    ok = (fake, 1, fake, 8, fake, 8, fake, 8, 4, None)
    for i, bad in [(0, None), (1, 0), (1, 65536), (1, -1), (2, None), (3, 0), (4, None), (5, 0), (6, None), (7, 0),
                   (8, 0), (8, -5)]:
        args = list(ok)
        args[i] = bad
        assert f(*args) == -1, (i, bad)


@lib_built
def test_torch_binding_of_the_rows_resampler_rejects_cpu_tensors():
    ops = _lib.torch_ops()
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.polyphase_fir_rows_f32(torch.zeros(1, 11, dtype=torch.long), 1, torch.zeros(8), 8,
                                   torch.zeros(8, dtype=torch.float64), 8, torch.zeros(8), 8, 4)


# ---- argument checks ---------------------------------------------------------------------------------------------------
BAD_RATES = [0, -8000, 44100.0, 22050.5, "48000", True]


@pytest.mark.parametrize("sr", BAD_RATES)
def test_bad_rates_raise(sr):
    with pytest.raises(ValueError):
        rates.check_rate(sr)
    with pytest.raises(ValueError):
        rates.ResamplerBank("cpu").open(sr, 22050)
    conv = longform.WindowedConverter(_FakeModel(), window_frames=300, windows_per_launch=1)
    pool = conv.stream_pool()
    for kw in (dict(sr_in=sr), dict(sr_out=sr)):
        with pytest.raises(ValueError):
            pool.open(torch.zeros(1, 256, 1), torch.zeros(1, 256, 1), **kw)
        with pytest.raises(ValueError):
            conv.stream(torch.zeros(1, 256, 1), torch.zeros(1, 256, 1), **kw)
    assert not pool.active
    assert rates.check_rate(np.int64(16000)) == 16000 and rates.check_rate(None) is None


class _FakeEngine:
    _bf16_on = _split3_on = False
    device = torch.device("cpu")


class _FakeLiveModel:
    model_cfg = CONVERTER_MODEL_CONFIG

    def engine(self):
        return _FakeEngine()


@pytest.mark.parametrize("sr", BAD_RATES)
def test_bad_rates_raise_at_live_pool_open(sr):
    from openvoice_amd import live
    pool = live.LivePool(_FakeLiveModel(), chunk_frames=15)
    for kw in (dict(sr_in=sr), dict(sr_out=sr)):
        with pytest.raises(ValueError):
            pool.open(torch.zeros(1, 256, 1), torch.zeros(1, 256, 1), **kw)
    assert not pool.active and pool.mem is None
