"""Host side of streaming synthesis (openvoice_amd/tts_live.py): the unit table, ``first_audio_frames``, the cascade and
arena bookkeeping of a ``TtsLivePool`` (run with its launches stubbed out), the feed records and the gap plan."""
import types

import pytest
import torch

from openvoice_amd import clone, live, tts_live
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG

SPF = 256


def test_unit_table_is_live_units_without_q_and_f():
    units = tts_live.tts_units(CFG)
    assert [u["name"] for u in units] == ["r", "g0", "g1", "g2", "g3"]
    by_name = {u["name"]: u for u in live.live_units(CFG)}
    for u in units:
        assert u == by_name[u["name"]]
        for field in ("left", "right", "rate", "stride", "align", "history"):
            assert u[field] == by_name[u["name"]][field]


@pytest.mark.parametrize("chunk", [15, 60])
def test_first_audio_frames_is_what_a_cascade_needs(chunk):
    units = tts_live.tts_units(CFG)
    cas, fed = live.Cascade(units, chunk), 0
    while True:
        pieces = cas.round(chunk)
        fed += chunk
        if any(k == len(units) - 1 for k, *_ in pieces):
            break
    assert tts_live.first_audio_frames(CFG, chunk) == fed
    # one frame less than the need cannot emit: the need is exact, not only its chunk rounding
    need = tts_live.first_audio_need(units)
    for n, emits in ((need - 1, False), (need, True)):
        cas = live.Cascade(units, 15 * 100)
        assert any(k == len(units) - 1 for k, *_ in cas.round(n)) == emits
    with pytest.raises(ValueError):
        tts_live.first_audio_frames(CFG, 16)


class HostPool(tts_live.TtsLivePool):
    """The pool's real bookkeeping with every launch stubbed: carries are checked against the arena and replayed as
    coverage counts, the units do nothing."""

    def __init__(self, chunk, M=4):
        core = types.SimpleNamespace(device=torch.device("cpu"), _bf16_on=False, _split3_on=False)
        eng = types.SimpleNamespace(core=core, n_vocab=68, n_speakers=10)
        super().__init__(types.SimpleNamespace(model_cfg=dict(CFG), engine=lambda: eng), chunk_frames=chunk,
                         max_streams_per_launch=M)
        self.tok_cap = 64
        self.emitted = {}

    def _launch(self, k, rows, B, L):
        assert L <= self.width[k]

    def _carry(self, recs, dst=None):
        n_dst = self.mem.numel() if dst is None else dst.numel()
        for src, d, rows, cols, sld, dld in recs:
            assert rows >= 1 and cols >= 1 and src >= 0 and d >= 0
            assert src + (rows - 1) * sld + cols <= self.mem.numel()
            assert d + (rows - 1) * dld + cols <= n_dst

    def admit(self, h, T):
        self._pending.remove(h)
        self._streams[h].T = self.frames[h] = T
        self._streams[h].conds = {}

    def run(self):
        """Rounds to the end -> ({handle: samples}, every feed record)."""
        out, records = {}, []
        while self._streams:
            live_before = dict(self._streams)
            jobs, plans = self._plan_round()
            recs = self._feed_records(jobs)
            assert len(recs) == len(jobs) and all(len(r) == tts_live.RECORD_FIELDS for r in recs)
            records += [(st, r) for (st, _, _), r in zip(jobs, recs)]
            for h, o in self._run_units(plans).items():
                out[h] = out.get(h, 0) + o.numel()
            for h, st, _ in plans:
                if st.cas.done:
                    self._free_slots.append(self._streams.pop(h).slot)
            assert plans, live_before
        return out, records


FAF = {c: tts_live.first_audio_frames(CFG, c) for c in (15, 60)}


@pytest.mark.parametrize("chunk", [15, 60])
def test_bookkeeping_reaches_done_with_every_column_once(chunk):
    lengths = sorted({1, chunk - 1, chunk, chunk + 1, FAF[chunk] - 1, FAF[chunk] + 1, 301})
    units = tts_live.tts_units(CFG)
    for T in lengths:
        cas, spans, fed = live.Cascade(units, chunk), [[] for _ in units], 0
        for _ in range(10 * (T // chunk + 10)):
            nf = min(chunk, T - fed)
            for k, b0, end, e0, e1 in cas.round(nf, final=fed + nf == T):
                assert 0 <= b0 <= e0 < e1 <= end <= cas.n[k] and end - b0 <= cas.width(k)
                spans[k].append((e0, e1))
            fed += nf
            if cas.done:
                break
        assert cas.done, T
        for k, u in enumerate(units):                  # every column of every unit exactly once, in order
            assert spans[k][0][0] == 0 and spans[k][-1][1] == T * u["rate"]
            assert all(a[1] == b[0] for a, b in zip(spans[k], spans[k][1:]))
    pool = HostPool(chunk)
    hs = [pool.open([1, 2, 3], 1) for _ in lengths]
    for h, T in zip(hs, lengths):
        pool.admit(h, T)
    out, _ = pool.run()
    assert out == {h: T * SPF for h, T in zip(hs, lengths)}


def test_feed_records_stay_inside_the_arena():
    pool = HostPool(15, M=2)
    hs = [pool.open(list(range(1, 4 + i)), i, seed=(7, i)) for i in range(5)]
    for h, T in zip(hs, (1, 44, 46, 150, 301)):
        pool.admit(h, T)
    sts = dict(pool._streams)
    _, records = pool.run()
    assert len(records) >= 301 // 15
    C, cap = pool.inter, pool.tok_cap
    seen = {}
    for st, (seed, stream, f0, nf, x_len, y_len, m_off, m_ld, l_off, l_ld, c_off, d_off, d_ld) in records:
        assert (seed, stream) == st.seed and x_len == st.Tx and y_len == st.T
        assert f0 == seen.get(st, 0) and 1 <= nf <= 15 and f0 + nf <= y_len
        seen[st] = f0 + nf
        assert m_ld == l_ld == cap >= x_len and l_off == m_off + C * cap and m_off == st.slot * 2 * C * cap
        assert c_off == st.slot * cap and l_off + (C - 1) * cap + x_len <= pool._slots * 2 * C * cap
        lo = pool.arena_off + st.slot * pool.slot_elems + pool.state_off[0]           # unit r's two state halves
        assert d_ld == pool.cap[0] and nf <= d_ld
        assert lo <= d_off and d_off + (C - 1) * d_ld + nf <= lo + 2 * C * pool.cap[0] <= pool.mem.numel()
        half = (d_off - lo) // (C * pool.cap[0])
        assert (d_off - lo) % pool.cap[0] + nf <= pool.cap[0] and half in (0, 1)
    assert {st.T for st in sts.values()} == set(seen.values())


def test_gap_and_sentence_plan_is_join_plan():
    counts = [3 * SPF, 1 * SPF, 40 * SPF]
    for speed in (1.0, 1.3):
        recs, total = tts_live.stream_plan(counts, 22050, speed)
        want, totals = clone.join_plan([counts], clone.gap_samples(22050, speed))
        assert recs == want[0] and total == totals[0]
        gap = int(22050 * 0.05 / speed)
        assert [r[2] for r in recs] == [gap] * 3 and total == sum(counts) + 3 * gap


def test_stream_sentences_yields_sentences_then_gaps_in_order():
    """The generator behind tts_stream_from_ids over the stubbed pool: chunk counts and gaps follow stream_plan."""
    pool = HostPool(15)
    lengths = [50, 7, 120]
    real_open = pool.open

    def open_and_admit(ids, speaker, **kw):
        h = real_open(ids, speaker, **kw)
        pool.admit(h, lengths[h])
        return h

    def step():
        jobs, plans = pool._plan_round()
        pool._feed_records(jobs)
        out = pool._run_units(plans)
        for h, st, _ in plans:
            if st.cas.done:
                pool._free_slots.append(pool._streams.pop(h).slot)
                pool.frames_fed.pop(h), pool.frames.pop(h)
        return out

    pool.open, pool.step = open_and_admit, step
    chunks = list(tts_live.stream_sentences(pool, [[1, 2], [3], [4, 5, 6]], 1, 1.3, 0.667, 0.6, 11, 22050))
    recs, total = tts_live.stream_plan([T * SPF for T in lengths], 22050, 1.3)
    assert sum(c.numel() for c in chunks) == total
    sizes, at = [c.numel() for c in chunks], 0
    for n, off, gap in recs:                          # a sentence's chunks end exactly where its gap starts
        acc = 0
        while acc < n:
            acc += sizes[at]
            at += 1
        assert acc == n and sizes[at] == gap and not chunks[at].any()
        at += 1
    assert at == len(sizes)
    assert pool._next == 3 and not pool._streams
