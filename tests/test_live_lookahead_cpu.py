"""Live streams with bounded look-ahead (openvoice_amd/live.py, ``lookahead_frames=``), host side: the emission schedule,
the back-propagated preview ranges, the latency bound and the argument checks.  No GPU."""
import pytest

from openvoice_amd import live
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG as CFG

HOP, NFFT = 256, 1024
UNITS = live.live_units(CFG)
REACH = live.live_right_samples(CFG)


@pytest.mark.parametrize("A", [0, 15, 45, 100, 110])
def test_schedule_is_monotone_and_follows_the_frames_taken(A):
    sch = live.lookahead_schedule(UNITS, 15, A, 0, 20)
    assert [r["F"] for r in sch] == [15 * (i + 1) for i in range(20)]
    prev = 0
    for r in sch:
        assert r["E"] == HOP * max(0, r["F"] - A) and r["E0"] == prev <= r["E"]
        assert r["C"] == max(0, HOP * r["F"] - REACH)
        prev = r["E"]


def _covered(plan, lo, hi, n, e):
    """Walks a plan forwards: every unit's buffer is made of stored columns and of what the unit before hands on, keeps
    its reaches inside the buffer (or at an end of the input), and the last unit hands on [lo, hi)."""
    assert [p[0] for p in plan] == list(range(plan[0][0], len(UNITS)))
    have = None                                   # columns of the current unit's input the unit before handed on
    for k, b0, end, olo, ohi in plan:
        u = UNITS[k]
        total = n[0] * u["rate"]
        assert 0 <= b0 < end <= total and b0 % u["align"] == 0
        if have is None:
            assert end <= n[k]                    # the first unit of a plan runs on stored columns only
        else:
            assert have == (max(b0, n[k]), end)
        s = u["stride"]
        pe0, pe1 = olo // s, -(-ohi // s)
        assert pe0 >= e[k] and (b0 == 0 or pe0 - b0 >= u["left"]) and (end == total or end - pe1 >= u["right"])
        assert b0 >= live._start(u, e[k])         # nothing before what the stream still stores
        have = (olo, ohi)
    assert have == (lo, hi)


@pytest.mark.parametrize("chunk", [15, 60])
@pytest.mark.parametrize("A", [0, 15, 45])
def test_preview_ranges_cover_the_piece_and_the_crossfade(chunk, A):
    X = min(HOP, HOP * A)
    cas = live.Cascade(UNITS, chunk)
    sch = live.lookahead_schedule(UNITS, chunk, A, X, 12)
    widths = live.preview_widths(UNITS, chunk, A, X)
    for r in sch:
        cas.round(chunk)
        if r["E"] <= max(r["C"], r["E0"]):
            assert r["plan"] is None
            continue
        assert r["lo"] == max(r["C"], r["E0"]) and r["hi"] == r["E"] + X <= HOP * r["F"]
        _covered(r["plan"], r["lo"], r["hi"], cas.n, cas.e)
        assert all(end - b0 <= widths[k] for k, b0, end, _, _ in r["plan"])
    assert any(r["plan"] for r in sch)


def test_no_preview_is_planned_past_the_reach():
    A = -(-REACH // HOP)
    assert A == 109 and HOP * A >= REACH
    for chunk in (15, 60):
        assert all(r["plan"] is None for r in live.lookahead_schedule(UNITS, chunk, A, HOP, 30))
        assert live.preview_widths(UNITS, chunk, A, HOP) == [0] * len(UNITS)
    assert any(r["plan"] for r in live.lookahead_schedule(UNITS, 15, A - 1, HOP, 30))


@pytest.mark.parametrize("A", [0, 15])
@pytest.mark.parametrize("chunk", [15, 60])
def test_latency_bound_is_the_largest_delay_of_the_schedule(A, chunk):
    """Sample by sample: with n samples arrived the stream has taken ``chunk * (interior_frames(n) // chunk)`` frames and
    emitted ``hop * max(0, F - A)`` samples; the bound is the largest ``n - t`` over samples t at the moment they leave."""
    lat = live.live_latency_samples(CFG, chunk, NFFT, HOP, lookahead_frames=A)
    worst, out_before = 0, 0
    for n in range(1, HOP * (A + 6 * chunk)):
        F = live.interior_frames(n, NFFT, HOP) // chunk * chunk
        out = HOP * max(0, F - A)
        if out > out_before:
            worst = max(worst, n - out_before)        # the oldest sample of the piece waited longest
            out_before = out
        assert out >= n - lat + 1
    assert worst == lat == HOP * (A + chunk) + (NFFT - HOP) // 2
    if chunk == 15:
        assert lat <= {0: 0.2, 15: 0.37}[A] * 22050
        assert 4 * live.live_latency_samples(CFG, 15, lookahead_frames=0) < live.live_latency_samples(CFG, 15)


def test_argument_validation():
    for bad in (-1, 1.0, True, "3"):
        with pytest.raises(ValueError):
            live.check_lookahead(bad)
        with pytest.raises(ValueError):
            live.live_latency_samples(CFG, 15, lookahead_frames=bad)
    assert live.check_lookahead(None) is None and live.check_lookahead(0) == 0
    assert live.check_crossfade(None, None, 15) == 0
    assert live.check_crossfade(None, 0, 15) == 0 and live.check_crossfade(None, 15, 15) == HOP
    assert live.check_crossfade(15 * HOP, 15, 15) == 15 * HOP and live.check_crossfade(HOP, 1, 60) == HOP
    for X, A in ((1, 0), (HOP + 1, 1), (15 * HOP + 1, 45), (-1, 15), (2.0, 15), (True, 15)):
        with pytest.raises(ValueError):
            live.check_crossfade(X, A, 15)
    with pytest.raises(ValueError):
        live.check_crossfade(4, None, 15)
    w = live.crossfade_weights(256)
    assert w.shape == (256,) and 0 < w[0] < w[127] < 0.5 < w[128] < w[255] < 1
    assert abs(float(w[127]) + float(w[128]) - 1) < 1e-6


def test_streaming_tts_and_cloned_speech_refuse_the_keyword_at_the_call():
    """Out of scope for look-ahead: ``TtsLivePool``, ``BaseSpeakerTTS.tts_live_pool`` and ``VoiceCloner.speak_stream*``
    raise ValueError naming the keyword -- at the call (``speak_stream_ids`` returns a generator, the check does not wait
    for its first ``next``) and before anything of the object is touched."""
    from types import SimpleNamespace
    from openvoice_amd import api, clone, tts_live
    with pytest.raises(ValueError, match="lookahead_frames"):
        tts_live.TtsLivePool(None, lookahead_frames=0)
    with pytest.raises(ValueError, match="lookahead_frames"):
        api.BaseSpeakerTTS.tts_live_pool(SimpleNamespace(model=None), lookahead_frames=15)
    with pytest.raises(ValueError, match="lookahead_frames"):
        clone.VoiceCloner.speak_stream_ids(None, [[1, 2]], 0, None, None, lookahead_frames=0)
    tts = SimpleNamespace(text_to_ids=lambda text, language: [[1, 2]])
    me = SimpleNamespace(tts=tts)
    me.speak_stream_ids = lambda *a, **kw: clone.VoiceCloner.speak_stream_ids(me, *a, **kw)
    with pytest.raises(ValueError, match="lookahead_frames"):
        clone.VoiceCloner.speak_stream(me, "hello", 0, None, None, lookahead_frames=0)


def test_a_generator_buffer_that_is_no_whole_number_of_vectors_is_refused():
    """The fp32 MRF kernels of the stride-2 stages have vector instances only: a preview buffer there is made even, and
    one that cannot be (it ends with the input, and ``align`` is odd) is refused on the host instead of reaching them."""
    units = [dict(u) for u in UNITS]
    cas = live.Cascade(units, 15)
    for _ in range(10):
        cas.round(15)
    for A in range(0, 109, 7):
        for rec in live.lookahead_schedule(UNITS, 15, A, min(HOP, HOP * A), 40):
            for k, b0, end, _, _ in rec["plan"] or []:
                assert UNITS[k]["kind"] != "g" or (end - b0) * UNITS[k]["stride"] % 4 == 0
    units[-1]["align"] = 1                           # an odd grid on the last (stride 2) stage
    E = HOP * cas.n[0]
    with pytest.raises(ValueError, match="16-byte"):
        for lo in range(E - 3840, E - 3830):
            live.preview_plan(units, cas.n, cas.e, lo, E)
