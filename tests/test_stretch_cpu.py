"""``speed=`` / ``duration=`` without a GPU (openvoice_amd/stretch.py): the mirror against brute force, the arguments, the
window context of a stretched long recording against the generator's reach, and the streams that refuse the keywords."""
import inspect
import pathlib
import re

import numpy as np
import pytest

from openvoice_amd import _lib, api, clone, longform, stretch
from openvoice_amd.generator import GENERATOR_MARGIN, generator_margin_frames
from openvoice_amd.utils import CONVERTER_MODEL_CONFIG

ROOT = pathlib.Path(__file__).resolve().parents[1]
ONE = stretch.ONE
SPEEDS = [0.5, 0.55, 0.75, 0.999, 1.0, 1.001, 1.37, 1.5, 1.999, 2.0]


# ---- the mirror ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_in", [1, 2, 17, 861])
def test_t_out_is_the_brute_force_count_and_positions_are_in_range(T_in):
    for speed in SPEEDS:
        step = stretch.step_of(speed)
        assert step == int(round(speed * 2 ** 32))
        count = 0
        while (count * step) >> 32 <= T_in - 1:          # every j whose source frame exists
            count += 1
        assert stretch.t_out(T_in, step) == count, (T_in, speed)
        i, f = stretch.positions(0, count, step)
        assert i[0] == 0 and np.all(np.diff(i) >= 0) and i[-1] <= T_in - 1
        assert f.dtype == np.float32 and np.all(f >= 0) and np.all(f < 1)
        assert ((count * step) >> 32) > T_in - 1           # the next one would not
        # f carries 24 bits: exact in fp32
        pos = np.arange(count, dtype=np.int64) * step
        assert np.array_equal(f.astype(np.float64) * 2.0 ** 24, ((pos & 0xffffffff) >> 8).astype(np.float64))
        assert stretch.first_output_at(T_in, step) == count


def test_speed_one_is_the_identity():
    z = np.random.default_rng(0).standard_normal((3, 17)).astype(np.float32)
    assert stretch.step_of(1.0) == ONE and stretch.t_out(17, ONE) == 17
    assert np.array_equal(stretch.stretch_rows(z, ONE), z)


def test_the_mirror_interpolates_and_clamps_at_the_end():
    z = np.arange(10, dtype=np.float32)[None] * 4.0
    out = stretch.stretch_rows(z, stretch.step_of(0.5))
    assert out.shape == (1, 20)
    assert np.array_equal(out[0, :19], np.arange(19, dtype=np.float32) * 2.0) and out[0, 19] == 36.0      # clamped
    out = stretch.stretch_rows(z, stretch.step_of(2.0))
    assert np.array_equal(out[0], z[0, ::2])


@pytest.mark.parametrize("speed", [0.5, 0.75, 1.37, 2.0])
def test_a_window_computes_the_slice_of_the_whole(speed):
    rng = np.random.default_rng(3)
    T = 65
    z = rng.standard_normal((5, T)).astype(np.float32)
    step = stretch.step_of(speed)
    whole = stretch.stretch_rows(z, step)
    for lo, hi in [(20, 45), (0, 30), (40, 65), (64, 65)]:
        j_lo, j_hi = stretch.first_output_at(lo, step), stretch.first_output_at(hi, step)
        if j_hi == j_lo:
            continue
        a, b = max(0, lo - 3), min(T, hi + 3)               # a slice with context: column 0 is global frame a
        win = stretch.stretch_rows(z[:, a:b], step, T_in=T, i0=a, j0=j_lo, n_out=j_hi - j_lo)
        assert np.array_equal(win, whole[:, j_lo:j_hi]), (speed, lo, hi)
    with pytest.raises(ValueError):                         # a slice that ends before the neighbour of its last frame
        j_lo, j_hi = stretch.first_output_at(20, step), stretch.first_output_at(45, step)
        stretch.stretch_rows(z[:, 20:44], step, T_in=T, i0=20, j0=j_lo, n_out=j_hi - j_lo)


def test_check_record_mirrors_the_kernel_checks():
    step = stretch.step_of(0.75)
    n = stretch.t_out(17, step)
    good = stretch.record(5, 3, 3, 20, 24, 17, 0, 0, n, step)
    assert stretch.check_record(good, 5 + 2 * 20 + 17, 3 + 2 * 24 + n)
    assert not stretch.check_record(good, 5 + 2 * 20 + 16, 3 + 2 * 24 + n)          # beyond the source extent
    assert not stretch.check_record(good, 5 + 2 * 20 + 17, 3 + 2 * 24 + n - 1)      # beyond the destination extent
    big = 1 << 20
    assert not stretch.check_record(stretch.record(0, 0, 3, 20, 24, 17, 0, 0, n + 1, step), big, big)    # i past t_in - 1
    assert not stretch.check_record(stretch.record(0, 0, 3, 20, 24, 17, 1, 0, n, step), big, big)        # negative reach
    assert not stretch.check_record(stretch.record(0, 0, 3, 16, 24, 17, 0, 0, n, step), big, big)        # ld < t_in
    assert not stretch.check_record(stretch.record(0, 0, 3, 20, 24, 17, 0, 0, n, ONE // 2 - 1), big, big)
    assert not stretch.check_record(stretch.record(-1, 0, 3, 20, 24, 17, 0, 0, n, step), big, big)
    assert not stretch.check_record(stretch.record(0, 0, 0, 20, 24, 17, 0, 0, n, step), big, big)


# ---- arguments -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0.49, 2.01, 0, -1.0, float("nan"), float("inf"), "1.0", True, [1.0]])
def test_speed_outside_the_range_is_a_value_error(bad):
    with pytest.raises(ValueError):
        stretch.step_of(bad)


def test_the_range_ends_are_accepted():
    assert stretch.step_of(0.5) == ONE // 2 and stretch.step_of(2.0) == 2 * ONE


def test_speed_and_duration_together_are_a_value_error():
    with pytest.raises(ValueError, match="one of them"):
        stretch.resolve(1.2, 3.0, 100, 256, 22050)
    assert stretch.resolve(None, None) is None
    with pytest.raises(ValueError):
        stretch.resolve_items([1.2, None], [None, 2.0, 3.0], [100, 100], 256, 22050)
    with pytest.raises(ValueError):                          # item 0 carries both
        stretch.resolve_items([1.2, None], [3.0, 2.0], [100, 100], 256, 22050)
    for bad in (0, -2.0, float("nan"), "3"):
        with pytest.raises(ValueError):
            stretch.resolve(None, bad, 100, 256, 22050)


def test_per_item_lists():
    assert stretch.resolve_items(None, None, [10, 20], 256, 22050) is None
    assert stretch.resolve_items([None, None], None, [10, 20], 256, 22050) is None
    assert stretch.resolve_items(1.5, None, [10, 20], 256, 22050) == [stretch.step_of(1.5)] * 2
    assert stretch.resolve_items([None, 0.75], None, [10, 20], 256, 22050) == [ONE, stretch.step_of(0.75)]
    assert stretch.resolve_items(np.array([1.0, 2.0]), None, [10, 20], 256, 22050) == [ONE, 2 * ONE]
    for bad in ([1.0], [1.0, 1.0, 1.0], ()):
        with pytest.raises(ValueError, match="one per item"):
            stretch.resolve_items(bad, None, [10, 20], 256, 22050)
    with pytest.raises(ValueError, match="one per item"):
        stretch.resolve_items(None, [2.0], [10, 20], 256, 22050)
    with pytest.raises(ValueError):
        stretch.resolve_items([1.0, 2.5], None, [10, 20], 256, 22050)


@pytest.mark.parametrize("T_in,duration", [(861, 10.0), (861, 7.3), (861, 19.9), (17, 0.2), (300, 2.0), (5168, 45.0)])
def test_duration_round_trip_is_within_one_hop(T_in, duration):
    hop, sr = 256, 22050
    step = stretch.resolve(None, duration, T_in, hop, sr)
    samples = stretch.t_out(T_in, step) * hop
    assert abs(samples - duration * sr) <= hop, (samples, duration * sr)
    with pytest.raises(ValueError):
        stretch.resolve(None, T_in * hop / sr / 2.2, T_in, hop, sr)          # would need speed 2.2


# ---- the window context of a stretched long recording -----------------------------------------------------------------------
@pytest.mark.parametrize("speed", [0.5, 1.0, 2.0, 0.75, 1.37])
def test_widened_context_covers_the_generators_reach(speed):
    """Pure integers.  For every window of a plan cut with ``stretch_context_frames``: the generator's input, output frames
    ``[ja, ja + n)``, reads (with the neighbour ``i + 1``) only source frames on which the window's latent is exact --
    ``frame_reach`` frames from a window edge that is not a file edge -- and it holds ``M = max(GENERATOR_MARGIN,
    generator_margin_frames(cfg))`` output frames beyond every core edge that is not a file edge; the emitted ranges
    partition ``[0, T_out)``; the first window starts at 0 and the last ends at ``T_out``."""
    cfg = CONVERTER_MODEL_CONFIG
    step = stretch.step_of(speed)
    R, M, grid = longform.frame_reach_frames(), longform.generator_context_frames(cfg), longform.winograd_grid_frames(cfg)
    assert R == 96 and M == max(GENERATOR_MARGIN, generator_margin_frames(cfg)) and M >= generator_margin_frames(cfg)
    ctx = longform.stretch_context_frames(cfg, step)
    assert ctx % grid == 0 and ctx >= longform.context_frames(cfg)
    assert ctx >= R + M * max(1.0, speed) + 1               # the reach itself, in source frames, and the neighbour
    if speed <= 1.0:
        assert ctx == longform.context_frames(cfg) == 120
    for T, Tw in [(300, 2 * ctx + grid), (1000, 2 * ctx + 4 * grid), (5168, 1024), (1025, 1024), (2047, 1024), (700, 1024)]:
        plan = longform.plan_windows(T, Tw, ctx, grid)
        splan = stretch.plan_windows(plan, T, Tw, step, R, M)
        To = stretch.t_out(T, step)
        twin = min(T, Tw)
        nxt = 0
        if T > Tw:
            assert len(plan) >= 2
        for (f0, lo, hi), (ja, n, j_lo, j_hi) in zip(plan, splan):
            assert j_lo == nxt and j_hi > j_lo
            nxt = j_hi
            i, _ = stretch.positions(j_lo, j_hi - j_lo, step)
            assert lo <= i[0] and i[-1] < hi                                     # emits the frames whose i is in its core
            assert ja <= max(0, j_lo - M) and ja + n >= min(To, j_hi + M) and ja >= 0 and ja + n <= To
            assert (ja == 0) == (f0 == 0) or ja > 0
            if f0 == 0:
                assert ja == 0
            if f0 + twin == T:
                assert ja + n == To
            i, _ = stretch.positions(ja, n, step)
            first, last = int(i[0]), min(int(i[-1]) + 1, T - 1)
            assert first >= (f0 + R if f0 > 0 else 0), (T, Tw, f0)
            assert last <= (f0 + twin - R - 1 if f0 + twin < T else T - 1), (T, Tw, f0)
            assert stretch.check_record(stretch.record(0, 0, 192, twin, n, twin, f0, ja, n, step), 192 * twin, 192 * n)
        assert nxt == To
        # regular windows share one shape
        regular = {n for (f0, lo, hi), (ja, n, _, _) in zip(plan, splan) if f0 > 0 and hi < T}
        assert len(regular) <= 1
    if speed == 2.0:                                         # a context that ignores the speed does not serve it
        small = longform.context_frames(cfg)
        with pytest.raises(ValueError, match="cannot serve its core"):
            stretch.plan_windows(longform.plan_windows(5168, 1024, small, grid), 5168, 1024, step, R, M)


# ---- the public surface ----------------------------------------------------------------------------------------------------
def test_keywords_are_keyword_only_and_default_to_none():
    T = api.ToneColorConverter
    for name, keys in [("convert", ("speed", "duration")), ("convert_batch", ("speed",)),
                       ("convert_many", ("speed", "duration")), ("convert_long", ("speed", "duration"))]:
        params = inspect.signature(getattr(T, name)).parameters
        for k in keys:
            assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None, (name, k)


def test_cloner_requests_carry_convert_speed_to_convert_many(monkeypatch):
    """The dict key and the eighth tuple entry both become the request's step, range-checked by ``step_of`` at the call;
    ``speak_ids_many`` hands the steps (``ONE`` for a request without one) to ``WindowedConverter.convert_many``."""
    import torch
    cloner = object.__new__(clone.VoiceCloner)
    ids = [[1, 2, 3]]
    reqs = cloner._parse([dict(ids=ids, speaker=0, src_se="s", tgt_se="t", speed=1.2, convert_speed=0.75),
                          (ids, 0, "s", "t", 1.0, None, None, 1.5),
                          (ids, 0, "s", "t", 0.9),
                          (ids, 0, "s", "t", 1.0, None, None, None)], None, None, None, None)
    assert [r.convert_step for r in reqs] == [stretch.step_of(0.75), stretch.step_of(1.5), None, None]
    assert [r.speed for r in reqs] == [1.2, 1.0, 0.9, 1.0]                      # the TTS speed is another thing
    for bad in (2.5, 0.1, "fast", True):
        with pytest.raises(ValueError):
            cloner._parse([(ids, 0, "s", "t", 1.0, None, None, bad)], None, None, None, None)
        with pytest.raises(ValueError):
            cloner._parse([dict(ids=ids, speaker=0, src_se="s", tgt_se="t", convert_speed=bad)], None, None, None, None)
    with pytest.raises(ValueError):
        cloner._parse([(ids, 0, "s", "t", 1.0, None, None, 1.5, "extra")], None, None, None, None)

    seen = {}

    class Windowed:
        def convert_many(self, waves, srcs, tgts, **kw):
            seen.update(kw, n=len(waves))
            return waves

    class Converter:
        device, hps = "cpu", type("H", (), {"data": type("D", (), {"sampling_rate": 22050})})()
        _windowed = lambda self, *a: Windowed()
        _finish_many = lambda self, outs, message, out_srs: [o.numpy() for o in outs]
        _wavenet_cores = lambda self: ()

    cloner.converter, cloner.tts_sr, cloner.device = Converter(), 22050, "cpu"
    cloner.tts = type("T", (), {"_wavenet_cores": lambda self: ()})()
    monkeypatch.setattr(clone.VoiceCloner, "synthesize_many", lambda self, reqs, *a, **k: [torch.zeros(8)] * len(reqs))
    monkeypatch.setattr(clone.rates, "resample_many", lambda waves, pairs, device: waves)
    cloner.speak_ids_many([(ids, 0, "s", "t", 1.0, None, None, 0.75), (ids, 0, "s", "t")])
    assert seen["n"] == 2 and seen["steps"] == [stretch.step_of(0.75), ONE]
    seen.clear()
    cloner.speak_ids_many([(ids, 0, "s", "t"), (ids, 0, "s", "t")])
    assert "steps" not in seen                                                  # no request asks: today's call


def test_convert_routes_on_the_longer_of_input_and_output(monkeypatch):
    """The generator runs on ``T_out`` frames, so a file that only the stretch takes past the one-pass limit goes to
    ``convert_long`` with its keywords, like a file that is over-length itself."""
    import torch
    from openvoice_amd import audio_io
    from openvoice_amd.utils import default_converter_hparams
    conv = object.__new__(api.ToneColorConverter)
    conv.watermark_model, conv.device = None, "cpu"
    conv.hps = default_converter_hparams("v2")
    conv.model = type("M", (), {"model_cfg": CONVERTER_MODEL_CONFIG})()
    limit = longform.one_pass_limit_frames(CONVERTER_MODEL_CONFIG)
    T = limit // 2 + 200                                     # half the limit: one pass unless slowed down
    wave = torch.empty(256 * T)
    assert longform.frames_of(wave.numel(), 1024, 256) == T
    monkeypatch.setattr(audio_io, "load_to_device", lambda path, sr, device: wave)
    calls = []
    monkeypatch.setattr(api.ToneColorConverter, "convert_long", lambda self, y, *a, **kw: calls.append(("long", kw)))
    monkeypatch.setattr(api.ToneColorConverter, "convert_batch",
                        lambda self, y, *a, **kw: (calls.append(("batch", kw)), (torch.zeros(1, 1, 4), torch.tensor([4])))[1])
    conv.convert("x.wav", None, None, speed=0.5)
    conv.convert("x.wav", None, None, duration=T * 256 / 22050 * 1.99)
    conv.convert("x.wav", None, None, speed=1.5)
    conv.convert("x.wav", None, None)
    assert [c[0] for c in calls] == ["long", "long", "batch", "batch"]
    assert calls[0][1]["speed"] == 0.5 and "duration" in calls[1][1] and calls[2][1]["speed"] == 1.5
    assert "speed" not in calls[3][1]


def test_record_check_does_not_rely_on_wrap_around():
    """A ``j0`` near 2^63 must not pass by overflowing ``j0 + n_out`` (the host check of the C entry point and the Python
    mirror agree on it)."""
    import ctypes
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    step = stretch.step_of(0.75)
    for j0 in ((1 << 63) - 1, (1 << 63) - 20, (1 << 62), (1 << 29)):
        rec = stretch.record(0, 0, 3, 20, 24, 17, 0, j0, 22, step)
        assert not stretch.check_record(rec, 1000, 1000)
        assert lib.ov_stretch_rows_f32(p, (ctypes.c_int64 * 10)(*rec), 1, p, 1000, p, 1000, None) != 0


def test_streams_and_pools_reject_the_keywords():
    conv = object.__new__(api.ToneColorConverter)           # the check comes first: no attribute of the object is touched
    for call in (lambda **kw: conv.stream(None, None, **kw), lambda **kw: conv.live_stream(None, None, **kw),
                 lambda **kw: conv.stream_pool(**kw), lambda **kw: conv.live_pool(**kw)):
        for kw in ({"speed": 1.2}, {"duration": 3.0}, {"speed": 1.0}):
            with pytest.raises(ValueError, match="streams and pools"):
                call(**kw)


def test_convert_checks_the_arguments_before_it_loads_anything():
    conv = object.__new__(api.ToneColorConverter)
    conv.watermark_model = None
    with pytest.raises(ValueError, match="one of them"):
        conv.convert("no-such-file.wav", None, None, speed=1.2, duration=2.0)
    with pytest.raises(TypeError):
        conv.convert_batch([], None, None, 0.3, None, None, 1.2)             # keyword only


def test_abi_surface():
    header = (ROOT / "include" / "openvoice_amd.h").read_text()
    assert re.search(r"\bint ov_stretch_rows_f32\(", header) and "ov_stretch_rows_f32" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ov_stretch_rows_f32"][1]) == 8
    assert "stretch.hip" in (ROOT / "openvoice_amd" / "csrc" / "Makefile").read_text()
    lib = _lib.load()
    assert hasattr(_lib.torch_ops(), "stretch_rows_f32")
    import ctypes
    p = ctypes.c_void_p(64)
    step = stretch.step_of(0.75)
    n = stretch.t_out(17, step)
    good = (ctypes.c_int64 * 10)(*stretch.record(0, 0, 3, 20, 24, 17, 0, 0, n, step))
    bad = lib.ov_stretch_rows_f32(None, good, 1, p, 1000, p, 1000, None)
    assert bad != 0
    assert bad == lib.ov_stretch_rows_f32(p, None, 1, p, 1000, p, 1000, None)            # the host copy is required
    assert bad == lib.ov_stretch_rows_f32(p, good, 0, p, 1000, p, 1000, None)
    # a bad record in the host table: OV_E_BADARG before anything is launched (no device is touched here)
    assert bad == lib.ov_stretch_rows_f32(p, good, 1, p, 2 * 20 + 16, p, 1000, None)
    worse = (ctypes.c_int64 * 10)(*stretch.record(0, 0, 3, 20, 24, 17, 1, 0, n, step))
    assert bad == lib.ov_stretch_rows_f32(p, worse, 1, p, 1000, p, 1000, None)
