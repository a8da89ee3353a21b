"""The block-wise watermark of streams (``openvoice_amd/watermark.py``, "streams") on the host: the float64 mirror reads
back at every hold and keeps the window's guarantee, a hold of one whole window is the file mark, the schedule
(``plan_blocks``) does not depend on how the samples arrive, never releases a sample of an unfinished block and flushes at
the end, ``message_repeat`` cycles the groups, and the keywords are checked at the call.  No kernel is launched."""
import types

import numpy as np
import pytest

from openvoice_amd import api, clone, longform, rates, watermark

N = 48000
MESSAGE = "@MyShell"
KEY = 0x1234ABCD5678
W, S = watermark.WINDOW, watermark.STRIDE


def _signal():
    """48 000 samples: loud noise, a silent stretch and a 1e-5 stretch inside window 0, a modulated tone in window 1."""
    gen = np.random.default_rng(7)
    t = np.arange(N) / 22050.0
    x = 0.1 * gen.standard_normal(N)
    x[3200:6400] = 0.0
    x[6400:9600] = 1e-5 * gen.standard_normal(3200)
    x[S:] = 0.3 * np.sin(2 * np.pi * 220.0 * t[S:]) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t[S:]))
    return x


def _bits(word):
    return np.array([(word >> j) & 1 for j in range(32)], dtype=np.float64)


@pytest.mark.parametrize("H", watermark.HOLDS)
def test_mirror_reads_back_and_keeps_the_window_guarantee(H):
    """``decode_host`` of each window gives the payload, and ``b_j q_j >= (1 - 1e-12) mean_m a_m`` (``a_m``: the level of
    block m of the unmarked window); everything outside the two carrier windows is untouched."""
    x = _signal()
    y = watermark.mark_stream_host(x, MESSAGE, KEY, hold=H)
    words = watermark.groups_of(MESSAGE)
    assert len(words) == 2 and y.dtype == np.float64
    for n, word in enumerate(words):
        win, src = y[n * S:n * S + W], x[n * S:n * S + W]
        bits = _bits(word)
        assert np.array_equal(watermark.decode_host(win, KEY)[0] >= 0.5, bits == 1)
        levels = [watermark.read_host(src[m:m + H], KEY)[1][0] for m in range(0, W, H)]
        q, _ = watermark.read_host(win, KEY)
        assert np.all((2.0 * bits - 1.0) * q[0] >= (1.0 - 1e-12) * np.mean(levels))
        assert np.mean(levels) >= watermark.DEFAULT_FLOOR
    assert np.array_equal(y[W:S], x[W:S]) and not np.array_equal(y[:W], x[:W]) and not np.array_equal(y[S:], x[S:])


def test_a_hold_of_one_window_is_the_file_mark_exactly():
    x = _signal()
    y = watermark.mark_stream_host(x, MESSAGE, KEY, hold=16000)
    ref = x.copy()
    for n, word in enumerate(watermark.groups_of(MESSAGE)):
        ref[n * S:n * S + W] = watermark.encode_host(x[n * S:n * S + W], _bits(word)[None], KEY)
    assert np.array_equal(y, ref)


def test_holds_are_the_divisors_of_the_window_that_are_multiples_of_32_and_at_least_512():
    assert watermark.HOLDS == (16000, 8000, 4000, 3200, 1600, 800, 640)
    assert list(watermark.HOLDS) == [h for h in range(16000, 511, -1) if 16000 % h == 0 and h % 32 == 0]


def _drive(total, chunks, H, groups=2, repeat=False):
    """The schedule driven through pushes of ``chunks`` (repeating) and a close: per-sample (release step, marked?) and
    the block runs as absolute ``(first sample, blocks, window, group, chip_off)``, merged per window."""
    pos, held, fed, i = 0, 0, 0, 0
    released, runs = [], []
    while True:
        n = min(chunks[i % len(chunks)], total - fed)
        closing = n == 0
        fed += n
        i += 1
        n_out, recs = watermark.plan_blocks(pos, held + n, closing, H, groups, repeat)
        assert 0 <= n_out <= held + n and (not closing or n_out == held + n)
        for off, blocks, window, group, chip_off, reset in recs:
            a = pos + off
            assert a == window * S + chip_off and chip_off % H == 0 and reset == (chip_off == 0)
            assert a + blocks * H <= pos + n_out                       # a marked block leaves in the step that marks it
            runs.append((a, blocks, window, group))
        if not closing:                                                  # no sample of an unfinished block has left
            end = pos + n_out
            w, r = divmod(end, S)
            if watermark._group_of(w, groups, repeat) is not None and r < W:
                assert r % H == 0
            assert held + n - n_out < H
        released.append((pos, pos + n_out))
        pos, held = pos + n_out, held + n - n_out
        if closing:
            break
    assert pos == total and held == 0
    blocks = sorted((a + m * H, window, group) for a, k, window, group in runs for m in range(k))
    return blocks, released


@pytest.mark.parametrize("H", [640, 3200, 16000])
@pytest.mark.parametrize("total", [50000, 47999, 16000, 15999, 100])
def test_the_schedule_does_not_depend_on_the_chunking(H, total):
    want = [(n * S + m, n, n) for n in range(2) for m in range(0, W, H) if n * S + m + H <= total]
    for chunks in ([total], [1000, 37, 7001], [256], [1]):
        if chunks == [1] and total > 16000:
            continue
        blocks, released = _drive(total, chunks, H)
        assert blocks == want, chunks                                    # the same samples in the same blocks
        assert [a for a, _ in released[1:]] == [b for _, b in released[:-1]]


def test_close_flushes_the_rest_unmarked():
    n_out, recs = watermark.plan_blocks(0, 1000, False, 640, 2, False)
    assert (n_out, recs) == (640, [(0, 1, 0, 0, 0, True)])
    n_out, recs = watermark.plan_blocks(640, 360 + 100, True, 640, 2, False)         # 460 samples of block 1: unmarked
    assert (n_out, recs) == (460, [])
    x = _signal()[:S + 700]
    y = watermark.mark_stream_host(x, MESSAGE, KEY, hold=640)
    assert np.array_equal(y[S + 640:], x[S + 640:])                                   # the unfinished block
    assert not np.array_equal(y[S:S + 640], x[S:S + 640])                             # the whole one before it
    # outside the carrier windows nothing waits
    assert watermark.plan_blocks(16000, 5000, False, 640, 2, False) == (5000, [])
    assert watermark.plan_blocks(48000, 99999, False, 640, 2, False) == (99999, [])   # past the message: untouched
    with pytest.raises(ValueError, match="inside a block"):
        watermark.plan_blocks(100, 1000, False, 640, 2, False)


def test_message_repeat_cycles_the_groups():
    blocks, _ = _drive(4 * S + 100, [7001], 16000, groups=2, repeat=True)
    assert blocks == [(n * S, n, n % 2) for n in range(4)]
    blocks, _ = _drive(4 * S + 100, [7001], 16000, groups=2, repeat=False)
    assert blocks == [(n * S, n, n) for n in range(2)]
    x = np.tile(_signal()[:S], 4)
    y = watermark.mark_stream_host(x, MESSAGE, KEY, hold=3200, repeat=True)
    conv = object.__new__(api.ToneColorConverter)                        # the reader is the hook's, unchanged
    conv.device, conv.watermark_model = "cpu", _HostModel()
    assert conv.detect_watermark(y, 4) == MESSAGE + MESSAGE
    once = watermark.mark_stream_host(x, MESSAGE, KEY, hold=3200)
    assert np.array_equal(once[:2 * S], y[:2 * S]) and np.array_equal(once[2 * S:], x[2 * S:])


class _HostModel:
    """The mirror behind the hook's ``decode`` (``detect_watermark`` passes [1, 16000] tensors)."""

    def decode(self, carrier):
        import torch
        return torch.from_numpy(watermark.decode_host(carrier.numpy().astype(np.float64), KEY))


def test_a_bad_hold_or_a_non_native_model_raises_at_the_call():
    native = watermark.NativeWatermark(key=KEY)
    model, words, H, repeat = watermark.stream_mark(native, MESSAGE, 640, True)
    assert (model, words, H, repeat) == (native, watermark.groups_of(MESSAGE), 640, True)
    assert watermark.stream_mark(None, None) is None and watermark.stream_mark(native, None, 800) is None
    for hold in (1000, 512, 32000, 0, 640.0, True, None):
        with pytest.raises(ValueError, match="watermark_hold"):
            watermark.stream_mark(native, MESSAGE, hold)
        with pytest.raises(ValueError, match="watermark_hold"):
            watermark.stream_mark(None, None, hold)                      # checked even when nothing is marked
    for model in (None, _HostModel(), object()):
        with pytest.raises(ValueError, match="native"):
            watermark.stream_mark(model, MESSAGE)
    # the stream constructors ask before they touch anything else
    conv = types.SimpleNamespace(watermark_model=_HostModel())
    with pytest.raises(ValueError, match="native"):
        longform.ConversionStream(conv, None, None, message=MESSAGE)
    conv.watermark_model = native
    with pytest.raises(ValueError, match="watermark_hold"):
        longform.ConversionStream(conv, None, None, message=MESSAGE, watermark_hold=1000)
    # speak_stream*: at the call, not at the first next()
    cloner = object.__new__(clone.VoiceCloner)
    cloner.converter = types.SimpleNamespace(watermark_model=None)
    with pytest.raises(ValueError, match="native"):
        cloner.speak_stream_ids([[1, 2]], 0, None, None, message=MESSAGE)
    cloner.converter.watermark_model = native
    with pytest.raises(ValueError, match="watermark_hold"):
        cloner.speak_stream_ids([[1, 2]], 0, None, None, message=MESSAGE, watermark_hold=12345)


def test_the_latency_bound_says_what_the_hold_adds():
    sec, samples = rates.stream_latency(4224)
    assert rates.stream_latency(4224, hold_samples=0) == (sec, samples)
    sec_h, samples_h = rates.stream_latency(4224, hold_samples=639)
    assert samples_h == samples + 639 and sec_h - sec == pytest.approx(639 / 22050)
    native = watermark.NativeWatermark()
    assert watermark.hold_wait(None) == 0 and watermark.hold_wait(watermark.stream_mark(native, "x", 3200)) == 3199
