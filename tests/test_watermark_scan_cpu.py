"""The host side of the watermark scan (``watermark.scan_host``, ``build_chains``, ``false_alarm``, ``judge``,
``plan_windows``, the argument checks), on the CPU: no kernel runs here."""
import re
from pathlib import Path

import numpy as np
import pytest

from openvoice_amd import _lib, watermark as wm

ROOT = Path(__file__).resolve().parents[1]
KEY = 0x1234ABCD5678
STRIDE = wm.STRIDE
MESSAGE = "@MyShell"


def _signal(n, seed=3):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    return (0.3 * np.sin(2 * np.pi * 180.0 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.02 * rng.standard_normal(n))


def test_scan_host_is_read_host_at_every_sampled_offset():
    x = _signal(wm.WINDOW + 3000)
    p, level = wm.scan_host(x, KEY)
    S = x.size - wm.WINDOW + 1
    assert p.shape == (S, 32) and level.shape == (S,)
    offsets = sorted({0, 1, 31, 32, 33, S - 1} | set(np.random.default_rng(0).choice(np.arange(34, S - 1), 44, replace=False).tolist()))
    assert len(offsets) == 50
    for s in offsets:
        q, a = wm.read_host(x[s:s + wm.WINDOW], KEY)
        assert np.abs(p[s] - q[0]).max() <= 1e-15 and abs(level[s] - a[0]) <= 1e-15 * a[0]
    with pytest.raises(ValueError):
        wm.scan_host(x[:wm.WINDOW - 1], KEY)


def test_scan_host_finds_a_cut_mark_and_nothing_in_unmarked_audio():
    x = _signal(2 * wm.WINDOW + 3000, seed=5)
    word = wm.groups_of(MESSAGE)[1]
    bits = [(word >> j) & 1 for j in range(32)]
    y = x.copy()
    y[2000:2000 + wm.WINDOW] = wm.encode_host(x[2000:2000 + wm.WINDOW], bits, KEY)
    cut = y[763:763 + wm.WINDOW + 2500]                  # the window now starts at 1237
    p, level = wm.scan_host(cut, KEY)
    words = ((p >= 0) * (1 << np.arange(32))).sum(axis=1)
    assert np.flatnonzero(words == word).tolist() == [1237]
    assert np.flatnonzero(np.abs(p).min(axis=1) >= 0.98 * level).tolist() == [1237]
    p0, level0 = wm.scan_host(x[763:763 + wm.WINDOW + 2500], KEY)
    assert not (np.abs(p0).min(axis=1) >= 0.98 * level0).any()


def _hit(s, k, e=0, words=(11, 22)):
    return (s, words[k] if k >= 0 else 99, k, e)


def test_chains_follow_stride_and_group_order():
    # two windows in order, then a repeat wrap: 0, 1, 0 at the stride
    chains = wm.build_chains([_hit(500, 0), _hit(500 + STRIDE, 1), _hit(500 + 2 * STRIDE, 0)], 2)
    assert [len(c) for c in chains] == [3] and chains[0][0][0] == 500
    # a wrong stride: two chains of one
    chains = wm.build_chains([_hit(500, 0), _hit(500 + STRIDE + 1, 1)], 2)
    assert sorted(len(c) for c in chains) == [1, 1]
    # a wrong group order: the same group twice does not chain
    chains = wm.build_chains([_hit(500, 0), _hit(500 + STRIDE, 0)], 2)
    assert sorted(len(c) for c in chains) == [1, 1]
    # ... but does with one group (G = 1: k + 1 mod 1 = 0)
    assert [len(c) for c in wm.build_chains([_hit(500, 0), _hit(500 + STRIDE, 0)], 1)] == [2]
    # best first: longest, then fewest errors, then earliest
    chains = wm.build_chains([_hit(10, 0, 2), _hit(20, 1), _hit(20 + STRIDE, 0, 1), _hit(30, 0), _hit(30 + STRIDE, 1)], 2)
    assert [(len(c), c[0][0]) for c in chains] == [(2, 30), (2, 20), (1, 10)]
    # blind: anything at the stride chains
    chains = wm.build_chains([_hit(7, -1), _hit(7 + STRIDE, -1), _hit(9, -1)], 0)
    assert [(len(c), c[0][0]) for c in chains] == [(2, 7), (1, 9)]
    assert wm.build_chains([], 2) == []
    with pytest.raises(ValueError):
        wm.build_chains([_hit(5, 0), _hit(5, 1)], 2)


def test_false_alarm_formula():
    S = 10 * 22050 - wm.WINDOW + 1
    assert wm.false_alarm(S, 2, 0, 1) == pytest.approx(S * 2 / 2.0 ** 32) and 5e-5 < wm.false_alarm(S, 2, 0, 1) < 2e-4
    assert wm.false_alarm(S, 2, 0, 2) == pytest.approx(S * 2 / 2.0 ** 64) and wm.false_alarm(S, 2, 0, 2) < 1e-13
    assert wm.false_alarm(S, 2, 2, 1) == pytest.approx(S * 2 * (1 + 32 + 496) / 2.0 ** 32)
    assert wm.false_alarm(1000, 1, 32, 3) == pytest.approx(1000.0)
    with pytest.raises(ValueError):
        wm.false_alarm(S, 2, 0, 0)


def test_judge_known_blind_and_overflow():
    words = wm.groups_of(MESSAGE)
    S = 200000
    one = wm.judge([(30763, words[1], 1, 0)], 1, S, words, MESSAGE, 0, 1e-6, [1.01])
    assert not one["marked"] and one["offset"] == 30763 and one["first_group"] == 1 and len(one["windows"]) == 1
    assert one["false_alarm"] == pytest.approx(S * 2 / 2.0 ** 32) and one["windows"][0] == (30763, 1, words[1], 0, 1.01)
    two = wm.judge([(30763, words[1], 1, 0), (30763 + STRIDE, words[0], 0, 0)], 2, S, words, MESSAGE, 0, 1e-6)
    assert two["marked"] and two["offset"] == 30763 and two["first_group"] == 1 and two["false_alarm"] < 1e-13
    assert two["message"] == MESSAGE and not two["overflow"] and two["hits"] == 2
    none = wm.judge([], 0, S, words, MESSAGE, 0, 1e-6)
    assert not none["marked"] and none["offset"] is None and none["windows"] == [] and none["false_alarm"] is None
    # a capacity overflow is reported as such: 7 hits, 2 rows kept
    over = wm.judge([(5, words[0], 0, 0), (9, words[0], 0, 0)], 7, S, words, MESSAGE, 0, 1e-6)
    assert over["overflow"] and over["hits"] == 7
    # blind: the characters in chain order, marked from two windows on, no false-alarm figure
    blind = wm.judge([(30763, words[1], -1, 0), (30763 + STRIDE, words[0], -1, 0)], 2, S, [], None, 0, 1e-6)
    assert blind["marked"] and blind["message"] == "hell@MyS" and blind["false_alarm"] is None
    assert blind["first_group"] is None and [w[1] for w in blind["windows"]] == [None, None]
    lone = wm.judge([(30763, words[1], -1, 0)], 1, S, [], None, 0, 1e-6)
    assert not lone["marked"] and lone["message"] == "hell"
    assert wm.word_to_string(words[0]) + wm.word_to_string(words[1]) == MESSAGE


def test_message_repeat_windows_of_the_planner():
    n = 3 * STRIDE + wm.WINDOW
    assert wm.plan_windows(n, 2) == [(0, 0), (STRIDE, 1)]                  # today's windows
    assert wm.plan_windows(n, 2, True) == [(0, 0), (STRIDE, 1), (2 * STRIDE, 0), (3 * STRIDE, 1)]
    assert wm.plan_windows(n - 1, 2, True) == [(0, 0), (STRIDE, 1), (2 * STRIDE, 0)]
    assert wm.plan_windows(wm.WINDOW - 1, 2, True) == [] and wm.plan_windows(wm.WINDOW, 2) == [(0, 0)]
    assert wm.plan_windows(n, 1) == [(0, 0)] and wm.plan_windows(n, 0, True) == []
    # the default plan is the one mark_many has always made: the leading groups that fit
    for length in (0, 15999, 16000, 47999, 48000, 200000):
        fit = [(k * STRIDE, k) for k in range(2) if k * STRIDE + wm.WINDOW <= length]
        assert wm.plan_windows(length, 2, False) == fit


def test_bad_arguments_raise():
    ok = dict(message=MESSAGE, max_errors=0, margin=0.98, max_false_alarm=1e-6)
    assert wm.check_find_args(**ok) == (wm.groups_of(MESSAGE), 0, 0.98, 1e-6, wm.HIT_CAPACITY)
    assert wm.check_find_args(None, 3, 1, 1.0, 0) == ([], 3, 1.0, 1.0, 0)
    for bad in (dict(message=5), dict(message=b"x"), dict(max_errors=-1), dict(max_errors=33), dict(max_errors=1.0),
                dict(max_errors=True), dict(margin=0.0), dict(margin=1.5), dict(margin="1"), dict(margin=float("nan")),
                dict(max_false_alarm=0.0), dict(max_false_alarm=2.0), dict(max_false_alarm=None), dict(capacity=-1),
                dict(capacity=1.5)):
        with pytest.raises(ValueError):
            wm.check_find_args(**{**ok, **bad})
    model = wm.NativeWatermark(KEY)
    with pytest.raises(ValueError):
        model.find([np.zeros(20000, dtype=np.float32)], MESSAGE)              # no CPU path
    with pytest.raises(ValueError):
        model.find([], MESSAGE, max_errors=40)
    with pytest.raises(ValueError):
        model.mark_many([np.zeros(20000, dtype=np.float32)], MESSAGE, message_repeat=True)
    with pytest.raises(TypeError):
        model.mark_many([], MESSAGE, True)                                    # keyword only


def test_abi_surface():
    header = (ROOT / "include" / "openvoice_amd.h").read_text()
    assert int(re.search(r"#define OV_ABI_VERSION (\d+)", header).group(1)) == 212 == _lib.MIN_VERSION
    for name in ("ov_wm_scan_f32", "ov_wm_scan_tile", "ov_wm_scan_pick"):
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", header)
    assert len(_lib.SIGNATURES["ov_wm_scan_f32"][1]) == 14 and len(_lib.SIGNATURES["ov_wm_scan_pick"][1]) == 14
    shim = (ROOT / "openvoice_amd" / "csrc" / "torch_shim.cpp").read_text()
    assert "bind_device<&ov_wm_scan_f32>" in shim and "bind_device<&ov_wm_scan_pick>" in shim
    assert "watermark_scan.hip" in (ROOT / "openvoice_amd" / "csrc" / "Makefile").read_text()
    lib = _lib.load()
    assert lib.ov_wm_scan_tile() == 896 == _lib.torch_ops().wm_scan_tile()
    import ctypes
    p = ctypes.c_void_p(64)
    bad = lib.ov_wm_scan_f32(None, 20000, p, 1, 20000, 0, 0.02, 0.001, p, p, p, None, 4001, None)
    assert bad != 0 and bad == lib.ov_wm_scan_f32(p, 20000, p, 0, 20000, 0, 0.02, 0.001, p, p, p, None, 4001, None)
    assert bad == lib.ov_wm_scan_f32(p, 20000, p, 1, 15999, 0, 0.02, 0.001, p, p, p, None, 4001, None)
    assert bad == lib.ov_wm_scan_pick(p, p, p, 100, p, 1, None, 2, 0, 0.98, p, 4, p, None)       # groups missing
    assert bad == lib.ov_wm_scan_pick(p, p, p, 100, p, 1, p, 9, 0, 0.98, p, 4, p, None)
    assert bad == lib.ov_wm_scan_pick(p, p, p, 100, p, 1, p, 2, 0, 0.98, None, 4, p, None)       # cap > 0 without rows
