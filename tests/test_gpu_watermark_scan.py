"""The watermark scan on the MI355X (``ov_wm_scan_f32``, ``ov_wm_scan_pick``, ``NativeWatermark.find``,
``ToneColorConverter.find_watermark``): the scan kernel against the float64 mirror ``watermark.scan_host`` under derived
bounds inside NaN-filled buffers, its independence of records, tiles and alignment bit for bit, rejected records, the
pick kernel against a numpy selection, and marks found in cut, shifted and clipped conversions end to end.

The bounds (u = 2^-24, one fp32 rounding; x is the same fp32 input on both sides, exact in float64; a factor 1 + 2^-10
covers second-order terms).

* p_j(s).  The products x * (+-1) are exact.  Q[t][j] is a chain of 250 MFMAs, each adding two products to the
  accumulator in an order and with a number of roundings (one or two) the instruction does not disclose: at most 500
  roundings of partial sums, each partial sum at most sum_{S_j} |x| in magnitude.  One more rounding for the division
  by 500, two spare:  |dp_j| <= 503 u mean_{S_j} |x|.
* pmin(s) = min_j |p_j(s)|:  | min |a| - min |b| | <= max |a - b|, so the largest of the 32 bounds of the offset.  (The
  kernel divides the minimum once: rounding is monotonic, so that is the minimum of the divided values.)
* level(s).  W[t] is two FMA chains of 250 non-negative terms (one rounding each) added once; the skewed read adds 16 of
  them per lane half (15 roundings) and the halves once: 250 + 1 + 15 + 1 = 267 roundings on the longest path, all terms
  non-negative, so the relative error of the energy is at most 267 u, and 268 u after the division by 16 000.  The
  square root halves it (134 u) and rounds (1), the product with the strength rounds (1) and the strength itself is the
  fp32 nearest to the mirror's float64 (1): |dlevel| <= 137 u level.  The maximum with the floor (exact) is 1-Lipschitz.

Measured on the MI355X, worst error / bound: see DESIGN.md section 29."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib, api, audio_io, watermark  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
KEY, STRENGTH, FLOOR = 0x1234ABCD5678, watermark.DEFAULT_STRENGTH, watermark.DEFAULT_FLOOR
W, STRIDE = watermark.WINDOW, watermark.STRIDE
TILE = 896
SRC_OFF, OUT_OFF = 13, 5                                  # unaligned on purpose
MESSAGE = "@MyShell"


def _noise(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, generator=gen, dtype=torch.float64)).float()


def _patchwork(seed=2):
    """A loud stretch, a silent stretch and a long 1e-5 stretch: windows that mix them, and (from offset 1000 on) windows
    that lie wholly in the 1e-5 stretch, whose level is the floor."""
    gen = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(W + 1400, generator=gen, dtype=torch.float64)
    x[600:1000] = 0.0
    x[1000:] = 1e-5 * torch.randn(W + 400, generator=gen, dtype=torch.float64)
    return x.float()


def _marked_noise(n, at, word, seed):
    x = _noise(n, seed).numpy().astype(np.float64)
    x[at:at + W] = watermark.encode_host(x[at:at + W], [(word >> j) & 1 for j in range(32)], KEY, STRENGTH, FLOOR)
    return torch.from_numpy(x).float()


def _scan(x, recs=None, projections=True, src_pad=8, out_elems=None):
    """``x`` at SRC_OFF of a NaN-filled buffer, scanned by ``recs`` (default: one record for all of it, outputs at
    OUT_OFF) -> the output arrays on the host, whole, with their fills where no record wrote."""
    n = x.numel()
    src = torch.full((SRC_OFF + n + src_pad,), float("nan"))
    src[SRC_OFF:SRC_OFF + n] = x
    S = n - W + 1
    recs = [(SRC_OFF, n, OUT_OFF)] if recs is None else recs
    out = watermark.scan(src.to(DEV), recs, KEY, STRENGTH, FLOOR, out_elems=OUT_OFF + max(S, 1) + 3 if out_elems is None
                         else out_elems, projections=projections)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _check_against_mirror(x, got, marked_at=None, payload=None):
    """The docstring's bounds at every offset; returns the worst error / bound per quantity and the left-out share."""
    words, pmin, level, p = got
    n = x.numel()
    S = n - W + 1
    x64 = x.numpy().astype(np.float64)
    p64, level64 = watermark.scan_host(x64, KEY, STRENGTH, FLOOR)
    # mean_{S_j} |x| of window s, bit j: the same skewed read of the absolute values
    absx = np.abs(x64)
    T = S + 31
    A = np.lib.stride_tricks.as_strided(absx, shape=(T, W // 32), strides=(8, 256)).sum(axis=1)
    mabs = A[np.arange(S)[:, None] + np.arange(32)[None, :]] / (W // 32)
    bp = 503 * U * mabs * SLACK
    sl = slice(OUT_OFF, OUT_OFF + S)
    # nothing outside the record's output range was written
    for arr in (pmin, level, p):
        assert torch.isnan(arr[:OUT_OFF]).all() and torch.isnan(arr[OUT_OFF + S:]).all()
    assert (words[:OUT_OFF] == 0).all() and (words[OUT_OFF + S:] == 0).all()
    gp = p[sl].numpy().astype(np.float64)
    assert np.isfinite(gp).all()
    ep = np.abs(gp - p64)
    assert (ep <= bp).all(), f"p: worst error / bound {np.max(ep / np.maximum(bp, 1e-300))}"
    gmin = pmin[sl].numpy().astype(np.float64)
    emin = np.abs(gmin - np.abs(p64).min(axis=1))
    assert (emin <= bp.max(axis=1)).all()
    assert np.array_equal(pmin[sl].numpy(), np.abs(p[sl].numpy()).min(axis=1))        # pmin IS the minimum of the p it wrote
    bl = 137 * U * level64 * SLACK
    el = np.abs(level[sl].numpy().astype(np.float64) - level64)
    assert (el <= bl).all(), f"level: worst error / bound {np.max(el / bl)}"
    # the words: equal to the mirror's wherever the mirror's projection is outside the bound
    gw = (words[sl].numpy().astype(np.int64)[:, None] >> np.arange(32)[None, :]) & 1
    assert np.array_equal(gw, (gp >= 0).astype(np.int64))                               # ... and ARE the signs of its p
    decided = np.abs(p64) > bp
    assert np.array_equal(gw[decided], (p64 >= 0).astype(np.int64)[decided])
    left_out = 1.0 - decided.mean()
    if marked_at is not None:
        assert decided[marked_at].all() and int(words[OUT_OFF + marked_at]) & 0xFFFFFFFF == payload
    ratios = (float(np.max(ep / np.maximum(bp, 1e-300))), float(np.max(emin / np.maximum(bp.max(axis=1), 1e-300))),
              float(np.max(el / bl)))
    return ratios, left_out


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("extra", [0, 31, TILE + 37])
def test_scan_against_the_float64_mirror(extra, binding, monkeypatch):
    """n = 16 000 (one offset), 16 031 (every residue once), 16 000 + a tile + 37 (a tile edge and a ragged tail); the
    last one holds a marked window at offset 411, where every bit is compared and exact."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    assert _lib.call("ov_wm_scan_tile") == TILE
    word = watermark.groups_of(MESSAGE)[0]
    x = _marked_noise(W + extra, 411, word, 7) if extra > 411 else _noise(W + extra, 7)
    ratios, left_out = _check_against_mirror(x, _scan(x), 411 if extra > 411 else None, word)
    print(f"scan n = {W + extra} [{binding}]: worst error / bound p {ratios[0]:.3f} pmin {ratios[1]:.3f} level {ratios[2]:.3f}; "
          f"left out {100 * left_out:.3f} %")
    assert left_out <= 0.01


def test_scan_of_loud_silent_and_tiny_stretches():
    x = _patchwork()
    got = _scan(x)
    ratios, left_out = _check_against_mirror(x, got)
    print(f"patchwork: worst error / bound p {ratios[0]:.3f} pmin {ratios[1]:.3f} level {ratios[2]:.3f}; left out "
          f"{100 * left_out:.3f} %")
    assert left_out <= 0.01
    level = got[2][OUT_OFF:OUT_OFF + x.numel() - W + 1]
    assert (level[1000:] == FLOOR).all() and (level[:100] > FLOOR).all()     # the floor where the window is all tiny


def test_an_offset_depends_on_its_window_alone():
    """torch.equal: one record for the whole, the same range cut into three records at non-multiples of 32, and a record
    that starts d samples later against the slice of the whole."""
    n = W + 2 * TILE + 300
    x = _noise(n, 9)
    S = n - W + 1
    whole = _scan(x, projections=False)
    cuts = [0, 701, 1403, S]
    recs = [(SRC_OFF + a, (b - a) + W - 1, OUT_OFF + a) for a, b in zip(cuts[:-1], cuts[1:])]
    three = _scan(x, recs, projections=False)
    for a, b in zip(whole, three):
        assert torch.equal(a[OUT_OFF:OUT_OFF + S], b[OUT_OFF:OUT_OFF + S])
        assert torch.equal(torch.isnan(a), torch.isnan(b))                   # and the same fills around it
    assert not torch.isnan(whole[1][OUT_OFF:OUT_OFF + S]).any()
    for d in (1, 31, 33):
        later = _scan(x, [(SRC_OFF + d, n - d, OUT_OFF)], projections=False)
        for a, b in zip(whole, later):
            assert torch.equal(a[OUT_OFF + d:OUT_OFF + S], b[OUT_OFF:OUT_OFF + S - d])


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
def test_bad_scan_records_write_nothing(binding, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    n = W + 100
    src = _noise(n + 50, 1).to(DEV)
    E = 300
    words = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    pmin, level = torch.full((E,), -7.0, device=DEV), torch.full((E,), -7.0, device=DEV)
    bad = [(0, W - 1, 0),                                 # shorter than a window
           (51, n, 0), (-1, n, 0),                        # past src, a negative source offset
           (0, n, E - 100), (0, n, -1),                   # past the outputs, a negative output offset
           (0, n + 1, 0),                                 # longer than max_n
           (1 << 62, n, 0), (0, n, 1 << 62)]
    good = (7, W + 19, 150)
    recs = torch.tensor(bad + [good], dtype=torch.int64).to(DEV)
    args = (src, src.numel(), recs, len(bad) + 1, n, KEY, STRENGTH, FLOOR, words, pmin, level, None, E)
    _lib.call("ov_wm_scan_f32", *args)
    torch.cuda.synchronize()
    w, p, l = words.cpu(), pmin.cpu(), level.cpu()
    for arr in (w, p, l):
        assert (arr[:150] == -7).all() and (arr[170:] == -7).all()
    assert (p[150:170] >= 0).all() and (l[150:170] > 0).all()                # only the good record wrote
    for i, v in ((0, None), (1, 0), (2, None), (3, 0), (3, 65536), (4, W - 1), (5, -1), (6, 1.5), (7, 0.0), (8, None), (9, None),
                 (10, None), (12, 0)):
        call = list(args)
        call[i] = v
        with pytest.raises(_lib.OvError):
            _lib.call("ov_wm_scan_f32", *call)
    assert torch.equal(words.cpu(), w) and torch.equal(pmin.cpu(), p) and torch.equal(level.cpu(), l)


# ---- the pick kernel -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scanned():
    """Two waveforms scanned into one set of arrays: noise holding the message's two windows 32 000 apart from offset
    517, and silence."""
    words = watermark.groups_of(MESSAGE)
    n = STRIDE + W + 1500
    x = _marked_noise(n, 517, words[0], 21).numpy().astype(np.float64)
    x[517 + STRIDE:517 + STRIDE + W] = watermark.encode_host(x[517 + STRIDE:517 + STRIDE + W],
                                                              [(words[1] >> j) & 1 for j in range(32)], KEY, STRENGTH, FLOOR)
    src = torch.cat([torch.from_numpy(x).float(), torch.zeros(W + 700)]).to(DEV)
    S0, S1 = n - W + 1, 701
    sw, pmin, level = watermark.scan(src, [(0, n, 3), (n, W + 700, 3 + S0 + 2)], KEY, STRENGTH, FLOOR)
    return sw, pmin, level, [(3, S0), (3 + S0 + 2, S1)], words


def _select(scanned, groups, max_errors, margin):
    """The numpy selection the pick kernel must equal: per record the rows (s, word, k, errors) in ascending s."""
    sw, pmin, level, recs, _ = scanned
    sw, pmin, level = sw.cpu().numpy(), pmin.cpu().numpy(), level.cpu().numpy()
    out = []
    for off, S in recs:
        w = sw[off:off + S]
        if groups:
            errs = np.stack([np.array([bin(int(v) & 0xFFFFFFFF ^ g).count("1") for v in w]) for g in groups], axis=1)
            k = errs.argmin(axis=1)                       # the lowest k among equals
            e = errs.min(axis=1)
            idx = np.flatnonzero(e <= max_errors)
            out.append(np.stack([idx, w[idx], k[idx], e[idx]], axis=1).astype(np.int64))
        else:
            idx = np.flatnonzero(pmin[off:off + S] >= np.float32(margin) * level[off:off + S])
            out.append(np.stack([idx, w[idx], np.full(idx.size, -1), np.zeros(idx.size, np.int64)], axis=1).astype(np.int64))
    return out


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("mode", ["exact", "errors9", "blind", "blind_loose"])
def test_pick_is_the_numpy_selection(mode, binding, scanned, monkeypatch):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    sw, pmin, level, recs, words = scanned
    groups, max_errors, margin = {"exact": (words, 0, 0.98), "errors9": (words, 9, 0.98), "blind": ([], 0, 0.98),
                                  "blind_loose": ([], 0, 0.25)}[mode]
    want = _select(scanned, groups, max_errors, margin)
    if mode in ("exact", "blind"):
        assert want[0][:, 0].tolist() == [517, 517 + STRIDE] and want[1].shape[0] == 0     # silence: no hit, count 0
    else:
        assert want[0].shape[0] > 150                     # enough to overflow a capacity of 100 across many steps
    for cap in (4096, 100, 0):
        hits, counts = watermark.scan_pick(sw, pmin, level, recs, groups, max_errors, margin, cap)
        torch.cuda.synchronize()
        hits, counts = hits.cpu().numpy().astype(np.int64), counts.cpu().numpy()
        for r, rows in enumerate(want):
            assert counts[r] == rows.shape[0]             # the true count, overflow or not
            keep = min(cap, rows.shape[0])
            assert np.array_equal(hits[r, :keep], rows[:keep])
            assert (hits[r, keep:] == 0).all()            # nothing beyond
            assert (np.diff(hits[r, :keep, 0]) > 0).all()


def test_bad_pick_records_write_nothing(scanned):
    sw, pmin, level, recs, words = scanned
    E = sw.numel()
    hits = torch.full((4, 8, 4), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    table = torch.tensor([(-1, 10), (E - 5, 6), (0, -1), recs[0]], dtype=torch.int64).to(DEV)
    g = torch.tensor(words, dtype=torch.int64).to(torch.int32).to(DEV)
    _lib.call("ov_wm_scan_pick", sw, pmin, level, E, table, 4, g, 2, 0, 0.98, hits, 8, counts)
    torch.cuda.synchronize()
    assert (hits[:3] == -7).all() and (counts[:3] == -7).all() and int(counts[3]) == 2
    assert hits[3, :2, 0].tolist() == [517, 517 + STRIDE] and (hits[3, 2:] == -7).all()
    for i, v in ((0, None), (3, 0), (5, 0), (6, None), (7, 9), (8, -1), (8, 33), (9, -1.0), (11, -1), (12, None)):
        call = [sw, pmin, level, E, table, 4, g, 2, 0, 0.98, hits, 8, counts]
        call[i] = v
        with pytest.raises(_lib.OvError):
            _lib.call("ov_wm_scan_pick", *call)


# ---- end to end on the synthetic weights -----------------------------------------------------------------------------
N_IN = 3 * STRIDE + W + 1200                              # four carrier windows


def _make(tmp_path_factory, synth_sd, name, **kw):
    from openvoice_amd.utils import default_converter_hparams
    d = tmp_path_factory.mktemp(name)
    hps = default_converter_hparams("v2")
    (d / "config.json").write_text(json.dumps({"_version_": "v2", "data": dict(hps.data.items()),
                                               "model": dict(hps.model.items())}))
    torch.save({"model": synth_sd}, d / "checkpoint.pth")
    t = api.ToneColorConverter(str(d / "config.json"), device=DEV, **kw)
    t.load_ckpt(str(d / "checkpoint.pth"))
    return t


@pytest.fixture(scope="module")
def native(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "scan_native", watermark="native", watermark_key=KEY)


@pytest.fixture(scope="module")
def plain(tmp_path_factory, synth_sd):
    return _make(tmp_path_factory, synth_sd, "scan_plain", enable_watermark=False)


@pytest.fixture(scope="module")
def ses():
    gen = torch.Generator().manual_seed(11)
    return (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV), (0.3 * torch.randn(1, 256, 1, generator=gen)).to(DEV)


def _wave(n, seed):
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64) / 22050.0
    phase = 2 * np.pi * torch.cumsum(140.0 + 40.0 * torch.sin(2 * np.pi * 0.3 * t), 0) / 22050.0
    y = (0.35 * torch.sin(phase) + 0.15 * torch.sin(3.1 * phase + 0.5)) * (0.6 + 0.4 * torch.sin(2 * np.pi * 4.0 * t))
    return (y + 0.01 * torch.randn(n, generator=gen, dtype=torch.float64)).float()


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("scan_audio") / "five_seconds.wav")
    audio_io.write(p, _wave(N_IN, 4).numpy(), 22050)
    return p


@pytest.fixture(scope="module")
def unmarked(plain, ses, path):
    return plain.convert(path, *ses, seed=5)


@pytest.fixture(scope="module")
def repeated(native, ses, path):
    out = native.convert(path, *ses, message=MESSAGE, seed=5, message_repeat=True)
    assert len(out) >= 3 * STRIDE + W
    return out


@pytest.fixture(scope="module")
def once(native, ses, path):
    return native.convert(path, *ses, message=MESSAGE, seed=5)


def test_message_repeat_false_is_todays_output(native, ses, path, once, repeated, unmarked):
    assert np.array_equal(once, native.convert(path, *ses, message=MESSAGE, seed=5, message_repeat=False))
    assert np.array_equal(once, native.add_watermark(unmarked.copy(), MESSAGE))         # the host loop: two windows
    assert np.array_equal(once[:STRIDE + W], repeated[:STRIDE + W])
    assert np.array_equal(once[STRIDE + W:], unmarked[STRIDE + W:])
    for n in (2, 3):                                       # windows 2 and 3 carry groups 0 and 1 again
        a = n * STRIDE
        assert not np.array_equal(repeated[a:a + W], unmarked[a:a + W])
        assert native.detect_watermark(repeated[a:], 1) == MESSAGE[4 * (n % 2):4 * (n % 2) + 4]
    assert np.array_equal(repeated[3 * STRIDE + W:], unmarked[3 * STRIDE + W:])
    assert native.detect_watermark(once, 2) == MESSAGE                                   # untouched


def test_a_cut_front_is_found(native, repeated):
    model = native.watermark_model
    before = model.launches
    res = native.find_watermark(repeated[1237:], MESSAGE)
    assert model.launches == before + 2                   # one scan, one pick
    assert res["marked"] and res["offset"] == STRIDE - 1237 and res["first_group"] == 1
    assert [w[0] for w in res["windows"]] == [STRIDE - 1237 + k * STRIDE for k in range(3)]
    assert [w[1] for w in res["windows"]] == [1, 0, 1] and all(w[3] == 0 for w in res["windows"])
    assert all(w[4] >= 0.98 for w in res["windows"]) and res["false_alarm"] < 1e-20 and not res["overflow"]
    assert res["hits"] == 3 and res["message"] == MESSAGE
    # blind: the characters in chain order
    blind = native.find_watermark(repeated[1237:])
    assert blind["marked"] and blind["offset"] == STRIDE - 1237 and blind["message"] == "hell@MyShell"
    assert blind["false_alarm"] is None and blind["first_group"] is None


def test_a_prepended_jingle_is_skipped(native, repeated):
    jingle = 0.2 * np.sin(np.arange(777) * 0.05).astype(np.float32)
    res = native.find_watermark(np.concatenate([jingle, repeated]), MESSAGE)
    assert res["marked"] and res["offset"] == 777 and res["first_group"] == 0 and len(res["windows"]) == 4
    assert [w[1] for w in res["windows"]] == [0, 1, 0, 1]
    blind = native.find_watermark(np.concatenate([jingle, repeated]))
    assert blind["marked"] and blind["offset"] == 777 and blind["message"] == 2 * MESSAGE


def test_a_clip_from_the_middle_of_a_repeating_live_stream(native, ses):
    wave = _wave(N_IN, 6)
    s = native.live_stream(*ses, seed=5, message=MESSAGE, message_repeat=True, watermark_hold=3200)
    outs = [s.push(wave[i:i + 8000]) for i in range(0, wave.numel(), 8000)] + [s.close()]
    out = torch.cat([o for o in outs if o.numel()])
    assert out.numel() >= 3 * STRIDE + W
    clip = out[STRIDE + 5003:3 * STRIDE + W + 900]        # windows 2 and 3 whole, window 1 cut
    res = native.watermark_model.find([clip], MESSAGE)[0]
    assert res["marked"] and res["offset"] == STRIDE - 5003 and res["first_group"] == 0
    assert [w[1] for w in res["windows"]] == [0, 1]


def test_one_window_is_reported_but_not_called_marked(native, once):
    res = native.find_watermark(once[1237:], MESSAGE)     # window 0 is cut, window 1 survives
    assert not res["marked"] and res["offset"] == STRIDE - 1237 and res["first_group"] == 1 and len(res["windows"]) == 1
    assert 1e-5 < res["false_alarm"] < 1e-4
    assert native.find_watermark(once[1237:], MESSAGE, max_false_alarm=1e-3)["marked"]
    blind = native.find_watermark(once[1237:])
    assert not blind["marked"] and blind["message"] == "hell"
    whole = native.find_watermark(once, MESSAGE)
    assert whole["marked"] and whole["offset"] == 0 and whole["first_group"] == 0 and len(whole["windows"]) == 2


def test_unmarked_audio_and_a_wrong_key(native, plain, unmarked, repeated, tmp_path_factory, synth_sd):
    for message in (MESSAGE, None):
        res = native.find_watermark(unmarked, message)
        assert not res["marked"] and res["hits"] == 0 and res["offset"] is None and res["windows"] == []
    other = _make(tmp_path_factory, synth_sd, "scan_other", watermark="native", watermark_key=KEY + 1)
    for message in (MESSAGE, None):
        res = other.find_watermark(repeated, message)
        assert not res["marked"] and res["hits"] == 0
    with pytest.raises(ValueError, match="native"):
        plain.find_watermark(repeated, MESSAGE)
    with pytest.raises(ValueError, match="native"):
        plain.convert_long(unmarked, *[None, None], message_repeat=True)
    short = native.find_watermark(repeated[:W - 1], MESSAGE)                  # no window fits: nothing to scan
    assert not short["marked"] and short["hits"] == 0
    many = native.watermark_model.find([torch.from_numpy(repeated[1237:]).to(DEV), torch.from_numpy(unmarked).to(DEV),
                                        torch.zeros(100, device=DEV)], MESSAGE)
    assert [m["marked"] for m in many] == [True, False, False] and many[0]["offset"] == STRIDE - 1237
