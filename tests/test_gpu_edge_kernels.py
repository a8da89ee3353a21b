"""The waveform-edge kernels of csrc/ov_api.hip and csrc/longform.hip, one by one, against the mirrors of
oracle/edge_ref.py: ``ov_conv_post_tanh_f32`` / ``ov_conv_post_tanh_limited_f32`` and ``ov_linear_f32`` on EVERY element
against float64 (lim = S_POST absacc + T_TANH 2^-24 |ref|, lim = S_LIN absacc; allowances measured reference against
reference, tests/test_edge_criterion_cpu.py), ``ov_sequence_mask_f32``, ``ov_frame_limits_i32``, ``ov_unpad_rows_f32``,
``ov_stitch_window_cores_f32``, ``ov_frame_hops_f32``, ``ov_frame_hops_windows_f32`` and ``ov_frame_hops_multi_f32`` bit
for bit against exact index mirrors.

Every test runs under both bindings through ``_lib.call``.  Inputs and outputs sit at an offset inside larger NaN-filled
buffers (entry points without a row stride get a guard in front and behind): a kernel that reads outside its operand
returns NaN, and everything outside the valid block must still be NaN afterwards.  Each test prints ``RATIO <what>
<worst err / lim>`` (``EXACT <what>`` for the copy kernels) before it asserts.  The shapes are the smallest at which each
mechanism exists: one group, first / last group and both sides of the 1024-sample workgroup boundary of the 16-byte
conv_post path, the 256-thread block boundaries, the ``grid.y`` loop of the unpad, both stitch templates."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from openvoice_amd import _lib  # noqa: E402
from oracle import edge_ref as E  # noqa: E402
from oracle.nanbuf import DEV, NAN  # noqa: E402

BINDINGS = ["torch", "ctypes"]
GUARD = 8                       # floats in front of and behind every operand (a multiple of 4: bases stay 16-byte aligned)


# ---- NaN-guarded buffers ----------------------------------------------------------------------------------------------------
def _put(t, shift=0, guard=GUARD):
    """The flat host tensor ``t`` inside a NaN-filled device buffer -> (buffer, element offset of t): ``shift`` = 1 puts
    its base one float past a 16-byte boundary."""
    flat = torch.full((guard + shift + t.numel() + guard,), NAN)
    flat[guard + shift:guard + shift + t.numel()] = t.reshape(-1)
    flat = flat.to(DEV)
    assert flat.data_ptr() % 16 == 0
    return flat, guard + shift


def _out(n, shift=0, guard=GUARD):
    flat = torch.full((guard + shift + n + guard,), NAN, device=DEV)
    assert flat.data_ptr() % 16 == 0
    return flat, guard + shift


def _take(flat, off, n):
    """The n floats at ``off`` on the host, after checking that everything else is still NaN."""
    torch.cuda.synchronize()
    host = flat.cpu()
    assert torch.isnan(host[:off]).all() and torch.isnan(host[off + n:]).all(), "written outside the output"
    return host[off:off + n].clone()


def _bits(t):
    """The bit patterns of ``t``, every NaN as one pattern (the guards' NaN need not be the mirrors' NaN)."""
    return torch.where(torch.isnan(t), torch.full((), 0x7FC00000, dtype=torch.int32), t.contiguous().view(torch.int32))


def _same_bits(got, want):
    return torch.equal(_bits(got), _bits(want))


def _expect(flat, off, block_shape, valid, what):
    """The device buffer ``flat`` must hold, bit for bit, ``valid`` [.., n] in the first n columns of the block
    ``block_shape`` at ``off`` (or, given a list of (column slice, values) pairs, those columns) and NaN elsewhere."""
    torch.cuda.synchronize()
    got = flat.cpu()
    want = torch.full_like(got, NAN)
    n = int(np.prod(block_shape))
    block = want[off:off + n].view(block_shape)
    for cols, v in (valid if isinstance(valid, list) else [(slice(0, valid.shape[-1]), valid)]):
        block[..., cols] = torch.as_tensor(v)
    ok = _same_bits(got, want)
    print(f"EXACT {what}: {'equal' if ok else 'DIFFERENT'}")
    assert ok, f"{what}: {(_bits(got) != _bits(want)).sum().item()} elements differ"
    return got[off:off + n].view(block_shape)


def _refused(name, *args, untouched=()):
    with pytest.raises(_lib.OvError, match="OV_E_BADARG"):
        _lib.call(name, *args)
    torch.cuda.synchronize()
    for flat in untouched:
        assert torch.isnan(flat).all(), f"{name}: a refused call wrote"


# ---- conv_post + tanh -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _post_case(C, K, L, stress):
    o = E.post_operands(C, K, L, stress=stress)
    return o["x"], o["w"], E.conv_post_tanh(o["x"], o["w"])


def _run_post(x, w, x_shift=0, out_shift=0, limit=None, scale=0):
    Bn, C, L = x.shape
    xf, xo = _put(x, x_shift)
    of, oo = _out(Bn * L, out_shift)
    wd = w.contiguous().to(DEV)
    if limit is None:
        _lib.call("ov_conv_post_tanh_f32", (xf, xo), wd, (of, oo), Bn, C, L, w.shape[1], E.SLOPE)
    else:
        _lib.call("ov_conv_post_tanh_limited_f32", (xf, xo), wd, (of, oo), Bn, C, L, w.shape[1], E.SLOPE, limit, scale)
    return _take(of, oo, Bn * L).view(Bn, L)


@pytest.mark.parametrize("C", E.POST_CS)
@pytest.mark.parametrize("binding", BINDINGS)
def test_conv_post_16_byte_path_and_its_agreement_with_the_per_sample_path(monkeypatch, binding, C):
    """K = 7, L % 4 == 0, aligned bases: one group (neither halo vector loaded), first and last group, both sides of the
    256-thread x 4-sample workgroup boundary.  The same operands forced down the per-sample path (x, then out, one float
    past a 16-byte boundary) must give the same bits: both kernels are fmaf chains in the same (c, j) order, and a halo
    term outside the row is fmaf(w, lrelu(0), acc) = acc."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    worst, identical = 0.0, True
    for L in E.POST_VEC_LS:
        for stress in (False, True):
            x, w, ref = _post_case(C, 7, L, stress)
            got = _run_post(x, w)
            q = E.worst(got, ref)
            same = all(torch.equal(_run_post(x, w, **kw), got) for kw in (dict(x_shift=1), dict(out_shift=1)))
            print(f"RATIO conv_post 16-byte C={C} L={L} stress={stress} {q:.3f} per-sample path bit-identical: {same}")
            worst, identical = max(worst, q), identical and same
            if stress:
                assert (got[2] == 0).all()
    print(f"RATIO conv_post 16-byte C={C} worst {worst:.3f}")
    assert worst <= 1.0
    assert identical


@pytest.mark.parametrize("K", E.POST_KS)
@pytest.mark.parametrize("C", E.POST_CS)
@pytest.mark.parametrize("binding", BINDINGS)
def test_conv_post_per_sample_path(monkeypatch, binding, C, K):
    """Lengths that are no multiple of 4 (and every K but 7) take the per-sample kernel: both sides of its 256-sample
    block boundary, rows shorter than the kernel's reach."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    worst = 0.0
    for L in E.POST_LS:
        for stress in (False, True):
            x, w, ref = _post_case(C, K, L, stress)
            got = _run_post(x, w)
            q = E.worst(got, ref)
            print(f"RATIO conv_post per-sample C={C} K={K} L={L} stress={stress} {q:.3f}")
            worst = max(worst, q)
            if stress:
                assert (got[2] == 0).all()
    print(f"RATIO conv_post per-sample C={C} K={K} worst {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("scale,L", [(4, 16), (256, 1024), (3, 16)], ids=["vec_scale4", "vec_scale256", "scalar_scale3"])
@pytest.mark.parametrize("binding", BINDINGS)
def test_conv_post_limited(monkeypatch, binding, scale, L):
    """col_limit = [0, 1, 3, 100], B = 4: beyond n = min(L, limit * scale) exact zeros, below it the bits of the unlimited
    launch -- also when x[b, :, n + 3:] is NaN: a sample below the limit reads (K - 1) / 2 = 3 columns past it and no more."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    o = E.post_operands(32, 7, L, batch=4)
    x, w = o["x"], o["w"]
    limits = [0, 1, 3, 100]
    lim_dev = torch.tensor(limits, dtype=torch.int32, device=DEV)
    full = _run_post(x, w)
    ref = E.conv_post_tanh(x, w)
    print(f"RATIO conv_post limited scale={scale} L={L} (unlimited launch) {E.worst(full, ref):.3f}")
    assert E.worst(full, ref) <= 1.0
    poisoned = x.clone()
    ns = [min(L, v * scale) for v in limits]
    for b, n in enumerate(ns):
        poisoned[b, :, n + 3:] = NAN
    for name, xin in (("clean", x), ("NaN from n + 3 on", poisoned)):
        got = _run_post(xin, w, limit=lim_dev, scale=scale)
        for b, n in enumerate(ns):
            assert (got[b, n:] == 0).all(), (name, b)
            assert torch.equal(got[b, :n], full[b, :n]), (name, b)
        r = E.conv_post_tanh(x, w, limit=ns)
        print(f"RATIO conv_post limited scale={scale} L={L} {name} {E.worst(got, r):.3f}")
        assert E.worst(got, r) <= 1.0


@pytest.mark.parametrize("binding", BINDINGS)
def test_conv_post_argument_checks(monkeypatch, binding):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    Bn, C, L = 2, 4, 8
    x, w = torch.zeros(Bn * C * L, device=DEV), torch.zeros(C * 8, device=DEV)
    out = torch.full((Bn * L,), NAN, device=DEV)
    lim = torch.ones(Bn, dtype=torch.int32, device=DEV)
    _refused("ov_conv_post_tanh_f32", x, w, out, Bn, C, L, 6, E.SLOPE, untouched=[out])                  # even K
    _refused("ov_conv_post_tanh_f32", x, w, out, 65536, C, L, 7, E.SLOPE, untouched=[out])
    for a in ((None, w, out), (x, None, out), (x, w, None)):
        _refused("ov_conv_post_tanh_f32", *a, Bn, C, L, 7, E.SLOPE, untouched=[out])
    for scale in (0, -4):
        _refused("ov_conv_post_tanh_limited_f32", x, w, out, Bn, C, L, 7, E.SLOPE, lim, scale, untouched=[out])


# ---- linear ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lin_case(M, Kd, stress):
    o = E.linear_operands(M, Kd, stress=stress)
    return o, E.linear(o["x"], o["w"], o["bias"]), E.linear(o["x"], o["w"], None)


@pytest.mark.parametrize("M,Kd", E.LIN_SHAPES)
@pytest.mark.parametrize("binding", BINDINGS)
def test_linear(monkeypatch, binding, M, Kd):
    """Kdim < 64 (idle lanes), Kdim % 64 != 0, M % 4 != 0 (a workgroup with idle waves), with and without bias."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    worst = 0.0
    for stress in (False, True):
        o, with_bias, without = _lin_case(M, Kd, stress)
        xf, xo = _put(o["x"])
        wf, wo = _put(o["w"])
        bf, bo = _put(o["bias"])
        for ref, bias in ((with_bias, (bf, bo)), (without, None)):
            yf, yo = _out(E.B * M)
            _lib.call("ov_linear_f32", (xf, xo), (wf, wo), bias, (yf, yo), E.B, M, Kd)
            q = E.worst(_take(yf, yo, E.B * M).view(E.B, M), ref)
            print(f"RATIO linear M={M} Kdim={Kd} stress={stress} bias={bias is not None} {q:.3f}")
            worst = max(worst, q)
    assert worst <= 1.0


# ---- sequence_mask, frame_limits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 255, 256, 257])
@pytest.mark.parametrize("binding", BINDINGS)
def test_sequence_mask(monkeypatch, binding, T):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    lengths = torch.tensor([-3, 0, 1, T - 1, T, T + 5, 1 << 40])
    want = torch.from_numpy(E.sequence_mask(lengths, T))
    for ld in (0, (T + 3) // 4 * 4 + 4):
        mf, mo = _out(7 * (ld or T))
        _lib.call("ov_sequence_mask_f32", lengths.to(DEV), (mf, mo), 7, T, ld)
        _expect(mf, mo, (7, ld or T), want, f"sequence_mask T={T} ld={ld}")      # pad columns and guards stay NaN


@pytest.mark.parametrize("margin", [0, 14])
@pytest.mark.parametrize("Bn", [1, 256, 257])
@pytest.mark.parametrize("binding", BINDINGS)
def test_frame_limits(monkeypatch, binding, Bn, margin):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    T = 100
    pattern = [T - margin - 1, -5, 0, T - margin, T, 1 << 40, 1, (1 << 31) + 7]
    lengths = torch.tensor([pattern[b % len(pattern)] for b in range(Bn)])
    limits = torch.full((Bn + 1,), -7777, dtype=torch.int32, device=DEV)
    _lib.call("ov_frame_limits_i32", lengths.to(DEV), limits, Bn, T, margin)
    torch.cuda.synchronize()
    got = limits.cpu()
    ok = np.array_equal(got[:Bn].numpy(), E.frame_limits(lengths, T, margin)) and got[Bn].item() == -7777
    print(f"EXACT frame_limits B={Bn} margin={margin}: {'equal' if ok else 'DIFFERENT'}")
    assert ok


# ---- unpad_rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,T,ld", [(1, 1, 1), (5, 255, 256), (5, 256, 260), (5, 257, 260), (65535, 1, 4), (65536, 1, 4),
                                       (65539, 3, 4)])
@pytest.mark.parametrize("binding", BINDINGS)
def test_unpad_rows(monkeypatch, binding, rows, T, ld):
    """The last two shapes cross the launcher's loop over grid.y (65535 rows per launch), as the latents of a batch of 114
    do."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    src = E.rand(rows, ld, seed=rows + T)
    src[:, T:] = NAN                                       # a pad column read as data shows
    sf, so = _put(src)
    df, do = _out(rows * T)
    _lib.call("ov_unpad_rows_f32", (sf, so), (df, do), rows, T, ld)
    _expect(df, do, (rows, T), torch.from_numpy(E.unpad_rows(src, rows, T, ld)), f"unpad_rows rows={rows} T={T} ld={ld}")


@pytest.mark.parametrize("binding", BINDINGS)
def test_unpad_rows_refusals(monkeypatch, binding):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    src, dst = torch.zeros(64, device=DEV), torch.full((64,), NAN, device=DEV)
    _refused("ov_unpad_rows_f32", src, dst, 4, 8, 7, untouched=[dst])          # ld < T
    _refused("ov_unpad_rows_f32", src, dst, 0, 8, 8, untouched=[dst])
    _refused("ov_unpad_rows_f32", src, dst, -1, 8, 8, untouched=[dst])


# ---- stitch_window_cores ------------------------------------------------------------------------------------------------------------
STITCH_TW = 8


def _stitch_records(F0):
    """(first_frame, core_lo, core_hi) in absolute frames for an output that covers frames [F0, F0 + 24): good records
    interleaved with one record per refusal of the header."""
    return [[F0, F0 + 1, F0 + 5],              # an ordinary core
            [F0 + 6, F0 + 5, F0 + 8],          # refused: lo < first_frame
            [F0 + 6, F0 + 6, F0 + 14],         # the whole window
            [F0 + 14, F0 + 16, F0 + 15],       # refused: hi < lo
            [F0 + 14, F0 + 15, F0 + 15],       # an empty core
            [F0 + 14, F0 + 15, F0 + 23],       # refused: hi > first_frame + Tw
            [F0 - 3, F0 - 1, F0 + 1],          # refused: lo < out_frame0
            [F0 + 18, F0 + 20, F0 + 25],       # refused: would end beyond out_len
            [F0 + 16, F0 + 20, F0 + 24]]       # ends exactly at out_len


@pytest.mark.parametrize("F0", [0, 5])
@pytest.mark.parametrize("binding", BINDINGS)
def test_stitch_window_cores(monkeypatch, binding, F0):
    """Both templates: spf = 256 aligned (16-byte), the same with ``out`` one float past a 16-byte boundary (per-sample),
    spf = 3 (per-sample), spf = 260 (16-byte; a core of 4 frames is 260 vectors: the second block is partial)."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    recs = _stitch_records(F0)
    W = len(recs)
    rec_dev = torch.tensor(recs, device=DEV)
    results = {}
    for spf, shift in ((256, 0), (256, 1), (3, 0), (260, 0)):
        guard = (2 * spf + 3) // 4 * 4 + 4                # a wrongly accepted record lands in the guard, not beyond it
        out_len = 24 * spf
        o_hat = E.rand(W, STITCH_TW * spf, seed=spf)
        hf, ho = _put(o_hat)
        of, oo = _out(out_len, shift, guard)
        _lib.call("ov_stitch_window_cores_f32", (hf, ho), rec_dev, W, STITCH_TW, spf, (of, oo), out_len, F0)
        want = E.stitch_window_cores(o_hat, recs, STITCH_TW, spf, np.full(out_len, np.nan, np.float32), F0)
        assert np.isfinite(want).sum() == (4 + 8 + 4) * spf
        results[(spf, shift)] = _expect(of, oo, (out_len,), torch.from_numpy(want),
                                        f"stitch_window_cores spf={spf} shift={shift} out_frame0={F0}")
    assert _same_bits(results[(256, 0)], results[(256, 1)])


@pytest.mark.parametrize("binding", BINDINGS)
def test_stitch_window_cores_argument_checks(monkeypatch, binding):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    o_hat, out = torch.zeros(64, device=DEV), torch.full((64,), NAN, device=DEV)
    recs = torch.tensor([[0, 0, 8]], device=DEV)
    for a in ((1, 0, 8, out, 64, 0), (1, 8, 0, out, 64, 0), (0, 8, 8, out, 64, 0), (1, 8, 8, out, 0, 0),
              (1, 8, 8, out, 64, -1), (1, 8, 8, None, 64, 0)):
        _refused("ov_stitch_window_cores_f32", o_hat, recs, *a, untouched=[out])


# ---- framing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 3, 64, 65, 256])
@pytest.mark.parametrize("binding", BINDINGS)
def test_framing_against_the_gather_mirror(monkeypatch, binding, hop):
    """All three entry points against ``E.frame_hops`` (ypad built explicitly): n = pad + 1 (the shortest waveform the
    reflection is defined on), frames past the padded end, hops that are no multiple of the 32 / 64 tiles, U % 4 != 0 and
    U % 32 in {31, 1, 0}, first frames beyond the end and at 2^40, spans of a NaN-separated pool at three alignments and
    the three refused records."""
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    pad = (3 * hop) // 2
    for n in (pad + 1, pad + 2, 10 * hop + 7):
        waves = E.rand(E.B, n, seed=hop + n)
        for U in (31, 33, 64):
            assert hop * (U - 1) >= n + 2 * pad                     # the last frames lie past the padded end
            what = f"hop={hop} n={n} U={U}"
            u4 = (U + 3) // 4 * 4
            ld = u4 + 4
            # ov_frame_hops_f32: [B][N] dense waveforms; columns >= U are not written
            wf, wo = _put(waves)
            hf, ho = _out(E.B * hop * ld)
            _lib.call("ov_frame_hops_f32", (wf, wo), (hf, ho), E.B, n, hop, pad, U, ld)
            want = np.stack([E.frame_hops(waves[b], hop, pad, U) for b in range(E.B)])
            whole = _expect(hf, ho, (E.B, hop, ld), torch.from_numpy(want), f"frame_hops {what}")
            # ov_frame_hops_windows_f32: the one waveform alone in its buffer, so an index outside [0, n) reads NaN
            firsts = [0, 1, 7, n // hop + 50, 1 << 40]
            wf, wo = _put(waves[0])
            hf, ho = _out(len(firsts) * hop * ld)
            _lib.call("ov_frame_hops_windows_f32", (wf, wo), n, torch.tensor(firsts, device=DEV), len(firsts), hop, pad, U,
                      ld, (hf, ho))
            want = E.frame_hops_windows(waves[0], firsts, hop, pad, U)
            assert (want[3:] == 0).all()
            zeros = torch.zeros(len(firsts), hop, u4 - U)
            win = _expect(hf, ho, (len(firsts), hop, ld), [(slice(0, U), torch.from_numpy(want)), (slice(U, u4), zeros)],
                          f"frame_hops_windows {what}")
            # ov_frame_hops_multi_f32: three spans at bases 0, 1 and 3 floats off alignment, NaN between them
            b1 = n + 4 + (1 - (n + 4)) % 4
            b2 = b1 + n + 4 + (3 - (b1 + n + 4)) % 4
            pool = torch.full((b2 + n + 2,), NAN)
            pool[:n], pool[b1:b1 + n], pool[b2:b2 + n] = waves[0], waves[1], waves[2]
            assert b1 % 4 == 1 and b2 % 4 == 3 and b1 - n >= 4
            recs = [[0, n, 0], [b1, n, 1], [b2, n, 7], [-1, n, 0], [0, pad, 0], [b2, len(pool) - b2 + 1, 0]]
            pf, po = _put(pool)
            hf, ho = _out(len(recs) * hop * ld)
            _lib.call("ov_frame_hops_multi_f32", (pf, po), len(pool), torch.tensor(recs, device=DEV), len(recs), hop, pad, U,
                      ld, (hf, ho))
            want = E.frame_hops_multi(pool, recs, hop, pad, U)
            assert (want[3:] == 0).all() and np.isfinite(want).all()
            zeros = torch.zeros(len(recs), hop, u4 - U)
            multi = _expect(hf, ho, (len(recs), hop, ld), [(slice(0, U), torch.from_numpy(want)), (slice(U, u4), zeros)],
                            f"frame_hops_multi {what}")
            # first_frame = 0: the three kernels write the same plane
            assert torch.equal(win[0, :, :U], whole[0, :, :U]) and torch.equal(multi[0, :, :U], whole[0, :, :U])


@pytest.mark.parametrize("binding", BINDINGS)
def test_framing_argument_checks(monkeypatch, binding):
    monkeypatch.setenv("OPENVOICE_AMD_BINDING", binding)
    wave, hops = torch.zeros(64, device=DEV), torch.full((256,), NAN, device=DEV)
    first = torch.zeros(1, dtype=torch.int64, device=DEV)
    _refused("ov_frame_hops_f32", wave, hops, 1, 8, 4, 8, 4, 8, untouched=[hops])                      # pad >= N
    _refused("ov_frame_hops_f32", wave, hops, 1, 8, 4, 6, 8, 4, untouched=[hops])                      # ld < U
    _refused("ov_frame_hops_windows_f32", wave, 8, first, 1, 4, 8, 4, 8, hops, untouched=[hops])       # pad >= n_samples
    _refused("ov_frame_hops_windows_f32", wave, 8, first, 1, 4, 6, 8, 4, hops, untouched=[hops])       # ld < U
    _refused("ov_frame_hops_multi_f32", wave, 0, torch.zeros(3, dtype=torch.int64, device=DEV), 1, 4, 6, 4, 8, hops,
             untouched=[hops])                                                                         # pool_len <= 0
