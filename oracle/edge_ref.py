"""ORACLE (test infrastructure, never the product path): mirrors of the waveform-edge kernels of
openvoice_amd/csrc/ov_api.hip and openvoice_amd/csrc/longform.hip, and an element-wise acceptance limit for the two that
compute.  Plain PyTorch / numpy on the CPU; only ``tests/`` imports it (tests/test_edge_criterion_cpu.py,
tests/test_gpu_edge_kernels.py).  ``Ref``, ``ratio``, ``worst`` and ``rand`` are oracle/fp32_ref.py's.

The two kernels that compute
----------------------------
``ov_conv_post_tanh_f32`` / ``ov_conv_post_tanh_limited_f32`` (16-byte path and per-sample path alike):

    ref    = tanh(pre),  pre = sum_{c, j} w[c][j] * v[c][t + j - (K - 1) / 2],  zero outside [0, L)
    v      = fp32(lrelu(x, slope)): the fp32 product is a storage point of the kernel, so the mirror rounds it too
    absacc = sum |w| |v|
    lim    = S_POST * absacc + T_TANH * 2^-24 * |ref|

tanh is 1-Lipschitz, so the error of the pre-activation passes through unchanged; tanhf's own error is relative.  Where
absacc = 0 (an all-zero item, or zero channels only) lim = 0: tanh(0) must be exactly 0.  A limited launch is mirrored by
``limit=``: beyond the limit ref = 0 and lim = 0.

``ov_linear_f32``:   ref = sum_k w[m][k] x[b][k] + bias[m],  absacc = sum |w| |x| + |bias|,  lim = S_LIN * absacc.

The kernels that copy
---------------------
``sequence_mask``, ``frame_limits``, ``unpad_rows``, ``stitch_window_cores`` (with the refusal rule of
include/openvoice_amd.h), ``frame_hops``, ``frame_hops_windows`` and ``frame_hops_multi`` are exact: integer index
arithmetic on numpy arrays, no float operation, to be met bit for bit.  The framing mirrors are written from the
header's definition -- reflect-pad by ``pad`` (``numpy.pad(mode="reflect")``), zero beyond, hops[c][u] =
ypad[hop (f0 + u) + c] -- and never restate the kernels' ``k = i < 0 ? -i : ...``.

The allowances -- measured, reference against reference, never from a kernel
----------------------------------------------------------------------------
``python -m oracle.edge_ref`` prints them.  Each constant is 4 x the largest measured value: the margin the project
takes for "the same arithmetic in a slightly different instruction order or libm" (oracle/fp32_ref.py, S32).  It is
never widened to make a kernel pass.

``S_POST``: max |pre_fp32 - pre_f64| / absacc.  pre_fp32 restates the kernels' own order in fp32: c outer, j inner, one
fmaf per term, rounded to fp32 after each (``conv_post_chain``).  The fma is a float64 multiply-add of fp32 operands
rounded to fp32: the float64 intermediate can differ from a true fma by a double rounding (the float64 sum is itself
rounded before the fp32 rounding), which moves a result by at most one fp32 ulp in rare ties and is far inside the
factor 4.  Every (C, K, L) of the GPU file (``POST_SHAPES``), seeds 0 .. 4, benign and stress data, B = 3:

    K = 1   C = 1   5.91e-08   C = 32   3.11e-07   C = 33   4.11e-07
    K = 3   C = 1   1.52e-07   C = 32   3.89e-07   C = 33   3.24e-07
    K = 7   C = 1   2.06e-07   C = 32   3.82e-07   C = 33   3.74e-07      (the lengths of both paths)
    K = 9   C = 1   2.17e-07   C = 32   3.27e-07   C = 33   3.55e-07
    largest 4.113e-07 (C = 33, K = 1, L = 1023; about 7 fp32 roundings of absacc -- one term alone, C = 1 and K = 1, is
    one rounding, 5.91e-08, and the chains of 32 and more terms all sit between 3e-07 and 4e-07)

    S_POST = 4 * 4.113e-07 = 1.645e-06

``T_TANH``: max |tanh_fp32(p) - tanh_f64(p)| / (2^-24 |tanh_f64(p)|) of PyTorch's CPU fp32 tanh on a dense grid of
fp32 p, both signs (``tanh_grid``): 400 001 points linear in [-20, 20] and 200 000 logarithmic in |p| from 1e-6 to 20;
tanh_fp32(0) = 0 exactly is checked separately.

    linear grid 1.054    logarithmic grid 1.054    largest 1.054 (half an fp32 ulp is 1 in this unit at the lower end
    of a binade: PyTorch's CPU tanh is nearly correctly rounded)

    T_TANH = 4 * 1.054 = 4.216

``S_LIN``: max |y_fp32 - y_f64| / absacc.  y_fp32 restates ``linear_kernel``: 64 lane partials, each a sequential fmaf
over k = lane, lane + 64, ...; the xor-butterfly additions (offsets 32, 16, 8, 4, 2, 1: fp32 adds, the same value in
every lane because fp32 addition commutes); then + bias, or + 0 without one (``linear_chain``).  Every (M, Kdim) of
the GPU file (``LIN_SHAPES``), seeds 0 .. 4, benign and stress data, with and without bias, B = 3:

    (1, 1) 6.12e-08   (3, 63) 3.81e-08   (4, 64) 4.46e-08   (5, 65) 3.83e-08   (7, 33) 7.56e-08
    (256, 513) 2.82e-08   (1536, 256) 4.86e-08
    largest 7.558e-08 (M = 7, Kdim = 33: lanes with one term each, so the butterfly's adds round at the full sum; the
    long rows average their roundings out)

    S_LIN = 4 * 7.558e-08 = 3.023e-07
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.fp32_ref import EPS, F32, F64, Ref, f32, rand, ratio, worst  # noqa: F401  (re-exported for the two test files)

S_POST = 4 * 4.113e-07      # 4 x the largest measured value (docstring); never widened to make a kernel pass
T_TANH = 4 * 1.054          # the same, in units of 2^-24 |tanh|
S_LIN = 4 * 7.558e-08       # the same
S_POST_SET_BY, S_LIN_SET_BY = (33, 1, 1023), (7, 33)

# ---- the shapes both test files run -----------------------------------------------------------------------------------
B = 3
SLOPE = 0.01                                             # the product's in_slope (reference openvoice/models.py:287)
POST_VEC_LS = (4, 8, 12, 1020, 1024, 1028, 2052)         # 16-byte path: K = 7, L % 4 == 0, aligned bases
POST_LS = (1, 2, 3, 5, 255, 256, 257, 1023, 1025)        # per-sample path
POST_CS = (1, 32, 33)
POST_KS = (1, 3, 7, 9)
POST_SHAPES = tuple((C, 7, L) for C in POST_CS for L in POST_VEC_LS) + \
    tuple((C, K, L) for C in POST_CS for K in POST_KS for L in POST_LS)
LIN_SHAPES = ((1, 1), (3, 63), (4, 64), (5, 65), (7, 33), (256, 513), (1536, 256))


# ---- operands (seeded; the tests and the tables use these and nothing else) ---------------------------------------------
def post_operands(C, K, L, seed=0, stress=False, batch=B):
    """x [batch, C, L], w [C, K] at scale (C K)^-1/2, so most |pre| <~ 2 and one dropped tap is far above the limit.
    ``stress`` (batch = 3): item 0 negative only (every term goes through the slope product), its last channel exact
    zeros when C > 1; item 1 scaled by 60 so that |pre| reaches 20 and beyond (tanh saturates); item 2 all zeros
    (lim = 0: the output must be exactly 0)."""
    s = 100 * seed + 9000 + 10 * K + C
    x, w = rand(batch, C, L, seed=s + 1), rand(C, K, seed=s + 2, scale=(C * K) ** -0.5)
    if stress:
        x[0] = -x[0].abs() * 30.0                          # x 30: the slope product still leaves |pre| of order 0.3
        if C > 1:
            x[0, C - 1] = 0.0
        x[1] *= 60.0
        x[2] = 0.0
    return dict(x=x, w=w)


def linear_operands(M, Kdim, seed=0, stress=False, batch=B):
    """x [batch, Kdim], w [M, Kdim] at scale Kdim^-1/2, bias [M].  ``stress``: item 1 x 1e3, item 2 all zeros (the output
    is the bias)."""
    s = 100 * seed + 9500 + M + Kdim
    o = dict(x=rand(batch, Kdim, seed=s + 1), w=rand(M, Kdim, seed=s + 2, scale=Kdim ** -0.5), bias=rand(M, seed=s + 3, scale=0.1))
    if stress:
        o["x"][1] *= 1e3
        o["x"][2] = 0.0
    return o


# ---- the mirrors that compute -------------------------------------------------------------------------------------------
def _lrelu(x, slope):
    """The kernels' lrelu: v > 0 ? v : v * slope, the product an fp32 value."""
    x = x.float()
    return torch.where(x > 0, x, x * f32(slope))


def conv_post_tanh(x, w, slope=SLOPE, dtype=F64, limit=None):
    """out[b][t] = tanh(sum_{c, j} w[c][j] lrelu(x[b][c][t + j - (K - 1) / 2])) -> Ref of [B, L] tensors.
    ``dtype`` = float32: the honest stand-in, ``F.conv1d`` in fp32 and ``torch.tanh``.  ``limit`` [B] sample counts:
    out[b][limit[b]:] = 0 with lim = 0 (ov_conv_post_tanh_limited_f32 at col_limit * col_limit_scale)."""
    K = w.shape[-1]
    assert K % 2 == 1
    v = _lrelu(x, slope)
    pre = F.conv1d(v.to(dtype), w.to(dtype)[None], padding=(K - 1) // 2)[:, 0]
    a = F.conv1d(v.to(F64).abs(), w.to(F64).abs()[None], padding=(K - 1) // 2)[:, 0]
    ref = torch.tanh(pre)
    ref64 = ref if dtype == F64 else torch.tanh(F.conv1d(v.to(F64), w.to(F64)[None], padding=(K - 1) // 2)[:, 0])
    if limit is not None:
        keep = torch.arange(x.shape[-1])[None, :] < torch.as_tensor(limit)[:, None]
        ref, ref64, a = ref * keep, ref64 * keep, a * keep
    return Ref(ref, a, S_POST * a + T_TANH * EPS * ref64.abs())


def linear(x, w, bias=None, dtype=F64):
    """y[b][m] = sum_k w[m][k] x[b][k] + bias[m] -> Ref of [B, M] tensors.  ``dtype`` = float32: x @ w.T + b in fp32."""
    y = x.to(dtype) @ w.to(dtype).t()
    a = x.to(F64).abs() @ w.to(F64).abs().t()
    if bias is not None:
        y, a = y + bias.to(dtype)[None], a + bias.to(F64).abs()[None]
    return Ref(y, a, S_LIN * a)


# ---- fp32 restatements of the kernels' own order (what S_POST and S_LIN are measured on) --------------------------------
def _fma32(a, b, c):
    """fp32(a * b + c) through float64: the product of two fp32 values is exact in float64, the sum is rounded to float64
    and then to fp32 (the double rounding the docstring mentions)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def conv_post_chain(x, w, slope=SLOPE):
    """The pre-activation in the kernels' order: c outer, j inner, acc = fmaf(w[c][j], v[c][t + j - pad], acc); a term
    outside [0, L) leaves acc as it is (per-sample path: skipped; 16-byte path: fmaf(w, 0, acc) = acc).  fp32 [B, L]."""
    Bn, C, L = x.shape
    K = w.shape[-1]
    pad = (K - 1) // 2
    v = np.zeros((Bn, C, L + 2 * pad), np.float32)
    v[:, :, pad:pad + L] = _lrelu(x, slope).numpy()
    wn = w.float().numpy()
    acc = np.zeros((Bn, L), np.float32)
    for c in range(C):
        for j in range(K):
            acc = _fma32(wn[c, j], v[:, c, j:j + L], acc)
    return torch.from_numpy(acc)


def linear_chain(x, w, bias=None, lanes=64):
    """``linear_kernel`` restated: lane partials by sequential fmaf over k = lane, lane + 64, ..., the xor butterfly, + bias
    (or + 0).  fp32 [B, M].  ``lanes`` < 64 keeps only the first lanes' partials (a wrong variant of the CPU test)."""
    xn, wn = x.float().numpy(), w.float().numpy()
    Bn, Kd = xn.shape
    M = wn.shape[0]
    part = np.zeros((Bn, M, 64), np.float32)
    for k0 in range(0, Kd, 64):
        n = min(64, Kd - k0)
        part[:, :, :n] = _fma32(wn[None, :, k0:k0 + n], xn[:, None, k0:k0 + n], part[:, :, :n])
    part[:, :, lanes:] = 0
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, :, lane ^ off]).astype(np.float32)
    b = np.zeros(M, np.float32) if bias is None else bias.float().numpy()
    return torch.from_numpy((part[:, :, 0] + b[None]).astype(np.float32))


# ---- the exact mirrors: integer index arithmetic, no float operation ---------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def sequence_mask(lengths, T):
    """mask[b][t] = t < lengths[b] ? 1 : 0 -> float32 [B, T] (lengths int64: negative and > 2^31 included)."""
    n = _np(lengths).astype(np.int64)
    return (np.arange(T, dtype=np.int64)[None, :] < n[:, None]).astype(np.float32)


def frame_limits(lengths, T, margin):
    """limits[b] = min(T, max(0, lengths[b]) + margin) -> int32 [B]."""
    n = np.maximum(_np(lengths).astype(np.int64), 0) + margin
    return np.minimum(n, T).astype(np.int32)


def unpad_rows(src, rows, T, ld):
    """dst[r][t] = src[r * ld + t] of the flat ``src`` -> [rows, T]."""
    idx = np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(T, dtype=np.int64)[None, :]
    return _np(src).reshape(-1)[idx]


def stitch_window_cores(o_hat, windows, Tw, spf, out, out_frame0=0):
    """A copy of the flat ``out`` with out[(lo - out_frame0) spf + s] = o_hat[w][(lo - f0) spf + s], s < (hi - lo) spf, for
    every record (f0, lo, hi) of ``windows`` the header does not refuse: a core that is not inside its window (lo < f0,
    hi < lo, hi > f0 + Tw) or whose samples would land outside [0, len(out)) (lo < out_frame0, (hi - out_frame0) spf >
    len(out)) copies nothing."""
    o_hat, out = _np(o_hat).reshape(len(windows), Tw * spf), _np(out).reshape(-1).copy()
    for w, (f0, lo, hi) in enumerate([tuple(int(v) for v in r) for r in _np(windows)]):
        if lo < f0 or hi < lo or hi > f0 + Tw or lo < out_frame0 or (hi - out_frame0) * spf > len(out):
            continue
        out[(lo - out_frame0) * spf:(hi - out_frame0) * spf] = o_hat[w, (lo - f0) * spf:(hi - f0) * spf]
    return out


def frame_hops(wave, hop, pad, U, first_frame=0):
    """hops[c][u] = ypad[hop (first_frame + u) + c], ypad = ``wave`` [n] reflect-padded by ``pad`` samples at both ends
    (pad < n) and zero beyond -> [hop, U].  ypad is built explicitly; the gather is done on int64 indices, so a first
    frame of 2^40 is an ordinary case (all zeros)."""
    wave = _np(wave)
    assert wave.ndim == 1 and 0 <= pad < len(wave)
    ypad = np.pad(wave, pad, mode="reflect") if pad else wave
    q = hop * (int(first_frame) + np.arange(U, dtype=np.int64))[None, :] + np.arange(hop, dtype=np.int64)[:, None]
    inside = (q >= 0) & (q < len(ypad))
    out = np.zeros((hop, U), wave.dtype)
    out[inside] = ypad[q[inside]]
    return out


def frame_hops_windows(wave, first_frames, hop, pad, U):
    """ov_frame_hops_windows_f32: the planes of ``frame_hops`` at every first frame of the ONE waveform -> [W, hop, U]."""
    return np.stack([frame_hops(wave, hop, pad, U, int(f0)) for f0 in _np(first_frames)])


def frame_hops_multi(pool, records, hop, pad, U):
    """ov_frame_hops_multi_f32: record (base, n, f0) frames pool[base : base + n] as its own waveform; base < 0, n <= pad
    or base + n > len(pool) gives an all-zero plane -> [W, hop, U]."""
    pool = _np(pool)
    planes = []
    for base, n, f0 in [tuple(int(v) for v in r) for r in _np(records)]:
        if base < 0 or n <= pad or base + n > len(pool):
            planes.append(np.zeros((hop, U), pool.dtype))
        else:
            planes.append(frame_hops(pool[base:base + n], hop, pad, U, f0))
    return np.stack(planes)


# ---- the measurements behind S_POST, T_TANH and S_LIN -------------------------------------------------------------------
def measure_s_post(shapes=POST_SHAPES, seeds=range(5), datas=(False, True)):
    """(C, K) -> (largest |pre_fp32 - pre_f64| / absacc, the L that gave it)."""
    table = collections.OrderedDict()
    for C, K, L in shapes:
        for seed in seeds:
            for stress in datas:
                o = post_operands(C, K, L, seed, stress)
                v = _lrelu(o["x"], SLOPE)
                pre = F.conv1d(v.to(F64), o["w"].to(F64)[None], padding=(K - 1) // 2)[:, 0]
                a = F.conv1d(v.to(F64).abs(), o["w"].to(F64).abs()[None], padding=(K - 1) // 2)[:, 0]
                ok = a > 0
                q = ((conv_post_chain(o["x"], o["w"]).to(F64) - pre).abs()[ok] / a[ok]).max().item() if ok.any() else 0.0
                if q >= table.get((C, K), (0.0, L))[0]:
                    table[(C, K)] = (q, L)
    return table


def tanh_grid():
    """name -> fp32 p: linear in [-20, 20], and logarithmic in |p| from 1e-6 to 20 with both signs."""
    log = torch.logspace(-6, math.log10(20.0), 100000, dtype=F64).float()
    return collections.OrderedDict([("linear grid", torch.linspace(-20.0, 20.0, 400001, dtype=F64).float()),
                                    ("logarithmic grid", torch.cat([-log, log]))])


def measure_t_tanh():
    table = collections.OrderedDict()
    for name, p in tanh_grid().items():
        p = p[p != 0]
        t64 = torch.tanh(p.to(F64))
        table[name] = ((torch.tanh(p).to(F64) - t64).abs() / (EPS * t64.abs())).max().item()
    assert torch.tanh(torch.zeros(1)).item() == 0.0
    return table


def measure_s_lin(shapes=LIN_SHAPES, seeds=range(5), datas=(False, True)):
    table = collections.OrderedDict()
    for M, Kd in shapes:
        for seed in seeds:
            for stress in datas:
                o = linear_operands(M, Kd, seed, stress)
                for bias in (o["bias"], None):
                    r = linear(o["x"], o["w"], bias)
                    ok = r.absacc > 0
                    q = ((linear_chain(o["x"], o["w"], bias).to(F64) - r.ref).abs()[ok] / r.absacc[ok]).max().item() \
                        if ok.any() else 0.0
                    table[(M, Kd)] = max(table.get((M, Kd), 0.0), q)
    return table


def main():
    torch.set_num_threads(max(1, min(4, torch.get_num_threads())))
    sp = measure_s_post()
    print("S_POST: max |pre_fp32 - pre_f64| / absacc of the fp32 chain (c outer, j inner), seeds 0..4, benign and stress")
    for (C, K), (q, L) in sp.items():
        print(f"    C={C:<3d} K={K}   {q:.2e}   (L = {L})")
    top = max(q for q, _ in sp.values())
    print(f"    largest {top:.3e};  4 x largest = {4 * top:.3e};  module S_POST = {S_POST:.3e}")
    tt = measure_t_tanh()
    print("T_TANH: max |tanh_fp32 - tanh_f64| / (2^-24 |tanh_f64|) of PyTorch's CPU fp32 tanh")
    for name, q in tt.items():
        print(f"    {name:<18s} {q:.3f}")
    top = max(tt.values())
    print(f"    largest {top:.3f};  4 x largest = {4 * top:.3f};  module T_TANH = {T_TANH:.3f}")
    sl = measure_s_lin()
    print("S_LIN: max |y_fp32 - y_f64| / absacc of the fp32 restatement of linear_kernel, seeds 0..4, benign and stress")
    for (M, Kd), q in sl.items():
        print(f"    M={M:<5d} Kdim={Kd:<4d} {q:.2e}")
    top = max(sl.values())
    print(f"    largest {top:.3e};  4 x largest = {4 * top:.3e};  module S_LIN = {S_LIN:.3e}")


if __name__ == "__main__":
    main()
