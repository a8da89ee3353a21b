"""Host-side driver of the MI355X tone-colour-converter kernels.

``ConverterEngine`` owns the load-time weight transforms (weight-norm folding, Flip folding,
gate/posterior row pairing, transposed-conv phase split, MFMA fragment packing) and issues the
kernel launches of one ``voice_conversion`` call through the C ABI (include/openvoice_amd.h) on
torch's current HIP stream.  PyTorch is used for device memory and streams only: every op between
``spec [B,513,T]`` and ``o_hat [B,1,256T]`` is a kernel from libopenvoice_amd.so.

Reference path being replaced: SynthesizerTrn.voice_conversion (openvoice/models.py:492-499) =
PosteriorEncoder (models.py:212-221) -> ResidualCouplingBlock forward with g_src and reverse with
g_tgt (models.py:390-397) -> Generator (models.py:272-291).
"""
import contextlib
import ctypes
import functools
import math
import numbers
import os

import torch

from . import _lib
from . import noise as noise_mod
from ._lib import (ConvParams, EPI_CONVT, EPI_COUPLE, EPI_GATE, EPI_LINEAR, EPI_POSTERIOR, EPI_RESSKIP,
                   F_CONVT_GROUPED, F_MASK_V, F_OUT2_INIT)
from .generator import (FINAL_LRELU_SLOPE, GENERATOR_MARGIN, LRELU_SLOPE, conv_transpose_as_conv,  # noqa: F401
                        generator_margin_frames, generator_stages, resblock_convs, samples_per_frame, scratch_per_frame)
from .params import ENC_Q_LAYERS, FLOW_LAYERS, N_FLOWS, REF_ENC_FILTERS, REF_ENC_GRU, effective_weight

LIMIT_MAX_BATCH = 256   # ovk::LIMIT_MAX_BATCH: utterances per launch the kernels' prefix table holds


# What the kernel library has instances for (csrc/conv1d_inst_*.hip; everything else returns OV_E_UNSUPPORTED at the
# first launch -- validate_config says so at load time, by field name, before any weight is packed).
SUPPORTED_RESBLOCK_KERNELS = (3, 7, 11)
SUPPORTED_RESBLOCK_DILATIONS = (1, 3, 5)


def validate_config(cfg):
    """Reject, naming the field, every hyper-parameter the kernels have no instance for.  The reference is
    config-driven (openvoice/models.py:225-270: ``resblock`` picks ResBlock1 / ResBlock2 at :242, kernel sizes, dilations
    and upsampling rates come from the JSON); this library instantiates the released family: ResBlock1, MRF kernels
    3 / 7 / 11 with dilations 1 / 3 / 5, ConvTranspose1d with kernel = 2 x stride (stride a divisor of 32), channel
    counts in whole 32-row MFMA fragments."""
    def bad(field, value, why):
        raise _lib.OvError(f"config field {field!r} = {value!r} is not supported by the MI355X kernels: {why}")

    rb = str(cfg.get("resblock", "1"))
    if rb != "1":
        bad("resblock", cfg.get("resblock"), "only ResBlock1 ('1') is built (ResBlock2 is not; reference "
            "openvoice/models.py:242, modules.py:312-357)")
    kernels, dils = list(cfg["resblock_kernel_sizes"]), [list(d) for d in cfg["resblock_dilation_sizes"]]
    if len(kernels) != len(dils) or not kernels:
        bad("resblock_dilation_sizes", cfg["resblock_dilation_sizes"], f"one dilation list per entry of "
            f"resblock_kernel_sizes ({len(kernels)}) is required")
    for k in kernels:
        if k not in SUPPORTED_RESBLOCK_KERNELS:
            bad("resblock_kernel_sizes", kernels, f"kernel size {k} has no conv instance (built: "
                f"{SUPPORTED_RESBLOCK_KERNELS})")
    for d in dils:
        for v in d:
            if v not in SUPPORTED_RESBLOCK_DILATIONS:
                bad("resblock_dilation_sizes", dils, f"dilation {v} has no conv instance (built: "
                    f"{SUPPORTED_RESBLOCK_DILATIONS})")
    rates, uk = list(cfg["upsample_rates"]), list(cfg["upsample_kernel_sizes"])
    if len(rates) != len(uk) or not rates:
        bad("upsample_kernel_sizes", uk, f"one kernel size per entry of upsample_rates ({len(rates)}) is required")
    for (i, cin, ch, u, *_), k in zip(generator_stages(cfg), uk):
        if k != 2 * u:
            bad("upsample_kernel_sizes", uk, f"stage {i}: the transposed conv is built as a 3-tap phase conv, which needs "
                f"kernel == 2 * stride (got kernel {k}, stride {u})")
        if u <= 0 or 32 % u != 0:
            bad("upsample_rates", rates, f"stage {i}: stride {u} must divide 32 (phases are interleaved inside one "
                f"32-row fragment)")
        if cin % 2 != 0 or ch % 32 != 0:
            bad("upsample_initial_channel", cfg["upsample_initial_channel"], f"stage {i} would have {ch} channels; "
                f"every stage needs a multiple of 32 (whole MFMA fragments)")
    if cfg["hidden_channels"] % 32 != 0:
        bad("hidden_channels", cfg["hidden_channels"], "must be a multiple of 32 (the WaveNet gate rows are paired in "
            "32-row MFMA fragments)")
    if cfg["inter_channels"] % 64 != 0:
        bad("inter_channels", cfg["inter_channels"], "must be a multiple of 64 (the couplings split the channels in halves "
            "of whole 32-row fragments)")


def on_own_device(method):
    """Run an engine method with the engine's device current: kernels go to ``current_stream(self.device)`` already,
    but event records (profile mode), HIP-graph capture and the per-device launch sizing inside the library follow
    the CURRENT device, which need not be the engine's (``ToneColorConverter(cfg, device='cuda:1')`` while cuda:0 is
    current)."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        dev = getattr(self, "device", None)
        if dev is None:      # GraphedConversion: the engine is an attribute, or the first constructor argument
            dev = (getattr(self, "engine", None) or kwargs.get("engine") or args[0]).device
        with torch.cuda.device(dev):
            return method(self, *args, **kwargs)
    return wrapper


def wavenet_keyword(method):
    """Gives a public method the keyword-only ``wavenet=None | "fp32" | "bf16"``: the kernels of the WaveNet layers of
    the posterior encoder and the flow for the launches the call issues (``ConverterEngine.wavenet_scope`` on every
    engine of ``self._wavenet_cores()``).  None follows ``use_bf16_wavenet``; a string chooses for this call without
    touching the switch; anything else is an ``OvError``.  Independent of ``generator=``."""
    @functools.wraps(method)
    def wrapper(self, *args, wavenet=None, **kwargs):
        if _lib.check_wavenet(wavenet, optional=True) is None:
            return method(self, *args, **kwargs)          # the default: today's call, nothing looked up
        with contextlib.ExitStack() as stack:
            for core in self._wavenet_cores():
                stack.enter_context(core.wavenet_scope(wavenet))
            return method(self, *args, **kwargs)
    wrapper.__doc__ = (method.__doc__ or "") + ("\n        ``wavenet`` (keyword only): None follows ``use_bf16_wavenet``; "
                                               "``\"fp32\"`` / ``\"bf16\"`` choose the WaveNet layers' kernels for this call "
                                               "(``engine.wavenet_keyword``).")
    return wrapper


def _ptr(t, offset_elems=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_elems)


class PackedConv:
    """One conv layer in kernel-ready form: fragment-packed weights + bias in packed row order."""

    def __init__(self, w_dense, bias, device, K, dil=1, cout=None):
        w_dense = w_dense.detach().to(torch.float32).cpu().contiguous()
        rows, cin, k = w_dense.shape
        assert k == K
        self.rows = rows                        # meaningful packed rows (M of the launch)
        self.cout = rows if cout is None else cout
        self.cin, self.K, self.dil = cin, K, dil
        n = _lib.call("ov_conv1d_pack_size", rows, cin, K)
        packed = torch.empty(n, dtype=torch.float32)
        _lib.call("ov_conv1d_pack_f32", w_dense, rows, cin, K, packed)
        self.w = packed.to(device)
        pack_rows = _lib.call("ov_conv1d_pack_rows", rows)
        b = torch.zeros(pack_rows, dtype=torch.float32)
        if bias is not None:
            b[:rows] = bias.detach().float().cpu()
        self.has_bias = bias is not None
        self.bias = b.to(device)


def padded_frames(T):
    """Row stride of the frame-rate tensors inside the engine: T rounded up to 4 floats so that every
    row starts 16-byte aligned and the conv kernels take their 16-byte staging path for any T."""
    return (T + 3) // 4 * 4


def item_tau(B, tau, device=None):
    """The ``tau=`` of a conversion of ``B`` items (the conversion's counterpart of ``tts_engine.item_controls``, which
    re-exports it; it lives here because ``tts_engine`` imports this module).  Returns

    * a float for one number (or a zero-dimensional tensor / array): the launch scalar, ``scale_b`` stays NULL;
    * a list of ``B`` floats for a sequence, an array or a HOST tensor of ``B`` numbers, each checked to be finite;
    * the tensor itself for a 1-D float32 DEVICE tensor of ``B`` values (on ``device`` when that is given): it is used
      as it is and its values are not read, so that nothing synchronises.

    ``OvError`` on anything else: a wrong length, a bool or a string (alone or as an element), a non-finite element, a
    device tensor of another dtype, rank or device."""
    def bad(why):
        raise _lib.OvError(f"tau must be one number or one finite number per item ({B}): {why}")

    if isinstance(tau, (bool, str, bytes)):
        bad(f"got {tau!r}")
    if isinstance(tau, numbers.Real) or (hasattr(tau, "ndim") and tau.ndim == 0):
        return float(tau)
    if isinstance(tau, torch.Tensor):
        if tau.ndim != 1 or tau.shape[0] != B:
            bad(f"got a tensor of shape {tuple(tau.shape)}")
        if tau.is_cuda:
            if tau.dtype != torch.float32:
                bad(f"a device tensor must be float32, got {tau.dtype}")
            if device is not None and tau.device != torch.device(device):
                bad(f"the tensor is on {tau.device}, the conversion runs on {device}")
            return tau.contiguous()
        if not (tau.dtype.is_floating_point or tau.dtype in (torch.int8, torch.int16, torch.int32, torch.int64)):
            bad(f"got a tensor of {tau.dtype}")
        vals = tau.tolist()
    else:
        try:
            vals = list(tau)
        except TypeError:
            bad(f"got {type(tau).__name__}")
    if len(vals) != B:
        bad(f"got {len(vals)} values")
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            bad(f"element {v!r}")
        if not math.isfinite(v):
            bad(f"non-finite element in {vals}")
    return [float(v) for v in vals]


def rows_tau(taus):
    """The ``tau`` of one launch from the taus of its rows: the number itself when the rows agree (the scalar launch,
    which a captured graph can serve), else the list (one value per row: ``ov_conv1d_params.scale_b``)."""
    taus = [float(t) for t in taus]
    return taus[0] if all(t == taus[0] for t in taus) else taus


def ref_enc_lengths(T, n_convs=len(REF_ENC_FILTERS)):
    """Frames an item of ``T`` spectrogram frames has at the input of each ReferenceEncoder conv and after the last one:
    ``[T, T1, ..., T_n]`` with ``T_{k+1} = (T_k - 1) // 2 + 1`` (3x3, stride 2, padding 1; reference
    openvoice/models.py:361-364 ``calculate_channels``).  ``T_n`` is the number of GRU steps."""
    T = int(T)
    if T < 1:
        raise ValueError(f"ref_enc_lengths: T must be >= 1, got {T}")
    out = [T]
    for _ in range(n_convs):
        out.append((out[-1] - 1) // 2 + 1)
    return out


def gate_row_order(hidden):
    """Packed row order pairing row c (tanh | m) with row c+hidden (sigmoid | logs) in adjacent
    32-row MFMA tiles, so both halves of a gate land in the same lane of one wave."""
    assert hidden % 32 == 0
    idx = []
    for q in range(hidden // 32):
        idx += list(range(32 * q, 32 * q + 32)) + list(range(hidden + 32 * q, hidden + 32 * q + 32))
    return torch.tensor(idx, dtype=torch.long)


def convt_row_order(cout, stride):
    """Packed row order of the grouped ConvTranspose kernels (``F_CONVT_GROUPED``, include/openvoice_amd.h
    OV_EPI_CONVT): natural row ``cout*stride + phase`` of ``conv_transpose_as_conv`` -> 32-row tiles that hold ONE
    phase group each -- tile 2q the phases < stride/2 (their tap x[t+1] is all zeros), tile 2q+1 the phases >=
    stride/2 (tap x[t-1] all zeros) of the same output channels -- so the kernel skips a third of the matrix
    work.  Returns None when the shape cannot be grouped (the natural order + generic kernel are used then)."""
    s = stride
    if s == 8 and cout % 8 == 0:
        per_tile = 8          # channels per tile pair; row-in-tile = 4 * (cout % 8) + phase % 4
    elif s == 2 and cout % 32 == 0:
        per_tile = 32         # row-in-tile = cout % 32
    else:
        return None
    idx = []
    for q in range(cout // per_tile):
        for grp in range(2):
            for c in range(per_tile):
                for ph in range(s // 2):
                    idx.append((q * per_tile + c) * s + grp * (s // 2) + ph)
    return torch.tensor(idx, dtype=torch.long)


# measurement knob (A/B runs of the same process image): flag bits OR-ed into every conv launch, e.g.
# OPENVOICE_AMD_CONV_FLAGS=8 (OV_F_NO_XCD_MAP) restores the round-robin tile order
_EXTRA_CONV_FLAGS = int(os.environ.get("OPENVOICE_AMD_CONV_FLAGS", "0"))
if _EXTRA_CONV_FLAGS & ~_lib.F_NO_XCD_MAP:
    # every other bit (MASK_V, OUT2_INIT, CONVT_GROUPED) changes RESULTS; an environment variable must not do that
    raise _lib.OvError(f"OPENVOICE_AMD_CONV_FLAGS={_EXTRA_CONV_FLAGS}: only the measurement bit OV_F_NO_XCD_MAP "
                       f"({_lib.F_NO_XCD_MAP}) may be set from the environment")


def launch_conv(layer, x, x_off, x_bs, out, out_off, out_bs, B, L, epi=EPI_LINEAR, flags=0, in_slope=1.0,
                scale=1.0, res=None, res_off=0, res_bs=0, add=None, add_bs=0, out2=None, out2_bs=0, mask=None,
                bias_b=None, bias_b_off=0, bias_b_bs=0, split=0, phase_s=1, cin=None, rows=None, tiles_per_wg=0,
                x_ld=0, out_ld=0, mask_bs=0, tile=0, loaders=0, chunk=0, col_limit=None, col_limit_scale=1,
                scale_b=None, scale_b_off=0):
    """Fill ``ov_conv1d_params`` and launch on torch's current stream of ``x``'s device.
    Offsets, row strides (``*_ld``, 0 = dense) and batch strides are in elements.  ``col_limit`` (int32 [B] on the
    device) x ``col_limit_scale`` = output columns per utterance that matter: tiles beyond are not computed.
    ``scale_b`` (``EPI_POSTERIOR``; contiguous fp32 on the device, ``B`` values from element ``scale_b_off`` on): one
    ``scale`` per batch item, ``scale`` itself is then ignored; the other epilogues ignore it."""
    flags |= _EXTRA_CONV_FLAGS
    if scale_b is not None:
        if not (scale_b.dtype == torch.float32 and scale_b.is_contiguous() and scale_b_off >= 0
                and scale_b.numel() - scale_b_off >= B):
            raise _lib.OvError(f"launch_conv: scale_b must be contiguous float32 with {B} values from element "
                               f"{scale_b_off} on, got {scale_b.dtype} x {scale_b.numel()}")
        flags |= _lib.F_SCALE_B
    if _lib.use_torch_binding():
        ip = [B, layer.cin if cin is None else cin, L, x_ld, out_ld, layer.rows if rows is None else rows, layer.cout,
              layer.K, layer.dil, epi, flags, split, phase_s, tiles_per_wg, tile, loaders, chunk,
              x_bs, out_bs, res_bs, add_bs, out2_bs, bias_b_bs, mask_bs, x_off, out_off, res_off, bias_b_off,
              col_limit_scale, scale_b_off]
        _lib.torch_op("conv1d_f32", x, layer.w, layer.bias, out, res, add, out2, mask, bias_b, col_limit, scale_b, ip,
                      [in_slope, scale])
        return
    p = ConvParams()
    p.x, p.w = _ptr(x, x_off), _ptr(layer.w)
    p.bias = _ptr(layer.bias)        # zeros when the layer has no bias (the kernel always adds it)
    p.bias_b = _ptr(bias_b, bias_b_off) if bias_b is not None else None
    p.out = _ptr(out, out_off)
    p.res = _ptr(res, res_off) if res is not None else None
    p.add = _ptr(add) if add is not None else None
    p.out2 = _ptr(out2) if out2 is not None else None
    p.mask = _ptr(mask) if mask is not None else None
    p.x_bstride, p.out_bstride, p.res_bstride = x_bs, out_bs, res_bs
    p.add_bstride, p.out2_bstride, p.bias_b_bstride = add_bs, out2_bs, bias_b_bs
    p.B, p.Cin, p.L = B, layer.cin if cin is None else cin, L
    p.M = layer.rows if rows is None else rows
    p.Cout = layer.cout
    p.K, p.dil, p.epi, p.flags, p.split, p.phase_s = layer.K, layer.dil, epi, flags, split, phase_s
    p.in_slope, p.scale = in_slope, scale
    p.tiles_per_wg, p.tile, p.loaders, p.chunk = tiles_per_wg, tile, loaders, chunk
    p.x_ld, p.out_ld, p.mask_bstride = x_ld, out_ld, mask_bs
    p.col_limit = ctypes.c_void_p(col_limit.data_ptr()) if col_limit is not None else None
    p.col_limit_scale = col_limit_scale
    p.scale_b = _ptr(scale_b, scale_b_off) if scale_b is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(_lib.load().ov_conv1d_f32(ctypes.byref(p), stream), "ov_conv1d_f32")


def launch_pair(c1, c2, x, x_bs, out, out_bs, B, L, add=None, add_bs=0, scale=1.0, slope=LRELU_SLOPE, ld=0, nwg=0,
                dbg=None, col_limit=None, col_limit_scale=1):
    """One fused ResBlock1 iteration (``ov_resblock_pair_f32``): out = (c2(lrelu(c1(lrelu(x)))) + x [+ add]) * scale.
    ``c1`` / ``c2`` are the ``PackedConv`` layers of the two convs; ``out`` must not alias ``x``."""
    if _lib.use_torch_binding():
        _lib.torch_op("resblock_pair_f32", x, c1.w, c1.bias, c2.w, c2.bias, out, add, dbg, col_limit,
                      [B, c1.cin, L, ld, c1.K, c1.dil, nwg, x_bs, out_bs, add_bs, col_limit_scale], [slope, scale])
        return
    p = _lib.RespairParams()
    p.x, p.w1, p.b1, p.w2, p.b2 = _ptr(x), _ptr(c1.w), _ptr(c1.bias), _ptr(c2.w), _ptr(c2.bias)
    p.out = _ptr(out)
    p.add = _ptr(add) if add is not None else None
    p.x_bstride, p.out_bstride, p.add_bstride = x_bs, out_bs, add_bs
    p.B, p.C, p.L, p.ld, p.K, p.dil, p.nwg = B, c1.cin, L, ld, c1.K, c1.dil, nwg
    p.slope, p.scale = slope, scale
    p.dbg = ctypes.c_void_p(dbg.data_ptr()) if dbg is not None else None
    p.col_limit = ctypes.c_void_p(col_limit.data_ptr()) if col_limit is not None else None
    p.col_limit_scale = col_limit_scale
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(_lib.load().ov_resblock_pair_f32(ctypes.byref(p), stream), "ov_resblock_pair_f32")


_pair_supported = {}


def pair_supported(C, K, dil):
    key = (C, K, dil)
    if key not in _pair_supported:
        _pair_supported[key] = bool(_lib.call("ov_resblock_pair_supported", C, K, dil))
    return _pair_supported[key]


# Where the fused pair beats its two launches on MI355X (profiles/r02_s5_pair_vs_two_launches.txt, B = 32 x 10 s):
# C = 32, k = 3: 0.91 vs 1.09 ms; C = 32, k = 7: 1.75 vs 1.85; C = 64, k = 3: 1.60 vs 1.64.  The MFMA-bound shapes
# (C = 32 k = 11, C = 64 k = 7) run 4-9 % SLOWER fused (32 accumulator registers per wave instead of 64: less matrix
# work per LDS operand) and stay on the two-launch path.  Round 6: at C = 64, k = 3 two Winograd-domain launches (0.56 +
# 0.73 ms, profiles/r06_s17) beat the fused direct pair (1.62 ms), so that shape left the policy.
PAIR_POLICY = {(32, 3), (32, 7)}


def wino_policy(C, K, dil):
    """Where a Winograd-domain launch (csrc/conv1d_wino.h) beats the direct conv it replaces (profiles/r06_s17, B = 32 x
    10 s): every instance at C >= 64; at C = 32 (K = 11, one 32-row fragment per workgroup: the input transform is shared by
    a single row fragment and its helper waves set the pace) the dilation-1 convs only (1.03 vs 1.21 ms; the dilated
    instances tie with the direct kernel and lose in the residual form)."""
    return C >= 64 or dil == 1


# A Winograd launch deals (utterance, column block, row block) items to ONE workgroup per CU; below about half of the
# chip's CUs in items the direct kernel's small tiles fill the machine better (profiles/r06_s20, r06_s21: generator stage 0,
# C = 256, 6 888 columns -- batch 1: 54 items, Winograd 0.45-0.6x the direct conv; batch 2: 108 items, 0.8-1.0x; batch 3:
# 162 items, ahead; batch 4: 216 items, 1.4-1.7x as at batch 32; every other stage has >= 216 items at batch 1 and runs
# 1.1-1.65x faster).  Batch 1 with the rule: 7.50 -> 6.18 ms.
WINO_MIN_ITEMS = 136

# Default of ConverterEngine.use_multi_launch (DESIGN.md section 8 has the measurement behind it)
USE_MULTI_LAUNCH = True

# Opt-in split-precision path (use_split_bf16x3): generator stages with at least this many channels run on ov_conv1d_split3
SPLIT_MIN_CHANNELS = 128


def _wino_mw(cout):
    return 4 if cout % 128 == 0 else (2 if cout % 64 == 0 else 1)


def wino_ncol(cout, dil):
    """Output columns of one ov_conv1d_wino_f32 N-block (csrc/conv1d_wino.h: 256 columns per matrix wave at dilation 1,
    4 * (64 // dil) * dil at dilation dil; 4 / MW column sub-blocks per workgroup)."""
    return (256 if dil == 1 else 4 * (64 // dil) * dil) * (4 // _wino_mw(cout))


def wino_items(cout, dil, B, L):
    """Work items of one ov_conv1d_wino_f32 launch: (utterance, N-block, M-block)."""
    ncol = wino_ncol(cout, dil)
    return B * ((L + ncol - 1) // ncol) * (cout // (32 * _wino_mw(cout)))


# Columns per work item of the direct kernel (csrc/conv1d_mfma.h N_BLK): the launcher picks 128, 256 or 512 by row count
# and device size.  Under a column limit a launch computes whole items, so the smallest is what skip_padding can rely on.
DIRECT_MIN_NCOL = 128


def conv_reach(family, K, dil=1):
    """(left, right): output column t of a stride-1 'same' K-tap conv run by kernel ``family`` can depend, in floating
    point and NaN propagation included, on input columns t - left .. t + right only.
    'direct' (ov_conv1d_f32), 'pair' (ov_resblock_pair_f32, per conv) and 'split3' (ov_conv1d_split3): the taps,
    (K - 1) / 2 * dil each way.  'wino' (ov_conv1d_wino_f32): an F(4, 3) tile computes the 4 outputs r + dil (4j + i)
    from the 3 (G - 1) + 6 inputs r + dil (4j + m) - PAD dil, PAD = (K - 1) / 2 + lead (wino.LEAD_TAPS), and the inputs
    reach outputs they cancel out of only in exact arithmetic: wider than the taps.  The window's first input enters point
    0 alone (Bt row 0), which only output 0 reads (At column 0), its last one point infinity alone, which only output 3
    reads; every other input reaches all 4 outputs.  So K = 3: 3 dil each way, K = 7: 6 dil, K = 11: 7 dil back and 8 dil
    ahead (tests/test_gpu_wino.py measures it, NaN propagation included)."""
    if family in ("direct", "pair", "split3"):
        r = (K - 1) // 2 * dil
        return r, r
    if family == "wino":
        from . import wino
        G = (K + 2) // 3
        pad = (K - 1) // 2 + wino.LEAD_TAPS[K]
        return (pad + 2) * dil, (3 * (G - 1) + 4 - pad) * dil
    raise ValueError(f"unknown conv family {family!r}")


def resblock_families(C, K, dils, B, L, use_winograd=True, fuse_pairs=True):
    """Kernel family of each conv of one ResBlock1 chain (C channels, kernel K, one (dilated, plain) pair per entry of
    ``dils``) in a (B, L) launch of the fp32 generator: [(family of conv 1, family of conv 2)] with 'pair' (both convs in
    one fused launch), 'wino' or 'direct'.  The policy ConverterEngine._mrf runs -- PAIR_POLICY, wino_policy,
    WINO_MIN_ITEMS -- and the one limit_margin_frames prices; nothing else restates it."""
    from . import wino
    if fuse_pairs and L % 4 == 0 and all((C, K) in PAIR_POLICY and pair_supported(C, K, d) for d in dils):
        return [("pair", "pair")] * len(dils)
    fam = lambda d: ("wino" if use_winograd and L % 4 == 0 and wino.supported(C, C, K, d) and wino_policy(C, K, d)
                     and wino_items(C, d, B, L) >= WINO_MIN_ITEMS else "direct")
    return [(fam(d), fam(1)) for d in dils]


def limit_margin_frames(cfg, B, T, use_winograd=True, fuse_pairs=True):
    """Frames beyond an utterance's length that the fp32 generator computes under ``skip_padding`` in a (B, T) launch:
    the receptive field of ``generator_margin_frames`` with every ResBlock conv charged the reach of the kernel that runs
    it (conv_reach of resblock_families), at least GENERATOR_MARGIN.  The columns beyond the computed ones hold stale
    scratch; a Winograd conv reads 2-3 dil columns further than its taps, so a direct-only launch keeps 16 while one with
    Winograd stages needs more (tests/test_host_algebra_cpu.py simulates every launch of decode() column by column)."""
    stages = generator_stages(cfg)

    def chain_reach(i, k, dils):
        C, L = stages[i].ch, T * stages[i].rate_out
        fams = resblock_families(C, k, dils, B, L, use_winograd, fuse_pairs)
        return sum(conv_reach(f1, k, d)[1] + conv_reach(f2, k, 1)[1] for (f1, f2), d in zip(fams, dils))

    return max(GENERATOR_MARGIN, generator_margin_frames(cfg), generator_margin_frames(cfg, chain_reach=chain_reach))


def wn_fused_row_order(hidden):
    """Gate row order of the fused WaveNet-layer kernel (``ov_wn_layer_f32``, include/openvoice_amd.h): 16-row block
    q holds, at rows 4j + {0, 1, 2, 3}, the tanh rows of channels 8q + j and 8q + j + 4, then their sigmoid rows, so
    that the four accumulator rows of a lane of the 16x16x4 MFMA are both halves of two gates."""
    assert hidden % 8 == 0
    idx = []
    for q in range(hidden // 8):
        for j in range(4):
            a, b = 8 * q + j, 8 * q + j + 4
            idx += [a, b, hidden + a, hidden + b]
    return torch.tensor(idx, dtype=torch.long)


def wn_pack(w_dense, device):
    """Dense [rows][cin][K] -> the 16x16x4 fragment order of ``ov_wn_pack_f32`` (device tensor)."""
    w_dense = w_dense.detach().to(torch.float32).cpu().contiguous()
    rows, cin, k = w_dense.shape
    n = _lib.call("ov_wn_pack_size", rows, cin, k)
    assert n > 0, (rows, cin, k)
    packed = torch.empty(n, dtype=torch.float32)
    _lib.call("ov_wn_pack_f32", w_dense, rows, cin, k, packed)
    return packed.to(device)


def wn_bf16_pack(w_dense, device):
    """Dense fp32 [rows][cin][K] -> bf16 (nearest even) in the 16x16x32 fragment order of ``ov_wn_bf16_pack``: a device
    tensor of bf16 data VIEWED as float32 (``ov_wn_layer_params.w_in`` / ``w_rs`` are ``const float*`` fields)."""
    w_dense = w_dense.detach().to(torch.float32).cpu().contiguous()
    rows, cin, k = w_dense.shape
    n = _lib.call("ov_wn_bf16_pack_size", rows, cin, k)
    assert n > 0 and n % 2 == 0, (rows, cin, k)
    packed = torch.empty(n, dtype=torch.bfloat16)
    _lib.call("ov_wn_bf16_pack", w_dense, rows, cin, k, packed)
    return packed.view(torch.float32).to(device)


# The Winograd-domain layer (csrc/wn_layer_wino.hip) deals (utterance, 128-column tile) items to one workgroup per CU, in
# rounds of one item per CU, and a round costs what a full one costs (168 us per layer on 256 CUs); the direct layer
# (csrc/wn_layer.hip) chooses tiles of 16 .. 128 columns that fill the CUs whatever the batch and costs 0.9-1.0 us per 128
# columns.  Measured per layer at 861 frames (profiles/r07_wn_wino_sweep.txt), direct / Winograd in us: batch 1 (7 items)
# 22 / 169, 2 (14) 36 / 168, 4 (28) 40 / 167, 8 (56) 68 / 168, 16 (112) 119 / 169, 24 (168) 178 / 171, 32 (224) 200 / 172,
# 48 (336 = 2 rounds) 334 / 322, 64 (448) 391 / 324.  So the Winograd layer runs where its rounds are at least this full:
# 168 of 256 items per round, the smallest fill measured at which it is ahead (batch 24 and batch 48).
WN_WINO_MIN_ITEMS = 168
WN_WINO_ROUND = 256          # items of a full round: the compute units of the chip the threshold was measured on


def wn_wino_items(B, T):
    """Work items of one ov_wn_layer_wino_f32 launch: (utterance, tile of ov_wn_layer_wino_tile() = 128 columns)."""
    return B * ((T + 127) // 128)


def wn_wino_policy(B, T):
    """True where a (B, T) launch runs the Winograd-domain WaveNet layer: every round of WN_WINO_ROUND items it needs is, on
    average, at least WN_WINO_MIN_ITEMS full."""
    items = wn_wino_items(B, T)
    rounds = (items + WN_WINO_ROUND - 1) // WN_WINO_ROUND
    return items >= WN_WINO_MIN_ITEMS * rounds


def wn_wino_pack(w_dense, device):
    """Dense gate-ordered [2H][H][5] -> the transform-domain fragment stream of ``ov_wn_wino_pack_f32`` (device tensor)."""
    w_dense = w_dense.detach().to(torch.float32).cpu().contiguous()
    rows, cin, k = w_dense.shape
    n = _lib.call("ov_wn_wino_pack_size", rows, cin, k)
    assert n > 0, (rows, cin, k)
    packed = torch.empty(n, dtype=torch.float32)
    _lib.call("ov_wn_wino_pack_f32", w_dense, rows, cin, k, packed)
    return packed.to(device)


def launch_wn_layer(layer, x, out, skip, mask, B, T, ld, cond=None, cond_off=0, cond_bs=0, first=False, last=False,
                    width=0, mask_bs=0, dbg=None, acts=None, row_split=0, winograd=False, bf16=False):
    """One fused WaveNet layer (``ov_wn_layer_f32``): out = (x + res) * mask, skip (+)= rs; ``layer`` is a dict of
    the packed tensors built by ``_WaveNet``; x / out / skip are [B][H][ld].  ``acts`` ([B][H][ld] scratch) lets the
    launcher run one or two utterances as the row-split launch pair (bit-identical results); ``row_split`` 1 / 3 force
    the fused / the split form.  ``winograd``: the same layer with its gate conv in the Winograd domain
    (``ov_wn_layer_wino_f32``, ``layer["w_in_wino"]``; one launch, 128-column tiles).  ``bf16``: the same layer with its
    matrix operands rounded to bf16 and the state kept fp32 (``ov_wn_layer_bf16``, ``layer["w_in_bf16"]`` /
    ``layer["w_rs_bf16"]``; one launch; ``acts`` / ``row_split`` / ``winograd`` are ignored)."""
    entry, w_in = ("wn_layer_wino_f32", layer["w_in_wino"]) if winograd else ("wn_layer_f32", layer["w_in"])
    w_rs = layer["w_rs"]
    if bf16:
        entry, w_in, w_rs, acts, row_split = "wn_layer_bf16", layer["w_in_bf16"], layer["w_rs_bf16"], None, 0
    if _lib.use_torch_binding():
        H = layer["hidden"]
        _lib.torch_op(entry, x, out, skip, w_in, layer["b_in"], cond, w_rs, layer["b_rs"],
                      mask, dbg, acts, [B, H, T, ld, layer["K"], int(first), int(last), width, H * ld, cond_bs, mask_bs,
                                        cond_off, row_split])
        return
    p = _lib.WnLayerParams()
    p.x, p.out, p.skip = _ptr(x), _ptr(out), _ptr(skip)
    p.w_in, p.b_in, p.w_rs, p.b_rs = _ptr(w_in), _ptr(layer["b_in"]), _ptr(w_rs), _ptr(layer["b_rs"])
    p.cond = _ptr(cond, cond_off) if cond is not None else None
    p.mask = _ptr(mask)
    H = layer["hidden"]
    p.bstride, p.cond_bstride, p.mask_bstride = H * ld, cond_bs, mask_bs
    p.B, p.H, p.T, p.ld, p.K = B, H, T, ld, layer["K"]
    p.first, p.last, p.width, p.row_split = int(first), int(last), width, row_split
    p.dbg = ctypes.c_void_p(dbg.data_ptr()) if dbg is not None else None
    p.acts = _ptr(acts) if acts is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    _lib.check(getattr(_lib.load(), "ov_" + entry)(ctypes.byref(p), stream), "ov_" + entry)


class _WaveNet:
    """Packed WN stack (reference: openvoice/modules.py:133-210).  Two forms of every layer: the fused one-launch
    layer (``ov_wn_layer_f32``) where the shape has an instance, and the gate + res/skip launch pair."""

    def __init__(self, sd, prefix, n_layers, hidden, device):
        order = gate_row_order(hidden)
        self.hidden, self.n_layers = hidden, n_layers
        self.in_layers, self.rs_layers, self.fused_layers = [], [], []
        self.device, self._sd, self._prefix = device, sd, prefix      # a reference: bf16_layers() derives its weights from it
        K = sd[f"{prefix}.in_layers.0.weight_v"].shape[2] if f"{prefix}.in_layers.0.weight_v" in sd else \
            sd[f"{prefix}.in_layers.0.weight"].shape[2]
        self.fused = bool(_lib.call("ov_wn_layer_supported", hidden, K))
        forder = wn_fused_row_order(hidden) if self.fused else None
        for i in range(n_layers):
            w_in = effective_weight(sd, f"{prefix}.in_layers.{i}")
            b_in = sd[f"{prefix}.in_layers.{i}.bias"].float()
            self.in_layers.append(PackedConv(w_in[order], b_in[order], device, K=w_in.shape[2], cout=hidden))
            w_rs = effective_weight(sd, f"{prefix}.res_skip_layers.{i}")
            b_rs = sd[f"{prefix}.res_skip_layers.{i}.bias"].float()
            self.rs_layers.append(PackedConv(w_rs, b_rs, device, K=1))
            if self.fused:
                if w_rs.shape[0] == hidden:      # last layer: skip rows only (modules.py:170-173, :203-207)
                    w_rs = torch.cat([torch.zeros_like(w_rs), w_rs])
                    b_rs = torch.cat([torch.zeros_like(b_rs), b_rs])
                self.fused_layers.append(dict(hidden=hidden, K=w_in.shape[2], w_in=wn_pack(w_in[forder], device),
                                              w_in_wino=wn_wino_pack(w_in[forder], device),
                                              b_in=b_in[forder].contiguous().to(device), w_rs=wn_pack(w_rs, device),
                                              b_rs=b_rs.contiguous().to(device)))
        # cond_layer rows re-ordered per layer so its output is directly the gate's per-batch bias
        wc = effective_weight(sd, prefix + ".cond_layer")[:, :, 0]
        bc = sd[prefix + ".cond_layer.bias"].float()
        full = torch.cat([order + 2 * hidden * i for i in range(n_layers)])
        self.cond_w = wc[full].contiguous().to(device)
        self.cond_b = bc[full].contiguous().to(device)
        if self.fused:
            full = torch.cat([forder + 2 * hidden * i for i in range(n_layers)])
            self.cond_w_fused = wc[full].contiguous().to(device)
            self.cond_b_fused = bc[full].contiguous().to(device)

    def bf16_layers(self):
        """The fused layers with ``w_in_bf16`` / ``w_rs_bf16`` (``ov_wn_bf16_pack``), packed on first use -- as
        ``ConverterEngine.bf16_generator`` builds its weights -- from the same gate row order as the fp32 packing."""
        if not (self.fused and _lib.call("ov_wn_layer_bf16_supported", self.hidden, self.fused_layers[0]["K"])):
            raise _lib.OvError(f"no bf16 WaveNet layer kernel for hidden = {self.hidden}: a missing kernel is an error")
        if "w_in_bf16" not in self.fused_layers[0]:
            forder = wn_fused_row_order(self.hidden)
            for i, layer in enumerate(self.fused_layers):
                w_rs = effective_weight(self._sd, f"{self._prefix}.res_skip_layers.{i}")
                if w_rs.shape[0] == self.hidden:      # last layer: skip rows only, padded as for the fp32 packing
                    w_rs = torch.cat([torch.zeros_like(w_rs), w_rs])
                layer["w_in_bf16"] = wn_bf16_pack(effective_weight(self._sd, f"{self._prefix}.in_layers.{i}")[forder],
                                                  self.device)
                layer["w_rs_bf16"] = wn_bf16_pack(w_rs, self.device)
        return self.fused_layers


def multi_launch_scratch_buffers(cfg):
    """Decoder scratch buffers a multi-launch MRF needs beyond the workspace's t1 / ra: every ResBlock keeps a t1 and an ra of
    its own while the three run side by side (generator.scratch_per_frame sizes each)."""
    return 2 * (len(cfg["resblock_kernel_sizes"]) - 1)


_DEC_BUFFERS = 5         # decoder scratch buffers of a workspace: the stage input, the ConvTranspose output, t1 / ra, the MRF sum


def _workspace_elems(cfg, B, T):
    """Float32 elements of a ``ConverterEngine._workspace(B, T)``: ``(frame-rate tensors together, each of the _DEC_BUFFERS
    decoder scratch buffers)`` -- the one size computation behind ``_workspace`` and ``workspace_bytes``."""
    H, C, Tp = cfg["hidden_channels"], cfg["inter_channels"], padded_frames(T)
    # mask, h / h2 / acts / skip, noise, the three latents, the conv_pre output
    frame_rate = Tp + 4 * H * Tp + C * Tp + 3 * C * Tp + generator_stages(cfg)[0].cin * Tp
    return B * frame_rate, B * T * scratch_per_frame(cfg)


def _resblock_tree(sd, cfg, make, keep=lambda stage: True):
    """``[stage][ResBlock][(conv 1, conv 2) per dilation]`` of ``make(c, weight, bias, dilation)`` over
    ``resblock_convs(cfg)`` (``c``: the pair's record); None in place of a stage that ``keep(stage index)`` refuses."""
    convs = list(resblock_convs(cfg))
    layer = lambda c, name, d: make(c, effective_weight(sd, name), sd[name + ".bias"], d)
    return [[[(layer(c, f"{c.prefix}.convs1.{c.n}", c.dil), layer(c, f"{c.prefix}.convs2.{c.n}", 1))
              for c in convs if (c.stage, c.j) == (i, j)]
             for j in range(len(cfg["resblock_kernel_sizes"]))] if keep(i) else None
            for i in range(len(cfg["upsample_rates"]))]


class ConverterEngine:
    """Kernel-level implementation of the converter model for one device."""

    def __init__(self, state_dict, model_cfg, spec_channels, device, zero_g=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.OvError("ConverterEngine needs a ROCm device ('cuda:N'); there is no CPU path")
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        cfg = dict(model_cfg.items()) if hasattr(model_cfg, "items") else dict(model_cfg)
        validate_config(cfg)          # names the unsupported field before any weight is packed
        self.cfg = cfg
        self.zero_g = bool(zero_g)
        self.inter = cfg["inter_channels"]
        self.hidden = cfg["hidden_channels"]
        self.gin = cfg.get("gin_channels", 256)
        self.spec_channels = spec_channels
        dev = self.device
        H, C = self.hidden, self.inter
        half = C // 2
        # ---- posterior encoder -----------------------------------------------------------------
        self.q_pre = PackedConv(sd["enc_q.pre.weight"], sd["enc_q.pre.bias"], dev, K=1)
        self.q_wn = _WaveNet(sd, "enc_q.enc", ENC_Q_LAYERS, H, dev)
        order = gate_row_order(C)
        self.q_proj = PackedConv(sd["enc_q.proj.weight"][order], sd["enc_q.proj.bias"][order], dev, K=1, cout=C)
        # ---- flow: Flip folded into channel order of pre (inputs) / post (outputs) ---------------
        self.couplings = []
        for f in range(N_FLOWS):
            p = f"flow.flows.{2 * f}"
            flipped = f % 2 == 1   # an odd number of Flips precedes this coupling in both directions
            w_pre, w_post, b_post = sd[p + ".pre.weight"], sd[p + ".post.weight"], sd[p + ".post.bias"]
            if flipped:
                w_pre = torch.flip(w_pre, [1])
                w_post, b_post = torch.flip(w_post, [0]), torch.flip(b_post, [0])
            self.couplings.append(dict(
                flipped=flipped,
                pre=PackedConv(w_pre, sd[p + ".pre.bias"], dev, K=1),
                wn=_WaveNet(sd, p + ".enc", FLOW_LAYERS, H, dev),
                post=PackedConv(w_post, b_post, dev, K=1)))
        self.half = half
        # ---- generator -------------------------------------------------------------------------
        self.conv_pre = PackedConv(sd["dec.conv_pre.weight"], sd["dec.conv_pre.bias"], dev, K=7)
        self.dec_cond_w = sd["dec.cond.weight"][:, :, 0].contiguous().to(dev)
        self.dec_cond_b = sd["dec.cond.bias"].contiguous().to(dev)
        self.stages = generator_stages(cfg)
        self.ups = []
        for i, _, ch, u, *_ in self.stages:
            wc = conv_transpose_as_conv(effective_weight(sd, f"dec.ups.{i}"), u)
            bias = sd[f"dec.ups.{i}.bias"].repeat_interleave(u)
            order = convt_row_order(ch, u)
            if order is not None:
                wc, bias = wc[order], bias[order]
            self.ups.append(dict(conv=PackedConv(wc, bias, dev, K=3, cout=ch), stride=u,
                                 flags=F_CONVT_GROUPED if order is not None else 0))
        self.resblocks = _resblock_tree(sd, cfg, lambda c, w, b, d: PackedConv(w, b, dev, K=c.K, dil=d))
        # Winograd-domain twins (csrc/conv1d_wino.h) of the ResBlock convs of the MFMA-bound stages: the same fp32 conv
        # with 1.6-2x fewer executed multiplies; per stage / ResBlock / pair (w1 | None, w2 | None)
        from . import wino as _wino
        self.wino_resblocks = _resblock_tree(sd, cfg, lambda c, w, b, d: _wino.PackedConvWino(w, b, dev, dil=d)
                                             if _wino.supported(c.ch, c.ch, c.K, d) and wino_policy(c.ch, c.K, d) else None)
        self.final_channels = self.stages[-1].ch
        self.post_w = sd["dec.conv_post.weight"][0].contiguous().to(dev)   # [C, 7]
        self.total_upsample = samples_per_frame(cfg)
        # ---- reference encoder (extract_se): present in converter checkpoints only -------------------
        self.ref_enc = None
        if "ref_enc.gru.weight_ih_l0" in sd:
            convs = [(effective_weight(sd, f"ref_enc.convs.{i}").contiguous().to(dev),
                      sd[f"ref_enc.convs.{i}.bias"].contiguous().to(dev)) for i in range(len(REF_ENC_FILTERS))]
            w_ih = sd["ref_enc.gru.weight_ih_l0"]
            self.ref_enc = dict(
                ln_w=sd["ref_enc.layernorm.weight"].contiguous().to(dev),
                ln_b=sd["ref_enc.layernorm.bias"].contiguous().to(dev),
                convs=convs,
                gru_in=PackedConv(w_ih.unsqueeze(-1), sd["ref_enc.gru.bias_ih_l0"], dev, K=1),
                whh_t=sd["ref_enc.gru.weight_hh_l0"].t().contiguous().to(dev),
                bhh=sd["ref_enc.gru.bias_hh_l0"].contiguous().to(dev),
                proj_w=sd["ref_enc.proj.weight"].contiguous().to(dev),
                proj_b=sd["ref_enc.proj.bias"].contiguous().to(dev))
        self._ws, self._graphs, self._limit_margins = {}, {}, {}
        self._live_ws, self._live_ws_bf16, self.live_ws_builds = {}, {}, 0    # live unit scratch, per (unit, rows)
        # (B, T) workspaces kept resident at once, least recently used evicted first.  1 (the default): a new shape
        # frees the previous one.  StreamPool raises it to its ladder of launch sizes so that a varying ready count
        # does not rebuild gigabytes of decoder scratch per step (workspace_bytes() prices a shape).
        self.resident_workspaces = 1
        self.profile = None   # set to [] to collect per-launch HIP-event timings
        # independent ResBlock chains of a generator stage on this many HIP streams when the batch is at most
        # chain_streams_max_batch utterances (decode()); 1 = always the serial one-stream order
        # Measured (round 4, profiles/r04_s14_sweep_chain_ab.txt): batch 1 8.75 vs 8.81 ms, batch 4 20.4 vs 20.2 ms -- the
        # chains do overlap, but every kernel then runs proportionally longer (the chip is occupied by one-tile
        # workgroups either way) -- so the default is the serial order; results are bit-identical both ways.
        self.chain_streams = 1
        self.chain_streams_max_batch = 8
        self._streams = []
        self._zeros = {}
        # frames the generator computes beyond an utterance's length under skip_padding: this checkpoint's own
        # receptive field (larger ResBlock kernels / dilations or other upsampling than the released models' would
        # silently corrupt the last samples with a hard-wired 16)
        self.generator_margin = max(GENERATOR_MARGIN, generator_margin_frames(self.cfg))
        self.fuse_wn = True      # WaveNet layers as one launch each (ov_wn_layer_f32) where the shape has an instance
        self.wn_row_split = 0    # 0: the launcher splits a layer's rows over two launches for one or two utterances; 1: never
        self.fuse_pairs = True   # ResBlock pairs of the HBM-bound stages as one launch each (PAIR_POLICY)
        # ResBlock convs in the Winograd domain where wino_policy() says so (ov_conv1d_wino_f32):
        # fp32 arithmetic, 6 G / (4 K) of the direct form's multiplies, ~4x its rounding error
        self.use_winograd = True
        # The three ResBlocks' convs of one MRF step (k = 3 / 7 / 11, independent of each other) as ONE persistent launch
        # (ov_conv1d_wino_multi_f32) on the stages whose convs are all Winograd launches; bit-identical to the single
        # launches (False: one launch per conv, ResBlock by ResBlock)
        self.use_multi_launch = USE_MULTI_LAUNCH
        self._cus = None         # compute units of the device (read on first use)
        # opt-in fast generator: bf16 activations, fp32 accumulation (waveform within
        # ~1e-2 of the fp32 path instead of ~1e-5).  Built on first use by bf16_generator().
        self._state_dict_for_bf16 = sd
        self.generator_bf16 = None
        self._bf16_on = False
        # opt-in: the WaveNet layers of the posterior encoder and of the flow on the bf16 matrix pipe with fp32 state
        # (ov_wn_layer_bf16).  _wn_choice: a call's own wavenet= while it runs (wavenet_scope).
        self._wn_bf16_on, self._wn_choice = False, None
        # opt-in split-precision MRF stages: fp32-level products on the bf16 matrix pipe
        self._split3_on = False
        self.split3_products = 6
        self.split_resblocks = None      # per stage: None, or [[(c1, c2) PackedConvSplit3 pairs] per ResBlock]

    # ---- launch helpers --------------------------------------------------------------------------
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _timed(self, tag, flops, fn, *extra):
        """Run ``fn()``; when ``self.profile`` is a list, bracket it with HIP events on the launch stream and record
        ``(tag, algorithmic FLOPs, start, end, *extra)`` for bench.py's roofline."""
        if self.profile is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.profile.append((tag, flops, e0, e1) + extra)
        return out

    def _conv(self, layer, x, x_off, x_bs, out, out_off, out_bs, B, L, tag="conv", alg_flops=None, **kwargs):
        """Launch one conv, profiled under ``tag`` with its algorithmic FLOPs."""
        if alg_flops is None:
            alg_flops = 2.0 * layer.rows * (kwargs.get("cin") or layer.cin) * layer.K * L * B
        self._timed(tag, alg_flops, lambda: launch_conv(layer, x, x_off, x_bs, out, out_off, out_bs, B, L, **kwargs))

    def _wino(self, layer, x, out, bs, B, L, res=None, add=None, scale=1.0, in_slope=LRELU_SLOPE, out_slope=1.0, **lim):
        """One Winograd-domain ResBlock conv (leaky ReLU on the input, LINEAR epilogue); profiled under the MRF tag with its
        algorithmic FLOPs and, as a fifth field, the FLOPs the kernel EXECUTES (wino.PRODUCTS_PER_TILE[K] / (4 K) of them)."""
        from . import wino
        kw = dict(in_slope=in_slope, out_slope=out_slope, scale=scale, res=res, res_bs=bs if res is not None else 0, add=add,
                  add_bs=bs if add is not None else 0, **lim)
        alg = 2.0 * layer.cout * layer.cin * layer.K * L * B
        self._timed("mrf", alg, lambda: wino.launch_conv_wino(layer, x, bs, out, bs, B, L, **kw),
                    alg * wino.PRODUCTS_PER_TILE[layer.K] / (4.0 * layer.K))

    def _wino_multi(self, convs, B, L, **lim):
        """One ov_conv1d_wino_multi_f32 launch (``wino.launch_convs_wino``); profiled as ONE record under the MRF tag with
        the algorithmic and the executed FLOPs of all its convs."""
        from . import wino
        alg = [2.0 * c["layer"].cout * c["layer"].cin * c["layer"].K * L * B for c in convs]
        exe = sum(a * wino.PRODUCTS_PER_TILE[c["layer"].K] / (4.0 * c["layer"].K) for a, c in zip(alg, convs))
        self._timed("mrf", sum(alg), lambda: wino.launch_convs_wino(convs, B, L, **lim), exe)

    def _pair(self, c1, c2, x, out, bs, B, L, add, scale, **lim):
        """One fused ResBlock1 iteration; profiled under the same tag as the two launches it replaces, with their
        algorithmic FLOPs (both convs)."""
        self._timed("mrf", 2 * 2.0 * c1.rows * c1.cin * c1.K * L * B,
                    lambda: launch_pair(c1, c2, x, bs, out, bs, B, L, add=add, add_bs=bs, scale=scale, **lim))

    def _linear(self, x2d, w, b):
        Bg, Kd = x2d.shape
        M = w.shape[0]
        y = torch.empty(Bg, M, dtype=torch.float32, device=self.device)
        _lib.call("ov_linear_f32", x2d, w, b, y, Bg, M, Kd)
        return y

    def _wn_cond(self, wn, g):
        """cond_layer (modules.py:189-190) for every layer of ``wn`` at once, rows in the order the gate kernel in
        use expects them as its per-utterance bias."""
        if self.fuse_wn and wn.fused:
            return self._linear(g, wn.cond_w_fused, wn.cond_b_fused)
        return self._linear(g, wn.cond_w, wn.cond_b)

    def _workspace(self, B, T):
        key = (B, T)
        ws = self._ws.pop(key, None)
        if ws is not None:
            self._ws[key] = ws     # re-inserted last: the dict is the LRU order
        else:
            # resident_workspaces shapes at a time (default one: the decoder scratch is GBs at B=32); the least
            # recently used one goes first
            while self._ws and len(self._ws) >= max(1, int(self.resident_workspaces)):
                self._ws.pop(next(iter(self._ws)))
            dev, H, C = self.device, self.hidden, self.inter
            Tp = padded_frames(T)
            # zero-filled once: the pad columns [T, Tp) are never written by a kernel and never read as data
            f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
            lat = f(3, B, C, Tp)         # the three latents in ONE allocation: one ov_unpad_rows_f32 returns them dense
            ws = dict(Tp=Tp, mask=f(B, Tp), h=f(B, H, Tp), h2=f(B, H, Tp), acts=f(B, H, Tp), skip=f(B, H, Tp), noise=f(B, C, Tp),
                      lat=lat, z=lat[0], z_p=lat[1], z_hat=lat[2])
            ws["pre"] = f(B, self.stages[0].cin, Tp)
            dec = _workspace_elems(self.cfg, B, T)[1]
            ws["dec"] = [torch.empty(dec, dtype=torch.float32, device=dev) for _ in range(_DEC_BUFFERS)]
            # a multi launch keeps every ResBlock's t1 / ra live at once: part of the workspace, not of a step
            self._chain_scratch(ws, self._multi_launch_scratch(B, T))
            self._ws[key] = ws
        return ws

    def workspace_bytes(self, B, T):
        """Device bytes of the ``_workspace(B, T)`` allocation (the frame-rate tensors and the decoder scratch, the multi
        launches' ``multi_launch_scratch_buffers`` included while ``use_multi_launch`` is on; the opt-in paths' lazily added
        buffers not included)."""
        frame_rate, dec = _workspace_elems(self.cfg, B, T)
        return 4 * (frame_rate + (_DEC_BUFFERS + self._multi_launch_scratch(B, T)) * dec)

    def _zeros_like_cached(self, t):
        """An all-zero tensor of ``t``'s shape (the ``zero_g`` conditioning, models.py:495,498) without a fill launch
        per conversion."""
        key = tuple(t.shape)
        z = self._zeros.get(key)
        if z is None:
            z = self._zeros[key] = torch.zeros_like(t)
        return z

    def _side_streams(self, n):
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(self.device))
        return self._streams[:n]

    def _chain_scratch(self, ws, n):
        """``n`` more decoder scratch buffers (the t1 / ra of the ResBlocks beyond the first: concurrent chains and multi
        launches keep them live at once), allocated on first use."""
        extra = ws.setdefault("dec_extra", [])
        while len(extra) < n:
            extra.append(torch.empty_like(ws["dec"][0]))
        return extra

    def _wavenet(self, wn, ws, B, T, cond, mask):
        """h (in place) -> skip accumulator; reference: openvoice/modules.py:192-210.  The final
        ``output * x_mask`` (modules.py:210) is dropped: every consumer (proj / post) is a 1x1 conv
        whose own epilogue multiplies by the same 0/1 mask, which makes it a no-op."""
        H, Tp = wn.hidden, ws["Tp"]
        cbs = 0 if cond.shape[0] == 1 else cond.shape[1]
        if self.wavenet_bf16():
            # every layer of the stack as one ov_wn_layer_bf16 launch; use_winograd / wn_wino_policy / wn_row_split do not
            # apply.  The cond rows are in the fused gate order (_wn_cond), which this kernel shares.
            if not self.fuse_wn:
                raise _lib.OvError("wavenet='bf16' runs the fused layer kernel: fuse_wn must be on")
            layers = wn.bf16_layers()
            src, dst = ws["h"], ws["h2"]
            for i in range(wn.n_layers):
                layer, last = layers[i], i == wn.n_layers - 1
                self._timed("wn_layer_bf16", 2.0 * (2 * H * H * layer["K"] + (H if last else 2 * H) * H) * T * B,
                            lambda: launch_wn_layer(layer, src, dst, ws["skip"], mask, B, T, Tp, cond=cond,
                                                    cond_off=2 * H * i, cond_bs=cbs, first=i == 0, last=last,
                                                    mask_bs=Tp, bf16=True))
                src, dst = dst, src
            return
        if self.fuse_wn and wn.fused:
            # one launch per layer; h ping-pongs between two buffers (a tile reads its neighbours' halo columns)
            src, dst = ws["h"], ws["h2"]
            # gate conv in the Winograd domain where the launch fills the chip in whole rounds of (utterance, tile) items
            winograd = self.use_winograd and wn_wino_policy(B, T)
            for i in range(wn.n_layers):
                layer = wn.fused_layers[i]
                args = dict(cond=cond, cond_off=2 * H * i, cond_bs=cbs, first=i == 0, last=i == wn.n_layers - 1,
                            mask_bs=Tp, acts=ws["acts"], row_split=self.wn_row_split, winograd=winograd)
                rs_rows = H if args["last"] else 2 * H
                self._timed("wn_layer", 2.0 * (2 * H * H * layer["K"] + rs_rows * H) * T * B,
                            lambda: launch_wn_layer(layer, src, dst, ws["skip"], mask, B, T, Tp, **args))
                src, dst = dst, src
            return
        for i in range(wn.n_layers):
            self._conv(wn.in_layers[i], ws["h"], 0, H * Tp, ws["acts"], 0, H * Tp, B, T, epi=EPI_GATE,
                       bias_b=cond, bias_b_off=2 * H * i, bias_b_bs=cbs, rows=2 * H, x_ld=Tp, out_ld=Tp, tag="wn_in")
            last = i == wn.n_layers - 1
            self._conv(wn.rs_layers[i], ws["acts"], 0, H * Tp, ws["h"], 0, H * Tp, B, T, epi=EPI_RESSKIP,
                       flags=F_OUT2_INIT if i == 0 else 0, out2=ws["skip"], out2_bs=H * Tp, mask=mask, mask_bs=Tp,
                       split=0 if last else H, x_ld=Tp, out_ld=Tp, tag="wn_rs")

    def _flow(self, src, buf, ws, B, T, conds, mask, reverse):
        """ResidualCouplingBlock (models.py:390-397) from ``src`` into ``buf`` without a copy: a coupling rewrites one
        half of the channels (x1) and leaves the other (x0) alone, and consecutive couplings alternate halves (the
        folded Flips), so the first two couplings read their x1 operand from ``src`` and write it to ``buf`` -- after
        them every channel of ``buf`` has been written -- and the rest run in place."""
        C, half, H, Tp = self.inter, self.half, self.hidden, ws["Tp"]
        order = range(N_FLOWS - 1, -1, -1) if reverse else range(N_FLOWS)
        for n, f in enumerate(order):
            cp = self.couplings[f]
            x0_off = half * Tp if cp["flipped"] else 0
            x1_off = 0 if cp["flipped"] else half * Tp
            self._conv(cp["pre"], src if n == 0 else buf, x0_off, C * Tp, ws["h"], 0, H * Tp, B, T, flags=F_MASK_V,
                       mask=mask, mask_bs=Tp, x_ld=Tp, out_ld=Tp, tag="cpl_pre")
            self._wavenet(cp["wn"], ws, B, T, conds[f], mask)
            self._conv(cp["post"], ws["skip"], 0, H * Tp, buf, x1_off, C * Tp, B, T, epi=EPI_COUPLE, mask=mask,
                       mask_bs=Tp, x_ld=Tp, out_ld=Tp, scale=-1.0 if reverse else 1.0, tag="cpl_post",
                       res=src if n < 2 else None, res_off=x1_off, res_bs=C * Tp)

    def _wavenet_cores(self):
        return (self,)

    # ---- the path ----------------------------------------------------------------------------------
    @torch.no_grad()
    @on_own_device
    def voice_conversion(self, spec, spec_lengths, sid_src, sid_tgt, tau=1.0, noise=None, skip_padding=False, *,
                         seed=None, generator=None, wavenet=None):
        """Same contract as the reference seam (openvoice/models.py:492-499):
        ``(o_hat [B,1,256T], y_mask [B,1,T], (z, z_p, z_hat) [B,192,T])``.  ``noise`` [B,192,T]
        replaces the reference's ``torch.randn_like`` draw (models.py:220); when omitted it is drawn
        from torch's generator on the device.  ``seed`` (instead of ``noise``): counter-based noise (``noise.py``,
        purpose 0) generated straight into the workspace rows by one launch -- an int ``s`` gives row ``b`` the pair
        ``(s, b)``, a list holds one seed, pair or ``(seed, stream, first frame)`` per row (``noise.rows``).
        ``skip_padding``: the generator -- 98 % of the work, and unmasked in
        the reference, so a padded batch costs as if every utterance had the longest length -- computes only the
        first ``length + limit_margin(B, T)`` frames of each utterance (length-aware work lists,
        ``ov_conv1d_params.col_limit``); every sample of the first ``length`` frames is bit-identical to the full
        computation, and everything beyond them in ``o_hat`` is zero instead of the reference's bias-driven junk.
        ``generator``: None follows the ``use_bf16_generator`` switch; ``"fp32"`` / ``"bf16"`` choose the generator's
        kernels for this call, whatever the switch says and without touching it (the bf16 generator is built on first
        use, as for a bf16 live pool).  ``wavenet``: the same for the WaveNet layers of the posterior encoder and of the
        flow -- None follows ``use_bf16_wavenet``, ``"fp32"`` / ``"bf16"`` choose for this call (``ov_wn_layer_bf16``:
        bf16 matrix operands, fp32 state); independent of ``generator``.  ``tau``: one number for the batch, or one per
        item -- a sequence (uploaded once per call as a float32 device vector) or a 1-D float32 device tensor of ``B``
        values (used as it is, nothing synchronises); see ``item_tau``.  Per item it reaches the one place ``tau``
        enters, the ``q_proj`` epilogue, as ``ov_conv1d_params.scale_b``: the same launches as with a number, and item
        ``b`` holds the bits of the batch run with the number ``tau[b]``."""
        use_bf16 = self._bf16_on
        if _lib.check_generator(generator, optional=True) is not None:
            use_bf16 = generator == "bf16"
        with self.wavenet_scope(wavenet):
            return self._voice_conversion(spec, spec_lengths, sid_src, sid_tgt, tau, noise, skip_padding, seed, use_bf16)

    def _tau_args(self, B, tau):
        """``(scale, scale_b)`` of a ``q_proj`` launch of ``B`` rows from a ``tau=`` argument (``item_tau``)."""
        tau = item_tau(B, tau, self.device)
        if isinstance(tau, float):
            return tau, None
        if isinstance(tau, list):
            tau = torch.tensor(tau, dtype=torch.float32).to(self.device)
        return 1.0, tau

    def _voice_conversion(self, spec, spec_lengths, sid_src, sid_tgt, tau, noise, skip_padding, seed, use_bf16):
        dev = self.device
        spec = spec.to(dev, torch.float32)
        B, F, T = spec.shape
        tau = self._tau_args(B, tau)
        assert F == self.spec_channels
        # rows may be padded (the native spectrogram returns a [B, F, T] view of 16-byte aligned rows)
        if not (spec.stride(2) == 1 and spec.stride(1) >= T and spec.stride(0) >= F * spec.stride(1)):
            spec = spec.contiguous()
        C = self.inter
        lengths = spec_lengths.to(dev, torch.int64).contiguous()
        g_src = sid_src.to(dev, torch.float32).reshape(sid_src.shape[0], -1).contiguous()
        g_tgt = sid_tgt.to(dev, torch.float32).reshape(sid_tgt.shape[0], -1).contiguous()
        noise_mod.exclusive(seed, noise=noise)
        ws = self._workspace(B, T)
        Tp, mask = ws["Tp"], ws["mask"]
        if seed is not None:
            self.seed_noise(ws["noise"], seed, B, T, Tp)
        elif noise is None:
            # one launch, the RNG stream of a dense torch.randn(B, C, T) (the reference's randn_like, models.py:220):
            # the pad columns [T, Tp) are not drawn into, so a seeded conversion does not depend on the row padding
            ws["noise"][:, :, :T].normal_()
        else:
            ws["noise"][:, :, :T].copy_(noise.to(dev, torch.float32))     # into the padded-row layout
        _lib.call("ov_sequence_mask_f32", lengths, mask, B, T, Tp)
        conds = self._conds(g_src, g_tgt)
        # ---- posterior encoder + flows at frame rate ---------------------------------------------------
        # (measured and dropped: issuing this part -- ~100 launches of <= 1.3 tiles per workgroup slot -- as 2 / 4
        # independent sub-batch chains on separate HIP streams, so that one chain's tiles would fill the other's
        # launch tails, takes 16.1 / 14.0 ms instead of 12.1 ms: profiles/r02_s7_frame_streams_ab.txt)
        # Its 48 WaveNet layers run the fp32 kernels unless wavenet= / use_bf16_wavenet chooses ov_wn_layer_bf16 (_wavenet).
        self._frames(ws, 0, B, spec, conds, tau)
        z, z_p, z_hat = ws["z"], ws["z_p"], ws["z_hat"]
        # ---- generator (models.py:272-291); z_hat * y_mask is the identity (z_hat already masked) --
        if use_bf16:
            g_d = self._zeros_like_cached(g_tgt) if self.zero_g else g_tgt
            o_hat = self._timed("gen_bf16", 0.0, lambda: self.bf16_generator().decode(z_hat[:, :, :T], g_d.unsqueeze(-1)))
            if skip_padding:
                # the bf16 generator has no length-aware work lists (it computes the padded batch); the contract of
                # skip_padding -- every sample beyond an utterance's own length is zero -- is kept by masking
                keep_samples = (lengths.clamp(max=T) * self.total_upsample).view(B, 1, 1)
                o_hat.masked_fill_(torch.arange(o_hat.shape[2], device=dev).view(1, 1, -1) >= keep_samples, 0.0)
        else:
            limits = self.frame_limits(lengths, T) if skip_padding else None
            o_hat = self.decode(z_hat, conds["d"], ws, T=T, limits=limits)
        # fresh dense tensors for the caller (the workspace is reused by the next call): padded rows -> [.., T]
        dense = torch.empty(3, B, C, T, dtype=torch.float32, device=dev)
        _lib.call("ov_unpad_rows_f32", ws["lat"], dense, 3 * B * C, T, Tp)
        y_mask = torch.empty(B, 1, T, dtype=torch.float32, device=dev)
        _lib.call("ov_unpad_rows_f32", mask, y_mask, B, T, Tp)
        return o_hat, y_mask, (dense[0], dense[1], dense[2])

    def seed_noise(self, dst, seed, B, T, ld, purpose=noise_mod.PURPOSE_POSTERIOR):
        """Counter-based noise of ``seed`` (``noise.rows``: one ``(seed, stream, first frame)`` per row) into the first
        ``T`` columns of the ``[B, inter, ld]`` rows of ``dst``: one record per row, one launch, no dense temporary; the
        pad columns ``[T, ld)`` keep their contents."""
        C = self.inter
        noise_mod.fill([(s, k, purpose, f0, T, b * C * ld, ld) for b, (s, k, f0) in enumerate(noise_mod.rows(seed, B))],
                       C, dst)

    def _frames(self, ws, b0, b1, spec, conds, tau):
        """Posterior encoder and the two flow passes for the utterances [b0, b1) (views of the whole-batch workspace);
        ``tau``: the whole batch's ``(scale, scale_b)`` (``_tau_args``)."""
        nb, T, Tp = b1 - b0, spec.shape[2], ws["Tp"]
        C, H = self.inter, self.hidden
        sub = {k: (v[b0:b1] if torch.is_tensor(v) else v) for k, v in ws.items() if k != "dec"}
        rows = lambda t: t if t.shape[0] == 1 else t[b0:b1]
        mask = sub["mask"]
        x = spec[b0:b1]
        # ---- posterior encoder (models.py:212-221) -------------------------------------------------
        self._conv(self.q_pre, x, 0, spec.stride(0), sub["h"], 0, H * Tp, nb, T, flags=F_MASK_V, mask=mask, mask_bs=Tp,
                   x_ld=spec.stride(1), out_ld=Tp, tag="q_pre")
        self._wavenet(self.q_wn, sub, nb, T, rows(conds["q"]), mask)
        z, z_p, z_hat = sub["z"], sub["z_p"], sub["z_hat"]
        self._conv(self.q_proj, sub["skip"], 0, H * Tp, z, 0, C * Tp, nb, T, epi=EPI_POSTERIOR, res=sub["noise"],
                   res_bs=C * Tp, scale=tau[0], scale_b=tau[1], scale_b_off=b0, mask=mask, mask_bs=Tp, rows=2 * C, x_ld=Tp,
                   out_ld=Tp, tag="q_proj")
        # ---- flow forward with g_src, reverse with g_tgt (models.py:496-497) -----------------------
        self._flow(z, z_p, sub, nb, T, [rows(c) for c in conds["src"]], mask, reverse=False)
        self._flow(z_p, z_hat, sub, nb, T, [rows(c) for c in conds["tgt"]], mask, reverse=True)

    def graphed(self, B, T, tau, src_rows=1, tgt_rows=1, max_cached=4, skip_padding=False):
        """``voice_conversion`` for one fixed (B, T, tau) as a captured HIP graph (see ``GraphedConversion``);
        the most recent ``max_cached`` shapes stay resident.  ``tau`` is one number here: it is part of the key and a
        constant of the captured launch.  A per-item ``tau`` takes the ungraphed path (``voice_conversion``)."""
        if not isinstance(item_tau(B, tau), float):
            raise _lib.OvError("graphed: a captured conversion is keyed on one tau; a per-item tau takes the ungraphed "
                               "path (voice_conversion)")
        key = (int(B), int(T), float(tau), int(src_rows), int(tgt_rows), self._bf16_on,
               bool(skip_padding), bool(self._split3_on), self.split3_products, self.wavenet_bf16())
        cache = self._graphs
        g = cache.pop(key, None)
        if g is None:
            g = GraphedConversion(self, B, T, tau, src_rows, tgt_rows, skip_padding=skip_padding,
                                  wavenet="bf16" if key[-1] else "fp32")
            while len(cache) >= max_cached:
                cache.pop(next(iter(cache)))
        cache[key] = g     # re-inserted last: the dict is the LRU order
        return g

    def use_bf16_wavenet(self, enable=True):
        """Run every WaveNet layer of the posterior encoder and of both flow passes on ``ov_wn_layer_bf16``: bf16 matrix
        operands, fp32 state.  Off by default: the fp32 layers are the ones held to the 1e-3
        parity bar.  Independent of ``use_bf16_generator``; a call's ``wavenet=`` overrides it for that call."""
        self._wn_bf16_on = bool(enable)
        self._graphs.clear()                      # captured graphs hold the other path's launches
        return self

    def wavenet_bf16(self):
        """True where a WaveNet stack launched NOW runs the bf16 layers: the running call's ``wavenet=`` if it gave one,
        else the ``use_bf16_wavenet`` switch."""
        return self._wn_bf16_on if self._wn_choice is None else self._wn_choice == "bf16"

    @contextlib.contextmanager
    def wavenet_scope(self, wavenet):
        """``wavenet=`` of one call: None follows the switch; ``"fp32"`` / ``"bf16"`` choose for the launches issued
        inside the ``with`` block without touching the switch (anything else: ``OvError``).  Scopes nest: an inner None
        keeps the outer choice.  The choice is state of THIS engine while the block runs, like its workspaces and its
        other switches: not re-entrant -- two threads, or two interleaved callers, on one engine would see each other's
        choice (an engine serves one caller at a time; streams and pools re-enter their own scope at every launch)."""
        if _lib.check_wavenet(wavenet, optional=True) is None:
            yield self
            return
        saved, self._wn_choice = self._wn_choice, wavenet
        try:
            yield self
        finally:
            self._wn_choice = saved

    def use_bf16_generator(self, enable=True):
        """Route ``voice_conversion``'s generator through the bf16 kernels (BASELINE.json configs[4]).  Off by
        default: the fp32 path is the one held to the 1e-3 parity bar."""
        if enable:
            self.bf16_generator()
        self._bf16_on = bool(enable)
        return self

    def bf16_generator(self):
        """The bf16 channels-last generator of this checkpoint (``bf16.GeneratorBf16``), built on first use.  Asking for
        it neither reads nor sets the ``use_bf16_generator`` switch: a call's or a live pool's ``generator="bf16"`` and
        the fp32 path share one engine."""
        if self.generator_bf16 is None:
            from .bf16 import GeneratorBf16
            self.generator_bf16 = GeneratorBf16(self._state_dict_for_bf16, self.cfg, self.device)
        return self.generator_bf16

    def use_split_bf16x3(self, enable=True, products=6):
        """Run the MRF ResBlocks of the generator stages with C >= 128 (``SPLIT_MIN_CHANNELS``; stages 0-1 of the released
        configuration; instances exist down to C = 64) on ``ov_conv1d_split3``: every fp32 operand
        carried as three bf16 planes (lossless), every product as the six plane products of weight >= 2^-18 on the bf16
        matrix pipe with fp32 accumulation -- fp32-level results (against float64 the error is BELOW the fp32 MFMA
        kernels' on every shape, profiles/r05_s2_split3_table_all_shapes.txt) at 1.3-2.1x the DIRECT fp32 kernels' speed.  Since
        round 6 the default path runs these convs in the Winograd domain, and the two are within 1 % of each other: 102.8
        (this path) vs 103.8 ms per batch-32 conversion.  ``products=3`` uses the hi / mid planes only (16-bit operands, ~2e-5 per
        conv, 80 ms).  Off by default: the contract path is the fp32 kernels
        (reference: openvoice/modules.py:296-309, models.py:280-286)."""
        if products not in (6, 3):
            raise _lib.OvError(f"use_split_bf16x3: products must be 6 or 3, got {products!r}")
        if enable and self.split_resblocks is None:
            from . import split3
            convs = list(resblock_convs(self.cfg))
            # C = 64 (stage 2) stays on the fp32 Winograd launches: its split convs tie with them (20.9 vs 21.5 ms) and
            # cost two layout passes over the stage's tensors (1.3 ms): 104.3 -> 102.8 ms (profiles/r06_s34_*)
            keep = lambda i: all(c.ch >= SPLIT_MIN_CHANNELS and split3.supported(c.ch, c.ch, c.K, c.dil)
                                 and split3.supported(c.ch, c.ch, c.K, 1) for c in convs if c.stage == i)
            self.split_resblocks = _resblock_tree(self._state_dict_for_bf16, self.cfg, lambda c, w, b, d:
                                                  split3.PackedConvSplit3(w, b, self.device, dil=d), keep)
        self._split3_on = bool(enable)
        self.split3_products = products
        self._graphs.clear()                      # captured graphs hold the other path's launches
        return self

    def _split_buffers(self, ws, B, st, L):
        """Plane tensors (3, B, L, ch) bf16 of split-precision stage ``st``: the activated stage input, the conv1 output,
        two ping-pong pair outputs and one result per ResBlock; allocated once per workspace at the largest stage."""
        nk = len(self.cfg["resblock_kernel_sizes"])
        need = 3 * B * L * st.ch
        bufs = ws.get("split3")
        if bufs is None:
            # sized ONCE per workspace, at the largest split stage of this (batch, frames) -- stage i has ch_i channels at
            # frames x rate_out_i columns -- and never from a capturing graph's private pool
            if torch.cuda.is_current_stream_capturing():
                raise _lib.OvError("split-precision plane buffers must exist before graph capture: run one eager conversion "
                                   "of this (batch, frames) shape first")
            frames = L // st.rate_out
            largest = max([need] + [3 * B * frames * o.rate_out * o.ch for o in self.stages
                                    if self.split_resblocks[o.index] is not None])
            bufs = ws["split3"] = [torch.empty(largest, dtype=torch.bfloat16, device=self.device) for _ in range(4 + nk)]
        assert bufs[0].numel() >= need
        return [b[:need].view(3, B, L, st.ch) for b in bufs]

    def _mrf_split(self, st, u, acc, ws, B, L, limits=None):
        """The MRF of stage ``st`` on the split-precision kernels: u (B, ch, L) fp32 raw -> acc (B, ch, L) fp32 = mean of the
        ResBlock1 outputs.  Tensors between the launches are plane tensors stored ACTIVATED (the producer applies the
        next conv's leaky ReLU before it splits); conv2 reads its residual from the pair's activated input and inverts
        the activation in fp32; the last pair of a ResBlock stores raw; the sum / mean is the layout kernel back."""
        from . import split3
        stage, ch = self.split_resblocks[st.index], st.ch
        nk = len(stage)
        bufs = self._split_buffers(ws, B, st, L)
        xa, t, ping, pong, results = bufs[0], bufs[1], bufs[2], bufs[3], bufs[4:]
        prod = self.split3_products
        # length-aware work lists (skip_padding): 128-column tiles beyond an utterance's limit are dropped from every
        # conv's (dense) work list; the two layout kernels stream whole tensors
        lim = dict(col_limit=limits, col_limit_scale=st.rate_out) if limits is not None else {}
        timed = self._timed
        uv = u[:B * ch * L].view(B, ch, L)
        timed("split_layout", 0.0, lambda: split3.to_planes(uv, LRELU_SLOPE, out=xa))
        for j, pairs in enumerate(stage):
            cur = xa
            for n, (c1, c2) in enumerate(pairs):
                last = n == len(pairs) - 1
                flops = 2.0 * ch * ch * c1.K * L * B
                timed("mrf_split", flops, lambda: split3.launch_conv_split3(c1, cur, t, out_slope=LRELU_SLOPE, products=prod, **lim))
                dst = results[j] if last else (pong if cur is ping else ping)
                timed("mrf_split", flops, lambda: split3.launch_conv_split3(c2, t, dst, res=cur, res_slope=LRELU_SLOPE,
                                                                             out_slope=1.0 if last else LRELU_SLOPE,
                                                                             products=prod, **lim))
                cur = dst
        ops = list(results[:nk]) + [None] * (3 - nk)
        if nk > 3:
            raise _lib.OvError("split-precision MRF: at most 3 ResBlocks per stage")
        av = acc[:B * ch * L].view(B, ch, L)
        timed("split_layout", 0.0, lambda: split3.from_planes(ops[0], ops[1], ops[2], in_slope=1.0, scale=1.0 / nk, out=av))

    def limit_margin(self, B, T):
        """``limit_margin_frames`` of this engine's configuration for a (B, T) launch under the CURRENT
        ``use_winograd`` / ``fuse_pairs`` (they may be switched after construction); at least ``generator_margin``."""
        key = (int(B), int(T), bool(self.use_winograd), bool(self.fuse_pairs))
        cache = self._limit_margins
        if key not in cache:
            cache[key] = max(self.generator_margin, limit_margin_frames(self.cfg, *key))
        return cache[key]

    def frame_limits(self, lengths, T):
        """Two int32 [B] device vectors (``ov_frame_limits_i32``, no host sync): the frames of each utterance the
        generator must COMPUTE so that its first ``lengths[b]`` frames are unaffected by what lies beyond
        (``length + limit_margin(B, T)``), and the frames it KEEPS (``length``): ``conv_post`` writes zeros beyond them,
        so the whole of ``o_hat`` is defined -- what lies between the two is computed from neighbours that were skipped
        and must not leak into the result."""
        B = lengths.shape[0]
        lim = torch.empty(2, B, dtype=torch.int32, device=self.device)
        _lib.call("ov_frame_limits_i32", lengths, lim[0], B, int(T), self.limit_margin(B, T))
        _lib.call("ov_frame_limits_i32", lengths, lim[1], B, int(T), 0)
        return lim

    def _upsample(self, i, x, x_ld, u, B, L, cin, ch, **lim):
        """leaky_relu(0.1) + ConvTranspose1d of generator stage ``i`` (models.py:278-279): x [B, cin, x_ld] with ``L``
        valid columns -> u, dense [B, ch, L * stride]."""
        up = self.ups[i]
        s = up["stride"]
        self._conv(up["conv"], x, 0, cin * x_ld, u, 0, ch * L * s, B, L, epi=EPI_CONVT, in_slope=LRELU_SLOPE,
                   flags=up["flags"], phase_s=s, x_ld=x_ld, tag="ups", alg_flops=2.0 * cin * ch * 2 * s * L * B, **lim)

    def _mrf(self, i, u, t1, ra, acc, ws, B, ch, L, limits, rate):
        """MRF of generator stage ``i`` on the fp32 kernels: u (dense [B, ch, L]) -> acc = mean of the ResBlock1
        outputs; t1 / ra are scratch of the same size.  ``limits`` / ``rate``: the length-aware work lists of decode()."""
        cfg = self.cfg
        nk = len(cfg["resblock_kernel_sizes"])
        lim = lambda scale: dict(col_limit=limits, col_limit_scale=scale) if limits is not None else {}
        bs = ch * L
        # MRF: mean of the 3 ResBlock1 outputs (models.py:280-286, modules.py:296-306).  The three ResBlocks of a
        # stage are independent chains until the sum.  At small batches one launch does not fill the chip (batch 1,
        # stage 0: 108 workgroups for 512 slots; stages 1-3: one partial round of 431), so there the chains run on
        # separate HIP streams and fill each other's ramps and tails; chain j's last launch waits for chain j - 1's
        # (the running sum keeps its order: bit-identical to the serial sequence).
        concurrent = (self.chain_streams > 1 and nk > 1 and B <= self.chain_streams_max_batch and self.profile is None
                      # the chains' extra scratch is allocated lazily: never from a capturing graph's private pool
                      and not (torch.cuda.is_current_stream_capturing() and len(ws.get("dec_extra", [])) < 2 * (nk - 1)))
        scratch = [(t1, ra)]
        if concurrent:
            extra = self._chain_scratch(ws, 2 * (nk - 1))
            scratch += [(extra[2 * j], extra[2 * j + 1]) for j in range(nk - 1)]

        def chain(j, pairs):
            t1_, ra_ = scratch[j if concurrent else 0]
            cur = u
            # fused pairs, or Winograd-domain convs where an instance exists, wino_policy() picks it and the launch has
            # WINO_MIN_ITEMS items; all carry the same length-aware work lists (skip_padding)
            fams = resblock_families(ch, pairs[0][0].K, [c1.dil for c1, _ in pairs], B, L, self.use_winograd,
                                     self.fuse_pairs)
            fused = fams[0][0] == "pair"
            wn = self.wino_resblocks[i][j]
            for n, (c1, c2) in enumerate(pairs):
                last = n == len(pairs) - 1
                if last and concurrent and j > 0:
                    torch.cuda.current_stream(self.device).wait_event(done[j - 1])
                add = acc if (last and j > 0) else None
                scale = 1.0 / nk if (last and j == nk - 1) else 1.0
                if fused:
                    # one launch per pair, intermediate in LDS; out must not alias x: ra / t1 ping-pong
                    dst = acc if last else (t1_ if cur is ra_ else ra_)
                    self._pair(c1, c2, cur, dst, bs, B, L, add, scale, **lim(rate))
                else:
                    w1, w2 = (w if f == "wino" else None for w, f in zip(wn[n], fams[n]))
                    # t1 is read by c2 only, which activates it: a Winograd c1 stores it activated (the same
                    # values, modules.py:298-301) and c2 -- either kernel -- stages it as is
                    if w1 is not None:
                        self._wino(w1, cur, t1_, bs, B, L, out_slope=LRELU_SLOPE, **lim(rate))
                    else:
                        self._conv(c1, cur, 0, bs, t1_, 0, bs, B, L, in_slope=LRELU_SLOPE, tag="mrf", **lim(rate))
                    c2_slope = 1.0 if w1 is not None else LRELU_SLOPE
                    dst = acc if last else ra_
                    if w2 is not None:
                        self._wino(w2, t1_, dst, bs, B, L, res=cur, add=add, scale=scale, in_slope=c2_slope, **lim(rate))
                    else:
                        self._conv(c2, t1_, 0, bs, dst, 0, bs, B, L, in_slope=c2_slope, res=cur, res_bs=bs,
                                   add=add, add_bs=bs, scale=scale, tag="mrf", **lim(rate))
                cur = dst

        if not concurrent and self._mrf_multi(i, u, t1, ra, acc, ws, B, ch, L, lim(rate)):
            return
        if not concurrent:
            for j, pairs in enumerate(self.resblocks[i]):
                chain(j, pairs)
        else:
            main = torch.cuda.current_stream(self.device)
            side = self._side_streams(nk)
            fork = torch.cuda.Event()
            fork.record(main)
            done = [None] * nk
            for j, pairs in enumerate(self.resblocks[i]):
                with torch.cuda.stream(side[j]):
                    side[j].wait_event(fork)
                    chain(j, pairs)
                    done[j] = torch.cuda.Event()
                    done[j].record(side[j])
            for j in range(nk):                     # every chain's scratch is free again before the next stage
                main.wait_event(done[j])

    def _multi_launch_stage(self, i, B, ch, L):
        """Whether the MRF of stage ``i`` runs as multi launches in a (B, ch, L) conversion: the switches, three (or two)
        ResBlocks of different kernel sizes and equal dilations, every conv a Winograd launch (``resblock_families``: an
        instance, wino_policy, WINO_MIN_ITEMS) of the 64- or 128-row families -- and more items per conv than the device has
        CUs.  Up to one item per workgroup there is no tail to level and the three launches already run one item each; with
        every ResBlock on scratch of its own the stage then only loses the cache hits that shared t1 / ra buffers give a
        small conversion (batch 1 x 10 s: 6.02 ms against 5.95), so those stay launch by launch."""
        blocks = self.resblocks[i]
        nk = len(blocks)
        ks = [pairs[0][0].K for pairs in blocks]
        dils = [[c1.dil for c1, _ in pairs] for pairs in blocks]
        if not (self.use_multi_launch and self.use_winograd and 2 <= nk <= 3 and len(set(ks)) == nk and set(ks) <= {3, 7, 11}
                and ch % 64 == 0 and all(d == dils[0] for d in dils)):
            return False
        if self._cus is None:
            self._cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if wino_items(ch, 1, B, L) <= self._cus:
            return False
        fams = [resblock_families(ch, k, d, B, L, self.use_winograd, self.fuse_pairs) for k, d in zip(ks, dils)]
        return all(f == ("wino", "wino") for fam in fams for f in fam)

    def _multi_launch_scratch(self, B, T):
        """``multi_launch_scratch_buffers`` when some stage of a (B, T) conversion runs multi launches, else 0."""
        return (multi_launch_scratch_buffers(self.cfg)
                if any(self._multi_launch_stage(st.index, B, st.ch, T * st.rate_out) for st in self.stages) else 0)

    def _mrf_multi(self, i, u, t1, ra, acc, ws, B, ch, L, lim):
        """The MRF of stage ``i`` walked PAIR BY PAIR with the three ResBlocks' convs of a step in one launch
        (ov_conv1d_wino_multi_f32): c1 of every ResBlock, then c2 of every ResBlock.  The c2 of the LAST pair adds the
        running MRF sum of the ResBlock before it, so those stay single launches in ResBlock order: the same operations on
        the same operands as ``_mrf``'s chains, bit for bit.  Returns False -- nothing launched -- where the stage is not made
        of Winograd launches of one shape (``_mrf`` then runs it launch by launch)."""
        cfg = self.cfg
        blocks, wn = self.resblocks[i], self.wino_resblocks[i]
        nk = len(blocks)
        dils = [[c1.dil for c1, _ in pairs] for pairs in blocks]
        if not self._multi_launch_stage(i, B, ch, L):
            return False
        need = multi_launch_scratch_buffers(cfg)
        if torch.cuda.is_current_stream_capturing() and len(ws.get("dec_extra", [])) < need:
            return False           # the scratch is never allocated from a capturing graph's private pool
        extra = self._chain_scratch(ws, need)
        ts, ras = [t1] + extra[0:need:2], [ra] + extra[1:need:2]
        bs, npairs = ch * L, len(dils[0])
        cur = [u] * nk
        for n in range(npairs):
            self._wino_multi([dict(layer=wn[j][n][0], x=cur[j], out=ts[j], bs=bs, in_slope=LRELU_SLOPE, out_slope=LRELU_SLOPE)
                              for j in range(nk)], B, L, **lim)
            if n < npairs - 1:
                self._wino_multi([dict(layer=wn[j][n][1], x=ts[j], out=ras[j], bs=bs, res=cur[j]) for j in range(nk)], B, L, **lim)
                cur = list(ras)
            else:
                for j in range(nk):
                    self._wino(wn[j][n][1], ts[j], acc, bs, B, L, res=cur[j], add=acc if j > 0 else None,
                               scale=1.0 / nk if j == nk - 1 else 1.0, in_slope=1.0, **lim)
        return True

    def _stage(self, st, x, x_ld, x_bs, bufs, out, ws, B, L, cond_d=None, limits=None, keep=None):
        """Generator stage ``st`` (models.py:274-291) on the fp32 kernels: [conv_pre + cond into ``ws["pre"]`` (stage 0)],
        leaky_relu + ConvTranspose, the MRF, [leaky_relu(0.01) + conv_post + tanh into ``out`` (last stage)].  ``x``
        [B rows of ``x_bs``][cin][``x_ld``] with ``L`` columns; ``bufs`` = (u, t1, ra, acc), dense [B, ch, L * stride]
        each: the ConvTranspose output, the MRF's two scratch buffers -- None for a split-precision stage, which takes
        its plane buffers from ``ws`` -- and the MRF mean.  ``limits`` / ``keep``: the two rows of ``frame_limits``."""
        lim = lambda scale: dict(col_limit=limits, col_limit_scale=scale) if limits is not None else {}
        if st.index == 0:
            Tp = ws["Tp"]
            self._conv(self.conv_pre, x, 0, x_bs, ws["pre"], 0, st.cin * Tp, B, L, bias_b=cond_d,
                       bias_b_bs=0 if cond_d.shape[0] == 1 else cond_d.shape[1], x_ld=x_ld, out_ld=Tp, tag="conv_pre",
                       **lim(1))
            x, x_ld = ws["pre"], Tp
        u, t1, ra, acc = bufs
        self._upsample(st.index, x, x_ld, u, B, L, st.cin, st.ch, **lim(st.rate_in))
        L *= st.stride
        if t1 is None:
            self._mrf_split(st, u, acc, ws, B, L, limits=limits)
        else:
            self._mrf(st.index, u, t1, ra, acc, ws, B, st.ch, L, limits, st.rate_out)
        if st.last and keep is not None:
            _lib.call("ov_conv_post_tanh_limited_f32", acc, self.post_w, out, B, st.ch, L, self.post_w.shape[1],
                      FINAL_LRELU_SLOPE, keep, st.rate_out)
        elif st.last:
            _lib.call("ov_conv_post_tanh_f32", acc, self.post_w, out, B, st.ch, L, self.post_w.shape[1], FINAL_LRELU_SLOPE)

    def decode(self, z_hat, cond_d, ws=None, T=None, limits=None):
        """Generator (models.py:272-291).  ``z_hat`` is [B, C, ld] with ``T`` valid frames per row
        (``T`` defaults to the full row, i.e. a dense tensor).  ``limits`` (``frame_limits``): frames per utterance
        to compute -- time tiles wholly beyond are dropped from every launch's work list."""
        B, C, ld = z_hat.shape
        T = ld if T is None else T
        if ws is None:
            ws = self._workspace(B, T)
        keep = None
        if limits is not None:
            limits, keep = limits[0], limits[1]
            if B > LIMIT_MAX_BATCH:
                # the conv kernels' prefix table holds 256 utterances: beyond that every launch computes the whole
                # tensors, but conv_post (a per-utterance limit, no table) still keeps `length` frames and writes zeros
                # beyond them -- the skip_padding contract ("the padded tail of o_hat is zero") holds at any batch size
                limits = None
        o_hat = torch.empty(B, 1, T * self.total_upsample, dtype=torch.float32, device=self.device)
        x, x_ld, x_bs = z_hat, ld, C * ld
        free = list(ws["dec"])
        for st in self.stages:
            u = free.pop()
            if st.index > 0:
                free.append(x)            # the stage's input is free once its ConvTranspose has read it: it serves as t1
            # a split-precision stage (opt-in) keeps its intermediates in plane buffers of its own
            split = self._split3_on and self.split_resblocks[st.index] is not None
            t1, ra = (None, None) if split else (free.pop(), free.pop())
            acc = free.pop()
            self._stage(st, x, x_ld, x_bs, (u, t1, ra, acc), o_hat, ws, B, T * st.rate_in, cond_d, limits, keep)
            free += [u] if split else [u, t1, ra]
            x, x_ld = acc, T * st.rate_out
        return o_hat

    # ---- live streams (openvoice_amd/live.py): one conversion unit on caller-given buffers -----------------------
    # A unit runs on B rows of [left history | new columns] of equal width L, with the kernels' ordinary "same" zero
    # padding at both ends; the caller keeps the output columns whose receptive field lies inside the buffer.  Inputs and
    # outputs are views of the caller's memory with explicit row (ld) and batch strides; the scratch comes from
    # ``live_workspace`` (sized by the unit's widest buffer, never by a file length).
    def live_workspace(self, key, B, width, stage=None):
        """Scratch of one live unit launch of ``B`` rows, ``width`` input columns at most; allocated once per
        ``(key, B)`` and kept (``self.live_ws_builds`` counts the allocations).  Frame-rate units (``stage`` None): the
        WaveNet tensors and the mask in the ``_workspace`` layout (ld = ``padded_frames(width)``).  Generator stage i:
        the conv_pre output (stage 0), the ConvTranspose output and the two MRF scratch buffers, and the MRF output of
        the last stage (conv_post reads it)."""
        cache = self._live_ws
        ws = cache.get((key, B))
        if ws is not None:
            assert ws["width"] >= width, "live unit wider than its workspace"
            return ws
        self.live_ws_builds += 1
        dev, H = self.device, self.hidden
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        Tp = padded_frames(width)
        if stage is None:
            ws = dict(Tp=Tp, mask=z(B, Tp), mask_len=-1, h=z(B, H, Tp), h2=z(B, H, Tp), acts=z(B, H, Tp),
                      skip=z(B, H, Tp))
        else:
            st = self.stages[stage]
            n = B * st.ch * width * st.stride
            ws = dict(Tp=Tp, dec=[z(n) for _ in range(3)])
            if stage == 0:
                ws["pre"] = z(B, st.cin, Tp)
            if st.last:
                ws["acc"] = z(n)
        ws["width"] = width
        cache[(key, B)] = ws
        return ws

    def _conds(self, g_src, g_tgt):
        """Conditioning GEMVs (T = 1) of ``g_src`` / ``g_tgt`` [rows, gin]: the WaveNet gate biases (modules.py:189-190)
        of the posterior encoder (``q``) and of every coupling in both directions (``src``, ``tgt``), and the generator's
        cond bias (``d``, models.py:275)."""
        g_q = self._zeros_like_cached(g_src) if self.zero_g else g_src
        g_d = self._zeros_like_cached(g_tgt) if self.zero_g else g_tgt
        return dict(q=self._wn_cond(self.q_wn, g_q), src=[self._wn_cond(cp["wn"], g_src) for cp in self.couplings],
                    tgt=[self._wn_cond(cp["wn"], g_tgt) for cp in self.couplings],
                    d=self._linear(g_d, self.dec_cond_w, self.dec_cond_b))

    live_conds = _conds      # per-row conditioning of a live launch

    def _live_mask(self, ws, B, L):
        if ws["mask_len"] != L:
            lengths = torch.full((B,), L, dtype=torch.int64, device=self.device)
            _lib.call("ov_sequence_mask_f32", lengths, ws["mask"], B, L, ws["Tp"])
            ws["mask_len"] = L
        return ws["mask"]

    @torch.no_grad()
    @on_own_device
    def live_posterior(self, spec, spec_ld, spec_bs, noise, noise_bs, out, ld, bs, B, L, cond_q, tau, ws):
        """Posterior encoder unit (models.py:212-221: q_pre, the 16-layer WaveNet, q_proj with ``OV_EPI_POSTERIOR``):
        ``spec`` [B rows of ``spec_bs``][513][``spec_ld``] -> ``out`` z [B rows of ``bs``][inter][``ld``]; ``noise``
        [B rows of ``noise_bs``][inter][``ld``]; ``L`` columns; ``cond_q`` the rows' gate biases (``live_conds``);
        ``tau`` one number or one per row (``item_tau``)."""
        scale, scale_b = self._tau_args(B, tau)
        H, C, Tp = self.hidden, self.inter, ws["Tp"]
        mask = self._live_mask(ws, B, L)
        self._conv(self.q_pre, spec, 0, spec_bs, ws["h"], 0, H * Tp, B, L, flags=F_MASK_V, mask=mask, mask_bs=Tp,
                   x_ld=spec_ld, out_ld=Tp, tag="q_pre")
        self._wavenet(self.q_wn, ws, B, L, cond_q, mask)
        self._conv(self.q_proj, ws["skip"], 0, H * Tp, out, 0, bs, B, L, epi=EPI_POSTERIOR, res=noise, res_bs=noise_bs,
                   scale=scale, scale_b=scale_b, mask=mask, mask_bs=Tp, rows=2 * C, x_ld=Tp, out_ld=ld, tag="q_proj")

    @torch.no_grad()
    @on_own_device
    def live_flow(self, src, dst, B, L, conds, reverse, ws):
        """One flow direction (models.py:390-397) as a unit: ``src`` -> ``dst``, both [B][inter][ws Tp] (``_flow``'s
        layout), ``L`` columns, ``conds`` the rows' per-coupling gate biases."""
        self._flow(src, dst, ws, B, L, conds, self._live_mask(ws, B, L), reverse)

    @torch.no_grad()
    @on_own_device
    def live_generator_stage(self, i, x, x_ld, x_bs, out, B, L, ws, cond_d=None):
        """Generator stage ``i`` as a unit (models.py:274-291): [conv_pre + cond (stage 0)], leaky_relu, the
        ConvTranspose and the MRF; the last stage adds leaky_relu(0.01), conv_post and tanh.  ``x`` [B rows of
        ``x_bs``][C_in][``x_ld``] with ``L`` columns -> ``out`` dense [B, C_out, L * stride] ([B, 1, L * stride] for the
        last stage).  ``decode``'s own launches (``_upsample``, ``_mrf``): bit-identical per column to a one-pass run
        whose columns line up with the same Winograd tiles."""
        if self._bf16_on or self._split3_on:
            raise _lib.OvError("live streams run the fp32 generator only (use_bf16_generator / split_bf16x3 are off)")
        st = self.stages[i]
        u, t1, ra = ws["dec"]
        self._stage(st, x, x_ld, x_bs, (u, t1, ra, ws["acc"] if st.last else out), out, ws, B, L, cond_d)

    # The same unit on the bf16 channels-last generator (``LivePool(generator="bf16")``).  The precision belongs to the
    # pool that asks for it: nothing here reads or sets ``_bf16_on``, so fp32 and bf16 pools share one engine.
    @torch.no_grad()
    @on_own_device
    def live_cond_bf16(self, g_tgt):
        """``g_tgt`` [rows, gin] -> the bf16 generator's conv_pre bias rows [rows, ch] (``GeneratorBf16.cond_rows``: the
        launch ``decode`` issues, conv_pre's bias folded in -- not ``live_conds``' ``d``)."""
        g_d = self._zeros_like_cached(g_tgt) if self.zero_g else g_tgt
        return self.bf16_generator().cond_rows(g_d)

    def live_workspace_bf16(self, key, B, width, stage):
        """Scratch of one bf16 generator unit launch of ``B`` rows, ``width`` input columns at most, cached per
        ``(key, B)`` like ``live_workspace`` (same counter, ``live_ws_builds``): the channels-last bf16 input and
        output of the stage, the stage's own scratch buffers, and the conv_pre output (stage 0)."""
        cache = self._live_ws_bf16
        ws = cache.get((key, B))
        if ws is not None:
            assert ws["width"] >= width, "live unit wider than its workspace"
            return ws
        self.live_ws_builds += 1
        f = lambda n: torch.empty(n, dtype=torch.bfloat16, device=self.device)
        st = self.stages[stage]
        n = self.bf16_generator().stage_scratch_elems(stage, B, width)
        ws = dict(width=width, xin=f(B * width * (self.inter if stage == 0 else st.cin)), out=None if st.last else f(n),
                  bufs=[f(n) for _ in range(4 if st.last else 3)], pre=f(B * width * st.cin) if stage == 0 else None)
        cache[(key, B)] = ws
        return ws

    @torch.no_grad()
    @on_own_device
    def live_generator_stage_bf16(self, i, x, x_ld, x_bs, out, B, L, ws, cond_d=None):
        """``live_generator_stage`` on the bf16 kernels, same contract: ``x`` [B rows of ``x_bs``][C_in][``x_ld``] fp32
        with ``L`` columns -> ``out`` dense fp32 [B, C_out, L * stride] ([B, 1, L * stride] for the last stage).
        ``ov_rows_f32_to_cl_bf16`` -> ``GeneratorBf16.stage`` -> ``ov_cl_bf16_to_rows_f32`` (the last stage writes fp32
        itself); ``ws`` from ``live_workspace_bf16``, ``cond_d`` [B, ch] from ``live_cond_bf16`` (stage 0).  The tensor
        between two stages is what ``GeneratorBf16.decode`` keeps there, widened to fp32 and rounded back without
        loss.  Exactly ``L`` columns are launched: the bf16 launchers take any L >= 1."""
        if self._bf16_on or self._split3_on:
            raise _lib.OvError("a live unit's generator is chosen by its pool (use_bf16_generator / split_bf16x3 are off)")
        gen, st = self.bf16_generator(), self.stages[i]
        cin, s = self.inter if i == 0 else st.cin, st.stride
        xin = ws["xin"][: B * L * cin].view(B, L, cin)
        _lib.call("ov_rows_f32_to_cl_bf16", x, x_bs, x_ld, xin, B, cin, L)
        bufs = list(ws["bufs"])
        if st.last:
            gen.stage(i, xin, out[: B * L * s].view(B, 1, L * s), B, L, cond=cond_d, bufs=bufs, pre=ws["pre"])
            return
        o = ws["out"][: B * L * s * st.ch].view(B, L * s, st.ch)
        gen.stage(i, xin, o, B, L, cond=cond_d, bufs=bufs, pre=ws["pre"])
        _lib.call("ov_cl_bf16_to_rows_f32", o, out, st.ch * L * s, L * s, B, st.ch, L * s)

    # ---- extract_se path -----------------------------------------------------------------------------
    @torch.no_grad()
    @on_own_device
    def reference_encoder(self, spec_t):
        """``spec_t`` [N, Ty, n_freq] (the transposed spectrogram the reference API passes,
        openvoice/api.py:131) -> [N, gin]; reference: openvoice/models.py:339-359.  Internally every
        tensor is [N][C][F][T] (time contiguous), i.e. the un-transposed spectrogram: when the caller
        passes ``spec.transpose(1, 2)`` the transpose back is a view and nothing is copied."""
        re = self.ref_enc
        if re is None:
            raise _lib.OvError("this checkpoint has no ref_enc.* weights")
        dev = self.device
        x = spec_t.to(dev, torch.float32).transpose(1, 2).contiguous()     # [N, F, T]
        N, F, T = x.shape
        assert F == self.spec_channels
        cur = torch.empty_like(x)
        _lib.call("ov_layernorm_freq_f32", x, re["ln_w"], re["ln_b"], cur, N, F, T, 1e-5)
        cin = 1
        for w, b in re["convs"]:
            cout = w.shape[0]
            Fo, To = (F - 1) // 2 + 1, (T - 1) // 2 + 1
            nxt = torch.empty(N, cout, Fo, To, dtype=torch.float32, device=dev)
            _lib.call("ov_conv2d_s2_relu_f32", cur, w, b, nxt, N, cin, cout, F, T)
            cur, cin, F, T = nxt, cout, Fo, To
        feat = cin * F                                                        # 128 * 9 = 1152
        H = REF_ENC_GRU
        gi = torch.empty(N, 3 * H, T, dtype=torch.float32, device=dev)
        self._conv(re["gru_in"], cur, 0, feat * T, gi, 0, 3 * H * T, N, T, tag="gru_in")
        h = torch.empty(N, H, dtype=torch.float32, device=dev)
        _lib.call("ov_gru_f32", gi, re["whh_t"], re["bhh"], h, N, H, T)
        return self._linear(h, re["proj_w"], re["proj_b"])

    @torch.no_grad()
    @on_own_device
    def reference_encoder_ragged(self, spec, frames):
        """``reference_encoder`` for P items of DIFFERENT lengths in one launch sequence (csrc/ref_enc_ragged.hip).
        ``spec`` [P, n_freq, W] float32, un-transposed (time contiguous); rows may be padded -- a ``[:, :, :W]`` view of
        a ``[P, n_freq, ld]`` buffer is taken as it is.  ``frames``: host sequence of P ints, item p's own number of
        frames, ``1 <= frames[p] <= W``; what the buffer holds beyond them is never read (it may be NaN).  Returns
        [P, gin]: row p is what ``reference_encoder`` gives for ``spec[p:p + 1, :, :frames[p]]`` alone -- LayerNorm,
        the six convs and the GRU bit for bit (each ragged kernel performs its dense twin's operations in the twin's
        order, with the conv's zero padding at the item's own end and the GRU stopping after its last true step); the
        MFMA ``gru_in`` conv in between is column-independent.  The per-layer length table (7 rows of P,
        ``ref_enc_lengths``) is built on the host and uploaded in one copy."""
        re = self.ref_enc
        cur, steps, L = self._reference_encoder_ragged_stack(spec, frames)
        P, H = cur.shape[0], REF_ENC_GRU
        feat = cur.shape[1] * cur.shape[2]                                    # 128 * 9 = 1152
        gi = torch.empty(P, 3 * H, L, dtype=torch.float32, device=self.device)
        self._conv(re["gru_in"], cur, 0, feat * L, gi, 0, 3 * H * L, P, L, tag="gru_in")
        h = torch.empty(P, H, dtype=torch.float32, device=self.device)
        _lib.call("ov_gru_ragged_f32", gi, re["whh_t"], re["bhh"], steps, h, P, H, L)
        return self._linear(h, re["proj_w"], re["proj_b"])

    @torch.no_grad()
    @on_own_device
    def _reference_encoder_ragged_stack(self, spec, frames):
        """The first half of ``reference_encoder_ragged`` -- ragged LayerNorm and the six ragged convs (not part of the
        public surface: a seam for tests/test_gpu_enrol.py, which compares the conv stack's output with the dense one's):
        ``(out [P, 128, 9, L], steps, L)`` with ``steps`` the device int32 [P] GRU step counts (the last row of the
        length table) and ``L`` the row stride; columns at and beyond ``steps[p]`` of item p are 0."""
        re = self.ref_enc
        if re is None:
            raise _lib.OvError("this checkpoint has no ref_enc.* weights")
        dev = self.device
        x = spec.to(dev, torch.float32)
        if x.dim() != 3:
            raise ValueError(f"reference_encoder_ragged: spec must be [P, n_freq, W], got {tuple(x.shape)}")
        P, F, W = x.shape
        assert F == self.spec_channels
        frames = [int(f) for f in frames]
        if len(frames) != P or P < 1:
            raise ValueError(f"reference_encoder_ragged: {len(frames)} lengths for {P} items")
        if min(frames) < 1 or max(frames) > W:
            raise ValueError(f"reference_encoder_ragged: every length must be in [1, {W}], got {frames}")
        ld = x.stride(1)
        if x.stride() != (F * ld, ld, 1) or ld < W:
            x = x.contiguous()
            ld = W
        n_convs = len(re["convs"])
        table = torch.tensor([list(col) for col in zip(*(ref_enc_lengths(f, n_convs) for f in frames))],
                             dtype=torch.int32).to(dev)                       # [n_convs + 1, P], one copy
        lds = ref_enc_lengths(ld, n_convs)
        cur = torch.empty(P, F, ld, dtype=torch.float32, device=dev)
        _lib.call("ov_layernorm_freq_ragged_f32", x, re["ln_w"], re["ln_b"], table[0], cur, P, F, ld, 1e-5)
        cin = 1
        for k, (w, b) in enumerate(re["convs"]):
            cout = w.shape[0]
            Fo = (F - 1) // 2 + 1
            nxt = torch.empty(P, cout, Fo, lds[k + 1], dtype=torch.float32, device=dev)
            _lib.call("ov_conv2d_s2_relu_ragged_f32", cur, w, b, table[k], nxt, P, cin, cout, F, lds[k], lds[k + 1])
            cur, cin, F = nxt, cout, Fo
        return cur, table[n_convs], lds[-1]


class GraphedConversion:
    """One conversion shape -- (B, T frames, tau, rows of src/tgt speaker embedding) -- captured once into a HIP graph
    and replayed.  The path is ~330 kernel launches with no host sync and no data-dependent control flow, so a
    replay is one ``hipGraphLaunch``: at batch 1 (what ``ToneColorConverter.convert`` issues per file) the eager
    path is bound by the ~10 us of Python/ctypes per launch, not by the GPU.

    Inputs are copied into static device buffers, outputs are static too: **they are overwritten by the next
    replay** -- clone what must outlive it (``ToneColorConverter.convert_batch`` does).  The engine's workspace of
    this shape is pinned for the life of the graph.  Reference contract unchanged: openvoice/models.py:492-499."""

    @on_own_device
    def __init__(self, engine, B, T, tau, src_rows=1, tgt_rows=1, skip_padding=False, wavenet=None):
        # one number: a constant of the captured q_proj launch (a per-item tau runs ungraphed, ConverterEngine.graphed)
        dev = engine.device
        self.engine, self.B, self.T, self.tau = engine, int(B), int(T), float(tau)
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.spec = f(B, engine.spec_channels, padded_frames(T))[:, :, :T]      # 16-byte aligned rows
        self.lengths = torch.full((B,), T, dtype=torch.int64, device=dev)
        self.g_src, self.g_tgt = f(src_rows, engine.gin, 1), f(tgt_rows, engine.gin, 1)
        self.noise = f(B, engine.inter, T)
        run = lambda: engine.voice_conversion(self.spec, self.lengths, self.g_src, self.g_tgt, tau=self.tau,
                                              noise=self.noise, skip_padding=skip_padding, **_lib.wavenet_kw(wavenet))
        saved, engine.profile = engine.profile, None       # event records are not capturable
        try:
            side = torch.cuda.Stream(dev)                      # torch's rule: warm up off the default stream
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                run()                                          # allocates the workspace, fills the occupancy caches
            torch.cuda.current_stream(dev).wait_stream(side)
            self.workspace = engine._workspace(B, T)           # keep it alive if the engine moves to another shape
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = run()
        finally:
            engine.profile = saved

    @torch.no_grad()
    @on_own_device
    def __call__(self, spec, spec_lengths, sid_src, sid_tgt, noise=None, *, seed=None):
        noise_mod.exclusive(seed, noise=noise)
        if tuple(spec.shape) != (self.B, self.engine.spec_channels, self.T):
            raise _lib.OvError(f"graph captured for spec {(self.B, self.engine.spec_channels, self.T)}, got {tuple(spec.shape)}")
        self.spec.copy_(spec)
        self.lengths.copy_(spec_lengths)
        self.g_src.copy_(sid_src.reshape(self.g_src.shape))
        self.g_tgt.copy_(sid_tgt.reshape(self.g_tgt.shape))
        if seed is not None:        # outside the captured region, like the copies: the graph reads the static buffer
            self.engine.seed_noise(self.noise, seed, self.B, self.T, self.T)
        elif noise is None:
            self.noise.normal_()
        else:
            self.noise.copy_(noise)
        self.graph.replay()
        return self.out
