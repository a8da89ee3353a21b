"""Kernel launches of the fp32 path through the C ABI (include/openvoice_amd.h) on torch's current HIP stream: the packed
conv layer, the two conv launchers, and ``Launcher`` -- the one place that profiles a launch.  ``engine`` re-exports the
module-level names."""
import ctypes
import functools
import os

import torch

from . import _lib
from ._lib import EPI_LINEAR, ConvParams
from .generator import LRELU_SLOPE


def on_own_device(method):
    """Run an engine method with the engine's device current: kernels go to ``current_stream(self.device)`` already,
    but event records (profile mode), HIP-graph capture and the per-device launch sizing inside the library follow
    the CURRENT device, which need not be the engine's (``ToneColorConverter(cfg, device='cuda:1')`` while cuda:0 is
    current)."""
    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        dev = getattr(self, "device", None)
        if dev is None:      # GraphedConversion: the engine is an attribute, or the first constructor argument
            dev = (getattr(self, "engine", None) or kwargs.get("engine") or args[0]).device
        with torch.cuda.device(dev):
            return method(self, *args, **kwargs)
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


class Launcher:
    """The launches of one device as the model parts issue them, each recorded when ``profile`` is a list: set it to []
    to collect per-launch HIP-event timings, None (the default) launches without events."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.profile = None
        self._streams = []

    def timed(self, tag, flops, fn, *extra):
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

    def conv(self, layer, x, x_off, x_bs, out, out_off, out_bs, B, L, tag="conv", alg_flops=None, **kwargs):
        """Launch one conv, profiled under ``tag`` with its algorithmic FLOPs."""
        if alg_flops is None:
            alg_flops = 2.0 * layer.rows * (kwargs.get("cin") or layer.cin) * layer.K * L * B
        self.timed(tag, alg_flops, lambda: launch_conv(layer, x, x_off, x_bs, out, out_off, out_bs, B, L, **kwargs))

    def wino(self, layer, x, out, bs, B, L, res=None, add=None, scale=1.0, in_slope=LRELU_SLOPE, out_slope=1.0, **lim):
        """One Winograd-domain ResBlock conv (leaky ReLU on the input, LINEAR epilogue); profiled under the MRF tag with its
        algorithmic FLOPs and, as a fifth field, the FLOPs the kernel EXECUTES (wino.PRODUCTS_PER_TILE[K] / (4 K) of them)."""
        from . import wino
        kw = dict(in_slope=in_slope, out_slope=out_slope, scale=scale, res=res, res_bs=bs if res is not None else 0, add=add,
                  add_bs=bs if add is not None else 0, **lim)
        alg = 2.0 * layer.cout * layer.cin * layer.K * L * B
        self.timed("mrf", alg, lambda: wino.launch_conv_wino(layer, x, bs, out, bs, B, L, **kw),
                   alg * wino.PRODUCTS_PER_TILE[layer.K] / (4.0 * layer.K))

    def wino_multi(self, convs, B, L, **lim):
        """One ov_conv1d_wino_multi_f32 launch (``wino.launch_convs_wino``); profiled as ONE record under the MRF tag with
        the algorithmic and the executed FLOPs of all its convs."""
        from . import wino
        alg = [2.0 * c["layer"].cout * c["layer"].cin * c["layer"].K * L * B for c in convs]
        exe = sum(a * wino.PRODUCTS_PER_TILE[c["layer"].K] / (4.0 * c["layer"].K) for a, c in zip(alg, convs))
        self.timed("mrf", sum(alg), lambda: wino.launch_convs_wino(convs, B, L, **lim), exe)

    def pair(self, c1, c2, x, out, bs, B, L, add, scale, **lim):
        """One fused ResBlock1 iteration; profiled under the same tag as the two launches it replaces, with their
        algorithmic FLOPs (both convs)."""
        self.timed("mrf", 2 * 2.0 * c1.rows * c1.cin * c1.K * L * B,
                   lambda: launch_pair(c1, c2, x, bs, out, bs, B, L, add=add, add_bs=bs, scale=scale, **lim))

    def linear(self, x2d, w, b):
        Bg, Kd = x2d.shape
        M = w.shape[0]
        y = torch.empty(Bg, M, dtype=torch.float32, device=self.device)
        _lib.call("ov_linear_f32", x2d, w, b, y, Bg, M, Kd)
        return y

    def side_streams(self, n):
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(self.device))
        return self._streams[:n]
