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

import torch

from . import _lib
from . import noise as noise_mod
from . import stretch as stretch_mod
from ._lib import EPI_COUPLE, EPI_GATE, EPI_POSTERIOR, EPI_RESSKIP, F_MASK_V, F_OUT2_INIT
from .generator import (FINAL_LRELU_SLOPE, GENERATOR_MARGIN, LRELU_SLOPE, conv_transpose_as_conv,  # noqa: F401
                        generator_margin_frames, generator_stages, resblock_convs, samples_per_frame, scratch_per_frame)
# the launch policy and the launchers live with the objects that use them; their names stay importable from here
from .generator_fp32 import (_DEC_BUFFERS, DIRECT_MIN_NCOL, LIMIT_MAX_BATCH, PAIR_POLICY, SPLIT_MIN_CHANNELS,  # noqa: F401
                             USE_MULTI_LAUNCH, WINO_MIN_ITEMS, GeneratorFp32, conv_reach, convt_row_order,
                             limit_margin_frames, multi_launch_scratch_buffers, pair_supported, resblock_families,
                             scratch_elems, wino_items, wino_ncol, wino_policy)
from .launch import Launcher, PackedConv, _ptr, launch_conv, launch_pair, on_own_device, padded_frames  # noqa: F401
from .params import ENC_Q_LAYERS, FLOW_LAYERS, N_FLOWS, effective_weight
from .ref_enc import ReferenceEncoder, ref_enc_lengths  # noqa: F401


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


def stretch_rows(table, host, n, src, dst):
    """One ``ov_stretch_rows_f32`` launch: ``table`` the DEVICE int64 records (``stretch.record``), ``host`` their host
    copy -- the call checks it and raises ``OvError`` (OV_E_BADARG) on a bad record before anything is launched --
    ``src`` / ``dst`` fp32 device tensors, the records' offsets relative to their first elements."""
    _lib.call("ov_stretch_rows_f32", table, host, int(n), src, src.numel(), dst, dst.numel())


def rows_tau(taus):
    """The ``tau`` of one launch from the taus of its rows: the number itself when the rows agree (the scalar launch,
    which a captured graph can serve), else the list (one value per row: ``ov_conv1d_params.scale_b``)."""
    taus = [float(t) for t in taus]
    return taus[0] if all(t == taus[0] for t in taus) else taus


def gate_row_order(hidden):
    """Packed row order pairing row c (tanh | m) with row c+hidden (sigmoid | logs) in adjacent
    32-row MFMA tiles, so both halves of a gate land in the same lane of one wave."""
    assert hidden % 32 == 0
    idx = []
    for q in range(hidden // 32):
        idx += list(range(32 * q, 32 * q + 32)) + list(range(hidden + 32 * q, hidden + 32 * q + 32))
    return torch.tensor(idx, dtype=torch.long)


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


def _workspace_elems(cfg, B, T):
    """Float32 elements of a ``ConverterEngine._workspace(B, T)``: ``(frame-rate tensors together, each of the _DEC_BUFFERS
    decoder scratch buffers)`` -- the one size computation behind ``_workspace`` and ``workspace_bytes``."""
    H, C, Tp = cfg["hidden_channels"], cfg["inter_channels"], padded_frames(T)
    pre, dec = scratch_elems(cfg, B, T)       # the generator's part: the conv_pre output counts as a frame-rate tensor
    # mask, h / h2 / acts / skip, noise, the three latents
    return B * (Tp + 4 * H * Tp + C * Tp + 3 * C * Tp) + pre, dec


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
        # ---- the launches, the generator, the reference encoder (extract_se; converter checkpoints only) ------------
        self.launcher = Launcher(dev)
        self.generator = GeneratorFp32(sd, cfg, dev, self.launcher)
        self.ref_enc = ReferenceEncoder(sd, spec_channels, dev, self.launcher) if "ref_enc.gru.weight_ih_l0" in sd else None
        self._ws, self._graphs = {}, {}
        self._stretch_ws = None       # (key, workspace): the generator's workspace of a stretched call
        self._live_ws, self._live_ws_bf16, self.live_ws_builds = {}, {}, 0    # live unit scratch, per (unit, rows)
        # (B, T) workspaces kept resident at once, least recently used evicted first.  1 (the default): a new shape
        # frees the previous one.  StreamPool raises it to its ladder of launch sizes so that a varying ready count
        # does not rebuild gigabytes of decoder scratch per step (workspace_bytes() prices a shape).
        self.resident_workspaces = 1
        self._zeros = {}
        self.fuse_wn = True      # WaveNet layers as one launch each (ov_wn_layer_f32) where the shape has an instance
        self.wn_row_split = 0    # 0: the launcher splits a layer's rows over two launches for one or two utterances; 1: never
        # opt-in fast generator: bf16 activations, fp32 accumulation (waveform within
        # ~1e-2 of the fp32 path instead of ~1e-5).  Built on first use by bf16_generator().
        self._state_dict_for_bf16 = sd
        self.generator_bf16 = None
        self._bf16_on = False
        # opt-in: the WaveNet layers of the posterior encoder and of the flow on the bf16 matrix pipe with fp32 state
        # (ov_wn_layer_bf16).  _wn_choice: a call's own wavenet= while it runs (wavenet_scope).
        self._wn_bf16_on, self._wn_choice = False, None

    def _wn_cond(self, wn, g):
        """cond_layer (modules.py:189-190) for every layer of ``wn`` at once, rows in the order the gate kernel in
        use expects them as its per-utterance bias."""
        if self.fuse_wn and wn.fused:
            return self.launcher.linear(g, wn.cond_w_fused, wn.cond_b_fused)
        return self.launcher.linear(g, wn.cond_w, wn.cond_b)

    def _workspace(self, B, T, frames_only=False):
        """The workspace of a (B, T) conversion.  ``frames_only`` (a stretched call, whose generator runs on another
        shape out of ``generator_workspace``): the frame-rate tensors alone, a shape of its own in the same LRU -- so a
        stretched call never holds decoder scratch for the frames it does not generate."""
        key = (B, T, "frames") if frames_only else (B, T)
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
            if not frames_only:
                self.generator.add_workspace(ws, B, T)       # pre, dec, dec_extra
            self._ws[key] = ws
        return ws

    def workspace_bytes(self, B, T):
        """Device bytes of the ``_workspace(B, T)`` allocation (the frame-rate tensors and the decoder scratch, the multi
        launches' ``multi_launch_scratch_buffers`` included while ``use_multi_launch`` is on; the opt-in paths' lazily added
        buffers not included)."""
        frame_rate, dec = _workspace_elems(self.cfg, B, T)
        return 4 * (frame_rate + self.generator.workspace_buffers(B, T) * dec)

    def _g(self, g):
        """The conditioning a ``zero_g`` model sees in place of ``g`` (models.py:495,498): an all-zero tensor of its
        shape, cached so that no conversion pays a fill launch; ``g`` itself otherwise."""
        if not self.zero_g:
            return g
        key = tuple(g.shape)
        z = self._zeros.get(key)
        if z is None:
            z = self._zeros[key] = torch.zeros_like(g)
        return z

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
                self.launcher.timed("wn_layer_bf16", 2.0 * (2 * H * H * layer["K"] + (H if last else 2 * H) * H) * T * B,
                                    lambda: launch_wn_layer(layer, src, dst, ws["skip"], mask, B, T, Tp, cond=cond,
                                                            cond_off=2 * H * i, cond_bs=cbs, first=i == 0, last=last,
                                                            mask_bs=Tp, bf16=True))
                src, dst = dst, src
            return
        if self.fuse_wn and wn.fused:
            # one launch per layer; h ping-pongs between two buffers (a tile reads its neighbours' halo columns)
            src, dst = ws["h"], ws["h2"]
            # gate conv in the Winograd domain where the launch fills the chip in whole rounds of (utterance, tile) items
            winograd = self.generator.use_winograd and wn_wino_policy(B, T)      # the one switch: see use_winograd
            for i in range(wn.n_layers):
                layer = wn.fused_layers[i]
                args = dict(cond=cond, cond_off=2 * H * i, cond_bs=cbs, first=i == 0, last=i == wn.n_layers - 1,
                            mask_bs=Tp, acts=ws["acts"], row_split=self.wn_row_split, winograd=winograd)
                rs_rows = H if args["last"] else 2 * H
                self.launcher.timed("wn_layer", 2.0 * (2 * H * H * layer["K"] + rs_rows * H) * T * B,
                                    lambda: launch_wn_layer(layer, src, dst, ws["skip"], mask, B, T, Tp, **args))
                src, dst = dst, src
            return
        for i in range(wn.n_layers):
            self.launcher.conv(wn.in_layers[i], ws["h"], 0, H * Tp, ws["acts"], 0, H * Tp, B, T, epi=EPI_GATE,
                               bias_b=cond, bias_b_off=2 * H * i, bias_b_bs=cbs, rows=2 * H, x_ld=Tp, out_ld=Tp, tag="wn_in")
            last = i == wn.n_layers - 1
            self.launcher.conv(wn.rs_layers[i], ws["acts"], 0, H * Tp, ws["h"], 0, H * Tp, B, T, epi=EPI_RESSKIP,
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
            self.launcher.conv(cp["pre"], src if n == 0 else buf, x0_off, C * Tp, ws["h"], 0, H * Tp, B, T, flags=F_MASK_V,
                               mask=mask, mask_bs=Tp, x_ld=Tp, out_ld=Tp, tag="cpl_pre")
            self._wavenet(cp["wn"], ws, B, T, conds[f], mask)
            self.launcher.conv(cp["post"], ws["skip"], 0, H * Tp, buf, x1_off, C * Tp, B, T, epi=EPI_COUPLE, mask=mask,
                               mask_bs=Tp, x_ld=Tp, out_ld=Tp, scale=-1.0 if reverse else 1.0, tag="cpl_post",
                               res=src if n < 2 else None, res_off=x1_off, res_bs=C * Tp)

    def _wavenet_cores(self):
        return (self,)

    # ---- the path ----------------------------------------------------------------------------------
    @torch.no_grad()
    @on_own_device
    def voice_conversion(self, spec, spec_lengths, sid_src, sid_tgt, tau=1.0, noise=None, skip_padding=False, *,
                         seed=None, generator=None, wavenet=None, stretch=None):
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
        ``b`` holds the bits of the batch run with the number ``tau[b]``.  ``stretch`` (None: everything above,
        launch for launch): one entry per item, a step (``stretch.step_of(speed)``) or, for a window of a long
        recording, ``(step, i0, j0, n_out)`` -- the masked ``z_hat`` is resampled along time by ``ov_stretch_rows_f32``
        (the project's own definition: ``openvoice_amd/stretch.py``) between the reverse flow and the generator, which
        then runs on ``T_out[b]`` frames per item (length-aware work lists when they differ).  ``o_hat``, ``y_mask``
        and the lengths it implies are the stretched ones; ``z``, ``z_p`` and ``z_hat`` are returned unstretched;
        ``tau``, ``seed`` and ``noise`` act before the stretch.  The item lengths are read on the host (one copy of
        ``spec_lengths`` when it lives on the device)."""
        use_bf16 = self._bf16_on
        if _lib.check_generator(generator, optional=True) is not None:
            use_bf16 = generator == "bf16"
        with self.wavenet_scope(wavenet):
            return self._voice_conversion(spec, spec_lengths, sid_src, sid_tgt, tau, noise, skip_padding, seed, use_bf16,
                                          stretch)

    def _tau_args(self, B, tau):
        """``(scale, scale_b)`` of a ``q_proj`` launch of ``B`` rows from a ``tau=`` argument (``item_tau``)."""
        tau = item_tau(B, tau, self.device)
        if isinstance(tau, float):
            return tau, None
        if isinstance(tau, list):
            tau = torch.tensor(tau, dtype=torch.float32).to(self.device)
        return 1.0, tau

    def _voice_conversion(self, spec, spec_lengths, sid_src, sid_tgt, tau, noise, skip_padding, seed, use_bf16,
                          stretch=None):
        dev = self.device
        spec = spec.to(dev, torch.float32)
        B, F, T = spec.shape
        tau = self._tau_args(B, tau)
        assert F == self.spec_channels
        # rows may be padded (the native spectrogram returns a [B, F, T] view of 16-byte aligned rows)
        if not (spec.stride(2) == 1 and spec.stride(1) >= T and spec.stride(0) >= F * spec.stride(1)):
            spec = spec.contiguous()
        C = self.inter
        if stretch is not None:       # the stretch's records are built on the host: the lengths are read before any launch
            stretch = self._stretch_plan(stretch, spec_lengths, B, T)
        lengths = spec_lengths.to(dev, torch.int64).contiguous()
        g_src = sid_src.to(dev, torch.float32).reshape(sid_src.shape[0], -1).contiguous()
        g_tgt = sid_tgt.to(dev, torch.float32).reshape(sid_tgt.shape[0], -1).contiguous()
        noise_mod.exclusive(seed, noise=noise)
        ws = self._workspace(B, T, frames_only=stretch is not None)
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
        if stretch is None:
            o_hat = self.generate(z_hat, T, lengths, conds["d"], g_tgt, ws, skip_padding, use_bf16)
            out_mask, T_out = mask, T
        else:
            # the masked z_hat, resampled along time in front of the generator (and of the bf16 generator's layout change)
            zs, gws, lengths_out, T_out, ragged = self._stretch(z_hat, Tp, stretch, B)
            o_hat = self.generate(zs, T_out, lengths_out, conds["d"], g_tgt, gws, ragged, use_bf16)
            out_mask = gws["mask"]
            _lib.call("ov_sequence_mask_f32", lengths_out, out_mask, B, T_out, gws["Tp"])
        # fresh dense tensors for the caller (the workspace is reused by the next call): padded rows -> [.., T]
        dense = torch.empty(3, B, C, T, dtype=torch.float32, device=dev)
        _lib.call("ov_unpad_rows_f32", ws["lat"], dense, 3 * B * C, T, Tp)
        y_mask = torch.empty(B, 1, T_out, dtype=torch.float32, device=dev)
        _lib.call("ov_unpad_rows_f32", out_mask, y_mask, B, T_out, ws["Tp"] if stretch is None else gws["Tp"])
        return o_hat, y_mask, (dense[0], dense[1], dense[2])

    def generate(self, z_rows, T, lengths, cond_d, g_tgt, ws, skip_padding=False, use_bf16=False):
        """The generator on a masked latent in the fp32 rows layout: ``z_rows`` [B, inter, ld] with ``T`` valid columns
        per row, ``lengths`` int64 [B] on the device, ``cond_d`` = ``generator.cond(g_tgt)``, ``ws`` a workspace that
        holds the generator's entries for (B, T) (``_workspace`` or ``generator_workspace``) -> ``o_hat`` [B, 1, T *
        spf].  ``skip_padding``: the fp32 generator computes ``length + limit_margin`` frames per item and writes zeros
        beyond ``length``; the bf16 generator computes the padded batch and the tail is masked.  This is the generator
        step of ``voice_conversion``, on ``z_hat`` or -- with ``stretch=`` -- on the stretched ``z_hat``."""
        B, dev = z_rows.shape[0], self.device
        if use_bf16:
            g_d = self._g(g_tgt)
            o_hat = self.launcher.timed("gen_bf16", 0.0,
                                        lambda: self.bf16_generator().decode(z_rows[:, :, :T], g_d.unsqueeze(-1)))
            if skip_padding:
                # the bf16 generator has no length-aware work lists (it computes the padded batch); the contract of
                # skip_padding -- every sample beyond an utterance's own length is zero -- is kept by masking
                keep_samples = (lengths.clamp(max=T) * self.generator.total_upsample).view(B, 1, 1)
                o_hat.masked_fill_(torch.arange(o_hat.shape[2], device=dev).view(1, 1, -1) >= keep_samples, 0.0)
        else:
            limits = self.generator.frame_limits(lengths, T) if skip_padding else None
            o_hat = self.generator.decode(z_rows, cond_d, ws, T=T, limits=limits)
        return o_hat

    # ---- speed= / duration=: the stretch between the reverse flow and the generator (openvoice_amd/stretch.py) ------
    def _stretch_plan(self, stretch, spec_lengths, B, T):
        """Per item ``(step, t_in, i0, j0, n_out)`` from ``voice_conversion``'s ``stretch=``: a step stretches the whole
        item (``i0 = j0 = 0``, ``n_out = T_out``), a ``(step, i0, j0, n_out)`` tuple is a window of a long recording."""
        if len(stretch) != B:
            raise ValueError(f"stretch: one entry per item ({B}), got {len(stretch)}")
        lens = [min(int(n), T) for n in torch.as_tensor(spec_lengths).reshape(-1).tolist()]
        plan = []
        for item, t_in in zip(stretch, lens):
            if isinstance(item, (tuple, list)):
                step, i0, j0, n_out = (int(v) for v in item)
            else:
                step, i0, j0, n_out = int(item), 0, 0, stretch_mod.t_out(max(t_in, 1), int(item))
            if not stretch_mod.ONE // 2 <= step <= 2 * stretch_mod.ONE:
                raise ValueError(f"stretch: step {step} outside [2^31, 2^33]")
            plan.append((step, max(t_in, 1), i0, j0, n_out))
        return plan

    def generator_workspace(self, B, T):
        """The generator's own workspace of a (B, T) launch -- what ``generate`` needs and nothing of the frame-rate
        part: the conv_pre output and the decoder scratch (``GeneratorFp32.add_workspace``), the stretched latent ``zs``
        [B, inter, Tp] and its mask.  One shape stays resident (the stretched path's counterpart of ``_workspace``, next
        to the frames-only workspace of the call: together what an unstretched conversion of ``max(T, T_out)`` frames
        holds at most); ``release_stretch_workspace`` frees it."""
        key = (B, T)
        if self._stretch_ws is None or self._stretch_ws[0] != key:
            Tp = padded_frames(T)
            f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.device)
            gws = dict(Tp=Tp, zs=f(B, self.inter, Tp), mask=f(B, Tp))
            self.generator.add_workspace(gws, B, T)
            self._stretch_ws = (key, gws)
        return self._stretch_ws[1]

    def release_stretch_workspace(self):
        """Drop the generator workspace a stretched call left resident (the next stretched call builds its own)."""
        self._stretch_ws = None

    def _stretch(self, z_hat, Tp, plan, B):
        """``ov_stretch_rows_f32`` of the workspace's masked ``z_hat`` [B, inter, Tp] into the generator workspace's
        ``zs``: one record per item, one launch.  Returns ``(zs, workspace, lengths_out int64 [B] on the device, T_out of
        the batch, whether the items' output lengths differ)``.  Columns beyond an item's ``n_out`` are zero, as the
        masked latent's are."""
        C = self.inter
        n_outs = [p[4] for p in plan]
        T_out = max(n_outs)
        gws = self.generator_workspace(B, T_out)
        zs, Tp2 = gws["zs"], gws["Tp"]
        ragged = any(n != T_out for n in n_outs)
        if ragged:
            zs.zero_()                      # a shorter item's tail: zero, whatever the previous call left there
        recs = [stretch_mod.record(b * C * Tp, b * C * Tp2, C, Tp, Tp2, t_in, i0, j0, n_out, step)
                for b, (step, t_in, i0, j0, n_out) in enumerate(plan)]
        # records and output lengths in one host table: one host -> device copy
        host = torch.tensor([v for r in recs for v in r] + n_outs, dtype=torch.int64)
        table = host.to(self.device)
        stretch_rows(table, host, B, z_hat, zs)
        return zs, gws, table[10 * B:], T_out, ragged

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
        self.launcher.conv(self.q_pre, x, 0, spec.stride(0), sub["h"], 0, H * Tp, nb, T, flags=F_MASK_V, mask=mask, mask_bs=Tp,
                           x_ld=spec.stride(1), out_ld=Tp, tag="q_pre")
        self._wavenet(self.q_wn, sub, nb, T, rows(conds["q"]), mask)
        z, z_p, z_hat = sub["z"], sub["z_p"], sub["z_hat"]
        self.launcher.conv(self.q_proj, sub["skip"], 0, H * Tp, z, 0, C * Tp, nb, T, epi=EPI_POSTERIOR, res=sub["noise"],
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
               bool(skip_padding), bool(self.generator._split3_on), self.generator.split3_products, self.wavenet_bf16())
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
        self.generator.use_split_bf16x3(enable, products)
        self._graphs.clear()                      # captured graphs hold the other path's launches
        return self

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
        def frame_rate():
            H, Tp = self.hidden, padded_frames(width)
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.device)
            return dict(Tp=Tp, mask=z(B, Tp), mask_len=-1, h=z(B, H, Tp), h2=z(B, H, Tp), acts=z(B, H, Tp), skip=z(B, H, Tp))
        return self._live_cached(self._live_ws, key, B, width,
                                 frame_rate if stage is None else lambda: self.generator.live_workspace(stage, B, width))

    def _live_cached(self, cache, key, B, width, build):
        """The live workspace of ``(key, B)`` in ``cache``: ``build()``'s dict, made on first use (``live_ws_builds``
        counts) and kept; it was sized for ``width`` columns, and no later launch may be wider."""
        ws = cache.get((key, B))
        if ws is None:
            self.live_ws_builds += 1
            ws = cache[(key, B)] = dict(build(), width=width)
        assert ws["width"] >= width, "live unit wider than its workspace"
        return ws

    def _conds(self, g_src, g_tgt):
        """Conditioning GEMVs (T = 1) of ``g_src`` / ``g_tgt`` [rows, gin]: the WaveNet gate biases (modules.py:189-190)
        of the posterior encoder (``q``) and of every coupling in both directions (``src``, ``tgt``), and the generator's
        cond bias (``d``, models.py:275)."""
        return dict(q=self._wn_cond(self.q_wn, self._g(g_src)), src=[self._wn_cond(cp["wn"], g_src) for cp in self.couplings],
                    tgt=[self._wn_cond(cp["wn"], g_tgt) for cp in self.couplings],
                    d=self.generator.cond(self._g(g_tgt)))

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
        self.launcher.conv(self.q_pre, spec, 0, spec_bs, ws["h"], 0, H * Tp, B, L, flags=F_MASK_V, mask=mask, mask_bs=Tp,
                           x_ld=spec_ld, out_ld=Tp, tag="q_pre")
        self._wavenet(self.q_wn, ws, B, L, cond_q, mask)
        self.launcher.conv(self.q_proj, ws["skip"], 0, H * Tp, out, 0, bs, B, L, epi=EPI_POSTERIOR, res=noise, res_bs=noise_bs,
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
        last stage).  ``GeneratorFp32.decode``'s own launches (its ``stage``): bit-identical per column to a one-pass run
        whose columns line up with the same Winograd tiles."""
        if self._bf16_on or self.generator._split3_on:
            raise _lib.OvError("live streams run the fp32 generator only (use_bf16_generator / split_bf16x3 are off)")
        self.generator.live_stage(i, x, x_ld, x_bs, out, B, L, ws, cond_d)

    # The same unit on the bf16 channels-last generator (``LivePool(generator="bf16")``).  The precision belongs to the
    # pool that asks for it: nothing here reads or sets ``_bf16_on``, so fp32 and bf16 pools share one engine.
    @torch.no_grad()
    @on_own_device
    def live_cond_bf16(self, g_tgt):
        """``g_tgt`` [rows, gin] -> the bf16 generator's conv_pre bias rows [rows, ch] (``GeneratorBf16.cond_rows``: the
        launch ``decode`` issues, conv_pre's bias folded in -- not ``live_conds``' ``d``)."""
        return self.bf16_generator().cond_rows(self._g(g_tgt))

    def live_workspace_bf16(self, key, B, width, stage):
        """Scratch of one bf16 generator unit launch of ``B`` rows, ``width`` input columns at most, cached per
        ``(key, B)`` like ``live_workspace`` (same counter, ``live_ws_builds``): the channels-last bf16 input and
        output of the stage, the stage's own scratch buffers, and the conv_pre output (stage 0)."""
        def build():
            f = lambda n: torch.empty(n, dtype=torch.bfloat16, device=self.device)
            st = self.generator.stages[stage]
            n = self.bf16_generator().stage_scratch_elems(stage, B, width)
            return dict(xin=f(B * width * (self.inter if stage == 0 else st.cin)), out=None if st.last else f(n),
                        bufs=[f(n) for _ in range(4 if st.last else 3)], pre=f(B * width * st.cin) if stage == 0 else None)
        return self._live_cached(self._live_ws_bf16, key, B, width, build)

    @torch.no_grad()
    @on_own_device
    def live_generator_stage_bf16(self, i, x, x_ld, x_bs, out, B, L, ws, cond_d=None):
        """``live_generator_stage`` on the bf16 kernels, same contract: ``x`` [B rows of ``x_bs``][C_in][``x_ld``] fp32
        with ``L`` columns -> ``out`` dense fp32 [B, C_out, L * stride] ([B, 1, L * stride] for the last stage).
        ``ov_rows_f32_to_cl_bf16`` -> ``GeneratorBf16.stage`` -> ``ov_cl_bf16_to_rows_f32`` (the last stage writes fp32
        itself); ``ws`` from ``live_workspace_bf16``, ``cond_d`` [B, ch] from ``live_cond_bf16`` (stage 0).  The tensor
        between two stages is what ``GeneratorBf16.decode`` keeps there, widened to fp32 and rounded back without
        loss.  Exactly ``L`` columns are launched: the bf16 launchers take any L >= 1."""
        if self._bf16_on or self.generator._split3_on:
            raise _lib.OvError("a live unit's generator is chosen by its pool (use_bf16_generator / split_bf16x3 are off)")
        gen, st = self.bf16_generator(), self.generator.stages[i]
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

    # ---- names other code uses on the engine: each reads and writes its owner's attribute ----------------------------
    def decode(self, z_hat, cond_d, ws=None, T=None, limits=None):
        return self.generator.decode(z_hat, cond_d, ws or self._workspace(z_hat.shape[0], T or z_hat.shape[2]), T, limits)


def _forward(owner, name, attr=None, missing=None):
    """``engine.name`` as a read/write property on ``engine.<owner>.<attr or name>``; ``missing``: the ``OvError`` text
    where the engine has no such owner (None in its place)."""
    def owned(self):
        obj = getattr(self, owner)
        if obj is None:
            raise _lib.OvError(missing)
        return obj
    return property(lambda self: getattr(owned(self), attr or name), lambda self, v: setattr(owned(self), attr or name, v))


ConverterEngine.profile = _forward("launcher", "profile")      # set to [] to collect per-launch HIP-event timings
# use_winograd means both: the generator's ResBlock convs and the WaveNet layers' gate conv (_wavenet) read this one value
for _name in ("total_upsample", "stages", "fuse_pairs", "use_winograd", "use_multi_launch", "chain_streams",
              "chain_streams_max_batch", "split_resblocks", "split3_products", "_split3_on", "generator_margin", "frame_limits",
              "limit_margin", "_chain_scratch"):
    setattr(ConverterEngine, _name, _forward("generator", _name))
for _name, _attr in (("reference_encoder", "__call__"), ("reference_encoder_ragged", None),
                     ("_reference_encoder_ragged_stack", None)):
    setattr(ConverterEngine, _name, _forward("ref_enc", _name, _attr, "this checkpoint has no ref_enc.* weights"))


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
