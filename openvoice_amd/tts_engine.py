"""Host-side driver of the V1 base-speaker TTS model, ``SynthesizerTrn.infer``
(reference: openvoice/models.py:467-490).

The token-rate front end -- text encoder with windowed relative-position attention
(models.py:48-57, attentions.py:104-121, :264-329, :440-448), the deterministic and the stochastic
duration predictor (models.py:86-100, :129-138 / :171-180 with DDSConv modules.py:117-130 and the
inverse rational-quadratic spline of ConvFlow modules.py:485-516 / transforms.py:50-188), the
duration arithmetic and the duration-driven expansion of the prior (models.py:474-487) -- runs on the
kernels of csrc/tts.hip plus the MFMA conv kernel for every dense 1x1 / k3 conv.  The frame-rate back
end (flow in reverse, HiFi-GAN generator: 98 % of the FLOPs) is the converter engine's
(``engine.ConverterEngine._flow``, ``generator_fp32.GeneratorFp32.decode``), conditioned on the speaker-table embedding.

Load-time transforms: the q, k, v projections of a layer are concatenated into one 576-row conv; the
single-row ``dp.proj`` and the 29-row spline projections are zero-padded to 32 rows (the conv kernel
stores whole 32-row fragments); the Flips between the spline flows are not materialised (channel roles
alternate); of ``sdp.flows.0`` (ElementwiseAffine) only channel 0 is ever read, so it is two scalars.
"""
import math
import numbers

import torch

from . import _lib
from . import noise as noise_mod
from ._lib import F_MASK_V, LN_POST_GELU, LN_PRE_RELU
from .engine import ConverterEngine, PackedConv, item_tau, on_own_device, padded_frames, wavenet_keyword  # noqa: F401
from .params import ATTN_WINDOW, SDP_DDS_LAYERS, SDP_FLOWS, SDP_KERNEL, SDP_NUM_BINS, SDP_TAIL_BOUND

LN_EPS = 1e-5   # modules.LayerNorm / attentions.LayerNorm default
# ov_rel_attention_f32 keeps 8 query rows of scores against all Tx keys in LDS next to its q and k / v tiles:
# (8 * 96 + 96 * 65 + 8 * Tx) * 4 bytes <= 64 KiB (csrc/tts.hip), so Tx <= 1172 tokens per utterance.
MAX_TOKENS = (64 * 1024 // 4 - 8 * 96 - 96 * 65) // 8


def check_token_count(Tx):
    """Refuse a token axis that the attention kernel cannot hold, in words instead of its OV_E_UNSUPPORTED."""
    if Tx > MAX_TOKENS:
        raise ValueError(f"infer: token axis of {Tx} tokens, but the text encoder's attention kernel holds at most "
                         f"{MAX_TOKENS}; split the text into shorter pieces (BaseSpeakerTTS splits by sentence)")


CONTROLS = ("noise_scale", "length_scale", "noise_scale_w", "sdp_ratio")


def _is_number(v):
    """One value for the whole batch: a Python (or numpy) number, or a tensor / array of exactly zero dimensions."""
    return isinstance(v, numbers.Real) or (hasattr(v, "ndim") and v.ndim == 0)


def item_controls(B, noise_scale, length_scale, noise_scale_w, sdp_ratio):
    """The four synthesis controls of ``infer`` as per-item values.  Each is one number for the batch or a sequence /
    tensor of ``B`` numbers.  All four plain numbers: returns None (the scalar kernels run).  Any of them per item:
    returns ``{name: [B floats]}`` with the plain numbers broadcast.  A per-item control of the wrong length, a
    non-finite value in it, or a per-item ``length_scale <= 0`` is a ValueError.  ``sdp_ratio`` is not confined to
    [0, 1]: the reference's ``sdp * r + dp * (1 - r)`` (models.py:474) extrapolates outside it and so do the kernels.
    (The conversion's per-item control, ``tau``, is validated by ``item_tau``, defined in ``engine`` and re-exported here.)"""
    given = dict(zip(CONTROLS, (noise_scale, length_scale, noise_scale_w, sdp_ratio)))
    if all(_is_number(v) for v in given.values()):
        return None
    out = {}
    for name, v in given.items():
        if _is_number(v):
            out[name] = [float(v)] * B
            continue
        vals = [float(x) for x in (v.detach().reshape(-1).cpu().tolist() if isinstance(v, torch.Tensor) else list(v))]
        if len(vals) != B:
            raise ValueError(f"infer: {name} has {len(vals)} values for a batch of {B}; give one number, or one per item")
        if not all(math.isfinite(x) for x in vals):
            raise ValueError(f"infer: {name} holds a non-finite value: {vals}")
        if name == "length_scale" and not all(x > 0 for x in vals):
            raise ValueError(f"infer: length_scale must be positive for every item, got {vals}")
        out[name] = vals
    return out


def _pad_rows(w, b, rows):
    """Zero-pad a [r, Cin, K] weight and its bias to ``rows`` output rows."""
    wp = torch.zeros(rows, w.shape[1], w.shape[2], dtype=torch.float32)
    wp[:w.shape[0]] = w
    bp = torch.zeros(rows, dtype=torch.float32)
    bp[:b.shape[0]] = b
    return wp, bp


class _DDS:
    """Packed DDSConv (reference: openvoice/modules.py:84-130)."""

    def __init__(self, sd, prefix, device):
        self.layers = []
        for i in range(SDP_DDS_LAYERS):
            self.layers.append(dict(
                dil=SDP_KERNEL ** i,
                w_sep=sd[f"{prefix}.convs_sep.{i}.weight"][:, 0].contiguous().to(device),
                b_sep=sd[f"{prefix}.convs_sep.{i}.bias"].contiguous().to(device),
                c1x1=PackedConv(sd[f"{prefix}.convs_1x1.{i}.weight"], sd[f"{prefix}.convs_1x1.{i}.bias"], device, K=1),
                g1=sd[f"{prefix}.norms_1.{i}.gamma"].to(device), b1=sd[f"{prefix}.norms_1.{i}.beta"].to(device),
                g2=sd[f"{prefix}.norms_2.{i}.gamma"].to(device), b2=sd[f"{prefix}.norms_2.{i}.beta"].to(device)))


class TtsEngine:
    """Kernel-level implementation of the V1 TTS model for one device."""

    def __init__(self, state_dict, model_cfg, spec_channels, device, n_vocab, n_speakers):
        self.device = torch.device(device)
        cfg = dict(model_cfg.items()) if hasattr(model_cfg, "items") else dict(model_cfg)
        self.cfg = cfg
        self.core = ConverterEngine(state_dict, cfg, spec_channels, device, zero_g=False)
        sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        dev = self.device
        self.n_vocab, self.n_speakers = n_vocab, n_speakers
        H = self.H = cfg["hidden_channels"]
        self.inter = cfg["inter_channels"]
        self.n_heads, self.n_layers, ks = cfg["n_heads"], cfg["n_layers"], cfg["kernel_size"]
        assert ks % 2 == 1, "FFN 'same' padding is symmetric only for odd kernels (attentions.py:457-465)"
        self.emb = sd["enc_p.emb.weight"].contiguous().to(dev)
        self.layers = []
        for i in range(self.n_layers):
            a, f = f"enc_p.encoder.attn_layers.{i}", f"enc_p.encoder.ffn_layers.{i}"
            wqkv = torch.cat([sd[f"{a}.conv_{c}.weight"] for c in "qkv"], 0)
            bqkv = torch.cat([sd[f"{a}.conv_{c}.bias"] for c in "qkv"], 0)
            self.layers.append(dict(
                qkv=PackedConv(wqkv, bqkv, dev, K=1),
                o=PackedConv(sd[a + ".conv_o.weight"], sd[a + ".conv_o.bias"], dev, K=1),
                emb_k=sd[a + ".emb_rel_k"][0].contiguous().to(dev), emb_v=sd[a + ".emb_rel_v"][0].contiguous().to(dev),
                g1=sd[f"enc_p.encoder.norm_layers_1.{i}.gamma"].to(dev), b1=sd[f"enc_p.encoder.norm_layers_1.{i}.beta"].to(dev),
                ffn1=PackedConv(sd[f + ".conv_1.weight"], sd[f + ".conv_1.bias"], dev, K=ks),
                ffn2=PackedConv(sd[f + ".conv_2.weight"], sd[f + ".conv_2.bias"], dev, K=ks),
                g2=sd[f"enc_p.encoder.norm_layers_2.{i}.gamma"].to(dev), b2=sd[f"enc_p.encoder.norm_layers_2.{i}.beta"].to(dev)))
        self.proj = PackedConv(sd["enc_p.proj.weight"], sd["enc_p.proj.bias"], dev, K=1)
        # duration predictor
        self.dp_cond_w = sd["dp.cond.weight"][:, :, 0].contiguous().to(dev)
        self.dp_cond_b = sd["dp.cond.bias"].contiguous().to(dev)
        self.dp_c1 = PackedConv(sd["dp.conv_1.weight"], sd["dp.conv_1.bias"], dev, K=sd["dp.conv_1.weight"].shape[2])
        self.dp_c2 = PackedConv(sd["dp.conv_2.weight"], sd["dp.conv_2.bias"], dev, K=sd["dp.conv_2.weight"].shape[2])
        self.dp_n = [(sd[f"dp.norm_{n}.gamma"].to(dev), sd[f"dp.norm_{n}.beta"].to(dev)) for n in (1, 2)]
        self.dp_filter = sd["dp.conv_1.weight"].shape[0]
        wp, bp = _pad_rows(sd["dp.proj.weight"], sd["dp.proj.bias"], 32)
        self.dp_proj = PackedConv(wp, bp, dev, K=1)
        # stochastic duration predictor (reverse direction only)
        self.sdp_filter = F = sd["sdp.pre.weight"].shape[0]
        self.sdp_pre = PackedConv(sd["sdp.pre.weight"], sd["sdp.pre.bias"], dev, K=1)
        self.sdp_cond_w = sd["sdp.cond.weight"][:, :, 0].contiguous().to(dev)
        self.sdp_cond_b = sd["sdp.cond.bias"].contiguous().to(dev)
        self.sdp_convs = _DDS(sd, "sdp.convs", dev)
        self.sdp_proj = PackedConv(sd["sdp.proj.weight"], sd["sdp.proj.bias"], dev, K=1)
        self.sdp_flows = []
        for f in range(SDP_FLOWS, 1, -1):          # reverse order; ConvFlow 1 is dropped (models.py:173)
            p = f"sdp.flows.{2 * f - 1}"
            wp, bp = _pad_rows(sd[p + ".proj.weight"], sd[p + ".proj.bias"], 32)
            self.sdp_flows.append(dict(pre_w=sd[p + ".pre.weight"][:, 0, 0].contiguous().to(dev),
                                       pre_b=sd[p + ".pre.bias"].contiguous().to(dev),
                                       dds=_DDS(sd, p + ".convs", dev), proj=PackedConv(wp, bp, dev, K=1)))
        self.ea_m = float(sd["sdp.flows.0.m"][0, 0])
        self.ea_logs = float(sd["sdp.flows.0.logs"][0, 0])
        self.emb_g = sd["emb_g.weight"].contiguous().to(dev)

    # ---- helpers ---------------------------------------------------------------------------------------
    def _conv(self, layer, x, xc, out, oc, B, T, ld, **kw):
        """Token-rate conv: x (B, xc, ld) -> out (B, oc, ld)."""
        self.core.launcher.conv(layer, x, 0, xc * ld, out, 0, oc * ld, B, T, x_ld=ld, out_ld=ld, tag="tts", **kw)

    def _ln(self, x, gamma, beta, out, B, C, T, ld, res=None, res2=None, mask=None, flags=0):
        _lib.call("ov_layernorm_ch_f32", x, res, gamma, beta, res2, mask, out, B, C, T, ld, LN_EPS, flags)

    def _dds(self, dds, x, tmp1, tmp2, mask, B, C, T, ld):
        """DDSConv in place on ``x`` (modules.py:117-130); ``x`` already holds ``x + g`` when conditioned."""
        n = len(dds.layers)
        for i, L in enumerate(dds.layers):
            _lib.call("ov_dwconv1d_f32", x, L["w_sep"], L["b_sep"], mask, tmp1, B, C, T, ld, SDP_KERNEL, L["dil"])
            self._ln(tmp1, L["g1"], L["b1"], tmp1, B, C, T, ld, flags=LN_POST_GELU)
            self._conv(L["c1x1"], tmp1, C, tmp2, C, B, T, ld)
            # x = x + gelu(LN(y)); the block's final `x * mask` rides on the last layer
            self._ln(tmp2, L["g2"], L["b2"], x, B, C, T, ld, res2=x, mask=mask if i == n - 1 else None,
                     flags=LN_POST_GELU)

    # ---- the path ----------------------------------------------------------------------------------------
    def _wavenet_cores(self):
        return (self.core,)

    @torch.no_grad()
    @on_own_device
    def front(self, tokens, lengths, sid, noise_scale=1.0, length_scale=1.0, noise_scale_w=1.0, sdp_ratio=0.2,
              noise_w=None, *, seed=None):
        """The token-rate front half of ``infer`` (models.py:468-479): text encoder, both duration predictors and the
        duration arithmetic, for a padded batch.  Everything here runs at the token rate and nothing waits for the host;
        the caller makes the one sync when it reads ``y_len``.  Arguments as for ``infer`` (``noise_scale`` is only
        validated and uploaded with the other controls: the expansion applies it).  Returns a dict: ``stats``
        ``[B, 2 * inter, Lx]`` (``m`` and ``logs`` of every token: the two halves), ``cum`` ``[B, Lx]`` int32 (inclusive
        prefix sums of the durations), ``y_len`` ``[B]`` int64, ``logw`` ``[B, Lx]``, ``g`` ``[B, gin]`` (the speaker
        embeddings), ``lengths``, ``B`` / ``Tx`` / ``Lx``, ``items`` (``item_controls``), ``noise_scale_b`` (its device
        vector or None), ``streams`` (``noise.rows`` of ``seed`` or None) and ``zeros`` (the allocator).  ``infer`` is
        this followed by the frame-rate back half."""
        dev = self.device
        noise_mod.exclusive(seed, noise_w=noise_w)
        check_token_count(tokens.shape[-1])
        items = item_controls(tokens.shape[0], noise_scale, length_scale, noise_scale_w, sdp_ratio)
        if items is not None:       # one host -> device copy: row i is control i of CONTROLS, one value per item
            ctl = torch.tensor([items[name] for name in CONTROLS], dtype=torch.float32).to(dev)
            noise_scale_b, length_scale_b, noise_scale_w_b, sdp_ratio_b = ctl[0], ctl[1], ctl[2], ctl[3]
        else:
            noise_scale_b = None
        tokens = tokens.to(dev, torch.int64).contiguous()
        lengths = lengths.to(dev, torch.int64).contiguous()
        sid = sid.to(dev, torch.int64).reshape(-1)
        B, Tx = tokens.shape
        if int(tokens.min()) < 0 or int(tokens.max()) >= self.n_vocab:
            raise IndexError("token id out of range")            # nn.Embedding's error in the reference
        if int(sid.min()) < 0 or int(sid.max()) >= self.n_speakers:
            raise IndexError("speaker id out of range")
        H, C, Lx = self.H, self.inter, padded_frames(Tx)
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        x, y, mask = f(B, H, Lx), f(B, H, Lx), f(B, Lx)
        _lib.call("ov_sequence_mask_f32", lengths, mask, B, Tx, Lx)
        _lib.call("ov_embed_f32", tokens, self.emb, lengths, x, B, Tx, H, self.n_vocab, Lx, math.sqrt(H))
        # ---- text encoder (attentions.py:104-121) ---------------------------------------------------------
        qkv, att = f(B, 3 * H, Lx), f(B, H, Lx)
        filt = self.layers[0]["ffn1"].rows
        hid = f(B, filt, Lx)
        dk = H // self.n_heads
        for L in self.layers:
            self._conv(L["qkv"], x, H, qkv, 3 * H, B, Tx, Lx)
            _lib.call("ov_rel_attention_f32", qkv, (qkv, H * Lx), (qkv, 2 * H * Lx), L["emb_k"], L["emb_v"], mask, att,
                      3 * H * Lx, H * Lx, B, self.n_heads, dk, Tx, Lx, ATTN_WINDOW)
            self._conv(L["o"], att, H, y, H, B, Tx, Lx)
            self._ln(x, L["g1"], L["b1"], x, B, H, Tx, Lx, res=y, mask=mask)
            self._conv(L["ffn1"], x, H, hid, filt, B, Tx, Lx, flags=F_MASK_V, mask=mask, mask_bs=Lx)
            self._conv(L["ffn2"], hid, filt, y, H, B, Tx, Lx, in_slope=0.0, flags=F_MASK_V, mask=mask, mask_bs=Lx)
            self._ln(x, L["g2"], L["b2"], x, B, H, Tx, Lx, res=y, mask=mask)
        stats = f(B, 2 * C, Lx)
        self._conv(self.proj, x, H, stats, 2 * C, B, Tx, Lx, flags=F_MASK_V, mask=mask, mask_bs=Lx)
        g = self.emb_g.index_select(0, sid).contiguous()                       # [B, gin]  (models.py:470)
        # ---- duration predictor (models.py:86-100) --------------------------------------------------------
        Fd = self.dp_filter
        xd, d1, d2, dp_out = f(B, H, Lx), f(B, Fd, Lx), f(B, Fd, Lx), f(B, 32, Lx)
        cg = self.core.launcher.linear(g, self.dp_cond_w, self.dp_cond_b)
        _lib.call("ov_add_bias_mask_f32", x, cg, mask, xd, B, H, Tx, Lx)
        self._conv(self.dp_c1, xd, H, d1, Fd, B, Tx, Lx)
        self._ln(d1, *self.dp_n[0], d1, B, Fd, Tx, Lx, mask=mask, flags=LN_PRE_RELU)
        self._conv(self.dp_c2, d1, Fd, d2, Fd, B, Tx, Lx)
        self._ln(d2, *self.dp_n[1], d2, B, Fd, Tx, Lx, mask=mask, flags=LN_PRE_RELU)
        self._conv(self.dp_proj, d2, Fd, dp_out, 32, B, Tx, Lx, flags=F_MASK_V, mask=mask, mask_bs=Lx)
        # ---- stochastic duration predictor, reverse (models.py:129-138, :171-180) -------------------------
        Fs = self.sdp_filter
        xs, t1, t2, hflow, hp = f(B, Fs, Lx), f(B, Fs, Lx), f(B, Fs, Lx), f(B, Fs, Lx), f(B, 32, Lx)
        cs = self.core.launcher.linear(g, self.sdp_cond_w, self.sdp_cond_b)
        self._conv(self.sdp_pre, x, H, xs, Fs, B, Tx, Lx, bias_b=cs, bias_b_bs=Fs)
        self._dds(self.sdp_convs, xs, t1, t2, mask, B, Fs, Tx, Lx)
        self._conv(self.sdp_proj, xs, Fs, t1, Fs, B, Tx, Lx, flags=F_MASK_V, mask=mask, mask_bs=Lx)
        xs, t1 = t1, xs                                                         # xs = conditioning of the flows
        streams = None
        if seed is not None:
            streams = noise_mod.rows(seed, B)
            noise_w = torch.empty(B, 2, Tx, dtype=torch.float32, device=dev)
            noise_mod.fill([(s, k, noise_mod.PURPOSE_TTS_W, f0, Tx, b * 2 * Tx, Tx)
                            for b, (s, k, f0) in enumerate(streams)], 2, noise_w)
        elif noise_w is None:
            noise_w = torch.randn(B, 2, Tx, dtype=torch.float32, device=dev)
        zw = f(B, 2, Lx)
        if items is None:
            zw[:, :, :Tx].copy_(noise_w.to(dev, torch.float32) * float(noise_scale_w))
        else:                       # a product of two fp32 numbers has one result: the scalar path's bits per item
            zw[:, :, :Tx].copy_(noise_w.to(dev, torch.float32) * noise_scale_w_b.view(B, 1, 1))
        c0, c1 = 1, 0                                                           # a Flip precedes every ConvFlow
        for fl in self.sdp_flows:
            _lib.call("ov_expand1_f32", (zw, c0 * Lx), 2 * Lx, fl["pre_w"], fl["pre_b"], xs, hflow, B, Fs, Tx, Lx)
            self._dds(fl["dds"], hflow, t1, t2, mask, B, Fs, Tx, Lx)
            self._conv(fl["proj"], hflow, Fs, hp, 32, B, Tx, Lx, flags=F_MASK_V, mask=mask, mask_bs=Lx)
            _lib.call("ov_rq_spline_inverse_f32", zw, 2 * Lx, c0, c1, hp, 32 * Lx, mask, B, Tx, Lx, SDP_NUM_BINS, Fs,
                      SDP_TAIL_BOUND)
            c0, c1 = c1, c0
        # after the last Flip logical channel 0 is physical channel 0: logw_sdp = EA^-1(z)[0]
        logw = f(B, Lx)
        cum = torch.zeros(B, Lx, dtype=torch.int32, device=dev)
        y_len = torch.zeros(B, dtype=torch.int64, device=dev)
        if items is None:
            _lib.call("ov_duration_f32", zw, 2 * Lx, self.ea_m, self.ea_logs, dp_out, 32 * Lx, mask, logw, cum, y_len,
                      B, Tx, Lx, float(sdp_ratio), float(length_scale))
        else:
            _lib.call("ov_duration_items_f32", zw, 2 * Lx, self.ea_m, self.ea_logs, dp_out, 32 * Lx, mask, logw, cum,
                      y_len, B, Tx, Lx, sdp_ratio_b, length_scale_b)
        return dict(stats=stats, cum=cum, y_len=y_len, logw=logw, g=g, lengths=lengths, B=B, Tx=Tx, Lx=Lx, items=items,
                    noise_scale_b=noise_scale_b, streams=streams, zeros=f)

    @wavenet_keyword
    @torch.no_grad()
    @on_own_device
    def infer(self, tokens, lengths, sid, noise_scale=1.0, length_scale=1.0, noise_scale_w=1.0, sdp_ratio=0.2,
              max_len=None, noise_w=None, noise_z=None, return_attn=True, skip_padding=False, *, seed=None,
              generator="fp32"):
        """Same contract as the reference (models.py:467-490): returns
        ``(o [B,1,256*Ty'], attn [B,1,Ty,Tx], y_mask [B,1,Ty], (z, z_p, m_p, logs_p) [B,192,Ty])``.
        ``noise_w`` [B,2,Tx] / ``noise_z`` [B,192,>=Ty] replace the reference's two RNG draws when given.
        ``seed`` (instead of them): both draws counter-based (``noise.py``), row ``b`` of an int ``s`` on stream
        ``(s, b)`` (or one seed / pair per row): ``noise_w`` is purpose 1 over the token positions ``[0, Tx)``,
        ``noise_z`` purpose 2 over the frames ``[0, Ty)``, generated straight into the workspace rows once ``Ty`` is
        known -- nobody has to guess a bound for it.
        ``skip_padding``: the generator computes only ``y_length + core.generator.limit_margin(B, Ty)`` frames (16-20) of each
        utterance of a padded batch
        (valid samples bit-identical, the padded tail of ``o`` zero; ``ConverterEngine.voice_conversion``).
        ``generator``: ``"fp32"`` (default) or ``"bf16"`` -- the generator alone on the bf16 channels-last kernels
        (``bf16.GeneratorBf16``, built on first use; ``use_bf16_generator`` is neither read nor set), everything before
        it unchanged: ``attn``, ``y_mask`` and the four latents are the fp32 call's bits.  With ``skip_padding`` the
        padded batch then runs as a few dense length groups (``GeneratorBf16.decode_groups``: valid samples the bits of
        the padded bf16 run, the tail zero), without it as one padded ``GeneratorBf16.decode``.
        ``noise_scale`` / ``length_scale`` / ``noise_scale_w`` / ``sdp_ratio``: each one number for the batch, or a
        sequence / tensor with one value per item (``item_controls``).  Four plain numbers are the scalar launches
        (``ov_duration_f32``, ``ov_expand_prior_f32``); otherwise all four become ``[B]`` device vectors and
        ``ov_duration_items_f32`` / ``ov_expand_prior_items_f32`` run in their place: item ``b`` gets the durations,
        alignment and prior that a call with item ``b``'s four numbers gives it, bit for bit; everything downstream
        (flow, generator, ``skip_padding``, ``seed``) is per item already."""
        _lib.check_generator(generator)
        noise_mod.exclusive(seed, noise_w=noise_w, noise_z=noise_z)
        fh = self.front(tokens, lengths, sid, noise_scale=noise_scale, length_scale=length_scale,
                        noise_scale_w=noise_scale_w, sdp_ratio=sdp_ratio, noise_w=noise_w, **noise_mod.kw(seed))
        dev, f = self.device, fh["zeros"]
        items, noise_scale_b, streams = fh["items"], fh["noise_scale_b"], fh["streams"]
        lengths, stats, cum, y_len, logw, g = fh["lengths"], fh["stats"], fh["cum"], fh["y_len"], fh["logw"], fh["g"]
        B, Tx, Lx, C = fh["B"], fh["Tx"], fh["Lx"], self.inter
        if generator == "bf16":       # the same one sync, carrying every length: decode_groups plans on the host
            y_host = y_len.cpu().tolist()
            Ty = max(y_host)
        else:
            Ty = int(y_len.max())                                               # host sync, as in the reference
        # ---- expansion + prior sample + flow (reverse) + generator ---------------------------------------
        core = self.core
        ws = core._workspace(B, Ty)
        Ly, mask_y = ws["Tp"], ws["mask"]
        _lib.call("ov_sequence_mask_f32", y_len, mask_y, B, Ty, Ly)
        if seed is not None:
            core.seed_noise(ws["noise"], streams, B, Ty, Ly, purpose=noise_mod.PURPOSE_TTS_Z)
        else:
            if noise_z is None:
                noise_z = torch.randn(B, C, Ty, dtype=torch.float32, device=dev)
            ws["noise"][:, :, :Ty].copy_(noise_z[:, :, :Ty].to(dev, torch.float32))
        m_p, logs_p = f(B, C, Ly), f(B, C, Ly)
        attn = f(B, Ty, Tx) if return_attn else None
        z_p, z = ws["z_p"], ws["z_hat"]
        if items is None:
            _lib.call("ov_expand_prior_f32", stats, (stats, C * Lx), 2 * C * Lx, Lx, cum, lengths, y_len, ws["noise"],
                      C * Ly, Ly, z_p, m_p, logs_p, attn, B, C, Tx, Ty, Ly, float(noise_scale))
        else:
            _lib.call("ov_expand_prior_items_f32", stats, (stats, C * Lx), 2 * C * Lx, Lx, cum, lengths, y_len,
                      ws["noise"], C * Ly, Ly, z_p, m_p, logs_p, attn, B, C, Tx, Ty, Ly, noise_scale_b)
        cond_flow = [core._wn_cond(cp["wn"], g) for cp in core.couplings]
        core._flow(z_p, z, ws, B, Ty, cond_flow, mask_y, reverse=True)      # z_p -> z, no copy
        cond_d = core.generator.cond(g)
        Td = Ty if max_len is None else min(Ty, int(max_len))
        if generator == "bf16":
            gen = core.bf16_generator()
            if skip_padding:
                o = gen.decode_groups(z, Ly, gen.cond_rows(g), y_host, Td)
            else:
                o = gen.decode(z[:, :, :Td], g.unsqueeze(-1))
        else:
            gen = core.generator
            o = gen.decode(z, cond_d, ws, T=Td, limits=gen.frame_limits(y_len, Td) if skip_padding else None)
        outs = tuple(t[:, :, :Ty].contiguous() for t in (z, z_p, m_p, logs_p))
        self.last_logw = logw[:, :Tx]
        return (o, attn.unsqueeze(1) if attn is not None else None, mask_y[:, :Ty].unsqueeze(1).contiguous(), outs)
