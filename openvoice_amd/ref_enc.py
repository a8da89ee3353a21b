"""The ReferenceEncoder of a converter checkpoint (``extract_se``; reference: openvoice/models.py:339-364) on the MI355X
kernels: dense batches and ragged ones (csrc/ref_enc_ragged.hip).  Not part of a conversion."""
import torch

from . import _lib
from .launch import PackedConv, on_own_device
from .params import REF_ENC_FILTERS, REF_ENC_GRU, effective_weight


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


class ReferenceEncoder:
    """The ``ref_enc.*`` weights of ``sd`` (float32, host) in kernel-ready form on ``device``, and the launch sequences
    over them; ``launcher``: the ``launch.Launcher`` of the device."""

    def __init__(self, sd, spec_channels, device, launcher):
        self.device, self.spec_channels, self.launcher = torch.device(device), spec_channels, launcher
        dev = self.device
        self.convs = [(effective_weight(sd, f"ref_enc.convs.{i}").contiguous().to(dev),
                       sd[f"ref_enc.convs.{i}.bias"].contiguous().to(dev)) for i in range(len(REF_ENC_FILTERS))]
        self.ln_w = sd["ref_enc.layernorm.weight"].contiguous().to(dev)
        self.ln_b = sd["ref_enc.layernorm.bias"].contiguous().to(dev)
        self.gru_in = PackedConv(sd["ref_enc.gru.weight_ih_l0"].unsqueeze(-1), sd["ref_enc.gru.bias_ih_l0"], dev, K=1)
        self.whh_t = sd["ref_enc.gru.weight_hh_l0"].t().contiguous().to(dev)
        self.bhh = sd["ref_enc.gru.bias_hh_l0"].contiguous().to(dev)
        self.proj_w = sd["ref_enc.proj.weight"].contiguous().to(dev)
        self.proj_b = sd["ref_enc.proj.bias"].contiguous().to(dev)

    def __getitem__(self, name):
        """The weights under the names they had as a dict (``ref_enc["convs"]``, ``["ln_w"]``, ...)."""
        return getattr(self, name)

    @torch.no_grad()
    @on_own_device
    def __call__(self, spec_t):
        """``spec_t`` [N, Ty, n_freq] (the transposed spectrogram the reference API passes,
        openvoice/api.py:131) -> [N, gin]; reference: openvoice/models.py:339-359.  Internally every
        tensor is [N][C][F][T] (time contiguous), i.e. the un-transposed spectrogram: when the caller
        passes ``spec.transpose(1, 2)`` the transpose back is a view and nothing is copied."""
        dev = self.device
        x = spec_t.to(dev, torch.float32).transpose(1, 2).contiguous()     # [N, F, T]
        N, F, T = x.shape
        assert F == self.spec_channels
        cur = torch.empty_like(x)
        _lib.call("ov_layernorm_freq_f32", x, self.ln_w, self.ln_b, cur, N, F, T, 1e-5)
        cin = 1
        for w, b in self.convs:
            cout = w.shape[0]
            Fo, To = (F - 1) // 2 + 1, (T - 1) // 2 + 1
            nxt = torch.empty(N, cout, Fo, To, dtype=torch.float32, device=dev)
            _lib.call("ov_conv2d_s2_relu_f32", cur, w, b, nxt, N, cin, cout, F, T)
            cur, cin, F, T = nxt, cout, Fo, To
        feat = cin * F                                                        # 128 * 9 = 1152
        H = REF_ENC_GRU
        gi = torch.empty(N, 3 * H, T, dtype=torch.float32, device=dev)
        self.launcher.conv(self.gru_in, cur, 0, feat * T, gi, 0, 3 * H * T, N, T, tag="gru_in")
        h = torch.empty(N, H, dtype=torch.float32, device=dev)
        _lib.call("ov_gru_f32", gi, self.whh_t, self.bhh, h, N, H, T)
        return self.launcher.linear(h, self.proj_w, self.proj_b)

    @torch.no_grad()
    @on_own_device
    def reference_encoder_ragged(self, spec, frames):
        """The dense call for P items of DIFFERENT lengths in one launch sequence (csrc/ref_enc_ragged.hip).
        ``spec`` [P, n_freq, W] float32, un-transposed (time contiguous); rows may be padded -- a ``[:, :, :W]`` view of
        a ``[P, n_freq, ld]`` buffer is taken as it is.  ``frames``: host sequence of P ints, item p's own number of
        frames, ``1 <= frames[p] <= W``; what the buffer holds beyond them is never read (it may be NaN).  Returns
        [P, gin]: row p is what the dense call gives for ``spec[p:p + 1, :, :frames[p]]`` alone -- LayerNorm,
        the six convs and the GRU bit for bit (each ragged kernel performs its dense twin's operations in the twin's
        order, with the conv's zero padding at the item's own end and the GRU stopping after its last true step); the
        MFMA ``gru_in`` conv in between is column-independent.  The per-layer length table (7 rows of P,
        ``ref_enc_lengths``) is built on the host and uploaded in one copy."""
        cur, steps, L = self._reference_encoder_ragged_stack(spec, frames)
        P, H = cur.shape[0], REF_ENC_GRU
        feat = cur.shape[1] * cur.shape[2]                                    # 128 * 9 = 1152
        gi = torch.empty(P, 3 * H, L, dtype=torch.float32, device=self.device)
        self.launcher.conv(self.gru_in, cur, 0, feat * L, gi, 0, 3 * H * L, P, L, tag="gru_in")
        h = torch.empty(P, H, dtype=torch.float32, device=self.device)
        _lib.call("ov_gru_ragged_f32", gi, self.whh_t, self.bhh, steps, h, P, H, L)
        return self.launcher.linear(h, self.proj_w, self.proj_b)

    @torch.no_grad()
    @on_own_device
    def _reference_encoder_ragged_stack(self, spec, frames):
        """The first half of ``reference_encoder_ragged`` -- ragged LayerNorm and the six ragged convs (not part of the
        public surface: a seam for tests/test_gpu_enrol.py, which compares the conv stack's output with the dense one's):
        ``(out [P, 128, 9, L], steps, L)`` with ``steps`` the device int32 [P] GRU step counts (the last row of the
        length table) and ``L`` the row stride; columns at and beyond ``steps[p]`` of item p are 0."""
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
        n_convs = len(self.convs)
        table = torch.tensor([list(col) for col in zip(*(ref_enc_lengths(f, n_convs) for f in frames))],
                             dtype=torch.int32).to(dev)                       # [n_convs + 1, P], one copy
        lds = ref_enc_lengths(ld, n_convs)
        cur = torch.empty(P, F, ld, dtype=torch.float32, device=dev)
        _lib.call("ov_layernorm_freq_ragged_f32", x, self.ln_w, self.ln_b, table[0], cur, P, F, ld, 1e-5)
        cin = 1
        for k, (w, b) in enumerate(self.convs):
            cout = w.shape[0]
            Fo = (F - 1) // 2 + 1
            nxt = torch.empty(P, cout, Fo, lds[k + 1], dtype=torch.float32, device=dev)
            _lib.call("ov_conv2d_s2_relu_ragged_f32", cur, w, b, table[k], nxt, P, cin, cout, F, lds[k], lds[k + 1])
            cur, cin, F = nxt, cout, Fo
        return cur, table[n_convs], lds[-1]
