"""Linear-magnitude spectrogram front-end of the converter (same signature as the reference's
``spectrogram_torch``, reference: openvoice/mel_processing.py:40-75):

    reflect-pad (n_fft - hop)/2 -> STFT (periodic Hann, center=False, onesided) -> sqrt(re^2 + im^2 + 1e-6)

On a ROCm device the whole thing is two launches of this repo's own kernels (no rocFFT, no eager
elementwise ops): ``ov_frame_hops_f32`` lays the reflect-padded waveform out as (B, hop, U) "hop
phases", after which -- because n_fft = 4 * hop for every released config -- the windowed DFT of frame t
is a 4-tap conv over u with ``hop`` input channels and 2 * (n_fft/2 + 1) output rows, run on the fp32
MFMA conv kernel with the magnitude fused into its epilogue (``OV_EPI_MAGNITUDE``: real / imaginary
rows paired in one wave, like the WaveNet gate).  DFT-as-GEMM costs 1.8 GFLOP per 10 s utterance against
0.05 for an FFT -- 0.3 % of a conversion -- and removes ~10 launches, three full-size temporaries and the
FFT library from the path.  Weights ``hann[n] * cos / -sin(2 pi f n / n_fft)`` are built once in float64.

For CPU tensors (host-side tooling, the CPU test-suite) and for configs with n_fft != 4 * hop the
function evaluates the same definition with ``torch.stft``; the engine itself never runs on CPU.

Difference from the reference, on purpose: the reference evaluates ``torch.min(y) < -1.1`` /
``torch.max(y) > 1.1`` as Python bools purely to print a warning, which costs two device->host
syncs per call (hard part 7).  Here the range check runs only when
``OV_CHECK_RANGE=1`` is set.
"""
import math
import os

import torch

_hann = {}
_native = {}


class _NativeSpectrogram:
    """Packed DFT weights + launch logic for one (device, n_fft, hop)."""

    def __init__(self, device, n_fft, hop):
        from .engine import PackedConv
        self.device, self.n_fft, self.hop = device, n_fft, hop
        self.bins = n_fft // 2 + 1
        tiles = (self.bins + 31) // 32
        n = torch.arange(n_fft, dtype=torch.float64)
        window = 0.5 - 0.5 * torch.cos(2 * math.pi * n / n_fft)                   # periodic Hann (torch.hann_window)
        f = torch.arange(self.bins, dtype=torch.float64)[:, None]
        ang = 2 * math.pi * f * n[None, :] / n_fft
        re, im = window * torch.cos(ang), -window * torch.sin(ang)               # [bins, n_fft]
        w = torch.zeros(tiles * 64, n_fft, dtype=torch.float64)                   # row pairing: tile 2q re, 2q+1 im
        for q in range(tiles):
            lo, hi = 32 * q, min(32 * q + 32, self.bins)
            w[64 * q: 64 * q + hi - lo] = re[lo:hi]
            w[64 * q + 32: 64 * q + 32 + hi - lo] = im[lo:hi]
        # conv weight [rows, Cin = hop, K = 4]: W[r][c][j] = w[r][hop * j + c]
        wc = w.reshape(tiles * 64, n_fft // hop, hop).transpose(1, 2).contiguous().float()
        self.layer = PackedConv(wc, None, device, K=n_fft // hop, cout=self.bins)

    def __call__(self, y):
        from . import _lib
        from .engine import launch_conv, padded_frames
        y = y.contiguous()
        B, N = y.shape
        pad = (self.n_fft - self.hop) // 2
        if pad >= N:
            raise ValueError("waveform shorter than the reflect padding")       # torch's reflect pad raises too
        T = (N + 2 * pad - self.n_fft) // self.hop + 1
        if T < 1:
            raise ValueError("waveform shorter than one frame")
        U = T + self.n_fft // self.hop - 1
        ldu, lds = padded_frames(U), padded_frames(T)
        hops = torch.empty(B, self.hop, ldu, dtype=torch.float32, device=y.device)
        _lib.call("ov_frame_hops_f32", y, hops, B, N, self.hop, pad, U, ldu)
        spec = torch.zeros(B, self.bins, lds, dtype=torch.float32, device=y.device)
        launch_conv(self.layer, hops, 0, self.hop * ldu, spec, 0, self.bins * lds, B, T, epi=_lib.EPI_MAGNITUDE,
                    scale=1e-6, rows=self.layer.rows, x_ld=ldu, out_ld=lds)
        # rows are padded to a multiple of 4 floats (16-byte aligned for the next conv); the caller sees [B, bins, T]
        return spec[:, :, :T]

    def windows(self, wave, n_samples, first_frames, Tw):
        """Spectrogram frames [f0, f0 + Tw) of the 1-D waveform ``wave`` (its first ``n_samples`` samples are the file)
        for every f0 of the device int64 vector ``first_frames``: ``[W, bins, Tw]``, bit-identical to
        ``self(wave[None])[0, :, f0:f0 + Tw]`` without framing the whole file (``ov_frame_hops_windows_f32``, reflect
        padding at the file's true ends only)."""
        from . import _lib
        from .engine import launch_conv, padded_frames
        W = first_frames.shape[0]
        pad = (self.n_fft - self.hop) // 2
        U = Tw + self.n_fft // self.hop - 1
        ldu, lds = padded_frames(U), padded_frames(Tw)
        hops = torch.empty(W, self.hop, ldu, dtype=torch.float32, device=wave.device)
        _lib.call("ov_frame_hops_windows_f32", wave, int(n_samples), first_frames, W, self.hop, pad, U, ldu, hops)
        spec = torch.zeros(W, self.bins, lds, dtype=torch.float32, device=wave.device)
        launch_conv(self.layer, hops, 0, self.hop * ldu, spec, 0, self.bins * lds, W, Tw, epi=_lib.EPI_MAGNITUDE,
                    scale=1e-6, rows=self.layer.rows, x_ld=ldu, out_ld=lds)
        return spec[:, :, :Tw]

    def windows_multi(self, pool, records, Tw):
        """``windows`` with one source per window: ``records`` is a device int64 ``[W, 3]`` of (base, n_samples,
        first_frame), and window w is frames [first_frame, first_frame + Tw) of the waveform
        ``pool[base:base + n_samples]`` (reflect padding at that span's two ends; ``ov_frame_hops_multi_f32``).
        ``[W, bins, Tw]``, bit-identical to ``self.windows(pool[base:base + n_samples], n_samples, ...)`` per window."""
        from . import _lib
        from .engine import launch_conv, padded_frames
        W = records.shape[0]
        pad = (self.n_fft - self.hop) // 2
        U = Tw + self.n_fft // self.hop - 1
        ldu, lds = padded_frames(U), padded_frames(Tw)
        hops = torch.empty(W, self.hop, ldu, dtype=torch.float32, device=pool.device)
        _lib.call("ov_frame_hops_multi_f32", pool, pool.numel(), records, W, self.hop, pad, U, ldu, hops)
        spec = torch.zeros(W, self.bins, lds, dtype=torch.float32, device=pool.device)
        launch_conv(self.layer, hops, 0, self.hop * ldu, spec, 0, self.bins * lds, W, Tw, epi=_lib.EPI_MAGNITUDE,
                    scale=1e-6, rows=self.layer.rows, x_ld=ldu, out_ld=lds)
        return spec[:, :, :Tw]


def native_spectrogram(device, n_fft, hop):
    """The cached ``_NativeSpectrogram`` of (device, n_fft, hop) -- the object ``spectrogram_torch`` runs on a device."""
    device = torch.device(device)
    if n_fft != 4 * hop:
        from ._lib import OvError
        raise OvError(f"native spectrogram: n_fft == 4 * hop only (got {n_fft} / {hop})")
    key = (str(device), n_fft, hop)
    eng = _native.get(key)
    if eng is None:
        eng = _native[key] = _NativeSpectrogram(device, n_fft, hop)
    return eng


def spectrogram_torch(y, n_fft, sampling_rate, hop_size, win_size, center=False):
    if os.environ.get("OV_CHECK_RANGE") == "1":
        lo, hi = torch.min(y), torch.max(y)
        if lo < -1.1:
            print("min value is ", lo)
        if hi > 1.1:
            print("max value is ", hi)
    if y.is_cuda:
        # Device tensors take the native kernels or fail loudly -- never a silent torch.stft / rocFFT fallback.
        if not (y.dtype == torch.float32 and not center and win_size == n_fft and n_fft == 4 * hop_size):
            from ._lib import OvError
            raise OvError(f"native spectrogram: float32, center=False and win_size == n_fft == 4 * hop_size only "
                          f"(every released OpenVoice config: 1024 / 256); got dtype={y.dtype}, center={center}, "
                          f"n_fft={n_fft}, win_size={win_size}, hop_size={hop_size}.  CPU tensors are evaluated with "
                          f"torch.stft (host tooling); there is no rocFFT path on the device")
        key = (str(y.device), n_fft, hop_size)
        eng = _native.get(key)
        if eng is None:
            eng = _native[key] = _NativeSpectrogram(y.device, n_fft, hop_size)
        return eng(y)
    key = (win_size, y.dtype, str(y.device))
    window = _hann.get(key)
    if window is None:
        window = _hann[key] = torch.hann_window(win_size, dtype=y.dtype, device=y.device)
    pad = int((n_fft - hop_size) / 2)
    y = torch.nn.functional.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, n_fft, hop_length=hop_size, win_length=win_size, window=window, center=center,
                      pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    spec = torch.view_as_real(spec)
    return torch.sqrt(spec.pow(2).sum(-1) + 1e-6)
