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
    return _stft_torch(y, n_fft, hop_size, win_size, center)


def _stft_torch(y, n_fft, hop_size, win_size, center):
    """The definition itself, evaluated with ``torch.stft`` (CPU tensors: host tooling and the CPU test-suite)."""
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


# ---- general device STFT and mel features ---------------------------------------------------------------------------
# ``spectrogram_torch`` above stays what it was, in behaviour and in bits.  The functions below are the rest of the
# reference module (openvoice/mel_processing.py:8-33 and :122-183) plus ``stft_magnitude``, the general door to the device
# STFT: csrc/stft.hip, ``ov_stft_mag_f32`` and ``ov_mel_log_f32``.  ``mel_spectrogram_torch`` on a device tensor is the
# two-launch composition of those kernels (the linear spectrogram makes one round trip through memory; DESIGN.md has the
# measured cost).  The definition is ``torch.stft``'s, evaluated in float64 (``stft_magnitude_host``): parity with the
# reference's rocFFT bits is unpinned, as is parity of ``mel_filterbank`` with librosa.

TILE_FRAMES = 32          # frames one workgroup of the two kernels owns (== ov_stft_tile_frames(); the tests size by it)
STFT_MIN_N_FFT, STFT_MAX_N_FFT = 16, 2048
MEL_MAX_MELS, MEL_MAX_BINS = 256, 1025
_U24 = 2.0 ** -24         # unit roundoff of fp32

_stft_packs = {}
_mel_bases = {}


def dynamic_range_compression_torch(x, C=1, clip_val=1e-5):
    return torch.log(torch.clamp(x, min=clip_val) * C)


def dynamic_range_decompression_torch(x, C=1):
    return torch.exp(x) / C


def spectral_normalize_torch(magnitudes):
    return dynamic_range_compression_torch(magnitudes)


def spectral_de_normalize_torch(magnitudes):
    return dynamic_range_decompression_torch(magnitudes)


def _check_range(y, bound):
    if os.environ.get("OV_CHECK_RANGE") == "1":
        lo, hi = torch.min(y), torch.max(y)
        if lo < -bound:
            print("min value is ", lo)
        if hi > bound:
            print("max value is ", hi)


def hz_to_mel(f):
    """Slaney's auditory-toolbox scale (librosa's default, ``htk=False``): 3 mel per 200 Hz below 1000 Hz, then
    logarithmic with ln(6.4) / 27 per mel.  float64 numpy."""
    import numpy as np
    f = np.asarray(f, dtype=np.float64)
    return np.where(f < 1000.0, f * (3.0 / 200.0), 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) * (27.0 / math.log(6.4)))


def mel_to_hz(m):
    """Inverse of ``hz_to_mel``."""
    import numpy as np
    m = np.asarray(m, dtype=np.float64)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((np.maximum(m, 15.0) - 15.0) * (math.log(6.4) / 27.0)))


def mel_filterbank(sampling_rate, n_fft, num_mels, fmin=0.0, fmax=None):
    """float64 numpy ``[num_mels, n_fft // 2 + 1]``: the filterbank ``librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)``
    of librosa 0.9.1 gives with its defaults (what the reference's positional call at openvoice/mel_processing.py:127 gets):
    Slaney scale, Slaney area normalisation.  ``num_mels + 2`` centres equally spaced in mel between ``fmin`` and ``fmax``
    (None: ``sampling_rate / 2``); filter m is the triangle over the bin frequencies ``k * sr / n_fft`` rising from centre m
    to centre m + 1 and falling to centre m + 2, scaled by ``2 / (f[m + 2] - f[m])``.

    Written from that definition: librosa is not a dependency of this package, so parity with librosa is unpinned (it
    returns the same numbers rounded to float32)."""
    import numpy as np
    if fmax is None:
        fmax = sampling_rate / 2.0
    if not (num_mels >= 1 and n_fft >= 2 and sampling_rate > 0):
        raise ValueError(f"mel_filterbank: num_mels >= 1, n_fft >= 2, sampling_rate > 0 (got {num_mels}, {n_fft}, {sampling_rate})")
    if not (0 <= fmin < fmax <= sampling_rate / 2.0):
        raise ValueError(f"mel_filterbank: 0 <= fmin < fmax <= sampling_rate / 2 (got fmin={fmin}, fmax={fmax}, "
                         f"sampling_rate={sampling_rate})")
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sampling_rate) / n_fft)
    centres = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), num_mels + 2))
    fdiff = np.diff(centres)
    ramps = centres[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    return weights * (2.0 / (centres[2:] - centres[:-2]))[:, None]


def _stft_geometry(N, n_fft, hop, win, center):
    """(pad1, pad2, T) of the definition; ``OvError`` outside the kernel's range, ``ValueError`` for a waveform no longer
    than a pad it must reflect (torch's reflect pad raises then, too)."""
    from ._lib import OvError
    ok = all(isinstance(v, int) for v in (n_fft, hop, win))
    if not (ok and STFT_MIN_N_FFT <= n_fft <= STFT_MAX_N_FFT and n_fft % 2 == 0 and 1 <= hop <= n_fft and 1 <= win <= n_fft):
        raise OvError(f"stft_magnitude: {STFT_MIN_N_FFT} <= n_fft <= {STFT_MAX_N_FFT} and even, 1 <= hop <= n_fft, "
                      f"1 <= win <= n_fft (got n_fft={n_fft}, hop={hop}, win={win})")
    pad1, pad2 = (n_fft - hop) // 2, (n_fft // 2 if center else 0)
    n1 = N + 2 * pad1
    if N <= pad1 or n1 <= pad2 or n1 + 2 * pad2 < n_fft:
        raise ValueError(f"stft_magnitude: {N} samples are no longer than the reflect padding ({pad1}"
                         f"{', then ' + str(pad2) if center else ''}) or shorter than one frame")
    if N > 1 << 30:
        raise ValueError("stft_magnitude: at most 2^30 samples per item")
    return pad1, pad2, (n1 + 2 * pad2 - n_fft) // hop + 1


def stft_window(n_fft, win):
    """float64 numpy ``[n_fft]``: ``torch.hann_window(win)`` (periodic) with ``(n_fft - win) // 2`` zeros to its left, as
    ``torch.stft`` pads a short window."""
    import numpy as np
    w = np.zeros(n_fft, dtype=np.float64)
    left = (n_fft - win) // 2
    w[left:left + win] = 0.5 - 0.5 * np.cos(2.0 * math.pi * np.arange(win, dtype=np.float64) / win)
    return w


def stft_weights(n_fft, win):
    """float64 numpy ``(re, im)``, each ``[n_fft // 2 + 1, n_fft]``: window * cos / -sin(2 pi f n / n_fft), the angle
    reduced exactly (f n mod n_fft in integers)."""
    import numpy as np
    f = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
    n = np.arange(n_fft, dtype=np.int64)[None, :]
    ang = (2.0 * math.pi / n_fft) * ((f * n) % n_fft).astype(np.float64)
    w = stft_window(n_fft, win)[None, :]
    return w * np.cos(ang), -w * np.sin(ang)


def pack_stft_weights(n_fft, win):
    """The fp32 weight table of ``ov_stft_mag_f32`` (include/openvoice_amd.h): record ``(bt * 2 + c) * G + g``, lane l,
    element u = ``W_c[32 bt + (l & 31)][8 g + 2 u + (l >> 5)]``; float32 numpy, flat."""
    import numpy as np
    bins, G = n_fft // 2 + 1, (n_fft + 7) // 8
    tiles = (bins + 31) // 32
    wp = np.zeros((2, tiles * 32, 8 * G), dtype=np.float32)
    re, im = stft_weights(n_fft, win)
    wp[0, :bins, :n_fft], wp[1, :bins, :n_fft] = re, im            # rounded once, float64 -> fp32
    wp = wp.reshape(2, tiles, 32, G, 4, 2)                         # [c][bt][i][g][u][h], k = 8 g + 2 u + h
    return np.ascontiguousarray(wp.transpose(1, 0, 3, 5, 2, 4)).reshape(-1)      # [bt][c][g][h][i][u], l = 32 h + i


def _frames_host(y, n_fft, hop, win, center):
    import numpy as np
    y = np.asarray(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("stft_magnitude: y is [B, N]")
    pad1, pad2, T = _stft_geometry(y.shape[1], n_fft, hop, win, center)
    yp = np.pad(y, ((0, 0), (pad1, pad1)), mode="reflect")
    if pad2:
        yp = np.pad(yp, ((0, 0), (pad2, pad2)), mode="reflect")      # the second reflection reflects the FIRST one's result
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return yp[:, idx]                                               # [B, T, n_fft]


def stft_magnitude_host(y, n_fft, hop_size, win_size, center=False, exact_weights=False):
    """float64 mirror of ``ov_stft_mag_f32``'s definition and its per-element error bound: ``(ref, lim)``, float64 numpy
    ``[B, bins, T]``.  ``ref`` uses the kernel's fp32-rounded weights (``exact_weights=True``: the unrounded float64
    ones, which is ``torch.stft`` in float64 -- that, not the reference's rocFFT bits, is the definition).

    Each of re and im is a length-n_fft fp32 dot product, so whatever the order of summation
    ``e = (n_fft + 4) * 2^-24 * sum_n |w_n x_n|`` bounds its error, and the magnitude (1-Lipschitz in (re, im)) is within
    ``lim = hypot(e_re, e_im) + 2^-22 * ref`` (squares, sum, square root: four roundings)."""
    import numpy as np
    x = _frames_host(y, n_fft, hop_size, win_size, center)
    re, im = stft_weights(n_fft, win_size)
    if not exact_weights:
        re, im = re.astype(np.float32).astype(np.float64), im.astype(np.float32).astype(np.float64)
    ref = np.sqrt((x @ re.T) ** 2 + (x @ im.T) ** 2 + np.float64(np.float32(1e-6)))
    ax = np.abs(x)
    e = (n_fft + 4) * _U24
    lim = np.hypot(e * (ax @ np.abs(re).T), e * (ax @ np.abs(im).T)) + 4 * _U24 * ref
    return ref.transpose(0, 2, 1), lim.transpose(0, 2, 1)


def mel_log_host(spec, mel, clip=1e-5, spec_lim=None):
    """float64 mirror of ``ov_mel_log_f32`` and its per-element error bound: ``(ref, lim)`` for ``spec [B, bins, T]`` and
    ``mel [num_mels, bins]`` (both are taken at the values given; the device holds them in fp32).  The products are
    non-negative, so the fp32 sum v is within ``dv = (bins + 4) * 2^-24 * v`` (plus ``mel @ spec_lim`` when the spectrogram
    itself is only known to ``spec_lim``), and ``lim = dv / max(v - dv, clip) + 4 * 2^-24 * max(1, |ref|)``."""
    import numpy as np
    to_np = lambda a: np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    spec, mel = to_np(spec), to_np(mel)
    clip = float(np.float32(clip))
    v = mel @ spec
    dv = (spec.shape[-2] + 4) * _U24 * v
    if spec_lim is not None:
        dv = dv + mel @ to_np(spec_lim)
    ref = np.log(np.maximum(v, clip))
    return ref, dv / np.maximum(v - dv, clip) + 4 * _U24 * np.maximum(1.0, np.abs(ref))


def stft_magnitude(y, n_fft, hop_size, win_size, center=False):
    """``sqrt(re^2 + im^2 + 1e-6)`` of the STFT of ``y [B, N]``, ``[B, n_fft // 2 + 1, T]``: the reference's
    ``spectrogram_torch`` (openvoice/mel_processing.py:40-75) without its range check, at ANY shape the kernel supports --
    16 <= n_fft <= 2048 and even, 1 <= hop <= n_fft, 1 <= win <= n_fft, centred or not, float32.  A device tensor runs
    ``ov_stft_mag_f32`` (one launch; weights cached per (device, n_fft, hop, win)) or raises ``OvError`` / ``ValueError``;
    a CPU tensor is evaluated with ``torch.stft``.  The storage behind the result has rows of ``padded_frames(T)`` floats
    whose padded columns are zero, like ``spectrogram_torch``'s."""
    if not y.is_cuda:
        return _stft_torch(y, n_fft, hop_size, win_size, center)
    from . import _lib
    from .launch import padded_frames
    if y.dtype != torch.float32:
        raise _lib.OvError(f"stft_magnitude: float32 only on the device, got {y.dtype}")
    if y.dim() != 2 or y.shape[0] < 1:
        raise ValueError("stft_magnitude: y is [B, N]")
    B, N = y.shape
    _, _, T = _stft_geometry(N, n_fft, hop_size, win_size, center)
    key = (str(y.device), n_fft, hop_size, win_size)
    wpack = _stft_packs.get(key)
    if wpack is None:
        wpack = _stft_packs[key] = torch.from_numpy(pack_stft_weights(n_fft, win_size)).to(y.device)
    ld = padded_frames(T)
    out = torch.empty(B, n_fft // 2 + 1, ld, dtype=torch.float32, device=y.device)
    _lib.call("ov_stft_mag_f32", y.contiguous(), wpack, out, B, N, n_fft, hop_size, win_size, int(bool(center)), ld)
    return out[:, :, :T]


def _mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax, like):
    key = (sampling_rate, n_fft, num_mels, fmin, fmax, str(like.device), like.dtype)
    basis = _mel_bases.get(key)
    if basis is None:
        basis = torch.from_numpy(mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax))
        basis = _mel_bases[key] = basis.to(dtype=like.dtype, device=like.device).contiguous()
    return basis


def spec_to_mel_torch(spec, n_fft, num_mels, sampling_rate, fmin, fmax):
    """``log(clamp(mel_basis @ spec, min=1e-5))`` (reference: openvoice/mel_processing.py:122-133).  A device spectrogram
    (float32, ``[B, bins, T]`` or ``[bins, T]``, any row stride) runs ``ov_mel_log_f32``; a CPU one ``torch.matmul``.

    Difference from the reference, on purpose: the filterbank is cached per (sampling_rate, n_fft, num_mels, fmin, fmax,
    device, dtype).  The reference caches on ``fmax`` alone and hands back a stale basis when any other argument changes."""
    if not spec.is_cuda:
        return spectral_normalize_torch(torch.matmul(_mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax, spec), spec))
    from . import _lib
    from .launch import padded_frames
    if spec.dtype != torch.float32:
        raise _lib.OvError(f"spec_to_mel_torch: float32 only on the device, got {spec.dtype}")
    bins = n_fft // 2 + 1
    if not (1 <= num_mels <= MEL_MAX_MELS and bins <= MEL_MAX_BINS):
        raise _lib.OvError(f"spec_to_mel_torch: num_mels <= {MEL_MAX_MELS} and n_fft // 2 + 1 <= {MEL_MAX_BINS} on the "
                           f"device (got {num_mels}, {bins})")
    squeeze = spec.dim() == 2
    s = spec.unsqueeze(0) if squeeze else spec
    if s.dim() != 3 or s.shape[1] != bins or s.shape[2] < 1 or s.shape[0] < 1:
        raise ValueError(f"spec_to_mel_torch: spec is [B, {bins}, T] for n_fft={n_fft}, got {tuple(spec.shape)}")
    B, _, T = s.shape
    if s.stride(2) != 1 or s.stride(1) < T or (B > 1 and s.stride(0) < (bins - 1) * s.stride(1) + T):
        s = s.contiguous()
    basis = _mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax, s)
    ld = padded_frames(T)
    out = torch.empty(B, num_mels, ld, dtype=torch.float32, device=s.device)
    _lib.call("ov_mel_log_f32", s, basis, out, B, num_mels, bins, T, s.stride(1), s.stride(0), ld, 1e-5)
    out = out[:, :, :T]
    return out[0] if squeeze else out


def mel_spectrogram_torch(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """Log-mel spectrogram of ``y [B, N]`` (reference: openvoice/mel_processing.py:136-183), ``[B, num_mels, T]``.  On a
    device tensor: ``ov_stft_mag_f32`` then ``ov_mel_log_f32`` at any supported shape, two launches, nothing else; on a
    CPU tensor ``torch.stft`` and ``torch.matmul``.  The reference's range check (two device->host syncs) runs only under
    ``OV_CHECK_RANGE=1``; the filterbank cache is keyed as in ``spec_to_mel_torch``."""
    _check_range(y, 1.0)
    if y.is_cuda and not 1 <= num_mels <= MEL_MAX_MELS:
        from ._lib import OvError
        raise OvError(f"mel_spectrogram_torch: num_mels <= {MEL_MAX_MELS} on the device (got {num_mels})")
    return spec_to_mel_torch(stft_magnitude(y, n_fft, hop_size, win_size, center), n_fft, num_mels, sampling_rate, fmin, fmax)
