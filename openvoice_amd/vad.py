"""Silence removal on the device: what ``se_extractor.get_se(..., vad=True)`` does before it cuts a recording.

The reference (openvoice/se_extractor.py:77-97) asks a third-party voice-activity network (silero through
``whisper_timestamped.get_vad_segments(min_speech_duration=0.1, min_silence_duration=1)``) for speech segments and
concatenates them.  The network and its weights are out of scope; the PROCEDURE -- segments,
concatenated active audio, then equal pieces -- is kept, with a deterministic energy detector of the kind that function
offers as its non-neural method.  Parity with silero's decisions is not claimed and cannot be pinned offline.

The detector, at the model's sampling rate ``sr`` with ``H = hop`` and frames of ``W = 2 H`` samples:

1. ``T = ceil(N / H)`` frames; ``e[t]`` = mean of ``x[n]^2`` over the existing samples of ``[t H, min(N, t H + W))``.
2. ``thr = max(10^(floor_db / 10), max_t e[t] * 10^(-range_db / 10))``; frame t is raw-active iff ``e[t] > thr``.
3. A silent run between two raw-active frames shorter than ``ceil(min_silence_s * sr / H)`` frames becomes active.
4. Then an active run shorter than ``ceil(min_speech_s * sr / H)`` frames becomes silent.
5. Every remaining run grows by ``ceil(pad_s * sr / H)`` frames on each side, clipped to ``[0, T)``.
6. Sample n is kept iff frame ``n // H`` is kept.

Three launches (csrc/vad.hip: ``ov_vad_frame_energy_f32``, ``ov_vad_segments_i32``, ``ov_vad_compact_f32``) serve any
number of recordings packed into one pool, followed by ONE device-to-host copy (the counts and the kept-frame masks).
A recording whose frames are all raw-active comes back bit for bit; one whose peak energy is below the floor comes back
empty.  ``speech_frames_host`` restates steps 1-5 in float64 numpy for host tooling and the CPU tests.
"""
import math

import numpy as np

from . import _lib


class VadParams:
    """The five knobs of the detector (defaults: the issue's, with the reference's two durations)."""

    def __init__(self, range_db=35.0, floor_db=-55.0, min_silence_s=1.0, min_speech_s=0.1, pad_s=0.03):
        for name, v in (("range_db", range_db), ("floor_db", floor_db), ("min_silence_s", min_silence_s),
                        ("min_speech_s", min_speech_s), ("pad_s", pad_s)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"VadParams.{name} must be a finite number, got {v!r}")
        if range_db <= 0:
            raise ValueError(f"VadParams.range_db must be > 0 (dB below the peak frame), got {range_db}")
        if floor_db > 0:
            raise ValueError(f"VadParams.floor_db must be <= 0 (dB re full scale), got {floor_db}")
        if min_silence_s <= 0 or min_speech_s <= 0:
            raise ValueError("VadParams.min_silence_s and min_speech_s must be > 0")
        if pad_s < 0:
            raise ValueError(f"VadParams.pad_s must be >= 0, got {pad_s}")
        self.range_db, self.floor_db = float(range_db), float(floor_db)
        self.min_silence_s, self.min_speech_s, self.pad_s = float(min_silence_s), float(min_speech_s), float(pad_s)

    def frames(self, sr, hop):
        """``(min_silence_frames, min_speech_frames, pad_frames)`` at ``sr`` and ``hop``."""
        _check_rate(sr, hop)
        return (math.ceil(self.min_silence_s * sr / hop), math.ceil(self.min_speech_s * sr / hop),
                math.ceil(self.pad_s * sr / hop))

    def linear(self):
        """``(10^(floor_db / 10), 10^(-range_db / 10))``: the threshold's two factors in the linear domain."""
        return 10.0 ** (self.floor_db / 10.0), 10.0 ** (-self.range_db / 10.0)

    def __repr__(self):
        return (f"VadParams(range_db={self.range_db}, floor_db={self.floor_db}, min_silence_s={self.min_silence_s}, "
                f"min_speech_s={self.min_speech_s}, pad_s={self.pad_s})")


def _check_rate(sr, hop):
    if int(sr) != sr or sr <= 0:
        raise ValueError(f"sr must be a positive integer, got {sr!r}")
    if int(hop) != hop or hop <= 0 or hop % 4 != 0:
        raise ValueError(f"hop must be a positive multiple of 4, got {hop!r}")


def speech_frames_host(x, sr, hop, params=None):
    """Steps 1-5 in float64 numpy: the kept-frame mask (bool ``[ceil(N / hop)]``) of the 1-D waveform ``x``."""
    p = params or VadParams()
    min_sil, min_speech, pad = p.frames(sr, hop)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    N, H = x.shape[0], int(hop)
    T = -(-N // H)
    if T == 0:
        return np.zeros(0, dtype=bool)
    hops = np.concatenate([np.concatenate([x * x, np.zeros(T * H - N)]).reshape(T, H).sum(1), [0.0]])
    start = np.arange(T) * H
    e = (hops[:T] + hops[1:]) / (np.minimum(N, start + 2 * H) - start)       # a frame is two hops
    floor_lin, range_lin = p.linear()
    raw = e > max(floor_lin, e.max() * range_lin)
    t = np.arange(T)

    def last(flag):          # last u <= t with flag[u], -1 where none
        return np.maximum.accumulate(np.where(flag, t, -1))

    def first(flag):         # first u >= t with flag[u], T where none
        return np.minimum.accumulate(np.where(flag, t, T)[::-1])[::-1]

    L, F = last(raw), first(raw)
    closed = raw | ((L >= 0) & (F < T) & (F - L - 1 < min_sil))
    speech = closed & (first(~closed) - last(~closed) - 1 >= min_speech)
    L, F = last(speech), first(speech)
    return ((L >= 0) & (t - L <= pad)) | ((F < T) & (F - t <= pad))


def segments_of(mask, hop, n_samples):
    """The kept ``(start_sample, end_sample)`` spans of a kept-frame mask, in order."""
    m = np.concatenate([[False], np.asarray(mask, dtype=bool), [False]])
    edges = np.flatnonzero(m[1:] != m[:-1])
    return [(int(a) * int(hop), min(int(n_samples), int(b) * int(hop))) for a, b in zip(edges[::2], edges[1::2])]


def remove_silence_host(x, sr, hop, params=None):
    """``remove_silence`` on the host (float64 decisions, numpy indexing): ``(kept samples of x, segments)``."""
    x = np.asarray(x).reshape(-1)
    mask = speech_frames_host(x, sr, hop, params)
    return x[np.repeat(mask, int(hop))[:x.shape[0]]], segments_of(mask, hop, x.shape[0])


def remove_silence_many(waves, sr, hop, params=None):
    """Silence removal of many recordings in three launches and one device-to-host copy.

    ``waves``: list of 1-D float32 tensors on one ROCm device, at ``sr``.  Returns ``(kept, segments)``: per recording
    the kept samples in order (a device tensor, possibly of length 0) and its ``(start_sample, end_sample)`` spans."""
    import torch
    p = params or VadParams()
    min_sil, min_speech, pad = p.frames(sr, hop)
    floor_lin, range_lin = p.linear()
    H = int(hop)
    waves = [w.detach().to(torch.float32).reshape(-1) for w in waves]
    R = len(waves)
    if R == 0:
        return [], []
    if R > 65535:
        raise ValueError("remove_silence_many: at most 65535 recordings per call")
    dev = waves[0].device
    lens = [int(w.numel()) for w in waves]
    bases, total = [], 0
    for n in lens:                      # every recording starts 16-byte aligned in both pools
        bases.append(total)
        total += -(-n // 4) * 4
    ldT = max(1, max(-(-n // H) for n in lens))
    if total == 0:
        return [w[:0] for w in waves], [[] for _ in waves]
    if R == 1:
        pool = waves[0].contiguous()
    else:
        pool = torch.zeros(total, dtype=torch.float32, device=dev)
        for w, b, n in zip(waves, bases, lens):
            pool[b:b + n] = w
    table = torch.tensor([v for bn in zip(bases, lens) for v in bn] + bases, dtype=torch.int64).to(dev)
    records, out_bases = table[:2 * R].view(R, 2), table[2 * R:]       # the output pool is laid out like the input pool
    energy = torch.empty(R, ldT, dtype=torch.float32, device=dev)
    mask = torch.empty(R, ldT, dtype=torch.int32, device=dev)
    offsets = torch.empty(R, ldT, dtype=torch.int64, device=dev)
    n_active = torch.empty(R, dtype=torch.int64, device=dev)
    out = torch.empty(total, dtype=torch.float32, device=dev)
    _lib.call("ov_vad_frame_energy_f32", pool, pool.numel(), records, R, H, ldT, energy)
    _lib.call("ov_vad_segments_i32", energy, records, R, H, ldT, floor_lin, range_lin, min_sil, min_speech, pad, mask,
              offsets, n_active)
    _lib.call("ov_vad_compact_f32", pool, pool.numel(), records, R, H, ldT, mask, offsets, out_bases, out,
              out.numel())
    host = torch.cat([n_active, mask.reshape(-1).to(torch.int64)]).cpu().numpy()    # the one copy (and sync)
    counts, masks = host[:R], host[R:].reshape(R, ldT)
    kept, segments = [], []
    for r in range(R):
        kept.append(out[bases[r]:bases[r] + int(counts[r])])
        segments.append(segments_of(masks[r, :-(-lens[r] // H)], H, lens[r]))
    return kept, segments


def remove_silence(wave, sr, hop, params=None):
    """``remove_silence_many`` of one recording: ``(kept samples, [(start_sample, end_sample), ...])``."""
    kept, segments = remove_silence_many([wave], sr, hop, params)
    return kept[0], segments[0]
