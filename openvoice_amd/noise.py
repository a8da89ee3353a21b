"""Counter-based Gaussian noise: ``seed=`` for conversions, streams and TTS.

Every conversion draws Gaussian noise (the posterior sample, reference openvoice/models.py:220) and every TTS call
draws two (``noise_w`` / ``noise_z``, models.py:476, :486).  torch's generator is sequential: what a stream draws
depends on its push sizes and on the streams it shares a pool with.  Here the value at ``(seed, stream, purpose, channel c,
frame t)`` is a pure function of those five numbers, generated where and when it is needed by one record-driven launch
(``ov_normal_philox_f32``, csrc/noise.hip), so with ``seed=s`` a live stream pushed in any chunking, alone or in a
pool, a windowed stream, ``convert_long``, ``convert_many`` and a one-pass ``convert`` are the same function of the
input audio, and no noise tensor is kept anywhere.

The definition (``0 <= seed < 2^63``, ``0 <= stream, purpose, c < 2^32``, ``0 <= t < 2^34``)::

    (r0, r1, r2, r3) = Philox4x32-10(counter = (t // 4, c, stream, purpose), key = (seed & 0xffffffff, seed >> 32))
    j = t % 4;  (ra, rb) = (r0, r1) if j < 2 else (r2, r3)
    u1 = ((ra >> 8) + 0.5) * 2^-24;  u2 = (rb >> 8) * 2^-24
    n = sqrt(-2 ln u1) * (cos if j is even else sin)(2 pi u2)                    |n| <= sqrt(50 ln 2) = 5.887

Purposes: 0 the converter's posterior noise (192 channels, frames of the spectrogram), 1 the TTS ``noise_w`` (2
channels, frames are token positions), 2 the TTS ``noise_z`` (192 channels, frames of the output).

``normal`` / ``fill`` run the kernel; ``normal_host`` restates the definition, Philox core included, in float64 numpy
(the pattern of ``clone.join_segments_host``): it is what tools and the CPU tests use.  There is no CPU fallback.
"""
import numpy as np

from . import _lib

PURPOSE_POSTERIOR, PURPOSE_TTS_W, PURPOSE_TTS_Z = 0, 1, 2
PURPOSE_WATERMARK = 3       # not a Gaussian draw: single bits of the same Philox core are watermark.py's chips
RECORD_FIELDS = 7           # ov_normal_philox_f32's record: (seed, stream, purpose, f0, nf, dst_off, dst_ld)
MAX_RECORDS = 65535
SEED_LIMIT = 1 << 63
WORD_LIMIT = 1 << 32        # stream, purpose, channel
FRAME_LIMIT = 1 << 34

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_seed(seed, index=0):
    """``seed`` -> ``(seed, stream)``: a non-bool int ``s`` gives ``(s, index)``, a pair ``(s, stream)`` itself.
    ``0 <= s < 2^63`` and ``0 <= stream < 2^32``, ValueError otherwise."""
    if _is_int(seed):
        s, k = int(seed), index
    elif isinstance(seed, (tuple, list)) and len(seed) == 2 and _is_int(seed[0]) and _is_int(seed[1]):
        s, k = int(seed[0]), seed[1]
    else:
        raise ValueError(f"seed: an int, or a pair (seed, stream) of ints, got {seed!r}")
    if not _is_int(k):
        raise ValueError(f"seed: stream must be an int, got {k!r}")
    k = int(k)
    if not 0 <= s < SEED_LIMIT:
        raise ValueError(f"seed {s} outside [0, 2^63)")
    if not 0 <= k < WORD_LIMIT:
        raise ValueError(f"stream {k} outside [0, 2^32)")
    return s, k


def per_item(seed, n):
    """The ``(seed, stream)`` of each of ``n`` items (batch rows, recordings, sentences): an int ``s`` gives item ``i``
    the pair ``(s, i)``, a pair ``(s, k)`` gives it ``(s, k + i)``, a list holds one seed or pair per item (an int
    there means stream 0).  ValueError for a list of another length."""
    if isinstance(seed, list):
        if len(seed) != n:
            raise ValueError(f"seed: one per item ({n}), got a list of {len(seed)}")
        return [check_seed(s) for s in seed]
    s, k = check_seed(seed)
    return [check_seed((s, k + i)) for i in range(n)]


def rows(seed, n):
    """What the engines take for a launch of ``n`` rows: ``(seed, stream, f0)`` per row, ``f0`` the frame of the row's
    first column.  ``seed`` as for ``per_item``, or a list whose items may also be such triples (the windows of a
    recording, each at its own first frame)."""
    if isinstance(seed, list) and len(seed) == n and any(isinstance(s, (tuple, list)) and len(s) == 3 for s in seed):
        out = []
        for s in seed:
            if isinstance(s, (tuple, list)) and len(s) == 3:
                f0 = s[2]
                if not _is_int(f0) or not 0 <= int(f0) < FRAME_LIMIT:
                    raise ValueError(f"seed: first frame {f0!r} outside [0, 2^34)")
                out.append(check_seed((s[0], s[1])) + (int(f0),))
            else:
                out.append(check_seed(s) + (0,))
        return out
    return [p + (0,) for p in per_item(seed, n)]


def exclusive(seed, **noises):
    """``seed=`` and an explicit noise tensor are two answers to one question: ValueError when both are given."""
    if seed is not None:
        for name, value in noises.items():
            if value is not None:
                raise ValueError(f"seed= and {name}= are mutually exclusive: pass one of them")


def kw(seed, name="seed"):
    """``{name: seed}``, or nothing for None: callers forward ``seed`` only when it was given, so that an unseeded call
    is, argument for argument, the call it was before ``seed=`` existed."""
    return {} if seed is None else {name: seed}


# ---- the definition in float64 numpy --------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """The standard Philox4x32-10: ``counter`` four and ``key`` two arrays (or ints) of 32-bit words, broadcast against
    each other -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for k in key)
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0          # < 2^64: both factors are below 2^32
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(PHILOX_W0)) & mask
        k1 = (k1 + np.uint64(PHILOX_W1)) & mask
    return tuple(np.asarray(c, dtype=np.uint64).astype(np.uint32) for c in (c0, c1, c2, c3))


def normal_host(seed, channels, f0, frames, purpose=0, c0=0):
    """The definition restated in float64 numpy: ``[channels, frames]`` float64, the values of channels
    ``[c0, c0 + channels)`` and frames ``[f0, f0 + frames)`` (``seed``: an int, stream 0, or a pair)."""
    s, stream = check_seed(seed)
    channels, f0, frames, purpose, c0 = int(channels), int(f0), int(frames), int(purpose), int(c0)
    if channels < 0 or c0 < 0 or c0 + channels > WORD_LIMIT or not 0 <= purpose < WORD_LIMIT:
        raise ValueError("channels / purpose outside [0, 2^32)")
    if f0 < 0 or frames < 0 or f0 + frames > FRAME_LIMIT:
        raise ValueError("frames outside [0, 2^34)")
    t = np.arange(f0, f0 + frames, dtype=np.uint64)[None, :]
    c = np.arange(c0, c0 + channels, dtype=np.uint64)[:, None]
    r = philox4x32_10((t // np.uint64(4), c, stream, purpose), (s & 0xFFFFFFFF, s >> 32))
    r = [np.broadcast_to(w, (channels, frames)) for w in r]
    j = np.broadcast_to(t % np.uint64(4), (channels, frames))
    ra = np.where(j < 2, r[0], r[2])
    rb = np.where(j < 2, r[1], r[3])
    u1 = ((ra >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = (rb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    radius = np.sqrt(-2.0 * np.log(u1))
    return radius * np.where(j % np.uint64(2) == 0, np.cos(2.0 * np.pi * u2), np.sin(2.0 * np.pi * u2))


# ---- the device side ------------------------------------------------------------------------------------------------
def fill(records, C, dst):
    """The many-slab form: ``records`` host rows ``(seed, stream, purpose, f0, nf, dst_off, dst_ld)``; writes
    ``dst[dst_off + c * dst_ld + i] = n(seed, stream, purpose, c, f0 + i)`` for ``c < C``, ``i < nf`` and nothing
    else.  ``dst``: a float32 device tensor, dense from its first element (offsets are relative to it; a view into a
    larger tensor is fine as long as the slabs stay inside ``dst``'s own extent).  Validated here, uploaded in one
    copy, ONE launch (per 65535 records)."""
    import torch
    C = int(C)
    if not isinstance(dst, torch.Tensor) or dst.dtype != torch.float32 or not dst.is_cuda or not dst.is_contiguous():
        raise ValueError("dst must be a contiguous float32 tensor on a ROCm device")
    if not 0 < C <= WORD_LIMIT // 2:
        raise ValueError(f"C = {C}")
    elems = dst.numel()
    table = []
    for rec in records:
        if len(rec) != RECORD_FIELDS or not all(_is_int(v) for v in rec):
            raise ValueError(f"record {rec!r}: (seed, stream, purpose, f0, nf, dst_off, dst_ld) as ints")
        s, k, purpose, f0, nf, off, ld = (int(v) for v in rec)
        check_seed((s, k))
        if not 0 <= purpose < WORD_LIMIT:
            raise ValueError(f"purpose {purpose} outside [0, 2^32)")
        if f0 < 0 or nf < 0 or f0 + nf > FRAME_LIMIT:
            raise ValueError(f"frames [{f0}, {f0 + nf}) outside [0, 2^34)")
        if nf == 0:
            continue
        if ld < nf or off < 0 or off + (C - 1) * ld + nf > elems:
            raise ValueError(f"record {rec!r}: the slab ({C} rows of {nf}, ld {ld}, at {off}) leaves dst ({elems} elements) "
                             f"or its rows overlap")
        table.append((s, k, purpose, f0, nf, off, ld))
    for i in range(0, len(table), MAX_RECORDS):
        part = table[i:i + MAX_RECORDS]
        recs = torch.tensor(part, dtype=torch.int64).to(dst.device)                 # one host -> device copy
        _lib.call("ov_normal_philox_f32", recs, len(part), C, dst, elems, max(r[4] for r in part))


def normal(seed, channels, f0, frames, device, purpose=0):
    """``[channels, frames]`` float32 on ``device``: the noise of ``seed`` (an int, stream 0, or a pair ``(seed,
    stream)``) for channels ``[0, channels)`` and frames ``[f0, f0 + frames)``.  One launch."""
    import torch
    s, k = check_seed(seed)
    out = torch.empty(int(channels), int(frames), dtype=torch.float32, device=device)
    fill([(s, k, int(purpose), int(f0), int(frames), 0, int(frames))], channels, out)
    return out
