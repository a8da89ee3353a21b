"""The project's own keyed watermark: marks and reads converted audio on the device, without wavmark.

``ToneColorConverter``'s provenance hook (``add_watermark`` / ``detect_watermark``, reference openvoice/api.py:162-201)
calls a model with wavmark's interface, ``encode(carrier [B, L], bits [B, 32]) -> [B, L]`` and ``decode(carrier [B, L])
-> scores [B, 32]``.  ``NativeWatermark`` is such a model.  It is NOT wavmark-compatible and does not claim to be:
neither reads the other's marks.  It is informed spread spectrum in the time domain, pinned down so that reading back an
unattacked mark is exact by construction.

The definition, for one window ``x[0 .. L)`` (``L >= 512``) carrying 32 bits, ``0 <= key < 2^63``::

    (r0, r1, r2, r3) = Philox4x32-10(counter = (i // 128, 0, 0, 3), key = (key & 0xffffffff, key >> 32))
    c[i] = +1 if bit (i % 32) of r[(i % 128) // 32] is set else -1                         the chips: key and i only
    S_j  = {i : i % 32 == j}                                                                bit j owns every 32nd sample
    p_j  = (1 / |S_j|) sum_{i in S_j} c[i] x[i]                                             the projection
    a    = max(strength * sqrt(mean x^2), floor)                                            the level
    embed:  d_j = b_j * max(a - b_j p_j, 0),  b_j = +1 / -1 for bit 1 / 0;   y[i] = x[i] + d_{i % 32} c[i]
    read:   q_j = p_j(y),  score_j = 0.5 + 0.5 tanh(q_j / a_y),  a_y the level of y;  bit j = score_j >= 0.5

The chips are single bits of the Philox core ``noise.py`` defines (purpose 3, next to its three Gaussian purposes); they
do not depend on which window is marked, because ``encode`` sees only the carrier.  ``d`` is the smallest change along
the chips that brings ``b_j p_j(y)`` up to ``a`` (``p_j(y) = p_j(x) + d_j`` exactly, since ``c^2 = 1``), so a bit the
host audio already carries strongly enough is left alone and an unattacked read gives ``b_j q_j >= a``.  ``strength =
0.02`` and ``floor = 2^-12`` are design parameters: the floor keeps a silent window's mark above int16 rounding (which
moves a projection by at most half an LSB, 1.6e-5).

Out of scope: deciding whether audio is marked at all (like upstream's ``detect_watermark``, reading unmarked audio
returns arbitrary characters), and robustness to resampling, MP3 coding or a time shift.

``encode`` / ``decode`` / ``mark_many`` run the kernels (csrc/watermark.hip: ``ov_wm_embed_windows_f32``,
``ov_wm_detect_windows_f32``, record-driven, one workgroup per window, ONE launch for all windows); ``encode_host`` /
``decode_host`` restate the definition in float64 numpy (the pattern of ``noise.normal_host``): it is what tools and the
CPU tests use.  There is no CPU fallback.
"""
import numpy as np

from . import _lib
from .noise import philox4x32_10, PURPOSE_WATERMARK, SEED_LIMIT

BITS = 32                   # payload bits of a window
MIN_WINDOW = BITS * 16      # every bit owns at least 16 samples
MAX_WINDOW = 1 << 31
RECORD_FIELDS = 4           # (src_off, dst_off, L, bits)
MAX_RECORDS = 65535
DEFAULT_STRENGTH = 0.02
DEFAULT_FLOOR = 2.0 ** -12
# the carrier windows of the converter's hook (ToneColorConverter.WATERMARK_*): group n in the 16 000 samples from 32 000 n
WINDOW = 16000
STRIDE = 2 * WINDOW


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_params(key, strength, floor):
    """``(key, strength, floor)`` as Python numbers; ValueError outside ``0 <= key < 2^63``, ``0 <= strength <= 1``,
    ``0 < floor <= 1``."""
    if not _is_int(key) or not 0 <= int(key) < SEED_LIMIT:
        raise ValueError(f"key: an int in [0, 2^63), got {key!r}")
    strength, floor = float(strength), float(floor)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"strength {strength} outside [0, 1]")
    if not 0.0 < floor <= 1.0:
        raise ValueError(f"floor {floor} outside (0, 1]")
    return int(key), strength, floor


def pack_bits(bits):
    """32 values (>= 0.5 reads as 1) -> the record's payload word: bit j of the result is ``bits[j]``."""
    b = np.asarray(bits).reshape(-1)
    if b.size != BITS:
        raise ValueError(f"a window carries {BITS} bits, got {b.size}")
    return int(sum(1 << j for j in range(BITS) if b[j] >= 0.5))


# ---- the definition in float64 numpy --------------------------------------------------------------------------------
def chips_host(key, L):
    """``c[0 .. L)`` as float64 +-1."""
    key, L = int(key), int(L)
    blocks = np.arange((L + 127) // 128, dtype=np.uint64)
    r = philox4x32_10((blocks, 0, 0, PURPOSE_WATERMARK), (key & 0xFFFFFFFF, key >> 32))
    words = np.stack([np.broadcast_to(w, blocks.shape) for w in r], axis=1)                 # [blocks, 4]
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return 2.0 * bits.reshape(-1)[:L].astype(np.float64) - 1.0


def _check_window(L):
    if not MIN_WINDOW <= int(L) <= MAX_WINDOW:
        raise ValueError(f"a window of {int(L)} samples: the watermark needs {MIN_WINDOW} <= L <= 2^31")


def read_host(carrier, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
    """``(q [B, 32], a [B])`` of ``carrier [B, L]`` (or ``[L]``: ``B = 1``) in float64: projections and level."""
    key, strength, floor = check_params(key, strength, floor)
    x = np.atleast_2d(np.asarray(carrier, dtype=np.float64))
    _check_window(x.shape[1])
    cx = x * chips_host(key, x.shape[1])[None, :]
    q = np.stack([cx[:, j::BITS].mean(axis=1) for j in range(BITS)], axis=1)
    a = np.maximum(strength * np.sqrt(np.mean(x * x, axis=1)), floor)
    return q, a


def encode_host(carrier, bits, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
    """The marked ``carrier [B, L]`` (or ``[L]``) in float64; ``bits [B, 32]`` (>= 0.5 reads as 1)."""
    x = np.asarray(carrier, dtype=np.float64)
    x2 = np.atleast_2d(x)
    p, a = read_host(x2, key, strength, floor)
    b = np.where(np.asarray(bits, dtype=np.float64).reshape(x2.shape[0], BITS) >= 0.5, 1.0, -1.0)
    d = b * np.maximum(a[:, None] - b * p, 0.0)                                             # [B, 32]
    L = x2.shape[1]
    y = x2 + d[:, np.arange(L) % BITS] * chips_host(key, L)[None, :]
    return y.reshape(x.shape)


def decode_host(carrier, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
    """Scores ``[B, 32]`` in float64: ``0.5 + 0.5 tanh(q / a)``."""
    q, a = read_host(carrier, key, strength, floor)
    return 0.5 + 0.5 * np.tanh(q / a[:, None])


# ---- the device side ------------------------------------------------------------------------------------------------
def _check_buffer(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor on a ROCm device")


def check_records(records, src_elems, dst_elems=None):
    """Host rows ``(src_off, dst_off, L, bits)`` checked as the kernel checks them (``dst_elems`` None: the reader, which
    ignores ``dst_off``): ValueError for a window shorter than 512 samples or one that leaves its buffer."""
    table = []
    for rec in records:
        if len(rec) != RECORD_FIELDS or not all(_is_int(v) for v in rec):
            raise ValueError(f"record {rec!r}: (src_off, dst_off, L, bits) as ints")
        so, do, L, bits = (int(v) for v in rec)
        _check_window(L)
        if not 0 <= bits < 1 << BITS:
            raise ValueError(f"record {rec!r}: the payload is 32 bits")
        if so < 0 or so + L > src_elems or (dst_elems is not None and (do < 0 or do + L > dst_elems)):
            raise ValueError(f"record {rec!r}: the window leaves its buffer ({src_elems} / {dst_elems} elements)")
        table.append((so, do, L, bits))
    return table


def embed_windows(src, dst, records, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
    """Mark the windows ``records`` names (host rows ``(src_off, dst_off, L, bits)``, offsets in elements of ``src`` /
    ``dst``, which may be one tensor: in place) and nothing else.  Validated here, uploaded in one copy, ONE launch (per
    65535 windows).  The windows of a call must not overlap each other."""
    import torch
    key, strength, floor = check_params(key, strength, floor)
    _check_buffer(src, "src")
    _check_buffer(dst, "dst")
    table = check_records(records, src.numel(), dst.numel())
    for i in range(0, len(table), MAX_RECORDS):
        part = table[i:i + MAX_RECORDS]
        recs = torch.tensor(part, dtype=torch.int64).to(src.device)
        _lib.call("ov_wm_embed_windows_f32", src, src.numel(), dst, dst.numel(), recs, len(part), key, strength, floor)


def detect_windows(src, records, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
    """``(q [W, 32], level [W])`` float32 on the device for the windows ``records`` names (``dst_off`` and ``bits`` are
    ignored).  ONE launch (per 65535 windows)."""
    import torch
    key, strength, floor = check_params(key, strength, floor)
    _check_buffer(src, "src")
    table = check_records(records, src.numel())
    q = torch.empty(len(table), BITS, dtype=torch.float32, device=src.device)
    level = torch.empty(len(table), dtype=torch.float32, device=src.device)
    for i in range(0, len(table), MAX_RECORDS):
        part = table[i:i + MAX_RECORDS]
        recs = torch.tensor(part, dtype=torch.int64).to(src.device)
        _lib.call("ov_wm_detect_windows_f32", src, src.numel(), recs, len(part), key, strength, floor, q[i:i + len(part)],
                  level[i:i + len(part)])
    return q, level


class NativeWatermark:
    """A watermark model for ``ToneColorConverter``'s hook (``watermark="native"`` installs one): wavmark's interface on
    device tensors, the scheme of the module docstring.  ``launches`` counts kernel launches."""

    def __init__(self, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
        self.key, self.strength, self.floor = check_params(key, strength, floor)
        self.device = None
        self.launches = 0
        self._pow2 = None

    def to(self, device):
        import torch
        self.device = torch.device(device)
        self._pow2 = None
        return self

    def _params(self):
        return self.key, self.strength, self.floor

    def _rows(self, carrier, what):
        import torch
        if not isinstance(carrier, torch.Tensor) or carrier.dtype != torch.float32 or not carrier.is_cuda or carrier.dim() != 2:
            raise ValueError(f"{what}: carrier must be a float32 [B, L] tensor on a ROCm device (there is no CPU path; "
                             f"encode_host / decode_host are the float64 mirror)")
        B, L = carrier.shape
        if B < 1:
            raise ValueError(f"{what}: no windows")
        _check_window(L)
        return carrier.contiguous(), B, L

    def encode(self, carrier, bits):
        """``carrier [B, L]`` float32 on the device, ``bits [B, 32]`` (>= 0.5 reads as 1; host or device) -> the marked
        ``[B, L]``; one launch for all ``B``, and no copy to the host."""
        import torch
        x, B, L = self._rows(carrier, "encode")
        dev = x.device
        bits = torch.as_tensor(bits).reshape(B, BITS)
        if self._pow2 is None or self._pow2.device != dev:
            self._pow2 = torch.tensor([1 << j for j in range(BITS)], dtype=torch.int64).to(dev)
        recs = torch.tensor([(i * L, i * L, L, 0) for i in range(B)], dtype=torch.int64).to(dev)
        recs[:, 3] = ((bits.to(dev) >= 0.5).to(torch.int64) * self._pow2).sum(dim=1)
        y = torch.empty_like(x)
        for i in range(0, B, MAX_RECORDS):
            n = min(MAX_RECORDS, B - i)
            _lib.call("ov_wm_embed_windows_f32", x, x.numel(), y, y.numel(), recs[i:i + n], n, *self._params())
            self.launches += 1
        return y

    def read(self, carrier):
        """``(q [B, 32], level [B])`` of ``carrier [B, L]``: projections and level, float32 on the device."""
        x, B, L = self._rows(carrier, "decode")
        q, level = detect_windows(x, [(i * L, 0, L, 0) for i in range(B)], *self._params())
        self.launches += (B + MAX_RECORDS - 1) // MAX_RECORDS
        return q, level

    def decode(self, carrier):
        """Scores ``[B, 32]`` float32 on the device (``>= 0.5``: the bit reads 1); one launch for all ``B``."""
        import torch
        q, level = self.read(carrier)
        return 0.5 + 0.5 * torch.tanh(q / level[:, None])

    def encode_host(self, carrier, bits):
        return encode_host(carrier, bits, *self._params())

    def decode_host(self, carrier):
        return decode_host(carrier, *self._params())

    @staticmethod
    def groups_of(message):
        """The payload words of ``message`` (padded / cut to 8 latin-1 characters): one per 32-bit group, in order."""
        from .api import string_to_bits
        payload = string_to_bits(message).reshape(-1)
        return [pack_bits(payload[i:i + BITS]) for i in range(0, len(payload) - BITS + 1, BITS)]

    def mark_many(self, waves, messages):
        """Mark, in place and in ONE launch, every carrier window of every waveform of ``waves`` (1-D float32 device
        tensors at the model rate) with its message (``messages``: one string for all, or one per waveform).  The
        windows are the hook's: group n of the message in the 16 000 samples from 32 000 n.  A waveform too short for
        all groups carries the leading ones and the upstream notice is printed, once per such waveform.  Waveforms that
        are views of one tensor (``convert_many``'s outputs) are marked where they are; others are gathered into one
        buffer first and copied back.  Returns ``waves``."""
        import torch
        waves = list(waves)
        msgs = [messages] * len(waves) if isinstance(messages, str) else list(messages)
        if len(msgs) != len(waves):
            raise ValueError("mark_many: one message for all waveforms, or one per waveform")
        for w in waves:
            if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or not w.is_cuda or w.dim() != 1 or \
                    (w.numel() > 1 and w.stride(0) != 1):
                raise ValueError("mark_many: waveforms must be dense 1-D float32 tensors on a ROCm device")
        plan = []                                        # (wave index, first sample, payload)
        words = {m: self.groups_of(m) for m in set(msgs)}
        for i, (w, m) in enumerate(zip(waves, msgs)):
            groups = words[m]
            fit = [g for n, g in enumerate(groups) if n * STRIDE + WINDOW <= w.numel()]
            plan += [(i, n * STRIDE, g) for n, g in enumerate(fit)]
            if len(fit) < len(groups):
                print("Audio too short, fail to add watermark")
        if not plan:
            return waves
        used = sorted({i for i, _, _ in plan})
        storages = {waves[i].untyped_storage().data_ptr() for i in used}
        if len(storages) == 1:                           # views of one tensor: mark them where they are
            w0 = waves[used[0]]
            base = w0.as_strided((w0.untyped_storage().nbytes() // w0.element_size(),), (1,), 0)
            offs = {i: waves[i].storage_offset() for i in used}
        else:
            base = torch.cat([waves[i] for i in used])
            offs, acc = {}, 0
            for i in used:
                offs[i], acc = acc, acc + waves[i].numel()
        embed_windows(base, base, [(offs[i] + s, offs[i] + s, WINDOW, g) for i, s, g in plan], *self._params())
        self.launches += (len(plan) + MAX_RECORDS - 1) // MAX_RECORDS
        if len(storages) != 1:
            for i in used:
                waves[i].copy_(base[offs[i]:offs[i] + waves[i].numel()])
        return waves
