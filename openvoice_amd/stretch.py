"""``speed=`` / ``duration=`` of a conversion: the definition, as a float64 / integer mirror (numpy only, no device code).

This is the PROJECT'S OWN definition -- nothing in the reference stretches a conversion.  The HiFi-GAN generator makes
``hop`` samples from every latent frame, so resampling its input ``z_hat * y_mask`` along time changes the duration while
the generator makes pitch and phase afresh (the base-speaker TTS changes speed the same way, through its path expansion).

Fixed-point step: ``step = round(speed * 2**32)`` (a Python int), ``0.5 <= speed <= 2.0``.  Output frame ``j`` -- a GLOBAL
index, counted from the recording's first frame -- sits at ``pos = j * step`` (int64):

    i = pos >> 32,    f = ((pos & 0xffffffff) >> 8) * 2**-24   (24 bits: exact in fp32),
    out[c][j] = z[c][i] + f * (z[c][min(i + 1, T_in - 1)] - z[c][i])      (fp32: subtract, multiply, add; no fma)
    T_out = (T_in * 2**32 - 1) // step + 1                                   (the j with i <= T_in - 1)

``step == 2**32`` is the identity (f = 0 everywhere).  The weights depend on the global ``j`` alone, so a window of a long
recording -- a slice of the source whose column 0 is global frame ``i0``, writing the output frames from ``j0`` on --
computes the bits of the whole-file stretch (``stretch_rows(..., i0=, j0=)``).  ``ov_stretch_rows_f32``
(csrc/stretch.hip) is the kernel; ``check_record`` mirrors its record checks.
"""
import math
import numbers

import numpy as np

ONE = 1 << 32                        # the step of speed 1
MIN_SPEED, MAX_SPEED = 0.5, 2.0
RECORD_FIELDS = 10                   # (src_off, dst_off, rows, src_ld, dst_ld, t_in, i0, j0, n_out, step)
_MAX_DIM, _MAX_OFF, _MAX_J = 1 << 31, 1 << 61, 1 << 29      # j * step < 2^29 * 2^33 = 2^62


def step_of(speed):
    """``round(speed * 2**32)`` of a speed in ``[0.5, 2.0]``; anything else (a bool, a string, a non-finite number, a
    number outside the range) is a ValueError."""
    if isinstance(speed, (bool, str, bytes)) or not isinstance(speed, numbers.Real):
        raise ValueError(f"speed must be a number in [{MIN_SPEED}, {MAX_SPEED}], got {speed!r}")
    speed = float(speed)
    if not math.isfinite(speed) or not MIN_SPEED <= speed <= MAX_SPEED:
        raise ValueError(f"speed must lie in [{MIN_SPEED}, {MAX_SPEED}], got {speed!r}")
    return int(round(speed * ONE))


def speed_of_duration(duration, T_in, hop, sr):
    """The speed that makes ``T_in`` frames of ``hop`` samples last ``duration`` seconds at ``sr`` Hz:
    ``T_in * hop / (duration * sr)`` (range-checked by ``step_of`` like any speed)."""
    if isinstance(duration, (bool, str, bytes)) or not isinstance(duration, numbers.Real) or not duration > 0 \
            or not math.isfinite(duration):
        raise ValueError(f"duration must be a positive number of seconds, got {duration!r}")
    return int(T_in) * int(hop) / (float(duration) * float(sr))


def resolve(speed, duration, T_in=None, hop=None, sr=None):
    """The step of one item from its ``speed=`` / ``duration=``: None when both are None (today's path), a ValueError
    when both are given or the resulting speed leaves ``[0.5, 2.0]``."""
    if speed is not None and duration is not None:
        raise ValueError("speed= and duration= are two ways to say the same thing: give one of them")
    if duration is not None:
        speed = speed_of_duration(duration, T_in, hop, sr)
    return None if speed is None else step_of(speed)


def per_item(name, value, n):
    """``value`` -- None, one number, or a list / tuple / array with one entry (a number or None) per item -- as a list
    of ``n`` entries; a list of another length is a ValueError."""
    if isinstance(value, np.ndarray):
        value = value.tolist()
    if hasattr(value, "tolist") and not isinstance(value, (list, tuple)):      # a tensor
        value = value.tolist()
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError(f"{name}: one value, or one per item ({n}), got {len(value)}")
        return list(value)
    return [value] * n


def resolve_items(speed, duration, frames, hop, sr):
    """Steps of ``len(frames)`` items (``frames[b]``: item b's ``T_in``) from ``speed=`` / ``duration=``, each one value
    or one per item: None when no item is stretched at all, else a list of steps (``ONE`` for an item left alone)."""
    n = len(frames)
    speeds, durations = per_item("speed", speed, n), per_item("duration", duration, n)
    steps = [resolve(s, d, T, hop, sr) for s, d, T in zip(speeds, durations, frames)]
    if all(s is None for s in steps):
        return None
    return [ONE if s is None else s for s in steps]


def kw(**named):
    """The keywords that are not None: a callee that was not given any sees today's call."""
    return {k: v for k, v in named.items() if v is not None}


def reject_stream(what, speed=None, duration=None):
    """Streams and pools take no ``speed=`` / ``duration=``: a stretched stream has a rate mismatch between its input
    and its output that needs a design of its own.  ValueError when either is given."""
    if speed is not None or duration is not None:
        raise ValueError(f"{what}: speed= / duration= are not supported on streams and pools (a stretched stream's input "
                         f"and output run at different rates); convert the recording with convert / convert_long / "
                         f"convert_many")


def t_out(T_in, step):
    """Output frames of ``T_in`` input frames: the number of ``j`` with ``(j * step) >> 32 <= T_in - 1``."""
    return (int(T_in) * ONE - 1) // int(step) + 1


def first_output_at(i, step):
    """The first ``j`` whose ``i(j) >= i``: ``ceil(i * 2**32 / step)``."""
    return -((-int(i) * ONE) // int(step))


def positions(j0, n, step):
    """``(i int64 [n], f float32 [n])`` of the output frames ``j0 .. j0 + n``."""
    pos = (np.arange(int(j0), int(j0) + int(n), dtype=np.int64)) * np.int64(step)
    return pos >> 32, ((pos & 0xffffffff) >> 8).astype(np.float32) * np.float32(2.0 ** -24)


def stretch_rows(z, step, T_in=None, i0=0, j0=0, n_out=None):
    """The mirror: ``z`` [rows, t_in] float32, column 0 being global frame ``i0`` of a recording of ``T_in`` frames
    (default: ``z`` is the whole recording) -> the output frames ``[j0, j0 + n_out)`` (default: all from ``j0`` on),
    [rows, n_out] float32, in the kernel's operation order."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    T_in = i0 + z.shape[1] if T_in is None else int(T_in)
    n_out = t_out(T_in, step) - j0 if n_out is None else int(n_out)
    i, f = positions(j0, n_out, step)
    if n_out < 1 or i[0] < i0 or i[-1] > T_in - 1 or i[-1] - i0 > z.shape[1] - 1:
        raise ValueError("stretch_rows: the output frames reach outside the slice")
    i1 = np.minimum(i + 1, T_in - 1)
    if i1[-1] - i0 > z.shape[1] - 1:
        raise ValueError("stretch_rows: the slice ends before the neighbour of its last frame")
    a, b = z[:, i - i0], z[:, i1 - i0]
    d = (b - a).astype(np.float32)                       # three fp32 roundings: subtract, multiply, add
    return (a + (f[None, :] * d).astype(np.float32)).astype(np.float32)


def record(src_off, dst_off, rows, src_ld, dst_ld, t_in, i0, j0, n_out, step):
    return (int(src_off), int(dst_off), int(rows), int(src_ld), int(dst_ld), int(t_in), int(i0), int(j0), int(n_out),
            int(step))


def check_record(rec, src_elems, dst_elems):
    """True where ``ov_stretch_rows_f32`` accepts the record (the same checks, in Python integers): sane fields, both
    extents, and ``0 <= i - i0 <= t_in - 1`` for every ``j`` it covers (``i`` is monotone: the first and the last)."""
    if len(rec) != RECORD_FIELDS:
        return False
    so, do, rows, sld, dld, t_in, i0, j0, n_out, step = (int(v) for v in rec)
    if not (1 <= rows <= _MAX_DIM and 1 <= t_in <= _MAX_DIM and 1 <= n_out <= _MAX_DIM):
        return False
    if not (t_in <= sld <= _MAX_DIM and n_out <= dld <= _MAX_DIM and 0 <= so <= _MAX_OFF and 0 <= do <= _MAX_OFF):
        return False
    if not (0 <= i0 <= _MAX_DIM and 0 <= j0 and j0 + n_out <= _MAX_J and ONE // 2 <= step <= 2 * ONE):
        return False
    if so + (rows - 1) * sld + t_in > src_elems or do + (rows - 1) * dld + n_out > dst_elems:
        return False
    first, last = (j0 * step) >> 32, ((j0 + n_out - 1) * step) >> 32
    return first >= i0 and last - i0 <= t_in - 1


# ---- long recordings: windows cut on source frames, stretched with their global (i0, j0) ------------------------------
def context_frames(frame_reach, generator_margin, step, grid=1):
    """One-sided context, in SOURCE frames, of a window whose latent is stretched by ``step`` before the generator.
    ``frame_reach`` source frames serve the posterior encoder and the flow (they run before the stretch);
    the generator then needs ``generator_margin`` OUTPUT frames beyond a core edge, which are ``generator_margin *
    speed`` source frames -- charged at ``max(1, speed)`` -- plus what the stretch itself needs: one frame for the
    neighbour ``i + 1`` and, per edge, up to three output frames lost to the two ceilings that place the window on the
    output grid (``plan_windows``).  Rounded up to ``grid``.  At speed 1 this is ``longform.context_frames`` (120)."""
    num = (int(generator_margin) + 3) * max(int(step), ONE)
    reach = int(frame_reach) + -(-num // ONE) + 2
    return -(-reach // int(grid)) * int(grid)


def plan_windows(plan, T, window_frames, step, frame_reach, generator_margin):
    """The stretched form of a ``longform.plan_windows`` plan (``(first_frame, core_lo, core_hi)`` in source frames, made
    with ``context_frames(...)`` of context): per window ``(ja, n, j_lo, j_hi)`` in OUTPUT frames.  The window's latent
    is exact on the source frames ``[f0 + frame_reach, f0 + Tw - frame_reach)`` (to the file's edge where it touches
    one); the generator runs on the ``n`` output frames from ``ja`` on, all of which read source frames in that range,
    and the window emits ``[j_lo, j_hi)``: the output frames whose ``i`` lies in its core.  ``[ja, ja + n)`` holds
    ``generator_margin`` output frames beyond each core edge that is not a file edge, starts at 0 in the first window
    and ends at ``T_out`` in the last, so every launch is a dense batch as in the unstretched plan.  Regular windows
    share one ``n``; ValueError where a window cannot serve its core (a context smaller than ``context_frames``)."""
    T, Tw, step, R, M = int(T), min(int(T), int(window_frames)), int(step), int(frame_reach), int(generator_margin)
    To = t_out(T, step)
    spans = []
    for f0, lo, hi in plan:
        va = f0 + R if f0 > 0 else 0                                    # valid source frames [va, vb)
        vb = f0 + Tw - R if f0 + Tw < T else T
        ja_min = first_output_at(va, step)
        # the last j whose neighbour i + 1 is still inside [va, vb): i <= vb - 2 (at the true end the clamp serves it)
        jb_max = To if vb == T else first_output_at(vb - 1, step)
        j_lo, j_hi = first_output_at(lo, step), (To if hi == T else first_output_at(hi, step))
        spans.append((ja_min, jb_max, max(0, j_lo - M), min(To, j_hi + M), j_lo, j_hi))
    regular = [s[3] - s[2] for s, (f0, lo, hi) in zip(spans, plan) if f0 > 0 and hi < T]
    n_reg = max(regular) if regular else 0
    out = []
    for (ja_min, jb_max, need_a, need_b, j_lo, j_hi) in spans:
        n = max(need_b - need_a, n_reg if jb_max - ja_min >= n_reg else 0)
        ja = min(need_a, jb_max - n)
        if ja < ja_min or ja + n < need_b:
            raise ValueError(f"stretched window cannot serve its core: output frames [{need_a}, {need_b}) needed, "
                             f"[{ja_min}, {jb_max}) available (window_frames too small for this speed?)")
        out.append((ja, n, j_lo, j_hi))
    return out
