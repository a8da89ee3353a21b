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

Out of scope: robustness to resampling or MP3 coding, and audio at another rate than the model's (the chips are counted
in model-rate samples).  ``detect_watermark`` keeps upstream's behaviour -- it reads the windows counted from sample 0 and
returns arbitrary characters for unmarked audio; ``find`` (below, "the scan") is the reader that decides whether audio
is marked and where.

``encode`` / ``decode`` / ``mark_many`` run the kernels (csrc/watermark.hip: ``ov_wm_embed_windows_f32``,
``ov_wm_detect_windows_f32``, record-driven, one workgroup per window, ONE launch for all windows); ``encode_host`` /
``decode_host`` restate the definition in float64 numpy (the pattern of ``noise.normal_host``): it is what tools and the
CPU tests use.  There is no CPU fallback.

Streams (``stream``, ``live_stream``, the pools, ``VoiceCloner.speak_stream*`` with ``message=``) carry a block-wise form
of the same mark, because a window's ``d_j`` needs the whole window and a live stream cannot wait 0.73 s for it.  The
carrier windows stay the hook's: window ``n`` is the stream's model-rate output samples ``[32 000 n, 32 000 n + 16 000)``
and carries one 32-bit group; chips and bit ownership are those above, ``i`` counted from the window's start.  A window
is cut into ``M = 16 000 / H`` blocks of ``H`` samples, ``H`` (the hold) one of ``HOLDS`` -- the divisors of 16 000 that
are multiples of 32 and at least ``MIN_WINDOW`` -- so every bit owns exactly ``H / 32`` samples of every block.  Per
window and bit the stream carries one float ``R_j >= 0``, the surplus of the blocks so far in projection units, zero at
the window's start.  For block ``m`` with samples ``x``::

    p_j = mean_{i in block, i % 32 == j} c[i] x[i]
    a_m = max(strength * sqrt(mean_block x^2), floor)
    u_j = b_j p_j + R_j
    d_j = b_j max(a_m - u_j, 0)
    y[i] = x[i] + d_{i % 32} c[i]
    R_j <- max(u_j - a_m, 0)

Block ``m`` moves ``b_j p_j`` of the block to ``b_j p_j + max(a_m - u_j, 0)``, and ``R`` after it is the sum of those
values over the blocks so far minus the sum of their ``a_m``, never below zero: by induction ``sum_m b_j p_j(y_m) >=
sum_m a_m``, and a window's projection is the mean of its blocks', so ``b_j p_j(y) >= mean_m a_m >= floor`` for the
whole window and the unchanged reader returns every bit -- exact by construction, like the file mark.  A block the host
audio (or an earlier block's surplus) already carries is left alone.  With ``H = 16 000`` there is one block, ``R = 0``
and ``u = b p`` exactly: the formulas and, on the device, the bits are the file's (``ov_wm_embed_blocks_f32`` reduces a
block in the order ``ov_wm_embed_windows_f32`` reduces a window).  The block grid is fixed to the stream's sample index,
not to pushes, so the marked stream is a pure function of the unmarked samples, message, key, strength, floor and ``H``:
it does not depend on chunking, on the pool or on the launch.  A sample leaves once its block is complete, at most
``H - 1`` samples later than without a message; samples outside carrier windows pass through in order, behind a held
block; at the end of the stream the samples of an unfinished block leave unmarked.  ``plan_blocks`` is the schedule,
``mark_stream_host`` the float64 mirror of a whole stream, ``MarkBank`` the device side for many streams in one launch.

The scan (``NativeWatermark.find``, ``ToneColorConverter.find_watermark``): chips and bit ownership are counted from the
window's start, so a mark survives any change to the start of the audio -- a cut, a prepended jingle, a clip from the
middle of a ``message_repeat`` stream -- and only a reader that looks at EVERY offset is needed.  With ``i = 32 m + j``,
``t = s + j`` and ``C[m][j] = c[32 m + j]`` (500 x 32, entries +-1)::

    Q[t][j] = sum_{m < 500} x[t + 32 m] C[m][j]          p_j(s) = Q[s + j][j] / 500
    W[t]    = sum_{m < 500} x[t + 32 m]^2                a(s)   = max(strength sqrt(sum_j W[s + j] / 16 000), floor)

which is, for 32 consecutive ``t``, one 32 x 32 x 500 product of the waveform read as a ``[., 32]`` matrix with ``C``:
``ov_wm_scan_f32`` (csrc/watermark_scan.hip) runs it on the fp32 matrix pipe and writes per offset the 32 read bits, ``min_j
|p_j|`` and the level; ``ov_wm_scan_pick`` compacts the offsets whose bits are within ``max_errors`` of a group of the
message -- or, without a message ("blind"), whose weakest projection reaches ``margin`` times the level, which an
unattacked file mark does at every bit by construction and the unmarked test signals did at 11 of 6.5 million offsets,
never twice at the stride -- into an ordered list.  The host
then chains hits that lie ``STRIDE`` apart and whose groups follow each other.  With a known message the expected number
of chance chains of that length, ``S G (sum_{e <= max_errors} C(32, e) / 2^32)^len`` over ``S`` offsets, is reported as
``false_alarm`` and decides ``marked``; the blind criterion (a chain of at least two windows) is a heuristic without
such a figure.  ``scan_host`` is the float64 mirror.
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
# the holds of a marked stream: the divisors of WINDOW that are multiples of BITS and at least MIN_WINDOW
HOLDS = tuple(h for h in range(WINDOW, MIN_WINDOW - 1, -1) if WINDOW % h == 0 and h % BITS == 0)
DEFAULT_HOLD = WINDOW
BLOCK_RECORD_FIELDS = 8     # (src_off, dst_off, H, blocks, bits, chip_off, state_row, reset)


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
    return _read(x, chips_host(key, x.shape[1]), strength, floor)


def _read(x, chips, strength, floor):
    """``read_host`` of rows ``x [B, L]`` with their chips given (a stream's block takes them from inside a window)."""
    cx = x * chips[None, :]
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


def plan_windows(length, groups, repeat=False):
    """The carrier windows of a file of ``length`` samples whose message has ``groups`` groups: ``[(start, group)]`` for
    every window ``n`` (``start = 32 000 n``) that lies wholly inside the file and carries a group -- ``n`` itself below
    ``groups``, ``n % groups`` for every ``n`` with ``repeat``."""
    out, n = [], 0
    while n * STRIDE + WINDOW <= int(length):
        group = _group_of(n, int(groups), repeat)
        if group is None:
            break
        out.append((n * STRIDE, group))
        n += 1
    return out


def scan_host(x, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
    """The float64 mirror of ``ov_wm_scan_f32``: ``(p [S, 32], level [S])`` of the waveform ``x`` (1-D, ``S = len(x) -
    15 999`` offsets): row ``s`` is ``read_host(x[s:s + 16 000])``, computed through the decomposition of the module
    docstring -- ``Q = X C`` on a strided view of ``x``, then the skewed read ``p[s][j] = Q[s + j][j] / 500``."""
    key, strength, floor = check_params(key, strength, floor)
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    S = x.size - WINDOW + 1
    if S < 1:
        raise ValueError(f"scan_host: {x.size} samples hold no window of {WINDOW}")
    rows = WINDOW // BITS
    C = chips_host(key, WINDOW).reshape(rows, BITS)
    T = S + BITS - 1                                     # t = s + j
    X = np.lib.stride_tricks.as_strided(x, shape=(T, rows), strides=(x.strides[0], BITS * x.strides[0]), writeable=False)
    Q, W = np.empty((T, BITS)), np.empty(T)
    for t0 in range(0, T, 8192):                         # (the strided view is copied by the product: bound it)
        part = X[t0:t0 + 8192]
        Q[t0:t0 + 8192] = part @ C
        W[t0:t0 + 8192] = np.einsum("tm,tm->t", part, part)
    sj = np.arange(S)[:, None] + np.arange(BITS)[None, :]
    p = Q[sj, np.arange(BITS)[None, :]] / rows
    energy = W[sj].sum(axis=1)
    return p, np.maximum(strength * np.sqrt(energy / WINDOW), floor)


# ---- the scan: chains of hits and their chance -------------------------------------------------------------------------
HIT_CAPACITY = 4096         # hit rows kept per waveform (the true count is reported beyond it)
MAX_GROUPS = 8
SCAN_RECORD_FIELDS = 3      # (src_off, n, out_off)


def word_to_string(word):
    """The four latin-1 characters a payload word carries (the inverse of ``groups_of`` for one group)."""
    from .api import bits_to_string
    bits = np.array([(int(word) >> j) & 1 for j in range(BITS)], dtype=np.uint8)
    return bits_to_string(bits.reshape(-1, 8))


def false_alarm(offsets, groups, max_errors, length):
    """The expected number of chance chains of ``length`` windows among ``offsets`` scanned offsets for a message of
    ``groups`` groups: ``offsets * groups * (sum_{e <= max_errors} C(32, e) / 2^32)^length`` -- unmarked audio's read
    bits taken as fair coins, independent between windows ``STRIDE`` apart."""
    from math import comb
    if length < 1:
        raise ValueError("false_alarm: a chain has at least one window")
    q = sum(comb(BITS, e) for e in range(int(max_errors) + 1)) / 2.0 ** BITS
    return float(offsets) * float(groups) * q ** int(length)


def build_chains(hits, groups):
    """Chains among ``hits`` (rows ``(s, word, k, errors)`` in ascending ``s``, at most one per ``s``): maximal runs of
    hits at ``s, s + 32 000, ...`` whose group indices run ``k, (k + 1) % groups, ...``; with ``groups == 0`` (blind) any
    hits at that stride chain.  Returns the chains, each a list of hit rows, best first: longest, then fewest errors,
    then earliest."""
    by_s = {int(h[0]): tuple(int(v) for v in h) for h in hits}
    if len(by_s) != len(hits):
        raise ValueError("build_chains: two hits at one offset")

    def follows(a, b):
        return groups == 0 or b[2] == (a[2] + 1) % groups

    chains = []
    for s in sorted(by_s):
        h = by_s[s]
        prev = by_s.get(s - STRIDE)
        if prev is not None and follows(prev, h):
            continue                                     # inside a chain that started earlier
        chain = [h]
        while True:
            nxt = by_s.get(chain[-1][0] + STRIDE)
            if nxt is None or not follows(chain[-1], nxt):
                break
            chain.append(nxt)
        chains.append(chain)
    chains.sort(key=lambda c: (-len(c), sum(h[3] for h in c), c[0][0]))
    return chains


def judge(hits, count, offsets, words, message, max_errors, max_false_alarm, ratios=None):
    """One waveform's verdict from its hit rows (``count``: the true number of hits, which may exceed ``len(hits)``;
    ``words``: the message's groups, empty for blind mode; ``ratios``: ``pmin / level`` per hit row, or None)."""
    G = len(words)
    ratios = [None] * len(hits) if ratios is None else [float(r) for r in ratios]
    ratio_of = {int(h[0]): r for h, r in zip(hits, ratios)}
    chains = build_chains(hits, G)
    res = {"marked": False, "offset": None, "first_group": None, "message": message, "windows": [], "false_alarm": None,
           "hits": int(count), "overflow": int(count) > len(hits)}
    if not chains:
        return res
    best = chains[0]
    res["offset"] = best[0][0]
    res["windows"] = [(s, k if G else None, w & 0xFFFFFFFF, e, ratio_of[s]) for s, w, k, e in best]
    if G:
        res["first_group"] = best[0][2]
        res["false_alarm"] = false_alarm(offsets, G, max_errors, len(best))
        res["marked"] = res["false_alarm"] <= max_false_alarm
    else:
        res["message"] = "".join(word_to_string(w) for _, w, _, _ in best)
        res["marked"] = len(best) >= 2
    return res


def check_find_args(message, max_errors, margin, max_false_alarm, capacity=HIT_CAPACITY):
    """The arguments of ``find`` as ``(payload words, max_errors, margin, max_false_alarm, capacity)``; ValueError for a
    message that is no string, ``max_errors`` outside ``[0, 32]``, ``margin`` outside ``(0, 1]``, ``max_false_alarm``
    outside ``(0, 1]`` or a negative capacity."""
    if message is not None and not isinstance(message, str):
        raise ValueError(f"message must be a string or None, got {message!r}")
    if not _is_int(max_errors) or not 0 <= int(max_errors) <= BITS:
        raise ValueError(f"max_errors: an int in [0, {BITS}], got {max_errors!r}")
    if not isinstance(margin, (int, float, np.floating)) or isinstance(margin, bool) or not 0.0 < float(margin) <= 1.0:
        raise ValueError(f"margin outside (0, 1]: {margin!r}")
    if not isinstance(max_false_alarm, (int, float, np.floating)) or isinstance(max_false_alarm, bool) or \
            not 0.0 < float(max_false_alarm) <= 1.0:
        raise ValueError(f"max_false_alarm outside (0, 1]: {max_false_alarm!r}")
    if not _is_int(capacity) or int(capacity) < 0:
        raise ValueError(f"capacity: a non-negative int, got {capacity!r}")
    words = [] if message is None else groups_of(message)
    return words, int(max_errors), float(margin), float(max_false_alarm), int(capacity)


# ---- streams: the schedule and the float64 mirror ---------------------------------------------------------------------
def check_hold(hold):
    """``hold`` as an int of ``HOLDS``; ValueError otherwise."""
    if not _is_int(hold) or int(hold) not in HOLDS:
        raise ValueError(f"watermark_hold must be one of {HOLDS}, got {hold!r}")
    return int(hold)


def groups_of(message):
    """The payload words of ``message`` (padded / cut to 8 latin-1 characters): one per 32-bit group, in order."""
    from .api import string_to_bits
    payload = string_to_bits(message).reshape(-1)
    return [pack_bits(payload[i:i + BITS]) for i in range(0, len(payload) - BITS + 1, BITS)]


def _group_of(n, groups, repeat):
    """The message group window ``n`` carries, or None: ``n`` itself below ``groups``, ``n % groups`` with ``repeat``."""
    if groups < 1 or (n >= groups and not repeat):
        return None
    return n % groups


def plan_blocks(pos, n_new, closing, H, groups, repeat):
    """The schedule of a marked stream, a pure function.  ``pos``: the stream's samples that have left; ``n_new``: the
    samples at hand from ``pos`` on (the held ones, then the new ones); ``closing``: they are the stream's last;
    ``groups``: the message's group count; ``repeat``: ``message_repeat``.  Returns ``(n_out, records)``: the first
    ``n_out`` of the samples at hand leave now -- all of them, except the samples of an unfinished block of a carrier
    window (which leave too, unmarked, when ``closing``) -- and ``records`` = ``[(off, blocks, window, group, chip_off,
    reset)]``: the run of ``blocks`` whole blocks that starts ``off`` samples after ``pos`` belongs to carrier window
    ``window``, carries message group ``group``, begins ``chip_off`` samples after the window's start, and starts the
    window's state afresh (``reset``) or continues it.  At most one record per window.  ``pos`` is where an earlier call
    left it: outside the carrier windows, or on a block boundary."""
    pos, n_new, H = int(pos), int(n_new), check_hold(H)
    if pos < 0 or n_new < 0:
        raise ValueError(f"plan_blocks: pos {pos}, n_new {n_new}")
    end, records, n_out = pos + n_new, [], n_new
    n = pos // STRIDE
    while n * STRIDE < end:
        group = _group_of(n, groups, repeat)
        if group is None:
            if not repeat:
                break                                    # no later window carries anything
            n += 1
            continue
        w0 = n * STRIDE
        lo, hi = max(pos, w0), min(end, w0 + WINDOW)
        if lo < w0 + WINDOW:
            if (lo - w0) % H:
                raise ValueError(f"plan_blocks: pos {pos} lies inside a block of window {n}")
            m0, m1 = (lo - w0) // H, (hi - w0) // H
            if m1 > m0:
                records.append((lo - pos, m1 - m0, n, group, m0 * H, m0 == 0))
            if hi < w0 + WINDOW and not closing:         # the stream ends inside this window, for now
                n_out = w0 + m1 * H - pos
        n += 1
    return n_out, records


def mark_stream_host(x, message, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR, hold=DEFAULT_HOLD, repeat=False):
    """The float64 mirror of a whole marked stream: ``x`` (1-D, the stream's unmarked model-rate output from its start
    to its end) -> the samples the stream emits with ``message=message, watermark_hold=hold, message_repeat=repeat``.
    Every whole block of a carrier window inside ``x`` is marked, the samples of an unfinished block are not."""
    key, strength, floor = check_params(key, strength, floor)
    H, words = check_hold(hold), groups_of(message)
    y = np.array(x, dtype=np.float64).reshape(-1)
    c = chips_host(key, WINDOW)
    _, records = plan_blocks(0, y.size, True, H, len(words), repeat)
    for off, blocks, _, group, chip_off, reset in records:
        assert reset and chip_off == 0                   # one call: every window from its start
        b = np.array([1.0 if (words[group] >> j) & 1 else -1.0 for j in range(BITS)])
        R = np.zeros(BITS)
        for m in range(blocks):
            blk = y[off + m * H:off + (m + 1) * H]       # a view: marked in place
            cm = c[m * H:(m + 1) * H]
            p, a = _read(blk[None, :], cm, strength, floor)          # as read_host adds a window
            p, a = p[0], a[0]
            u = b * p + R
            d = b * np.maximum(a - u, 0.0)
            R = np.maximum(u - a, 0.0)
            blk += np.tile(d, H // BITS) * cm
    return y


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


def embed_blocks(src, dst, records, state, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR):
    """``ov_wm_embed_blocks_f32`` on host rows ``(src_off, dst_off, H, blocks, bits, chip_off, state_row, reset)``
    (``state``: float32 ``[rows, 32]`` on the device), uploaded in one copy, ONE launch (per 65535 records).  The rows go
    to the kernel as they are: it checks every one and a bad one writes nothing."""
    import torch
    key, strength, floor = check_params(key, strength, floor)
    _check_buffer(src, "src")
    _check_buffer(dst, "dst")
    _check_buffer(state, "state")
    if state.dim() != 2 or state.shape[1] != BITS:
        raise ValueError(f"state must be [rows, {BITS}]")
    table = [tuple(int(v) for v in rec) for rec in records]
    if any(len(rec) != BLOCK_RECORD_FIELDS for rec in table):
        raise ValueError("a block record is (src_off, dst_off, H, blocks, bits, chip_off, state_row, reset)")
    for i in range(0, len(table), MAX_RECORDS):
        part = table[i:i + MAX_RECORDS]
        recs = torch.tensor(part, dtype=torch.int64).to(src.device)
        _lib.call("ov_wm_embed_blocks_f32", src, src.numel(), dst, dst.numel(), recs, len(part), state, state.shape[0], key,
                  strength, floor)


def scan(src, records, key=0, strength=DEFAULT_STRENGTH, floor=DEFAULT_FLOOR, out_elems=None, projections=False):
    """``ov_wm_scan_f32`` on host rows ``(src_off, n, out_off)``: ``(words int32 [E], pmin [E], level [E])`` on the
    device (``E = out_elems``, default: where the last output range ends), and ``p [E, 32]`` as a fourth with
    ``projections``.  What no record covers keeps its fill: 0 / NaN.  ONE launch (per 65535 records).  The rows go to the
    kernel as they are: it checks every one and a bad one writes nothing."""
    import torch
    key, strength, floor = check_params(key, strength, floor)
    _check_buffer(src, "src")
    table = [tuple(int(v) for v in rec) for rec in records]
    if not table or any(len(rec) != SCAN_RECORD_FIELDS for rec in table):
        raise ValueError("a scan record is (src_off, n, out_off), and a call has at least one")
    if out_elems is None:
        out_elems = max(oo + max(n - WINDOW + 1, 0) for _, n, oo in table)
    out_elems = max(int(out_elems), 1)
    dev = src.device
    words = torch.zeros(out_elems, dtype=torch.int32, device=dev)
    pmin = torch.full((out_elems,), float("nan"), dtype=torch.float32, device=dev)
    level = torch.full((out_elems,), float("nan"), dtype=torch.float32, device=dev)
    p = torch.full((out_elems, BITS), float("nan"), dtype=torch.float32, device=dev) if projections else None
    for i in range(0, len(table), MAX_RECORDS):
        part = table[i:i + MAX_RECORDS]
        max_n = min(max(max(n for _, n, _ in part), WINDOW), MAX_WINDOW)
        recs = torch.tensor(part, dtype=torch.int64).to(dev)
        _lib.call("ov_wm_scan_f32", src, src.numel(), recs, len(part), max_n, key, strength, floor, words, pmin, level, p,
                  out_elems)
    return (words, pmin, level, p) if projections else (words, pmin, level)


def scan_pick(words, pmin, level, records, groups=(), max_errors=0, margin=0.98, capacity=HIT_CAPACITY):
    """``ov_wm_scan_pick`` on host rows ``(scan_off, S)``: ``(hits int32 [R, capacity, 4], counts int32 [R])`` on the
    device; ``groups``: up to 8 payload words, none for blind mode.  ONE launch (per 65535 records)."""
    import torch
    dev = words.device
    table = [tuple(int(v) for v in rec) for rec in records]
    if not table or any(len(rec) != 2 for rec in table):
        raise ValueError("a pick record is (scan_off, S), and a call has at least one")
    groups = [int(g) for g in groups]
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"at most {MAX_GROUPS} groups")
    g = None
    if groups:
        g = torch.tensor([w - (1 << BITS) if w >= 1 << (BITS - 1) else w for w in groups], dtype=torch.int32).to(dev)
    hits = torch.zeros(len(table), capacity, 4, dtype=torch.int32, device=dev)
    counts = torch.zeros(len(table), dtype=torch.int32, device=dev)
    for i in range(0, len(table), MAX_RECORDS):
        part = table[i:i + MAX_RECORDS]
        recs = torch.tensor(part, dtype=torch.int64).to(dev)
        _lib.call("ov_wm_scan_pick", words, pmin, level, words.numel(), recs, len(part), g, len(groups), int(max_errors),
                  float(margin), hits[i:i + len(part)] if capacity else None, capacity, counts[i:i + len(part)])
    return hits, counts


def stream_mark(model, message, hold=DEFAULT_HOLD, repeat=False):
    """The ``message=`` / ``watermark_hold=`` / ``message_repeat=`` keywords of the stream entry points, checked at the
    call: None without a message, else ``(model, payload words, H, repeat)``.  ValueError for a hold outside ``HOLDS``
    and for a message on a converter whose ``watermark_model`` is not a ``NativeWatermark``."""
    H = check_hold(hold)
    if message is None:
        return None
    if not isinstance(message, str):
        raise ValueError(f"message must be a string or None, got {message!r}")
    if not isinstance(model, NativeWatermark):
        raise ValueError('message= on a stream needs the native watermark: ToneColorConverter(..., watermark="native")')
    return model, groups_of(message), H, bool(repeat)


def hold_wait(mark):
    """Samples a marked stream's output waits at most behind the unmarked one: ``H - 1`` (0 without a mark)."""
    return 0 if mark is None else mark[2] - 1


class _Marked:
    def __init__(self, mark, slot, dev):
        import torch
        self.model, self.words, self.H, self.repeat = mark
        self.slot = slot                # state rows 2 slot and 2 slot + 1
        self.pos = 0                    # samples that have left
        self.held = torch.empty(0, dtype=torch.float32, device=dev)      # samples [pos, ..) of an unfinished block
        self.pending, self.ending = [], False
        self.cur = 0                    # the state row of the window left open
        self.whole = set()              # message groups that got a whole carrier window


class MarkBank:
    """The block-wise marks of many streams, stepped together (module docstring, "streams"); the interface of
    ``rates.ResamplerBank``.  ``open(mark)`` (``mark``: what ``stream_mark`` returned) -> key; ``push(key, x)`` queues
    this round's model-rate output of a stream; ``end(key)`` marks the end of it; ``step()`` -> ``{key: the samples that
    may leave}`` (views of one packed tensor) after ONE launch of ``ov_wm_embed_blocks_f32`` per model in use for every
    whole block at hand.  Per stream the bank holds the position, the held samples of an unfinished block (fewer than
    ``H``) and two state rows.  A piece that spans several windows has a record per window, and no two records of a
    launch share a row: the window a piece continues keeps the stream's current row, a window it leaves open takes the
    other one (which becomes the current one), and a window that begins and ends inside the piece, whose row nobody
    reads again, takes a scratch row of the launch.  An ended key leaves the bank with its ``step()``, which prints the
    upstream notice if some group of its message never got a whole window."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self._ms, self._next = {}, 0
        self._free, self._slots, self._state = [], 0, None
        self.launches = 0

    def __contains__(self, key):
        return key in self._ms

    def __len__(self):
        return len(self._ms)

    def open(self, mark):
        import torch
        if not self._free:
            grown = max(1, 2 * self._slots)
            state = torch.zeros(2 * grown, BITS, dtype=torch.float32, device=self.device)
            if self._state is not None:
                state[:2 * self._slots].copy_(self._state[:2 * self._slots])
            self._free, self._slots, self._state = list(range(grown - 1, self._slots - 1, -1)), grown, state
        k = self._next
        self._next += 1
        self._ms[k] = _Marked(mark, self._free.pop(), self.device)
        return k

    def push(self, key, x):
        m = self._ms[key]
        if m.ending:
            raise RuntimeError("push() after end()")
        if x.numel():
            m.pending.append(x.reshape(-1))

    def end(self, key):
        self._ms[key].ending = True

    def drop(self, key):
        m = self._ms.pop(key, None)
        if m is not None:
            self._free.append(m.slot)

    def step(self):
        import torch
        work = [(k, m) for k, m in self._ms.items() if m.pending or m.ending]
        if not work:
            return {}
        pieces, spans, recs, acc, n_scratch = [], [], {}, 0, 0
        for k, m in work:
            pieces += [m.held] + m.pending
            n = m.held.numel() + sum(p.numel() for p in m.pending)
            n_out, plan = plan_blocks(m.pos, n, m.ending, m.H, len(m.words), m.repeat)
            for off, blocks, window, group, chip_off, reset in plan:
                whole = chip_off + blocks * m.H == WINDOW
                if not reset:                            # continues the window the last step left open
                    row = 2 * m.slot + m.cur
                elif whole:                              # begins and ends here: nobody reads its row again
                    row, n_scratch = ("scratch", n_scratch), n_scratch + 1
                else:                                    # left open: the stream's other row becomes its current one
                    m.cur ^= 1
                    row = 2 * m.slot + m.cur
                recs.setdefault(m.model, []).append([acc + off, acc + off, m.H, blocks, m.words[group], chip_off, row,
                                                     int(reset)])
                if whole:
                    m.whole.add(group)
            spans.append((k, m, acc, n_out, n))
            m.pos, m.pending = m.pos + n_out, []
            acc += n
        pieces = [p for p in pieces if p.numel()]
        # always a fresh tensor: marked in place, and the held samples below are views of it
        arena = torch.cat(pieces) if pieces else torch.empty(0, dtype=torch.float32, device=self.device)
        rows = 2 * self._slots
        if self._state.shape[0] < rows + n_scratch:       # the streams' rows first, this launch's scratch rows behind
            grown = torch.zeros(rows + 2 * n_scratch, BITS, dtype=torch.float32, device=self.device)
            grown[:rows].copy_(self._state[:rows])
            self._state = grown
        for model, table in recs.items():
            for rec in table:
                if type(rec[6]) is tuple:
                    rec[6] = rows + rec[6][1]
            embed_blocks(arena, arena, table, self._state, model.key, model.strength, model.floor)
            n_launch = (len(table) + MAX_RECORDS - 1) // MAX_RECORDS
            self.launches += n_launch
            model.launches += n_launch
        res = {}
        for k, m, a, n_out, n in spans:
            if n_out:
                res[k] = arena[a:a + n_out]
            m.held = arena[a + n_out:a + n]
            if m.ending:
                if len(m.whole) < len(m.words):
                    print("Audio too short, fail to add watermark")
                self.drop(k)
        return res


class StreamMarker:
    """One stream's mark (a bank of one): ``push(x)`` -> the samples that may leave, ``close(x=None)`` -> the rest."""

    def __init__(self, mark, device):
        import torch
        self.bank = MarkBank(device)
        self.key = self.bank.open(mark)
        self._none = torch.empty(0, dtype=torch.float32, device=self.bank.device)

    def push(self, x):
        self.bank.push(self.key, x)
        return self.bank.step().get(self.key, self._none)

    def close(self, x=None):
        if x is not None:
            self.bank.push(self.key, x)
        self.bank.end(self.key)
        return self.bank.step().get(self.key, self._none)


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
        return groups_of(message)

    def mark_many(self, waves, messages, *, message_repeat=False):
        """Mark, in place and in ONE launch, every carrier window of every waveform of ``waves`` (1-D float32 device
        tensors at the model rate) with its message (``messages``: one string for all, or one per waveform).  The
        windows are the hook's: group n of the message in the 16 000 samples from 32 000 n; with ``message_repeat``
        every window n the file holds carries group ``n % G``, as a stream's may, so that a file cut anywhere still
        holds a chain ``find`` can follow.  A waveform too short for
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
            fit = plan_windows(w.numel(), len(groups), bool(message_repeat))
            plan += [(i, start, groups[k]) for start, k in fit]
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

    def find(self, waves, message=None, *, max_errors=0, margin=0.98, max_false_alarm=1e-6, capacity=HIT_CAPACITY):
        """Look for the mark at EVERY offset of every waveform of ``waves`` (1-D float32 device tensors at the model
        rate): one ``ov_wm_scan_f32`` launch and one ``ov_wm_scan_pick`` launch for all of them, then chains on the
        host.  With ``message`` an offset is a hit when its 32 read bits are within ``max_errors`` of one of the
        message's groups; hits ``32 000`` apart whose groups follow each other (``k, k + 1 mod G``) form a chain, and
        the best chain (longest, fewest errors, earliest) is the answer.  Returns one dict per waveform:

        * ``marked``: ``false_alarm <= max_false_alarm``;
        * ``offset``: the start of the chain's first window (None without a hit), ``first_group``: the group it carries;
        * ``message``: the message asked for, or in blind mode the characters read, four per window in chain order;
        * ``windows``: ``(offset, group, word, errors, pmin / level)`` per window of the chain;
        * ``false_alarm``: the expected number of chance chains of this length, ``S G (sum_{e <= max_errors} C(32, e) /
          2^32)^len`` over the ``S`` offsets scanned -- about 1e-4 for ONE exact window in a 10 s file, which is
          therefore reported but not called marked at the default, and 1e-14 for two;
        * ``hits``: hit offsets in all, ``overflow``: more than ``capacity`` of them (the chains then come from the first
          ``capacity``).

        Without a message (blind mode) an offset is a hit when ``min_j |p_j| >= margin * level`` -- every bit reaches
        the level, as the embedder guarantees for a file mark and unmarked test signals gave at 11 of 6.5 million
        offsets; any hits ``32 000`` apart chain, ``marked`` needs a chain of at least two windows and ``false_alarm`` is
        None: this criterion is a HEURISTIC, with no proven false-alarm figure (DESIGN.md section 29 gives the counts
        measured on unmarked signals), and audio that went through int16 or any other change may fall under
        ``margin``.  Audio at another rate than the model's is out of scope.  Arguments are checked at the call."""
        import torch
        words, max_errors, margin, max_false_alarm, capacity = check_find_args(message, max_errors, margin, max_false_alarm,
                                                                               capacity)
        waves = list(waves)
        for w in waves:
            if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or not w.is_cuda or w.dim() != 1:
                raise ValueError("find: waveforms must be 1-D float32 tensors on a ROCm device")
        long = [i for i, w in enumerate(waves) if w.numel() >= WINDOW]
        results = [judge([], 0, 0, words, message, max_errors, max_false_alarm) for _ in waves]
        if not long:
            return results
        src = torch.cat([waves[i] for i in long]) if len(long) > 1 else waves[long[0]].contiguous()
        recs, picks, so, oo = [], [], 0, 0
        for i in long:
            n = waves[i].numel()
            recs.append((so, n, oo))
            picks.append((oo, n - WINDOW + 1))
            so, oo = so + n, oo + n - WINDOW + 1
        sw, pmin, level = scan(src, recs, *self._params(), out_elems=oo)
        hits, counts = scan_pick(sw, pmin, level, picks, words, max_errors, margin, capacity)
        self.launches += 2 * ((len(recs) + MAX_RECORDS - 1) // MAX_RECORDS)
        counts = counts.cpu().numpy()
        kept = np.minimum(counts, capacity)
        hits = hits.cpu().numpy()
        where = np.concatenate([picks[r][0] + hits[r, :kept[r], 0].astype(np.int64) for r in range(len(long))])
        ratios = np.zeros(0)
        if where.size:
            idx = torch.from_numpy(where).to(src.device)
            ratios = (pmin[idx] / level[idx]).cpu().numpy()
        at = 0
        for r, i in enumerate(long):
            rows = [tuple(int(v) for v in h) for h in hits[r, :kept[r]]]
            results[i] = judge(rows, counts[r], picks[r][1], words, message, max_errors, max_false_alarm,
                               ratios[at:at + kept[r]])
            at += kept[r]
        return results
