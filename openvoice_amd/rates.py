"""Rate conversion inside streams: resamplers that carry their state across pushes, for many streams in one launch.

Live and windowed streams convert at the model rate (22 050 Hz); clients send and want audio at their own rates.  A
stream opened with ``sr_in`` / ``sr_out`` runs its input through a resampler to the model rate and its output through
another one back out.  Both apply ``audio_io.kaiser_best_phases``, the filter of ``resample_kaiser_best`` and
``resample_on_device``, and each output sample is computed by the same device function as ``ov_polyphase_fir_f32``'s, so a
stream's output equals the whole-file conversion bit for bit however the input was split into pushes.

Schedule of one resampler (``Schedule``): output t sits at input time ``t Q / P`` and reads input samples
``n - taps + 1 .. n + taps`` (n = ``(t Q) // P``).  It leaves as soon as all of its right taps have arrived
(``n + taps < received``); at the end of the input the remaining outputs up to ``n_in P // Q`` (resampy's count) are
computed with the indices past the end skipped, then zero-padded to ``ceil(n_in P / Q)`` (librosa's ``fix=True``).  What
is kept between steps is the input from the first tap of the next output on: fewer than ``2 taps`` samples.  A sample of
the output leaves at most ``taps`` input samples after its own instant (``latency_seconds``: 2.9 ms at 48 kHz -> 22.05
kHz, 2.9 ms at 22.05 kHz -> 48 kHz).

Device side, a ``ResamplerBank`` steps the resamplers of many streams (one direction) with ONE launch of
``ov_polyphase_fir_rows_f32``: each stream's kept window and its new pushes are packed into one arena tensor, one record
per stream names its window, rate pair and outputs, and the outputs land in one packed tensor that the streams receive
views of.  A stream's kept window is a view into the arena of its last step (no copy).  The phase tables of every rate
pair in use sit in one float64 tensor, built from ``audio_io``'s resident per-(pair, device) tables.
"""
import math
import numbers
from fractions import Fraction

import torch

from . import _lib, audio_io

MODEL_RATE = 22050
RECORD_FIELDS = 11          # ov_polyphase_fir_rows_f32's record (include/openvoice_amd.h)
MAX_RECORDS = 65535


def check_rate(sr, what="sample rate"):
    """``None`` or a positive integer rate (Python or numpy integer, not bool); ValueError otherwise."""
    if sr is None:
        return None
    if isinstance(sr, bool) or not isinstance(sr, numbers.Integral) or int(sr) <= 0:
        raise ValueError(f"{what} must be a positive integer (Hz) or None, got {sr!r}")
    return int(sr)


_pairs = {}


def pair(sr_in, sr_out):
    """``(P, Q, taps)`` of the resampler sr_in -> sr_out (P / Q = sr_out / sr_in in lowest terms)."""
    key = (int(sr_in), int(sr_out))
    if key not in _pairs:
        _, P, Q, taps = audio_io.kaiser_best_phases(*key)
        _pairs[key] = (P, Q, taps)
    return _pairs[key]


def latency_seconds(sr_in, sr_out):
    """The most any output sample of an sr_in -> sr_out resampler waits after its own instant: ``taps / sr_in``
    (0 for equal rates).  Exact: with 1-sample pushes an output at an integer input position waits exactly that."""
    if sr_in is None or sr_out is None or int(sr_in) == int(sr_out):
        return Fraction(0)
    return Fraction(pair(sr_in, sr_out)[2], int(sr_in))


def stream_latency(core_samples, model_sr=MODEL_RATE, sr_in=None, sr_out=None, hold_samples=0):
    """``(seconds, samples)``: the latency bound of a stream whose conversion at the model rate waits at most
    ``core_samples`` and whose input / output are resampled from ``sr_in`` / to ``sr_out`` (None: the model rate).
    ``hold_samples``: what a stream with a message waits on top at the model rate, ``watermark_hold - 1`` (a sample
    leaves once its watermark block is whole; ``watermark.hold_wait``).
    ``seconds = taps_in / sr_in + (core_samples + hold_samples + taps_out) / model_sr`` (the output resampler waits
    ``taps_out`` model-rate samples), ``samples = ceil(seconds * output rate)``: ``core_samples + hold_samples`` itself
    when neither rate is given."""
    sec = latency_seconds(sr_in, model_sr) + Fraction(int(core_samples) + int(hold_samples), int(model_sr))
    if sr_out is not None and int(sr_out) != int(model_sr):
        sec += Fraction(pair(model_sr, sr_out)[2], int(model_sr))
    rate = int(model_sr) if sr_out is None else int(sr_out)
    return sec, math.ceil(sec * rate)


def owned_samples(samples, device):
    """``samples`` as a 1-D float32 tensor on ``device`` that shares no memory with the caller's object, so that it can
    wait in a ``ResamplerBank`` until the next step (a host array is copied to the device anyway; a device tensor is
    cloned)."""
    x = torch.as_tensor(samples, dtype=torch.float32).reshape(-1).to(device)
    if isinstance(samples, torch.Tensor) and x.numel() and x.data_ptr() == samples.data_ptr():
        x = x.clone()
    return x


class Schedule:
    """Host bookkeeping of one resampler (no device work): ``advance(n_new, end)`` takes ``n_new`` more input samples
    (``end``: the input is complete) and returns the record fields of the step, ``(base, end, n_total, t0, n_out)``: the
    kept window + new samples are input indices ``[base, end)``, ``n_total`` the input length once ended (-1 before),
    outputs ``t0 .. t0 + n_out - 1`` leave now.  Afterwards the window is kept from ``base`` (the first tap of the next
    output)."""

    def __init__(self, sr_in, sr_out):
        self.P, self.Q, self.taps = pair(sr_in, sr_out)
        self.received = 0           # input samples taken
        self.t = 0                  # next output
        self.base = 0               # first input index kept
        self.ended = False

    def ready_count(self, received):
        """Outputs whose right taps have all arrived after ``received`` input samples: t with (t Q) // P + taps <
        received, i.e. t < ceil((received - taps) P / Q)."""
        m = received - self.taps
        return 0 if m <= 0 else -(-m * self.P // self.Q)

    def final_count(self, received):
        """Outputs of an input of ``received`` samples: ``ceil(received P / Q)`` (librosa's fix=True length)."""
        return -(-received * self.P // self.Q)

    def advance(self, n_new, end=False):
        base, self.received = self.base, self.received + int(n_new)
        self.ended = self.ended or bool(end)
        stop = self.final_count(self.received) if self.ended else max(self.t, self.ready_count(self.received))
        t0, self.t = self.t, stop
        self.base = min(self.received, max(base, (stop * self.Q) // self.P - self.taps + 1))
        return base, self.received, self.received if self.ended else -1, t0, stop - t0


class _Resampler:
    def __init__(self, sr_in, sr_out, dev):
        self.sched = Schedule(sr_in, sr_out)
        self.pair = (int(sr_in), int(sr_out))
        self.win = torch.empty(0, dtype=torch.float32, device=dev)    # input [sched.base, sched.received)
        self.pending, self.n_pending = [], 0
        self.ending = False


class ResamplerBank:
    """The resamplers of many streams, one direction, stepped together (see the module docstring).  ``open(sr_in,
    sr_out)`` -> key; ``push(key, x)`` queues device samples; ``end(key)`` marks the end of the key's input; ``step()``
    -> ``{key: new output samples}`` (device tensors, views of one packed output) in ONE kernel launch for every key with
    new work, whatever its rate pair; an ended key is dropped once its last outputs are out."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._rs, self._next = {}, 0
        self._h, self._h_off = None, {}
        self.launches = 0

    def __contains__(self, key):
        return key in self._rs

    def __len__(self):
        return len(self._rs)

    def open(self, sr_in, sr_out):
        sr_in, sr_out = check_rate(sr_in, "sr_in"), check_rate(sr_out, "sr_out")
        if sr_in is None or sr_out is None or sr_in == sr_out:
            raise ValueError("a resampler needs two different rates")
        p = (sr_in, sr_out)
        if p not in self._h_off:                     # the phase tables of every pair in use, in one float64 tensor
            h = audio_io.device_phases(sr_in, sr_out, self.device)[0].reshape(-1)
            self._h_off[p] = 0 if self._h is None else self._h.numel()
            self._h = h if self._h is None else torch.cat([self._h, h])
        k = self._next
        self._next += 1
        self._rs[k] = _Resampler(sr_in, sr_out, self.device)
        return k

    def push(self, key, x):
        """Queue ``x`` (a 1-D float32 tensor on the bank's device); it is read by the next ``step()``, so it must not
        change before then (``owned_samples`` makes a caller's samples safe to queue)."""
        r = self._rs[key]
        if r.ending:
            raise RuntimeError("push() after end()")
        if x.numel():
            r.pending.append(x.reshape(-1))
            r.n_pending += x.numel()

    def end(self, key):
        self._rs[key].ending = True

    def final_count(self, key):
        """Output samples the key yields in all, once its queued input is its whole input."""
        r = self._rs[key]
        return r.sched.final_count(r.sched.received + r.n_pending)

    def emitted(self, key):
        return self._rs[key].sched.t

    def drop(self, key):
        self._rs.pop(key, None)

    def step(self):
        work = [(k, r) for k, r in self._rs.items() if r.n_pending or (r.ending and not r.sched.ended)]
        if not work:
            return {}
        pieces, recs, spans, src_acc, dst_acc, max_out = [], [], [], 0, 0, 0
        for k, r in work:
            n_new = r.n_pending
            pieces += [r.win] + r.pending
            win_off = src_acc
            src_acc += r.win.numel() + n_new
            base, end, n_total, t0, n_out = r.sched.advance(n_new, r.ending)
            spans.append((k, r, win_off, base, end, dst_acc, n_out))
            if n_out > 0:
                P, Q, taps = r.sched.P, r.sched.Q, r.sched.taps
                recs.append((win_off, base, end, n_total, t0, n_out, dst_acc, self._h_off[r.pair], P, Q, taps))
                max_out = max(max_out, n_out)
            dst_acc += n_out
            r.pending, r.n_pending = [], 0
        pieces = [p for p in pieces if p.numel()]
        # always a fresh tensor: the kept windows below are views of it, never of a caller's pushed tensor
        arena = torch.cat(pieces) if pieces else torch.zeros(1, dtype=torch.float32, device=self.device)
        out = torch.empty(max(dst_acc, 1), dtype=torch.float32, device=self.device)
        if recs:
            table = torch.tensor(recs, dtype=torch.int64).to(self.device)
            for i in range(0, len(recs), MAX_RECORDS):
                n = min(MAX_RECORDS, len(recs) - i)
                _lib.call("ov_polyphase_fir_rows_f32", table[i:i + n], n, arena, arena.numel(), self._h, self._h.numel(),
                          out, out.numel(), max_out)
                self.launches += 1
        res = {}
        for k, r, win_off, base, end, d0, n_out in spans:
            r.win = arena[win_off + r.sched.base - base:win_off + end - base]
            if n_out > 0:
                res[k] = out[d0:d0 + n_out]
            if r.sched.ended:
                del self._rs[k]
        return res


def resample_many(waves, pairs, device):
    """Whole waveforms (1-D float32 device tensors), ``pairs[i] = (sr_in, sr_out)`` (equal rates or None: passed
    through) -> the resampled waveforms, every one equal to ``audio_io.resample_on_device`` of it, in ONE launch."""
    bank, keys, outs = ResamplerBank(device), {}, list(waves)
    for i, (x, (a, b)) in enumerate(zip(waves, pairs)):
        if a is None or b is None or int(a) == int(b) or x.numel() == 0:
            continue
        keys[i] = bank.open(a, b)
        bank.push(keys[i], x.to(device, torch.float32))
        bank.end(keys[i])
    res = bank.step()
    for i, k in keys.items():
        outs[i] = res.get(k, torch.empty(0, dtype=torch.float32, device=device))
    return outs


class StreamResampler:
    """One stream's resampler (a bank of one): ``push(x)`` -> new output samples, ``close(x=None)`` -> the rest."""

    def __init__(self, sr_in, sr_out, device):
        self.bank = ResamplerBank(device)
        self.key = self.bank.open(sr_in, sr_out)

    def _take(self):
        return self.bank.step().get(self.key, torch.empty(0, dtype=torch.float32, device=self.bank.device))

    def push(self, x):
        self.bank.push(self.key, x)
        return self._take()

    def final_count(self):
        return self.bank.final_count(self.key)

    def close(self, x=None):
        """The last input ``x`` (or none) and the end: the remaining outputs, in one launch."""
        if x is not None:
            self.bank.push(self.key, x)
        self.bank.end(self.key)
        return self._take()
