"""What ``longform.StreamPool`` and ``live.LivePool`` do to a pushed stream before and after their conversion launches:
the growing waveform buffer (``WaveBuffer``) and the handle table with its per-stream resamplers (``PushedPool``).
Nothing here knows of windows, units, rounds or noise.  A stream object brings ``wave`` (its ``WaveBuffer``), ``closed``
and ``tau``, and ``mark`` when it was opened with a message (``watermark.stream_mark``'s answer); ``_register`` gives it
``sr_in`` / ``sr_out``, its resampler keys ``rin`` / ``rout`` (None: the model rate) and, with a ``mark``, its place in
the pool's ``watermark.MarkBank``."""
import torch

from . import _lib, rates
from . import watermark as watermark_mod
from .engine import item_tau


class WaveBuffer:
    """The buffered tail of one pushed waveform."""

    def __init__(self, device):
        self.buf = torch.empty(0, dtype=torch.float32, device=device)
        self.len = 0                # valid samples in buf
        self.base = 0               # file index of buf[0]; a multiple of hop
        self.n = 0                  # samples received

    def append(self, x):
        n = x.numel()
        if self.len + n > self.buf.numel():            # grow geometrically: pushes of one sample stay O(1) amortised
            grown = torch.empty(max(2 * self.buf.numel(), self.len + n, 1 << 16), dtype=torch.float32,
                                device=self.buf.device)
            grown[:self.len].copy_(self.buf[:self.len])
            self.buf = grown
        self.buf[self.len:self.len + n].copy_(x)
        self.len += n
        self.n += n

    def trim(self, keep_from_frame, hop, pad):
        """Drop samples no frame from ``keep_from_frame`` on reads (whole hops, kept from before the reflect padding)."""
        base = max(0, keep_from_frame * hop - -(-pad // hop) * hop)
        if base > self.base:
            keep = self.buf[base - self.base:self.len].clone()
            self.buf, self.len, self.base = keep, keep.numel(), base

    def valid(self):
        return self.buf[:self.len]

    def release(self):
        self.buf, self.len = self.buf[:0], 0


class PushedPool:
    """Base of the pools of pushed streams: handles, pushes, the end of a stream's input, retiring, and the two
    ``rates.ResamplerBank`` s that bring every stream's input to the model rate and its output to its own in one launch
    each per ``step()``."""

    def _init_streams(self, device, model_sr):
        self.model_sr = int(model_sr)
        self._streams, self._retired, self._next = {}, set(), 0       # handle -> stream, in handle order
        self._rin, self._rout = rates.ResamplerBank(device), rates.ResamplerBank(device)
        self._rin_owner = {}        # input resampler key -> stream
        self._rout_ending = []      # output resampler keys of streams that finished in this step
        # streams opened with message=: their block-wise watermark (watermark.MarkBank), made on first use
        self._mark, self._mark_keys, self._mark_ending = None, {}, []       # handle -> mark key; keys ending this step

    @property
    def active(self):
        """Handles of the streams not yet retired (open, or closed with their tail still to run)."""
        return list(self._streams)

    def _stream(self, h):
        st = self._streams.get(h)
        if st is None:
            raise RuntimeError(f"stream {h!r} is closed" if h in self._retired else f"no stream {h!r} in this pool")
        return st

    def _stream_tau(self, tau, who):
        """``tau`` of a new stream: None = the pool's, else this stream's own number."""
        tau = self.tau if tau is None else item_tau(1, tau)
        if not isinstance(tau, float):
            raise _lib.OvError(f"{who}: tau is one number per stream")
        return tau

    def _register(self, st, sr_in, sr_out):
        """The last step of ``open``, after everything that can raise: ``st``'s resampler keys and its handle."""
        st.sr_in, st.sr_out, st.rin, st.rout = sr_in, sr_out, None, None
        mark = getattr(st, "mark", None)        # watermark.stream_mark's answer, checked by open() before this
        if sr_in is not None and sr_in != self.model_sr:
            st.rin = self._rin.open(sr_in, self.model_sr)
            self._rin_owner[st.rin] = st
        if sr_out is not None and sr_out != self.model_sr:
            st.rout = self._rout.open(self.model_sr, sr_out)
        h = self._next
        self._next += 1
        self._streams[h] = st
        if mark is not None:
            if self._mark is None:
                self._mark = watermark_mod.MarkBank(self._rin.device)
            self._mark_keys[h] = self._mark.open(mark)
        return h

    def _hold_wait(self):
        """The longest wait a message adds to a stream open in this pool, in model-rate samples (``H - 1``)."""
        return max((watermark_mod.hold_wait(getattr(st, "mark", None)) for st in self._streams.values()), default=0)

    @torch.no_grad()
    def push(self, h, samples):
        st = self._stream(h)
        if st.closed:
            raise RuntimeError(f"push() after close() on stream {h!r}")
        if st.rin is not None:                  # resampled to the model rate by the next step()
            self._rin.push(st.rin, rates.owned_samples(samples, self._rin.device))
        else:
            st.wave.append(torch.as_tensor(samples, dtype=torch.float32).reshape(-1).to(self._rin.device))

    def _end_input(self, h):
        """Marks the end of h's input -> its length at the model rate."""
        st = self._stream(h)
        if st.closed:
            raise RuntimeError(f"close() called twice on stream {h!r}")
        st.closed = True
        n = st.wave.n
        if st.rin is not None:                  # the model-rate samples the input resampler has still to deliver
            n += self._rin.final_count(st.rin) - self._rin.emitted(st.rin)
            self._rin.end(st.rin)
        return n

    def _retire(self, h, finished=False):
        """``finished``: h ran to its end, so its output resampler (if any) still delivers its tail in this step."""
        st = self._streams.pop(h)
        st.wave.release()
        self._retired.add(h)
        if st.rin is not None:
            self._rin.drop(st.rin)
            self._rin_owner.pop(st.rin, None)
        if st.rout is not None:
            if finished:
                self._rout_ending.append(st.rout)     # ended after this step's last output is queued
            else:
                self._rout.drop(st.rout)
        if h in self._mark_keys:
            if finished:
                self._mark_ending.append(self._mark_keys[h])      # flushed by this step's _deliver
            else:
                self._mark.drop(self._mark_keys.pop(h))
        self._released(st)

    def _released(self, st):
        pass

    def _take_input(self):
        """First in a ``step()``: the new input of the resampled streams, at the model rate (one launch)."""
        for key, y in self._rin.step().items():
            self._rin_owner[key].wave.append(y)

    def _output_rates(self):
        """``{handle: output resampler key}``, taken before a step's launches: streams retire during them."""
        return {h: st.rout for h, st in self._streams.items() if st.rout is not None}

    def _deliver(self, outs, routs):
        """Last in a ``step()``: ``outs`` with the output of the streams that carry a message marked (one launch, at
        the model rate; a sample leaves once its block is whole, a finished stream's rest at once), then with the output
        of the streams in ``routs`` at their own rates (one launch).  A pool without a marked stream runs no mark code."""
        if self._mark_keys:
            for h, key in self._mark_keys.items():
                if h in outs:
                    self._mark.push(key, outs.pop(h))
            for key in self._mark_ending:
                self._mark.end(key)
            ys = self._mark.step()
            outs.update({h: ys[key] for h, key in self._mark_keys.items() if key in ys})
            if self._mark_ending:
                self._mark_keys = {h: k for h, k in self._mark_keys.items() if k not in self._mark_ending}
                self._mark_ending = []
        if routs:
            for h, key in routs.items():
                if h in outs:
                    self._rout.push(key, outs.pop(h))
            for key in self._rout_ending:
                self._rout.end(key)
            self._rout_ending.clear()
            ys = self._rout.step()
            outs.update({h: ys[key] for h, key in routs.items() if key in ys})
        return outs
