"""What every live-stream batch shares (DESIGN.md "Stream batches"): the two ping-ponged device records, the reset requests that wait
for a stream's next active tick, the bool-mask arguments, save / restore, and the head and tail of a tick.  A model's class keeps its
record layout, its constructor checks and the body of `step`."""
from __future__ import annotations

import numpy as np

from .clips import flag_timestamps


class StreamBatch:
    """`streams` live streams whose whole state is a device record of `record_bytes` bytes (uint8, all-zero = fresh streams).  A tick reads
    `record` and writes the other of the two tensors, then they swap: the record just read is never written.  The contract -- when a
    reset applies, what an inactive stream keeps, save and restore -- is stated once, in DESIGN.md "Stream batches".

    One inconsistency is public and stays: `stream_bytes` is `(record, s)` in FSMN, FireRed and DFSMN, `(s, record=None)` in MarbleNet."""

    def __init__(self, engine, streams, record_bytes):
        self.engine, self.streams = engine, int(streams)
        if self.streams <= 0:
            raise ValueError(f"streams={streams} must be positive")
        t = engine.torch
        self._rec = [t.zeros(record_bytes, dtype=t.uint8, device=engine.device) for _ in range(2)]
        self._cur = 0
        self._pending = np.zeros(self.streams, dtype=bool)       # reset_states() requests not yet applied to an active tick
        self._everyone = np.ones(self.streams, dtype=bool)       # `act` of a tick without an `active` mask (never written)

    @property
    def record(self):
        """The current device record (uint8); the class docstring of the model gives its layout."""
        return self._rec[self._cur]

    def load_record(self, record):
        """Continue from a saved copy of `record` (uint8, numpy or torch, of a batch built with the same arguments): the bytes are copied
        into the current record and pending reset requests are dropped."""
        t = self.engine.torch
        r = record if t.is_tensor(record) else t.from_numpy(np.ascontiguousarray(record))
        if r.dtype != t.uint8 or r.numel() != self.record.numel():
            raise ValueError(f"record must be uint8 [{self.record.numel()}], got {r.dtype} [{r.numel()}]")
        self.record.copy_(r.reshape(-1))
        self._pending[:] = False
        self._record_loaded()

    def _record_loaded(self):
        """Hook of load_record: a class that mirrors words of the record on the host re-reads them here."""

    def reset_states(self, streams=None):
        """None = every stream; else stream indices or a bool mask of any shape that flattens to [S] (so [S, 1] is taken, by every model).
        Applies at the next tick in which the stream is active."""
        if streams is None:
            self._pending[:] = True
            return
        idx = np.asarray(streams.cpu() if hasattr(streams, "cpu") else streams)
        if idx.dtype == bool:
            self._pending |= self._mask(idx, "reset mask")
        else:
            self._pending[idx.astype(np.int64).reshape(-1)] = True

    def _mask(self, m, name):
        a = np.asarray(m.cpu() if hasattr(m, "cpu") else m).astype(bool).reshape(-1)
        if a.shape != (self.streams,):
            raise ValueError(f"{name} must have shape ({self.streams},), got {a.shape}")
        return a

    def _samples(self, x, want=None, bad=None, floats=False, where=""):
        """A tick's samples (host or device, numpy or torch) as a tensor where they are: int16 (floats=True: or floating point, taken as
        float32) of shape [S, n] for which `bad(x)` is false.  `want` and `where` word the refusal."""
        t = self.engine.torch
        if not t.is_tensor(x):
            x = t.from_numpy(np.ascontiguousarray(x))
        if x.dtype != t.int16:
            if not (floats and x.is_floating_point()):
                raise ValueError(f"samples must be {'float32 or ' if floats else ''}int16, got {x.dtype}")
            x = x.to(t.float32)
        if x.dim() != 2 or x.shape[0] != self.streams or (bad is not None and bad(x)):
            raise ValueError(f"samples must be {want or f'[{self.streams}, n]'}, got {tuple(x.shape)}{where}")
        return x

    def _begin(self, reset=None, active=None, upload_active=True):
        """The head of a tick with `reset` / `active` masks (bool [S] or None) -> (act, req, reset_d, act_d, src, dst): the active streams
        and the resets this tick applies (host bool [S]: a pending or explicit request of an ACTIVE stream), their uint8 copies on the
        device -- reset_d None when no request applies, act_d None when `active` is None or not wanted -- and the records to read and write."""
        req = self._pending | self._mask(reset, "reset") if reset is not None else self._pending.copy()
        if active is None:
            act = self._everyone
        else:
            act = self._mask(active, "active")
            req &= act
        t, dev = self.engine.torch, self.engine.device
        reset_d = t.from_numpy(req.astype(np.uint8)).to(dev) if np.count_nonzero(req) else None      # (a fifth of the time of req.any())
        act_d = t.from_numpy(act.astype(np.uint8)).to(dev) if upload_active and active is not None else None
        return act, req, reset_d, act_d, self._rec[self._cur], self._rec[1 - self._cur]

    def _end(self, act):
        """The tail of that tick: the record written becomes the current one; the requests of the active streams have been applied."""
        self._cur = 1 - self._cur
        if act is self._everyone:                # (what the line below comes to, without its two temporaries)
            self._pending[:] = False
        else:
            self._pending &= ~act


class WindowStreamBatch(StreamBatch):
    """Streams cut into overlapping analysis windows of engine.L samples, `self.stride` apart, whose flags last `self.frame_s` seconds
    (FSMN, DFSMN): a stream's first tick, and its first after a reset, takes a whole window, every other one only the new strides.  The
    host mirrors the record's "has a carry" word in `_primed`; a class says where that word is in `_primed_words`."""

    def __init__(self, engine, streams, record_bytes):
        super().__init__(engine, streams, record_bytes)
        self._primed = np.zeros(self.streams, dtype=bool)

    def _record_loaded(self):
        self._primed = self._primed_words().cpu().numpy() != 0

    def samples_needed(self, windows, reset=None):
        """int64 [S]: new samples (per channel) each stream consumes in the next tick of `windows` windows: windows * stride with a
        carry, L + (windows - 1) * stride without one (first tick, or reset -- requested here or pending from reset_states)."""
        k = int(windows)
        if k < 1:
            raise ValueError(f"windows={windows} must be at least 1")
        fresh = ~self._primed | self._pending | (False if reset is None else self._mask(reset, "reset"))
        return np.where(fresh, self.engine.L + (k - 1) * self.stride, k * self.stride).astype(np.int64)

    def samples_needed_ragged(self, counts, reset=None):
        """int64 [S]: new samples each stream consumes in the next RAGGED tick of counts[s] windows: 0 for a count of 0, n * stride with
        a carry, L + (n - 1) * stride without one.  A pending or requested reset makes a stream one without a carry only when its count
        is above 0 (a stream without audio keeps its record and its pending reset)."""
        from . import ragged
        c = ragged.stream_counts(counts, self.streams).astype(np.int64)
        fresh = ~self._primed | self._pending | (False if reset is None else self._mask(reset, "reset"))
        return np.where(c == 0, 0, np.where(fresh, self.engine.L + (c - 1) * self.stride, c * self.stride)).astype(np.int64)

    def _counts_of_lengths(self, lengths, reset=None):
        """The counts for which samples_needed_ragged gives `lengths` (new samples per stream), or ValueError naming the first stream
        whose length is off its grid."""
        n = np.asarray(lengths, dtype=np.int64)
        fresh = ~self._primed | self._pending | (False if reset is None else self._mask(reset, "reset"))
        L, st = self.engine.L, self.stride
        c = np.where(n == 0, 0, np.where(fresh, (n - L) // st + 1, n // st))
        ok = (n == 0) | np.where(fresh, (n >= L) & ((n - L) % st == 0), n % st == 0)
        if not ok.all():
            s = int(np.flatnonzero(~ok)[0])
            want = f"{L} + m * {st} (no carry yet, or a reset)" if fresh[s] else f"a multiple of {st}"
            raise ValueError(f"samples[{s}] holds {int(n[s])} samples: stream {s} takes 0 or {want} (samples_needed_ragged)")
        return c.astype(np.int64)

    def _end(self, act):
        super()._end(act)
        self._primed |= act

    def timestamps(self, flags_so_far, tail, fusion_threshold=0.3, min_speech_duration=0.2):
        """One stream's accumulated flags (1-D, every tick so far) + the last tick's tail -> [(start_s, end_s)], the reference's
        vad_to_timestamps + process_timestamps over its `saved` list."""
        f = np.concatenate([np.asarray(a.cpu() if hasattr(a, "cpu") else a).reshape(-1) for a in (flags_so_far, tail)])
        return flag_timestamps(f, self.frame_s, fusion_threshold, min_speech_duration)
