"""Timestamps on the device: per-frame decisions or a segment table of a resident batch -> a TimestampTable, seconds and sample rows
for every clip, without the flags, tracks or tables crossing to the host (csrc/timestamps.hip, include/vadx.h "Timestamps").

Three sources, each the device form of host code the `detect` calls run per clip, bit for bit:
    from_flags    FSMN / DFSMN silence flags: `clips.flag_timestamps` = vad_to_timestamps + process_timestamps;
    from_frames   the frame table of vadx_vadpost: `VadPostprocessor.segments_to_seconds` (float32 products, Python round(, 3));
    from_samples  the sample table of vadx_silero_segments: the return_seconds branch of get_speech_timestamps (round(x / sr, 1))
                  and, when asked for, the process_timestamps pass of the Silero driver.
The table's `samples` rows are what `vadx.chunks.collect_chunks_batch` / `drop_chunks_batch` take as a device table (`chunks_table()`).
`round3_host`, `round1_host`, `fuse_host` and `flags_host` state the device rules on the host, as `chunks.plan_host` does for the plan.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

NEAREST, TRUNC = 0, 1                                    # VADX_TS_NEAREST / VADX_TS_TRUNC
ST_BAD_CLIP, ST_OVERFLOW = 1, 2                          # VADX_TS_ST_*
_STATUS_TEXT = {ST_BAD_CLIP: "a clip's frame / row count or length lies outside its table (that clip's count is 0)",
                ST_OVERFLOW: "a clip has more segments than the table's cap (rows beyond cap were not written)"}
_RULES = {"nearest": NEAREST, "trunc": TRUNC, NEAREST: NEAREST, TRUNC: TRUNC}


# ---- the device rules on the host ---------------------------------------------------------------------------------------------------
def round3_host(x):
    """Python's round(x, 3) for float32-valued x, as the device computes it: x * 1000.0 is exact in double (24 + 10 bits), so the
    nearest integer (ties to even) over 1000.0 is the correctly rounded decimal.  -> float64 array."""
    return np.rint(np.asarray(x, dtype=np.float32).astype(np.float64) * 1000.0) / 1000.0


def round1_host(x, sampling_rate):
    """Python's round(x / sampling_rate, 1) for integer sample indices x (|x| < 2^53), sampling_rate 16000 or 8000, as the device
    computes it.  step = sr / 10; (m, r) = divmod(|x|, step): off a tie, m + (r > step / 2) tenths; on one, the double q = x / sr lies
    above, below or on the decimal tie -- the sign of the exact residual q * sr - x says which; on it, the even tenth.  -> float64 array."""
    sr = int(sampling_rate)
    if sr not in (16000, 8000):
        raise ValueError(f"sampling_rate={sampling_rate} must be 16000 or 8000")
    x = np.asarray(x, dtype=np.int64)
    ax = np.abs(x)
    step, half = sr // 10, sr // 20
    m, r = np.divmod(ax, step)
    k = m + (r > half)
    for i in np.flatnonzero((r == half).reshape(-1)).tolist():
        xi, mi = int(ax.reshape(-1)[i]), int(m.reshape(-1)[i])
        num, den = (xi / sr).as_integer_ratio()           # the double quotient, exactly
        res = num * sr - xi * den                         # sign of q * sr - x
        k.reshape(-1)[i] = mi + 1 if res > 0 else (mi if res < 0 else mi + (mi & 1))
    return np.where(x < 0, -1.0, 1.0) * (k.astype(np.float64) / 10.0)


def fuse_host(rows, fusion_threshold, min_duration):
    """process_timestamps as the device runs it: keep (e - s) >= min_duration; a kept row opens a segment when there is none before it or
    not (s - previous kept end <= fusion_threshold), and extends the open one otherwise.  ONE pass: the reference's second pass compares
    the same numbers across every boundary the first left."""
    out = []
    prev = None
    for s, e in rows:
        if not (e - s) >= min_duration:
            continue
        if prev is not None and (s - prev) <= fusion_threshold:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
        prev = e
    return out


def flags_host(flags, frame_s, fusion_threshold, min_duration):
    """One clip's silence flags -> [(start_s, end_s)] by the device's rule: speech is flag == 0; the positions 0 .. n inclusive are
    walked with position n silent, a run [a, b) gives (a * fd, n * fd if b == n else b * fd + fd); then `fuse_host`."""
    f = np.asarray(flags).reshape(-1)
    n = int(f.shape[0])
    speech = np.concatenate(([False], f == 0, [False]))
    edges = np.flatnonzero(speech[1:] != speech[:-1]).tolist()
    rows = [(a * frame_s, n * frame_s if b == n else b * frame_s + frame_s) for a, b in zip(edges[0::2], edges[1::2])]
    return fuse_host(rows, fusion_threshold, min_duration)


def samples_host(rows, sampling_rate, sample_rule=NEAREST):
    """(start_s, end_s) rows -> sample rows by the table's rule: NEAREST int(round(s * sr)) (`chunks.from_seconds`), TRUNC int(s * sr)
    (`timestamps.indices`)."""
    sr = float(sampling_rate)
    if _RULES[sample_rule] == NEAREST:
        return [(int(round(s * sr)), int(round(e * sr))) for s, e in rows]
    return [(int(s * sr), int(e * sr)) for s, e in rows]


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def table_bytes(batch, cap):
    """Bytes of one table's storage: the 16-byte head, seconds f64 [B, cap, 2], samples int64 [B, cap, 2], counts int32 [B]."""
    return (16 + 32 * int(batch) * int(cap) + 4 * int(batch) + 15) // 16 * 16


class TimestampTable:
    """The timestamps of one batch on the device; nothing synchronises except `head()`, `check()` and `lists()`.
        seconds   f64   [B, cap, 2] device: (start_s, end_s)
        samples   int64 [B, cap, 2] device: the same rows in samples (NEAREST or TRUNC, as asked for)
        counts    int32 [B] device: the true number of segments of every clip (> cap: rows beyond cap were not written)
    `storage`: a uint8 device tensor of at least table_bytes(batch, cap) bytes, 16-byte aligned, to build the table in."""

    def __init__(self, batch, cap, device, sampling_rate, sample_rule=NEAREST, dicts=False, storage=None):
        t = _lib.require_gpu()
        self.batch, self.cap, self.device = int(batch), int(cap), t.device(device)
        self.sampling_rate, self.sample_rule, self.dicts = int(sampling_rate), _RULES[sample_rule], bool(dicts)
        if self.batch < 1 or self.cap < 1:
            raise ValueError(f"a table needs batch >= 1 and cap >= 1, got {batch} and {cap}")
        need = table_bytes(self.batch, self.cap)
        if storage is None:
            storage = t.empty(need, dtype=t.uint8, device=self.device)
        elif storage.dtype != t.uint8 or storage.dim() != 1 or storage.numel() < need or storage.data_ptr() % 16 or not storage.is_contiguous():
            raise ValueError(f"storage must be a contiguous 16-byte aligned uint8 vector of at least {need} bytes")
        self.storage = storage
        rows = 16 * self.batch * self.cap
        self._head_t = storage[:16].view(t.int32)
        self.seconds = storage[16:16 + rows].view(t.float64).reshape(self.batch, self.cap, 2)
        self.samples = storage[16 + rows:16 + 2 * rows].view(t.int64).reshape(self.batch, self.cap, 2)
        self.counts = storage[16 + 2 * rows:16 + 2 * rows + 4 * self.batch].view(t.int32)
        self._head = None

    def _outs(self):
        return (self.seconds.data_ptr(), self.samples.data_ptr(), self.counts.data_ptr(), self.cap, self._head_t.data_ptr(), _lib.stream_ptr())

    def head(self):
        """(status, largest count): one 16-byte read (synchronises); remembered."""
        if self._head is None:
            h = self._head_t.cpu().numpy()
            self._head = (int(h[0]), int(h[1]))
        return self._head

    def check(self):
        """Raise VadxError when a status bit is set (reads the head)."""
        status = self.head()[0]
        if status:
            raise _lib.VadxError("timestamps: " + "; ".join(text for bit, text in _STATUS_TEXT.items() if status & bit))
        return self

    def lists(self):
        """Per clip [(start_s, end_s)] of Python floats -- [{'start', 'end'}] for a Silero table -- from ONE read-back of the counts and the
        used columns of `seconds` (after the head, which a constructor that retried has read already).  Raises for a status bit."""
        t = _lib.require_gpu()
        self.check()
        m = min(self.head()[1], self.cap)
        packed = t.cat([self.counts.to(t.float64).unsqueeze(1), self.seconds[:, :m].reshape(self.batch, 2 * m)], dim=1).cpu().numpy()
        out = []
        for row in packed.tolist():
            c = int(row[0])
            if self.dicts:
                out.append([{"start": row[1 + 2 * k], "end": row[2 + 2 * k]} for k in range(c)])
            else:
                out.append([(row[1 + 2 * k], row[2 + 2 * k]) for k in range(c)])
        return out

    def chunks_table(self):
        """(samples int64 [B, cap, 2], counts int32 [B]) on the device: what collect_chunks_batch / drop_chunks_batch take as `tss`."""
        return self.samples, self.counts


def _build(launch, batch, cap, device, sampling_rate, sample_rule, dicts, storage, retry):
    """Run `launch(table)` into a table of `cap` rows per clip; with retry, read the head once and, when some clip has more segments,
    run once more with cap = the largest count."""
    tab = TimestampTable(batch, cap, device, sampling_rate, sample_rule, dicts, storage)
    launch(tab)
    if retry:
        status, most = tab.head()
        if most > tab.cap:
            tab = TimestampTable(batch, most, device, sampling_rate, sample_rule, dicts)
            launch(tab)
            tab._head = (status & ~ST_OVERFLOW, most)          # the same clips are refused, and now every one fits
    return tab


def _params(sampling_rate, sample_rule, fusion_threshold, min_duration, **kw):
    if (fusion_threshold is None) != (min_duration is None):
        raise ValueError("fusion_threshold and min_duration go together (both None: no process_timestamps pass)")
    process = fusion_threshold is not None
    return _lib.TsParams(frame_s=kw.get("frame_s", 0.0), fusion_threshold=float(fusion_threshold) if process else 0.0,
                         min_duration=float(min_duration) if process else 0.0, frame_shift=kw.get("frame_shift", 0.0),
                         frame_length=kw.get("frame_length", 0.0), use_frame_length=kw.get("use_frame_length", 0),
                         sampling_rate=int(sampling_rate), process=int(process), sample_rule=_RULES[sample_rule])


def _i32(v, n, device, what, fill=None):
    """`v` (device tensor, host array, or None = `fill` for every clip) as int32 [n] on the device"""
    t = _lib.require_gpu()
    if v is None:
        return t.full((n,), int(fill), dtype=t.int32, device=device)
    v = v.to(device=device, dtype=t.int32) if t.is_tensor(v) else t.from_numpy(np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int32)).to(device)
    v = v.reshape(-1).contiguous()
    if v.shape[0] != n:
        raise ValueError(f"{what} must have one entry per clip ({n}), got {v.shape[0]}")
    return v


def from_flags(flags, n_flags, frame_s, fusion_threshold, min_duration, sampling_rate=16000, sample_rule=NEAREST, cap=64, retry=True,
               storage=None):
    """Silence flags uint8 [B, S] on the device (what FsmnEngine.flags / flags_ragged and the DFSMN vote write; n_flags [B] valid per
    row, None = S) -> TimestampTable: `clips.flag_timestamps` of every row, one launch.  fusion_threshold = min_duration = None skips
    process_timestamps.  A clip with more than `cap` segments: retry=True reads the head and runs once more with the largest count."""
    t = _lib.require_gpu()
    if not t.is_tensor(flags) or not flags.is_cuda or flags.dtype != t.uint8 or flags.dim() != 2 or flags.shape[0] < 1:
        raise ValueError("flags must be a uint8 device tensor [B, S] with B >= 1")
    if flags.shape[1] and flags.stride(1) != 1:
        flags = flags.contiguous()
    B, S = int(flags.shape[0]), int(flags.shape[1])
    stride = int(flags.stride(0)) if S else 0
    src = flags if S else t.zeros(16, dtype=t.uint8, device=flags.device)         # an empty tensor has no address; nothing of it is read
    nf = _i32(n_flags, B, flags.device, "n_flags", S)
    prm = _params(sampling_rate, sample_rule, fusion_threshold, min_duration, frame_s=float(frame_s))

    def launch(tab):
        with t.cuda.device(flags.device):
            _lib.check(_lib.lib().vadx_timestamps_flags(C.byref(prm), src.data_ptr(), stride, nf.data_ptr(), B, *tab._outs()))
    return _build(launch, B, cap, flags.device, sampling_rate, sample_rule, False, storage, retry)


def from_frames(pp, segs, counts, n_frames, durations_s, sampling_rate=16000, sample_rule=NEAREST, fusion_threshold=None, min_duration=None,
                cap=None, retry=True, storage=None):
    """The frame table of `pp.process_batch` (segs int32 [B, cap_in, 2], counts int32 [B], on the device) -> TimestampTable:
    `pp.segments_to_seconds(rows_b, n_frames[b], durations_s[b])` of every clip, one launch.  n_frames [B] (None: not allowed here, the
    table does not know the track's width); durations_s [B] seconds, None entries (or None for all) = no cap by the duration.
    cap defaults to cap_in, which always fits; a smaller one retries once with the head's largest count."""
    t = _lib.require_gpu()
    if not t.is_tensor(segs) or not segs.is_cuda or segs.dtype != t.int32 or segs.dim() != 3 or segs.shape[2] != 2 or segs.shape[0] < 1 or segs.shape[1] < 1:
        raise ValueError("segs must be an int32 device tensor [B, cap_in, 2] with B, cap_in >= 1")
    if n_frames is None:
        raise ValueError("n_frames is needed: the valid frames of every clip's track")
    dev, B, cap_in = segs.device, int(segs.shape[0]), int(segs.shape[1])
    segs = segs.contiguous()
    cnt, nf = _i32(counts, B, dev, "counts"), _i32(n_frames, B, dev, "n_frames")
    dur = np.full((B,), np.nan) if durations_s is None else np.asarray([np.nan if d is None else float(d) for d in durations_s], dtype=np.float64)
    if dur.shape != (B,):
        raise ValueError(f"durations_s must have one entry per clip ({B})")
    dur = t.from_numpy(dur).to(dev)
    prm = _params(sampling_rate, sample_rule, fusion_threshold, min_duration, frame_shift=float(pp.frame_shift),
                  frame_length=0.0 if pp.frame_length is None else float(pp.frame_length), use_frame_length=int(pp.frame_length is not None))

    def launch(tab):
        with t.cuda.device(dev):
            _lib.check(_lib.lib().vadx_timestamps_frames(C.byref(prm), segs.data_ptr(), cnt.data_ptr(), cap_in, nf.data_ptr(), dur.data_ptr(), B,
                                                         *tab._outs()))
    return _build(launch, B, cap_in if cap is None else cap, dev, sampling_rate, sample_rule, False, storage, retry)


def from_samples(segs, counts, lengths, sampling_rate=16000, fusion_threshold=None, min_duration=None, time_resolution=1, sample_rule=NEAREST,
                 cap=None, retry=True, storage=None):
    """The sample table of SileroEngine.segments (segs int64 [B, cap_in, 2], counts int32 [B], on the device; lengths [B] in samples)
    -> TimestampTable whose `lists()` are the {'start', 'end'} dicts of get_speech_timestamps_batch(return_seconds=True), and with
    fusion_threshold / min_duration the process_timestamps pass of the Silero driver over them.  Only time_resolution = 1."""
    t = _lib.require_gpu()
    if time_resolution != 1:
        raise ValueError(f"time_resolution={time_resolution}: the device table rounds to one decimal (time_resolution=1) only")
    if not t.is_tensor(segs) or not segs.is_cuda or segs.dtype != t.int64 or segs.dim() != 3 or segs.shape[2] != 2 or segs.shape[0] < 1 or segs.shape[1] < 1:
        raise ValueError("segs must be an int64 device tensor [B, cap_in, 2] with B, cap_in >= 1")
    dev, B, cap_in = segs.device, int(segs.shape[0]), int(segs.shape[1])
    segs = segs.contiguous()
    cnt = _i32(counts, B, dev, "counts")
    lens = (lengths if t.is_tensor(lengths) else t.from_numpy(np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int64)))
    lens = lens.to(device=dev, dtype=t.int64).reshape(-1).contiguous()
    if lens.shape[0] != B:
        raise ValueError(f"lengths must have one entry per clip ({B})")
    prm = _params(sampling_rate, sample_rule, fusion_threshold, min_duration)

    def launch(tab):
        with t.cuda.device(dev):
            _lib.check(_lib.lib().vadx_timestamps_samples(C.byref(prm), segs.data_ptr(), cnt.data_ptr(), cap_in, lens.data_ptr(), B, *tab._outs()))
    return _build(launch, B, cap_in if cap is None else cap, dev, sampling_rate, sample_rule, True, storage, retry)


def empty(batch, device, sampling_rate=16000, dicts=False):
    """A table in which no clip has a segment (what empty audio gives)."""
    tab = TimestampTable(batch, 1, device, sampling_rate, NEAREST, dicts)
    tab.storage.zero_()
    tab._head = (0, 0)
    return tab
