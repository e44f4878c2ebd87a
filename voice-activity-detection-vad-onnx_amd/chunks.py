"""Cut the speech out of a resident batch -- or drop it -- on the device: the batched form of the reference's `collect_chunks` and
`drop_chunks` (Silero/modeling_modified/utils_vad.py:588-631 / 634-682), and those two functions themselves as single-clip drop-ins.

A *piece* is a half-open source interval of one clip, resolved by exactly Python's slice rule (an index i < 0 becomes i + len, it is then
clamped to [0, len], lo >= hi is empty).  From the n = counts[b] table rows (start_k, end_k) of clip b:
    collect   n pieces:      wav[start_k : end_k]
    drop      n + 1 pieces:  wav[cur_k : start_k] with cur_0 = 0, cur_k = end_{k-1}; the last piece is wav[cur_n :]
Rows may overlap, be unsorted, reversed or out of range: they give what the reference's slicing gives.

The output is a packed vector in the layout of `vadx.ragged`: clip after clip, each starting on a multiple of `align` elements (align = 8
for int16 = a 16-byte boundary), filler written as zeros -- so it can be fed straight back to the ragged entry points of the other models.
Two steps on the device (csrc/chunks.hip, include/vadx.h "Chunks"): `vadx_chunks_plan` turns the table into a PLAN record (resolved
intervals, the prefix of the piece lengths inside each clip, the prefix of the clips' output lengths, the total, a status word), and
`vadx_chunks_copy` fills the output over 16 KB destination tiles.  `plan_host` is the host mirror of the plan arithmetic.
"""
from __future__ import annotations

import numpy as np

from . import _lib

COLLECT, DROP = 0, 1                                     # VADX_CHUNKS_COLLECT / VADX_CHUNKS_DROP
ST_BAD_CLIP, ST_OVERFLOW, ST_SRC_RANGE = 1, 2, 4         # VADX_CHUNKS_ST_*
_STATUS_TEXT = {ST_BAD_CLIP: "a clip's segment count lies outside [0, cap] or its length is negative (that clip's output is empty)",
                ST_OVERFLOW: "the packed output does not fit `out`: nothing was written",
                ST_SRC_RANGE: "a piece lies outside the audio buffer (clip_offsets / lengths do not describe it): those samples are zeros"}
_MODES = {"collect": COLLECT, "drop": DROP, COLLECT: COLLECT, DROP: DROP}


def plan_layout(batch, cap):
    """Byte offsets of the plan record of (batch, cap) -- include/vadx.h, "Chunks": total int64 at 0, status int32 at 8, then clip_dst
    int64 [B+1], piece_dst int64 [B][cap+2], piece_src int64 [B][cap+1][2], n_pieces int32 [B]; `bytes` = vadx_chunks_plan_bytes."""
    batch, cap = int(batch), int(cap)
    clip_dst = 16
    piece_dst = clip_dst + 8 * (batch + 1)
    piece_src = piece_dst + 8 * batch * (cap + 2)
    n_pieces = piece_src + 16 * batch * (cap + 1)
    return dict(total=0, status=8, clip_dst=clip_dst, piece_dst=piece_dst, piece_src=piece_src, n_pieces=n_pieces,
                bytes=(n_pieces + 4 * batch + 15) // 16 * 16)


def _bound(i, n):
    """Python's slice bound: i < 0 counts from the end, then clamp to [0, n]."""
    i = int(i)
    if i < 0:
        i += n
    return min(max(i, 0), n)


def table_of(tss, cap=None):
    """Host timestamps -> (segments int64 [B, cap, 2], counts int32 [B]): `tss` is a list (per clip) of lists of {'start', 'end'} dicts
    or (start, end) pairs, in samples.  cap defaults to the longest list (at least 1)."""
    rows = [[((r["start"], r["end"]) if isinstance(r, dict) else (r[0], r[1])) for r in clip] for clip in tss]
    if len(rows) == 0:
        raise ValueError("a batch needs at least one clip")
    most = max(len(r) for r in rows)
    cap = max(1, most) if cap is None else int(cap)
    if cap < max(1, most):
        raise ValueError(f"cap={cap} is smaller than the longest list ({most} rows)")
    segs = np.zeros((len(rows), cap, 2), dtype=np.int64)
    for b, r in enumerate(rows):
        if r:
            segs[b, :len(r)] = np.asarray(r, dtype=np.int64).reshape(-1, 2)
    return segs, np.asarray([len(r) for r in rows], dtype=np.int32)


def plan_host(segments, counts, clip_len, mode, align=1):
    """The plan arithmetic on the host, field for field what vadx_chunks_plan writes: dict(total, status, clip_dst [B+1], piece_dst
    [B, cap+2], piece_src [B, cap+1, 2], n_pieces [B], lengths [B])."""
    mode = _MODES[mode]
    segments = np.asarray(segments, dtype=np.int64)
    counts, clip_len = np.asarray(counts, dtype=np.int64).reshape(-1), np.asarray(clip_len, dtype=np.int64).reshape(-1)
    B, cap = segments.shape[0], segments.shape[1]
    align = _check_align(align)
    piece_dst, piece_src = np.zeros((B, cap + 2), np.int64), np.zeros((B, cap + 1, 2), np.int64)
    n_pieces, status = np.zeros(B, np.int32), 0
    for b in range(B):
        n, ln = int(counts[b]), int(clip_len[b])
        if n < 0 or n > cap or ln < 0:
            n_pieces[b], status = -1, status | ST_BAD_CLIP
            continue
        if mode == COLLECT:
            raw = [(_bound(s, ln), _bound(e, ln)) for s, e in segments[b, :n].tolist()]
        else:
            cur, raw = 0, []
            for s, e in segments[b, :n].tolist():
                raw.append((cur, _bound(s, ln)))
                cur = _bound(e, ln)
            raw.append((cur, ln))
        at = 0
        for k, (lo, hi) in enumerate(raw):
            hi = max(lo, hi)
            piece_src[b, k], piece_dst[b, k] = (lo, hi), at
            at += hi - lo
        n_pieces[b], piece_dst[b, len(raw):] = len(raw), at
    lengths = piece_dst[:, cap + 1].copy()
    clip_dst = np.concatenate([[0], np.cumsum((lengths + align - 1) // align * align)]).astype(np.int64)
    return dict(total=int(clip_dst[-1]), status=status, clip_dst=clip_dst, piece_dst=piece_dst, piece_src=piece_src, n_pieces=n_pieces,
                lengths=lengths)


def _check_align(align):
    align = int(align)
    if align < 1 or align > 4096 or align & (align - 1):
        raise ValueError(f"align={align} must be a power of two in [1, 4096]")
    return align


class ChunkPlan:
    """The device plan record of one batch (include/vadx.h, "Chunks") and views of its fields; nothing here synchronises except
    `total`, `status` and `check()`, which read the record's 16-byte head back.
        total          int: elements of the packed output (= clip_offsets[B])
        lengths        int64 [B] device: every clip's output length
        clip_offsets   int64 [B+1] device: where every clip starts in the packed output
        piece_offsets  int64 [B, cap+2] device: the prefix of the piece lengths inside each clip
        piece_src      int64 [B, cap+1, 2] device: the resolved (lo, hi) of every piece;  n_pieces int32 [B] device (-1: a bad clip)"""

    def __init__(self, segments, counts, clip_len, mode, align=1):
        t = _lib.require_gpu()
        self.mode, self.align = _MODES[mode], _check_align(align)
        if segments.dim() != 3 or segments.shape[2] != 2 or segments.dtype != t.int64 or segments.shape[0] < 1 or segments.shape[1] < 1:
            raise ValueError(f"segments must be int64 [B, cap, 2] with B, cap >= 1, got {segments.dtype} {tuple(segments.shape)}")
        self.device = segments.device
        self.batch, self.cap = int(segments.shape[0]), int(segments.shape[1])
        segments = segments.contiguous()
        counts = counts.to(device=self.device, dtype=t.int32).reshape(-1).contiguous()
        clip_len = clip_len.to(device=self.device, dtype=t.int64).reshape(-1).contiguous()
        if counts.shape[0] != self.batch or clip_len.shape[0] != self.batch:
            raise ValueError(f"counts [{counts.shape[0]}] and lengths [{clip_len.shape[0]}] must have one entry per clip ({self.batch})")
        self.layout = plan_layout(self.batch, self.cap)
        self.record = t.empty(self.layout["bytes"], dtype=t.uint8, device=self.device)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_chunks_plan(segments.data_ptr(), counts.data_ptr(), clip_len.data_ptr(), self.batch, self.cap, self.mode,
                                                   self.align, self.record.data_ptr(), self.record.numel(), _lib.stream_ptr()))

    def _view(self, name, dtype, shape):
        n = int(np.prod(shape)) * (8 if dtype == "int64" else 4)
        t = _lib.require_gpu()
        return self.record[self.layout[name]:self.layout[name] + n].view(getattr(t, dtype)).reshape(shape)

    def head(self):
        """(total, status): one 16-byte read of the record's head (synchronises)."""
        h = self.record[:16].cpu().numpy()
        return int(h[:8].view(np.int64)[0]), int(h[8:12].view(np.int32)[0])

    @property
    def total(self):
        return self.head()[0]

    @property
    def status(self):
        return self.head()[1]

    @property
    def clip_offsets(self):
        return self._view("clip_dst", "int64", (self.batch + 1,))

    @property
    def piece_offsets(self):
        return self._view("piece_dst", "int64", (self.batch, self.cap + 2))

    @property
    def piece_src(self):
        return self._view("piece_src", "int64", (self.batch, self.cap + 1, 2))

    @property
    def n_pieces(self):
        return self._view("n_pieces", "int32", (self.batch,))

    @property
    def lengths(self):
        return self.piece_offsets[:, self.cap + 1]

    def check(self, status=None):
        """Raise VadxError when a status bit is set (reads the record's head: synchronises)."""
        status = self.status if status is None else status
        if status:
            raise _lib.VadxError("chunks: " + "; ".join(text for bit, text in _STATUS_TEXT.items() if status & bit))
        return self

    def copy(self, src, clip_src, out):
        """Fill out[0, total) from the 1-D device tensor `src` (int16 or float32; clip b starts at element clip_src[b]) by this plan
        (vadx_chunks_copy: one launch, no synchronisation).  `src` and `out` must start on a 16-byte boundary."""
        t = _lib.require_gpu()
        if src.dtype not in (t.int16, t.float32) or out.dtype != src.dtype:
            raise ValueError(f"audio must be int16 or float32 and `out` of the same type, got {src.dtype} and {out.dtype}")
        if src.dim() != 1 or out.dim() != 1 or not src.is_contiguous() or not out.is_contiguous():
            raise ValueError("audio and `out` must be contiguous 1-D tensors here")
        if src.device != self.device or out.device != self.device or clip_src.device != self.device:
            raise ValueError(f"audio, offsets and `out` must live on the plan's device {self.device}")
        pad = None
        if src.numel() == 0 or out.numel() == 0:           # an empty tensor has no address: stand-in (no element of it is touched)
            pad = t.zeros(8, dtype=src.dtype, device=self.device)
        sp, op = (pad if src.numel() == 0 else src), (pad if out.numel() == 0 else out)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_chunks_copy(sp.data_ptr(), int(src.numel()), clip_src.data_ptr(), src.element_size(), self.record.data_ptr(),
                                                   self.record.numel(), self.batch, self.cap, op.data_ptr(), int(out.numel()), _lib.stream_ptr()))
        return out


def _device_table(tss, device):
    """(segments, counts) on the device: the pair SileroEngine.segments returns goes through as it is (no host round trip), a host list is
    uploaded once as a table."""
    t = _lib.require_gpu()
    if isinstance(tss, tuple) and len(tss) == 2 and t.is_tensor(tss[0]) and t.is_tensor(tss[1]):
        return tss[0].to(device), tss[1].to(device)
    segs, counts = table_of(tss)
    return t.from_numpy(segs).to(device), t.from_numpy(counts).to(device)


def _batch(mode, tss, audio, lengths, clip_offsets, align, out, return_plan):
    t = _lib.require_gpu()
    if not t.is_tensor(audio) or not audio.is_cuda:
        raise ValueError("audio must be a device tensor (int16 or float32): [B, N], or a packed 1-D vector with clip_offsets and lengths")
    if audio.dtype not in (t.int16, t.float32):
        raise ValueError(f"audio must be int16 or float32, got {audio.dtype}")
    dev = audio.device
    as_dev = lambda v: (v if t.is_tensor(v) else t.as_tensor(np.asarray(v, dtype=np.int64))).to(device=dev, dtype=t.int64).reshape(-1)   # noqa: E731
    if audio.dim() == 2:
        if clip_offsets is not None:
            raise ValueError("clip_offsets goes with a packed 1-D audio vector, not with [B, N]")
        audio = audio.contiguous()
        B, N = audio.shape
        if lengths is None:
            lengths = t.full((B,), N, dtype=t.int64, device=dev)
        elif not t.is_tensor(lengths) and (np.asarray(lengths).shape != (B,) or np.min(lengths) < 0 or np.max(lengths) > N):
            raise ValueError(f"lengths must be {B} values in [0, {N}]")
        clip_src = t.arange(B, dtype=t.int64, device=dev) * N
        flat = audio.reshape(-1)
    elif audio.dim() == 1:
        if clip_offsets is None or lengths is None:
            raise ValueError("a packed 1-D audio vector needs clip_offsets and lengths")
        clip_src, flat = as_dev(clip_offsets), audio.contiguous()
    else:
        raise ValueError(f"audio must be [B, N] or a packed 1-D vector, got {audio.dim()} dimensions")
    if flat.data_ptr() % 16:
        flat = flat.clone()                                 # a view that starts off a 16-byte boundary
    segs, counts = _device_table(tss, dev)
    lengths = as_dev(lengths)
    if clip_src.shape[0] != segs.shape[0]:
        raise ValueError(f"{segs.shape[0]} clips of timestamps for {clip_src.shape[0]} clips of audio")
    plan = ChunkPlan(segs, counts, lengths, mode, align)
    if out is None:
        total, status = plan.head()                         # the one read-back: 16 bytes, total and status together
        plan.check(status)
        out = t.empty(total, dtype=flat.dtype, device=dev)
        if total:
            plan.copy(flat, clip_src.contiguous(), out)
    else:
        if out.data_ptr() % 16 and out.numel():
            raise ValueError("`out` must start on a 16-byte boundary")
        plan.copy(flat, clip_src.contiguous(), out)
    return (out, plan.clip_offsets, plan) if return_plan else (out, plan.clip_offsets)


def collect_chunks_batch(tss, audio, lengths=None, clip_offsets=None, align=1, out=None, return_plan=False):
    """collect_chunks (utils_vad.py:588-631) for every clip of a resident batch, in three launches.
    tss: the device pair (segs int64 [B, cap, 2], counts int32 [B]) exactly as SileroEngine.segments returns it -- no host round trip --
         or a host list (per clip) of lists of {'start', 'end'} dicts / (start, end) pairs in samples, uploaded once as a table;
    audio: device tensor, int16 or float32: [B, N] with optional `lengths`, or a packed 1-D vector with `clip_offsets` and `lengths`.
    -> (packed, offsets int64 [B+1]) on the device: clip b's speech is packed[offsets[b] : offsets[b] + n_b], every offset a multiple of
    `align`, filler zeros; n_b = `plan.lengths[b]` (offsets[b+1] - offsets[b] with align = 1).
    Without `out` the call reads the total back (one 16-byte read, like the range-flag read) and allocates; a refused clip raises there.
    With `out` (1-D, same dtype) nothing synchronises: ask for the plan (return_plan=True -> a third result) and call `plan.check()`
    when convenient -- it raises VadxError for a set status bit (`out` too small: nothing was written)."""
    return _batch(COLLECT, tss, audio, lengths, clip_offsets, align, out, return_plan)


def drop_chunks_batch(tss, audio, lengths=None, clip_offsets=None, align=1, out=None, return_plan=False):
    """drop_chunks (utils_vad.py:634-682) for every clip of a resident batch: what is left after cutting the rows out.  Arguments and
    results as `collect_chunks_batch`."""
    return _batch(DROP, tss, audio, lengths, clip_offsets, align, out, return_plan)


def from_seconds(lists, sampling_rate):
    """(start_s, end_s) lists, as the FSMN / FireRed / MarbleNet / DFSMN `detect` calls return them (one list per clip; dicts with
    'start' / 'end' in seconds are taken too) -> sample rows (int(round(start_s * sr)), int(round(end_s * sr))).
    THIS PROJECT'S OWN RULE, the nearest sample -- not the reference's `_seconds_to_samples_tss` (utils_vad.py:685-691), which rounds to
    whole seconds first and is what the `seconds=True` drop-ins below reproduce."""
    sr = float(sampling_rate)
    pair = lambda r: (r["start"], r["end"]) if isinstance(r, dict) else (r[0], r[1])       # noqa: E731
    return [[(int(round(s * sr)), int(round(e * sr))) for s, e in map(pair, clip)] for clip in lists]


def _seconds_rows(tss, sampling_rate):
    """utils_vad.py:685-691 as it stands: round(x) * sampling_rate -- whole seconds, Python's round-half-to-even."""
    return [{"start": round(c["start"]) * sampling_rate, "end": round(c["end"]) * sampling_rate} for c in tss]


def _single(mode, tss, wav, seconds, sampling_rate):
    if seconds and not sampling_rate:
        raise ValueError("sampling_rate must be provided when seconds is True")
    t = _lib.require_gpu()
    if not t.is_tensor(wav):
        raise TypeError("wav must be a torch.Tensor")
    if wav.dim() != 1:
        raise ValueError(f"wav must be one dimensional, got {tuple(wav.shape)}")
    rows = _seconds_rows(tss, sampling_rate) if seconds else list(tss)
    if mode == COLLECT and len(rows) == 0:
        raise ValueError("torch.cat(): expected a non-empty list of Tensors")       # what the reference's torch.cat([]) raises
    if not wav.is_cuda:
        raise ValueError("wav must live on the device: the vadx product path runs only on an MI355X (no CPU fallback)")
    packed, _ = _batch(mode, [rows], wav.unsqueeze(0), None, None, 1, None, False)
    return packed


def collect_chunks(tss, wav, seconds: bool = False, sampling_rate: int = None):
    """Single-clip reference signature (utils_vad.py:588-631): the pieces wav[start:end] of `tss`, concatenated -- a 1-D tensor of wav's
    dtype (int16 or float32) on wav's device.  seconds=True converts as the reference does, round(x) * sampling_rate."""
    return _single(COLLECT, tss, wav, seconds, sampling_rate)


def drop_chunks(tss, wav, seconds: bool = False, sampling_rate: int = None):
    """Single-clip reference signature (utils_vad.py:634-682): wav without the pieces of `tss`."""
    return _single(DROP, tss, wav, seconds, sampling_rate)
