"""A ragged batch prepared on the device: normalise, pad to the window grid and pack B clips that already lie in device memory
(include/vadx.h, "Prepare"; csrc/prepare.hip), and the host MIRROR that states the arithmetic the kernels must reproduce bit for bit.

The contract, all float32 with one rounding per operation:
    ms32(x)     what `np.mean(x * x)` returns for a contiguous float32 vector: the squares, rounded, are summed in consecutive chunks of
                CHUNK = 8192 elements (numpy's reduction buffer) whose sums are added in order; a chunk is numpy's pairwise sum (fewer
                than 8: in order; up to 128: eight strided accumulators combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
                remainder in order; otherwise the two halves split at n/2 - (n/2) % 8); the sum is divided by float32(n)
    "peak"      timestamps.normalize_to_int16 of the float32 clip: p = max|x|, s = 32767 / p (1 when p = 0), y = trunc(x * s)
    "rms"       timestamps.normalise_audio: r = sqrt(ms32(x)); unless r > 0 the clip stays; g = target_rms / (r + 1e-7),
                y = trunc(clip(x * g, -32768, 32767))
    grid        clips.pad_to_window_grid: pad = clips.pad_count(n, window, stride); the reference region is the last `pad` samples of y
                when n > window and all of y otherwise; rt = sqrt(ms32(ref)); fill_k = the low 16 bits of trunc(float64(rt) * z_k)
`prepare_host` is that contract in numpy (tests/test_prepare_cpu.py pins it to the functions named above); `prepare_device` is the three
launches.  `RaggedBatch.from_packed` / `RaggedFrames.from_packed` (vadx.ragged) are the public way in."""
from __future__ import annotations

import numpy as np

from .clips import pad_count

CHUNK = 8192                         # numpy's reduction buffer in elements: part of the contract, and csrc/prepare.hip's CHUNK
MODES = {None: 0, "none": 0, "peak": 1, "rms": 2}        # VADX_PREPARE_*
ST_SRC_RANGE, ST_NOISE_RANGE, ST_GRID = 1, 2, 4          # VADX_PREPARE_ST_*
STATUS_TEXT = {ST_SRC_RANGE: "a clip's source range lies outside the audio buffer (clip_offsets / lengths do not describe it): its samples are zeros",
               ST_NOISE_RANGE: "a clip's pad noise lies outside the noise buffer: those samples are zeros",
               ST_GRID: "a clip's room in the output is not what its window grid gives"}
_F = np.float32


def _pairwise32(sq):
    """numpy's pairwise sum (umath loops, pairwise_sum) of a float32 vector, in float32"""
    n = sq.shape[0]
    if n < 8:
        res = _F(0.0)
        for v in sq:
            res = _F(res + v)
        return res
    if n <= 128:
        r = sq[:8].copy()
        m = n - n % 8
        for i in range(8, m, 8):
            r += sq[i:i + 8]
        res = _F(_F(_F(r[0] + r[1]) + _F(r[2] + r[3])) + _F(_F(r[4] + r[5]) + _F(r[6] + r[7])))
        for v in sq[m:]:
            res = _F(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _F(_pairwise32(sq[:n2]) + _pairwise32(sq[n2:]))


def ms32(x):
    """np.mean(x * x) of a float32 vector, spelled out: see the module docstring"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    sq = x * x
    total = _F(0.0)
    for c0 in range(0, sq.shape[0], CHUNK):
        total = _F(total + _pairwise32(sq[c0:c0 + CHUNK]))
    return _F(total / _F(sq.shape[0]))


def scale_host(x, mode, target_rms=8192.0, ms=ms32):
    """One int16 clip -> (y int16, scale float32): the normalisation of `mode` (None | "peak" | "rms")."""
    x = np.asarray(x)
    xf = x.astype(np.float32)
    m = MODES[mode]
    if m == 1:
        p = _F(np.max(np.abs(xf)))
        s = _F(_F(32767.0) / p) if p > 0 else _F(1.0)
        return (xf * s).astype(np.int16), s
    if m == 2:
        r = _F(np.sqrt(ms(xf)))
        if not r > 0:
            return x.copy(), _F(1.0)
        g = _F(_F(target_rms) / _F(r + _F(1e-7)))
        return np.clip(xf * g, _F(-32768.0), _F(32767.0)).astype(np.int16), g
    return x.copy(), _F(1.0)


def fill_host(rt, z):
    """pad_to_window_grid's fill: the low 16 bits of trunc(float64(rt) * z)"""
    return np.trunc(np.float64(rt) * np.asarray(z, dtype=np.float64)).astype(np.int64).astype(np.int16)


def noise_rows(pads, pad_noise):
    """The standard-normal samples of every clip's fill, packed: (float64 [sum pads], int64 [B] where each clip's start).  None draws
    np.random.normal(size=pad_b) per clip with a pad, in clip order -- the draws pad_to_window_grid makes when the clips go through it
    one after the other; otherwise clip b takes the first pad_b samples of row b."""
    off = np.concatenate([[0], np.cumsum(pads)[:-1]]).astype(np.int64)
    if pad_noise is None:
        rows = [np.random.normal(loc=0.0, scale=1.0, size=int(p)) if p > 0 else np.zeros(0) for p in pads]
    else:
        if len(pad_noise) < len(pads):
            raise ValueError(f"pad_noise has {len(pad_noise)} rows for {len(pads)} clips")
        rows = [np.asarray(pad_noise[b], dtype=np.float64).reshape(-1)[:int(p)] for b, p in enumerate(pads)]
        for b, (r, p) in enumerate(zip(rows, pads)):
            if r.shape[0] < p:
                raise ValueError(f"pad_noise row {b} has {r.shape[0]} samples, clip {b} needs {int(p)}")
    return (np.concatenate(rows) if rows else np.zeros(0)).astype(np.float64), off


def prepare_host(clips, window=None, stride=None, pad_noise=None, normalize=None, target_rms=8192.0, ms=ms32):
    """The mirror: int16 clips -> a host-only vadx.ragged.RaggedBatch (window given) or RaggedFrames (window None) whose `pcm` and tables
    are what the device path must give, plus `scales` and `tail_rms` float32 [B] (the records of vadx_prepare_scale).  `ms` is the
    mean-of-squares rule (tests swap in wrong ones to show that the inputs tell them apart)."""
    from . import ragged
    if normalize not in MODES:
        raise ValueError(f"normalize must be one of {sorted(k for k in MODES if k)} or None, got {normalize!r}")
    clips = [np.asarray(c).reshape(-1) for c in clips]
    for b, c in enumerate(clips):
        if c.dtype != np.int16 or c.shape[0] == 0:
            raise ValueError(f"clip {b} must be a non-empty int16 vector")
    lengths = np.asarray([c.shape[0] for c in clips], dtype=np.int64)
    ys, scales = zip(*[scale_host(c, normalize, target_rms, ms) for c in clips])
    if window is None:
        self = ragged.RaggedFrames()
        self._set_tables(lengths)
        self.pcm_host = np.concatenate(ys)
        self.scales, self.tail_rms = np.asarray(scales, dtype=np.float32), np.zeros(len(clips), dtype=np.float32)
        self.device = None
        for name in self.TABLES:
            setattr(self, name, getattr(self, name + "_host"))
        return self
    window, stride = ragged.check_grid(window, stride)
    pads = np.asarray([pad_count(int(n), window, stride) for n in lengths], dtype=np.int64)
    z, zoff = noise_rows(pads, pad_noise)
    rows, tails = [], []
    for y, n, p, o in zip(ys, lengths, pads, zoff):
        rt = _F(0.0)
        if p > 0:
            ref = (y[-p:] if n > window else y).astype(np.float32)
            rt = _F(np.sqrt(ms(ref)))
            y = np.concatenate((y, fill_host(rt, z[o:o + p])))
        rows.append(y)
        tails.append(rt)
    self = ragged.RaggedBatch()
    self._set_grid(lengths, lengths + pads, window, stride)
    self.pcm_host = np.concatenate(rows)
    self.scales, self.tail_rms = np.asarray(scales, dtype=np.float32), np.asarray(tails, dtype=np.float32)
    self.device = None
    self.pcm, self.win_first, self.win_src, self.order = self.pcm_host, self.win_first_host, self.win_src_host, self.order_host
    return self


# ---- the device path -------------------------------------------------------------------------------------------------------------------

def read_tables(clip_offsets, lengths):
    """(clip_offsets, lengths) as host int64 [B] each.  Device tensors come back in ONE copy of 16 * B bytes -- the only synchronisation of
    the device path: every table of the batch is a function of the lengths."""
    from . import _lib
    t = _lib.require_gpu()
    if t.is_tensor(clip_offsets) and t.is_tensor(lengths) and clip_offsets.device == lengths.device:
        both = t.stack([clip_offsets.reshape(-1).to(t.int64), lengths.reshape(-1).to(t.int64)]).cpu().numpy()
        return both[0].copy(), both[1].copy()
    host = lambda a: (a.detach().cpu().numpy() if t.is_tensor(a) else np.asarray(a)).reshape(-1).astype(np.int64)      # noqa: E731
    return host(clip_offsets), host(lengths)


def chunk_tables(lengths):
    """(tile_first int32 [B+1], tile_clip int32 [tiles]): the 8192-sample chunks of vadx_prepare_stats"""
    per = (np.asarray(lengths, dtype=np.int64) + CHUNK - 1) // CHUNK
    total = int(per.sum())
    if total >= 2 ** 31:
        raise ValueError(f"{total} chunks of {CHUNK} samples do not fit the int32 tile tables")
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int32), np.repeat(np.arange(len(per), dtype=np.int32), per)


class Prepared:
    """What `prepare_device` returns: pcm int16 [total] (device), records (device float32 [B, 4] view of the workspace: scale, tail RMS,
    status bits, 0) and the host tables it was laid out by."""

    def __init__(self, pcm, workspace, batch, dst_off):
        self.pcm, self.workspace, self.batch, self.dst_off = pcm, workspace, batch, dst_off

    @property
    def records(self):
        return self.workspace[:16 * self.batch].view(_lib_torch().float32).view(self.batch, 4)

    def status(self):
        """int32 [B] host: the VADX_PREPARE_ST_* bits of every clip (synchronises)"""
        return self.workspace[:16 * self.batch].view(_lib_torch().int32).view(self.batch, 4)[:, 2].cpu().numpy()

    def check(self):
        st = self.status()
        for bit, text in STATUS_TEXT.items():
            if np.any(st & bit):
                raise ValueError(f"clip {int(np.flatnonzero(st & bit)[0])}: {text}")


def _lib_torch():
    from . import _lib
    return _lib.require_gpu()


def prepare_device(pcm, src_off, lengths, dst_off, window, stride, normalize, target_rms, noise, noise_off, out=None, workspace=None):
    """The three launches.  pcm: device int16 [n], contiguous; src_off, lengths [B], dst_off [B+1], noise_off [B]: host int64; noise: device
    float64 1-D (contiguous), or None when no clip has a fill.  out: a device int16 tensor of at least dst_off[B] elements on a 16-byte
    boundary to write into (default: a new one); workspace: a device uint8 tensor (default: a new one).  -> Prepared."""
    from . import _lib
    t = _lib.require_gpu()
    L = _lib.lib()
    if normalize not in MODES:
        raise ValueError(f"normalize must be one of {sorted(k for k in MODES if k)} or None, got {normalize!r}")
    mode = MODES[normalize]
    if not t.is_tensor(pcm) or pcm.dim() != 1 or pcm.dtype != t.int16 or not pcm.is_cuda or not pcm.is_contiguous():
        raise ValueError("pcm must be a contiguous 1-D int16 tensor on the device")
    dev = pcm.device
    src_off, lengths, dst_off = (np.ascontiguousarray(a, dtype=np.int64).reshape(-1) for a in (src_off, lengths, dst_off))
    B = lengths.shape[0]
    if B < 1 or src_off.shape[0] != B or dst_off.shape[0] != B + 1:
        raise ValueError(f"{B} lengths, {src_off.shape[0]} offsets, {dst_off.shape[0]} output offsets: a batch needs B >= 1, B and B + 1")
    if int(lengths.min()) < 1:
        raise ValueError(f"clip {int(np.argmin(lengths))} is empty")
    total = int(dst_off[-1])
    # a view that starts off a 16-byte boundary: walk from the boundary below it, which lies in the same allocation
    shift = (pcm.data_ptr() % 16) // 2
    tile_first, tile_clip = chunk_tables(lengths)
    tiles = int(tile_first[-1])
    if noise is None:
        noise = t.zeros(1, dtype=t.float64, device=dev)
        noise_off = np.zeros(B, dtype=np.int64)
    if noise.dtype != t.float64 or noise.dim() != 1 or not noise.is_contiguous() or noise.device != dev:
        raise ValueError("noise must be a contiguous 1-D float64 tensor on pcm's device")
    i64 = t.from_numpy(np.concatenate([src_off + shift, lengths, dst_off, np.ascontiguousarray(noise_off, dtype=np.int64).reshape(-1)])).to(dev)
    i32 = t.from_numpy(np.concatenate([tile_first, tile_clip])).to(dev)
    p_src_off, p_len, p_dst_off, p_noise_off = (i64.data_ptr() + 8 * k for k in (0, B, 2 * B, 3 * B + 1))
    p_tile_first, p_tile_clip = i32.data_ptr(), i32.data_ptr() + 4 * (B + 1)
    need = L.vadx_prepare_workspace_bytes(B, tiles)
    if workspace is None:
        workspace = t.empty(need, dtype=t.uint8, device=dev)
    if out is None:
        out = t.empty(total, dtype=t.int16, device=dev)
    if out.dtype != t.int16 or out.dim() != 1 or not out.is_contiguous() or out.device != dev or out.numel() < total:
        raise ValueError(f"out must be a contiguous 1-D int16 tensor of at least {total} elements on pcm's device")
    src, src_elems = pcm.data_ptr() - 2 * shift, int(pcm.numel()) + shift
    ws, ws_bytes, s = workspace.data_ptr(), int(workspace.numel()) * workspace.element_size(), _lib.stream_ptr
    with t.cuda.device(dev):
        if mode:
            _lib.check(L.vadx_prepare_stats(src, src_elems, p_src_off, p_len, p_tile_first, p_tile_clip, B, tiles, mode, ws, ws_bytes, s()))
        _lib.check(L.vadx_prepare_scale(src, src_elems, p_src_off, p_len, p_dst_off, p_tile_first, B, tiles, int(window), int(stride), mode,
                                        float(target_rms), ws, ws_bytes, s()))
        _lib.check(L.vadx_prepare_write(src, src_elems, p_src_off, p_len, p_dst_off, noise.data_ptr(), int(noise.numel()), p_noise_off, B, tiles,
                                        mode, ws, ws_bytes, out.data_ptr(), total, s()))
    return Prepared(out[:total], workspace, B, dst_off)


def device_noise(pads, pad_noise, device):
    """(noise float64 1-D on the device or None, noise_off int64 [B] host) for `prepare_device`, from any of the three forms of pad_noise:
    None (drawn on the host as the reference does, uploaded packed), host rows (the first pad_b samples of row b, uploaded packed) or a
    device float64 matrix [B or 1, >= max pad], used where it lies."""
    t = _lib_torch()
    B = len(pads)
    if int(np.max(pads)) == 0:
        return None, np.zeros(B, dtype=np.int64)
    if t.is_tensor(pad_noise) and pad_noise.is_cuda:
        if pad_noise.dtype != t.float64 or pad_noise.dim() != 2 or pad_noise.shape[0] not in (1, B) or pad_noise.shape[1] < int(np.max(pads)):
            raise ValueError(f"a device pad_noise must be float64 [{B} or 1, >= {int(np.max(pads))}], got {pad_noise.dtype} {tuple(pad_noise.shape)}")
        m = pad_noise.to(device).contiguous()
        return m.reshape(-1), (np.arange(B, dtype=np.int64) * m.shape[1] if m.shape[0] == B else np.zeros(B, dtype=np.int64))
    if t.is_tensor(pad_noise):
        pad_noise = pad_noise.numpy()
    z, off = noise_rows(pads, pad_noise)
    return t.from_numpy(z).to(device), off
