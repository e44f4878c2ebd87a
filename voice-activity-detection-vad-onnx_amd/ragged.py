"""A RAGGED batch: clips of any lengths packed into one int16 vector, with the tables the device needs to walk it.

Every clip is padded to its own window grid on the host (`clips.pad_to_window_grid`: the reference's tail-noise arithmetic, bit-pinned
there), the padded clips are laid end to end -- each starting on a multiple of 8 samples, so that every analysis window is a whole
number of 16-byte runs -- and uploaded ONCE.  Overlapping windows (FSMN: 16000 samples every 11040) exist only on the device, after
vadx_windows_gather; the padding a rectangular [B, max N] batch would add to short clips is neither uploaded nor computed: the work
of every later launch is proportional to sum(W_b) windows, not B * max(W_b).

Tables (include/vadx.h, "Ragged batches"):
    win_first [B+1]  prefix sum of the windows per clip: clip b owns windows win_first[b] .. win_first[b+1]-1 of every per-window buffer
    win_src   [sum W] sample offset of every window in `pcm`: clip_off[b] + k * stride
    order     [B]    clips by window count, longest first (stable): the launch order of one-workgroup-per-clip kernels

`RaggedBatch.from_packed` / `RaggedFrames.from_packed` build the same objects from clips that already lie in DEVICE memory (the output of
vadx.chunks.collect_chunks_batch or audio_io.ingest_ragged): normalisation, padding and packing run there (vadx.prepare), bit for bit
what `from_clips` does on the host, and the tables -- functions of the lengths alone -- come from the same code.

`RaggedPairs` is the batch of DFSMN's near / far pairs: two packed vectors on one grid of odd window and stride (no 16-byte runs:
vadx_windows_gather_any), sharing win_first and win_src.

`RaggedFrames` (below) is the batch of the model whose window is the whole clip (MarbleNet, dynamic axis): no window grid, no padding --
the clips as they are, with per-clip frame prefixes and tile tables.

`RaggedClips` (at the end) is Silero's batch: float32 or int16 clips as they are, sorted into groups of sixteen by window count, with the
slot, group and workgroup tables of include/vadx.h's vadx_silero_ragged.
"""
from __future__ import annotations

import numpy as np

from .clips import pad_to_window_grid

ALIGN = 8            # samples: window and stride are multiples of it, so every clip starts on a 16-byte boundary of the packed vector


def check_grid(window, stride):
    window, stride = int(window), int(stride)
    if window < ALIGN or window % ALIGN or stride < ALIGN or stride % ALIGN:
        raise ValueError(f"window={window} and stride={stride} must be positive multiples of {ALIGN} samples")
    return window, stride


class RaggedBatch:
    """Fields: pcm int16 [total], lengths [B] (original sample counts, host), windows int32 [B] (host), win_first int32 [B+1],
    win_src int64 [sum W], order int32 [B]; clip_off int64 [B] (host) = where each padded clip starts in pcm, padded_lengths [B].
    With a device, pcm / win_first / win_src / order are tensors there and the `*_host` attributes keep the numpy tables; with
    device=None everything stays numpy (the host tables ARE the fields)."""

    @classmethod
    def from_clips(cls, clips, window, stride, pad_noise=None, prep=None, device="cuda:0"):
        """clips: list of 1-D int16 arrays (or whatever `prep` turns into one: FSMN passes timestamps.normalize_to_int16);
        pad_noise: None (numpy's global RNG, as the reference) or standard-normal rows, a list or a matrix -- clip b uses the first
        pad_b samples of row b."""
        window, stride = check_grid(window, stride)
        if len(clips) == 0:
            raise ValueError("a ragged batch needs at least one clip")
        if pad_noise is not None and len(pad_noise) < len(clips):
            raise ValueError(f"pad_noise has {len(pad_noise)} rows for {len(clips)} clips")
        rows, lengths = [], []
        for b, c in enumerate(clips):
            a = np.asarray(c).reshape(-1)
            if a.shape[0] == 0:
                raise ValueError(f"clip {b} is empty")
            lengths.append(a.shape[0])
            a = np.asarray(prep(a) if prep is not None else a)
            if a.dtype != np.int16:
                raise ValueError(f"clip {b} must be int16 (after prep), got {a.dtype}")
            rows.append(pad_to_window_grid(a, window, stride, None if pad_noise is None else np.asarray(pad_noise[b]).reshape(-1)))
        self = cls()
        self._set_grid(lengths, [len(r) for r in rows], window, stride)
        pcm = np.concatenate(rows)
        self.pcm_host = pcm
        self.device = None
        self.pcm, self.win_first, self.win_src, self.order = pcm, self.win_first_host, self.win_src_host, self.order_host
        if device is not None:
            self.to(device)
        return self

    def _set_grid(self, lengths, padded_lengths, window, stride):
        """Every table of the batch: a function of the clips' lengths before and after padding, and of the grid."""
        self.window, self.stride = window, stride
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.padded_lengths = np.asarray(padded_lengths, dtype=np.int64)
        self.windows = ((self.padded_lengths - window) // stride + 1).astype(np.int32)
        # a padded clip is (W-1) * stride + window samples, a multiple of 8 like both terms: laid end to end, every clip (and so every
        # window) starts on a 16-byte boundary with no filler between clips
        self.clip_off = np.concatenate([[0], np.cumsum(self.padded_lengths)[:-1]]).astype(np.int64)
        nwin = int(self.windows.sum())
        if nwin >= 2 ** 31:
            raise ValueError(f"{nwin} windows do not fit the int32 window tables")
        self.n_windows, self.max_windows = nwin, int(self.windows.max())
        self.win_first_host = np.concatenate([[0], np.cumsum(self.windows, dtype=np.int64)]).astype(np.int32)
        k = np.arange(nwin, dtype=np.int64) - np.repeat(self.win_first_host[:-1].astype(np.int64), self.windows)
        self.win_src_host = np.repeat(self.clip_off, self.windows) + k * stride
        self.order_host = np.argsort(-self.windows.astype(np.int64), kind="stable").astype(np.int32)

    @classmethod
    def from_packed(cls, pcm, clip_offsets, lengths, window, stride, pad_noise=None, normalize=None, target_rms=8192.0, device=None,
                    out=None):
        """The batch `from_clips` builds, from clips that already lie in device memory (vadx.prepare; include/vadx.h, "Prepare"): bit for
        bit the same `pcm` and tables, and the PCM never visits the host.
        pcm: 1-D int16 tensor on the device, clip b = lengths[b] samples from element clip_offsets[b] (any element: what
        chunks.collect_chunks_batch or audio_io.ingest_ragged return); clip_offsets / lengths: host arrays or device tensors (device
        tensors are read back once, 16 * B bytes -- the only synchronisation).  normalize: None, "peak" (timestamps.normalize_to_int16 of
        the float32 clip: FSMN's prep) or "rms" (timestamps.normalise_audio with `target_rms`).  pad_noise: None (numpy's global RNG, one
        draw of pad_b per clip in clip order, as the reference), standard-normal host rows (clip b uses the first pad_b samples of row b)
        or a device float64 matrix [B or 1, >= the longest pad], used where it lies.  out: an int16 device tensor to write the packed
        vector into (16-byte aligned, long enough).  `pcm_host` is None; `records` holds per clip (scale, tail RMS, status bits, 0) on the
        device and `check()` reads the status bits (a clip whose offsets lie outside `pcm` is zeros and says so there)."""
        from . import _lib, prepare
        from .clips import pad_count
        t = _lib.require_gpu()
        window, stride = check_grid(window, stride)
        src_off, lengths = prepare.read_tables(clip_offsets, lengths)
        if lengths.shape[0] == 0:
            raise ValueError("a ragged batch needs at least one clip")
        if src_off.shape[0] != lengths.shape[0]:
            raise ValueError(f"{src_off.shape[0]} clip_offsets for {lengths.shape[0]} lengths")
        if int(lengths.min()) < 1:
            raise ValueError(f"clip {int(np.argmin(lengths))} is empty")
        pcm = pcm.to(device) if device is not None else pcm
        pads = np.asarray([pad_count(int(n), window, stride) for n in lengths], dtype=np.int64)
        self = cls()
        self._set_grid(lengths, lengths + pads, window, stride)
        self.device = pcm.device
        noise, noise_off = prepare.device_noise(pads, pad_noise, self.device)
        dst_off = np.concatenate([self.clip_off, [int(self.padded_lengths.sum())]])
        self.prepared = prepare.prepare_device(pcm.contiguous(), src_off, lengths, dst_off, window, stride, normalize, target_rms, noise, noise_off,
                                               out=out)
        self.pcm, self.records, self.pcm_host = self.prepared.pcm, self.prepared.records, None
        self.win_first = t.from_numpy(self.win_first_host).to(self.device)
        self.win_src = t.from_numpy(self.win_src_host).to(self.device)
        self.order = t.from_numpy(self.order_host).to(self.device)
        return self

    def check(self):
        """Raise ValueError when the device refused a clip of a `from_packed` batch (one small read-back)."""
        if getattr(self, "prepared", None) is not None:
            self.prepared.check()
        return self

    def to(self, device):
        """Upload the packed PCM (once) and the three tables."""
        from . import _lib
        t = _lib.require_gpu()
        self.device = t.device(device)
        self.pcm = t.from_numpy(self.pcm_host).to(self.device)
        self.win_first = t.from_numpy(self.win_first_host).to(self.device)
        self.win_src = t.from_numpy(self.win_src_host).to(self.device)
        self.order = t.from_numpy(self.order_host).to(self.device)
        return self

    def __len__(self):
        return int(self.lengths.shape[0])

    def padded(self, b):
        """Clip b as it was packed (host int16 [padded_lengths[b]]) = pad_to_window_grid of the prepped clip (a `from_packed` batch keeps
        no host copy: its slice is downloaded)."""
        if self.pcm_host is None:
            return self.pcm[int(self.clip_off[b]):int(self.clip_off[b] + self.padded_lengths[b])].cpu().numpy()
        return self.pcm_host[self.clip_off[b]:self.clip_off[b] + self.padded_lengths[b]]

    def gather(self):
        """window_buf int16 [n_windows, window] on the device (vadx_windows_gather): row win_first[b] + k is window k of clip b."""
        from . import _lib
        if self.device is None:
            raise ValueError("this batch is host-only: call .to(device) first")
        t = _lib.require_gpu()
        wbuf = t.empty((self.n_windows, self.window), dtype=t.int16, device=self.device)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_windows_gather(self.pcm.data_ptr(), int(self.pcm.numel()), self.win_src.data_ptr(), self.n_windows,
                                                      self.window, wbuf.data_ptr(), _lib.stream_ptr()))
        return wbuf


class RaggedPairs:
    """DFSMN's ragged batch: near / far clip pairs of any lengths (far None = the near-end-only model) on ONE window grid that need not be
    made of 16-byte runs (16 001 samples every 10 881).  Per pair both sides are cut to the shorter one, go through `prep` and through
    `pad_to_window_grid`, each side with its own noise row (DFSMN/near_and_far_end_audio/Inference_DFSMN_VAD_ONNX.py:124-163); the padded
    clips lie end to end with NO alignment filler in two int16 vectors, `near` and `far`, which share every table: lengths [B] (samples
    after the cut), padded_lengths [B], windows int32 [B], clip_off int64 [B], win_first int32 [B+1], win_src int64 [sum W].
    With a device near / far / win_first / win_src are tensors there and the `*_host` attributes keep numpy; device=None keeps numpy."""

    @classmethod
    def from_clips(cls, near_clips, far_clips, window, stride, pad_noise_near=None, pad_noise_far=None, prep=None, device="cuda:0"):
        """near_clips / far_clips: lists of 1-D arrays (int16, or whatever `prep` turns into int16); pad_noise_*: None (numpy's global RNG,
        as the reference) or standard-normal rows -- pair b uses the first pad_b samples of row b of its side."""
        window, stride = int(window), int(stride)
        if window < 1 or stride < 1:
            raise ValueError(f"window={window} and stride={stride} must be positive")
        B = len(near_clips)
        if B == 0:
            raise ValueError("a ragged batch needs at least one clip")
        if far_clips is not None and len(far_clips) != B:
            raise ValueError(f"{B} near clips but {len(far_clips)} far clips")
        for name, nz in (("pad_noise_near", pad_noise_near), ("pad_noise_far", pad_noise_far)):
            if nz is not None and len(nz) < B:
                raise ValueError(f"{name} has {len(nz)} rows for {B} clips")

        def side(clips, noise, lengths):
            rows = []
            for b, n in enumerate(lengths):
                a = np.asarray(clips[b]).reshape(-1)[:n]
                a = np.asarray(prep(a) if prep is not None else a)
                if a.dtype != np.int16:
                    raise ValueError(f"clip {b} must be int16 (after prep), got {a.dtype}")
                rows.append(pad_to_window_grid(a, window, stride, None if noise is None else np.asarray(noise[b]).reshape(-1)))
            return rows

        lengths = [np.asarray(c).reshape(-1).shape[0] for c in near_clips]
        if far_clips is not None:
            lengths = [min(n, np.asarray(c).reshape(-1).shape[0]) for n, c in zip(lengths, far_clips)]
        if min(lengths) == 0:
            raise ValueError(f"clip {int(np.argmin(lengths))} is empty")
        near = side(near_clips, pad_noise_near, lengths)
        far = None if far_clips is None else side(far_clips, pad_noise_far, lengths)
        self = cls()
        self.window, self.stride = window, stride
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.padded_lengths = np.asarray([len(r) for r in near], dtype=np.int64)       # both sides: the same length, so the same grid
        self.windows = ((self.padded_lengths - window) // stride + 1).astype(np.int32)
        self.clip_off = np.concatenate([[0], np.cumsum(self.padded_lengths)[:-1]]).astype(np.int64)
        self.win_first_host = _prefix(self.windows, "windows")
        self.n_windows, self.max_windows = int(self.win_first_host[-1]), int(self.windows.max())
        k = np.arange(self.n_windows, dtype=np.int64) - np.repeat(self.win_first_host[:-1].astype(np.int64), self.windows)
        self.win_src_host = np.repeat(self.clip_off, self.windows) + k * stride
        self.near_host, self.far_host = np.concatenate(near), None if far is None else np.concatenate(far)
        self.device = None
        self.near, self.far, self.win_first, self.win_src = self.near_host, self.far_host, self.win_first_host, self.win_src_host
        if device is not None:
            self.to(device)
        return self

    def to(self, device):
        """Upload the two packed vectors (once) and the two tables."""
        from . import _lib
        t = _lib.require_gpu()
        self.device = t.device(device)
        up = lambda a: None if a is None else t.from_numpy(a).to(self.device)      # noqa: E731
        self.near, self.far, self.win_first, self.win_src = up(self.near_host), up(self.far_host), up(self.win_first_host), up(self.win_src_host)
        return self

    def __len__(self):
        return int(self.lengths.shape[0])

    def padded(self, b):
        """Pair b as it was packed: (near, far) host int16 [padded_lengths[b]] each (far None for a near-only batch) =
        pad_to_window_grid of the cut, prepped clip with that side's noise row."""
        at = slice(int(self.clip_off[b]), int(self.clip_off[b] + self.padded_lengths[b]))
        return self.near_host[at], None if self.far_host is None else self.far_host[at]

    def gather(self):
        """(near_buf, far_buf) int16 [n_windows, window] on the device (vadx_windows_gather_any, once per channel; far_buf None for a
        near-only batch): row win_first[b] + k is window k of pair b."""
        from . import _lib
        if self.device is None:
            raise ValueError("this batch is host-only: call .to(device) first")
        t = _lib.require_gpu()
        out = []
        for pcm in (self.near, self.far):
            if pcm is None:
                out.append(None)
                continue
            wbuf = t.empty((self.n_windows, self.window), dtype=t.int16, device=self.device)
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().vadx_windows_gather_any(pcm.data_ptr(), int(pcm.numel()), self.win_src.data_ptr(), self.n_windows,
                                                              self.window, wbuf.data_ptr(), _lib.stream_ptr()))
            out.append(wbuf)
        return tuple(out)


FE_TILE, ENC_TILE = 64, 32   # frames per front-end / encoder tile (csrc/frontend.hip: TF_FOLD, csrc/marblenet.hip: TILE)
HOP = 160                    # the MarbleNet preset's hop: a clip of n samples has n // HOP + 1 log-mel frames (centre-padded)


def _prefix(counts, what):
    """int32 prefix sum [B+1] of per-clip counts, refused when the total leaves the int32 range."""
    total = int(np.sum(counts, dtype=np.int64))
    if total >= 2 ** 31:
        raise ValueError(f"{total} {what} do not fit the int32 tables of a ragged batch")
    return np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32)


class RaggedFrames:
    """MarbleNet's ragged batch (dynamic-axis mode: one window = one whole clip, so every clip has its own frame count; include/vadx.h,
    "MarbleNet over a RAGGED batch").  The clips lie end to end in `pcm` with NO padding and no alignment filler: the front-end's sample
    loads are single int16 loads from clamped indices (csrc/frontend.hip: split_tile), so a clip may start at any sample.
    Fields: pcm int16 [sum n_b]; clip_off int64 [B], clip_len int32 [B]; mel_first int32 [B+1] = prefix of F_b = n_b // 160 + 1 log-mel
    frames; enc_first int32 [B+1] = prefix of T1_b = (F_b - 1) // 2 + 1 encoder frames (the stride-2, k 11 prologue); per tiling
    (front-end 64 frames, encoder 32) a prefix `*_tile_first` int32 [B+1] and the clip of every tile `*_tile_clip` int32 [n_tiles]: a
    workgroup finds (clip, tile) with two uniform loads, no search -- the tables cost one int per tile, and a search would put a
    dependent chain of log2(B) loads in front of every tile's first useful load.
    With a device every field is a tensor there and the `*_host` attributes keep the numpy tables; device=None keeps numpy only."""

    TABLES = ("pcm", "clip_off", "clip_len", "mel_first", "enc_first", "fe_tile_first", "fe_tile_clip", "enc_tile_first", "enc_tile_clip")

    @classmethod
    def from_clips(cls, clips, device="cuda:0"):
        if len(clips) == 0:
            raise ValueError("a ragged batch needs at least one clip")
        rows = []
        for b, c in enumerate(clips):
            a = np.asarray(c)
            if a.dtype != np.int16:
                raise ValueError(f"clip {b} must be int16, got {a.dtype}")
            a = a.reshape(-1)
            if a.shape[0] == 0:
                raise ValueError(f"clip {b} is empty")
            rows.append(a)
        self = cls()
        self._set_tables([len(r) for r in rows])
        self.pcm_host = np.concatenate(rows)
        self.device = None
        for name in self.TABLES:
            setattr(self, name, getattr(self, name + "_host"))
        if device is not None:
            self.to(device)
        return self

    def _set_tables(self, lengths):
        """Every table of the batch: a function of the clips' lengths."""
        self.lengths = np.asarray(lengths, dtype=np.int64)
        if int(self.lengths.max()) >= 2 ** 31:
            raise ValueError("a clip of 2^31 samples or more does not fit the int32 clip_len table")
        self.clip_len_host = self.lengths.astype(np.int32)
        self.clip_off_host = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        self.mel_frames = (self.lengths // HOP + 1).astype(np.int64)
        self.enc_frames = (self.mel_frames - 1) // 2 + 1
        self.mel_first_host, self.enc_first_host = _prefix(self.mel_frames, "log-mel frames"), _prefix(self.enc_frames, "encoder frames")
        fe_tiles, enc_tiles = (self.mel_frames + FE_TILE - 1) // FE_TILE, (self.enc_frames + ENC_TILE - 1) // ENC_TILE
        self.fe_tile_first_host, self.enc_tile_first_host = _prefix(fe_tiles, "front-end tiles"), _prefix(enc_tiles, "encoder tiles")
        ids = np.arange(len(self.lengths), dtype=np.int32)
        self.fe_tile_clip_host, self.enc_tile_clip_host = np.repeat(ids, fe_tiles), np.repeat(ids, enc_tiles)
        self.n_mel, self.n_enc = int(self.mel_first_host[-1]), int(self.enc_first_host[-1])
        self.n_fe_tiles, self.n_enc_tiles = int(self.fe_tile_first_host[-1]), int(self.enc_tile_first_host[-1])

    @classmethod
    def from_packed(cls, pcm, clip_offsets, lengths, normalize=None, target_rms=8192.0, device=None, out=None):
        """The batch `from_clips` builds, from clips that already lie in device memory (vadx.prepare): the PCM is repacked end to end on the
        device -- RMS-normalised on the way with normalize="rms" (timestamps.normalise_audio, bit for bit) -- and never visits the host.
        pcm, clip_offsets, lengths, out: as RaggedBatch.from_packed; `pcm_host` is None."""
        from . import _lib, prepare
        t = _lib.require_gpu()
        if normalize not in (None, "rms"):
            raise ValueError(f"normalize must be None or 'rms', got {normalize!r}")
        src_off, lengths = prepare.read_tables(clip_offsets, lengths)
        if lengths.shape[0] == 0:
            raise ValueError("a ragged batch needs at least one clip")
        if src_off.shape[0] != lengths.shape[0]:
            raise ValueError(f"{src_off.shape[0]} clip_offsets for {lengths.shape[0]} lengths")
        if int(lengths.min()) < 1:
            raise ValueError(f"clip {int(np.argmin(lengths))} is empty")
        pcm = pcm.to(device) if device is not None else pcm
        self = cls()
        self._set_tables(lengths)
        self.device = pcm.device
        dst_off = np.concatenate([self.clip_off_host, [int(self.lengths.sum())]])
        # no grid: every clip's room is its own length, so nothing is filled and the grid arguments only have to be well formed
        self.prepared = prepare.prepare_device(pcm.contiguous(), src_off, lengths, dst_off, ALIGN, ALIGN, normalize, target_rms, None, None, out=out)
        self.pcm, self.records, self.pcm_host = self.prepared.pcm, self.prepared.records, None
        for name in self.TABLES[1:]:
            setattr(self, name, t.from_numpy(getattr(self, name + "_host")).to(self.device))
        return self

    def check(self):
        """Raise ValueError when the device refused a clip of a `from_packed` batch (one small read-back)."""
        if getattr(self, "prepared", None) is not None:
            self.prepared.check()
        return self

    def to(self, device):
        """Upload the packed PCM (once) and the tables."""
        from . import _lib
        t = _lib.require_gpu()
        self.device = t.device(device)
        for name in self.TABLES:
            setattr(self, name, t.from_numpy(getattr(self, name + "_host")).to(self.device))
        return self

    def __len__(self):
        return int(self.lengths.shape[0])

    def encoder_tables(self):
        """The vadx_marblenet_ragged struct of this batch (device pointers: the batch must be on a device)."""
        from . import _lib
        if self.device is None:
            raise ValueError("this batch is host-only: call .to(device) first")
        return _lib.MarbleNetRagged(self.enc_tile_first.data_ptr(), self.enc_tile_clip.data_ptr(), self.enc_first.data_ptr(),
                                    self.mel_first.data_ptr(), len(self), self.n_enc_tiles, self.n_enc, self.n_mel)


SNIP_NFFT = 400              # the FireRed preset's analysis frame: a clip of n >= 400 samples has (n - 400) // HOP + 1 frames (snip edges)
LONG_TILE = 64               # frames per tile of the FireRed long path and of its front-end (include/vadx.h: VADX_FIRERED_LONG_TILE)


def long_tables(frames):
    """The tables of vadx_firered_long_tables for windows of `frames` [B] frames each (0 allowed: no tile): (frame_first int32 [B+1],
    tile_first int32 [B+1], tile_clip int32 [n_tiles]).  A rectangular batch is the same tables with equal counts."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    if frames.shape[0] == 0:
        raise ValueError("a batch needs at least one window")
    if int(frames.min()) < 0:
        raise ValueError(f"window {int(np.argmin(frames))} has a negative frame count")
    tiles = (frames + LONG_TILE - 1) // LONG_TILE
    return _prefix(frames, "frames"), _prefix(tiles, "tiles"), np.repeat(np.arange(frames.shape[0], dtype=np.int32), tiles)


class PackedClips:
    """FireRed's batch in the dynamic-axis mode (FireRedEngine(long_windows=True, input_audio_length=None): one window = one whole clip;
    include/vadx.h, "FireRed windows of ANY length").  The clips lie end to end in one int16 vector `pcm`; no padding exists in this
    mode.  Fields: pcm int16 [>= sum n_b]; clip_off int64 [B], clip_len int32 [B]; frames int64 [B] (host) = snip-edge frame counts
    ((n - 400) // 160 + 1, 0 under 400 samples: no frame, no tile, no segment); frame_first / tile_first int32 [B+1], tile_clip int32
    [n_tiles] (64-frame tiles: ONE table set serves the front-end and the net).  With a device every table is a tensor there and the
    `*_host` attributes keep numpy; device=None keeps numpy only."""

    TABLES = ("pcm", "clip_off", "clip_len", "frame_first", "tile_first", "tile_clip")

    @classmethod
    def from_clips(cls, clips, device="cuda:0", max_frames=None):
        if len(clips) == 0:
            raise ValueError("a packed batch needs at least one clip")
        rows = []
        for b, c in enumerate(clips):
            a = np.asarray(c)
            if a.dtype != np.int16:
                raise ValueError(f"clip {b} must be int16, got {a.dtype}")
            a = a.reshape(-1)
            if a.shape[0] == 0:
                raise ValueError(f"clip {b} is empty")
            rows.append(a)
        self = cls()
        self._set_tables([len(r) for r in rows], None, max_frames)
        self.pcm_host = np.concatenate(rows)
        self.device = None
        for name in self.TABLES:
            setattr(self, name, getattr(self, name + "_host"))
        if device is not None:
            self.to(device)
        return self

    @classmethod
    def from_lengths(cls, lengths, clip_offsets=None, max_frames=None):
        """The host tables of clips of `lengths` samples (end to end, or at `clip_offsets`) without any PCM: what a caller with its own
        device buffer hands to the C entry points, and where a clip above `max_frames` frames is refused before a sample is touched."""
        self = cls()
        self._set_tables(lengths, clip_offsets, max_frames)
        self.device = self.pcm = self.pcm_host = None
        for name in self.TABLES[1:]:
            setattr(self, name, getattr(self, name + "_host"))
        return self

    @classmethod
    def from_packed(cls, pcm, clip_offsets, lengths, device=None, max_frames=None):
        """Tables only, around clips that already lie in device memory: pcm 1-D int16 tensor, clip b = lengths[b] samples from element
        clip_offsets[b] (any element) -- the output of chunks.collect_chunks_batch or audio_io.ingest_ragged goes straight in; nothing is
        copied.  clip_offsets / lengths: host arrays or device tensors (read back once)."""
        from . import _lib, prepare
        t = _lib.require_gpu()
        src_off, lengths = prepare.read_tables(clip_offsets, lengths)
        if lengths.shape[0] == 0:
            raise ValueError("a packed batch needs at least one clip")
        if src_off.shape[0] != lengths.shape[0]:
            raise ValueError(f"{src_off.shape[0]} clip_offsets for {lengths.shape[0]} lengths")
        if int(lengths.min()) < 1:
            raise ValueError(f"clip {int(np.argmin(lengths))} is empty")
        if pcm.dtype != t.int16 or pcm.dim() != 1:
            raise ValueError(f"pcm must be a 1-D int16 tensor, got {pcm.dtype} {list(pcm.shape)}")
        if int(src_off.min()) < 0 or int((src_off + lengths).max()) > int(pcm.numel()):
            raise ValueError("a clip lies outside pcm")
        pcm = (pcm.to(device) if device is not None else pcm).contiguous()
        self = cls()
        self._set_tables(lengths, src_off, max_frames)
        self.device, self.pcm, self.pcm_host = pcm.device, pcm, None
        for name in self.TABLES[1:]:
            setattr(self, name, t.from_numpy(getattr(self, name + "_host")).to(self.device))
        return self

    def _set_tables(self, lengths, offsets=None, max_frames=None):
        """Every table of the batch: a function of the clips' lengths (and of where they lie)."""
        self.lengths = np.asarray(lengths, dtype=np.int64)
        if int(self.lengths.max()) >= 2 ** 31:
            raise ValueError("a clip of 2^31 samples or more does not fit the int32 clip_len table")
        self.frames = np.where(self.lengths < SNIP_NFFT, 0, (self.lengths - SNIP_NFFT) // HOP + 1).astype(np.int64)
        if max_frames is not None and int(self.frames.max()) > int(max_frames):
            b = int(np.argmax(self.frames))
            raise ValueError(f"clip {b} has {int(self.frames[b])} frames ({int(self.lengths[b])} samples): a window holds at most {int(max_frames)} "
                             f"frames (3600 s); cut the file first")
        self.clip_len_host = self.lengths.astype(np.int32)
        self.clip_off_host = (np.concatenate([[0], np.cumsum(self.lengths)[:-1]]) if offsets is None else np.asarray(offsets)).astype(np.int64)
        self.frame_first_host, self.tile_first_host, self.tile_clip_host = long_tables(self.frames)
        self.n_frames, self.n_tiles = int(self.frame_first_host[-1]), int(self.tile_first_host[-1])

    def to(self, device):
        """Upload the packed PCM (once) and the tables."""
        from . import _lib
        t = _lib.require_gpu()
        self.device = t.device(device)
        for name in self.TABLES:
            setattr(self, name, t.from_numpy(getattr(self, name + "_host")).to(self.device))
        return self

    def __len__(self):
        return int(self.lengths.shape[0])

    def tables(self):
        """The vadx_firered_long_tables struct of this batch (device pointers: the batch must be on a device)."""
        from . import _lib
        if self.device is None:
            raise ValueError("this batch is host-only: call .to(device) first")
        return _lib.FireRedLongTables(self.frame_first.data_ptr(), self.tile_first.data_ptr(), self.tile_clip.data_ptr(), len(self),
                                      self.n_tiles, self.n_frames)


SILERO_WINDOW = 512          # samples per Silero window at 16 kHz
SILERO_WINDOWS = {16000: 512, 8000: 256}     # samples per window of the network of each rate
SILERO_GROUP = 16            # clips per group = columns of one MFMA tile
SILERO_RUN = 4               # windows per workgroup-table entry (include/vadx.h: VADX_SILERO_RAGGED_RUN)
GX_TILE_BYTES = 32768        # one (group, window) tile of gate pre-activations


def _wg_tab(group_windows):
    """The workgroup table int32 [n_runs, 2] = (group, run of SILERO_RUN windows) of groups with these window counts (which never grow
    with the group index): run-major over the groups that still have that run, which are the first n_r groups."""
    runs = (np.asarray(group_windows, dtype=np.int64) + SILERO_RUN - 1) // SILERO_RUN
    n_r = np.searchsorted(-runs, -np.arange(1, int(runs.max()) + 1), side="right")   # groups with runs >= r + 1
    grp = np.concatenate([np.arange(n, dtype=np.int32) for n in n_r])
    run = np.repeat(np.arange(len(n_r), dtype=np.int32), n_r)
    return np.ascontiguousarray(np.stack([grp, run], axis=1).astype(np.int32))


class RaggedClips:
    """Silero's ragged batch (include/vadx.h, "Silero over a RAGGED batch"): clips of any lengths in ONE packed vector, float32 on
    the +-1 scale or int16 PCM (scaled by SileroEngine.PCM16_SCALE while staging), as they are -- Silero needs no normalisation and no
    padding, so `from_packed` copies nothing.  The batch is built for ONE network: `sampling_rate` 16000 (`window` = 512 samples) or 8000
    (256).  The clips are sorted by window count T_b = ceil(len_b / window), descending and stable, and
    taken sixteen at a time as GROUPS; a group runs T_g = its first slot's window count, and the encoder's work is sum(T_g) tiles instead
    of ceil(B / 16) * max(T_b).
    Host fields (functions of the lengths and offsets alone, `_set_tables`): lengths int64 [B], clip_off int64 [B], windows int64 [B],
    order [B], group_windows [G]; tables `<name>_host`: slot_off int64 [16 G], slot_len / slot_clip int32 [16 G] (slot_clip = -1 behind the
    last clip of a partial group), gx_first int32 [G + 1], grp_min_len int32 [G], wg_tab int32 [n_runs, 2] = (group, run of four windows),
    run-major over the groups that still have that run, probs_first int64 [B + 1]; n_windows = sum(T_b), tiles = sum(T_g), n_runs,
    workspace_bytes = tiles * 32 KB.  With a device, `pcm`, the tables and the status word are tensors there.
    Scores of a batch: one packed float32 vector [n_windows], clip b's at probs_first[b] .. probs_first[b + 1] (`rows`).
    A batch whose workspace exceeds a cap runs in PARTS (`parts`, `part_tables`): runs of consecutive groups, each described by a table
    set of its own -- gx_first rebased to the part, wg_tab over the part's groups -- that shares the batch's slot and score tables."""

    TABLES = ("slot_off", "slot_len", "slot_clip", "gx_first", "grp_min_len", "wg_tab", "probs_first")

    @classmethod
    def from_clips(cls, clips, device="cuda:0", align=ALIGN, *, sampling_rate=16000):
        """clips: list of 1-D arrays, all float32 (+-1 scale) or all int16; packed on the host with every clip on a multiple of `align`
        elements (zero filler) and uploaded once.  sampling_rate: 16000 or 8000, the network the batch is for."""
        if len(clips) == 0:
            raise ValueError("a ragged batch needs at least one clip")
        align = int(align)
        if align < 1:
            raise ValueError(f"align={align} must be positive")
        rows = []
        for b, c in enumerate(clips):
            a = c.detach().cpu().numpy() if hasattr(c, "detach") else np.asarray(c)
            if a.dtype not in (np.float32, np.int16):
                raise ValueError(f"clip {b} must be float32 or int16, got dtype {a.dtype}")
            if rows and a.dtype != rows[0].dtype:
                raise ValueError(f"clip {b} has dtype {a.dtype}, clip 0 {rows[0].dtype}: one batch, one dtype")
            a = a.reshape(-1)
            if a.shape[0] == 0:
                raise ValueError(f"clip {b} is empty")
            rows.append(a)
        lengths = np.asarray([len(r) for r in rows], dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum((lengths + align - 1) // align * align)]).astype(np.int64)
        self = cls()
        self._set_tables(lengths, starts[:-1], sampling_rate)
        pcm = np.zeros(int(starts[-1]), dtype=rows[0].dtype)
        for k, r in enumerate(rows):
            pcm[starts[k]:starts[k] + len(r)] = r
        self.pcm_host, self.device = pcm, None
        self.pcm = pcm
        for name in self.TABLES:
            setattr(self, name, getattr(self, name + "_host"))
        self.status = None
        if device is not None:
            self.to(device)
        return self

    @classmethod
    def from_packed(cls, pcm, clip_offsets, lengths, *, sampling_rate=16000):
        """Tables only, over clips that already lie in DEVICE memory: pcm 1-D float32 or int16 tensor, clip b = lengths[b] samples from
        element clip_offsets[b] (any element: what chunks.collect_chunks_batch / drop_chunks_batch return goes in as it is).  No copy;
        clip_offsets / lengths are host arrays or device tensors (read back once, as prepare.read_tables does).  sampling_rate: 16000 or
        8000, the network the batch is for."""
        from . import _lib, prepare
        t = _lib.require_gpu()
        if not t.is_tensor(pcm) or not pcm.is_cuda or pcm.dim() != 1:
            raise ValueError("pcm must be a 1-D device tensor")
        if pcm.dtype not in (t.float32, t.int16):
            raise ValueError(f"pcm must be float32 or int16, got dtype {pcm.dtype}")
        off, lengths = prepare.read_tables(clip_offsets, lengths)
        if lengths.shape[0] == 0:
            raise ValueError("a ragged batch needs at least one clip")
        if off.shape[0] != lengths.shape[0]:
            raise ValueError(f"{off.shape[0]} clip_offsets for {lengths.shape[0]} lengths")
        self = cls()
        self._set_tables(lengths, off, sampling_rate)
        if int(off.min()) < 0 or int((off + self.lengths).max()) > int(pcm.numel()):
            raise ValueError(f"a clip lies outside the packed vector of {int(pcm.numel())} elements")
        self.pcm_host, self.device = None, pcm.device
        self.pcm = pcm.contiguous()
        self._upload_tables()
        return self

    def _set_tables(self, lengths, clip_off, sampling_rate=16000):
        """Every table of the batch: a function of the clips' lengths and offsets, and of the window length of the rate's network (the
        only thing that depends on the rate: groups, runs and gx tiles are the same at both).  Pure numpy."""
        if sampling_rate not in SILERO_WINDOWS:
            raise ValueError(f"sampling_rate={sampling_rate}: a ragged Silero batch is built for 16000 or 8000 Hz")
        self.sampling_rate = int(sampling_rate)
        self.window = SILERO_WINDOWS[self.sampling_rate]
        self.lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.clip_off = np.asarray(clip_off, dtype=np.int64).reshape(-1)
        B = int(self.lengths.shape[0])
        if B == 0:
            raise ValueError("a ragged batch needs at least one clip")
        if int(self.lengths.min()) < 1:
            raise ValueError(f"clip {int(np.argmin(self.lengths))} is empty")
        if int(self.lengths.max()) >= 2 ** 31:
            raise ValueError("a clip of 2^31 samples or more does not fit the int32 slot_len table")
        if B >= 2 ** 31 - SILERO_GROUP:
            raise ValueError(f"{B} clips do not fit the int32 slot tables")
        self.windows = (self.lengths + self.window - 1) // self.window
        self.order = np.argsort(-self.windows, kind="stable").astype(np.int32)
        G = (B + SILERO_GROUP - 1) // SILERO_GROUP
        self.groups = G
        self.slot_clip_host = np.full(G * SILERO_GROUP, -1, dtype=np.int32)
        self.slot_clip_host[:B] = self.order
        self.slot_off_host = np.zeros(G * SILERO_GROUP, dtype=np.int64)
        self.slot_off_host[:B] = self.clip_off[self.order]
        self.slot_len_host = np.zeros(G * SILERO_GROUP, dtype=np.int32)
        self.slot_len_host[:B] = self.lengths[self.order]
        self.group_windows = self.windows[self.order[::SILERO_GROUP]]                    # T_g: the group's first (longest) slot
        self.tiles = int(self.group_windows.sum())
        self.n_runs = int(((self.group_windows + SILERO_RUN - 1) // SILERO_RUN).sum())
        if self.tiles >= 2 ** 31 or self.n_runs * SILERO_RUN >= 2 ** 31:
            raise ValueError(f"{self.tiles} gx tiles do not fit the int32 tables of a ragged batch")
        self.wg_tab_host = _wg_tab(self.group_windows)
        self.gx_first_host = np.concatenate([[0], np.cumsum(self.group_windows)]).astype(np.int32)
        grp_min = self.slot_len_host.reshape(G, SILERO_GROUP).min(axis=1)                # 0 for a partial group (an empty slot)
        self.grp_min_len_host = grp_min.astype(np.int32)
        self.probs_first_host = np.concatenate([[0], np.cumsum(self.windows)]).astype(np.int64)
        self.n_windows = int(self.probs_first_host[-1])
        self.workspace_bytes = self.tiles * GX_TILE_BYTES
        self._parts = {}

    def parts(self, cap_bytes):
        """The batch as runs of consecutive groups [(g0, g1), ...] whose gx tiles fit a workspace of cap_bytes each: chosen greedily in
        group order, [(0, groups)] when the whole batch fits.  A single group above the cap raises (its T_g * 32 KB is one clip's own
        length: window spans with carried state are what the rectangular `clips` has and this path does not).  Pure numpy."""
        cap_tiles = int(cap_bytes) // GX_TILE_BYTES
        if int(self.group_windows[0]) > cap_tiles:
            raise ValueError(f"a ragged batch's longest group has {int(self.group_windows[0])} windows: its {int(self.group_windows[0])} gx "
                             f"tiles of 32 KB do not fit a workspace of {int(cap_bytes)} bytes (WORKSPACE_CAP_BYTES) -- a batch runs in "
                             "parts of whole groups, a single group is not split; score that clip with clips(), which spans windows")
        if self.tiles <= cap_tiles:
            return [(0, self.groups)]
        first = self.gx_first_host.astype(np.int64)
        out, g0 = [], 0
        while g0 < self.groups:
            g1 = int(np.searchsorted(first, first[g0] + cap_tiles, side="right")) - 1     # the last g1 with first[g1] - first[g0] <= cap_tiles
            out.append((g0, g1))
            g0 = g1
        return out

    def part_tables(self, parts):
        """One vadx_silero_ragged per part of `parts` (what `parts` returned): the part's gx_first rebased to its first tile and its wg_tab
        over its own groups, numbered from 0 -- built on the host for all parts at once and uploaded once per distinct `parts` --, the
        slot tables and grp_min_len as views of the batch's at the part's first group, and the batch's clips, probs_first and status
        (slot_clip, the scores and the state index the caller's clips)."""
        from . import _lib
        if self.device is None:
            raise ValueError("this batch is host-only: call .to(device) first")
        parts = [(int(a), int(b)) for a, b in parts]
        if parts == [(0, self.groups)]:
            return [self.tables()]
        key = tuple(parts)
        if key not in self._parts:
            t = _lib.require_gpu()
            gx, wg, at = [], [], []
            for g0, g1 in parts:
                if not 0 <= g0 < g1 <= self.groups:
                    raise ValueError(f"part [{g0}, {g1}) is not a run of the batch's {self.groups} groups")
                first = self.gx_first_host[g0:g1 + 1] - self.gx_first_host[g0]
                tab = _wg_tab(self.group_windows[g0:g1])
                at.append((sum(len(a) for a in gx), sum(len(a) for a in wg), int(tab.shape[0]), int(first[-1])))
                gx.append(first.astype(np.int32))
                wg.append(tab)
            self._parts[key] = (t.from_numpy(np.concatenate(gx)).to(self.device), t.from_numpy(np.concatenate(wg)).to(self.device), at)
        gx_dev, wg_dev, at = self._parts[key]
        out = []
        for (g0, g1), (gx_at, wg_at, n_runs, tiles) in zip(parts, at):
            out.append(_lib.SileroRagged(self.slot_off.data_ptr() + 8 * SILERO_GROUP * g0, self.slot_len.data_ptr() + 4 * SILERO_GROUP * g0,
                                         self.slot_clip.data_ptr() + 4 * SILERO_GROUP * g0, gx_dev.data_ptr() + 4 * gx_at,
                                         self.grp_min_len.data_ptr() + 4 * g0, wg_dev.data_ptr() + 8 * wg_at, self.probs_first.data_ptr(),
                                         self.status.data_ptr(), len(self), g1 - g0, n_runs, tiles))
        return out

    def _upload_tables(self):
        from . import _lib
        t = _lib.require_gpu()
        for name in self.TABLES:
            setattr(self, name, t.from_numpy(getattr(self, name + "_host")).to(self.device))
        self.status = t.zeros(1, dtype=t.int32, device=self.device)
        self._parts = {}         # part tables uploaded earlier belong to the tables they were views of

    def to(self, device):
        """Upload the packed vector (once), the tables and a cleared status word."""
        from . import _lib
        t = _lib.require_gpu()
        self.device = t.device(device)
        self.pcm = t.from_numpy(self.pcm_host).to(self.device)
        self._upload_tables()
        return self

    def __len__(self):
        return int(self.lengths.shape[0])

    def tables(self):
        """The vadx_silero_ragged struct of this batch (device pointers: the batch must be on a device)."""
        from . import _lib
        if self.device is None:
            raise ValueError("this batch is host-only: call .to(device) first")
        return _lib.SileroRagged(self.slot_off.data_ptr(), self.slot_len.data_ptr(), self.slot_clip.data_ptr(), self.gx_first.data_ptr(),
                                 self.grp_min_len.data_ptr(), self.wg_tab.data_ptr(), self.probs_first.data_ptr(), self.status.data_ptr(),
                                 len(self), self.groups, self.n_runs, self.tiles)

    def rows(self, packed):
        """per-clip views of a packed per-window vector (the scores): [packed[probs_first[b] : probs_first[b + 1]]]"""
        f = self.probs_first_host
        return [packed[int(f[b]):int(f[b + 1])] for b in range(len(self))]

    def check(self):
        """Raise ValueError when the device refused a slot (one 4-byte read-back; clears the word)."""
        if self.status is not None and int(self.status.item()) != 0:
            self.status.zero_()
            raise ValueError("a clip of the ragged batch lies outside the packed vector: the device did not read it and its scores are NaN")
        return self


# ---- ragged ticks of the Silero streams (include/vadx.h: vadx_silero_stream_plan, vadx_silero_stream_run_ragged) ----
STREAM_MAX_WINDOWS = 256     # windows per stream and tick (vadx_silero_stream_ragged_max_windows)
PLAN_BLOCK = 1024            # streams per workgroup of the device planner (csrc/silero_stream.hip: PLAN_THREADS)


def stream_counts(counts, streams, max_windows=None):
    """A tick's per-stream window counts as int32 [streams], or ValueError: wrong shape, not integers, negative, above max_windows, or
    max_windows above the cap of 256 (None = the cap)."""
    mw = STREAM_MAX_WINDOWS if max_windows is None else int(max_windows)
    if not 1 <= mw <= STREAM_MAX_WINDOWS:
        raise ValueError(f"max_windows={max_windows} must be in [1, {STREAM_MAX_WINDOWS}] (longer catch-ups go through step)")
    c = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts)
    if c.dtype.kind not in "iu":
        raise ValueError(f"counts must be integers, got dtype {c.dtype}")
    if c.shape != (int(streams),):
        raise ValueError(f"counts must have shape ({int(streams)},), got {c.shape}")
    if c.size and int(c.min()) < 0:
        raise ValueError(f"counts[{int(np.argmin(c))}]={int(c.min())} is negative")
    if c.size and int(c.max()) > mw:
        raise ValueError(f"counts[{int(np.argmax(c))}]={int(c.max())} is above max_windows={mw}")
    return c.astype(np.int32)


def window_stream_plan(counts, max_windows=None):
    """The host tables of a ragged tick of window streams (FSMN: vadx_fsmn_stream_windows_ragged / vadx_fsmn_stream_run_ragged), made
    with a cumsum, a repeat and a counting sort over np.bincount of the counts -- no comparison sort.  counts: int [S], 0 <= n_s <=
    max_windows (None = the cap).  -> (first int64 [S + 1] = prefix sum, win_stream int32 [sum n] = the stream of each window row,
    order int32 [S] = np.argsort(-counts, kind="stable"): streams with audio by count descending, idle streams last in index order)."""
    c = np.asarray(counts)
    c = stream_counts(c, c.shape[0] if c.ndim == 1 else -1, max_windows)
    S = int(c.shape[0])
    first = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(c, out=first[1:])
    idx = np.arange(S, dtype=np.int32)
    win_stream = np.repeat(idx, c)
    hist = np.bincount(c)
    order = np.empty(S, dtype=np.int32)
    at = 0
    for v in np.flatnonzero(hist)[::-1].tolist():        # one bucket per count that occurs, largest first; a bucket keeps index order
        order[at:at + int(hist[v])] = idx[c == v]
        at += int(hist[v])
    return first, win_stream, order


class StreamPlan:
    """The host half of a ragged tick's tables (see stream_plan)."""

    def staging(self):
        """counts | bucket_first | gx_first | grp_min_len | wg_tab as one int32 vector, and the element offset of each"""
        parts = [("counts", self.counts), ("bucket_first", self.bucket_first), ("gx_first", self.gx_first),
                 ("grp_min_len", self.grp_min_len), ("wg_tab", self.wg_tab.reshape(-1))]
        at, n = {}, 0
        for name, a in parts:
            at[name] = n
            n += int(a.shape[0])
        return np.concatenate([a for _, a in parts]).astype(np.int32), at


def stream_plan(counts, window, max_windows=None):
    """The group-level plan of a ragged Silero stream tick: everything that is a function of the HISTOGRAM of the counts -- one
    np.bincount, no sort.  counts: int [S] with 0 <= n_s <= max_windows (None = the largest count, at least 1); window 512 or 256.
    -> StreamPlan with streams, window, cw = window // 8, max_windows, counts int32 [S], active = streams with n_s > 0, groups =
    ceil(active / 16), group_windows [G] = the count at sorted position 16 g, gx_first int32 [G + 1], n_runs, tiles, wg_tab int32
    [n_runs, 2] (_wg_tab), grp_min_len int32 [G] = cw + window * the smallest count of a full group (0 for a partial one), n_windows =
    sum(n_s), bucket_first int32 [max_windows + 2] (bucket_first[c] = streams with a count above c = the first sorted position of count
    c) and row = cw + max_windows * window, the staged row length.  `staging()` is the one int32 buffer that goes to the device.
    All-zero counts give groups = 0 and no tables."""
    if int(window) not in SILERO_WINDOWS.values():
        raise ValueError(f"window={window} is not 512 (16 kHz) or 256 (8 kHz)")
    c = np.asarray(counts)
    c = stream_counts(c, c.shape[0] if c.ndim == 1 else -1, STREAM_MAX_WINDOWS)
    if c.shape[0] == 0:
        raise ValueError("a tick needs at least one stream")
    top = int(c.max())
    mw = max(top, 1) if max_windows is None else int(max_windows)
    if not max(top, 1) <= mw <= STREAM_MAX_WINDOWS:
        raise ValueError(f"max_windows={max_windows} must be in [{max(top, 1)}, {STREAM_MAX_WINDOWS}] for these counts")
    p = StreamPlan()
    p.streams, p.window, p.cw, p.max_windows, p.counts = int(c.shape[0]), int(window), int(window) // 8, mw, c
    p.row = p.cw + mw * p.window
    hist = np.bincount(c, minlength=mw + 1).astype(np.int64)
    above = np.zeros(mw + 2, dtype=np.int64)                      # above[c] = streams with a count > c
    above[:mw] = np.cumsum(hist[:0:-1])[::-1]
    p.bucket_first = above.astype(np.int32)
    p.active = int(above[0])
    p.n_windows = int((hist * np.arange(mw + 1)).sum())
    G = (p.active + SILERO_GROUP - 1) // SILERO_GROUP
    p.groups = G
    if G == 0:
        return p

    def count_at(pos):           # the count at sorted positions `pos` (descending): the number of c >= 1 with above[c - 1] > pos
        return np.searchsorted(-above[:mw], -np.asarray(pos, dtype=np.int64), side="left")
    first = np.arange(G, dtype=np.int64) * SILERO_GROUP
    p.group_windows = count_at(first).astype(np.int64)
    p.tiles = int(p.group_windows.sum())
    p.n_runs = int(((p.group_windows + SILERO_RUN - 1) // SILERO_RUN).sum())
    p.wg_tab = _wg_tab(p.group_windows)
    p.gx_first = np.concatenate([[0], np.cumsum(p.group_windows)]).astype(np.int32)
    last = first + SILERO_GROUP - 1
    p.grp_min_len = np.where(last < p.active, p.cw + p.window * count_at(np.minimum(last, p.active - 1)), 0).astype(np.int32)
    p.workspace_bytes = p.tiles * GX_TILE_BYTES
    return p


def stream_slots_mirror(counts, bucket_first, groups, window, max_windows):
    """What vadx_silero_stream_plan writes, computed the way it computes it (numpy): per block of 1024 streams the key histogram, the
    exclusive prefix of those over the blocks, and inside a block the rank of a stream among the earlier streams of its count; position =
    bucket_first[n_s] + prefix + rank.  A count outside [0, max_windows] counts as 0 and raises status bit 1, as a position outside the
    16 * groups slots does (it is not written).  -> (probs_first int64 [S + 1], slot_off int64, slot_len int32, slot_clip int32
    [16 * groups], status).  Slots nobody writes hold slot_clip -2 here (the device leaves them as they were)."""
    c = np.asarray(counts).astype(np.int64).reshape(-1)
    S, mw, win = int(c.shape[0]), int(max_windows), int(window)
    cw, K, slots = win // 8, mw + 1, SILERO_GROUP * int(groups)
    bad = (c < 0) | (c > mw)
    status = 2 if bad.any() else 0
    key = np.where(bad, 0, c)
    bucket_first = np.asarray(bucket_first).astype(np.int64)
    slot_off, slot_len, slot_clip = np.zeros(slots, np.int64), np.zeros(slots, np.int32), np.full(slots, -2, np.int32)
    base = np.zeros(K, dtype=np.int64)                           # streams of each key in the blocks before this one
    for b0 in range(0, S, PLAN_BLOCK):
        k = key[b0:b0 + PLAN_BLOCK]
        onehot = k[:, None] == np.arange(K)[None, :]
        before = np.cumsum(onehot, axis=0) - onehot               # earlier streams of the block, per key
        rank = before[np.arange(len(k)), k]
        pos = bucket_first[k] + base[k] + rank
        s = b0 + np.arange(len(k))
        act = k > 0
        ok = act & (pos >= 0) & (pos < slots)
        if (act & ~ok).any():
            status |= 2
        slot_clip[pos[ok]] = s[ok]
        slot_off[pos[ok]] = s[ok] * (cw + mw * win)
        slot_len[pos[ok]] = cw + k[ok] * win
        base += onehot.sum(axis=0)
    e = np.arange(max(0, int(bucket_first[0])), slots)
    if int(bucket_first[0]) >= 0:
        slot_clip[e], slot_off[e], slot_len[e] = -1, 0, 0
    probs_first = np.concatenate([[0], np.cumsum(key)]).astype(np.int64)
    return probs_first, slot_off, slot_len, slot_clip, status


# ---- ragged ticks of the FireRed streams (include/vadx.h: vadx_firered_stream_tick_ragged) ----
TICK_COLUMNS = 112           # LDS columns of a tick workgroup (csrc/firered.hip: MAX_T) = frames it holds


def chunk_counts(counts, streams, capacity):
    """A tick's per-stream chunk counts as int32 [streams], or ValueError: wrong shape, not integers, negative or above `capacity`
    (= 112 // frames per chunk, vadx_firered_stream_group_max)."""
    cap = int(capacity)
    if not 1 <= cap <= TICK_COLUMNS:
        raise ValueError(f"capacity={capacity} must be in [1, {TICK_COLUMNS}]")
    c = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts)
    if c.dtype.kind not in "iu":
        raise ValueError(f"counts must be integers, got dtype {c.dtype}")
    if c.shape != (int(streams),):
        raise ValueError(f"counts must have shape ({int(streams)},), got {c.shape}")
    if c.size and int(c.min()) < 0:
        raise ValueError(f"counts[{int(np.argmin(c))}]={int(c.min())} is negative")
    if c.size and int(c.max()) > cap:
        raise ValueError(f"counts[{int(np.argmax(c))}]={int(c.max())} is above {cap}, the chunks a workgroup's {TICK_COLUMNS} columns hold")
    return c.astype(np.int32)


def column_stream_plan(counts, capacity, group=0):
    """The host tables of a ragged FireRed tick: which streams share a workgroup's `capacity` chunks of LDS columns.  counts: int [S],
    0 <= n_s <= capacity = 112 // frames.  -> (first int64 [S + 1] = prefix sum of the counts: stream s owns the rows first[s] ..
    first[s + 1] - 1; order int32 [S] = np.argsort(-counts, kind="stable"), whose active prefix (the streams with n_s > 0) is the
    slot_stream table; wg_first int32 [W + 1]: workgroup w serves the positions wg_first[w] .. wg_first[w + 1] - 1 of it).
    Workgroups are formed by next-fit along that order: a workgroup takes consecutive positions while its counts sum to at most
    `capacity` and it holds at most g streams, g = group or, for group = 0, clamp(active // 256, 1, capacity) -- the rule of the
    rectangular tick (a compute unit with a workgroup beats a shared weight load).  The order is a counting sort and the boundaries have
    a closed form per distinct count (at most `capacity` classes): no comparison sort, no loop over streams.  All-zero counts give W = 0."""
    c = np.asarray(counts)
    c = chunk_counts(c, c.shape[0] if c.ndim == 1 else -1, capacity)
    S, cap = int(c.shape[0]), int(capacity)
    if not 0 <= int(group) <= cap:
        raise ValueError(f"group={group} outside [0, {cap}] (0 = the library's choice)")
    first = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(c, out=first[1:])
    idx = np.arange(S, dtype=np.int32)
    hist = np.bincount(c, minlength=1)
    active = S - int(hist[0])
    g = int(group) if group else min(max(active // 256, 1), cap)
    order = np.empty(S, dtype=np.int32)
    bounds = [np.zeros(1, dtype=np.int64)]
    at, used, held = 0, 0, 0                      # sorted position; chunks and streams of the workgroup still open
    for v in np.flatnonzero(hist)[::-1].tolist():        # one class per count that occurs, largest first; a class keeps index order
        n = int(hist[v])
        order[at:at + n] = idx[c == v]
        if v:
            per = min(cap // v, g)                        # streams of this count in a workgroup of its own
            fit = min(n, (cap - used) // v, g - held)     # those the open workgroup still takes
            rest = n - fit
            if rest:
                new = -(-rest // per)
                bounds.append(at + fit + per * np.arange(new, dtype=np.int64))
                last = rest - (new - 1) * per
                used, held = last * v, last
            else:
                used, held = used + fit * v, held + fit
        at += n
    if active:
        bounds.append(np.array([active], dtype=np.int64))
        wg_first = np.concatenate(bounds).astype(np.int32)
    else:
        wg_first = np.zeros(1, dtype=np.int32)
    return first, order, wg_first
