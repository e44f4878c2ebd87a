"""FSMN-VAD on MI355X: the reference's ORT-session boundary + its sliding-window host loop.

Mirrors FSMN/Inference_FSMN_VAD_ONNX.py (session.run feeds/fetches :170-187, loop :156-234) and the
graph FSMN/Export_FSMN_VAD.py:75-101.  `FsmnSession.run` keeps the named-tensor contract
(`audio`, `cache_0..3`, `one_minus_speech_threshold`, `noise_average_dB` -> `score`, `cache_0..3`,
`noisy_dB`) and is batched over independent streams; `FsmnEngine.detect` runs whole clips on device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import checkpoints as _checkpoints
from . import frontend as _frontend
from . import ragged as _ragged
from . import timestamps as _ts
from . import weights as _weights
from .clips import flag_timestamps, pad_batch, pad_to_window_grid  # noqa: F401  (`vadx.fsmn.pad_to_window_grid` is the name callers use)
from .session import Session, _Meta, io_types, require_int16
from .stream import WindowStreamBatch

SAMPLE_RATE = 16000
OUTPUT_FRAME_LENGTH = 160
PROJ, HIST = 128, 19
MAX_FRAMES = 128             # frames per window the kernel's score scratch holds (vadx_fsmn_run); `flags`, ragged batches and streams take 112
LOOP_MAX_FRAMES = 112
LONG_MAX_LENGTH = 9_600_000  # long_windows=True: a 10-minute window, VADX_FSMN_LONG_MAX_FRAMES = 60 001 frames (include/vadx.h)
# The stream record of S streams, mirroring the contract in include/vadx.h, as three sections in this order:
CACHES, HEADER, CARRY = 0, 1, 2      # f32 [S][4][128][19] | u32 [S][8]: word H_PRIMED = has a carry, H_DONE and the next = windows done (u64) | int16 [S][(lb + 1) * 160]
CACHE_BYTES, HDR_BYTES, H_PRIMED, H_DONE = 4 * PROJ * HIST * 4, 8 * 4, 2, 4


def _loop_params(lb, speaking_score=0.5, silence_score=0.5, snr_threshold=10.0, noise_init_dB=30.0, one_minus_speech_threshold=1.0):
    """vadx_fsmn_loop_params from the reference script's constants (FSMN/Inference_FSMN_VAD_ONNX.py:16-23, 79-81, 159-171)."""
    lp = _lib.FsmnLoopParams()
    lp.look_backward = int(lb)
    lp.one_minus_speech_threshold = float(one_minus_speech_threshold)
    lp.noise_db_init = float(np.float32(noise_init_dB + snr_threshold) * np.float32(0.1))
    lp.snr_threshold = float(snr_threshold * 0.1)
    lp.speaking_score, lp.silence_score = float(speaking_score), float(silence_score)
    return lp


def _prep(normalize):
    """The reference's peak normalisation of one clip (any numeric dtype -> int16), or None."""
    return (lambda a: _ts.normalize_to_int16(a.astype(np.float32))) if normalize else None


class FsmnEngine:
    def __init__(self, weights=None, input_audio_length=16000, device="cuda:0", speech_2_noise_ratio=1.0, long_windows=False):
        """long_windows=True: the model of an export with a long INPUT_AUDIO_LENGTH (FSMN/Export_FSMN_VAD.py; the driver reads it back from
        the session, FSMN/Inference_FSMN_VAD_ONNX.py:73-80): any 512 <= input_audio_length <= 9 600 000.  Such an engine runs the long
        entry points (vadx_fsmn_window_stats_long, vadx_fsmn_run_long, vadx_fsmn_clips_long: a window's scores in a global workspace instead
        of LDS) at EVERY length; up to 112 frames its results are bit for bit the default engine's."""
        torch = _lib.require_gpu()
        self.torch = torch
        self.device = torch.device(device)
        w = _checkpoints.resolve("fsmn", weights)
        w = {k: np.ascontiguousarray(np.asarray(v), dtype=np.float32) for k, v in w.items()}
        self.L = int(input_audio_length)
        self.long_windows = bool(long_windows)
        if self.long_windows:
            if not 512 <= self.L <= LONG_MAX_LENGTH:
                raise ValueError(f"input_audio_length={self.L} is outside [512, {LONG_MAX_LENGTH}]: a long window holds at most "
                                 f"{LONG_MAX_LENGTH // OUTPUT_FRAME_LENGTH + 1} frames (10 minutes); longer audio goes on the window grid")
        elif self.L // OUTPUT_FRAME_LENGTH + 1 > MAX_FRAMES:
            raise ValueError(f"input_audio_length={self.L} gives {self.L // OUTPUT_FRAME_LENGTH + 1} frames per window: the FSMN kernel takes at most "
                             f"{MAX_FRAMES} (input_audio_length <= {MAX_FRAMES * OUTPUT_FRAME_LENGTH - 1}); `flags`, ragged batches and streams "
                             f"need at most 112 (input_audio_length <= {112 * OUTPUT_FRAME_LENGTH - 1}).  long_windows=True takes windows of any "
                             f"length up to {LONG_MAX_LENGTH} samples")
        self.fe = _frontend.Frontend("fsmn", self.L, device=device)
        self.T = self.fe.frames
        dims = _lib.FsmnDims()
        dims.input_affine_dim, dims.linear_dim = w["in1_w"].shape[0], w["in2_w"].shape[0]
        dims.output_affine_dim, dims.output_dim = w["out1_w"].shape[0], w["out2_w"].shape[0]
        dims.frames, dims.speech_2_noise_ratio = self.T, float(speech_2_noise_ratio)
        if w["in1_w"].shape[1] != 400 or w["l0_lin_w"].shape[0] != PROJ or w["l0_fir_w"].shape != (PROJ, 20):
            raise ValueError("FSMN weights: input dim 400, proj 128 and lorder 20 are fixed by the reference cache shape")
        self._dims0 = dims
        hw = _lib.FsmnWeightsHost()
        for k in ("in1_w", "in1_b", "in2_w", "in2_b", "out1_w", "out1_b", "out2_w", "out2_b", "cmvn_means", "cmvn_vars"):
            setattr(hw, k, w[k].ctypes.data)
        for l in range(4):
            hw.lin_w[l], hw.fir_w[l] = w[f"l{l}_lin_w"].ctypes.data, w[f"l{l}_fir_w"].ctypes.data
            hw.aff_w[l], hw.aff_b[l] = w[f"l{l}_aff_w"].ctypes.data, w[f"l{l}_aff_b"].ctypes.data
        Lb = _lib.lib()
        self._hw, self._w = hw, w            # (the host arrays behind hw's pointers stay alive with the engine)

        def build(mode):
            """(dims, device blob) of one arithmetic: the blob carries the weight fragments of that arithmetic only"""
            d = _lib.FsmnDims()
            C.memmove(C.byref(d), C.byref(self._dims0), C.sizeof(d))
            d.arithmetic = _lib.GEMM_MODES[mode]
            n = Lb.vadx_fsmn_packed_floats(C.byref(d))
            if n == 0:
                if mode != "f32":             # dims outside the split tile: float32 MFMAs
                    return build("f32")
                raise ValueError("FSMN dims not supported by the HIP kernel (affine dims <= 144, linear/output <= 256)")
            packed = np.zeros(n, dtype=np.float32)
            _lib.check(Lb.vadx_fsmn_pack_host(C.byref(d), C.byref(hw), packed.ctypes.data))
            return d, torch.from_numpy(packed).to(self.device)

        def flag(d, blob):
            f, a = C.c_uint32(0), C.c_float(0.0)
            with torch.cuda.device(self.device):
                _lib.check(Lb.vadx_fsmn_range_flag(C.byref(d), blob.data_ptr(), 1, C.byref(f), C.byref(a), _lib.stream_ptr()))
            return int(f.value), float(a.value)
        self.blobs = _lib.ArithBlobs(build, flag)
        self.blobs.get()                     # pack now: unsupported dims raise here

    @property
    def dims(self):
        return self.blobs.get()[0]

    @property
    def packed(self):
        return self.blobs.get()[1]

    def _workspace(self, rows):
        """The long entry points' scratch for `rows` windows walked at a time (vadx_fsmn_long_workspace_bytes): a window's P(silence) and gate bits."""
        t = self.torch
        return t.empty(_lib.lib().vadx_fsmn_long_workspace_bytes(int(rows), self.T), dtype=t.uint8, device=self.device)

    def _long_grid(self, look_backward_s):
        """`grid` for the long clip loop, whose windows must advance: refused here by name, before anything is padded or launched."""
        lb, stride = self.grid(look_backward_s)
        if lb < 0 or lb >= self.T - 1 or stride <= 0:
            raise ValueError(f"look_backward_s={look_backward_s}: {lb} frames leave no window stride at input_audio_length={self.L}")
        return lb, stride

    # ---- front-end + energy for a [B, N] int16 batch cut into W windows at `stride`
    def features(self, audio_i16, windows_per_clip, stride):
        t = self.torch
        a = audio_i16.to(self.device).contiguous()
        B = a.shape[0]
        W = int(windows_per_clip)
        fe = self.fe
        logmel = t.empty((B * W, self.T, 80), dtype=t.float32, device=self.device)
        means = t.empty((B * W,), dtype=t.float32, device=self.device)
        db = t.empty((B * W, self.T), dtype=t.float32, device=self.device)
        L = _lib.lib()
        with t.cuda.device(self.device):
            # window means + frame energies in one pass over the PCM, then the log-mel front-end with those means
            if self.long_windows:             # a grid of (window, block of frames); the windows' 64-bit sums are its workspace
                sums = t.empty((B * W,), dtype=t.int64, device=self.device)
                _lib.check(L.vadx_fsmn_window_stats_long(a.data_ptr(), _lib.row_stride(a), int(stride), B, W, self.L, self.T, means.data_ptr(),
                                                         db.data_ptr(), sums.data_ptr(), _lib.stream_ptr()))
            else:
                _lib.check(L.vadx_fsmn_window_stats(a.data_ptr(), _lib.row_stride(a), int(stride), B, W, self.L, self.T, means.data_ptr(),
                                                    db.data_ptr(), _lib.stream_ptr()))
            _lib.check(L.vadx_frontend_logmel_means(C.byref(fe.cfg), fe.packed.data_ptr(), fe.mel_kb.ctypes.data, a.data_ptr(),
                                                    _lib.row_stride(a), int(stride), B, W, means.data_ptr(), logmel.data_ptr(),
                                                    _lib.stream_ptr()))
        return logmel, db

    def run(self, audio_i16, caches, thr, noise_db, return_psil=False):
        """One boundary call for B streams: audio int16 [B,L]; caches 4 x [B,128,19]; thr, noise_db [B]."""
        t = self.torch
        a = audio_i16.to(self.device)
        B = a.shape[0]
        if a.shape[1] != self.L:
            raise ValueError(f"audio must be [B,{self.L}], got {tuple(a.shape)}")
        logmel, db = self.features(a, 1, self.L)
        cin = [c.to(self.device, t.float32).contiguous() for c in caches]
        for c in cin:
            if tuple(c.shape) != (B, PROJ, HIST):
                raise ValueError(f"cache must be [{B},{PROJ},{HIST}], got {tuple(c.shape)}")
        cout = [t.empty_like(c) for c in cin]
        thr = t.as_tensor(thr, dtype=t.float32, device=self.device).reshape(-1).expand(B).contiguous()
        nz = t.as_tensor(noise_db, dtype=t.float32, device=self.device).reshape(-1).expand(B).contiguous()
        score = t.empty((B, self.T), dtype=t.uint8, device=self.device)
        noisy = t.empty((B,), dtype=t.float32, device=self.device)
        psil = t.empty((B, self.T), dtype=t.float32, device=self.device) if return_psil else None
        pin = (C.c_void_p * 4)(*[c.data_ptr() for c in cin])
        pout = (C.c_void_p * 4)(*[c.data_ptr() for c in cout])
        ws = self._workspace(B) if self.long_windows else None

        def launch(mode, dims, packed):
            with t.cuda.device(self.device):
                args = (C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), C.byref(pin), C.byref(pout), thr.data_ptr(),
                        nz.data_ptr(), B, score.data_ptr(), noisy.data_ptr(), None if psil is None else psil.data_ptr())
                if ws is None:
                    _lib.check(_lib.lib().vadx_fsmn_run(*args, _lib.stream_ptr()))
                else:
                    _lib.check(_lib.lib().vadx_fsmn_run_long(*args, ws.data_ptr(), _lib.stream_ptr()))
            return (score, cout, noisy, psil) if return_psil else (score, cout, noisy)
        return self.blobs.guarded(launch)

    # ---- whole clips
    def grid(self, look_backward_s=0.3):
        lb = int(look_backward_s * SAMPLE_RATE // OUTPUT_FRAME_LENGTH)
        stride = self.L - (lb + 1) * OUTPUT_FRAME_LENGTH
        return lb, stride

    def flags(self, padded_i16, windows_per_clip, *, look_backward_s=0.3, speaking_score=0.5, silence_score=0.5,
              snr_threshold=10.0, noise_init_dB=30.0, one_minus_speech_threshold=1.0, return_noise=False):
        """padded_i16 [B, (W-1)*stride + L] int16 on the window grid -> silence flags u8 [B, W*(T-lb)+lb]."""
        t = self.torch
        # lb may be 0: W*T flags, no tail (Inference_FSMN_VAD_ONNX.py:79-86)
        lb, stride = self._long_grid(look_backward_s) if self.long_windows else self.grid(look_backward_s)
        a = padded_i16.to(self.device).contiguous()
        B, W = a.shape[0], int(windows_per_clip)
        logmel, db = self.features(a, W, stride)
        lp = _loop_params(lb, speaking_score, silence_score, snr_threshold, noise_init_dB, one_minus_speech_threshold)
        nflags = W * (self.T - lb) + lb
        flags = t.empty((B, nflags), dtype=t.uint8, device=self.device)
        cache = t.empty((B, 4, PROJ, HIST), dtype=t.float32, device=self.device)
        trace = t.empty((B, W), dtype=t.float32, device=self.device) if return_noise else None
        ws = self._workspace(B) if self.long_windows else None

        def launch(mode, dims, packed):
            with t.cuda.device(self.device):
                if ws is None:
                    _lib.check(_lib.lib().vadx_fsmn_clips(C.byref(dims), packed.data_ptr(), logmel.data_ptr(),
                                                          db.data_ptr(), B, W, C.byref(lp), cache.data_ptr(), flags.data_ptr(),
                                                          None if trace is None else trace.data_ptr(), _lib.stream_ptr()))
                else:                         # the rectangular batch of the long loop: no window table, W windows for every clip
                    _lib.check(_lib.lib().vadx_fsmn_clips_long(C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), B, B * W, W,
                                                               None, None, C.byref(lp), cache.data_ptr(), flags.data_ptr(), nflags,
                                                               None if trace is None else trace.data_ptr(), ws.data_ptr(), _lib.stream_ptr()))
            return (flags, trace) if return_noise else flags
        return self.blobs.guarded(launch)

    def flags_from_host(self, host_padded_i16, windows_per_clip, chunk_clips=256, feed=None, **loop_kw):
        """`flags` fed from HOST memory (int16 [B, (W-1)*stride + L], ideally pinned: vadx.feed.pin): chunks of clips are uploaded on
        a copy stream while the previous chunk's launches run (vadx.feed.HostPcmFeed); bit-identical to `flags` of the resident batch."""
        from . import feed as _feed
        f = feed or _feed.HostPcmFeed(self.device, host_padded_i16.shape[1], chunk_clips)
        return _feed.cat_results(f.map([host_padded_i16], lambda a: self.flags(a, windows_per_clip, **loop_kw)))

    def ragged(self, clips, pad_noise=None, normalize=True, look_backward_s=0.3, device=True):
        """The packed batch of `clips` (list of 1-D arrays of any lengths) on this engine's window grid (vadx.ragged.RaggedBatch):
        peak-normalised like the reference (normalize) and padded per clip with pad_noise row b.  device=None keeps it on the host."""
        if self.long_windows and self.L % 8:
            raise ValueError(f"input_audio_length={self.L} must be a multiple of 8 for a ragged batch: the window gather moves 16-byte runs")
        stride = (self._long_grid(look_backward_s) if self.long_windows else self.grid(look_backward_s))[1]
        return _ragged.RaggedBatch.from_clips(clips, self.L, stride, pad_noise, _prep(normalize),
                                              self.device if device is True else device)

    def ragged_packed(self, pcm, clip_offsets, lengths, pad_noise=None, normalize=True, look_backward_s=0.3):
        """`ragged` for clips that already lie in device memory (RaggedBatch.from_packed: normalised, padded and packed on the device, bit
        for bit what `ragged` builds from the same clips and noise)."""
        if self.long_windows and self.L % 8:
            raise ValueError(f"input_audio_length={self.L} must be a multiple of 8 for a ragged batch: the window gather moves 16-byte runs")
        stride = (self._long_grid(look_backward_s) if self.long_windows else self.grid(look_backward_s))[1]
        return _ragged.RaggedBatch.from_packed(pcm, clip_offsets, lengths, self.L, stride, pad_noise, "peak" if normalize else None,
                                               device=self.device)

    def flags_ragged(self, rb, *, order=None, return_noise=False, look_backward_s=0.3, speaking_score=0.5, silence_score=0.5,
                     snr_threshold=10.0, noise_init_dB=30.0, one_minus_speech_threshold=1.0):
        """`flags` for a RaggedBatch on this engine's grid: one gather, the unchanged front-end over sum(W) windows, one
        vadx_fsmn_clips_ragged launch -> (flags u8 [B, max W * (T-lb) + lb], nflags int64 [B] (host)[, noise trace f32 [sum W]]).
        Row b holds clip b's nflags[b] = W_b * (T-lb) + lb flags -- bit for bit `flags(padded_b[None], W_b)` -- then 255.
        order: None = rb.order (longest clip first), "identity" = clip b on workgroup b, or an int32 permutation of the clips.
        A host-only batch (device=None) is uploaded first, in place: `rb.to(self.device)` turns its pcm and tables into device tensors."""
        t = self.torch
        lb, stride = self._long_grid(look_backward_s) if self.long_windows else self.grid(look_backward_s)
        if rb.window != self.L or rb.stride != stride:
            raise ValueError(f"the batch was packed for windows of {rb.window} every {rb.stride} samples, this call needs {self.L} every {stride}")
        if rb.device is None:
            rb.to(self.device)
        B, nwin, maxw = len(rb), rb.n_windows, rb.max_windows
        if order is None:
            order_d = rb.order
        elif isinstance(order, str):
            if order != "identity":
                raise ValueError(f"order must be None, 'identity' or a permutation, got {order!r}")
            order_d = None
        else:
            o = np.asarray(order.cpu() if t.is_tensor(order) else order).astype(np.int32).reshape(-1)
            if not np.array_equal(np.sort(o), np.arange(B)):
                raise ValueError(f"order must be a permutation of the {B} clips")
            order_d = t.from_numpy(o).to(self.device)
        logmel, db = self.features(rb.gather(), 1, self.L)
        lp = _loop_params(lb, speaking_score, silence_score, snr_threshold, noise_init_dB, one_minus_speech_threshold)
        slide = self.T - lb
        stride_f = maxw * slide + lb
        nflags = rb.windows.astype(np.int64) * slide + lb
        flags = t.empty((B, stride_f), dtype=t.uint8, device=self.device)
        cache = t.empty((B, 4, PROJ, HIST), dtype=t.float32, device=self.device)
        trace = t.empty((nwin,), dtype=t.float32, device=self.device) if return_noise else None
        ws = self._workspace(B) if self.long_windows else None

        def launch(mode, dims, packed):
            with t.cuda.device(self.device):
                args = (C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), B, nwin, maxw, rb.win_first.data_ptr(),
                        None if order_d is None else order_d.data_ptr(), C.byref(lp), cache.data_ptr(), flags.data_ptr(), stride_f,
                        None if trace is None else trace.data_ptr())
                if ws is None:
                    _lib.check(_lib.lib().vadx_fsmn_clips_ragged(*args, _lib.stream_ptr()))
                else:
                    _lib.check(_lib.lib().vadx_fsmn_clips_long(*args, ws.data_ptr(), _lib.stream_ptr()))
            return (flags, nflags, trace) if return_noise else (flags, nflags)
        return self.blobs.guarded(launch)

    def detect(self, clips_i16, pad_noise=None, fusion_threshold=0.3, min_speech_duration=0.2, normalize=True, **loop_kw):
        """Equal-length clips int16 [B,N] (host numpy) -> per clip [(start_s, end_s)], as the reference
        script would print for each.  pad_noise: standard-normal array [B, >=pad] replacing the
        reference's unseeded np.random.normal tail padding (explicit so results are reproducible).
        A LIST (or tuple) of 1-D clips of any lengths runs as one ragged batch (`flags_ragged`); clip b's result is that of
        `detect(clip_b[None, :], pad_noise=row_b[None, :])[0]`."""
        look_backward_s = loop_kw.get("look_backward_s", 0.3)
        if isinstance(clips_i16, _ragged.RaggedBatch):          # packed already (`ragged`, or RaggedBatch.from_packed on the device)
            flags, nflags = self.flags_ragged(clips_i16, **loop_kw)
        elif isinstance(clips_i16, (list, tuple)):
            flags, nflags = self.flags_ragged(self.ragged(clips_i16, pad_noise, normalize, look_backward_s), **loop_kw)
        else:
            stride = (self._long_grid(look_backward_s) if self.long_windows else self.grid(look_backward_s))[1]
            padded, W = pad_batch(clips_i16, self.L, stride, pad_noise, _prep(normalize))
            flags = self.flags(self.torch.from_numpy(padded), W, **loop_kw)
            nflags = [flags.shape[1]] * flags.shape[0]
        flags = flags.cpu().numpy()
        return [flag_timestamps(flags[b, :nflags[b]], OUTPUT_FRAME_LENGTH / SAMPLE_RATE, fusion_threshold, min_speech_duration)
                for b in range(flags.shape[0])]

    def detect_table(self, clips_i16, pad_noise=None, fusion_threshold=0.3, min_speech_duration=0.2, normalize=True, sample_rule="nearest",
                     **loop_kw):
        """`detect` with the flags staying on the device: the same launches, then one vadx_timestamps_flags launch -> a
        vadx.tstable.TimestampTable whose `lists()` is what `detect` returns and whose `chunks_table()` goes straight to
        vadx.chunks.collect_chunks_batch (sample rows at 16 kHz, by `sample_rule`)."""
        from . import tstable
        look_backward_s = loop_kw.get("look_backward_s", 0.3)
        if isinstance(clips_i16, _ragged.RaggedBatch):          # packed already (`ragged`, or RaggedBatch.from_packed on the device)
            flags, nflags = self.flags_ragged(clips_i16, **loop_kw)
        elif isinstance(clips_i16, (list, tuple)):
            flags, nflags = self.flags_ragged(self.ragged(clips_i16, pad_noise, normalize, look_backward_s), **loop_kw)
        else:
            stride = (self._long_grid(look_backward_s) if self.long_windows else self.grid(look_backward_s))[1]
            padded, W = pad_batch(clips_i16, self.L, stride, pad_noise, _prep(normalize))
            flags, nflags = self.flags(self.torch.from_numpy(padded), W, **loop_kw), None
        return tstable.from_flags(flags, nflags, OUTPUT_FRAME_LENGTH / SAMPLE_RATE, fusion_threshold, min_speech_duration, SAMPLE_RATE, sample_rule)


    def stream_detect(self, clips, windows_per_tick=1, pad_noise=None, normalize=True, fusion_threshold=0.3, min_speech_duration=0.2,
                      **loop_kw):
        """A list of 1-D int16 clips of any lengths run as the live streams of one FsmnStreamBatch with RAGGED ticks until the longest is
        done: every clip is normalised and padded to its own window grid exactly as `detect(list)` does, and stream s advances by
        min(windows_per_tick, windows left) windows per tick (0 once it is through) -> what `detect(list)` returns.  The clips are whole
        here; a caller with truly live audio drives FsmnStreamBatch.step_ragged itself and pads a stream's end."""
        k = int(windows_per_tick)
        if k < 1:
            raise ValueError(f"windows_per_tick={windows_per_tick} must be at least 1")
        look_backward_s = loop_kw.pop("look_backward_s", 0.3)
        rb = self.ragged(list(clips), pad_noise, normalize, look_backward_s, device=None)
        S = len(rb)
        sb = FsmnStreamBatch(self, S, look_backward_s=look_backward_s, **loop_kw)
        left, pos = rb.windows.astype(np.int64), rb.clip_off.astype(np.int64)
        parts, tails = [[] for _ in range(S)], [None] * S
        while left.any():
            counts = np.minimum(left, k)
            need = sb.samples_needed_ragged(counts)
            x = np.zeros((S, int(need.max())), dtype=np.int16)
            for s in np.flatnonzero(counts).tolist():
                x[s, :need[s]] = rb.pcm_host[pos[s]:pos[s] + need[s]]
            pos, left = pos + need, left - counts
            flags, tail, first = sb.step_ragged(x, counts, max_windows=k)
            for s in np.flatnonzero(counts).tolist():
                parts[s].append(flags[first[s]:first[s + 1]].reshape(-1))
                if left[s] == 0:
                    tails[s] = tail[s]
        return [flag_timestamps(self.torch.cat(parts[s] + [tails[s]]).cpu().numpy(), OUTPUT_FRAME_LENGTH / SAMPLE_RATE, fusion_threshold,
                                min_speech_duration) for s in range(S)]


class FsmnSession(Session):
    """onnxruntime.InferenceSession look-alike for the FSMN graph (names/dtypes/shapes of
    FSMN/Export_FSMN_VAD.py:115-134); feeds may carry a leading batch of independent streams.

    io_dtype="float16" is the drop-in for the reference's fp16-optimised model (FSMN/Optimize_ONNX.py:48-54 converts with
    keep_io_types=False, so caches, thresholds and noisy_dB cross the boundary as float16 and the driver builds float16
    feeds when `_inputs_meta[1].type` says so, Inference_FSMN_VAD_ONNX.py:40,157-164).  Only the BOUNDARY is half precision
    here: feeds are widened to float32, every kernel computes in float32 (>= the reference's precision), fetches are
    rounded to float16 once.  Against the float32 session fed the same (float16-representable) values the uint8 score
    is identical and caches / noisy_dB differ by that single rounding (<= 2^-11 relative)."""

    def __init__(self, weights=None, input_audio_length=16000, device="cuda:0", io_dtype="float32", speech_2_noise_ratio=1.0, long_windows=False):
        """long_windows=True: any 512 <= input_audio_length <= 9 600 000 (FsmnEngine), reported as `[1,1,L]` and `[T]` like any other."""
        self.io_dtype, ftype = io_types(io_dtype)
        self.engine = FsmnEngine(weights, input_audio_length, device, speech_2_noise_ratio, long_windows=long_windows)
        L, T = self.engine.L, self.engine.T
        cache = [1, PROJ, HIST, 1]
        self._inputs_meta = [_Meta("audio", [1, 1, L], "tensor(int16)")] + \
            [_Meta(f"cache_{i}", cache, ftype) for i in range(4)] + \
            [_Meta("one_minus_speech_threshold", [1], ftype), _Meta("noise_average_dB", [1], ftype)]
        self._outputs_meta = [_Meta("score", [T], "tensor(uint8)")] + \
            [_Meta(f"cache_{i}", cache, ftype) for i in range(4)] + [_Meta("noisy_dB", [], ftype)]

    def run(self, output_names, feeds):
        t = self.engine.torch
        audio = np.asarray(feeds["audio"])
        require_int16(audio)
        for name in [f"cache_{i}" for i in range(4)] + ["one_minus_speech_threshold", "noise_average_dB"]:
            got = np.asarray(feeds[name]).dtype
            if got != self.io_dtype:       # onnxruntime refuses a feed of the wrong element type; so does this session
                raise ValueError("Unexpected input data type. Actual: (tensor(%s)) , expected: (tensor(%s))"
                                 % (got, "float16" if self.io_dtype == np.float16 else "float"))
        audio = audio.reshape(-1, audio.shape[-1])
        B = audio.shape[0]
        caches = [t.from_numpy(np.ascontiguousarray(np.asarray(feeds[f"cache_{i}"], dtype=np.float32)).reshape(B, PROJ, HIST))
                  for i in range(4)]
        score, cout, noisy = self.engine.run(t.from_numpy(np.ascontiguousarray(audio)), caches,
                                             np.asarray(feeds["one_minus_speech_threshold"], dtype=np.float32),
                                             np.asarray(feeds["noise_average_dB"], dtype=np.float32))
        io = self.io_dtype
        res = {"score": score.cpu().numpy().reshape(-1) if B == 1 else score.cpu().numpy(),
               "noisy_dB": (noisy.cpu().numpy().reshape(()) if B == 1 else noisy.cpu().numpy()).astype(io)}
        for i in range(4):
            res[f"cache_{i}"] = cout[i].cpu().numpy().reshape(B, PROJ, HIST, 1).astype(io)
        # outputs are name-addressed; the reference script's positional names o0..o5 map in graph order
        order = ["score", "cache_0", "cache_1", "cache_2", "cache_3", "noisy_dB"]
        names = order if output_names is None else output_names
        return [res[n] for n in names]


class FsmnStreamBatch(WindowStreamBatch):
    """`streams` live FSMN streams on the device (vadx_fsmn_stream_windows + vadx_fsmn_stream_run): every `step` advances each stream by
    k analysis windows.  What the reference loop carries (FSMN/Inference_FSMN_VAD_ONNX.py:162-167, 176-234) -- the four FIR caches, the
    noise floor, the vote's `silence` and the (look_backward + 1) * 160 samples two windows share -- stays in the device `record`
    (DESIGN.md "Stream batches"; its first S*4*128*19 floats are the FIR caches [S,4,128,19], then the headers, then the carries); nothing
    crosses to the host per window.  Per stream, the flags of successive ticks followed by the last tick's tail are bit for bit
    `FsmnEngine.flags` over the concatenated audio.  On "h2" every tick reads the range flag and, when it is raised, recomputes the tick
    on "split" from the same record into the same record.  `step_ragged` is the tick in which every stream advances by its own number of
    windows (vadx_fsmn_stream_windows_ragged + vadx_fsmn_stream_run_ragged; 0 = no audio, which costs nothing); the record is the same, so
    the two forms interchange tick by tick.

    A stream's audio must end on the window grid: padding the end of a stream with noise is the caller's job (`pad_to_window_grid`), as
    it is for `flags`."""

    frame_s = OUTPUT_FRAME_LENGTH / SAMPLE_RATE

    def __init__(self, engine, streams, *, look_backward_s=0.3, speaking_score=0.5, silence_score=0.5, snr_threshold=10.0,
                 noise_init_dB=30.0, one_minus_speech_threshold=1.0):
        if not isinstance(engine, FsmnEngine):
            raise TypeError("FsmnStreamBatch needs a vadx.fsmn.FsmnEngine")
        if engine.long_windows and engine.T > LOOP_MAX_FRAMES:        # live streams want short windows
            raise ValueError(f"FsmnStreamBatch: the engine's input_audio_length={engine.L} gives {engine.T} frames per window; the stream "
                             f"kernel takes at most {LOOP_MAX_FRAMES} (input_audio_length <= {LOOP_MAX_FRAMES * OUTPUT_FRAME_LENGTH - 1}): "
                             f"long windows are not served as live streams")
        self.lb, self.stride = engine.grid(look_backward_s)
        if self.lb < 0 or self.stride <= 0 or self.lb >= engine.T - 2:
            raise ValueError(f"look_backward_s={look_backward_s}: {self.lb} frames leave no window stride")
        super().__init__(engine, streams, _lib.lib().vadx_fsmn_stream_state_bytes(int(streams), self.lb))
        self.slide = engine.T - self.lb
        self.carry = engine.L - self.stride              # (lb + 1) * 160 samples
        self._lp = _loop_params(self.lb, speaking_score, silence_score, snr_threshold, noise_init_dB, one_minus_speech_threshold)
        self._wbuf = None
        self.noise_trace = None                                  # float32 [S, windows] of the last tick: noise floor after each window

    def _section(self, record, i):
        """Section i (CACHES, HEADER or CARRY) of `record` as a uint8 view [S, that section's bytes per stream]."""
        per = (CACHE_BYTES, HDR_BYTES, self.carry * 2)
        at = self.streams * sum(per[:i])
        return record[at:at + self.streams * per[i]].view(self.streams, per[i])

    @property
    def caches(self):
        return self._section(self.record, CACHES).view(self.engine.torch.float32).view(self.streams, 4, PROJ, HIST)

    def stream_bytes(self, record, s):
        """Every byte of `record` that belongs to stream s (caches, header, carry), as one uint8 tensor."""
        return self.engine.torch.cat([self._section(record, i)[s] for i in (CACHES, HEADER, CARRY)])

    @property
    def windows_done(self):
        """int64 [S] (host): windows each stream has done since its reset, read from the device record.  Flag i of a stream's next tick
        is frame windows_done * (T - look_backward) + i of its audio, 10 ms per frame."""
        return self._section(self.record, HEADER).view(self.engine.torch.int64)[:, H_DONE // 2].cpu().numpy()

    def _primed_words(self):
        return self._section(self.record, HEADER).view(self.engine.torch.int32)[:, H_PRIMED]

    def step(self, samples_i16, windows=1, reset=None, active=None):
        """samples_i16 int16 [S, >= samples_needed(windows, reset).max() over the active streams] (host or device, numpy or torch), each
        row holding that stream's NEW samples from column 0 -> device tensors (flags u8 [S, windows*(T-lb)], tail u8 [S, lb]): the
        voted silence flags of this tick's windows, and what the reference's plain rule would append if the stream ended here.
        reset / active: bool [S] or None; an inactive stream keeps its record bit for bit, ignores a reset, and reads 255."""
        eng, t = self.engine, self.engine.torch
        k, S, L = int(windows), self.streams, self.engine.L
        x = self._samples(samples_i16)
        act, _, reset_d, act_d, src, dst = self._begin(reset, active)
        need = int(self.samples_needed(k, reset)[act].max(initial=0))       # refuses windows < 1; an active stream is fresh without a carry or with a reset
        if x.shape[1] < need:
            raise ValueError(f"samples rows hold {x.shape[1]} samples, this tick needs {need} (samples_needed)")
        x = x.to(eng.device)
        if x.shape[1] < 8 or x.stride(1) != 1 or (S > 1 and x.stride(0) % 8) or x.data_ptr() % 16:
            pad = t.zeros((S, (x.shape[1] + 7) // 8 * 8 + 8), dtype=t.int16, device=eng.device)      # 16-byte rows for the window kernel
            pad[:, :x.shape[1]] = x
            x = pad
        row = int(x.stride(0)) if S > 1 else int(x.shape[1]) // 8 * 8
        if self._wbuf is None or self._wbuf.numel() < S * k * L:
            self._wbuf = t.empty(S * k * L, dtype=t.int16, device=eng.device)
        wbuf = self._wbuf[:S * k * L].view(S, k * L)
        Lb = _lib.lib()
        with t.cuda.device(eng.device):
            _lib.check(Lb.vadx_fsmn_stream_windows(x.data_ptr(), row, S, k, L, self.lb, None if reset_d is None else reset_d.data_ptr(),
                                                   None if act_d is None else act_d.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                                   wbuf.data_ptr(), _lib.stream_ptr()))
        logmel, db = eng.features(wbuf, k, L)
        flags = t.empty((S, k * self.slide), dtype=t.uint8, device=eng.device)
        tail = t.empty((S, self.lb), dtype=t.uint8, device=eng.device)
        trace = t.empty((S, k), dtype=t.float32, device=eng.device)

        def launch(mode, dims, packed):
            with t.cuda.device(eng.device):
                _lib.check(Lb.vadx_fsmn_stream_run(C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), S, k,
                                                   C.byref(self._lp), None if reset_d is None else reset_d.data_ptr(),
                                                   None if act_d is None else act_d.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                                   flags.data_ptr(), tail.data_ptr() if self.lb else None, trace.data_ptr(),
                                                   _lib.stream_ptr()))
        eng.blobs.guarded(launch)
        self._end(act)
        self.noise_trace = trace
        return flags, tail

    def _ragged_samples(self, samples, counts, reset, max_windows):
        """The samples and counts of a ragged tick -> (x int16 [S, n] tensor where it is, counts int32 [S]).  A list of S 1-D host arrays
        gives its own counts: the lengths must be what samples_needed_ragged gives for some count."""
        S = self.streams
        if isinstance(samples, (list, tuple)):
            if len(samples) != S:
                raise ValueError(f"samples lists {len(samples)} arrays for {S} streams")
            rows = [np.asarray(r).reshape(-1) for r in samples]
            for s, r in enumerate(rows):
                if r.dtype != np.int16:
                    raise ValueError(f"samples[{s}] must be int16, got {r.dtype}")
            got = self._counts_of_lengths([r.shape[0] for r in rows], reset)
            if counts is not None and not np.array_equal(np.asarray(counts).reshape(-1), got):
                raise ValueError("counts disagree with the lengths of the listed samples")
            counts = _ragged.stream_counts(got, S, max_windows)
            x = np.zeros((S, max(max(r.shape[0] for r in rows), 8)), dtype=np.int16)
            for s, r in enumerate(rows):
                x[s, :r.shape[0]] = r
        else:
            if counts is None:
                raise ValueError("step_ragged needs counts with a [S, n] array")
            counts = _ragged.stream_counts(counts, S, max_windows)
            x = samples
        return self._samples(x), counts

    def step_ragged(self, samples, counts=None, reset=None, max_windows=None):
        """A tick in which stream s advances by counts[s] windows, 0 <= counts[s] <= max_windows (None = the cap of 256 a ragged tick
        has, vadx_fsmn_stream_ragged_max_windows): the work is sum(counts) windows.  samples: int16 [S, >=
        samples_needed_ragged(counts, reset).max()] (host or device, numpy or torch), row s holding that stream's new samples from
        column 0 -- or a list of S 1-D host arrays whose lengths ARE what samples_needed_ragged gives for some count (the counts then
        come from the lengths).  -> (flags u8 [sum(counts), T - lb] on the device: stream s owns rows first[s] .. first[s + 1] - 1;
        tail u8 [S, lb]: what the plain rule would append if the stream ended with ITS last window of this tick, 255 for a stream
        without audio; first: host int64 [S + 1]).  self.noise_trace becomes float32 [sum(counts)].  A stream with count 0 costs
        nothing: it keeps its record and its pending reset, and a reset request for it is ignored.  A tick whose counts are all 0
        launches nothing and leaves the current record where it is.  Bad counts raise ValueError before anything is launched.  `step`
        and `step_ragged` interchange tick by tick (one record); `step` stays the path for uniform ticks."""
        eng, t = self.engine, self.engine.torch
        S, L = self.streams, self.engine.L
        x, counts = self._ragged_samples(samples, counts, reset, max_windows)
        first, win_stream, order = _ragged.window_stream_plan(counts, max_windows)
        n = int(first[-1])
        if n == 0:                   # nobody delivered audio: no launch; the record, the pending resets and the trace's meaning stay
            self.noise_trace = t.empty(0, dtype=t.float32, device=eng.device)
            tail = t.from_numpy(np.full((S, self.lb), 255, dtype=np.uint8)).to(eng.device)
            return t.empty((0, self.slide), dtype=t.uint8, device=eng.device), tail, first
        need = int(self.samples_needed_ragged(counts, reset).max())
        if x.shape[1] < need:
            raise ValueError(f"samples rows hold {x.shape[1]} samples, this tick needs {need} (samples_needed_ragged)")
        act = counts > 0
        _, _, reset_d, _, src, dst = self._begin(reset, act, upload_active=False)
        x = x.to(eng.device)
        if x.shape[1] < 8 or x.stride(1) != 1 or (S > 1 and x.stride(0) % 8) or x.data_ptr() % 16:
            pad = t.zeros((S, (x.shape[1] + 7) // 8 * 8 + 8), dtype=t.int16, device=eng.device)      # 16-byte rows for the window kernel
            pad[:, :x.shape[1]] = x
            x = pad
        row = int(x.stride(0)) if S > 1 else int(x.shape[1]) // 8 * 8
        mw = int(counts.max())
        # the tick's tables in ONE copy: counts | win_first | order | win_stream | status (a zero the copy writes)
        tab = t.from_numpy(np.concatenate([counts, first.astype(np.int32), order, win_stream, np.zeros(1, np.int32)]).astype(np.int32)).to(eng.device)
        p_counts = tab.data_ptr()
        p_first, p_order, p_wst = p_counts + 4 * S, p_counts + 4 * (2 * S + 1), p_counts + 4 * (3 * S + 1)
        p_status = p_wst + 4 * n
        if self._wbuf is None or self._wbuf.numel() < n * L:
            self._wbuf = t.empty(max(n, S) * L, dtype=t.int16, device=eng.device)
        wbuf = self._wbuf[:n * L].view(n, L)
        Lb = _lib.lib()
        rst = None if reset_d is None else reset_d.data_ptr()
        with t.cuda.device(eng.device):
            _lib.check(Lb.vadx_fsmn_stream_windows_ragged(x.data_ptr(), row, S, n, mw, L, self.lb, p_counts, p_first, p_wst, rst,
                                                          src.data_ptr(), dst.data_ptr(), wbuf.data_ptr(), p_status, _lib.stream_ptr()))
        logmel, db = eng.features(wbuf, 1, L)
        flags = t.empty((n, self.slide), dtype=t.uint8, device=eng.device)
        tail = t.empty((S, self.lb), dtype=t.uint8, device=eng.device)
        trace = t.empty((n,), dtype=t.float32, device=eng.device)

        def launch(mode, dims, packed):
            with t.cuda.device(eng.device):
                _lib.check(Lb.vadx_fsmn_stream_run_ragged(C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), S, n, mw,
                                                          C.byref(self._lp), p_counts, p_first, p_order, rst, src.data_ptr(), dst.data_ptr(),
                                                          flags.data_ptr(), tail.data_ptr() if self.lb else None, trace.data_ptr(),
                                                          p_status, _lib.stream_ptr()))
        eng.blobs.guarded(launch)
        self._end(act)
        self.noise_trace = trace
        return flags, tail, first
