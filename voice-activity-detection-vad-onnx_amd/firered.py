"""FireRedVAD / FireRedAED (non-stream) and FireRed Stream-VAD on MI355X: ORT-session boundary + the
non-overlapping window loop of FireRedVAD/Inference_FireRed_ONNX.py:523-613 (VAD) / :620-742 (AED, odim = 3)
and the cache-carrying chunk loop of :744-822 (Stream-VAD)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import checkpoints as _checkpoints
from . import frontend as _frontend
from . import ragged as _ragged
from . import vadpost as _vadpost
from . import weights as _weights
from .clips import gather_tracks, pad_batch, track_segments, track_table
from .session import Session, _Meta, require_int16
from .stream import StreamBatch

SAMPLE_RATE, WINDOW_LENGTH, HOP_LENGTH = 16000, 400, 160
STREAM_CHUNK_SAMPLES = 2560          # 160 ms (Export_FireRedVAD.py:52-53)
MAX_FRAMES = 112                     # frames of one window / stream chunk the kernels keep in LDS (csrc/firered.hip: MAX_T)
LONG_MAX_FRAMES = _lib.FIRERED_LONG_MAX_FRAMES      # frames of one window of the long path: 3600 s, the reference driver's cap (:541)
LONG_MAX_SAMPLES = WINDOW_LENGTH + (LONG_MAX_FRAMES - 1) * HOP_LENGTH + HOP_LENGTH - 1      # the longest clip with that many frames
WORKSPACE_CAP = 32 << 30             # bytes: the default `workspace_cap` of a long engine


def valid_frame_count(num_samples, in_sample_rate=SAMPLE_RATE):
    """snip_edges frame count of a clip of `num_samples` input-rate samples (Inference_FireRed_ONNX.py:84-89)."""
    resampled = int(num_samples * SAMPLE_RATE / in_sample_rate)
    return 0 if resampled < WINDOW_LENGTH else 1 + (resampled - WINDOW_LENGTH) // HOP_LENGTH


def check_long_arguments(input_audio_length, in_sample_rate, long_windows):
    """The refusals of FireRedEngine's long-window arguments, by name; needs no GPU."""
    if input_audio_length is None:
        if not long_windows:
            raise ValueError("input_audio_length=None (the dynamic axis: one window per clip) needs long_windows=True")
    elif long_windows and not WINDOW_LENGTH <= int(input_audio_length) <= LONG_MAX_SAMPLES:
        raise ValueError(f"input_audio_length={int(input_audio_length)} outside [{WINDOW_LENGTH}, {LONG_MAX_SAMPLES}] samples: a long window "
                         f"holds 1 to {LONG_MAX_FRAMES} frames (3600 s)")
    if long_windows and int(in_sample_rate) != SAMPLE_RATE:
        raise ValueError(f"long_windows=True with in_sample_rate={int(in_sample_rate)}: the long path has no in-graph resampling, "
                         f"in_sample_rate must be {SAMPLE_RATE}")


class FireRedEngine:
    def __init__(self, weights=None, input_audio_length=16000, device="cuda:0", in_sample_rate=16000, long_windows=False,
                 workspace_cap=WORKSPACE_CAP):
        """in_sample_rate: the export's IN_SAMPLE_RATE (FireRedVAD/Export_FireRedVAD.py:431-449): windows hold
        `input_audio_length` samples at that rate and the graph resamples them to 16 kHz itself.
        long_windows=True: the export at ANY `input_audio_length` from 400 samples to 3600 s (Export_FireRedVAD.py:29,48), or -- with
        input_audio_length=None -- with the dynamic axis (DYNAMIC_AXES = True: one window per clip, as Inference_FireRed_ONNX.py:541-547
        runs it).  Such an engine uses the long entry points (vadx_firered_run_long: activations in a global workspace, tiles of 64
        frames) at every length; where the default engine applies too (<= 112 frames) the probabilities are bit for bit the same.  A
        longer window is another export with fewer zero-padded window edges: other numbers, not a faster way to the same ones.
        workspace_cap: bytes of workspace (3 * P * sum(T) floats) a call may ask for; a call above it is refused by that name."""
        self.long = bool(long_windows)
        check_long_arguments(input_audio_length, in_sample_rate, self.long)       # by name, before the GPU or the weights are touched
        self.dynamic = input_audio_length is None
        self.workspace_cap = int(workspace_cap)
        self._workspace, self._rect = None, {}
        torch = _lib.require_gpu()
        self.torch = torch
        self.device = torch.device(device)
        w = _checkpoints.resolve("firered", weights)
        c = dict(w["cfg"])
        w = {k: (np.ascontiguousarray(np.asarray(v), dtype=np.float32) if k != "cfg" else v) for k, v in w.items()}
        self.L = None if self.dynamic else int(input_audio_length)
        self.in_sample_rate = int(in_sample_rate)
        if not self.long and valid_frame_count(self.L, self.in_sample_rate) > MAX_FRAMES:      # refused by name, before anything is packed or uploaded
            raise ValueError(f"a FireRed window holds at most {MAX_FRAMES} frames, {self.L} samples at {self.in_sample_rate} Hz are "
                             f"{valid_frame_count(self.L, self.in_sample_rate)}")
        # (nothing in the front-end's tables depends on a window length: the dynamic engine's one Frontend serves every clip)
        self.fe = _frontend.Frontend("firered", SAMPLE_RATE if self.dynamic else self.L, device=device, in_sample_rate=self.in_sample_rate)
        self._fes = {self.L: self.fe}
        self.T = None if self.dynamic else self.fe.frames
        self.odim = c["odim"]
        self.cache_shape = (c["R"], 1, c["P"], (c["N1"] - 1) * c["S1"])
        cfg = _lib.FireRedCfg()
        for k in ("idim", "R", "M", "H", "P", "N1", "S1", "N2", "S2", "odim"):
            setattr(cfg, k, int(c[k]))
        cfg.frames = 1 if self.long else self.T          # (a long call's frame counts come with its tables; the blob does not depend on them)
        self._cfg0 = cfg
        hw = _lib.FireRedWeightsHost()
        hw.fc1_w, hw.fc1_b, hw.fc2_w, hw.fc2_b = (w[k].ctypes.data for k in ("fc1_w", "fc1_b", "fc2_w", "fc2_b"))
        for r in range(c["R"]):
            hw.fsmn_lb[r] = w[f"fsmn{r}_lb"].ctypes.data
            if c["N2"] > 0:
                hw.fsmn_la[r] = w[f"fsmn{r}_la"].ctypes.data
            if r > 0:
                hw.blk_fc1_w[r], hw.blk_fc1_b[r] = w[f"blk{r}_fc1_w"].ctypes.data, w[f"blk{r}_fc1_b"].ctypes.data
                hw.blk_fc2_w[r] = w[f"blk{r}_fc2_w"].ctypes.data
        for m in range(c["M"]):
            hw.dnn_w[m], hw.dnn_b[m] = w[f"dnn{m}_w"].ctypes.data, w[f"dnn{m}_b"].ctypes.data
        hw.out_w, hw.out_b = w["out_w"].ctypes.data, w["out_b"].ctypes.data
        Lb = _lib.lib()
        self._hw, self._w = hw, w            # (the host arrays behind hw's pointers stay alive with the engine)

        def build(mode):
            """(cfg, device blob) of one arithmetic: the blob carries the weight fragments of that arithmetic only"""
            c = _lib.FireRedCfg.from_buffer_copy(self._cfg0)
            c.arithmetic = _lib.GEMM_MODES[mode]
            n = Lb.vadx_firered_packed_floats(C.byref(c))
            if n == 0:
                if mode != "f32":             # H / P outside the split kernel's shape: float32 MFMAs
                    return build("f32")
                raise ValueError("FireRed config not supported by the HIP kernel (idim 80, H<=256, P<=128, frames<=112, odim<=4)")
            packed = np.zeros(n, dtype=np.float32)
            _lib.check(Lb.vadx_firered_pack_host(C.byref(c), C.byref(hw), packed.ctypes.data))
            return c, torch.from_numpy(packed).to(self.device)

        def flag(c, blob):
            f, a = C.c_uint32(0), C.c_float(0.0)
            with torch.cuda.device(self.device):
                _lib.check(Lb.vadx_firered_range_flag(C.byref(c), blob.data_ptr(), 1, C.byref(f), C.byref(a), _lib.stream_ptr()))
            return int(f.value), float(a.value)
        self.blobs = _lib.ArithBlobs(build, flag)
        self.blobs.get()                     # pack now: an unsupported config raises here

    @property
    def cfg(self):
        return self.blobs.get()[0]

    @property
    def packed(self):
        return self.blobs.get()[1]

    def run(self, audio_i16, windows_per_clip=1):
        """audio int16 [B, W*L] -> probs f32 [B*W, odim, T] (each window stateless, as the reference)."""
        t = self.torch
        if self.dynamic:
            raise ValueError("a dynamic-axis engine (input_audio_length=None) has no window grid: use run_packed / detect on a list of clips")
        if not t.is_tensor(audio_i16):
            audio_i16 = t.from_numpy(np.ascontiguousarray(audio_i16, dtype=np.int16))
        return self._run_logmel(self.fe.logmel(audio_i16, windows_per_clip, self.L))

    def workspace_bytes(self, frames_total):
        """Bytes of workspace a long call over `frames_total` frames needs: 3 * P * frames_total floats (vadx_firered_long_workspace_bytes)"""
        return int(_lib.lib().vadx_firered_long_workspace_bytes(C.byref(self._cfg0), int(frames_total)))

    def _run_long(self, logmel, tables, frames_total):
        """log-mel f32 [frames_total, 80] + a vadx_firered_long_tables -> probs f32 [odim, frames_total] (vadx_firered_run_long under the
        range protocol).  The workspace is kept between calls and grows to the largest call, never above `workspace_cap`."""
        t = self.torch
        need = self.workspace_bytes(frames_total)
        if need > self.workspace_cap:
            raise ValueError(f"this call needs a workspace of {need} bytes (3 * P * {frames_total} frames * 4), above workspace_cap = "
                             f"{self.workspace_cap}: run the batch in parts, or raise workspace_cap")
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = None
            self._workspace = t.empty((need,), dtype=t.uint8, device=self.device)
        ws = self._workspace
        probs = t.empty((self.odim, frames_total), dtype=t.float32, device=self.device)

        def launch(mode, cfg, packed):
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().vadx_firered_run_long(C.byref(cfg), packed.data_ptr(), logmel.data_ptr(), C.byref(tables), probs.data_ptr(),
                                                            ws.data_ptr(), int(ws.numel()), _lib.stream_ptr()))
            return probs
        return self.blobs.guarded(launch)

    def release_workspace(self):
        """Give the long path's workspace back to the allocator (it is kept between calls and grows to the largest call)."""
        self._workspace = None

    def _rect_tables(self, nwin):
        """The long tables of a rectangular batch of nwin windows of T frames (equal counts), kept on the device per nwin"""
        got = self._rect.get(nwin)
        if got is None:
            t = self.torch
            if len(self._rect) >= 8:
                self._rect.pop(next(iter(self._rect)))
            tabs = [t.from_numpy(a).to(self.device) for a in _ragged.long_tables(np.full(nwin, self.T, dtype=np.int64))]
            got = self._rect[nwin] = (tabs, _lib.FireRedLongTables(*(a.data_ptr() for a in tabs), nwin, int(tabs[2].numel()), nwin * self.T))
        return got[1]

    def pack(self, clips):
        """The packed batch of a dynamic-axis engine: `clips` (list of 1-D int16 arrays of any lengths) end to end, no padding
        (vadx.ragged.PackedClips).  A clip above 3600 s is refused by name (the reference's 3600 s windowing of such a file stays out)."""
        return _ragged.PackedClips.from_clips(clips, self.device, LONG_MAX_FRAMES)

    def run_packed(self, pc, return_logmel=False):
        """vadx.ragged.PackedClips -> probs f32 [odim, sum T_b] on the device: clip b's T_b = pc.frames[b] frames at columns
        pc.frame_first[b] .. (one snip-edge front-end launch, then vadx_firered_run_long); clip b's columns are bit for bit those of the
        one-clip call.  A batch without a single frame gives [odim, 0] and launches nothing."""
        if not self.dynamic:
            raise ValueError(f"this engine cuts windows of {self.L} samples: run_packed is the dynamic-axis call (input_audio_length=None)")
        if int(pc.frames.max()) > LONG_MAX_FRAMES:
            raise ValueError(f"clip {int(np.argmax(pc.frames))} has {int(pc.frames.max())} frames: a window holds at most {LONG_MAX_FRAMES} (3600 s)")
        if pc.device is None:
            pc.to(self.device)
        logmel = self.fe.logmel_ragged_snip(pc)
        if pc.n_frames == 0:
            probs = self.torch.empty((self.odim, 0), dtype=self.torch.float32, device=self.device)
        else:
            probs = self._run_long(logmel, pc.tables(), pc.n_frames)
        return (probs, logmel) if return_logmel else probs

    def _run_logmel(self, logmel):
        """log-mel f32 [windows, T, 80] -> probs f32 [windows, odim, T] (vadx_firered_run under the range protocol; a long engine:
        vadx_firered_run_long over the same windows as a rectangular batch, its planes [odim, windows * T] turned window-major)"""
        t = self.torch
        nwin = logmel.shape[0]
        if self.long:
            planes = self._run_long(logmel, self._rect_tables(nwin), nwin * self.T)
            return planes.view(self.odim, nwin, self.T).permute(1, 0, 2).contiguous()
        probs = t.empty((nwin, self.odim, self.T), dtype=t.float32, device=self.device)

        def launch(mode, cfg, packed):
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().vadx_firered_run(C.byref(cfg), packed.data_ptr(), logmel.data_ptr(), nwin,
                                                       probs.data_ptr(), _lib.stream_ptr()))
            return probs
        return self.blobs.guarded(launch)

    def ragged(self, clips, pad_noise=None, device=True):
        """The packed batch of `clips` (list of 1-D int16 arrays of any lengths) on this engine's non-overlapping window grid
        (vadx.ragged.RaggedBatch), each padded with pad_noise row b.  device=None keeps it on the host."""
        return _ragged.RaggedBatch.from_clips(clips, self.L, self.L, pad_noise, None, self.device if device is True else device)

    def ragged_packed(self, pcm, clip_offsets, lengths, pad_noise=None, normalize=None):
        """`ragged` for clips that already lie in device memory (RaggedBatch.from_packed: padded and packed on the device, bit for bit what
        `ragged` builds from the same clips and noise; normalize="rms" applies timestamps.normalise_audio on the way)."""
        if self.dynamic:             # no grid, no padding: tables only around the clips where they lie
            if normalize is not None:
                raise ValueError(f"normalize={normalize!r}: a dynamic-axis batch takes the clips as they lie (tables only); normalise them first")
            return _ragged.PackedClips.from_packed(pcm, clip_offsets, lengths, self.device, LONG_MAX_FRAMES)
        return _ragged.RaggedBatch.from_packed(pcm, clip_offsets, lengths, self.L, self.L, pad_noise, normalize, device=self.device)

    def run_ragged(self, rb):
        """RaggedBatch on this engine's grid -> probs f32 [sum W, odim, T]: rows win_first[b] .. win_first[b+1]-1 are clip b's windows
        (vadx_windows_gather, then the unchanged front-end and vadx_firered_run over sum W windows).  A host-only batch
        (device=None) is uploaded first, in place: `rb.to(self.device)` turns its pcm and tables into device tensors."""
        if self.dynamic:
            raise ValueError("a dynamic-axis engine (input_audio_length=None) has no window grid: use run_packed on a PackedClips")
        if rb.window != self.L or rb.stride != self.L:
            raise ValueError(f"the batch was packed for windows of {rb.window} every {rb.stride} samples, this engine cuts {self.L} every {self.L}")
        if rb.device is None:
            rb.to(self.device)
        return self._run_logmel(self.fe.logmel(rb.gather(), 1, self.L))

    def _track_source(self, clips, pad_noise, sample_rate):
        """Run the net over whole clips -> (channel, n_frames int64 [B] (host), durations in seconds [B]): `channel(k)` is output k as
        tracks f32 [B, frames] on the device, row b valid up to n_frames[b] = min(clip b's snip-edge frames, its windows' frames).
        A list (or tuple) of 1-D clips takes the ragged route (`run_ragged`, one vadx_tracks_gather per channel: [B, max(n_frames, 1)],
        zeros past n_frames[b]); an array [B, N] the rectangular one (`run`: [B, n_frames], cut from the windows laid end to end).
        sample_rate: what a sample count means in frames and in seconds -- `detect` passes in_sample_rate, the AED driver 16 kHz."""
        if self.dynamic:
            # one window per clip (Inference_FireRed_ONNX.py:541-547): no padding, so pad_noise has nothing to fill; an array [B, N] is B
            # clips of one length.  A clip under 400 samples has no frame and no segment.
            is_list = isinstance(clips, (list, tuple, _ragged.PackedClips))
            pc = clips if isinstance(clips, _ragged.PackedClips) else self.pack(list(clips) if is_list else [r for r in np.asarray(clips)])
            probs = self.run_packed(pc)
            nf = pc.frames.astype(np.int64)

            def channel(k):
                track = gather_tracks(self.device, probs[k], 1, 0, 1, pc.frame_first, nf)
                return track if is_list else track[:, :int(nf[0])].contiguous()
            return channel, nf, [int(n) / sample_rate for n in pc.lengths]
        if isinstance(clips, (list, tuple, _ragged.RaggedBatch)):
            # (a RaggedBatch is packed already: `ragged`, or RaggedBatch.from_packed on the device)
            rb = clips if isinstance(clips, _ragged.RaggedBatch) else self.ragged(clips, pad_noise)
            probs = self.run_ragged(rb)
            nf = np.minimum([valid_frame_count(int(n), sample_rate) for n in rb.lengths], rb.windows.astype(np.int64) * self.T)
            return (lambda k: gather_tracks(self.device, probs, self.odim * self.T, k * self.T, self.T, rb.win_first, nf),
                    nf, [int(n) / sample_rate for n in rb.lengths])
        B, n = np.asarray(clips).shape
        padded, W = pad_batch(clips, self.L, self.L, pad_noise)
        probs = self.run(padded, W).view(B, W, self.odim, self.T)
        nvalid = min(valid_frame_count(n, sample_rate), W * self.T)     # 10 s clips give 980 of the 998 snip-edge frames
        return (lambda k: probs[:, :, k, :].reshape(B, W * self.T)[:, :nvalid].contiguous(),
                np.full(B, nvalid, dtype=np.int64), [n / sample_rate] * B)

    def run_from_host(self, host_i16, windows_per_clip=1, chunk_clips=256, feed=None):
        """`run` fed from HOST memory (int16 [B, W*L], ideally pinned: vadx.feed.pin), uploads overlapped with compute
        (vadx.feed.HostPcmFeed); bit-identical to `run` of the resident batch."""
        from . import feed as _feed
        f = feed or _feed.HostPcmFeed(self.device, host_i16.shape[1], chunk_clips)
        return _feed.cat_results(f.map([host_i16], lambda a: self.run(a, windows_per_clip)))

    def _frontend_for(self, length):
        fe = self._fes.get(length)
        if fe is None:
            if len(self._fes) >= 8:                      # chunk length + a few tail lengths; keep it bounded
                self._fes.pop(next(k for k in self._fes if k != self.L))
            fe = self._fes[length] = _frontend.Frontend("firered", length, device=self.device, in_sample_rate=self.in_sample_rate)
        return fe

    def new_caches(self, streams=1):
        """zeros [R, streams, P, (N1-1)*S1] (Inference_FireRed_ONNX.py:775)"""
        R, _, P, pad = self.cache_shape
        return self.torch.zeros((R, streams, P, pad), dtype=self.torch.float32, device=self.device)

    def stream_run(self, audio_i16, caches_in):
        """One chunk of `streams` independent streams: audio int16 [streams, n] (400 <= n, any length),
        caches_in f32 [R, streams, P, pad] -> (probs f32 [streams, odim, T], caches_out); T = (n-400)//160+1.
        Look-back only (N2 == 0), as the Stream-VAD checkpoint (Export_FireRedVAD.py:479-612)."""
        t = self.torch
        if not t.is_tensor(audio_i16):
            audio_i16 = t.from_numpy(np.ascontiguousarray(audio_i16, dtype=np.int16))
        audio_i16 = audio_i16.to(self.device)
        S, n = audio_i16.shape
        if n < WINDOW_LENGTH:
            raise ValueError(f"a stream chunk needs at least {WINDOW_LENGTH} samples, got {n}")
        if valid_frame_count(n, self.in_sample_rate) > MAX_FRAMES:           # before the front-end runs: the net would refuse its log-mel
            raise ValueError(f"a stream chunk holds at most {MAX_FRAMES} frames, {n} samples are {valid_frame_count(n, self.in_sample_rate)}")
        R, _, P, pad = self.cache_shape
        if tuple(caches_in.shape) != (R, S, P, pad) or caches_in.dtype != t.float32:
            raise ValueError(f"caches_in must be float32 {[R, S, P, pad]}, got {list(caches_in.shape)}")
        fe = self._frontend_for(n)
        logmel = fe.logmel(audio_i16, 1, n)
        cfg = _lib.FireRedCfg.from_buffer_copy(self.cfg)
        cfg.frames = fe.frames
        caches_in = caches_in.to(self.device).contiguous()
        caches_out = t.empty_like(caches_in)
        probs = t.empty((S, self.odim, fe.frames), dtype=t.float32, device=self.device)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_firered_stream_run(C.byref(cfg), self.packed.data_ptr(), logmel.data_ptr(), S,
                                                          caches_in.data_ptr(), caches_out.data_ptr(), probs.data_ptr(),
                                                          _lib.stream_ptr()))
        return probs, caches_out

    def stream_detect(self, clips_i16, chunk=STREAM_CHUNK_SAMPLES, post=(5, 0.4, 5, 8, 2000, 20), return_probs=False, chunks_per_tick=1):
        """Equal-length clips int16 [B,N] (host): every clip is one stream, all streams advance one chunk per
        launch (Inference_FireRed_ONNX.py:788-822) -> per clip [(start_s, end_s)].
        A LIST (or tuple) of 1-D clips of any lengths runs as the streams of one `FireRedStreamBatch` on the chunk grid until the longest
        is done (`_stream_detect_list`); return_probs then gives a per-clip LIST of tracks.  chunks_per_tick = k > 1 (lists only) advances
        every stream by up to k whole chunks per tick (`FireRedStreamBatch.step_ragged`: stream b takes min(k, whole chunks left)); the
        segments and the tracks are those of k = 1."""
        k = int(chunks_per_tick)
        if k < 1:
            raise ValueError(f"chunks_per_tick={chunks_per_tick} must be at least 1")
        if isinstance(clips_i16, (list, tuple)):
            return self._stream_detect_list(clips_i16, chunk, post, return_probs, k)
        if k != 1:
            raise ValueError("chunks_per_tick above 1 takes a list of clips (equal-length arrays advance one chunk per launch)")
        t = self.torch
        clips = np.asarray(clips_i16)
        B, n = clips.shape
        dev = t.from_numpy(np.ascontiguousarray(clips, dtype=np.int16)).to(self.device)
        caches = self.new_caches(B)
        parts, pos = [], 0
        while pos < n:
            end = min(pos + chunk, n)
            x = dev[:, pos:end]
            if end - pos < WINDOW_LENGTH:
                x = t.nn.functional.pad(x, (0, WINDOW_LENGTH - (end - pos)))
            pr, caches = self.stream_run(x.contiguous(), caches)
            parts.append(pr[:, 0, :])
            pos = end
        nvalid = valid_frame_count(n)
        if not parts or nvalid == 0:
            out, track = [[] for _ in range(B)], np.zeros((B, 0), np.float32)
            return (out, track) if return_probs else out
        track_dev = t.cat(parts, dim=1)[:, :nvalid].contiguous()
        # the decisions of all streams in one launch (vadx_stream_vadpost: one thread per stream), not a host loop over streams
        out = _vadpost.StreamVadPostprocessorBatch(*post, streams=B, device=self.device).process_batch(track_dev)
        track = track_dev.cpu().numpy()
        return (out, track) if return_probs else out

    def _stream_detect_list(self, clips, chunk, post, return_probs, chunks_per_tick=1):
        """`stream_detect` over clips of any lengths: clip b is stream b of one FireRedStreamBatch.  At every position of the chunk grid the
        streams that still have a whole chunk tick together; a stream's short last chunk runs in a tick of its own length (zero-padded to
        400 samples if shorter), streams elsewhere inactive.  A padded last chunk adds one frame; where that frame lies beyond
        valid_frame_count(len) -- a clip of whole chunks plus fewer than 80 samples, or one under 400 samples -- the reference cuts it off
        the track again, so the tick is skipped.  Per clip: the events of all ticks, then the segment still open at its end.
        chunks_per_tick = k > 1: the grid steps by k chunks and the whole chunks of a step run as ONE ragged tick, stream b taking
        min(k, whole chunks left); the short last chunks run as above, each where its stream's whole chunks end."""
        t = self.torch
        clips = [np.ascontiguousarray(np.asarray(c).reshape(-1), dtype=np.int16) for c in clips]
        S, chunk = len(clips), int(chunk)
        if S == 0:
            return ([], []) if return_probs else []
        if chunk < WINDOW_LENGTH:
            raise ValueError(f"a stream chunk needs at least {WINDOW_LENGTH} samples, got {chunk}")
        lens = np.array([len(c) for c in clips], dtype=np.int64)
        grid = -(-int(lens.max()) // chunk) if lens.max() else 0
        host = np.zeros((S, grid * chunk + WINDOW_LENGTH), dtype=np.int16)        # zeros behind every clip: the padding of a short last chunk
        for b, c in enumerate(clips):
            host[b, :len(c)] = c
        dev = t.from_numpy(host).to(self.device)
        it = FireRedStreamBatch(self, S, post)
        out, tracks = [[] for _ in range(S)], [[] for _ in range(S)]
        done = np.zeros(S, dtype=np.int64)                                        # frames each stream has run
        valid = np.array([valid_frame_count(int(n), self.in_sample_rate) for n in lens], dtype=np.int64)
        if chunks_per_tick > 1:
            self._ragged_ticks(it, dev, lens, valid, done, chunk, chunks_per_tick, out, tracks, return_probs)
        for g in range(grid if chunks_per_tick == 1 else 0):
            pos = g * chunk
            left = lens - pos
            ticks = [(chunk, left >= chunk)] + [(int(n), left == n) for n in sorted(set(left[(left > 0) & (left < chunk)].tolist()))]
            for n, act in ticks:
                width = max(n, WINDOW_LENGTH)
                frames = valid_frame_count(width, self.in_sample_rate)
                if n < WINDOW_LENGTH:
                    act = act & (done + frames <= valid)
                if not act.any():
                    continue
                probs, events = it.step(dev[:, pos:pos + width].contiguous(), active=None if act.all() else act)
                done[act] += frames
                track = probs[:, 0, :].cpu().numpy() if return_probs else None
                for b in np.flatnonzero(act):
                    out[b] += events[b]
                    if return_probs:
                        tracks[b].append(track[b])
        for b, seg in enumerate(it.open_segments()):
            if seg is not None:
                out[b].append(seg)
        if not return_probs:
            return out
        return out, [np.concatenate(tr) if tr else np.zeros(0, np.float32) for tr in tracks]

    def _ragged_ticks(self, it, dev, lens, valid, done, chunk, k, out, tracks, return_probs):
        """The tick loop of `_stream_detect_list` at k > 1 chunks per tick (same arguments, filled in place)."""
        S = len(lens)
        frames = valid_frame_count(chunk, self.in_sample_rate)
        if frames > MAX_FRAMES:
            raise ValueError(f"a stream chunk holds at most {MAX_FRAMES} frames, {chunk} samples are {frames}")
        k = min(k, MAX_FRAMES // frames)                                          # what a workgroup's columns hold
        for pos in range(0, int(lens.max()), k * chunk):
            whole = np.clip((lens - pos) // chunk, 0, k)
            if whole.any():
                probs, events, first = it.step_ragged(dev[:, pos:pos + k * chunk], whole, chunk=chunk)
                done += whole * frames
                track = probs[0].cpu().numpy() if return_probs else None
                for b in np.flatnonzero(whole):
                    out[b] += events[b]
                    if return_probs:
                        tracks[b].append(track[first[b] * frames:first[b + 1] * frames])
            start = pos + whole * chunk                                           # where each stream's whole chunks of this step end
            left = lens - start
            tail = (whole < k) & (left > 0) & (left < chunk)
            for p, n in sorted(set(zip(start[tail].tolist(), left[tail].tolist()))):
                act = tail & (start == p) & (left == n)
                width = max(n, WINDOW_LENGTH)
                fr = valid_frame_count(width, self.in_sample_rate)
                if n < WINDOW_LENGTH:
                    act = act & (done + fr <= valid)
                if not act.any():
                    continue
                probs, events = it.step(dev[:, p:p + width].contiguous(), active=None if act.all() else act)
                done[act] += fr
                track = probs[:, 0, :].cpu().numpy() if return_probs else None
                for b in np.flatnonzero(act):
                    out[b] += events[b]
                    if return_probs:
                        tracks[b].append(track[b])

    def detect(self, clips_i16, pad_noise=None, post=(5, 0.4, 20, 2000, 20, 5, 0), return_probs=False):
        """Equal-length clips int16 [B,N] (host) -> per clip [(start_s, end_s)] for output channel 0
        (VAD driver :535-591).  pad_noise: standard-normal [B, >= pad] for the tail padding.
        A LIST (or tuple) of 1-D clips of any lengths runs as one ragged batch (`run_ragged`, one vadx_vadpost launch); clip b's
        result is that of `detect(clip_b[None, :], pad_noise=row_b[None, :])[0]`, its seconds computed with its own duration;
        return_probs then gives per-clip LISTS of tracks and decisions, each cut to its clip's frame count."""
        channel, nf, durations = self._track_source(clips_i16, pad_noise, self.in_sample_rate)
        track = channel(0)
        out, dec = track_segments(_vadpost.VadPostprocessor(*post, device=self.device), track, nf, durations)
        if not return_probs:
            return out
        if isinstance(clips_i16, (list, tuple, _ragged.RaggedBatch, _ragged.PackedClips)):
            return out, [track[b, :nf[b]] for b in range(len(nf))], [dec[b, :nf[b]] for b in range(len(nf))]
        return (out, track, dec) if track.shape[1] else (out, track)      # an array without a valid frame: no decisions are returned

    def detect_table(self, clips_i16, pad_noise=None, post=(5, 0.4, 20, 2000, 20, 5, 0), sample_rule="nearest"):
        """`detect` with the tracks and the frame table staying on the device (`clips.track_table`: one vadx_vadpost launch, one
        vadx_timestamps_frames launch) -> a vadx.tstable.TimestampTable whose `lists()` is what `detect` returns and whose
        `chunks_table()` goes straight to vadx.chunks.collect_chunks_batch (sample rows at in_sample_rate, by `sample_rule`)."""
        channel, nf, durations = self._track_source(clips_i16, pad_noise, self.in_sample_rate)
        return track_table(_vadpost.VadPostprocessor(*post, device=self.device), channel(0), nf, durations, self.in_sample_rate, sample_rule)[0]


IDX2EVENT = {0: "speech", 1: "singing", 2: "music"}      # Inference_FireRed_ONNX.py:632


def _detect_events(self, clips_i16, pad_noise=None, thresholds=(0.4, 0.5, 0.5), post=(5, 20, 2000, 20, 5, 0),
                   return_probs=False):
    """FireRedAED driver (Inference_FireRed_ONNX.py:620-742): equal-length clips int16 [B,N] through an
    odim == 3 model -> per clip (event2timestamps, event2ratio).  `post` = (smooth, min_event, max_event,
    min_silence, merge_silence, extend); `thresholds` per event in IDX2EVENT order.
    A LIST (or tuple) of 1-D clips of any lengths runs as one ragged batch, per event one vadx_tracks_gather + one vadx_vadpost launch;
    clip b's result is that of the [1, N] call on it alone.  return_probs adds the tracks: f32 [B, odim, n_frames] for an array, per
    clip f32 [odim, n_frames[b]] for a list.  Frames and seconds are counted at 16 kHz here, whatever in_sample_rate is."""
    if self.odim != len(IDX2EVENT):
        raise ValueError(f"the AED driver needs a {len(IDX2EVENT)}-output model, this one has odim = {self.odim}")
    t = self.torch
    channel, nf, durations = self._track_source(clips_i16, pad_noise, SAMPLE_RATE)
    B = len(nf)
    out = [({}, {}) for _ in range(B)]
    tracks, live = [], None
    for idx, event in IDX2EVENT.items():
        thr = thresholds[idx]
        track = channel(idx)
        tracks.append(track)
        segments, _ = track_segments(_vadpost.VadPostprocessor(post[0], thr, *post[1:], device=self.device), track, nf, durations)
        # frames over threshold per clip: a ragged batch's rows are zero-filled past n_frames[b], so the columns are masked, not the
        # values (one launch sequence, one read-back).  The ratio is the exact count times the float32 reciprocal of the frame count
        # (not count / N: an ulp apart for some pairs), which is bitwise torch's device mean of the 0 / 1 values
        # (tests/test_gpu_ragged.py checks the product against torch.mean for every count)
        if live is None:
            live = t.arange(track.shape[1], device=self.device)[None, :] < t.from_numpy(nf).to(self.device)[:, None]
        counts_over = ((track >= np.float32(thr)) & live).sum(dim=1).cpu().numpy()
        ratio = counts_over.astype(np.float32) * (np.float32(1.0) / np.maximum(nf, 1).astype(np.float32))
        for b in range(B):
            out[b][0][event] = segments[b]
            out[b][1][event] = round(float(ratio[b]), 3) if nf[b] else 0.0
    if not return_probs:
        return out
    if isinstance(clips_i16, (list, tuple, _ragged.PackedClips)):
        return out, [t.stack([tr[b, :nf[b]] for tr in tracks]) for b in range(B)]
    return out, t.stack(tracks, dim=1)


FireRedEngine.detect_events = _detect_events

HDR_WORDS, H_COUNT, H_LAST_START, H_DONE = 32, 19, 24, 28      # the record's per-stream header (csrc/firered.hip: TK_HDR, TK_DONE), in 32-bit words


class FireRedStreamBatch(StreamBatch):
    """`streams` live FireRed Stream-VAD streams on the device (vadx_firered_stream_tick): every `step` advances each stream by `chunks`
    chunks of audio.  What the reference's chunk loop carries (FireRedVAD/Inference_FireRed_ONNX.py:775-822) -- the FIR caches it feeds
    back and the StreamVadPostprocessor object -- stays in the device `record` (DESIGN.md "Stream batches"; its first S*R*P*pad floats are
    the FIR caches [S, R, P, pad], the headers follow); per tick the front-end and ONE net launch run, and only the events come back.
    `post` = the reference class's constructor arguments (smooth window, threshold, pad_start, min_speech, max_speech, min_silence, in
    frames); cap = segments a stream may end in one tick (None: one per frame, the most there can be).  On "h2" every tick reads the
    range flag and, when it is raised, recomputes the tick on "split" from the same record into the same record."""

    def __init__(self, engine, streams, post=(5, 0.4, 5, 8, 2000, 20), cap=None):
        if not isinstance(engine, FireRedEngine):
            raise TypeError("FireRedStreamBatch needs a vadx.firered.FireRedEngine")
        nb = _lib.lib().vadx_firered_stream_state_bytes(C.byref(engine.cfg), int(streams))
        super().__init__(engine, streams, nb)
        self.cap = cap
        if engine.cfg.N2 != 0:
            raise ValueError(f"the streaming model has no look-ahead filter, these weights have N2 = {engine.cfg.N2}")
        if max(1, int(post[0])) > 16:
            raise ValueError(f"smooth_window_size {post[0]} > 16: the device record's ring buffer holds 16 frames")
        self._prm = _lib.StreamVadPostParams(int(post[0]), float(np.float32(post[1])), *(int(v) for v in post[2:6]))
        self.frames_per_second = 100
        R, _, P, pad = engine.cache_shape
        self._cache_floats = self.streams * R * P * pad
        self._hdr_at = (self._cache_floats + 3) // 4 * 16             # the headers start on the next multiple of 16 bytes
        if nb != self._hdr_at + self.streams * HDR_WORDS * 4:
            raise _lib.VadxError(f"vadx_firered_stream_state_bytes = {nb}: not the record this binding was written for")
        self.open_start = None                                   # int32 [S] (device) of the last tick: 0-based start frame of the open segment, -1 = none

    @property
    def caches(self):
        R, _, P, pad = self.engine.cache_shape
        return self.record[:self._cache_floats * 4].view(self.engine.torch.float32).view(self.streams, R, P, pad)

    def headers(self, record=None):
        """int32 view [S, 32] of the per-stream headers of `record` (default: the current one): the decision machine and frames done."""
        record = self.record if record is None else record
        return record[self._hdr_at:].view(self.engine.torch.int32).view(self.streams, HDR_WORDS)

    def stream_bytes(self, record, s):
        """Every byte of `record` that belongs to stream s (caches, header), as one uint8 tensor."""
        n = self._cache_floats // self.streams * 4
        return self.engine.torch.cat([record[s * n:(s + 1) * n], record[self._hdr_at + s * HDR_WORDS * 4:self._hdr_at + (s + 1) * HDR_WORDS * 4]])

    @property
    def frames_done(self):
        """int64 [S] (host): frames each stream has done since its reset, read from the device record.  Frame i of a stream's next
        tick is frame frames_done + i of its audio, 10 ms per frame."""
        return self.headers()[:, H_DONE:H_DONE + 2].contiguous().view(self.engine.torch.int64)[:, 0].cpu().numpy()

    def open_segments(self):
        """Per stream the (start_s, end_s) of the segment still open after its last frame, or None: what the reference's process_batch
        appends at the end of its input (Export_FireRedVAD.py:1336-1338).  Read from the record; nothing is closed."""
        h = self.headers().cpu().numpy()
        inv_fps = 1.0 / self.frames_per_second
        start, count = h[:, H_LAST_START].astype(np.int64) - 1, h[:, H_COUNT].astype(np.int64)
        return [(max(0, int(a) - 1) * inv_fps, (int(n) - 1) * inv_fps) if a > 0 else None for a, n in zip(start, count)]

    def step(self, samples_i16, chunks=1, reset=None, active=None, group=0):
        """samples_i16 int16 [S, chunks * n] (host or device, numpy or torch): each row holds that stream's next `chunks` chunks of n
        samples (400 <= n; the call's width sets n) -> (probs f32 [S, odim, chunks * frames] on the device, events): per stream the
        [(start_s, end_s)] of the segments that ended in this tick, at 100 frames per second.  Every chunk's features are computed on
        its own, as the reference computes them; the net carries its caches across the chunks.  reset / active: bool [S] or None; an
        inactive stream keeps its record bit for bit, ignores a reset, has NaN probabilities and no events.  group: streams per
        workgroup (0 = the library's choice); no result depends on it."""
        eng, t = self.engine, self.engine.torch
        k, S = int(chunks), self.streams
        if k < 1:
            raise ValueError(f"chunks={chunks} must be at least 1")
        x = self._samples(samples_i16, f"[{S}, chunks * n]", lambda x: x.shape[1] % k, where=f" at chunks={k}")
        n = x.shape[1] // k
        if n < WINDOW_LENGTH:
            raise ValueError(f"a stream chunk needs at least {WINDOW_LENGTH} samples, got {n}")
        T = valid_frame_count(n, eng.in_sample_rate)
        F = k * T
        if F > MAX_FRAMES:
            raise ValueError(f"a stream tick holds at most {MAX_FRAMES} frames, {k} chunks of {n} samples are {F}")
        gmax = MAX_FRAMES // F                                    # vadx_firered_stream_group_max
        if not 0 <= int(group) <= gmax:
            raise ValueError(f"group={group} outside [0, {gmax}] at {F} frames per tick")
        act, _, reset_d, act_d, src, dst = self._begin(reset, active)
        fe = eng._frontend_for(n)
        logmel = fe.logmel(x.to(eng.device), k, n)
        cap = int(self.cap) if self.cap else F                    # F: a forced split per frame is the most a tick can end
        probs = t.empty((S, eng.odim, F), dtype=t.float32, device=eng.device)
        segs = t.empty((S, cap, 2), dtype=t.int32, device=eng.device)
        counts = t.empty((S,), dtype=t.int32, device=eng.device)
        opened = t.empty((S,), dtype=t.int32, device=eng.device)
        Lb = _lib.lib()

        def launch(mode, cfg, packed):
            c = _lib.FireRedCfg.from_buffer_copy(cfg)
            c.frames = T
            with t.cuda.device(eng.device):
                _lib.check(Lb.vadx_firered_stream_tick(C.byref(c), packed.data_ptr(), logmel.data_ptr(), S, k, int(group), C.byref(self._prm),
                                                       None if reset_d is None else reset_d.data_ptr(),
                                                       None if act_d is None else act_d.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                                       probs.data_ptr(), segs.data_ptr(), counts.data_ptr(), cap, opened.data_ptr(),
                                                       _lib.stream_ptr()))
        eng.blobs.guarded(launch)
        self._end(act)
        self.open_start = opened
        cn = counts.cpu().numpy()
        used = int(cn.max())
        if used > cap:
            raise _lib.VadxError(f"FireRedStreamBatch: {used} segments ended in one tick, cap={cap} (the record has advanced)")
        sg = segs[:, :used].cpu().numpy() if used else np.zeros((S, 0, 2), np.int32)      # only the used prefix of the table travels
        inv_fps = 1.0 / self.frames_per_second
        events = [[] for _ in range(S)]
        for s in np.flatnonzero(cn).tolist():                     # most streams end nothing in most ticks
            events[s] = [(int(a) * inv_fps, int(b) * inv_fps) for a, b in sg[s, :cn[s]].tolist()]
        return probs, events

    def _ragged_rows(self, samples, counts, n, capacity):
        """The samples and counts of a ragged tick -> (rows int16 [n_rows, n] or None, x int16 [S, >= max(counts) * n] tensor
        or None, counts int32 [S]).  A list of S 1-D arrays gives its own counts, and its concatenation IS the row matrix (made on the
        device when a listed row lies there)."""
        S, t = self.streams, self.engine.torch
        if isinstance(samples, (list, tuple)):
            if len(samples) != S:
                raise ValueError(f"samples lists {len(samples)} arrays for {S} streams")
            resident = any(t.is_tensor(r) and r.device.type != "cpu" for r in samples)      # then the rows are concatenated where they are
            rows = [(r if t.is_tensor(r) else t.from_numpy(np.ascontiguousarray(r))).reshape(-1) if resident else
                    np.asarray(r.cpu() if hasattr(r, "cpu") else r).reshape(-1) for r in samples]
            for s, r in enumerate(rows):
                if r.dtype != (t.int16 if resident else np.int16):
                    raise ValueError(f"samples[{s}] must be int16, got {r.dtype}")
                if r.shape[0] % n:
                    raise ValueError(f"samples[{s}] holds {r.shape[0]} samples: a stream takes whole chunks of {n}")
            got = np.array([r.shape[0] // n for r in rows], dtype=np.int64)
            if counts is not None and not np.array_equal(np.asarray(counts).reshape(-1), got):
                raise ValueError("counts disagree with the lengths of the listed samples")
            counts = _ragged.chunk_counts(got, S, capacity)
            if resident:
                return t.cat([r.to(self.engine.device) for r in rows]).view(-1, n), None, counts
            return np.concatenate(rows).reshape(-1, n), None, counts
        if counts is None:
            raise ValueError("step_ragged needs counts with a [S, n] array")
        counts = _ragged.chunk_counts(counts, S, capacity)
        need = int(counts.max(initial=0)) * n
        x = self._samples(samples, f"[{S}, >= max(counts) * chunk = {need}]", lambda x: x.shape[1] < need)
        return None, x, counts

    def step_ragged(self, samples_i16, counts=None, chunk=None, reset=None, group=0):
        """A tick in which stream s advances by counts[s] chunks of `chunk` samples (default: the engine's input length; at least 400,
        frames = valid_frame_count(chunk) <= 112), 0 <= counts[s] <= 112 // frames: the work is sum(counts) chunks behind the front-end
        and ONE net launch (vadx_firered_stream_tick_ragged).  samples_i16: int16 [S, >= max(counts) * chunk] (host or device, numpy or
        torch), row s holding that stream's counts[s] * chunk new samples from column 0 -- or a list of S 1-D arrays whose lengths are
        multiples of `chunk` (the counts then come from the lengths, and the concatenation is staged as it is).
        -> (probs f32 [odim, n_rows * frames] on the device: stream s owns the columns first[s] * frames .. first[s + 1] * frames - 1;
        events: as `step`; first: host int64 [S + 1], the prefix sum of the counts).  self.open_start is as after `step`.  A stream with
        count 0 costs nothing: it keeps its record and its pending reset, a reset request for it is ignored, it has no probabilities
        and no events.  A tick whose counts are all 0 launches nothing and leaves the record and the pending resets alone.  Counts
        outside [0, 112 // frames], a wrong shape or a non-integer dtype raise ValueError before anything is launched.  group: the most
        streams per workgroup (0 = the library's choice); no result depends on it.  `step` and `step_ragged` interchange tick by tick
        (one record); `step` stays the path for uniform ticks."""
        eng, t = self.engine, self.engine.torch
        S = self.streams
        n = int(eng.L if chunk is None else chunk)
        if n < WINDOW_LENGTH:
            raise ValueError(f"a stream chunk needs at least {WINDOW_LENGTH} samples, got {n}")
        T = valid_frame_count(n, eng.in_sample_rate)
        if T > MAX_FRAMES:
            raise ValueError(f"a stream chunk holds at most {MAX_FRAMES} frames, {n} samples are {T}")
        capacity = MAX_FRAMES // T                                # vadx_firered_stream_group_max(T)
        rows, x, counts = self._ragged_rows(samples_i16, counts, n, capacity)
        first, order, wg_first = _ragged.column_stream_plan(counts, capacity, group)
        n_rows, inv_fps = int(first[-1]), 1.0 / self.frames_per_second
        if n_rows == 0:              # nobody delivered audio: no launch; the record and the pending resets stay
            self.open_start = t.full((S,), -1, dtype=t.int32, device=eng.device)
            return t.empty((eng.odim, 0), dtype=t.float32, device=eng.device), [[] for _ in range(S)], first
        act = counts > 0
        _, _, reset_d, _, src, dst = self._begin(reset, act, upload_active=False)
        active, n_wg = int(np.count_nonzero(act)), int(wg_first.shape[0]) - 1
        # (the status word is not read back: chunk_counts and column_stream_plan cannot produce a table the kernel skips, and a skipped
        # stream would show in `frames_done`; a caller of the C entry point with tables of its own reads it)
        # the tick's tables in ONE copy: [win_src int64 [n_rows] |] counts | row_first | slot_stream | wg_first | status (a zero the copy writes)
        tabs = [counts, first[:S].astype(np.int32), order[:active], wg_first, np.zeros(1, np.int32)]
        gather = rows is None
        if gather:
            x = x.to(eng.device)
            if x.stride(1) != 1:
                x = x.contiguous()
            stride = int(x.stride(0)) if S > 1 else int(x.shape[1])
            win_stream = np.repeat(np.arange(S, dtype=np.int64), counts)
            win_src = win_stream * stride + (np.arange(n_rows, dtype=np.int64) - first[win_stream]) * n
            tabs.insert(0, win_src.view(np.int32))
        tab = t.from_numpy(np.concatenate(tabs).astype(np.int32, copy=False)).to(eng.device)
        p_counts = tab.data_ptr() + (8 * n_rows if gather else 0)
        p_first, p_slot, p_wg = p_counts + 4 * S, p_counts + 8 * S, p_counts + 4 * (2 * S + active)
        p_status = p_wg + 4 * (n_wg + 1)
        Lb = _lib.lib()
        if gather:
            wbuf = t.empty((n_rows, n), dtype=t.int16, device=eng.device)
            pcm_len = (S - 1) * stride + int(x.shape[1])
            runs = n % 8 == 0 and stride % 8 == 0 and x.data_ptr() % 16 == 0       # 16-byte runs: the aligned gather
            with t.cuda.device(eng.device):
                _lib.check((Lb.vadx_windows_gather if runs else Lb.vadx_windows_gather_any)(
                    x.data_ptr(), pcm_len, tab.data_ptr(), n_rows, n, wbuf.data_ptr(), _lib.stream_ptr()))
        else:
            wbuf = rows if t.is_tensor(rows) else t.from_numpy(rows).to(eng.device)
        fe = eng._frontend_for(n)
        logmel = fe.logmel(wbuf, 1, n)
        cap = int(self.cap) if self.cap else int(counts.max()) * T      # a forced split per frame is the most a tick can end
        probs = t.empty((eng.odim, n_rows * T), dtype=t.float32, device=eng.device)
        segs = t.empty((S, cap, 2), dtype=t.int32, device=eng.device)
        cnt = t.empty((S,), dtype=t.int32, device=eng.device)
        opened = t.empty((S,), dtype=t.int32, device=eng.device)

        def launch(mode, cfg, packed):
            c = _lib.FireRedCfg.from_buffer_copy(cfg)
            c.frames = T
            with t.cuda.device(eng.device):
                _lib.check(Lb.vadx_firered_stream_tick_ragged(C.byref(c), packed.data_ptr(), logmel.data_ptr(), S, n_rows, p_counts, p_first,
                                                              p_slot, p_wg, n_wg, C.byref(self._prm),
                                                              None if reset_d is None else reset_d.data_ptr(), src.data_ptr(),
                                                              dst.data_ptr(), probs.data_ptr(), segs.data_ptr(), cnt.data_ptr(), cap,
                                                              opened.data_ptr(), p_status, _lib.stream_ptr()))
        eng.blobs.guarded(launch)
        self._end(act)
        self.open_start = opened
        cn = cnt.cpu().numpy()
        used = int(cn.max())
        if used > cap:
            raise _lib.VadxError(f"FireRedStreamBatch: {used} segments ended in one tick, cap={cap} (the record has advanced)")
        sg = segs[:, :used].cpu().numpy() if used else np.zeros((S, 0, 2), np.int32)
        events = [[] for _ in range(S)]
        for s in np.flatnonzero(cn).tolist():
            events[s] = [(int(a) * inv_fps, int(b) * inv_fps) for a, b in sg[s, :cn[s]].tolist()]
        return probs, events, first


class FireRedSession(Session):
    """onnxruntime.InferenceSession look-alike: {'audio': int16 [1,1,L]} -> [probs f32 [1,odim,T]]
    (FireRedVAD/Export_FireRedVAD.py:785-807); a leading batch of windows is accepted."""

    def __init__(self, weights=None, input_audio_length=16000, device="cuda:0", in_sample_rate=16000, long_windows=False):
        """long_windows=True: a long or -- input_audio_length=None -- dynamic export (FireRedEngine).  The dynamic session reports
        [1, 1, "audio_len"] and [1, odim, "n_frames"] (the reference's driver keys on the string, Inference_FireRed_ONNX.py:541-547)
        and accepts any length from 400 samples."""
        self.engine = FireRedEngine(weights, input_audio_length, device, in_sample_rate, long_windows=long_windows)
        dyn = self.engine.dynamic
        self._inputs_meta = [_Meta("audio", [1, 1, "audio_len" if dyn else self.engine.L], "tensor(int16)")]
        self._outputs_meta = [_Meta("probs", [1, self.engine.odim, "n_frames" if dyn else self.engine.T], "tensor(float)")]

    def run(self, output_names, feeds):
        audio = np.asarray(feeds["audio"])
        require_int16(audio)
        if self.engine.dynamic:
            rows = audio.reshape(-1, audio.shape[-1])
            if rows.shape[1] < WINDOW_LENGTH:
                raise ValueError(f"Got invalid dimensions for input: audio, expected last dim >= {WINDOW_LENGTH}")
            pc = self.engine.pack([r for r in rows])
            T = int(pc.frames[0])
            probs = self.engine.run_packed(pc).view(self.engine.odim, rows.shape[0], T).permute(1, 0, 2).contiguous()
            return [probs.cpu().numpy()]
        if audio.shape[-1] != self.engine.L:
            raise ValueError(f"Got invalid dimensions for input: audio, expected last dim {self.engine.L}")
        probs = self.engine.run(audio.reshape(-1, audio.shape[-1])).cpu().numpy()
        return [probs]


class FireRedStreamSession(Session):
    """Stream-VAD session look-alike: {'audio': int16 [1,1,n], 'caches_in': f32 [R,1,P,pad]} ->
    [probs f32 [1,odim,T], caches_out] (FireRedVAD/Export_FireRedVAD.py:848-872; 'audio' axis 2 is dynamic).
    The weights must have no look-ahead filter (cfg N2 == 0)."""

    def __init__(self, weights=None, device="cuda:0"):
        self.engine = FireRedEngine(weights, STREAM_CHUNK_SAMPLES, device)      # None / "" raise in checkpoints.resolve: no silent default
        e = self.engine
        self._inputs_meta = [_Meta("audio", [1, 1, "audio_len"], "tensor(int16)"),
                             _Meta("caches_in", list(e.cache_shape), "tensor(float)")]
        self._outputs_meta = [_Meta("probs", [1, e.odim, "signal_len"], "tensor(float)"),
                              _Meta("caches_out", list(e.cache_shape), "tensor(float)")]

    def run(self, output_names, feeds):
        audio, caches = np.asarray(feeds["audio"]), np.asarray(feeds["caches_in"])
        require_int16(audio)
        if caches.dtype != np.float32 or caches.shape != self.engine.cache_shape:
            raise ValueError(f"Got invalid dimensions for input: caches_in, expected {list(self.engine.cache_shape)}")
        t = self.engine.torch
        probs, cout = self.engine.stream_run(audio.reshape(1, -1), t.from_numpy(np.ascontiguousarray(caches)))
        outs = {"probs": probs.cpu().numpy(), "caches_out": cout.cpu().numpy()}
        return [outs[k] for k in (output_names or ["probs", "caches_out"])]
