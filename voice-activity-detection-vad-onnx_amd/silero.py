"""Silero-VAD on MI355X: drop-in for the reference's Silero boundary objects.

Mirrors (same names / arguments / error behaviour):
  * `OnnxWrapper`            -- Silero/modeling_modified/utils_vad.py:10-146
  * `load_silero_vad`        -- Silero/modeling_modified/model.py:9-41
  * `get_speech_timestamps`  -- Silero/modeling_modified/utils_vad.py:248-491
  * `VADIterator`            -- Silero/modeling_modified/utils_vad.py:494-586 (host drop-in)
plus the batched entry points the reference does not have (`SileroEngine.clips`, `SileroEngine.clips_ragged`: clips of any lengths as one
ragged batch, `get_speech_timestamps_batch`, `VADIteratorBatch`: many live streams on the device).  All arithmetic runs in libvadx.so (HIP, gfx950); this file is
plumbing: tensors in, C-ABI call, tensors out.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

from . import _lib
from . import weights as _weights
from .chunks import collect_chunks, drop_chunks            # noqa: F401  (the reference keeps them beside get_speech_timestamps)
from .stream import StreamBatch

CONTEXT_SIZE = 64
NUM_SAMPLES = 512
HIDDEN = 128
GEOMETRY = {16000: (512, 64), 8000: (256, 32)}      # sampling rate -> (window, context) of the network


def _geom(sampling_rate):
    if int(sampling_rate) not in GEOMETRY:
        raise ValueError(f"Supported sampling rates: [8000, 16000] (got {sampling_rate})")
    return GEOMETRY[int(sampling_rate)]


def _as_weight_dict(path_or_weights):
    """dict | silero_vad.onnx | .npz with the keys of weights.silero_synthetic() | the explicit opt-in "synthetic:<seed>".
    None / "" raises: the reference's default (the silero_vad package's bundled model, model.py:9-41) does not exist here
    and random weights must never be a silent default (checkpoints.resolve)."""
    from . import checkpoints
    w = checkpoints.resolve("silero", path_or_weights)
    w = {k: np.ascontiguousarray(np.asarray(v), dtype=np.float32) for k, v in w.items()}
    _weights.silero_check(w)
    return w


def _as_weight_dict_8k(spec):
    """The 8 kHz network's weights: dict | .npz | "synthetic:<seed>" (checkpoints.resolve("silero8k"))."""
    from . import checkpoints
    w = checkpoints.resolve("silero8k", spec)
    w = {k: np.ascontiguousarray(np.asarray(v), dtype=np.float32) for k, v in w.items()}
    _weights.silero_check(w, sample_rate=8000)
    return w


def _weights_8k_spec(path_or_weights, weights_8k):
    """What SileroEngine loads as its 8 kHz network: `weights_8k` when given; otherwise, for an .onnx `path_or_weights`, that file's
    8 kHz branch when it has one (silero_8k_from_onnx, geometry checked: a branch that contradicts the restated network raises);
    otherwise None."""
    if weights_8k is not None:
        return _as_weight_dict_8k(weights_8k)
    if isinstance(path_or_weights, (str, os.PathLike)) and str(path_or_weights).lower().endswith(".onnx"):
        from . import checkpoints
        w = checkpoints.silero_8k_from_onnx(str(path_or_weights), missing_ok=True)
        if w is not None:
            w = {k: np.ascontiguousarray(np.asarray(v), dtype=np.float32) for k, v in w.items()}
            _weights.silero_check(w, sample_rate=8000)
        return w
    return None


def _pack(w, sample_rate):
    L = _lib.lib()
    hw = _lib.SileroWeightsHost()
    keep = []

    def ptr(a):
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    hw.stft_basis = ptr(w["stft_basis"])
    for i in range(4):
        hw.enc_w[i] = ptr(w[f"enc{i}_w"]).value
        hw.enc_b[i] = ptr(w[f"enc{i}_b"]).value
    hw.lstm_w_ih, hw.lstm_w_hh = ptr(w["lstm_w_ih"]), ptr(w["lstm_w_hh"])
    hw.lstm_b_ih, hw.lstm_b_hh = ptr(w["lstm_b_ih"]), ptr(w["lstm_b_hh"])
    hw.dec_w, hw.dec_b = ptr(w["dec_w"]), ptr(w["dec_b"])
    packed = np.zeros(L.vadx_silero_packed_floats_sr(int(sample_rate)), dtype=np.float32)
    _lib.check(L.vadx_silero_pack_host_sr(int(sample_rate), C.byref(hw), packed.ctypes.data_as(C.c_void_p)))
    return packed


WORKSPACE_CAP_BYTES = 8 << 30     # clips(): above this the gate-preactivation workspace is reused span by span


_default_mode = [None]


def encoder_mode(mode=None):
    """The kernel set engines use unless told otherwise per engine (`SileroEngine.arithmetic`): "f32" = exact-f32 MFMAs, "split" =
    bf16 x 3 exact-split products, "h2" = fp16 x 2 split products (float32-class accuracy at 3/16 of the matrix time; activations
    outside the fp16 range are detected and the batch recomputed on "split").  A Python-side default only -- the C ABI takes the
    arithmetic with every call (include/vadx.h: vadx_silero_cfg).  Returns the mode that was active; `None` only queries.  The initial
    value comes from VADX_SILERO_ENCODER, read once here."""
    return _lib.default_arith(_default_mode, "VADX_SILERO_ENCODER", "encoder", mode)


class SileroEngine:
    """Device-resident packed weights + workspace; thin wrappers over the C ABI."""

    def __init__(self, path_or_weights=None, device="cuda:0", weights_8k=None):
        """path_or_weights: the 16 kHz network (see _as_weight_dict).  weights_8k: the 8 kHz network (dict, .npz, "synthetic:<seed>" or
        an .onnx file's 8 kHz branch); None with an .onnx `path_or_weights` loads that file's 8 kHz branch when it has one, otherwise the
        engine has none (sampling_rate=8000 then raises).  `has_8k` says whether it is there."""
        torch = _lib.require_gpu()
        self.torch = torch
        self.device = torch.device(device)
        L = _lib.lib()
        w = _as_weight_dict(path_or_weights)
        packed = _pack(w, 16000)
        self.packed = torch.from_numpy(packed).to(self.device)
        self._ws = None
        self.arithmetic = None            # None = the module default (encoder_mode()); or "f32" | "split" | "h2" for this engine
        self.h2_ok = bool(packed[L.vadx_silero_packed_floats() - 4] != 0.0)      # the blob's fp16 x 2 section is usable (pack-time check)
        self.range_fallbacks = 0          # batches recomputed on bf16 x 3 because an activation left the fp16 range
        self.packed_8k, self.h2_ok_8k = None, False
        w8 = _weights_8k_spec(path_or_weights, weights_8k)
        if w8 is not None:
            p8 = _pack(w8, 8000)
            self.packed_8k = torch.from_numpy(p8).to(self.device)
            self.h2_ok_8k = bool(p8[L.vadx_silero_packed_floats() - 4] != 0.0)

    @property
    def has_8k(self):
        """True when the engine holds the 8 kHz network (sampling_rate=8000 on every entry point)"""
        return self.packed_8k is not None

    def blob(self, sampling_rate=16000):
        """the device blob of the network for `sampling_rate`"""
        _geom(sampling_rate)
        if int(sampling_rate) == 16000:
            return self.packed
        if self.packed_8k is None:
            raise ValueError(f"sr={sampling_rate}: this engine holds only the 16 kHz sub-graph of the Silero network (build it from an "
                             ".onnx file with an 8 kHz branch, or pass weights_8k= to SileroEngine)")
        return self.packed_8k

    # -- arithmetic selection + the fp16 x 2 range protocol
    def mode(self, sampling_rate=16000):
        m = self.arithmetic or encoder_mode()
        ok = self.h2_ok if int(sampling_rate) == 16000 else self.h2_ok_8k
        return "split" if (m == "h2" and not ok) else m

    def cfg(self, mode=None, sampling_rate=16000):
        """ctypes pointer to a vadx_silero_cfg for `mode` (default: this engine's current mode) and the network of `sampling_rate`"""
        c = _lib.SileroCfg()
        c.arithmetic = _lib.ARITH[mode or self.mode(sampling_rate)]
        c.sample_rate = 8000 if int(sampling_rate) == 8000 else 0
        return C.byref(c)

    def range_flag(self, reset=True, sampling_rate=16000):
        """(flag, largest |activation|) of the fp16 x 2 kernels since the last reset; synchronises the stream (vadx_silero_range_flag)"""
        flag, amax = C.c_uint32(0), C.c_float(0.0)
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_silero_range_flag(self.blob(sampling_rate).data_ptr(), 1 if reset else 0, C.byref(flag),
                                                         C.byref(amax), _lib.stream_ptr()))
        return int(flag.value), float(amax.value)

    def _guarded(self, run, sampling_rate=16000):
        """run(mode) -> result.  On "h2" the result stands only if no activation left the fp16 range; otherwise the batch is recomputed on
        "split" (bf16 terms have float32's range).  One 8-byte read-back + stream synchronisation per guarded call."""
        return _lib.range_guarded(self, self.mode(sampling_rate), run, lambda: self.range_flag(sampling_rate=sampling_rate)[0], "split")

    def _check_workspace_cap(self, batch, steps, who):
        """The whole-batch gx workspace is 32 KB per 16-clip group and window; `clips` falls back to spans above WORKSPACE_CAP_BYTES,
        the int16 / host-feed entry points have no spanned variant and say so instead of running the allocator out of memory."""
        need = _lib.lib().vadx_silero_workspace_bytes(int(batch), int(steps))
        if need > WORKSPACE_CAP_BYTES:
            raise ValueError(f"{who}: a batch of {batch} clips x {steps} windows needs a {need / 2**30:.1f} GiB workspace "
                             f"(cap {WORKSPACE_CAP_BYTES / 2**30:.0f} GiB): split the batch into groups of at most "
                             f"{max(16, WORKSPACE_CAP_BYTES // _lib.lib().vadx_silero_workspace_bytes(16, int(steps)) * 16)} clips, "
                             "or use clips() (float32, spanned automatically)")

    # -- scratch (gx tiles) grows on demand and is reused
    def _workspace(self, batch, steps):
        need = _lib.lib().vadx_silero_workspace_bytes(int(batch), int(steps))
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.torch.empty(need, dtype=self.torch.uint8, device=self.device)
        return self._ws

    def _dev_f32(self, x):
        t = self.torch
        if not t.is_tensor(x):
            x = t.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        return x.to(device=self.device, dtype=t.float32).contiguous()

    def step(self, x, state, sampling_rate=16000):
        """session.run equivalent: x [B,576] ([B,288] at 8000), state [2,B,128] -> (out [B,1], stateN [2,B,128]) on device."""
        t = self.torch
        win, ctx = _geom(sampling_rate)
        blob = self.blob(sampling_rate)
        x = self._dev_f32(x)
        state = self._dev_f32(state)
        if x.dim() != 2 or x.shape[1] != ctx + win:
            raise ValueError(f"input must be [B,{ctx + win}], got {tuple(x.shape)}")
        B = x.shape[0]
        if tuple(state.shape) != (2, B, HIDDEN):
            raise ValueError(f"state must be [2,{B},{HIDDEN}], got {tuple(state.shape)}")
        out = t.empty((B, 1), dtype=t.float32, device=self.device)
        state_n = t.empty_like(state)
        ws = self._workspace(B, 1)

        def run(mode):
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().vadx_silero_step(blob.data_ptr(), x.data_ptr(), state.data_ptr(), int(sampling_rate), B,
                                                       out.data_ptr(), state_n.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       _lib.stream_ptr(), self.cfg(mode, sampling_rate)))
            return out, state_n
        return self._guarded(run, sampling_rate)

    def clips(self, audio, n_samples=None, return_state=False, sampling_rate=16000):
        """audio f32 [B,N] (+-1 scale) -> probs [B, ceil(n/512)] (ceil(n/256) at 8000) on device (zero state/context at t=0)."""
        t = self.torch
        win, _ = _geom(sampling_rate)
        blob = self.blob(sampling_rate)
        audio = self._dev_f32(audio)
        if audio.dim() == 1:
            audio = audio.unsqueeze(0)
        if audio.dim() != 2:
            raise ValueError(f"Too many dimensions for input audio {audio.dim()}")
        B, N = audio.shape
        n = int(N if n_samples is None else n_samples)
        if n <= 0 or n > N:
            raise ValueError(f"n_samples={n} outside (0,{N}]")
        steps = (n + win - 1) // win
        probs = t.empty((B, steps), dtype=t.float32, device=self.device)
        state_n = t.empty((2, B, HIDDEN), dtype=t.float32, device=self.device) if return_state else None
        if _lib.lib().vadx_silero_workspace_bytes(B, steps) > WORKSPACE_CAP_BYTES:
            state_n = self.clips_spanned(audio, n, probs, state_n, sampling_rate=sampling_rate)
            return (probs, state_n) if return_state else probs
        ws = self._workspace(B, steps)

        def run(mode):
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().vadx_silero_clips(blob.data_ptr(), audio.data_ptr(), B, n, _lib.row_stride(audio),
                                                        probs.data_ptr(), None if state_n is None else state_n.data_ptr(),
                                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr(), self.cfg(mode, sampling_rate)))
            return (probs, state_n) if return_state else probs
        return self._guarded(run, sampling_rate)

    def clips_spanned(self, audio, n, probs, state=None, span=None, sampling_rate=16000):
        """`clips` for recordings whose whole-clip workspace (32 KB per 16-clip group and window) would not fit: the
        encoder and the recurrent kernel run span by span over windows [first, first + span) on the caller's stream,
        reusing one span-sized workspace, the LSTM state carried in `state` [2,B,128].  Same kernels and arithmetic
        order as `clips`: identical results.  audio f32 [B,N] on the device; probs [B,steps] is filled."""
        t = self.torch
        L = _lib.lib()
        B = int(audio.shape[0])
        win, _ = _geom(sampling_rate)
        blob = self.blob(sampling_rate)
        steps = (int(n) + win - 1) // win
        tile_bytes = L.vadx_silero_workspace_bytes(B, 1)
        if span is None:
            span = max(1, min(steps, WORKSPACE_CAP_BYTES // tile_bytes))
        if state is None:
            state = t.empty((2, B, HIDDEN), dtype=t.float32, device=self.device)
        ws = self._workspace(B, min(span, steps))

        def run(mode):
            with t.cuda.device(self.device):
                st = _lib.stream_ptr()
                for first in range(0, steps, span):
                    ns = min(span, steps - first)
                    _lib.check(L.vadx_silero_encode_span(blob.data_ptr(), audio.data_ptr(), B, int(n), _lib.row_stride(audio),
                                                         first, ns, ws.data_ptr(), ns * tile_bytes, st, self.cfg(mode, sampling_rate)))
                    _lib.check(L.vadx_silero_recur_span(blob.data_ptr(), ws.data_ptr(), ns * tile_bytes, B, ns,
                                                        None if first == 0 else state.data_ptr(), probs.data_ptr() + 4 * first,
                                                        steps, state.data_ptr(), st, self.cfg(mode, sampling_rate)))
            return state
        return self._guarded(run, sampling_rate)

    def encode(self, audio, n_samples=None, mode=None, sampling_rate=16000):
        """First half of `clips` as its own launch (fills the workspace); returns (batch, steps).  (The separate halves do not run the
        fp16 x 2 range protocol themselves: pair them through `clips*`, or call `range_flag()` before trusting an "h2" result.)"""
        t = self.torch
        B, N = audio.shape
        n = int(N if n_samples is None else n_samples)
        win, _ = _geom(sampling_rate)
        steps = (n + win - 1) // win
        ws = self._workspace(B, steps)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_silero_encode(self.blob(sampling_rate).data_ptr(), audio.data_ptr(), B, n, _lib.row_stride(audio),
                                                     ws.data_ptr(), ws.numel(), _lib.stream_ptr(), self.cfg(mode, sampling_rate)))
        return B, steps

    PCM16_SCALE = 0.000030517578       # Silero/Inference_Silero_VAD_ONNX.py:83: float32 = int16 * this

    def encode_pcm16(self, pcm, n_samples=None, scale=PCM16_SCALE, mode=None, sampling_rate=16000):
        """`encode` fed the int16 samples themselves (device tensor [B,N]): the kernel applies the reference's
        int16 -> float32 scaling while staging, bit-identical to encoding `pcm.float() * float32(scale)`."""
        t = self.torch
        if pcm.dtype != t.int16 or pcm.dim() != 2 or not pcm.is_cuda:
            raise ValueError("encode_pcm16 expects a device int16 tensor [B,N]")
        B, N = pcm.shape
        n = int(N if n_samples is None else n_samples)
        win, _ = _geom(sampling_rate)
        steps = (n + win - 1) // win
        self._check_workspace_cap(B, steps, "encode_pcm16")
        ws = self._workspace(B, steps)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_silero_encode_pcm16(self.blob(sampling_rate).data_ptr(), pcm.data_ptr(), float(scale), B, n,
                                                           _lib.row_stride(pcm), ws.data_ptr(), ws.numel(), _lib.stream_ptr(),
                                                           self.cfg(mode, sampling_rate)))
        return B, steps

    def clips_pcm16(self, pcm, n_samples=None, scale=PCM16_SCALE, sampling_rate=16000):
        """int16 PCM [B,N] on the device -> probs [B, ceil(n/512)] (/256 at 8000) (encode_pcm16 + recur)."""
        def run(mode):
            B, steps = self.encode_pcm16(pcm, n_samples, scale, mode=mode, sampling_rate=sampling_rate)
            return self.recur(B, steps, self.torch.empty((B, steps), dtype=self.torch.float32, device=self.device), mode=mode,
                              sampling_rate=sampling_rate)
        return self._guarded(run, sampling_rate)

    def host_feed(self, batch, n_samples, chunk_clips=512):
        """A reusable upload pipeline for `batch` clips of `n_samples` int16 samples held in HOST memory (the host link,
        not the kernels, bounds an 8-GPU node) -- see HostFeed."""
        return HostFeed(self, batch, n_samples, chunk_clips)

    def clips_from_host(self, host_pcm, chunk_clips=512, feed=None):
        """int16 PCM [B,N] in host memory (numpy or a CPU tensor; pinned memory makes the copies asynchronous) -> probs [B, T]
        on the device, the upload double-buffered against the encoder.  Same scores as `clips_pcm16` of the uploaded batch,
        bit for bit.  Pass a `host_feed(...)` object to reuse its device buffers across calls."""
        t = self.torch
        host = host_pcm if t.is_tensor(host_pcm) else t.from_numpy(np.ascontiguousarray(host_pcm, dtype=np.int16))
        if host.dtype != t.int16 or host.dim() != 2 or host.is_cuda:
            raise ValueError("clips_from_host expects host int16 PCM [B,N]")
        B, N = host.shape
        if feed is None:
            feed = HostFeed(self, B, N, chunk_clips)
        elif (feed.B, feed.N) != (B, N) or feed.eng is not self:
            raise ValueError("clips_from_host: the feed was built for another engine or batch shape")
        def run(mode):
            feed.encode(host, mode=mode)
            return self.recur(B, feed.T, t.empty((B, feed.T), dtype=t.float32, device=self.device), mode=mode)
        return self._guarded(run)

    def recur(self, batch, steps, probs, mode=None, sampling_rate=16000):
        """Second half of `clips`: workspace -> probs [B,steps] (zero initial state)."""
        t = self.torch
        ws = self._workspace(batch, steps)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_silero_recur(self.blob(sampling_rate).data_ptr(), ws.data_ptr(), ws.numel(), batch, steps,
                                                    None, probs.data_ptr(), None, _lib.stream_ptr(), self.cfg(mode, sampling_rate)))
        return probs

    # -- ragged batches (vadx.ragged.RaggedClips; include/vadx.h: "Silero over a RAGGED batch")
    def _ragged_workspace(self, batch, who, whole=False):
        """The gx workspace of a ragged batch: its sum(T_g) tiles of 32 KB, or -- above WORKSPACE_CAP_BYTES -- the tiles of its largest
        part (RaggedClips.parts: runs of whole groups under the cap; one group above it raises there).  whole: the caller cannot run
        in parts."""
        parts = batch.parts(WORKSPACE_CAP_BYTES)
        if whole and len(parts) > 1:
            raise ValueError(f"{who}: a ragged batch of {len(batch)} clips / {batch.tiles} gx tiles needs a {batch.workspace_bytes / 2**30:.1f} "
                             f"GiB workspace (cap {WORKSPACE_CAP_BYTES / 2**30:.0f} GiB, WORKSPACE_CAP_BYTES): the separate halves keep the "
                             "whole batch's gx; clips_ragged runs such a batch in parts")
        first = batch.gx_first_host
        need = max(int(first[g1]) - int(first[g0]) for g0, g1 in parts) * 32768
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.torch.empty(need, dtype=self.torch.uint8, device=self.device)
        return self._ws

    def _ragged_batch(self, batch, who, sampling_rate=None):
        """`batch` as a RaggedClips on this engine's device.  A list is packed for `sampling_rate` (None: 16000); a RaggedClips carries its
        own rate, which an explicit `sampling_rate` must not contradict."""
        from .ragged import RaggedClips
        if not isinstance(batch, RaggedClips):
            self.blob(16000 if sampling_rate is None else sampling_rate)       # (an engine without that network: refused before any upload)
            batch = RaggedClips.from_clips(batch, device=self.device, sampling_rate=16000 if sampling_rate is None else int(sampling_rate))
        elif sampling_rate is not None and int(sampling_rate) != batch.sampling_rate:
            raise ValueError(f"{who}: sampling_rate={sampling_rate}, but the RaggedClips was built for {batch.sampling_rate} Hz "
                             f"(windows of {batch.window} samples)")
        if batch.device is None:
            batch.to(self.device)
        if batch.device != self.device:
            raise ValueError(f"{who}: the batch lives on {batch.device}, the engine on {self.device}")
        return batch

    def encode_ragged(self, batch, mode=None):
        """First half of `clips_ragged` as its own launch (fills the workspace; no range protocol, as `encode`).  The network is the one
        of the batch's rate."""
        t, L = self.torch, _lib.lib()
        rate = batch.sampling_rate
        blob = self.blob(rate)
        ws = self._ragged_workspace(batch, "encode_ragged", whole=True)
        tab = batch.tables()
        k8 = rate == 8000
        with t.cuda.device(self.device):
            if batch.pcm.dtype == t.int16:
                call = L.vadx_silero_encode_ragged_8k_pcm16 if k8 else L.vadx_silero_encode_ragged_pcm16
                _lib.check(call(blob.data_ptr(), batch.pcm.data_ptr(), self.PCM16_SCALE, int(batch.pcm.numel()), C.byref(tab), ws.data_ptr(),
                                ws.numel(), _lib.stream_ptr(), self.cfg(mode, rate)))
            else:
                call = L.vadx_silero_encode_ragged_8k if k8 else L.vadx_silero_encode_ragged
                _lib.check(call(blob.data_ptr(), batch.pcm.data_ptr(), int(batch.pcm.numel()), C.byref(tab), ws.data_ptr(), ws.numel(),
                                _lib.stream_ptr(), self.cfg(mode, rate)))
        return batch

    def recur_ragged(self, batch, probs=None, state_n=None, mode=None):
        """Second half of `clips_ragged`: workspace -> packed scores [batch.n_windows] (+ state_n [2, B, 128] when given)."""
        t, L = self.torch, _lib.lib()
        rate = batch.sampling_rate
        blob = self.blob(rate)
        ws = self._ragged_workspace(batch, "recur_ragged", whole=True)
        if probs is None:
            probs = t.empty(batch.n_windows, dtype=t.float32, device=self.device)
        tab = batch.tables()
        call = L.vadx_silero_recur_ragged_8k if rate == 8000 else L.vadx_silero_recur_ragged
        with t.cuda.device(self.device):
            _lib.check(call(blob.data_ptr(), ws.data_ptr(), ws.numel(), int(batch.pcm.numel()), C.byref(tab), probs.data_ptr(),
                            None if state_n is None else state_n.data_ptr(), _lib.stream_ptr(), self.cfg(mode, rate)))
        return probs

    def clips_ragged(self, batch, return_state=False, sampling_rate=None):
        """A ragged batch (vadx.ragged.RaggedClips, or a list of 1-D float32 / int16 clips) -> (probs_packed float32 [sum T_b],
        probs_first int64 [B + 1]) on the device: clip b's T_b = ceil(len_b / 512) scores (/ 256 at 8000) are probs_packed[probs_first[b] :
        probs_first[b + 1]], bit for bit what `clips` gives for that clip alone; with return_state also state [2, B, 128], every clip's
        LSTM state after its own last window, in the caller's clip order.  sampling_rate (16000 | 8000; None = 16000 for a list, the
        batch's own for a RaggedClips) selects the network.  One encoder and one recurrent launch whose work follows the clips' own
        window counts; a batch whose gx workspace exceeds WORKSPACE_CAP_BYTES runs as PARTS of consecutive groups, one such launch pair
        each, on one cap-sized workspace and this stream -- groups are independent, so the results are the single launch's.  The fp16 x 2
        range protocol as `clips`: one flag read per call, the whole batch recomputed when it is raised."""
        t, L = self.torch, _lib.lib()
        batch = self._ragged_batch(batch, "clips_ragged", sampling_rate)
        rate = batch.sampling_rate
        blob = self.blob(rate)
        ws = self._ragged_workspace(batch, "clips_ragged")
        probs = t.empty(batch.n_windows, dtype=t.float32, device=self.device)
        state_n = t.empty((2, len(batch), HIDDEN), dtype=t.float32, device=self.device) if return_state else None
        pcm16 = batch.pcm.dtype == t.int16
        tabs = batch.part_tables(batch.parts(WORKSPACE_CAP_BYTES))
        call = L.vadx_silero_clips_ragged_8k if rate == 8000 else L.vadx_silero_clips_ragged

        def run(mode):
            with t.cuda.device(self.device):
                for tab in tabs:       # stream order keeps a part's encoder behind the recurrence of the part before it
                    _lib.check(call(blob.data_ptr(), batch.pcm.data_ptr(), 1 if pcm16 else 0, self.PCM16_SCALE, int(batch.pcm.numel()),
                                    C.byref(tab), probs.data_ptr(), None if state_n is None else state_n.data_ptr(), ws.data_ptr(),
                                    ws.numel(), _lib.stream_ptr(), self.cfg(mode, rate)))
            return (probs, batch.probs_first, state_n) if return_state else (probs, batch.probs_first)
        return self._guarded(run, rate)

    def segments_ragged(self, probs, probs_first, n_samples, cap=64, **kw):
        """`segments` on packed scores: probs float32 [sum T_b], probs_first int64 [B + 1] (device; a RaggedClips goes in as it is) ->
        (int64 [B, cap, 2] sample indices, int32 [B] counts), the tables `segments` gives for the per-clip rows."""
        t = self.torch
        if hasattr(probs_first, "probs_first"):
            probs_first = probs_first.probs_first
        first = probs_first.to(device=self.device, dtype=t.int64).contiguous()
        B = int(first.shape[0]) - 1
        if t.is_tensor(n_samples):
            lens = n_samples.to(device=self.device, dtype=t.int64).reshape(-1).contiguous()
        else:
            lens = t.as_tensor(np.asarray(n_samples, dtype=np.int64).reshape(-1).copy(), device=self.device)
        if lens.shape[0] != B:
            raise ValueError(f"{lens.shape[0]} lengths for {B} clips")
        if int(kw.get("sampling_rate", 16000)) not in (16000, 8000):
            raise ValueError(f"segments_ragged: sampling_rate={kw['sampling_rate']} is not 16000 or 8000")
        prm = seg_params(**kw)
        while True:
            segs = t.empty((B, cap, 2), dtype=t.int64, device=self.device)
            counts = t.empty((B,), dtype=t.int32, device=self.device)
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().vadx_silero_segments_ragged(probs.data_ptr(), first.data_ptr(), B, lens.data_ptr(), C.byref(prm),
                                                                  segs.data_ptr(), counts.data_ptr(), cap, _lib.stream_ptr()))
            worst = int(counts.max().item())
            if worst <= cap:
                return segs, counts
            cap = worst          # rare: a clip produced more segments than the table holds -> rerun

    def segments(self, probs, n_samples, cap=64, **kw):
        """Device segmenter: probs [B,T] -> (int64 [B,cap,2] sample indices, int32 [B] counts)."""
        t = self.torch
        probs = self._dev_f32(probs)
        B, T = probs.shape
        if t.is_tensor(n_samples):             # clip lengths may already live on the device
            lens = n_samples.to(device=self.device, dtype=t.int64).reshape(-1).expand(B).contiguous()
        else:
            lens = t.as_tensor(np.broadcast_to(np.asarray(n_samples, dtype=np.int64), (B,)).copy(), device=self.device)
        prm = seg_params(**kw)
        while True:
            segs = t.empty((B, cap, 2), dtype=t.int64, device=self.device)
            counts = t.empty((B,), dtype=t.int32, device=self.device)
            with t.cuda.device(self.device):
                _lib.check(_lib.lib().vadx_silero_segments(probs.data_ptr(), B, T, lens.data_ptr(), C.byref(prm),
                                                           segs.data_ptr(), counts.data_ptr(), cap, _lib.stream_ptr()))
            worst = int(counts.max().item())
            if worst <= cap:
                return segs, counts
            cap = worst          # rare: a clip produced more segments than the table holds -> rerun


class HostFeed:
    """Pinned-host -> device feed of the batched encoder.  Chunks of `chunk_clips` clips cross PCIe on a copy
    stream into one of two device int16 buffers while the encoder of the previous chunk runs on the caller's stream
    (`vadx_silero_encode_pcm16_part` fills the chunk's slice of the ONE batch workspace); the recurrent kernel then runs once
    over the whole batch.  int16 is what a host has (wav files): the encoder applies the reference's x 0.000030517578 itself,
    bit-identically (Silero/Inference_Silero_VAD_ONNX.py:83).  Measured on one MI355X, 4096 x 10 s: 23.7 ms per batch against
    23.0 ms for the upload alone (57 GB/s of PCIe Gen5 x16) -- the compute is hidden completely."""

    def __init__(self, engine, batch, n_samples, chunk_clips=512):
        t = engine.torch
        self.eng, self.B, self.N = engine, int(batch), int(n_samples)
        self.T = (self.N + NUM_SAMPLES - 1) // NUM_SAMPLES
        engine._check_workspace_cap(self.B, self.T, "HostFeed")
        self.chunk = max(16, (int(chunk_clips) + 15) // 16 * 16)       # slices of the workspace start on a 16-clip group boundary
        self.buf = [t.empty((self.chunk, self.N), dtype=t.int16, device=engine.device) for _ in range(2)]
        self.copy_stream = t.cuda.Stream(device=engine.device)
        self.ready = [t.cuda.Event() for _ in range(2)]
        self.free = [t.cuda.Event() for _ in range(2)]
        self.in_use = [False, False]

    def encode(self, host_pcm, mode=None):
        """Upload + encode every chunk of host_pcm [B,N] (int16 CPU tensor); afterwards the engine's workspace holds the batch
        (call `engine.recur(B, T, probs)` next, on the same stream)."""
        eng, t = self.eng, self.eng.torch
        if tuple(host_pcm.shape) != (self.B, self.N) or host_pcm.dtype != t.int16 or host_pcm.is_cuda:
            raise ValueError(f"HostFeed.encode expects host int16 PCM [{self.B},{self.N}]")
        ws = eng._workspace(self.B, self.T)
        L = _lib.lib()
        with t.cuda.device(eng.device):
            comp = t.cuda.current_stream()
            st = _lib.stream_ptr()
            for k2, b0 in enumerate(range(0, self.B, self.chunk)):
                nb = min(self.chunk, self.B - b0)
                k = k2 & 1
                with t.cuda.stream(self.copy_stream):
                    if self.in_use[k]:                  # the encoder launch that last read this buffer (also across calls)
                        self.copy_stream.wait_event(self.free[k])
                    self.buf[k][:nb].copy_(host_pcm[b0:b0 + nb], non_blocking=True)
                    self.ready[k].record(self.copy_stream)
                comp.wait_event(self.ready[k])
                _lib.check(L.vadx_silero_encode_pcm16_part(eng.packed.data_ptr(), self.buf[k].data_ptr(), eng.PCM16_SCALE, nb, self.N,
                                                           self.N, b0, self.B, ws.data_ptr(), ws.numel(), st, eng.cfg(mode)))
                self.free[k].record(comp)
                self.in_use[k] = True
        return self.B, self.T


def seg_params(threshold=0.5, sampling_rate=16000, min_speech_duration_ms=250,
               max_speech_duration_s=float("inf"), min_silence_duration_ms=100, speech_pad_ms=30,
               neg_threshold=None, min_silence_at_max_speech=98, use_max_poss_sil_at_max_speech=True, **_ignored):
    p = _lib.SileroSegParams()
    p.threshold = float(threshold)
    p.neg_threshold = -1.0 if neg_threshold is None else float(neg_threshold)
    p.sampling_rate = int(sampling_rate)
    p.min_speech_duration_ms = float(min_speech_duration_ms)
    p.max_speech_duration_s = float(max_speech_duration_s)
    p.min_silence_duration_ms = float(min_silence_duration_ms)
    p.speech_pad_ms = float(speech_pad_ms)
    p.min_silence_at_max_speech = float(min_silence_at_max_speech)
    p.use_max_poss_sil_at_max_speech = 1 if use_max_poss_sil_at_max_speech else 0
    return p


class SileroSession:
    """What the reference's OnnxWrapper holds as `self.session`: run(None, {'input' [B, ctx + n], 'state' [2,B,128], 'sr' int64})
    -> [out [B,1], stateN [2,B,128]] (utils_vad.py:116-119).  sr = 16000 runs the 16 kHz sub-graph (576-sample input), sr = 8000 the 8 kHz
    one (288-sample input, 128-point STFT, 65-channel first conv: csrc/silero8k.hip) when the engine holds its weights (`has_8k`);
    otherwise an 8000 Hz call fails loudly."""

    def __init__(self, engine):
        self.engine = engine

    def run(self, output_names, feeds):
        sr = int(np.asarray(feeds["sr"]))
        if sr != 16000 and not (sr == 8000 and self.engine.has_8k):
            raise ValueError(f"sr={sr}: only the 16 kHz sub-graph of the Silero network is loaded on the HIP path "
                             "(the engine has no 8 kHz weights: SileroEngine(..., weights_8k=...))")
        out, state = self.engine.step(feeds["input"], feeds["state"], sampling_rate=sr)
        return [out, state]


class OnnxWrapper:
    """Drop-in for the reference wrapper (utils_vad.py:10-146): validation, state / context carry, reset rules."""

    def __init__(self, path=None, force_onnx_cpu=True, device="cuda:0"):
        self.engine = path if isinstance(path, SileroEngine) else SileroEngine(path, device)
        self.torch = self.engine.torch
        self.session = SileroSession(self.engine)
        self.reset_states()
        if isinstance(path, str) and "16k" in path:
            warnings.warn("This model support only 16000 sampling rate!")
            self.sample_rates = [16000]
        else:
            self.sample_rates = [8000, 16000]        # utils_vad.py:63-67; an 8000 Hz call reaches SileroSession.run (8 kHz net or refusal)

    def _validate_input(self, x, sr: int):
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() > 2:
            raise ValueError(f"Too many dimensions for input audio chunk {x.dim()}")
        if sr != 16000 and (sr % 16000 == 0):
            x = x[:, ::sr // 16000]
            sr = 16000
        if sr not in self.sample_rates:
            raise ValueError(f"Supported sampling rates: {self.sample_rates} (or multiply of 16000)")
        if sr / x.shape[1] > 31.25:
            raise ValueError("Input audio chunk is too short")
        return x, sr

    def reset_states(self, batch_size=1):
        t = self.torch
        self._state = t.zeros((2, batch_size, HIDDEN), dtype=t.float32, device=self.engine.device)
        self._context = t.zeros(0)
        self._last_sr = 0
        self._last_batch_size = 0

    def __call__(self, x, sr: int):
        t = self.torch
        if not t.is_tensor(x):
            x = t.as_tensor(np.asarray(x, dtype=np.float32))
        x, sr = self._validate_input(x, sr)
        num_samples = NUM_SAMPLES if sr == 16000 else 256
        if x.shape[-1] != num_samples:
            raise ValueError(f"Provided number of samples is {x.shape[-1]} "
                             "(Supported values: 256 for 8000 sample rate, 512 for 16000)")
        batch_size = x.shape[0]
        context_size = CONTEXT_SIZE if sr == 16000 else 32
        if not self._last_batch_size:
            self.reset_states(batch_size)
        if self._last_sr and self._last_sr != sr:
            self.reset_states(batch_size)
        if self._last_batch_size and self._last_batch_size != batch_size:
            self.reset_states(batch_size)
        x = x.to(device=self.engine.device, dtype=t.float32)
        if not len(self._context):
            self._context = t.zeros(batch_size, context_size, device=self.engine.device)
        x = t.cat([self._context, x], dim=1)
        out, state = self.session.run(None, {"input": x, "state": self._state, "sr": np.array(sr, dtype="int64")})
        self._state = state if t.is_tensor(state) else t.as_tensor(np.asarray(state), device=self.engine.device)
        self._context = x[..., -context_size:]
        self._last_sr = sr
        self._last_batch_size = batch_size
        return out.cpu() if t.is_tensor(out) else t.as_tensor(np.asarray(out))

    def audio_forward(self, x, sr: int):
        """Whole clips in ONE device call (the reference loops window by window, utils_vad.py:130-146).  At 8000 Hz that needs the
        wrapper's own session over an engine with the 8 kHz network; otherwise this loops through `__call__` as the reference does, so a
        substituted session sees exactly the reference's feeds."""
        t = self.torch
        if not t.is_tensor(x):
            x = t.as_tensor(np.asarray(x, dtype=np.float32))
        x, sr = self._validate_input(x, sr)
        self.reset_states()
        if sr == 8000 and type(self.session) is SileroSession and self.session.engine is self.engine and self.engine.has_8k:
            probs, state = self.engine.clips(x, return_state=True, sampling_rate=8000)
            pad = (-x.shape[1]) % 256
            xp = t.nn.functional.pad(x.to(self.engine.device, t.float32), (0, pad))
            self._state, self._context = state, xp[:, -32:]
            self._last_sr, self._last_batch_size = sr, x.shape[0]
            return probs.cpu()
        if sr != 16000:
            num_samples = 256
            if x.shape[1] % num_samples:
                x = t.nn.functional.pad(x, (0, num_samples - (x.shape[1] % num_samples)), "constant", value=0.0)
            return t.cat([self(x[:, i:i + num_samples], sr) for i in range(0, x.shape[1], num_samples)], dim=1).cpu()
        probs, state = self.engine.clips(x, return_state=True)
        # leave the wrapper exactly where the reference's loop would: last state + last 64 samples
        pad = (-x.shape[1]) % NUM_SAMPLES
        xp = t.nn.functional.pad(x.to(self.engine.device, t.float32), (0, pad))
        self._state, self._context = state, xp[:, -CONTEXT_SIZE:]
        self._last_sr, self._last_batch_size = sr, x.shape[0]
        return probs.cpu()


class _IterMachine:
    """VADIterator's per-stream state machine (utils_vad.py:535-585) on one window's score; the device runs the same steps in double
    (csrc/silero_stream.hip: silero_stream_iter_kernel).  step(p, n) -> (kind, value): kind 0 none / 1 start / 2 end, value the sample
    position the reference computes before int()."""

    def __init__(self, threshold, sampling_rate, min_silence_duration_ms, speech_pad_ms):
        self.threshold = threshold
        self.min_silence_samples = sampling_rate * min_silence_duration_ms / 1000
        self.speech_pad_samples = sampling_rate * speech_pad_ms / 1000
        self.reset()

    def reset(self):
        self.triggered, self.temp_end, self.current_sample = False, 0, 0

    def step(self, p, n):
        self.current_sample += n
        speech = p >= self.threshold
        if speech and self.temp_end:
            self.temp_end = 0
        if speech:
            if self.triggered:
                return 0, None
            self.triggered = True
            return 1, max(0, self.current_sample - self.speech_pad_samples - n)
        if not (p < self.threshold - 0.15 and self.triggered):
            return 0, None
        if not self.temp_end:
            self.temp_end = self.current_sample
        if self.current_sample - self.temp_end < self.min_silence_samples:
            return 0, None
        end = self.temp_end + self.speech_pad_samples - n
        self.temp_end, self.triggered = 0, False
        return 2, end


def _event(kind, value, sampling_rate, return_seconds, time_resolution):
    if kind not in (1, 2):
        return None
    return {"start" if kind == 1 else "end": round(value / sampling_rate, time_resolution) if return_seconds else int(value)}


class VADIterator:
    """Drop-in for the reference's stream iterator (utils_vad.py:494-586): one stream, one model call per chunk on the host.
    `model` is anything the reference accepts (vadx.silero.OnnxWrapper, or a stand-in with reset_states() and __call__(x, sr)).
    Many streams at once: VADIteratorBatch."""

    def __init__(self, model, threshold: float = 0.5, sampling_rate: int = 16000, min_silence_duration_ms: int = 100,
                 speech_pad_ms: int = 30):
        self.model = model
        self.threshold = threshold
        self.sampling_rate = sampling_rate
        if sampling_rate not in [8000, 16000]:
            raise ValueError("VADIterator does not support sampling rates other than [8000, 16000]")
        self._m = _IterMachine(threshold, sampling_rate, min_silence_duration_ms, speech_pad_ms)
        self.min_silence_samples = self._m.min_silence_samples
        self.speech_pad_samples = self._m.speech_pad_samples
        self.reset_states()

    def reset_states(self):
        self.model.reset_states()
        self._m.reset()

    triggered = property(lambda self: self._m.triggered)
    temp_end = property(lambda self: self._m.temp_end)
    current_sample = property(lambda self: self._m.current_sample)

    def __call__(self, x, return_seconds=False, time_resolution: int = 1):
        import torch
        if not torch.is_tensor(x):
            try:
                x = torch.Tensor(x)
            except Exception:
                raise TypeError("Audio cannot be casted to tensor. Cast it manually")
        n = len(x[0]) if x.dim() == 2 else len(x)
        with torch.no_grad():
            p = self.model(x, self.sampling_rate).item()
        kind, value = self._m.step(p, n)
        return _event(kind, value, self.sampling_rate, return_seconds, time_resolution)


class VADIteratorBatch(StreamBatch):
    """`streams` live Silero streams on the device (vadx_silero_stream_run): every call advances each stream by k windows of 512
    samples (256 at 8 kHz); context, LSTM state and VADIterator machine of every stream stay in the device `record` (DESIGN.md "Stream
    batches"; its first 2*S*128 floats are the LSTM state [2,S,128]), and the start / end events come back from the device.  Per stream,
    the scores are bit for bit what `SileroEngine.clips` gives for the concatenated audio.  On "h2" every tick reads the range flag and,
    when it is raised, recomputes the tick on "split" from the same record."""

    def __init__(self, model, streams, threshold: float = 0.5, sampling_rate: int = 16000, min_silence_duration_ms: int = 100,
                 speech_pad_ms: int = 30):
        engine = model.engine if isinstance(model, OnnxWrapper) else model
        if not isinstance(engine, SileroEngine):
            raise TypeError("VADIteratorBatch needs a vadx.silero.OnnxWrapper or SileroEngine")
        if sampling_rate not in [8000, 16000]:
            raise ValueError("VADIterator does not support sampling rates other than [8000, 16000]")
        if sampling_rate != 16000 and not engine.has_8k:
            raise ValueError(f"sr={sampling_rate}: only the 16 kHz sub-graph of the Silero network is loaded on the HIP path "
                             "(the engine has no 8 kHz weights: SileroEngine(..., weights_8k=...))")
        super().__init__(engine, streams, _lib.lib().vadx_silero_stream_state_bytes(int(streams)))
        self.sampling_rate = sampling_rate
        p = _lib.SileroIterParams()
        p.threshold, p.sampling_rate = float(threshold), int(sampling_rate)
        p.min_silence_duration_ms, p.speech_pad_ms = float(min_silence_duration_ms), float(speech_pad_ms)
        self._prm = p
        self._ws = None

    @property
    def state(self):
        return self.record[:2 * self.streams * HIDDEN * 4].view(self.engine.torch.float32).view(2, self.streams, HIDDEN)

    def step(self, x, active=None):
        """x [S, k*512] ([S, k*256] at 8 kHz; float32 on the +-1 scale, or int16 PCM; host or device, numpy or torch) -> device tensors
        (kind int8 [S,k], value float64 [S,k], probs float32 [S,k]); kind 0 none / 1 start / 2 end / -1 score not finite,
        value the sample position before int().  active (bool [S], None = all): False = no audio for that stream this tick."""
        eng, t = self.engine, self.engine.torch
        win, _ = _geom(self.sampling_rate)
        S = self.streams
        x = self._samples(x, f"[{S}, k*{win}]", lambda x: x.shape[1] == 0 or x.shape[1] % win, floats=True).to(eng.device).contiguous()
        k = x.shape[1] // win
        act, _, reset_d, act_d, src, dst = self._begin(None, active)
        L = _lib.lib()
        need = L.vadx_silero_stream_workspace_bytes(S, k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = t.empty(need, dtype=t.uint8, device=eng.device)
        kind = t.empty((S, k), dtype=t.int8, device=eng.device)
        value = t.empty((S, k), dtype=t.float64, device=eng.device)
        probs = t.empty((S, k), dtype=t.float32, device=eng.device)
        pcm = x.dtype == t.int16

        def run(mode):
            with t.cuda.device(eng.device):
                _lib.check(L.vadx_silero_stream_run(eng.blob(self.sampling_rate).data_ptr(), C.byref(self._prm), x.data_ptr(),
                                                    1 if pcm else 0, eng.PCM16_SCALE, k * win, S, k,
                                                    None if reset_d is None else reset_d.data_ptr(),
                                                    None if act_d is None else act_d.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                                    probs.data_ptr(), kind.data_ptr(), value.data_ptr(), self._ws.data_ptr(),
                                                    self._ws.numel(), _lib.stream_ptr(), eng.cfg(mode, self.sampling_rate)))
        eng._guarded(run, self.sampling_rate)
        self._end(act)
        return kind, value, probs

    # -- ragged ticks: every stream its own number of windows (vadx_silero_stream_plan + vadx_silero_stream_run_ragged)
    def _ragged_samples(self, x, counts, max_windows, win):
        """-> (samples tensor [S, n >= max(counts) * win] on the device, counts int32 [S]); a list of S 1-D host arrays of whole windows
        (empty allowed) carries its own counts."""
        from . import ragged
        eng, t, S = self.engine, self.engine.torch, self.streams
        if isinstance(x, (list, tuple)):
            if counts is not None:
                raise ValueError("counts= goes with a [S, n] array: a list's rows carry their own lengths")
            if len(x) != S:
                raise ValueError(f"a list of samples must have {S} rows, got {len(x)}")
            rows = [np.asarray(r.cpu() if hasattr(r, "cpu") else r) for r in x]
            kinds = {r.dtype for r in rows if r.size}
            if any(r.ndim != 1 for r in rows) or len(kinds) > 1 or any(k != np.int16 and k.kind != "f" for k in kinds):
                raise ValueError("a list of samples must hold 1-D arrays, all float or all int16")
            if any(r.shape[0] % win for r in rows):
                raise ValueError(f"every row of a list of samples must be whole windows of {win} samples")
            counts = ragged.stream_counts(np.array([r.shape[0] // win for r in rows], dtype=np.int64), S, max_windows)
            dt = np.int16 if kinds == {np.dtype(np.int16)} else np.float32
            x = np.zeros((S, max(int(counts.max()), 1) * win), dtype=dt)
            for s, r in enumerate(rows):
                x[s, :r.shape[0]] = r
        else:
            if counts is None:
                raise ValueError("step_ragged needs counts with a [S, n] array")
            counts = ragged.stream_counts(counts, S, max_windows)
        top = int(counts.max())
        x = self._samples(x, f"[{S}, >= max(counts) * {win} = {top * win}]", lambda x: x.shape[1] < top * win, floats=True)
        return x.to(eng.device).contiguous(), counts

    def step_ragged(self, x, counts=None, max_windows=None):
        """A tick in which stream s advances by counts[s] windows, 0 = no audio (which costs nothing; the record and a pending reset are
        kept).  x [S, >= max(counts) * 512] (256 at 8 kHz), the first counts[s] windows of row s valid -- host or device, numpy or torch,
        float or int16 -- or a list of S 1-D host arrays of whole windows (counts then come from the list).  max_windows (None = the cap
        of 256 a ragged tick has) bounds the counts.  -> (kind int8, value float64, probs float32, first): packed device vectors
        [sum(counts)] of which stream s owns first[s] .. first[s + 1] (first: host int64 [S + 1]); kinds and values as `step`.  Bad
        counts raise ValueError before anything is launched.  `step` stays the path for uniform ticks (it is faster there)."""
        from . import ragged
        eng, t, S = self.engine, self.engine.torch, self.streams
        win, _ = _geom(self.sampling_rate)
        x, counts = self._ragged_samples(x, counts, max_windows, win)
        plan = ragged.stream_plan(counts, win)
        first = np.zeros(S + 1, dtype=np.int64)
        np.cumsum(counts, out=first[1:])
        n = plan.n_windows
        kind = t.empty(n, dtype=t.int8, device=eng.device)
        value = t.empty(n, dtype=t.float64, device=eng.device)
        probs = t.empty(n, dtype=t.float32, device=eng.device)
        if plan.groups == 0:         # nobody delivered audio: no launch, the record and the pending resets stay
            return kind, value, probs, first
        L = _lib.lib()
        mw = plan.max_windows
        need = L.vadx_silero_stream_ragged_workspace_bytes(S, mw, plan.tiles)
        if need > WORKSPACE_CAP_BYTES:
            raise ValueError(f"step_ragged: {S} streams x at most {mw} windows ({plan.tiles} gx tiles) need a {need / 2**30:.1f} GiB "
                             f"workspace (cap {WORKSPACE_CAP_BYTES / 2**30:.0f} GiB, WORKSPACE_CAP_BYTES): a tick is not run in parts")
        if self._ws is None or self._ws.numel() < need:
            self._ws = t.empty(need, dtype=t.uint8, device=eng.device)
        act = counts > 0
        _, _, reset_d, _, src, dst = self._begin(None, act, upload_active=False)
        # the host tables in one copy; the per-stream tables are written on the device
        host, at = plan.staging()
        dev = t.from_numpy(host).to(eng.device)
        slots = 16 * plan.groups
        out = t.empty(2 * (S + 1) + 2 * slots + 2 * slots + 2, dtype=t.int32, device=eng.device)     # probs_first | slot_off | len | clip | status
        p_first, p_off = out.data_ptr(), out.data_ptr() + 8 * (S + 1)
        p_len = p_off + 8 * slots
        p_clip, p_status = p_len + 4 * slots, p_len + 8 * slots
        out[-2:].zero_()
        base = dev.data_ptr()
        rg = _lib.SileroRagged(p_off, p_len, p_clip, base + 4 * at["gx_first"], base + 4 * at["grp_min_len"], base + 4 * at["wg_tab"],
                               p_first, p_status, S, plan.groups, plan.n_runs, plan.tiles)
        pcm = x.dtype == t.int16
        with t.cuda.device(eng.device):
            _lib.check(L.vadx_silero_stream_plan(base + 4 * at["counts"], base + 4 * at["bucket_first"], S, mw, win, plan.groups, p_first,
                                                 p_off, p_len, p_clip, p_status, self._ws.data_ptr(), self._ws.numel(), _lib.stream_ptr()))

        def run(mode):
            with t.cuda.device(eng.device):
                _lib.check(L.vadx_silero_stream_run_ragged(eng.blob(self.sampling_rate).data_ptr(), C.byref(self._prm), x.data_ptr(),
                                                           1 if pcm else 0, eng.PCM16_SCALE, x.stride(0), S, mw, C.byref(rg),
                                                           None if reset_d is None else reset_d.data_ptr(), src.data_ptr(), dst.data_ptr(),
                                                           probs.data_ptr(), kind.data_ptr(), value.data_ptr(), self._ws.data_ptr(),
                                                           self._ws.numel(), _lib.stream_ptr(), eng.cfg(mode, self.sampling_rate)))
        eng._guarded(run, self.sampling_rate)
        self._end(act)
        return kind, value, probs, first

    def call_ragged(self, x, counts=None, max_windows=None, return_seconds=False, time_resolution: int = 1):
        """Per stream, the list of the counts[s] results that counts[s] calls of the reference's VADIterator give (dict or None); [] for
        a stream without audio."""
        kind, value, _, first = self.step_ragged(x, counts, max_windows)
        kind, value = kind.cpu().numpy(), value.cpu().numpy()
        return [[_event(int(kd), float(v), self.sampling_rate, return_seconds, time_resolution)
                 for kd, v in zip(kind[first[s]:first[s + 1]], value[first[s]:first[s + 1]])] for s in range(self.streams)]

    def __call__(self, x, active=None, return_seconds=False, time_resolution: int = 1):
        """Per stream, what k calls of the reference's VADIterator would return: a list of k entries (dict or None); [] for an
        inactive stream."""
        kind, value, _ = self.step(x, active)
        kind, value = kind.cpu().numpy(), value.cpu().numpy()
        act = np.ones(self.streams, dtype=bool) if active is None else self._mask(active, "active")
        out = []
        for s in range(self.streams):
            if not act[s]:
                out.append([])
                continue
            out.append([_event(int(kd), float(v), self.sampling_rate, return_seconds, time_resolution)
                        for kd, v in zip(kind[s], value[s])])
        return out


def segments_from_probs(engine, probs, lengths, **kw):
    """The segmenter half of get_speech_timestamps on given window probabilities (device state machine, utils_vad.py:374-482):
    probs [B, T] (T windows of 512 samples at 16 kHz / 256 at 8 kHz), lengths [B] in samples -> list of per-clip lists of
    {'start','end'}.  kw as get_speech_timestamps (threshold, sampling_rate, min_speech_duration_ms, ..., return_seconds)."""
    engine = engine.engine if isinstance(engine, OnnxWrapper) else engine
    return_seconds = kw.pop("return_seconds", False)
    time_resolution = kw.pop("time_resolution", 1)
    sr = kw.get("sampling_rate", 16000)
    if sr not in (8000, 16000):
        raise ValueError("Currently silero VAD models support 8000 and 16000 (or multiply of 16000) sample rates")
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    segs, counts = engine.segments(probs, lens, **kw)
    return _finish(segs, counts, lens, sr, return_seconds, time_resolution, 1)


def load_silero_vad(onnx=True, opset_version=16, use_cpu=True, path="", device="cuda:0"):
    """Constructor of the boundary object (reference signature; `use_cpu` is accepted and ignored: this build runs on the
    MI355X only).  `path` = the silero_vad.onnx the reference would hand to onnxruntime (its initialisers are read by
    vadx.onnx_reader), a .npz of arrays, or "synthetic:<seed>"; the reference's `path=""` default (the pip package's bundled
    file) cannot be honoured here and raises.  An .onnx file's 8 kHz branch is loaded too, so the model serves sr = 8000 as well."""
    if onnx and opset_version not in (15, 16):
        raise Exception("Available ONNX opset_version: [15, 16]")
    return OnnxWrapper(path or None, force_onnx_cpu=use_cpu, device=device)


def _finish(segs, counts, lengths, sampling_rate, return_seconds, time_resolution, step):
    out = []
    segs = segs.cpu().numpy()
    counts = counts.cpu().numpy()
    for b in range(segs.shape[0]):
        row = []
        for s, e in segs[b, :counts[b]].tolist():
            if return_seconds:
                dur = int(lengths[b]) / sampling_rate
                row.append({"start": max(round(s / sampling_rate, time_resolution), 0),
                            "end": min(round(e / sampling_rate, time_resolution), dur)})
            elif step > 1:
                row.append({"start": s * step, "end": e * step})
            else:
                row.append({"start": s, "end": e})
        out.append(row)
    return out


def _segments_on_device(audio, model, lengths, sampling_rate, **seg_kw):
    """The device half of get_speech_timestamps_batch: -> (engine, audio f32 [B, N] as given (before decimation and masking), lens
    int64 [B] host (in samples of the network's rate), sampling_rate the network runs at, step, probs, segs, counts); probs / segs /
    counts are None for empty audio."""
    engine = model.engine if isinstance(model, OnnxWrapper) else model
    t = engine.torch
    audio = engine._dev_f32(audio)
    if audio.dim() == 1:
        audio = audio.unsqueeze(0)
    given = audio
    step = 1
    if sampling_rate > 16000 and sampling_rate % 16000 == 0:
        step = sampling_rate // 16000
        sampling_rate = 16000
        audio = audio[:, ::step].contiguous()
        warnings.warn("Sampling rate is a multiply of 16000, casting to 16000 manually!")
    if sampling_rate not in (8000, 16000):
        raise ValueError("Currently silero VAD models support 8000 and 16000 (or multiply of 16000) sample rates")
    if sampling_rate == 8000 and not engine.has_8k:
        raise ValueError("sampling_rate=8000: only the 16 kHz sub-graph of the Silero network is loaded on the HIP path (the engine has no "
                         "8 kHz weights); window probabilities from elsewhere can be segmented with segments_from_probs(..., sampling_rate=8000)")
    B, N = audio.shape
    if N == 0:           # empty audio: the reference's chunk loop never runs and it returns [] (utils_vad.py:330-344)
        return engine, given, np.zeros((B,), np.int64), sampling_rate, step, None, None, None
    if lengths is None:
        lens = np.full((B,), N, dtype=np.int64)
    else:
        lens = np.asarray(lengths, dtype=np.int64)
        if step > 1:
            lens = (lens + step - 1) // step
        if lens.shape != (B,) or lens.min() <= 0 or lens.max() > N:
            raise ValueError("lengths must be B positive values <= audio.shape[1]")
        if lens.min() != N:      # zero everything past each clip's end (the reference zero-pads the last window)
            mask = t.arange(N, device=engine.device).unsqueeze(0) < t.as_tensor(lens, device=engine.device).unsqueeze(1)
            audio = audio * mask
    probs = engine.clips(audio, n_samples=int(lens.max()), sampling_rate=sampling_rate)
    segs, counts = engine.segments(probs, lens, sampling_rate=sampling_rate, **seg_kw)
    return engine, given, lens, sampling_rate, step, probs, segs, counts


def _is_ragged(audio):
    from .ragged import RaggedClips
    return isinstance(audio, (list, tuple, RaggedClips))


def _segments_ragged(audio, model, lengths, sampling_rate, **seg_kw):
    """The device half of the batch entry points for a LIST of clips (or a vadx.ragged.RaggedClips): one ragged encoder + recurrent launch
    and the ragged segmenter -> (engine, batch, lens int64 [B] host, probs_packed, segs, counts)."""
    engine = model.engine if isinstance(model, OnnxWrapper) else model
    if sampling_rate not in (8000, 16000) and sampling_rate % 16000 == 0:
        raise ValueError(f"sampling_rate={sampling_rate}: a list of clips runs Silero's ragged path at 16000 or 8000 Hz only (a multiple of "
                         "16000 is decimated only in the [B, N] array form); pass the array with lengths=, or decimate the clips")
    if sampling_rate not in (8000, 16000):
        raise ValueError("Currently silero VAD models support 8000 and 16000 (or multiply of 16000) sample rates")
    if sampling_rate == 8000 and not engine.has_8k:
        raise ValueError("sampling_rate=8000: only the 16 kHz sub-graph of the Silero network is loaded on the HIP path (the engine has no "
                         "8 kHz weights: SileroEngine(..., weights_8k=...))")
    if lengths is not None:
        raise ValueError("lengths= goes with a [B, N] array: a list's clips carry their own lengths")
    batch = engine._ragged_batch(audio, "get_speech_timestamps_batch", sampling_rate)
    probs, first = engine.clips_ragged(batch)
    segs, counts = engine.segments_ragged(probs, first, batch.lengths, sampling_rate=batch.sampling_rate, **seg_kw)
    return engine, batch, batch.lengths, probs, segs, counts


def get_speech_timestamps_batch(audio, model, lengths=None, threshold: float = 0.5, sampling_rate: int = 16000,
                                min_speech_duration_ms: int = 250, max_speech_duration_s: float = float("inf"),
                                min_silence_duration_ms: int = 100, speech_pad_ms: int = 30,
                                return_seconds: bool = False, time_resolution: int = 1,
                                neg_threshold: float = None, min_silence_at_max_speech: int = 98,
                                use_max_poss_sil_at_max_speech: bool = True, return_probs: bool = False):
    """Batched get_speech_timestamps: audio f32 [B,N] (equal length, or `lengths` per clip with
    zero padding beyond) -> list (per clip) of lists of {'start','end'} dicts.
    audio may also be a LIST of 1-D clips (float32 on the +-1 scale, or int16) of any lengths, or a vadx.ragged.RaggedClips: the clips
    then run as one ragged batch (16000 or 8000 Hz; a RaggedClips must have been built for `sampling_rate`) -- every clip pays for its own windows, not for the longest clip's -- with the same
    lists; return_probs gives the list of per-clip score vectors (views of one packed vector)."""
    if _is_ragged(audio):
        engine, batch, lens, probs, segs, counts = _segments_ragged(
            audio, model, lengths, sampling_rate, threshold=threshold, min_speech_duration_ms=min_speech_duration_ms,
            max_speech_duration_s=max_speech_duration_s, min_silence_duration_ms=min_silence_duration_ms, speech_pad_ms=speech_pad_ms,
            neg_threshold=neg_threshold, min_silence_at_max_speech=min_silence_at_max_speech,
            use_max_poss_sil_at_max_speech=use_max_poss_sil_at_max_speech)
        res = _finish(segs, counts, lens, batch.sampling_rate, return_seconds, time_resolution, 1)
        return (res, batch.rows(probs)) if return_probs else res
    engine, given, lens, sampling_rate, step, probs, segs, counts = _segments_on_device(
        audio, model, lengths, sampling_rate, threshold=threshold, min_speech_duration_ms=min_speech_duration_ms,
        max_speech_duration_s=max_speech_duration_s, min_silence_duration_ms=min_silence_duration_ms, speech_pad_ms=speech_pad_ms,
        neg_threshold=neg_threshold, min_silence_at_max_speech=min_silence_at_max_speech,
        use_max_poss_sil_at_max_speech=use_max_poss_sil_at_max_speech)
    if probs is None:
        t = engine.torch
        res = [[] for _ in range(given.shape[0])]
        return (res, t.empty((given.shape[0], 0), dtype=t.float32, device=engine.device)) if return_probs else res
    res = _finish(segs, counts, lens, sampling_rate, return_seconds, time_resolution, step)
    return (res, probs) if return_probs else res


def get_speech_timestamps_table(audio, model, lengths=None, sampling_rate: int = 16000, time_resolution: int = 1, fusion_threshold=None,
                                min_duration=None, sample_rule="nearest", **kw):
    """The device half of get_speech_timestamps_batch(return_seconds=True): the same launches, then one vadx_timestamps_samples launch
    instead of the per-row round() on the host -> a vadx.tstable.TimestampTable whose `lists()` are those dicts.  With fusion_threshold
    and min_duration the table also carries the process_timestamps pass that `drivers.inference_silero` runs over them.  **kw: the
    segmenter arguments (threshold, min_speech_duration_ms, ...).  Only time_resolution = 1.  `chunks_table()` holds the seconds as
    sample rows of the rate the network ran at (16000 for a multiple of it)."""
    from . import tstable
    if time_resolution != 1:
        raise ValueError(f"time_resolution={time_resolution}: the device table rounds to one decimal (time_resolution=1) only")
    if _is_ragged(audio):        # a list of clips / a RaggedClips: the ragged launches, the same table
        engine, batch, lens, probs, segs, counts = _segments_ragged(audio, model, lengths, sampling_rate, **kw)
        return tstable.from_samples(segs, counts, lens, batch.sampling_rate, fusion_threshold, min_duration, sample_rule=sample_rule)
    engine, given, lens, sampling_rate, step, probs, segs, counts = _segments_on_device(audio, model, lengths, sampling_rate, **kw)
    if probs is None:
        return tstable.empty(given.shape[0], engine.device, sampling_rate, dicts=True)
    return tstable.from_samples(segs, counts, lens, sampling_rate, fusion_threshold, min_duration, sample_rule=sample_rule)


def get_speech_audio_batch(audio, model, lengths=None, drop=False, align=1, return_seconds: bool = False, time_resolution: int = 1,
                           sampling_rate: int = 16000, **kw):
    """Timestamps AND the audio they select, without the table leaving the device: clips -> segments -> chunks plan -> chunks copy, with
    one 16-byte read (the size of the packed result) in between.  audio f32 [B, N] and `lengths` as get_speech_timestamps_batch, **kw its
    segmenter arguments (threshold, min_speech_duration_ms, ...); drop=True keeps what is NOT speech (drop_chunks), align as
    vadx.chunks.collect_chunks_batch.  -> (packed float32, offsets int64 [B+1], timestamps): clip b's samples are
    packed[offsets[b] : offsets[b+1]] (up to alignment filler); `timestamps` is what get_speech_timestamps_batch returns.  With a
    sampling rate that is a multiple of 16000 the network sees every step-th sample and the cut is made in the audio as given."""
    from . import chunks
    if _is_ragged(audio):        # a list of clips / a RaggedClips: the cut is made in the batch's own packed vector
        engine, batch, lens, probs, segs, counts = _segments_ragged(audio, model, lengths, sampling_rate, **kw)
        run = chunks.drop_chunks_batch if drop else chunks.collect_chunks_batch
        packed, offsets = run((segs, counts), batch.pcm, lengths=lens, clip_offsets=batch.clip_off, align=align)
        return packed, offsets, _finish(segs, counts, lens, batch.sampling_rate, return_seconds, time_resolution, 1)
    engine, given, lens, sampling_rate, step, probs, segs, counts = _segments_on_device(audio, model, lengths, sampling_rate, **kw)
    t = engine.torch
    B = given.shape[0]
    if probs is None:
        return t.empty(0, dtype=t.float32, device=engine.device), t.zeros(B + 1, dtype=t.int64, device=engine.device), [[] for _ in range(B)]
    full = np.full((B,), given.shape[1], np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)
    run = chunks.drop_chunks_batch if drop else chunks.collect_chunks_batch
    packed, offsets = run((segs * step if step > 1 else segs, counts), given, lengths=full, align=align)
    return packed, offsets, _finish(segs, counts, lens, sampling_rate, return_seconds, time_resolution, step)


def get_speech_timestamps(audio, model, threshold: float = 0.5, sampling_rate: int = 16000,
                          min_speech_duration_ms: int = 250, max_speech_duration_s: float = float("inf"),
                          min_silence_duration_ms: int = 100, speech_pad_ms: int = 30, return_seconds: bool = False,
                          time_resolution: int = 1, visualize_probs: bool = False, progress_tracking_callback=None,
                          neg_threshold: float = None, window_size_samples: int = 512,
                          min_silence_at_max_speech: int = 98, use_max_poss_sil_at_max_speech: bool = True):
    """Single-clip reference signature (utils_vad.py:248-263); runs the whole clip in one device pass."""
    torch = _lib.require_gpu()
    if not torch.is_tensor(audio):
        try:
            audio = torch.Tensor(audio)
        except Exception:
            raise TypeError("Audio cannot be casted to tensor. Cast it manually")
    if len(audio.shape) > 1:
        for _ in range(len(audio.shape)):
            audio = audio.squeeze(0)
        if len(audio.shape) > 1:
            raise ValueError("More than one dimension in audio. Are you trying to process audio with 2 channels?")
    if visualize_probs:
        raise NotImplementedError("visualize_probs is outside the hot path (SURVEY §2 row 10)")
    res = get_speech_timestamps_batch(audio.unsqueeze(0), model, None, threshold, sampling_rate,
                                      min_speech_duration_ms, max_speech_duration_s, min_silence_duration_ms,
                                      speech_pad_ms, return_seconds, time_resolution, neg_threshold,
                                      min_silence_at_max_speech, use_max_poss_sil_at_max_speech)[0]
    if progress_tracking_callback:
        progress_tracking_callback(100.0)
    return res
