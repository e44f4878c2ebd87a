"""NVIDIA Frame-VAD MarbleNet v2.0 on MI355X: ORT-session boundary + the window loop of
NVIDIA_.../Inference_NVIDIA_MarbleNet_VAD_ONNX.py:130-147,369-402.

The encoder/decoder classes live in NeMo (not in the reference tree); weights come as the
checkpoint's conv + BatchNorm tensors and are BN-folded at load exactly like the reference's
`fold_bn_into_conv1d` (Export_NVIDIA_MarbleNet_VAD.py:58-105)."""
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
from .session import Session, _Meta, io_types, require_int16
from .stream import StreamBatch

SAMPLE_RATE = 16000
OUTPUT_FRAME_SHIFT_S = 320 / 16000


def _pad16(a, axes):
    pads = [(0, 0)] * a.ndim
    for ax in axes:
        pads[ax] = (0, (-a.shape[ax]) % 16)
    return np.ascontiguousarray(np.pad(a, pads), dtype=np.float32)


MAX_CHANNELS, MAX_TILE_FIELD = 128, 100      # csrc/marblenet.hip: MAXC, IN_LD_MAX


def check_blocks(blocks):
    """The layouts vadx_sepconv_block takes (include/vadx.h, next to vadx_sepconv_cfg), checked before anything is uploaded or launched:
    at most 128 channels, a 32-frame tile's receptive field of at most 100 frames, plain blocks 1x1 at stride 1, and the residual
    contract -- the kernel reads the block input with the output's frame index, so no sub-block of a residual block may change the frame
    count (a stride, or an even kernel, which 'same' padding turns into T - 1)."""
    for bi, (filt, rep, k, stride, dil, residual, sep) in enumerate(blocks):
        what = f"MarbleNet block {bi} {(filt, rep, k, stride, dil, residual, sep)}"
        if not (1 <= filt <= MAX_CHANNELS and rep >= 1 and k >= 1 and stride >= 1 and dil >= 1):
            raise ValueError(f"{what}: filters must be in [1, {MAX_CHANNELS}], repeat / kernel / stride / dilation at least 1")
        if not sep and (k != 1 or stride != 1):
            raise ValueError(f"{what}: a plain (non-separable) block must be a 1x1 conv at stride 1")
        if 31 * stride + (k - 1) * dil + 1 > MAX_TILE_FIELD:
            raise ValueError(f"{what}: the receptive field of a 32-frame tile, 31 * stride + (kernel - 1) * dilation + 1 = "
                             f"{31 * stride + (k - 1) * dil + 1}, exceeds {MAX_TILE_FIELD} frames")
        if residual and (stride != 1 or (dil * (k - 1)) % 2):
            raise ValueError(f"{what}: a residual block must keep the frame count (stride 1 and an odd kernel in every sub-block): "
                             "its input is added frame by frame to its output")


class MarbleNetEngine:
    def __init__(self, weights=None, device="cuda:0", blocks=None, bn_eps=None, in_sample_rate=16000):
        """in_sample_rate: the export's IN_SAMPLE_RATE (Export_NVIDIA_MarbleNet_VAD.py:237-254): audio arrives at that rate and
        the graph resamples every window to 16 kHz itself."""
        if blocks is not None:
            check_blocks(blocks)
        torch = _lib.require_gpu()
        self.in_sample_rate = int(in_sample_rate)
        self.torch = torch
        self.device = torch.device(device)
        w = _checkpoints.resolve("marblenet", weights)
        blocks = _weights.MARBLENET_BLOCKS if blocks is None else blocks
        eps = _weights.MARBLENET_BN_EPS if bn_eps is None else bn_eps
        self.stages = []          # (cfg, dev tensors..., block_start flag)
        cin = 80
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)   # noqa: E731
        for bi, (filt, rep, k, stride, dil, residual, sep) in enumerate(blocks):
            block_cin = cin
            for r in range(rep):
                p = f"b{bi}r{r}"
                pw, pb = _weights.fold_bn(np.asarray(w[p + "_pw"])[:, :, None], None, w[p + "_gamma"], w[p + "_beta"],
                                          w[p + "_mean"], w[p + "_var"], eps)
                last = r == rep - 1
                cfg = _lib.SepConvCfg(cin, filt, k, stride, dil, 1 if sep else 0, block_cin if (residual and last) else 0, 1)
                st = {"cfg": cfg, "dw": dev(w[p + "_dw"]) if sep else None, "pw": dev(_lib.frag_major(pw[:, :, 0])),
                      "pb": dev(_pad16(pb, (0,))), "rw": None, "rb": None, "first": r == 0, "res": residual and last,
                      "pw_host": _pad16(pw[:, :, 0], (0, 1)), "rw_host": None}
                if residual and last:
                    rw, rb = _weights.fold_bn(np.asarray(w[f"b{bi}res_pw"])[:, :, None], None, w[f"b{bi}res_gamma"],
                                              w[f"b{bi}res_beta"], w[f"b{bi}res_mean"], w[f"b{bi}res_var"], eps)
                    st["rw"], st["rb"] = dev(_lib.frag_major(rw[:, :, 0])), dev(_pad16(rb, (0,)))
                    st["rw_host"] = _pad16(rw[:, :, 0], (0, 1))
                self.stages.append(st)
                cin = filt
        self.cout = cin
        self.dec_w, self.dec_b = dev(w["dec_w"]), dev(w["dec_b"])
        self._fe = {}
        self._fe_ragged = None
        # the published 3x2x64 layout runs on the fused kernels: one launch per residual block, one for blocks 5 + 6 + decoder
        self.fused = tuple(tuple(b) for b in blocks) == tuple(tuple(b) for b in _weights.MARBLENET_BLOCKS)
        # fp16 x 2 split products for the 1x1 convs of the fused residual blocks (csrc/split2.h; include/vadx.h: vadx_marblenet_cfg)
        self.arithmetic = None            # None = the module default (_lib.gemm_mode()); "h2" | "f32" ("split" has no form here: float32)
        self.h2_ok = False
        self.range_fallbacks = 0          # batches recomputed on float32 because an activation left the fp16 range
        self._flag = torch.zeros(2, dtype=torch.int32, device=self.device)
        if self.fused:
            self.h2_ok = True
            for k in range(0, 9):             # prologue + blocks 5 / 6 of the tail launch (plane order), blocks 2-4 (kgemm_h's k order)
                st = self.stages[k]
                for name in ("pw", "rw"):
                    host = st[name + "_host"]
                    # k order: the fused block whose input has 128 channels (stages 1, 2) splits its operand in the GEMM waves (K_QUARTER);
                    # the 64-channel blocks, the prologue and the tail read operand planes (K_PLAIN)
                    frags = None if host is None else _lib.frag_h2(host, _lib.H2_K_QUARTER if k in (1, 2) else _lib.H2_K_PLAIN)
                    st[name + "_h"] = None if frags is None else dev(frags)
                    self.h2_ok = self.h2_ok and (host is None or frags is not None)

    def mode(self):
        m = self.arithmetic or _lib.gemm_mode()
        return "h2" if (m == "h2" and self.h2_ok) else "f32"

    def h2_macs_per_out_frame(self):
        """Multiply-accumulates per encoder output frame that run as fp16 x 2 split products when mode() is "h2": every 1x1 conv whose
        `_h` fragments _run_fused hands to a launch (prologue, the fused blocks' point-wise + residual convs, both tail blocks).
        bench_models.flop_marblenet_h2_out_frame prices exactly this set on the fp16 pipe."""
        mac = 0
        for st in self.stages:
            for name in ("pw", "rw"):
                if st.get(name + "_h") is not None:
                    mac += (st["cfg"].cin if name == "pw" else st["cfg"].residual_cin) * st["cfg"].cout
        return mac

    def frontend(self, L):
        if L not in self._fe:
            self._fe[L] = _frontend.Frontend("marblenet", L, device=self.device, in_sample_rate=self.in_sample_rate)
        return self._fe[L]

    def frontend_ragged(self):
        """The one Frontend behind `logmel_ragged`: its tables do not depend on a window length (the length it is built with is only
        a valid placeholder), so clips of every length share it."""
        if self.in_sample_rate != SAMPLE_RATE:
            raise ValueError(f"the ragged path has no in-graph resampling: in_sample_rate is {self.in_sample_rate}, not {SAMPLE_RATE}")
        if self._fe_ragged is None:
            self._fe_ragged = _frontend.Frontend("marblenet", SAMPLE_RATE, device=self.device)
        return self._fe_ragged

    def ragged(self, clips, device=True):
        """The packed batch of `clips` (list of 1-D int16 arrays of any lengths; vadx.ragged.RaggedFrames).  device=None keeps it on the host."""
        return _ragged.RaggedFrames.from_clips(clips, self.device if device is True else device)

    def run_ragged(self, rf):
        """RaggedFrames -> (score_silence, score_active f32 [sum T1_b] packed, enc_first int32 [B+1] on the host): clip b's scores are
        [enc_first[b], enc_first[b+1]), bit for bit what `run(clip_b[None])` gives.  One front-end launch and five encoder launches for
        the whole batch, whatever the lengths; the fp16 x 2 range protocol covers the whole batch (a raised flag recomputes all of it on
        float32 and counts once in range_fallbacks).  The published 3x2x64 layout only."""
        if not self.fused:
            raise ValueError("MarbleNetEngine.run_ragged: ragged batches are built for the published MarbleNet 3x2x64 layout (the fused "
                             "kernels); this engine was constructed with another `blocks` layout -- run its clips one length at a time")
        if rf.device is None:
            rf.to(self.device)
        x = self.frontend_ragged().logmel_ragged(rf)
        s0, s1 = _lib.range_guarded(self, self.mode(), lambda m: self._run_fused_ragged(x, rf, m), lambda: _lib.take_flag(self._flag), "f32")
        return s0, s1, rf.enc_first_host

    def _run_fused_ragged(self, x, rf, mode):
        """`_run_fused` over packed clips: the same five launches, (clip, tile) from rf's tables; the activation between two launches
        is clip b's [C][T1_b] block at float offset C * enc_first[b]."""
        t, lib, st = self.torch, _lib.lib(), self.stages
        p = lambda a: None if a is None else a.data_ptr()        # noqa: E731
        n = rf.n_enc
        with t.cuda.device(self.device):
            rt = rf.encoder_tables()
            mc = _lib.MarbleNetCfg(_lib.ARITH[mode], 0, self._flag.data_ptr())
            sfx = "_h" if mode == "h2" else ""
            s0 = st[0]
            cur = t.empty((n * s0["cfg"].cout,), dtype=t.float32, device=self.device)
            _lib.check(lib.vadx_sepconv_block_ragged(C.byref(s0["cfg"]), p(s0["dw"]), p(s0["pw" + sfx]), p(s0["pb"]), x.data_ptr(), x.shape[1],
                                                     cur.data_ptr(), C.byref(rt), _lib.stream_ptr(), C.byref(mc)))
            for k in (1, 3, 5):
                a, b = st[k], st[k + 1]
                y = t.empty((n * 64,), dtype=t.float32, device=self.device)
                _lib.check(lib.vadx_marblenet_block2_ragged(a["cfg"].cin, a["cfg"].kernel, p(a["dw"]), p(a["pw" + sfx]), p(a["pb"]), p(b["dw"]),
                                                            p(b["pw" + sfx]), p(b["pb"]), p(b["rw" + sfx]), p(b["rb"]), cur.data_ptr(),
                                                            y.data_ptr(), C.byref(rt), _lib.stream_ptr(), C.byref(mc)))
                cur = y
            s0o = t.empty((n,), dtype=t.float32, device=self.device)
            s1o = t.empty((n,), dtype=t.float32, device=self.device)
            _lib.check(lib.vadx_marblenet_tail_ragged(p(st[7]["dw"]), p(st[7]["pw" + sfx]), p(st[7]["pb"]), p(st[8]["pw" + sfx]), p(st[8]["pb"]),
                                                      self.dec_w.data_ptr(), self.dec_b.data_ptr(), cur.data_ptr(), s0o.data_ptr(),
                                                      s1o.data_ptr(), C.byref(rt), _lib.stream_ptr(), C.byref(mc)))
        return s0o, s1o

    def run(self, audio_i16, windows_per_clip=1, window_len=None):
        """audio int16 [B, W*L] -> (score_silence, score_active f32 [B*W, T'], signal_len = T' - 1)."""
        t = self.torch
        if not t.is_tensor(audio_i16):
            audio_i16 = t.from_numpy(np.ascontiguousarray(audio_i16, dtype=np.int16))
        a = audio_i16.to(self.device)
        L = int(a.shape[-1] // windows_per_clip if window_len is None else window_len)
        return self.run_features(self.frontend(L).logmel(a, windows_per_clip, L))

    def run_features(self, x):
        """log-mel float32 [N, T, 80], time-major and contiguous, on the device (what `frontend(L).logmel` returns)
        -> (score_silence, score_active f32 [N, T'], signal_len = T' - 1): everything of `run` behind the front-end."""
        t = self.torch
        if not (t.is_tensor(x) and x.dtype == t.float32 and x.dim() == 3 and x.shape[2] == 80 and x.is_contiguous()
                and x.shape[0] > 0 and x.shape[1] > 0):
            raise ValueError("run_features takes a contiguous float32 [N, T, 80] tensor")
        N, T = x.shape[0], x.shape[1]
        xs = (T * 80, 1, 80)
        cur, cur_T = x, T
        block_in = None
        lib = _lib.lib()
        if self.fused:
            # an activation that leaves the fp16 range: the batch again on float32 MFMAs
            return _lib.range_guarded(self, self.mode(), lambda m: self._run_fused(x, N, T, m), lambda: _lib.take_flag(self._flag), "f32")
        with t.cuda.device(self.device):
            for st in self.stages:
                cfg = st["cfg"]
                if st["first"]:
                    block_in = cur
                pad = (cfg.dilation * (cfg.kernel - 1)) // 2
                t_out = (cur_T + 2 * pad - cfg.dilation * (cfg.kernel - 1) - 1) // cfg.stride + 1
                y = t.empty((N, cfg.cout, t_out), dtype=t.float32, device=self.device)
                _lib.check(lib.vadx_sepconv_block(C.byref(cfg), None if st["dw"] is None else st["dw"].data_ptr(),
                                                  st["pw"].data_ptr(), st["pb"].data_ptr(),
                                                  None if st["rw"] is None else st["rw"].data_ptr(),
                                                  None if st["rb"] is None else st["rb"].data_ptr(),
                                                  cur.data_ptr(), xs[0], xs[1], xs[2], cur_T,
                                                  block_in.data_ptr() if st["res"] else None, y.data_ptr(), N, t_out,
                                                  _lib.stream_ptr(), None))
                cur, cur_T = y, t_out
                xs = (cfg.cout * t_out, t_out, 1)
            s0 = t.empty((N, cur_T), dtype=t.float32, device=self.device)
            s1 = t.empty((N, cur_T), dtype=t.float32, device=self.device)
            _lib.check(lib.vadx_frame_classifier(cur.data_ptr(), self.dec_w.data_ptr(), self.dec_b.data_ptr(), N, self.cout,
                                                 cur_T, s0.data_ptr(), s1.data_ptr(), _lib.stream_ptr()))
        return s0, s1, cur_T - 1

    def run_from_host(self, host_i16, windows_per_clip=1, window_len=None, chunk_clips=256, feed=None):
        """`run` fed from HOST memory (int16 [B, W*L], ideally pinned: vadx.feed.pin), the upload of chunk k + 1 overlapped with the
        launches of chunk k (vadx.feed.HostPcmFeed); bit-identical to `run` of the resident batch."""
        from . import feed as _feed
        f = feed or _feed.HostPcmFeed(self.device, host_i16.shape[1], chunk_clips)
        return _feed.cat_results(f.map([host_i16], lambda a: self.run(a, windows_per_clip, window_len)))

    def _run_fused(self, x, N, T, mode="f32"):
        """Published layout: block 1 (stride 2, time-major log-mel in) through the per-sub-block entry, blocks 2-4 as one
        fused launch each (the tensor between a block's two sub-blocks stays in LDS), blocks 5 + 6 + Linear + softmax as one
        launch (nothing but the two scores per frame is written)."""
        t, lib, st = self.torch, _lib.lib(), self.stages
        p = lambda a: None if a is None else a.data_ptr()        # noqa: E731
        with t.cuda.device(self.device):
            s0 = st[0]
            cfg = s0["cfg"]
            pad = (cfg.dilation * (cfg.kernel - 1)) // 2
            T1 = (T + 2 * pad - cfg.dilation * (cfg.kernel - 1) - 1) // cfg.stride + 1
            cur = t.empty((N, cfg.cout, T1), dtype=t.float32, device=self.device)
            mc = _lib.MarbleNetCfg(_lib.ARITH[mode], 0, self._flag.data_ptr())
            sfx = "_h" if mode == "h2" else ""
            _lib.check(lib.vadx_sepconv_block(C.byref(cfg), p(s0["dw"]), p(s0["pw" + sfx]), p(s0["pb"]), None, None, x.data_ptr(),
                                              T * 80, 1, 80, T, None, cur.data_ptr(), N, T1, _lib.stream_ptr(), C.byref(mc)))
            for k in (1, 3, 5):
                a, b = st[k], st[k + 1]
                y = t.empty((N, 64, T1), dtype=t.float32, device=self.device)
                _lib.check(lib.vadx_marblenet_block2(a["cfg"].cin, a["cfg"].kernel, p(a["dw"]), p(a["pw" + sfx]), p(a["pb"]), p(b["dw"]),
                                                     p(b["pw" + sfx]), p(b["pb"]), p(b["rw" + sfx]), p(b["rb"]), cur.data_ptr(), y.data_ptr(),
                                                     N, T1, _lib.stream_ptr(), C.byref(mc)))
                cur = y
            s0o = t.empty((N, T1), dtype=t.float32, device=self.device)
            s1o = t.empty((N, T1), dtype=t.float32, device=self.device)
            _lib.check(lib.vadx_marblenet_tail(p(st[7]["dw"]), p(st[7]["pw" + sfx]), p(st[7]["pb"]), p(st[8]["pw" + sfx]), p(st[8]["pb"]),
                                               self.dec_w.data_ptr(), self.dec_b.data_ptr(), cur.data_ptr(), s0o.data_ptr(),
                                               s1o.data_ptr(), N, T1, _lib.stream_ptr(), C.byref(mc)))
        return s0o, s1o, T1 - 1

    def detect(self, clips_i16, window_len=None, pad_noise=None, post=(3, 0.5, 10, 1000, 10, 3, 0), return_probs=False):
        """Equal-length clips int16 [B,N] (host) -> per clip [(start_s, end_s)].  window_len None = the
        dynamic-axis mode (one window = the whole clip, up to 3600 s, :130-135).
        A LIST (or tuple) of 1-D clips of any lengths runs as one ragged batch in either mode (`_list_track`); clip b's result is
        that of the [1, N] call on it alone, and return_probs then gives (segments, tracks f32 [B, max n_frames], decisions, n_frames).
        Dynamic-axis clips the ragged kernels do not take (longer than 3600 s: they are cut into windows; every clip when the graph
        resamples) keep the one-call-per-clip path and are spliced back in input order."""
        as_list = isinstance(clips_i16, (list, tuple))
        if as_list and not self.fused:
            raise ValueError("MarbleNetEngine.detect: a list of clips (a ragged batch) is built for the published MarbleNet 3x2x64 layout; this "
                             "engine was constructed with another `blocks` layout -- pass equal-length clips as a [B, N] array")
        rate = self.in_sample_rate
        pp = _vadpost.VadPostprocessor(*post, frame_shift_s=OUTPUT_FRAME_SHIFT_S, frame_length_s=None, device=self.device)
        if isinstance(clips_i16, (_ragged.RaggedBatch, _ragged.RaggedFrames)):        # packed already (from_clips / from_packed): as a list
            track, nf, lengths = self._batch_track(clips_i16)
            out, dec = track_segments(pp, track, nf, [int(n) / rate for n in lengths])
            return (out, track, dec, nf) if return_probs else out
        if not as_list:
            B, n = np.asarray(clips_i16).shape
            L = min(rate * 3600, n) if window_len is None else int(window_len)
            padded, W = pad_batch(clips_i16, L, L, pad_noise)
            s0, s1, slen = self.run(padded, W, L)
            valid = min(slen, s1.shape[1])
            track = s1.view(B, W, -1)[:, :, :valid].reshape(B, W * valid).contiguous()
            out, dec = track_segments(pp, track, None, [n / rate] * B)
            return (out, track, dec) if return_probs else out
        clips = [np.asarray(c) for c in clips_i16]
        if len(clips) == 0:
            raise ValueError("a ragged batch needs at least one clip")
        odd = [b for b, c in enumerate(clips) if window_len is None and (rate != SAMPLE_RATE or c.size > rate * 3600)]
        if not odd:
            track, nf, lengths = self._list_track(clips, window_len, pad_noise)
            out, dec = track_segments(pp, track, nf, [int(n) / rate for n in lengths])
            return (out, track, dec, nf) if return_probs else out
        rows = [None] * len(clips)                  # per clip (segments, track [n_frames[b]], decisions [n_frames[b]])
        for b in odd:                               # today's path, one call per clip
            o, tr, de = self.detect(clips[b].reshape(1, -1), None, None if pad_noise is None else np.asarray(pad_noise[b])[None, :], post, True)
            rows[b] = (o[0], tr[0], de[0])
        rag = [b for b in range(len(clips)) if b not in odd]
        if rag:
            track, nf, lengths = self._list_track([clips[b] for b in rag], None, None)
            out, dec = track_segments(pp, track, nf, [int(n) / rate for n in lengths])
            for k, b in enumerate(rag):
                rows[b] = (out[k], track[k, :nf[k]], dec[k, :nf[k]])
        out = [r[0] for r in rows]
        if not return_probs:
            return out
        nfs = np.array([r[1].shape[0] for r in rows], dtype=np.int32)
        return out, self._pad_rows([r[1] for r in rows], self.torch.float32), self._pad_rows([r[2] for r in rows], self.torch.int8), nfs

    def detect_table(self, clips_i16, window_len=None, pad_noise=None, post=(3, 0.5, 10, 1000, 10, 3, 0), sample_rule="nearest"):
        """`detect` with the tracks and the frame table staying on the device (`clips.track_table`: one vadx_vadpost launch, one
        vadx_timestamps_frames launch) -> a vadx.tstable.TimestampTable whose `lists()` is what `detect` returns and whose
        `chunks_table()` goes straight to vadx.chunks.collect_chunks_batch (sample rows at in_sample_rate, by `sample_rule`).
        A list holding a clip that `detect` would run on its own (dynamic axis: longer than 3600 s, or a graph that resamples) is
        refused: one table is one launch sequence."""
        as_list = isinstance(clips_i16, (list, tuple))
        if as_list and not self.fused:
            raise ValueError("MarbleNetEngine.detect_table: a list of clips (a ragged batch) is built for the published MarbleNet 3x2x64 layout; "
                             "this engine was constructed with another `blocks` layout -- pass equal-length clips as a [B, N] array")
        rate = self.in_sample_rate
        pp = _vadpost.VadPostprocessor(*post, frame_shift_s=OUTPUT_FRAME_SHIFT_S, frame_length_s=None, device=self.device)
        if isinstance(clips_i16, (_ragged.RaggedBatch, _ragged.RaggedFrames)):
            track, nf, lengths = self._batch_track(clips_i16)
            return track_table(pp, track, nf, [int(n) / rate for n in lengths], rate, sample_rule)[0]
        if not as_list:
            B, n = np.asarray(clips_i16).shape
            L = min(rate * 3600, n) if window_len is None else int(window_len)
            padded, W = pad_batch(clips_i16, L, L, pad_noise)
            s0, s1, slen = self.run(padded, W, L)
            valid = min(slen, s1.shape[1])
            track = s1.view(B, W, -1)[:, :, :valid].reshape(B, W * valid).contiguous()
            return track_table(pp, track, None, [n / rate] * B, rate, sample_rule)[0]
        clips = [np.asarray(c) for c in clips_i16]
        if len(clips) == 0:
            raise ValueError("a ragged batch needs at least one clip")
        if window_len is None and (rate != SAMPLE_RATE or any(c.size > rate * 3600 for c in clips)):
            raise ValueError("MarbleNetEngine.detect_table: a dynamic-axis clip longer than 3600 s, or a graph that resamples, runs one call per "
                             "clip in `detect`; build the table from clips the ragged kernels take, or pass window_len")
        track, nf, lengths = self._list_track(clips, window_len, pad_noise)
        return track_table(pp, track, nf, [int(n) / rate for n in lengths], rate, sample_rule)[0]

    def _list_track(self, clips, window_len, pad_noise):
        """A list of 1-D int16 clips of any lengths -> (track f32 [B, max n_frames] on the device, n_frames int32 [B], lengths [B]).
        Dynamic axis: RaggedFrames -> logmel_ragged -> run_ragged, one score per encoder frame.  window_len = L (the static export):
        the clips padded to their own window grids (vadx.ragged.RaggedBatch), every window through the unchanged front-end and
        `run_features`.  Either way one vadx_tracks_gather, and the track is the input of one vadx_vadpost launch."""
        if window_len is None:
            return self._batch_track(self.ragged(clips))
        L = int(window_len)
        return self._batch_track(_ragged.RaggedBatch.from_clips(clips, L, L, pad_noise, None, self.device))

    def ragged_packed(self, pcm, clip_offsets, lengths, window_len=None, pad_noise=None, normalize=None):
        """The batch `detect` builds from a list of clips, for clips that already lie in device memory: a RaggedFrames (window_len None,
        the dynamic axis) or a RaggedBatch on the grid window = stride = window_len, packed on the device (`from_packed`);
        normalize="rms" applies timestamps.normalise_audio on the way.  `detect` / `detect_table` take the result as they take a list."""
        if window_len is None:
            return _ragged.RaggedFrames.from_packed(pcm, clip_offsets, lengths, normalize, device=self.device)
        L = int(window_len)
        return _ragged.RaggedBatch.from_packed(pcm, clip_offsets, lengths, L, L, pad_noise, normalize, device=self.device)

    def _batch_track(self, batch):
        """`_list_track` of a batch that is packed already: a RaggedFrames (dynamic axis) or a RaggedBatch on a grid of window = stride = L
        (from_clips or from_packed: the PCM of a from_packed batch was never on the host)."""
        if isinstance(batch, _ragged.RaggedFrames):
            rf = batch
            _, s1, _ = self.run_ragged(rf)
            nf = (rf.enc_frames - 1).astype(np.int32)           # valid_b = min(signal_len, T1_b) = T1_b - 1
            return gather_tracks(self.device, s1, 1, 0, 1, rf.enc_first, nf), nf, rf.lengths
        rb = batch
        L = rb.window
        if rb.stride != L:
            raise ValueError(f"the batch was packed for windows of {rb.window} every {rb.stride} samples, MarbleNet cuts {L} every {L}")
        if rb.device is None:
            rb.to(self.device)
        s0, s1, slen = self.run_features(self.frontend(L).logmel(rb.gather(), 1, L))
        T1 = int(s1.shape[1])
        valid = min(slen, T1)
        nf = (rb.windows.astype(np.int64) * valid).astype(np.int32)
        if not valid:
            return self.torch.zeros((len(rb), 0), dtype=self.torch.float32, device=self.device), nf, rb.lengths
        return gather_tracks(self.device, s1, T1, 0, valid, rb.win_first, nf), nf, rb.lengths

    def stream_detect(self, clips, chunk_frames=16, post=(3, 0.5, 10, 1000, 10, 3, 0), return_probs=False):
        """A list of 1-D int16 clips of any lengths, every clip one live stream (MarbleNetStreamBatch): all streams advance `chunk_frames`
        frames per tick until the longest is done, each with its own final tick; the collected tracks go through the whole-clip
        VadPostprocessor path of `detect(list)`.  -> per clip [(start_s, end_s)], equal to `detect(clips)` (dynamic-axis mode);
        return_probs adds (tracks f32 [B, max n_frames], decisions, n_frames), the tracks `detect`'s (bit for bit up to the frames that
        read `detect`'s tail-tile log-mel, see MarbleNetStreamBatch).  The host knows every stream's sample count, so `stream_counts` says
        how many frames each tick's rows hold: no tick waits for a read-back, and the device's n_out of all ticks is checked against the
        counts once, at the end."""
        t = self.torch
        clips = [np.ascontiguousarray(np.asarray(c).reshape(-1)) for c in clips]
        if len(clips) == 0:
            raise ValueError("stream_detect needs at least one clip")
        for c in clips:
            if c.dtype != np.int16:
                raise ValueError(f"clips must be int16, got {c.dtype}")
        k = int(chunk_frames)
        check_stream_step(k, [0], [False])
        S, row = len(clips), k * STREAM_HOP
        sb = MarbleNetStreamBatch(self, S)
        last = np.array([c.size // row for c in clips])              # the tick that is the stream's final one
        fed = np.zeros(S, dtype=np.int64)
        parts, counts, n_outs = [[] for _ in range(S)], [], []
        for i in range(int(last.max()) + 1):
            host = np.zeros((S, row), dtype=np.int16)
            n = np.zeros(S, dtype=np.int64)
            for s, c in enumerate(clips):
                if i <= last[s]:
                    piece = c[i * row:(i + 1) * row]
                    host[s, :piece.size], n[s] = piece, piece.size
            fin = last == i
            cnt = stream_counts(fed, n, fin)[2]
            fed = np.where(fin, 0, fed + n)
            _, s1, n_out = sb.step(host, n, final=fin)
            counts.append(cnt); n_outs.append(n_out)
            for s in np.flatnonzero(cnt).tolist():
                parts[s].append(s1[s, :cnt[s]])
        if not np.array_equal(t.stack(n_outs).cpu().numpy(), np.stack(counts)):
            raise _lib.VadxError("stream_detect: the device emitted other frame counts than stream_counts gives for the samples it was fed")
        empty = t.zeros((0,), dtype=t.float32, device=self.device)
        rows = [t.cat(p) if p else empty for p in parts]
        nf = np.array([int(r.shape[0]) for r in rows], dtype=np.int32)
        track = self._pad_rows(rows, t.float32)
        pp = _vadpost.VadPostprocessor(*post, frame_shift_s=OUTPUT_FRAME_SHIFT_S, frame_length_s=None, device=self.device)
        out, dec = track_segments(pp, track, nf, [c.size / SAMPLE_RATE for c in clips])
        return (out, track, dec, nf) if return_probs else out

    def _pad_rows(self, rows, dtype):
        """1-D device rows of different lengths -> one zero-filled matrix [B, max len]."""
        t = self.torch
        m = t.zeros((len(rows), max(max(int(r.shape[0]) for r in rows), 1)), dtype=dtype, device=self.device)
        for b, r in enumerate(rows):
            m[b, :r.shape[0]] = r.to(self.device)
        return m


# ---- live streams (include/vadx.h: vadx_marblenet_stream_tick)
STREAM_HOP = 320                  # samples per score frame
STREAM_LOOKAHEAD = 73             # score frames a stream stands behind the audio it has been fed (70 encoder frames + the prologue's 3)
STREAM_MAX_FRAMES = 256           # frames per tick the entry point takes (vadx_marblenet_stream_max_frames)
STREAM_RECORD_WORDS, STREAM_FED_WORD, STREAM_EMITTED_WORD = 11512, 11508, 11510      # per stream, in 4-byte words (the counters are int64)
_STAGE_BEHIND = (3, 15, 29, 45, 73)      # prologue, blocks 2 - 4, scores: frames behind J = samples fed / 320


def stream_counts(fed_before, n_samples, final):
    """What one tick produces for each stream, from its sample counts alone (numpy, no GPU): -> (mel, enc, score) int64 arrays, the
    log-mel frames, encoder frames (the prologue's output) and score frames that become final in this tick.  fed_before: samples fed
    since the stream's reset (a multiple of 320); n_samples: this tick's; final: the stream's last tick.  After N = 320 J samples and no
    final tick log-mel frames 0 .. 2J - 2 are complete (frame i reads samples up to 160 i + 255), the prologue has written frames
    < J - 3 (frame p reads log-mel frames up to 2p + 5) and max(0, J - 73) scores are out; a final tick at n samples in all completes
    n // 160 + 1 log-mel frames, n // 320 + 1 encoder frames and brings the scores to n // 320 (the last encoder frame is dropped, as
    the session's signal_len - 1 drops it)."""
    fed = np.asarray(fed_before, dtype=np.int64)
    n = np.asarray(n_samples, dtype=np.int64)
    fin = np.asarray(final, dtype=bool)
    fed, n, fin = np.broadcast_arrays(fed, n, fin)
    if np.any(fed < 0) or np.any(fed % STREAM_HOP):
        raise ValueError("fed_before must be a non-negative multiple of 320 (a stream is fed whole frames until its final tick)")
    if np.any(n < 0) or np.any((n % STREAM_HOP != 0) & ~fin):
        raise ValueError("n_samples must be a non-negative multiple of 320 on a stream that is not final")
    J0, J1, total = fed // STREAM_HOP, (fed + n) // STREAM_HOP, fed + n
    pos = lambda J, behind: np.maximum(J - behind, 0)           # noqa: E731
    mel0, enc0, sc0 = np.maximum(2 * J0 - 1, 0), pos(J0, _STAGE_BEHIND[0]), pos(J0, STREAM_LOOKAHEAD)
    mel1 = np.where(fin, total // 160 + 1, np.maximum(2 * J1 - 1, 0))
    enc1 = np.where(fin, total // STREAM_HOP + 1, pos(J1, _STAGE_BEHIND[0]))
    sc1 = np.where(fin, total // STREAM_HOP, pos(J1, STREAM_LOOKAHEAD))
    return mel1 - mel0, enc1 - enc0, sc1 - sc0


def check_stream_step(k, n_samples, final):
    """The per-tick arguments MarbleNetStreamBatch.step takes, checked on the host before anything is uploaded: k frames per row,
    n_samples int [S], final bool [S].  Raises ValueError naming the offending value."""
    k = int(k)
    if not 1 <= k <= STREAM_MAX_FRAMES:
        raise ValueError(f"k={k} frames per tick is outside [1, {STREAM_MAX_FRAMES}] (vadx_marblenet_stream_max_frames)")
    n = np.asarray(n_samples, dtype=np.int64).reshape(-1)
    fin = np.asarray(final, dtype=bool).reshape(-1)
    if n.shape != fin.shape:
        raise ValueError(f"n_samples {n.shape} and final {fin.shape} must have one entry per stream")
    if np.any(n < 0) or np.any(n > k * STREAM_HOP):
        bad = int(n[(n < 0) | (n > k * STREAM_HOP)][0])
        raise ValueError(f"n_samples={bad} is outside [0, k * 320 = {k * STREAM_HOP}]")
    odd = (n % STREAM_HOP != 0) & ~fin
    if np.any(odd):
        raise ValueError(f"n_samples={int(n[odd][0])} is not a multiple of 320 on a stream that is not final: a stream is fed whole "
                         "score frames until its final tick")


class MarbleNetStreamBatch(StreamBatch):
    """`streams` live Frame-VAD MarbleNet streams on the device (vadx_marblenet_stream_tick).  A stream is the audio of one virtual clip
    arriving in pieces; every `step` feeds each stream up to k frames (k * 320 samples) and returns the score frames that became final:
    a stream stands 73 frames (1.46 s) behind its audio, and its last tick (`final`) emits the remaining look-ahead against the zero
    padding behind the clip's last frame.  The concatenated scores are what `MarbleNetEngine.run(clip[None])` gives for the whole
    clip (n // 320 frames): bit for bit wherever a frame reads none of the log-mel frames `run` computes in its front-end's tail tile
    (the clip's last F mod 64 <= 48 frames, F = n // 160 + 1), one float32 ulp of the log-mel apart behind that.  Per stream only the left context of every launch boundary is carried, in the device
    `record` (DESIGN.md "Stream batches"; streams * 46 048 bytes, layout in include/vadx.h).  There is no `active` mask here -- a stream
    without audio has n_samples = 0 -- and a reset request applies at the very next tick, before that tick's audio, whether or not the
    stream gets any.  On "h2" every tick reads the range flag and, when it is raised, is recomputed on float32 from the same record; that
    counts once in engine.range_fallbacks."""

    def __init__(self, engine, streams):
        if int(getattr(engine, "in_sample_rate", SAMPLE_RATE)) != SAMPLE_RATE:
            raise ValueError(f"MarbleNetStreamBatch has no in-graph resampling: in_sample_rate is {engine.in_sample_rate}, not {SAMPLE_RATE}")
        if not getattr(engine, "fused", False):
            raise ValueError("MarbleNetStreamBatch is built for the published MarbleNet 3x2x64 layout (the fused kernels); this engine was "
                             "constructed with another `blocks` layout")
        if int(streams) < 1:                # (the wording of vadx_marblenet_stream_tick's own refusal)
            raise ValueError(f"streams={streams} must be at least 1")
        nb = _lib.lib().vadx_marblenet_stream_state_bytes(int(streams))
        if nb != int(streams) * STREAM_RECORD_WORDS * 4:
            raise _lib.VadxError(f"vadx_marblenet_stream_state_bytes = {nb}: not the record this binding was written for")
        super().__init__(engine, streams, nb)
        self._ws = {}               # k -> workspace (uint8)
        self._weights = {}             # mode -> vadx_marblenet_stream_weights
        self._fe = engine.frontend_ragged()
        if self._fe.fold not in self._fe.RAGGED_KINDS:
            raise ValueError(f"the stream front-end is built for the split-product kinds {self._fe.RAGGED_KINDS} (KIND_SPLIT_H2 / KIND_SPLIT_B3); "
                             f"this engine's Frontend was packed as kind {self._fe.fold} (VADX_FRONTEND_FOLD)")

    def stream_bytes(self, s, record=None):
        """Every byte of `record` (default: the current one) that belongs to stream s, as one uint8 tensor."""
        r = self.record if record is None else record
        return r[s * STREAM_RECORD_WORDS * 4:(s + 1) * STREAM_RECORD_WORDS * 4]

    def _counter(self, word):
        r = self.record.view(self.engine.torch.int32).view(self.streams, STREAM_RECORD_WORDS)
        return r[:, word:word + 2].contiguous().view(self.engine.torch.int64)[:, 0].cpu().numpy()

    @property
    def fed(self):
        """int64 [S] (host): samples each stream has been fed since its reset, read from the device record."""
        return self._counter(STREAM_FED_WORD)

    @property
    def emitted(self):
        """int64 [S] (host): score frames each stream has emitted since its reset, read from the device record."""
        return self._counter(STREAM_EMITTED_WORD)

    def _weights_for(self, mode):
        if mode not in self._weights:
            st, sfx = self.engine.stages, "_h" if mode == "h2" else ""
            p = lambda a: a.data_ptr()        # noqa: E731
            w = _lib.MarbleNetStreamWeights()
            w.p_dw, w.p_pw, w.p_pb = p(st[0]["dw"]), p(st[0]["pw" + sfx]), p(st[0]["pb"])
            for i, k in enumerate((1, 3, 5)):
                a, b = st[k], st[k + 1]
                w.b_dw0[i], w.b_pw0[i], w.b_b0[i] = p(a["dw"]), p(a["pw" + sfx]), p(a["pb"])
                w.b_dw1[i], w.b_pw1[i], w.b_b1[i] = p(b["dw"]), p(b["pw" + sfx]), p(b["pb"])
                w.b_rw[i], w.b_rb[i] = p(b["rw" + sfx]), p(b["rb"])
            w.t_dw, w.t_pw, w.t_pb = p(st[7]["dw"]), p(st[7]["pw" + sfx]), p(st[7]["pb"])
            w.t_w6, w.t_b6 = p(st[8]["pw" + sfx]), p(st[8]["pb"])
            w.dec_w, w.dec_b = p(self.engine.dec_w), p(self.engine.dec_b)
            self._weights[mode] = w
        return self._weights[mode]

    def _workspace(self, k):
        if k not in self._ws:
            t = self.engine.torch
            nb = _lib.lib().vadx_marblenet_stream_workspace_bytes(self.streams, k)
            if not nb:
                raise ValueError(f"k={k} frames per tick is outside [1, {STREAM_MAX_FRAMES}] (vadx_marblenet_stream_max_frames)")
            self._ws = {k: t.empty(nb, dtype=t.uint8, device=self.engine.device)}        # one tick size at a time: a stream keeps nothing in it
        return self._ws[k]

    def tick_raw(self, x, n_dev, reset_dev, final_dev, k, src, dst, s0, s1, n_out, mode):
        """One vadx_marblenet_stream_tick on device tensors, no host-side checks (the tests reach the device-side guards through it)."""
        eng, t = self.engine, self.engine.torch
        ws = self._workspace(k)
        mc = _lib.MarbleNetCfg(_lib.ARITH[mode], 0, eng._flag.data_ptr())
        with t.cuda.device(eng.device):
            _lib.check(_lib.lib().vadx_marblenet_stream_tick(
                C.byref(self._fe.cfg), self._fe.packed.data_ptr(), self._fe.mel_kb.ctypes.data, C.byref(self._weights_for(mode)),
                x.data_ptr(), int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1]), n_dev.data_ptr(),
                None if reset_dev is None else reset_dev.data_ptr(), None if final_dev is None else final_dev.data_ptr(), self.streams, k,
                src.data_ptr(), dst.data_ptr(), s0.data_ptr(), s1.data_ptr(), n_out.data_ptr(), ws.data_ptr(), int(ws.numel()),
                _lib.stream_ptr(), C.byref(mc)))

    def step(self, samples_i16, n_samples=None, reset=None, final=None):
        """samples_i16 int16 [S, k * 320] (host or device): each row holds that stream's next samples; n_samples int [S] (None: every
        stream gets the full row): 0 = no audio this tick, a positive multiple of 320 on a stream that goes on, anything in 0 .. k * 320
        on a `final` stream.  reset / final: bool [S] or None; reset applies before the audio, final emits the stream's remaining
        look-ahead and leaves it reset.  -> (score_silence, score_active f32 [S, k + 73], n_out int32 [S]) on the device: row s holds
        n_out[s] new score frames, NaN behind them.  A stream with no samples that is not final keeps its record bit for bit."""
        eng, t, S = self.engine, self.engine.torch, self.streams
        x = self._samples(samples_i16, f"[{S}, k * 320]", lambda x: x.shape[1] % STREAM_HOP or x.shape[1] == 0)
        k = x.shape[1] // STREAM_HOP
        fin = np.zeros(S, dtype=bool) if final is None else self._mask(final, "final")
        n = np.full(S, k * STREAM_HOP, dtype=np.int64) if n_samples is None else \
            np.asarray(n_samples.cpu() if hasattr(n_samples, "cpu") else n_samples, dtype=np.int64).reshape(-1)
        if n.shape != (S,):
            raise ValueError(f"n_samples must have shape ({S},), got {n.shape}")
        check_stream_step(k, n, fin)
        req = self._pending | self._mask(reset, "reset") if reset is not None else self._pending.copy()
        x = x.to(eng.device).contiguous()
        n_dev = t.from_numpy(n.astype(np.int32)).to(eng.device)
        reset_dev = t.from_numpy(req.astype(np.uint8)).to(eng.device) if req.any() else None
        final_dev = t.from_numpy(fin.astype(np.uint8)).to(eng.device) if fin.any() else None
        cap = k + STREAM_LOOKAHEAD                                    # the most stream_counts gives a tick of k frames: a final tick's whole look-ahead
        s0 = t.empty((S, cap), dtype=t.float32, device=eng.device)
        s1 = t.empty((S, cap), dtype=t.float32, device=eng.device)
        n_out = t.empty((S,), dtype=t.int32, device=eng.device)
        src, dst = self._rec[self._cur], self._rec[1 - self._cur]
        _lib.range_guarded(eng, eng.mode(), lambda m: self.tick_raw(x, n_dev, reset_dev, final_dev, k, src, dst, s0, s1, n_out, m),
                           lambda: _lib.take_flag(eng._flag), "f32")
        self._cur = 1 - self._cur
        self._pending[:] = False
        return s0, s1, n_out


class MarbleNetSession(Session):
    """{'audio': int16 [1,1,L]} -> [score_silence [1,T,1], score_active [1,T,1], signal_len int32 [1]]
    (Export_NVIDIA_MarbleNet_VAD.py:436-457; dynamic audio length).  io_dtype="float16": I/O-compatible with the reference's
    fp16-optimised model (Optimize_ONNX.py:37-44 converts with keep_io_types=False, so the two scores leave as float16) -- the
    arithmetic here stays float32 and the scores are rounded once on the way out."""

    def __init__(self, weights=None, device="cuda:0", in_sample_rate=16000, io_dtype="float32"):
        self.io_dtype, ftype = io_types(io_dtype)
        self.engine = MarbleNetEngine(weights, device, in_sample_rate=in_sample_rate)
        self._inputs_meta = [_Meta("audio", [1, 1, "audio_len"], "tensor(int16)")]
        self._outputs_meta = [_Meta("score_silence", [1, "signal_len", 1], ftype),
                              _Meta("score_active", [1, "signal_len", 1], ftype),
                              _Meta("signal_len", [1], "tensor(int32)")]

    def run(self, output_names, feeds):
        audio = np.asarray(feeds["audio"])
        require_int16(audio)
        s0, s1, slen = self.engine.run(audio.reshape(-1, audio.shape[-1]))
        res = {"score_silence": s0.cpu().numpy()[:, :, None].astype(self.io_dtype), "score_active": s1.cpu().numpy()[:, :, None].astype(self.io_dtype),
               "signal_len": np.array([slen], dtype=np.int32)}
        names = ["score_silence", "score_active", "signal_len"] if output_names is None else output_names
        return [res[n] for n in names]
