"""Fused signal front-end (int16 PCM -> log-mel) for every model family: host-side presets + the
thin wrapper over `vadx_frontend_logmel` (csrc/frontend.hip).  Reference rows a1-a5."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from . import tables

# name -> (n_fft, win_length, hop, window kind, STFT_Process variant, centre pad?, prep, (k0,k1),
#          mel builder, log mode, log floor)
PRESETS = {
    # FSMN/Export_FSMN_VAD.py:25-29,63,76-81,106
    "fsmn": dict(n_fft=512, win=400, hop=160, window="hamming", variant="v1", center=True, prep=0, k=(0.0, 1.0),
                 mel=("torchaudio", 20, 8000, None, "htk"), log_mode=0, log_floor=1e-5),
    # Export_NVIDIA_MarbleNet_VAD.py:30-34,186-204,245-262 (int16 scale folded into the 2-tap kernel)
    "marblenet": dict(n_fft=512, win=400, hop=160, window="hann_sym", variant="v2", center=True, prep=1,
                      k=(-0.97 * (1.0 / 32768.0), 1.0 / 32768.0), mel=("torchaudio", 0, 8000, "slaney", "slaney"),
                      log_mode=1, log_floor=1e-7),
    # FireRedVAD/Export_FireRedVAD.py:42-47,396-418,428-461 (snip_edges: no centre pad)
    "firered": dict(n_fft=400, win=400, hop=160, window="povey", variant="v2", center=False, prep=1, k=(-0.97, 1.0),
                    mel=("kaldi", 20.0, 0.0), log_mode=0, log_floor=1e-7),
}


def resampled_length(in_len, in_sample_rate):
    """(samples after the in-graph resample to 16 kHz, float32 source step) as torch derives them from
    scale_factor = 1 / (in_sample_rate / 16000): out = floor(in * scale_factor) in double, step = float32(1 / scale_factor);
    (in_len, None) at 16 kHz."""
    if int(in_sample_rate) == 16000:
        return int(in_len), None
    scale_factor = 1.0 / (in_sample_rate / 16000.0)
    return int(np.floor(float(in_len) * scale_factor)), np.float32(1.0 / scale_factor)


# The DFT product kinds = vadx_frontend_cfg.fold (include/vadx.h: VADX_FE_KIND_*)
KIND_DENSE, KIND_FOLD_SYM, KIND_FOLD_PER, KIND_FOLD_TF, KIND_SPLIT_B3, KIND_SPLIT_H2 = range(6)
ENV_KINDS = {"3": KIND_FOLD_TF, "4": KIND_SPLIT_B3, "5": KIND_SPLIT_H2}      # the kinds VADX_FRONTEND_FOLD asks for by number
ENV_DEFAULT = "5"


def host_tables(preset, window_len, n_mels=80, sample_rate=16000, in_sample_rate=16000):
    """Host side of one preset (a PRESETS name or a dict like its entries) and one window length: (preset dict with the resampling prep
    resolved, vadx_frontend_cfg with fold = 0, cos table, sin table [n_bins][n_fft], mel filterbank [n_mels][n_bins]) -- the reference's
    own float32 tables as numpy arrays.  Needs no GPU."""
    p = dict(PRESETS[preset]) if isinstance(preset, str) else dict(preset)
    n_fft, win, hop = p["n_fft"], p["win"], p["hop"]
    half = n_fft // 2
    out_len, rs_scale = resampled_length(int(window_len), int(in_sample_rate))
    if rs_scale is not None:
        if p["prep"] != 1:
            raise ValueError("in-graph resampling exists only in the two-tap (MarbleNet / FireRed) exports")
        p["prep"] = 6 if int(in_sample_rate) > 16000 else 7
    frames = (out_len // hop + 1) if p["center"] else ((out_len - n_fft) // hop + 1)
    if frames <= 0:
        raise ValueError(f"window of {int(window_len)} samples at {int(in_sample_rate)} Hz is shorter than one analysis frame")
    w = tables.analysis_window(p["window"], win, n_fft, p["variant"])
    cos_t, sin_t = tables.windowed_dft(n_fft, w, p["variant"])
    if p["mel"][0] == "torchaudio":
        _, fmin, fmax, norm, scale = p["mel"]
        fb = tables.mel_filters_torchaudio(half + 1, fmin, fmax, n_mels, sample_rate, norm, scale)
    elif p["mel"][0] == "zeros":          # raw-spectrum users (vadx_frontend_stft_ft) never touch the mel stage
        import torch
        fb = torch.zeros((n_mels, half + 1), dtype=torch.float32)
    else:
        fb = tables.mel_filters_kaldi(n_fft, n_mels, sample_rate, p["mel"][1], p["mel"][2])
    cfg = _lib.FrontendCfg()
    cfg.prep, cfg.k0, cfg.k1 = p["prep"], p["k"][0], p["k"][1]
    cfg.center_pad = half if p["center"] else 0
    cfg.tap0 = (n_fft - win) // 2 if win < n_fft else 0
    cfg.taps = min(win, n_fft)
    cfg.hop, cfg.n_bins, cfg.n_mels = hop, half + 1, n_mels
    cfg.log_mode, cfg.log_floor = p["log_mode"], p["log_floor"]
    cfg.frames, cfg.window_len = frames, out_len
    cfg.in_window_len, cfg.rs_scale = (int(window_len), float(rs_scale)) if rs_scale is not None else (0, 0.0)
    return p, cfg, tables.as_np(cos_t), tables.as_np(sin_t), tables.as_np(fb)


def select_kind(cfg, cos, sin, n_fft, fbank, fold=None, env=None):
    """Choose the DFT product for one table and pack its blob, once: -> (kind, packed float32 blob, mel_kb int32); cfg.fold = kind on return.
    Host library only (no GPU).  `fold` is Frontend's argument, `env` the value of VADX_FRONTEND_FOLD (None = unset = "5").  The ladder:
      fold False / 0          KIND_DENSE
      fold True               the mirror fold the table admits (`vadx_frontend_fold_kind`); ValueError if it admits none
      fold k > 0              kind k, or the packer's ValueError (a geometry the kind does not take, a table it does not admit)
      fold None               env "0", or an all-zero filterbank (the "zeros" mel of the raw-STFT users): KIND_DENSE;
                              env "3" / "4" / "5": that kind if the packer takes it, else the admitted mirror fold, else KIND_DENSE;
                              any other env: the admitted mirror fold, else KIND_DENSE."""
    L = _lib.lib()

    def admitted():
        return int(L.vadx_frontend_fold_kind(C.byref(cfg), cos.ctypes.data, sin.ctypes.data, n_fft))

    def pack(kind):
        cfg.fold = kind
        n = L.vadx_frontend_packed_floats(C.byref(cfg))
        if n == 0:
            raise ValueError("front-end geometry not supported by the HIP kernel (hop % 16, n_mels % 16, <= 4 passes)")
        packed, mel_kb = np.zeros(n, dtype=np.float32), np.zeros(2 * (cfg.n_mels // 16), dtype=np.int32)
        _lib.check(L.vadx_frontend_pack_host(C.byref(cfg), cos.ctypes.data, sin.ctypes.data, n_fft, fbank.ctypes.data,
                                             packed.ctypes.data, mel_kb.ctypes.data))
        return kind, packed, mel_kb

    if fold is None:
        env = ENV_DEFAULT if env is None else env
        if env == "0" or not fbank.any():
            return pack(KIND_DENSE)
        if env in ENV_KINDS:
            try:
                return pack(ENV_KINDS[env])
            except ValueError:      # asked for through the environment: where the kind does not apply, what the table admits
                pass
    elif not isinstance(fold, bool) and isinstance(fold, int) and fold > 0:
        return pack(int(fold))
    elif not fold:
        return pack(KIND_DENSE)
    kind = admitted()
    if fold is True and kind == KIND_DENSE:
        raise ValueError("this table / geometry has no folded DFT product")
    return pack(kind)


class Frontend:
    """Device-resident packed tables for one preset and one window length."""

    def __init__(self, preset, window_len, device="cuda:0", n_mels=80, sample_rate=16000, in_sample_rate=16000, fold=None):
        """fold: None = the fastest DFT product that holds the dense f32 product's error bound: KIND_SPLIT_H2 (the reference table times
        the prepped samples as fp16 x 2 split products, csrc/split2.h; the samples are bounded by the int16 input and pre-scaled exactly,
        so no range check is involved) where the geometry has it (hop 160, int16 preps), else the mirror-folded f32 product the table
        admits (KIND_FOLD_SYM / KIND_FOLD_PER, `vadx_frontend_fold_kind`), else KIND_DENSE.  VADX_FRONTEND_FOLD, read at every
        construction, overrides that: 0 = dense, 1 = the admitted mirror fold, 3 = opt into KIND_FOLD_TF (time x frequency fold: faster,
        noisier on weak bands), 4 = KIND_SPLIT_B3 (the dense product on bf16 x 3 exactly split operands), 5 = the default.  False = dense
        (the table-level parity tests compare against it), True = require a mirror fold, 1 ... 5 = that kind or a ValueError.  The
        precedence is `select_kind`'s; self.fold is the kind chosen.
        window_len = samples per window IN THE AUDIO BUFFER.  in_sample_rate != 16000 reproduces the exports built with
        IN_SAMPLE_RATE set (Export_NVIDIA_MarbleNet_VAD.py:237-254, FireRedVAD/Export_FireRedVAD.py:431-449): the graph itself
        resamples each window to 16 kHz with F.interpolate(linear, align_corners=False), before the pre-emphasis when the
        input rate is higher, after it when lower (two-tap presets only)."""
        torch = _lib.require_gpu()
        self.torch = torch
        self.device = torch.device(device)
        self.p, cfg, cos_n, sin_n, fb_n = host_tables(preset, window_len, n_mels, sample_rate, in_sample_rate)
        self.cfg, self.n_mels = cfg, n_mels
        self.in_window_len, self.in_sample_rate = int(window_len), int(in_sample_rate)
        self.window_len, self.frames = cfg.window_len, cfg.frames
        self.fold, packed, self.mel_kb = select_kind(cfg, cos_n, sin_n, self.p["n_fft"], fb_n, fold, os.environ.get("VADX_FRONTEND_FOLD"))
        self.packed = torch.from_numpy(packed).to(self.device)

    def logmel(self, audio_i16, windows_per_clip=1, win_stride=None, out=None):
        """audio int16 [B, N] (device) -> log-mel f32 [B*W, frames, n_mels] (device)."""
        t = self.torch
        if not t.is_tensor(audio_i16):
            audio_i16 = t.from_numpy(np.ascontiguousarray(audio_i16, dtype=np.int16))
        a = audio_i16.to(self.device)
        if a.dtype != t.int16:
            raise ValueError(f"audio must be int16, got {a.dtype}")
        if a.dim() == 3 and a.shape[1] == 1:
            a = a[:, 0]
        if a.dim() != 2:
            raise ValueError("audio must be [B, N] (or [B,1,N])")
        a = a.contiguous()
        B, N = a.shape
        W = int(windows_per_clip)
        ws = self.in_window_len if win_stride is None else int(win_stride)
        if (W - 1) * ws + self.in_window_len > N:
            raise ValueError("windows run past the clip: pad the clip to the window grid first")
        if out is None:
            out = t.empty((B * W, self.frames, self.n_mels), dtype=t.float32, device=self.device)
        means = t.empty((B * W,), dtype=t.float32, device=self.device) if self.cfg.prep not in (1, 6, 7) else None
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_frontend_logmel(C.byref(self.cfg), self.packed.data_ptr(), self.mel_kb.ctypes.data,
                                                       a.data_ptr(), _lib.row_stride(a), ws, B, W,
                                                       None if means is None else means.data_ptr(), out.data_ptr(),
                                                       _lib.stream_ptr()))
        return out

    RAGGED_KINDS = (KIND_SPLIT_H2, KIND_SPLIT_B3)

    def logmel_ragged(self, rf):
        """vadx.ragged.RaggedFrames (clips of any lengths, one window = one clip) -> log-mel f32 [sum F_b, n_mels] on the device, clip
        b's rows from rf.mel_first[b]: one launch (vadx_frontend_logmel_ragged).  Nothing in the packed tables depends on a window
        length, so ONE Frontend serves every length.  A host-only batch is uploaded first, in place.  Built for the split-product kinds
        and the centre-padded two-tap preset at 16 kHz; anything else is a ValueError -- never another product behind the caller's back."""
        t = self.torch
        if self.fold not in self.RAGGED_KINDS:
            raise ValueError(f"the ragged front-end is built for the split-product kinds {self.RAGGED_KINDS} (KIND_SPLIT_H2 / KIND_SPLIT_B3); this "
                             f"Frontend was packed as kind {self.fold} (fold argument or VADX_FRONTEND_FOLD): no ragged form of that product")
        if self.cfg.prep != 1 or self.cfg.center_pad <= 0 or self.cfg.hop != 160:
            raise ValueError(f"the ragged front-end is built for the centre-padded two-tap preset at 16 kHz (prep 1, hop 160); this Frontend has "
                             f"prep {self.cfg.prep}, centre pad {self.cfg.center_pad}, hop {self.cfg.hop}")
        if rf.device is None:
            rf.to(self.device)
        out = t.empty((rf.n_mel, self.n_mels), dtype=t.float32, device=self.device)
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_frontend_logmel_ragged(C.byref(self.cfg), self.packed.data_ptr(), self.mel_kb.ctypes.data,
                                                              rf.pcm.data_ptr(), int(rf.pcm.numel()), rf.clip_off.data_ptr(),
                                                              rf.clip_len.data_ptr(), rf.mel_first.data_ptr(), rf.fe_tile_first.data_ptr(),
                                                              rf.fe_tile_clip.data_ptr(), len(rf), rf.n_fe_tiles, rf.n_mel, out.data_ptr(),
                                                              _lib.stream_ptr()))
        return out

    def logmel_ragged_snip(self, pc, out=None):
        """vadx.ragged.PackedClips (clips of any lengths, one window = one clip, snip edges) -> log-mel f32 [sum F_b, n_mels] on the device,
        clip b's (n_b - n_fft) // hop + 1 rows from pc.frame_first[b] (none for a clip under n_fft samples): one launch
        (vadx_frontend_logmel_ragged_snip).  Built for the split-product kinds and the two-tap preset without centre pad at 16 kHz
        (FireRed); anything else is a ValueError.  A batch without a single frame gives an empty tensor and launches nothing."""
        t = self.torch
        if self.fold not in self.RAGGED_KINDS:
            raise ValueError(f"the ragged front-end is built for the split-product kinds {self.RAGGED_KINDS} (KIND_SPLIT_H2 / KIND_SPLIT_B3); this "
                             f"Frontend was packed as kind {self.fold} (fold argument or VADX_FRONTEND_FOLD): no ragged form of that product")
        if self.cfg.prep != 1 or self.cfg.center_pad != 0 or self.cfg.hop != 160:
            raise ValueError(f"the snip-edge ragged front-end is built for the two-tap preset without centre pad at 16 kHz (prep 1, hop 160); this "
                             f"Frontend has prep {self.cfg.prep}, centre pad {self.cfg.center_pad}, hop {self.cfg.hop}")
        if pc.device is None:
            pc.to(self.device)
        if out is None:
            out = t.empty((pc.n_frames, self.n_mels), dtype=t.float32, device=self.device)
        if pc.n_frames == 0:
            return out
        with t.cuda.device(self.device):
            _lib.check(_lib.lib().vadx_frontend_logmel_ragged_snip(C.byref(self.cfg), self.packed.data_ptr(), self.mel_kb.ctypes.data,
                                                                   pc.pcm.data_ptr(), int(pc.pcm.numel()), pc.clip_off.data_ptr(),
                                                                   pc.clip_len.data_ptr(), pc.frame_first.data_ptr(), pc.tile_first.data_ptr(),
                                                                   pc.tile_clip.data_ptr(), len(pc), pc.n_tiles, pc.n_frames, out.data_ptr(),
                                                                   _lib.stream_ptr()))
        return out
