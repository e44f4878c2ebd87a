"""TEST INFRASTRUCTURE -- a torch restatement of the MarbleNet STREAMING definition, on the CPU.

A stream is the audio of one virtual clip arriving in pieces.  `StreamRef` carries, per launch boundary, only the left context the
next stage reaches back to (audio: 417 samples; log-mel: 10 frames; prologue: 24; blocks 2 - 4: 28 / 32 / 56 encoder frames), works
in GLOBAL frame indices (frame 0 = the clip's first), masks every index < 0 -- and, on the `final` tick, every index >= the clip's
frame count -- to zero exactly where the layers' own zero padding would stand, and on `final` runs every stage out against zeros
behind the clip's last frame, stage by stage.  It is built from the oracle's own pieces (oracle.marblenet's front-end tables, unfolded
conv + BatchNorm weights, F.conv1d) and is pinned to `oracle.marblenet.forward` on whole clips by tests/test_marblenet_stream_cpu.py.
Nothing here is imported by the product."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import marblenet as omb
from oracle import mel as omel
from oracle import stft as ostft

HOP = 320
CARRY = 417
BEHIND = (3, 15, 29, 45, 73)          # prologue, blocks 2 - 4, scores: frames behind J = samples fed / 320
HIST = (10, 24, 28, 32, 56)           # history in front of the prologue, blocks 2 - 4, the tail
CH = (80, 128, 64, 64, 64)


def _masked(x, g0, end):
    """x [C, W] whose column 0 is global frame g0: columns outside [0, end) zeroed (end None = no upper end)"""
    idx = torch.arange(x.shape[1]) + g0
    keep = idx >= 0 if end is None else (idx >= 0) & (idx < end)
    return x * keep.to(x.dtype)[None, :]


class StreamRef:
    def __init__(self, w, dtype=torch.float32, mel=None):
        """mel: None = the streaming front-end below; or the whole clip's log-mel [80, F] (oracle.marblenet.log_mel), from which a
        tick takes the frames its audio completes -- the encoder's streaming form on its own, free of the front-end's float32
        rounding (torch's conv1d and matmul round differently at different lengths)."""
        self.dtype, self.mel = dtype, mel
        self.w = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items()}
        fe = omb.Frontend()
        self.cos_k, self.sin_k, self.fbank = fe.cos_k, fe.sin_k, fe.fbank         # the front-end stays float32, as on the device
        self.reset()

    def reset(self):
        self.fed = 0
        self.emitted = 0
        self.pcm = torch.zeros(CARRY, dtype=torch.int16)
        self.hist = [torch.zeros(CH[i], HIST[i], dtype=self.dtype) for i in range(5)]

    # ---- stages: input [C, W] with column 0 = global frame g0, already masked; returns the frames [o0, o1)
    def _sub(self, x, p, k, dil=1, stride=1):
        w = self.w
        x = F.conv1d(x[None], w[p + "_dw"].unsqueeze(1), stride=stride, dilation=dil, groups=x.shape[0])
        x = F.conv1d(x, w[p + "_pw"].unsqueeze(-1))
        return omb._bn(x, w, p)[0]

    def _prologue(self, mel, g0, o0, o1):
        x = mel[:, 2 * o0 - 5 - g0:2 * (o1 - 1) + 5 - g0 + 1]
        return F.relu(self._sub(x, "b0r0", 11, 1, 2))

    def _block(self, bi, k, x, g0, o0, o1, end):
        pad = (k - 1) // 2
        xin = x[:, o0 - 2 * pad - g0:o1 + 2 * pad - g0]                     # frames o0 - 2 pad .. o1 + 2 pad
        h = F.relu(self._sub(xin, f"b{bi}r0", k))                           # frames o0 - pad .. o1 + pad
        h = _masked(h, o0 - pad, end)                                       # the zero padding sub-block 1 sees
        y = self._sub(h, f"b{bi}r1", k)                                     # frames o0 .. o1
        res = omb._bn(F.conv1d(x[None, :, o0 - g0:o1 - g0], self.w[f"b{bi}res_pw"].unsqueeze(-1)), self.w, f"b{bi}res")[0]
        return F.relu(y + res)

    def _tail(self, x, g0, o0, o1):
        xin = x[:, o0 - 28 - g0:o1 + 28 - g0]
        y = F.relu(self._sub(xin, "b4r0", 29, 2))
        y = F.relu(omb._bn(F.conv1d(y[None], self.w["b5r0_pw"].unsqueeze(-1)), self.w, "b5r0")[0])
        logits = F.linear(y.t(), self.w["dec_w"], self.w["dec_b"])
        return logits

    def feed(self, samples_i16, final=False):
        """One tick: int16 samples (a multiple of 320 unless final) -> logits [n_out, 2] of the score frames that became final."""
        x = torch.as_tensor(np.asarray(samples_i16, dtype=np.int16)).reshape(-1)
        n = int(x.shape[0])
        assert final or (n > 0 and n % HOP == 0)
        J, kf = self.fed // HOP, n // HOP
        T1 = J + kf + 1 if final else None                                  # the virtual clip's encoder frames, known on the final tick
        Fm = 2 * J + n // 160 + 1 if final else None                        # ... and its log-mel frames
        # ---- front-end on `carry || new`, no centre padding: frame i starts at row sample 1 + 160 i, sample 0 is the pre-emphasis tap
        mel_o0, mel_o1 = 2 * J - 1, (Fm if final else 2 * (J + kf) - 1)
        self.last_mel_range = (mel_o0, mel_o1)
        row = torch.cat([self.pcm, x]).float()
        pre = (row[1:] * (1.0 / 32768.0) + row[:-1] * (-0.97 * (1.0 / 32768.0)))          # sample r of `pre` = row sample r + 1
        need = 160 * (mel_o1 - mel_o0 - 1) + 512
        pre = F.pad(pre, (0, max(0, need - pre.shape[0])))[:need]           # zeros behind the clip's last sample (final only)
        re, im = ostft.stft(pre[None, None], self.cos_k, self.sin_k, 160, False)
        new_mel = omel.log_mel(re, im, self.fbank, 1e-7, "add")[0].to(self.dtype)         # [80, mel_o1 - mel_o0]
        self.last_mel = new_mel
        if self.mel is not None:
            assert final or mel_o1 <= self.mel.shape[1]
            new_mel = F.pad(self.mel[:, max(mel_o0, 0):mel_o1].to(self.dtype), (max(0, -mel_o0), 0))
        bufs, g0s = [], []
        buf, g0 = torch.cat([self.hist[0], new_mel], dim=1), mel_o0 - HIST[0]
        ends = [Fm, T1, T1, T1, T1]
        tailpad = (lambda b: F.pad(b, (0, 64))) if final else (lambda b: b)      # zeros behind the clip's last frame: every layer pads ITS input
        bufs.append(tailpad(_masked(buf, g0, ends[0]))); g0s.append(g0)
        # ---- prologue, blocks 2 - 4
        for i in range(4):
            o0, o1 = J - BEHIND[i], (T1 if final else J + kf - BEHIND[i])
            src, sg0 = bufs[i], g0s[i]
            if i == 0:
                new = self._prologue(src, sg0, o0, o1)
            else:
                new = self._block(i, (13, 15, 17)[i - 1], src, sg0, o0, o1, ends[i])
            buf, g0 = torch.cat([self.hist[i + 1], new], dim=1), o0 - HIST[i + 1]
            bufs.append(tailpad(_masked(buf, g0, ends[i + 1]))); g0s.append(g0)
        o0, o1 = J - BEHIND[4], (T1 - 1 if final else J + kf - BEHIND[4])               # (final: the last encoder frame is dropped)
        logits = self._tail(bufs[4], g0s[4], o0, o1)[max(0, -o0):max(0, o1 - o0)]
        # ---- what the next tick needs
        if final:
            self.reset()
        else:
            self.pcm = torch.cat([self.pcm, x])[-CARRY:]
            self.hist = [b[:, -HIST[i]:].clone() for i, b in enumerate(bufs)]
            self.fed += n
            self.emitted += logits.shape[0]
        return logits


def stream_clip(w, clip_i16, k, dtype=torch.float32, mel=None):
    """The whole clip through one StreamRef at k frames per tick, its own final tick last -> (logits [n // 320, 2], frames per tick)"""
    ref = StreamRef(w, dtype, mel)
    a = np.asarray(clip_i16, dtype=np.int16).reshape(-1)
    row, out, per_tick = k * HOP, [], []
    with torch.no_grad():
        at = 0
        while a.size - at >= row:
            out.append(ref.feed(a[at:at + row]))
            per_tick.append(out[-1].shape[0])
            at += row
        out.append(ref.feed(a[at:], final=True))
        per_tick.append(out[-1].shape[0])
    return torch.cat(out, dim=0), per_tick
