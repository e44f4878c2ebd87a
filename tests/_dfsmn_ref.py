"""The ICCRN's stages restated at the seams the device cuts them at, in plain torch; the dtype follows the input (float64 tensors with the
float32 weights and float32 table bits cast to double give the yardstick of tests/test_gpu_dfsmn_kernels.py, float32 ones the float32
graph whose error against it is the scale of the bound).  Everything the oracle already states is the oracle's: layer_norm, ch_lstm_f,
ch_lstm_t, ceps_unit, cfb, CepsTables come from oracle.dfsmn.  Only what csrc/dfsmn_cfb.hip cuts differently is restated here:

  cfb_front   x -> gx, r = xi - gx as oracle.dfsmn.cfb; y1 = conv31(LN1.w * gx) with NO bias and NO normalisation; S = cat(re, im) of the
              length-160 DFT of LN2(r); the statistics rows (mean, 1 / (std + 1e-6)) per frame of gx and of S
  lstm_f_hidden   LayerNorm of S from GIVEN statistics rows, then the bi-LSTM along F without its Linear (the device's `hf`)
  cfb_back    hf, S, y1, statistics of gx -> Linear 40 -> 40, complex product with S, pinv inverse,
              out = inv1 * (y1 - mean1 * CW) + CB + ceps with CW = conv31(LN1.w), CB = conv31(LN1.b) + bias

tests/test_dfsmn_ref_cpu.py pins front -> ch_lstm_f -> back to oracle.dfsmn.cfb in float64 with no device.

Tensors are the oracle's [1, C, F, T]; statistics are [T, 2]."""
import torch
import torch.nn.functional as F

from oracle import dfsmn as od

CH = 20


def frame_stats(x):
    """[1, C, F, T] -> [T, 2] = (mean, 1 / (unbiased std + 1e-6)) over (C, F) per frame: the two numbers oracle.dfsmn.layer_norm uses"""
    return torch.stack([x.mean([1, 2])[0], 1.0 / (x.std([1, 2])[0] + 1e-6)], dim=1)


def layer_norm_from(x, stats, w, p):
    """oracle.dfsmn.layer_norm with the frame's (mean, 1 / (std + eps)) GIVEN as [T, 2] rows"""
    return (x - stats[:, 0]) * stats[:, 1] * w[p + ".w"] + w[p + ".b"]


def conv31(x, w, p, bias=False):
    return F.conv2d(x, w[p + ".conv.weight"], w[p + ".conv.bias"] if bias else None, padding=(1, 0))


def dft_f(x, tb, ch=CH):
    """CepsUnit's forward transform, oracle.dfsmn.ceps_unit's first three lines: [1, ch, 160, T] -> cat(re, im) [1, 2 ch, 81, T]"""
    xr = x.permute(0, 1, 3, 2).contiguous().view(-1, 1, od.CEPS_N)
    re = F.conv1d(xr, tb.cos_k, stride=od.CEPS_N).view(1, ch, -1, od.CEPS_F).permute(0, 1, 3, 2).contiguous()
    im = F.conv1d(xr, tb.sin_k, stride=od.CEPS_N).view(1, ch, -1, od.CEPS_F).permute(0, 1, 3, 2).contiguous()
    return torch.cat([re, im], 1)


def cfb_front(x, w, p, tb):
    """The first half of oracle.dfsmn.cfb up to the frequency-axis LSTM's input, x [1, cin, 160, T] -> dict(gx, r, y1, S, stats1, stats_li)"""
    g = torch.sigmoid(F.conv2d(od.layer_norm(x, w, p + ".LN0"), w[p + ".conv_gate.weight"], w[p + ".conv_gate.bias"]))
    xi = F.conv2d(x, w[p + ".conv_input.weight"], w[p + ".conv_input.bias"])
    gx = g * xi
    r = xi - gx
    S = dft_f(od.layer_norm(r, w, p + ".LN2"), tb)
    return dict(gx=gx, r=r, y1=conv31(w[p + ".LN1.w"] * gx, w, p), S=S, stats1=frame_stats(gx), stats_li=frame_stats(S))


def lstm_f_hidden(S, stats_li, w, p, ch=CH):
    """hf [1, 2 ch, 81, T] (forward | reverse hidden states) = CepsUnit's bi-LSTM along F, without its Linear, on LayerNorm(S) taken
    from the given statistics rows"""
    x = layer_norm_from(S, stats_li, w, p + ".LN")
    y = x.permute(0, 3, 2, 1).contiguous().view(-1, od.CEPS_F, 2 * ch)
    y = od._lstm(y, w, p + ".ch_lstm_f.lstm2.", 2 * ch, ch, 1, True)
    return y.view(1, -1, od.CEPS_F, 2 * ch).permute(0, 3, 2, 1).contiguous()


def lstm_f_linear(hf, w, p, ch=CH):
    """The Linear 40 -> 40 behind that LSTM: hf -> lo, both [1, 2 ch, 81, T]"""
    y = F.linear(hf.permute(0, 3, 2, 1), w[p + ".ch_lstm_f.linear.weight"], w[p + ".ch_lstm_f.linear.bias"])
    return y.permute(0, 3, 2, 1).contiguous()


def cfb_back(S, y1, stats1, w, p, tb, hf=None, lo=None, ch=CH):
    """The second half: the LSTM's hidden states `hf` (or `lo`, what oracle.dfsmn.ch_lstm_f returns: its Linear applied), the spectrum
    S, the un-normalised y1 and the statistics rows of gx -> the block's output [1, ch, 160, T]"""
    if lo is None:
        lo = lstm_f_linear(hf, w, p + ".ceps_unit", ch)
    re, im = S[:, :ch], S[:, ch:]
    pr, pi = lo[:, :ch], lo[:, ch:]
    a = (pr * re - pi * im).permute(0, 1, 3, 2).contiguous().view(-1, od.CEPS_F, 1)
    b = (pr * im + pi * re).permute(0, 1, 3, 2).contiguous().view(-1, od.CEPS_F, 1)
    inv = F.conv_transpose1d(torch.cat((a, b), dim=1), tb.inv_basis, stride=od.CEPS_N)
    ceps = inv.view(1, ch, -1, od.CEPS_N).permute(0, 1, 3, 2).contiguous()
    cw = conv31(w[p + ".LN1.w"], w, p)                       # [1, ch, 160, 1]
    cb = conv31(w[p + ".LN1.b"], w, p, bias=True)
    return stats1[:, 1] * (y1 - stats1[:, 0] * cw) + cb + ceps


def rel_errors(y, y64):
    """The two figures of a tensor [chunks, C, F, T] against its float64 reference, both in double:
      all    max |y - y64| / max |y64| over the tensor
      frame  the largest, over the frames whose reference is not identically zero, of that frame's max |y - y64| / max |y64|
    -> (all, frame, max |y64|, the largest |y| among frames whose reference IS identically zero: the caller asserts it is 0)"""
    d = (y.double() - y64).abs().amax(dim=(1, 2))            # [chunks, T]
    s = y64.abs().amax(dim=(1, 2))
    live = s > 0
    dead = float(y.abs().amax(dim=(1, 2))[~live].max()) if bool((~live).any()) else 0.0
    scale = float(s.max())
    return float(d.max()) / scale, float((d[live] / s[live]).max()), scale, dead
