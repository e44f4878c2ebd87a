"""GPU parity: the ICCRN of the DFSMN path kernel by kernel against float64, each stage on its own input, at every frame-tile and chunk edge.

tests/test_gpu_dfsmn_shapes.py holds the final spectrum of the whole ICCRN; between a kernel and that figure lie ten gated blocks, thirteen
LayerNorms and two gated time LSTMs.  Here every launch of `Iccrn.forward` is held on its own, through the product's launch code (`Iccrn.lstm_f`,
`.pw`, `.cfb`, `.lstm_t`, `.stats`, `.merged_stats`), on an input that is read back and handed to the reference:

  stage       device                                                          reference (float64)                                paths
  in lstm     lstm_f_kernel<4> -> pw_conv 40 -> 20                            oracle ch_lstm_f(x, "in_ch_lstm")                  f32; split, h2 bit-identical
  in conv     pw_conv 24 -> 20 over two views, emitting partial statistics    conv2d(cat(the device's e0l, x))                   f32; split, h2 bit-identical
  front       cfb_front: y1, li, stats1, stats_li                             _dfsmn_ref.cfb_front of the block input            f32, split (h2 = split, bit-identical)
  lstm_f      lstm_f_kernel<40> / lstm_f_split_kernel<B3 / H2>: hf            _dfsmn_ref.lstm_f_hidden of the device's li, stats_li   f32, split, h2
  back        cfb_back (f32 MFMAs; the split form under cfb_back_split)       _dfsmn_ref.cfb_back of the device's hf, li, y1, stats1  f32, split
  block       the three launches together                                     oracle cfb of the block input                      f32, split, h2
  lstm_t 0    frame_stats + lstm_t2_kernel / lstm_t2h_kernel, mul = e5        e5 * ch_lstm_t(layer_norm(e5, "ln"), "ch_lstm")    f32, h2 (range flag (0, 0.0))
  lstm_t 1    lstm_t_kernel                                                   ch_lstm_t(x, "out_ch_lstm")                        f32; split, h2 bit-identical
  out         pw_conv 60 -> 2, b = channels [20, 40) of a 40-channel tensor   conv2d(cat(d0, d1))                                f32
  stats       stats1, stats_li, the partials pw_conv and cfb_back emit merged (stats_merge), frame_stats   float64 (mean, 1 / (std + 1e-6)) of
              the tensor they describe, valid frames: rtol 1e-5 (mean) / 1e-4 (1 / std), atol 1e-6, the tolerances of
              test_fused_layernorm_statistics_match_the_separate_pass

Blocks: cfb_e1 (20 in, statistics from the partials of its producer), cfb_d5 (20 in, statistics from a frame_stats pass), cfb_d3 (the two
halves of one 40-channel tensor with the partials of both, written into channels [20, 40) of a 40-channel tensor whose other half must stay
as it was).  A block input with partial statistics is produced by the product's pw_conv with an identity weight (a copy, asserted exact).

Shapes: T in {1, 3, 4, 5, 15, 16, 17, 33, 101} x chunks in {1, 2, 3} (quad edges of the loader wave, one step, a full tile, one frame
past it, two tiles + 1; 10 / 20 / 30 bin groups of time LSTM 0 at four per workgroup).  At T in {5, 17, 33, 101} every case also runs on the
packed layout (frame_stride = packed_stride(T), inputs moved by vadx_dfsmn_ft_repack: with 2 / 3 chunks a chunk starts mid-tile): valid
frames bit-identical to the tile-aligned run.  One persistent-loop case each: cfb_e1 at 300 chunks x T = 16 (chunks 0, 1, 255, 256, 299
compared), pw_conv 24 -> 20 at 4096 tiles (the one-workgroup-per-tile grid; tiles 0, 1, 4095).

Inputs: x = level[t % 3] (N(0, 1) + 25 [chunk 0]), level = (1, 0.1, 0.01), torch.randn seeded per (stage, T, chunks): every quad and tile
holds all three levels, chunk 0 carries an offset of 25 standard deviations in every frame (LayerNorm 0 cancels it; the float32 yardstick
grows with it), the last chunk of a multi-chunk case is all zeros.

Beside the float64 comparison, bitwise: a chunk in a batch = the same chunk alone; padding frames (and their statistics rows) filled with
seeded values of the data's scale instead of zeros leave every valid frame as it was, on every path.

Figures, per tensor, in double: all = max |y - y64| / max |y64|; frame = the largest over valid frames of that frame's max |y - y64| / max
|y64| (every kernel but the time LSTMs computes a frame from that frame alone: an error in a quiet frame beside loud ones shows).  A frame
whose reference is identically zero (e5 * ... of a zero chunk) must be identically zero on the device.  Bound: the scheme of
tests/test_gpu_dfsmn_shapes.py, its code reused: e_dev <= 2 max(e_dev(pinned), R e_32(case)), R = e_dev / e_32 at the stage's pinned shape
(T = 101, 3 chunks) per path and figure, e_32 the float32 torch restatement's error on the same input; and 2e-4 x max(1, scale) unconditionally.

li's im(bin 0) and im(bin 80) are structural zeros on the device (include/vadx.h).  The reference's float32 sine row of bin 80 is
-sin(fl(pi t)), up to 5.2e-5 instead of zero, so the reference's im(80) is a rounding artefact of its table (up to 7.8e-4 here, 1.9e-5 of a quiet
frame's maximum): with it in, li's `frame` read 1.9e-5 against a float32 oracle of 1.3e-6 (R 15) and hid everything below; it is asserted zero
on the device, held to the absolute tolerance in the reference, and left out of li's figures (R 0.7 .. 1.4).

Measured on one MI355X (profiles/dfsmn_kernels_errors.txt has every case and both figures), pinned shapes, figure `frame`: e_dev, e_32, R
  front y1   e1 f32 2.85e-06 1.99e-06 1.431  split 2.92e-06 1.99e-06 1.465 | d5 1.96e-06 1.41e-06 1.390  1.62e-06 1.41e-06 1.153 | d3 2.46e-06 1.28e-06 1.922  2.35e-06 1.28e-06 1.832
  front li   e1 f32 9.01e-07 1.28e-06 0.701  split 1.26e-06 1.28e-06 0.984 | d5 1.46e-06 2.57e-06 0.568  2.23e-06 2.57e-06 0.866 | d3 1.24e-06 1.71e-06 0.729  2.37e-06 1.71e-06 1.388
  lstm_f hf  e1 f32 1.09e-06 9.68e-07 1.123  split 1.03e-06 7.30e-07 1.406  h2 5.92e-07 7.30e-07 0.811 | d5 7.88e-07 8.29e-07 0.950  8.23e-07 9.46e-07 0.869  1.59e-06 9.46e-07 1.680
             d3 f32 9.68e-07 9.98e-07 0.971  split 1.24e-06 9.51e-07 1.304  h2 1.46e-06 9.51e-07 1.532
  back out   e1 f32 1.78e-06 5.49e-07 3.237  split 1.78e-06 4.94e-07 3.610 | d5 2.50e-06 5.02e-07 4.978  2.29e-06 5.67e-07 4.048 | d3 1.98e-06 4.62e-07 4.289  1.96e-06 5.17e-07 3.799
  block out  e1 f32 2.80e-06 2.03e-06 1.380  split 2.54e-06 2.03e-06 1.255  h2 2.53e-06 2.03e-06 1.247 | d5 2.72e-06 2.18e-06 1.246  2.54e-06 2.18e-06 1.166  2.52e-06 2.18e-06 1.154
             d3 f32 3.05e-06 1.27e-06 2.412  split 2.55e-06 1.27e-06 2.015  h2 2.52e-06 1.27e-06 1.988
  in lstm 1.07e-06 5.88e-07 1.814   in conv 2.91e-07 3.71e-07 0.784   out 7.21e-07 6.70e-07 1.076   pw 24 -> 20 3.23e-07 4.37e-07 0.738
  lstm_t 0   f32 2.01e-06 3.84e-06 0.523  h2 1.90e-06 3.84e-06 0.494        lstm_t 1  1.18e-06 1.38e-06 0.859
(back's R of 3 .. 5: the float32 restatement of the back half alone, fed float32 tensors, errs 5e-7 of a frame; the device's 2e-6 is the
block's own float32 grade, see `block`.)  Largest e / bound per stage, either figure: front 0.729 (cfb_d3, T = 17, 2 chunks, f32), lstm_f 0.723
(cfb_d3, T = 16, 3 chunks, split), back 0.900 (cfb_e1, T = 3, 1 chunk, split), block 0.881 (cfb_e1, T = 4, 2 chunks, h2), in lstm 0.508, in conv
0.590, out 0.561, pw 24 -> 20 at 4096 tiles 0.473, lstm_t 0 0.500 (the pinned shape itself), lstm_t 1 0.672 (T = 33, 3 chunks).  Statistics rows, 599
comparisons: largest |mean - mean64| 5.8e-6 (stats1 of cfb_d5, mean 25 standard deviations), largest relative error of 1 / (std + 1e-6) 2.0e-6.
The sweep found no wrong number: every case of every path passed on the library as it was; the zeroed im(80) above is its one finding.

That it notices a wrong number was checked once, on four scratch copies of the library with one one-line change each (values or indices inside
a tile, every address inside the same buffers; not committed).  Every case of a stage measures the stage's pinned shape first, so where
the pinned shape misses its absolute tolerance every case of that stage fails.  New tests that failed / test_iccrn_frame_count_sweep:
  the (3,1) conv loses its taps at bin 159 (it runs in cfb_front here: the ring slot of bin 159 written as zero, both arithmetics)
      test_cfb_front 162 of 162, test_cfb_block 243 of 243, the persistent case's front and block rows (6 of 12); lstm_f, back (fed the
      device's own y1) and every other stage passed / 72 of 72 failed
  cfb_front's DFT correction uses the previous frame's mean
      test_cfb_front 162 of 162, test_cfb_block 243 of 243, persistent 6 of 12, test_cfb_bitwise_properties 72 of 243 (every packed case
      with 2 or 3 chunks: a chunk's first frame then takes its mean from the frame before it in the tile) / 72 of 72 failed
  time LSTM 0 multiplies with `mul` one frame late at a quad's first frame (f32: frame t - 1; fp16 x 2, whose quad sits in registers: t + 1)
      test_time_lstm_0 54 of 54, nothing else / 72 of 72 failed
  pw_conv reads view b from channel offset 0 instead of c_off
      test_output_stage 27 of 27, test_pw_conv_one_workgroup_per_tile_grid (b = channels [20, 24)), nothing else (in conv's b starts at
      channel 0) / 72 of 72 failed
So the end-to-end sweep does notice all four at this size of defect (each moves the spectrum by far more than 2e-6); what this file adds is the
name of the kernel, and the stages the end-to-end figure dilutes: a defect confined to one tensor's quiet frames, to one block, or to the
statistics rows.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, dfsmn
from oracle import dfsmn as od

import _dfsmn_ref as ref
import test_gpu_dfsmn_shapes as sh          # the bound's code (pinned, assert_float32_grade), the engine, weights and tables, shared

pytestmark = pytest.mark.gpu
SEED = 1234
PIN = (101, 3)
PATHS = ["f32", "split", "h2"]
FRAMES = [1, 3, 4, 5, 15, 16, 17, 33, 101]
CHUNKS = [1, 2, 3]
PACKED_FRAMES = [5, 17, 33, 101]
BLOCKS = {"cfb_e1": 20, "cfb_d5": 20, "cfb_d3": 40}
STAGE_IDS = ["in", "cfb_e1", "cfb_d5", "cfb_d3", "lstm_t0", "lstm_t1", "out", "pw4096"]
F64, F32 = torch.float64, torch.float32


def net():
    n = sh.engine().iccrn
    if "test.copy.weight" not in n.d:              # pw_conv 24 -> 20 as a copy of its first view: how a block input gets partial statistics
        n.d["test.copy.weight"] = torch.eye(32, 24, dtype=F32, device=n.device)
        n.d["test.copy.bias"] = torch.zeros(32, dtype=F32, device=n.device)
    return n


def W(dtype):
    return sh.iccrn_weights(dtype)


def ceps(dtype):
    return sh.tables(dtype).tb.ceps


@contextlib.contextmanager
def layout(stride, back_split=False):
    n = net()
    prev = n.frame_stride, n.cfb_back_split
    n.frame_stride, n.cfb_back_split = stride, back_split
    try:
        yield n
    finally:
        n.frame_stride, n.cfb_back_split = prev


# ---- FT tensors with any frame stride, from and to [chunks, C, F, T] --------------------------------------------------------------------
def columns(chunk_ids, frames, stride):
    return (torch.as_tensor(list(chunk_ids)).view(-1, 1) * stride + torch.arange(frames).view(1, -1))


def valid_columns(total, chunks, frames, stride):
    m = torch.zeros(total, dtype=torch.bool)
    m[columns(range(chunks), frames, stride).reshape(-1)] = True
    return m


def ft_read(data, stride, frames, chunk_ids):
    """FT data [tiles, C, F, 16] -> the valid frames of the chunks `chunk_ids` as a host tensor [n, C, F, frames]"""
    idx = columns(chunk_ids, frames, stride).reshape(-1).to(data.device)
    v = data[idx // 16, :, :, idx % 16]                                         # [n * frames, C, F]
    return v.view(len(chunk_ids), frames, data.shape[1], data.shape[2]).permute(0, 2, 3, 1).contiguous().cpu()


def stats_read(s, stride, frames, chunk_ids):
    idx = columns(chunk_ids, frames, stride).reshape(-1).to(s.device)
    return s.view(-1, 2)[idx].view(len(chunk_ids), frames, 2).cpu()


def fill_padding(ft, chunks, seed):
    """Every column of `ft` that is no valid frame <- seeded N(0, 1) clipped to 3: finite, and no larger than the data"""
    bad = ~valid_columns(ft.tiles * 16, chunks, ft.frames, ft.stride)
    if not bool(bad.any()):
        return
    g = torch.Generator().manual_seed(seed)
    cols = ft.data.permute(1, 2, 0, 3).reshape(ft.C, ft.F, -1).clone()
    cols[:, :, bad.to(cols.device)] = torch.randn(ft.C, ft.F, int(bad.sum()), generator=g).clamp_(-3.0, 3.0).to(cols.device)
    ft.data.copy_(cols.view(ft.C, ft.F, ft.tiles, 16).permute(2, 0, 1, 3))


def fill_stats_padding(s, chunks, frames, stride, seed):
    bad = ~valid_columns(s.shape[0] * 16, chunks, frames, stride)
    if bool(bad.any()):
        g = torch.Generator().manual_seed(seed)
        rows = torch.stack([torch.randn(int(bad.sum()), generator=g), 0.5 + torch.rand(int(bad.sum()), generator=g)], dim=1)
        s.view(-1, 2)[bad.to(s.device)] = rows.to(s.device)


def make_ft(x, stride=None, fill=None):
    """Host [chunks, C, F, T] -> FT on the device, tile-aligned or (stride) moved to the packed layout by vadx_dfsmn_ft_repack; fill: a
    seed for its padding frames"""
    n, c, f, frames = x.shape
    dev = net().device
    ft = dfsmn.to_ft(torch, x, dev)
    if stride is not None and stride != ft.stride:
        p = dfsmn.FT(torch, dev, n, frames, c, f, stride=stride)
        _lib.check(_lib.lib().vadx_dfsmn_ft_repack(ft.data.data_ptr(), p.data.data_ptr(), c, f, frames, n, ft.stride, stride, _lib.stream_ptr()))
        ft = p
    if fill is not None:
        fill_padding(ft, n, fill)
    return ft


def empty_ft(chunks, frames, channels, stride, bins=od.F_BINS):
    return dfsmn.FT(torch, net().device, chunks, frames, channels, bins, stride=stride)


@functools.lru_cache(maxsize=4)
def stage_input(stage, channels, frames, chunks):
    g = torch.Generator().manual_seed(SEED + 100000 * STAGE_IDS.index(stage) + 1000 * chunks + frames)
    x = torch.randn(chunks, channels, od.F_BINS, frames, generator=g)
    x[0] += 25.0
    x *= torch.tensor([1.0, 0.1, 0.01])[torch.arange(frames) % 3]
    if chunks > 1:
        x[-1] = 0.0
    return x


def per_chunk(fn, *tensors):
    """fn on [1, ...] slices of each tensor, chunk by chunk (the oracle is batch 1), results concatenated"""
    with torch.no_grad():
        return torch.cat([fn(*[t[k:k + 1] if t.dim() == 4 else t[k] for t in tensors]) for k in range(tensors[0].shape[0])], 0)


def stats64(t):
    """[n, C, F, T] -> float64 [n, T, 2] = (mean, 1 / (std + 1e-6)) per frame"""
    t = t.double()
    return torch.stack([t.mean(dim=(1, 2)), 1.0 / (t.std(dim=(1, 2), unbiased=True) + 1e-6)], dim=-1)


def assert_stats(got, want, what):
    """device statistics rows [n, T, 2] against float64 ones, valid frames"""
    got, want = got.double(), want.double()
    dm, di = float((got[..., 0] - want[..., 0]).abs().max()), float(((got[..., 1] - want[..., 1]).abs() / want[..., 1].abs()).max())
    print(f"dfsmn kernels stats {what}: max |mean - mean64| {dm:.2e}, max rel 1/std {di:.2e}")
    torch.testing.assert_close(got[..., 0], want[..., 0], rtol=1e-5, atol=1e-6, msg=lambda m: f"{what} mean: {m}")
    torch.testing.assert_close(got[..., 1], want[..., 1], rtol=1e-4, atol=1e-6, msg=lambda m: f"{what} 1/std: {m}")


def figures(stage, path, what, tensors):
    """tensors {name: (device, float64 reference, float32 restatement)}, each [n, C, F, T] -> {"name all" / "name frame": (e_dev, e_32)},
    the absolute tolerance asserted on the way"""
    figs = {}
    for name, (y, y64, y32) in tensors.items():
        assert y.dtype == F32 and y.shape == y64.shape and bool(torch.isfinite(y).all()), (stage, path, what, name)
        e_all, e_frame, scale, dead = ref.rel_errors(y, y64)
        r_all, r_frame, _, _ = ref.rel_errors(y32, y64)
        print(f"dfsmn kernels {stage} {path} {what} {name}: all {e_all:.2e} (e32 {r_all:.2e}) frame {e_frame:.2e} (e32 {r_frame:.2e}) scale {scale:.3g}")
        assert dead == 0.0, (stage, path, what, name, dead)                      # a frame whose reference is all zeros is all zeros
        assert e_all * scale <= sh.SCALE_TOL * max(1.0, scale), (stage, path, what, name, e_all, scale)
        figs[name + " all"], figs[name + " frame"] = (e_all, r_all), (e_frame, r_frame)
    return figs


def hold(stage, case, path, frames, chunks, **kw):
    """One case against the bound measured at the stage's pinned shape on the same path"""
    if stage not in sh._PINNED_RUN:
        sh._PINNED_RUN[stage] = lambda p: case(p, *PIN)
    sh.assert_float32_grade(stage, path, case(path, frames, chunks, **kw), (frames, chunks, kw))


def same_valid_frames(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


# ======================================================================================================================================
# the gated conv block: cfb_front -> lstm_f -> cfb_back
# ======================================================================================================================================
def block_run(path, name, frames, chunks, packed=False, fill=False, only=None, back_split=False, pick=None):
    """`Iccrn.cfb` of block `name` on the stage's input (only: that chunk alone) -> host tensors [n, C, F, T] / [n, T, 2] of the chunks
    `pick`: the input as the device holds it, y1, li, hf, out, stats1, stats_li and the merged partial statistics of out"""
    cin = BLOCKS[name]
    x = stage_input(name, cin, frames, chunks)
    if only is not None:
        x = x[only:only + 1]
    n = x.shape[0]
    pick = list(range(n)) if pick is None else pick
    stride = dfsmn.packed_stride(frames) if packed else None
    seed = SEED + frames if fill else None
    src = make_ft(x, stride, seed)
    with sh.arithmetic(path), layout(stride, back_split) as nn:
        tiles = nn._tiles(n, frames)
        assert tiles == src.tiles
        if name == "cfb_d5":                                                    # statistics: a frame_stats pass inside Iccrn.cfb
            xin, views, parts = src, (src.view(), None), {}
        else:                                                                   # statistics: the partials of the kernel that wrote the input
            xin, z4 = empty_ft(n, frames, cin, stride), empty_ft(n, frames, 4, stride)
            parts, views = {}, []
            for key, off in (("a_part", 0), ("b_part", 20))[:cin // 20]:
                parts[key] = nn.new_part(tiles)
                nn.pw(0, src.view(off, 20), z4.view(), None, "test.copy.weight", "test.copy.bias", xin.view(off, 20), od.F_BINS, 20, tiles=tiles,
                      part0=parts[key])
                views.append(xin.view(off, 20))
            views = (views[0], views[1] if cin == 40 else None)
            assert torch.equal(xin.data, src.data)                              # a copy, padding frames included
        out = empty_ft(n, frames, 40 if name == "cfb_d3" else 20, stride)
        if name == "cfb_d3":
            out.data.copy_(torch.arange(out.data.numel(), device=out.data.device, dtype=F32).view_as(out.data) % 251.0 - 125.0)
            before = out.data[:, :20].clone()
        sc, out_part = nn.cfb(name, views[0], views[1], out.view(20, 20) if name == "cfb_d3" else out.view(), n, frames, {}, **parts)
        out_stats = nn.merged_stats(out_part, None, tiles)
        if name == "cfb_d3":
            assert torch.equal(out.data[:, :20], before)                        # the other half of the output tensor: untouched
    st = src.stride
    r = dict(x=ft_read(xin.data, st, frames, pick), out=ft_read(out.data, st, frames, pick)[:, -20:], out_stats=stats_read(out_stats, st, frames, pick))
    for k in ("y1", "li", "hf"):
        assert sc[k].stride == st and sc[k].tiles == tiles
        r[k] = ft_read(sc[k].data, st, frames, pick)
    for k in ("stats1", "stats_li"):
        r[k] = stats_read(sc[k], st, frames, pick)
    assert torch.equal(r["x"], x[pick])                                         # the reference sees what the block was fed
    return r


@functools.lru_cache(maxsize=4)
def block_reference(name, frames, chunks, pick=None):
    """float64 and float32: the front restatement and oracle.dfsmn.cfb of the stage's input"""
    x = stage_input(name, BLOCKS[name], frames, chunks)
    x = x if pick is None else x[list(pick)]
    r = {}
    for dt in (F64, F32):
        fr = [ref.cfb_front(x[k:k + 1].to(dt), W(dt), name, ceps(dt)) for k in range(x.shape[0])]
        r[dt] = {k: (torch.cat if fr[0][k].dim() == 4 else torch.stack)([f[k] for f in fr], 0) for k in ("y1", "S", "stats1", "stats_li")}
        r[dt]["out"] = per_chunk(lambda xx: od.cfb(xx, W(dt), name, ceps(dt)), x.to(dt))
    return r


def front_case(name, path, frames, chunks, pick=None, **kw):
    with torch.no_grad():
        d, r = block_run(path, name, frames, chunks, pick=pick, **kw), block_reference(name, frames, chunks, None if pick is None else tuple(pick))
    what = f"T={frames} chunks={chunks}"
    assert_stats(d["stats1"], r[F64]["stats1"], f"{name} {path} {what} stats1 (gx)")
    assert_stats(d["stats_li"], r[F64]["stats_li"], f"{name} {path} {what} stats_li (S)")
    # im(bin 0) and im(bin 80) are structural zeros on the device (include/vadx.h: "written as 0").  The reference's float32 sine row of bin
    # 80 is -sin(fl(pi t)), up to 5.2e-5 instead of zero, so its im(80) is a rounding artefact of the table, not a signal: it is held on its
    # own to the absolute tolerance and left out of li's figures, where it would be the whole of `frame` (1.9e-5 against 1e-6)
    dead = r[F64]["S"][:, 20:, 80].abs().max()
    print(f"dfsmn kernels front {name} {path} {what} li im(80): device 0, reference max {float(dead):.2e}")
    assert float(d["li"][:, 20:, [0, 80]].abs().max()) == 0.0 and float(r[F64]["S"][:, 20:, 0].abs().max()) == 0.0
    assert float(dead) <= sh.SCALE_TOL * max(1.0, float(r[F64]["S"].abs().max()))
    s64, s32 = r[F64]["S"].clone(), r[F32]["S"].clone()
    s64[:, 20:, 80], s32[:, 20:, 80] = 0.0, 0.0
    return figures("front " + name, path, what, {"y1": (d["y1"], r[F64]["y1"], r[F32]["y1"]), "li": (d["li"], s64, s32)})


def lstm_f_case(name, path, frames, chunks, pick=None, **kw):
    d = block_run(path, name, frames, chunks, pick=pick, **kw)
    cu = name + ".ceps_unit"
    hid = {dt: per_chunk(lambda s, st: ref.lstm_f_hidden(s, st, W(dt), cu), d["li"].to(dt), d["stats_li"].to(dt)) for dt in (F64, F32)}
    return figures("lstm_f " + name, path, f"T={frames} chunks={chunks}", {"hf": (d["hf"], hid[F64], hid[F32])})


def back_case(name, path, frames, chunks, pick=None, **kw):
    d = block_run(path, name, frames, chunks, pick=pick, back_split=path == "split", **kw)
    out = {dt: per_chunk(lambda s, y1, st, hf: ref.cfb_back(s, y1, st, W(dt), name, ceps(dt), hf=hf),
                         d["li"].to(dt), d["y1"].to(dt), d["stats1"].to(dt), d["hf"].to(dt)) for dt in (F64, F32)}
    assert_stats(d["out_stats"], stats64(d["out"]), f"{name} {path} T={frames} chunks={chunks} merged partials of out")
    return figures("back " + name, path, f"T={frames} chunks={chunks}", {"out": (d["out"], out[F64], out[F32])})


def whole_block_case(name, path, frames, chunks, pick=None, **kw):
    with torch.no_grad():
        d, r = block_run(path, name, frames, chunks, pick=pick, **kw), block_reference(name, frames, chunks, None if pick is None else tuple(pick))
    return figures("block " + name, path, f"T={frames} chunks={chunks}", {"out": (d["out"], r[F64]["out"], r[F32]["out"])})


BLOCK_STAGES = {"front": (front_case, ["f32", "split"]), "lstm_f": (lstm_f_case, PATHS), "back": (back_case, ["f32", "split"]),
                "block": (whole_block_case, PATHS)}


def block_stage(stage, name):
    return functools.partial(BLOCK_STAGES[stage][0], name)


@pytest.mark.parametrize("path", ["f32", "split"])
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("name", list(BLOCKS))
def test_cfb_front(name, frames, chunks, path):
    """cfb_front on its own: y1 = conv31(LN1.w gx) un-normalised, li = DFT_F(LN2(r)), the statistics rows of gx and of li"""
    hold("front " + name, block_stage("front", name), path, frames, chunks)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("name", list(BLOCKS))
def test_cfb_lstm_f(name, frames, chunks, path):
    """The CepsUnit's bi-LSTM along F on the device's own li and stats_li: float32 MFMAs, bf16 x 3 and fp16 x 2 split products"""
    hold("lstm_f " + name, block_stage("lstm_f", name), path, frames, chunks)
    assert sh.range_flag(net()) == (0, 0.0)


@pytest.mark.parametrize("path", ["f32", "split"])
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("name", list(BLOCKS))
def test_cfb_back(name, frames, chunks, path):
    """cfb_back on the device's own hf, li, y1 and stats1 (split: the opt-in split-product form, cfb_back_split), and the partial
    statistics it emits, merged, against the float64 statistics of what it wrote"""
    hold("back " + name, block_stage("back", name), path, frames, chunks)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("name", list(BLOCKS))
def test_cfb_block(name, frames, chunks, path):
    hold("block " + name, block_stage("block", name), path, frames, chunks)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("name", list(BLOCKS))
def test_cfb_bitwise_properties(name, frames, chunks, path):
    """Valid frames of every tensor the block writes, bit for bit: with the padding frames of the input filled; each chunk of the batch
    alone; on the packed layout (T in PACKED_FRAMES), plain, filled and alone; the split-product cfb_back likewise (path split);
    h2 = split in cfb_front."""
    for back_split in ([False, True] if path == "split" else [False]):
        kw = dict(back_split=back_split)
        base = block_run(path, name, frames, chunks, **kw)
        same_valid_frames(base, block_run(path, name, frames, chunks, fill=True, **kw), "padding filled")
        layouts = [False, True] if frames in PACKED_FRAMES else [False]
        for packed in layouts:
            if packed:
                same_valid_frames(base, block_run(path, name, frames, chunks, packed=True, **kw), "packed")
                same_valid_frames(base, block_run(path, name, frames, chunks, packed=True, fill=True, **kw), "packed, padding filled")
            for k in range(chunks if chunks > 1 else 0):
                alone = block_run(path, name, frames, chunks, packed=packed, only=k, **kw)
                same_valid_frames({key: v[k:k + 1] for key, v in base.items()}, alone, f"chunk {k} alone, packed {packed}")
    if path == "h2":
        split = block_run("split", name, frames, chunks)
        same_valid_frames({k: base[k] for k in ("y1", "li", "stats1", "stats_li")}, split, "h2 = split in cfb_front")


PERSISTENT = (16, 300)
PERSISTENT_PICK = [0, 1, 255, 256, 299]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("stage", list(BLOCK_STAGES))
def test_cfb_persistent_workgroups_walk_a_second_tile(stage, path):
    """300 tiles on 256 CUs: cfb_front / cfb_back run one workgroup per CU and walk the rest; tiles 0, 1, 255, 256, 299 are compared, held
    to the bound of the stage's pinned shape"""
    if path not in BLOCK_STAGES[stage][1]:
        path = "split"                                                          # (front / back have no h2 form: the split one again)
    hold(stage + " cfb_e1", block_stage(stage, "cfb_e1"), path, *PERSISTENT, pick=PERSISTENT_PICK)


# ======================================================================================================================================
# the input and output stages: lstm_f (4 channels), pw_conv 40 -> 20, 24 -> 20, 60 -> 2
# ======================================================================================================================================
def in_run(path, frames, chunks, packed=False, fill=False, only=None):
    x = stage_input("in", 4, frames, chunks)
    if only is not None:
        x = x[only:only + 1]
    n = x.shape[0]
    stride = dfsmn.packed_stride(frames) if packed else None
    x4 = make_ft(x, stride, SEED + frames if fill else None)
    with sh.arithmetic(path), layout(stride) as nn:
        tiles = nn._tiles(n, frames)
        hf0, e0l, e0, part = empty_ft(n, frames, 40, stride), empty_ft(n, frames, 20, stride), empty_ft(n, frames, 20, stride), nn.new_part(tiles)
        nn.lstm_f("in_ch_lstm", x4.view(), None, hf0.view(), od.F_BINS, tiles)
        nn.pw(0, hf0.view(), None, None, "in_ch_lstm.linear.weight", "in_ch_lstm.linear.bias", e0l.view(), od.F_BINS, 20, tiles=tiles)
        nn.pw(0, e0l.view(), x4.view(), None, "in_conv.weight", "in_conv.bias", e0.view(), od.F_BINS, 20, tiles=tiles, part0=part)
        e0_stats = nn.merged_stats(part, None, tiles)
    ids, st = list(range(n)), x4.stride
    r = dict(x=ft_read(x4.data, st, frames, ids), e0l=ft_read(e0l.data, st, frames, ids), e0=ft_read(e0.data, st, frames, ids),
             e0_stats=stats_read(e0_stats, st, frames, ids))
    assert torch.equal(r["x"], x)
    return r


def in_lstm_case(path, frames, chunks, **kw):
    d = in_run(path, frames, chunks, **kw)
    e = {dt: per_chunk(lambda xx: od.ch_lstm_f(xx, W(dt), "in_ch_lstm", 4, 20, 20, od.F_BINS), d["x"].to(dt)) for dt in (F64, F32)}
    return figures("in lstm", path, f"T={frames} chunks={chunks}", {"e0l": (d["e0l"], e[F64], e[F32])})


def in_conv_case(path, frames, chunks, **kw):
    d = in_run(path, frames, chunks, **kw)
    cat = torch.cat([d["e0l"], d["x"]], 1)
    e = {dt: torch.nn.functional.conv2d(cat.to(dt), W(dt)["in_conv.weight"], W(dt)["in_conv.bias"]) for dt in (F64, F32)}
    assert_stats(d["e0_stats"], stats64(d["e0"]), f"in conv {path} T={frames} chunks={chunks} merged partials of e0")
    return figures("in conv", path, f"T={frames} chunks={chunks}", {"e0": (d["e0"], e[F64], e[F32])})


@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
def test_input_stage(frames, chunks):
    """lstm_f (4 channels) -> pw_conv 40 -> 20 against oracle ch_lstm_f; pw_conv 24 -> 20 over two views on the device's own e0l; one kernel
    for every arithmetic: split and h2 bit-identical to f32; the bitwise properties on all of it"""
    hold("in lstm", in_lstm_case, "f32", frames, chunks)
    hold("in conv", in_conv_case, "f32", frames, chunks)
    base = in_run("f32", frames, chunks)
    for path in ("split", "h2"):
        same_valid_frames(base, in_run(path, frames, chunks), path + " = f32")
    same_valid_frames(base, in_run("f32", frames, chunks, fill=True), "padding filled")
    for packed in ([False, True] if frames in PACKED_FRAMES else [False]):
        if packed:
            same_valid_frames(base, in_run("f32", frames, chunks, packed=True), "packed")
            same_valid_frames(base, in_run("f32", frames, chunks, packed=True, fill=True), "packed, padding filled")
        for k in range(chunks if chunks > 1 else 0):
            same_valid_frames({key: v[k:k + 1] for key, v in base.items()}, in_run("f32", frames, chunks, packed=packed, only=k), f"chunk {k} alone")


def out_run(path, frames, chunks, packed=False, fill=False, only=None):
    x = stage_input("out", 80, frames, chunks)                                  # d0 = channels [0, 40), the other tensor = [40, 80): its [20, 40) is view b
    if only is not None:
        x = x[only:only + 1]
    n = x.shape[0]
    stride = dfsmn.packed_stride(frames) if packed else None
    seed = SEED + frames if fill else None
    d0, cat = make_ft(x[:, :40].contiguous(), stride, seed), make_ft(x[:, 40:].contiguous(), stride, None if seed is None else seed + 1)
    with sh.arithmetic(path), layout(stride) as nn:
        tiles = nn._tiles(n, frames)
        y = empty_ft(n, frames, 2, stride)
        nn.pw(0, d0.view(), cat.view(20, 20), None, "out_conv.weight", "out_conv.bias", y.view(), od.F_BINS, 2, tiles=tiles)
    ids = list(range(n))
    r = dict(d0=ft_read(d0.data, d0.stride, frames, ids), d1=ft_read(cat.data, d0.stride, frames, ids)[:, 20:], y=ft_read(y.data, d0.stride, frames, ids))
    assert torch.equal(torch.cat([r["d0"], r["d1"]], 1), torch.cat([x[:, :40], x[:, 60:]], 1))
    return r


def out_case(path, frames, chunks, **kw):
    d = out_run(path, frames, chunks, **kw)
    cat = torch.cat([d["d0"], d["d1"]], 1)
    e = {dt: torch.nn.functional.conv2d(cat.to(dt), W(dt)["out_conv.weight"], W(dt)["out_conv.bias"]) for dt in (F64, F32)}
    return figures("out", path, f"T={frames} chunks={chunks}", {"y": (d["y"], e[F64], e[F32])})


@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
def test_output_stage(frames, chunks):
    """pw_conv 60 -> 2: a = a 40-channel tensor, b = channels [20, 40) of another 40-channel tensor whose first half differs"""
    hold("out", out_case, "f32", frames, chunks)
    base = out_run("f32", frames, chunks)
    same_valid_frames(base, out_run("f32", frames, chunks, fill=True), "padding filled")
    for packed in ([False, True] if frames in PACKED_FRAMES else [False]):
        if packed:
            same_valid_frames(base, out_run("f32", frames, chunks, packed=True), "packed")
            same_valid_frames(base, out_run("f32", frames, chunks, packed=True, fill=True), "packed, padding filled")
        for k in range(chunks if chunks > 1 else 0):
            same_valid_frames({key: v[k:k + 1] for key, v in base.items()}, out_run("f32", frames, chunks, packed=packed, only=k), f"chunk {k} alone")


PW_TILES, PW_PICK = 4096, [0, 1, 4095]


def pw4096_case(path, frames, chunks, **kw):
    """pw_conv 24 -> 20 on `chunks` one-tile chunks, drawn on the device; (frames, chunks) = PIN is the stage's pinned shape, tile-aligned"""
    nn, pick = net(), (PW_PICK if chunks == PW_TILES else list(range(chunks)))
    g = torch.Generator(device=nn.device).manual_seed(SEED + 100000 * STAGE_IDS.index("pw4096") + chunks)
    src = empty_ft(chunks, frames, 24, None)
    src.data.copy_(torch.randn(src.data.shape, generator=g, device=nn.device))
    src.data[:src.nt] += 25.0
    src.data.mul_(torch.tensor([1.0, 0.1, 0.01], device=nn.device)[torch.arange(16, device=nn.device) % 3])
    src.data[-src.nt:] = 0.0
    e0, part = empty_ft(chunks, frames, 20, None), nn.new_part(src.tiles)
    with sh.arithmetic(path):
        nn.pw(0, src.view(0, 20), src.view(20, 4), None, "in_conv.weight", "in_conv.bias", e0.view(), od.F_BINS, 20, tiles=src.tiles, part0=part)
        st = nn.merged_stats(part, None, src.tiles)
    x, y = ft_read(src.data, src.stride, frames, pick), ft_read(e0.data, src.stride, frames, pick)
    e = {dt: torch.nn.functional.conv2d(x.to(dt), W(dt)["in_conv.weight"], W(dt)["in_conv.bias"]) for dt in (F64, F32)}
    assert_stats(stats_read(st, src.stride, frames, pick), stats64(y), f"pw4096 T={frames} chunks={chunks} merged partials")
    return figures("pw 24 -> 20", path, f"T={frames} chunks={chunks}", {"e0": (y, e[F64], e[F32])})


def test_pw_conv_one_workgroup_per_tile_grid():
    """At 4096 tiles pw_conv's grid changes from two workgroups per tile to one (each then emits both partial statistics)"""
    hold("pw 24 -> 20", pw4096_case, "f32", 16, PW_TILES)


# ======================================================================================================================================
# the time LSTMs
# ======================================================================================================================================
def lstm_t_run(which, path, frames, chunks, packed=False, fill=False, only=None):
    stage, cin, prefix = ("lstm_t0", 20, "ch_lstm") if which == 0 else ("lstm_t1", 40, "out_ch_lstm")
    x = stage_input(stage, cin, frames, chunks)
    if only is not None:
        x = x[only:only + 1]
    n = x.shape[0]
    stride = dfsmn.packed_stride(frames) if packed else None
    seed = SEED + frames if fill else None
    xin = make_ft(x, stride, seed)
    with sh.arithmetic(path), layout(stride) as nn:
        assert nn.lstm_t_h2
        out = empty_ft(n, frames, cin, stride)
        r = {}
        if which == 0:
            st = nn.stats(xin.view(), None, od.F_BINS, xin.tiles)
            r["stats"] = stats_read(st, xin.stride, frames, list(range(n)))
            if fill:
                fill_stats_padding(st, n, frames, xin.stride, seed + 2)
            nn.lstm_t(0, prefix, xin.view(), nn._ln(st, "ln"), xin.view(), out.view(), frames, n)
        else:
            nn.lstm_t(1, prefix, xin.view(), None, None, out.view(), frames, n)
        assert sh.range_flag(nn) == (0, 0.0), (which, path, frames, chunks)      # in-range operands never raise the fp16 x 2 flag
    r.update(x=ft_read(xin.data, xin.stride, frames, list(range(n))), y=ft_read(out.data, xin.stride, frames, list(range(n))))
    assert torch.equal(r["x"], x)
    return r


def lstm_t_case(which, path, frames, chunks, **kw):
    d = lstm_t_run(which, path, frames, chunks, **kw)
    if which == 0:
        fn = lambda dt: (lambda xx: xx * od.ch_lstm_t(od.layer_norm(xx, W(dt), "ln"), W(dt), "ch_lstm", 20, 40, 20, 2))      # noqa: E731
        assert_stats(d["stats"], stats64(d["x"]), f"lstm_t 0 {path} T={frames} chunks={chunks} frame_stats of e5")
    else:
        fn = lambda dt: (lambda xx: od.ch_lstm_t(xx, W(dt), "out_ch_lstm", 40, 20, 40, 1))      # noqa: E731
    e = {dt: per_chunk(fn(dt), d["x"].to(dt)) for dt in (F64, F32)}
    return figures(f"lstm_t {which}", path, f"T={frames} chunks={chunks}", {"y": (d["y"], e[F64], e[F32])})


def lstm_t_properties(which, path, frames, chunks):
    base = lstm_t_run(which, path, frames, chunks)
    same_valid_frames(base, lstm_t_run(which, path, frames, chunks, fill=True), "padding filled")
    for packed in ([False, True] if frames in PACKED_FRAMES else [False]):
        if packed:
            same_valid_frames(base, lstm_t_run(which, path, frames, chunks, packed=True), "packed")
            same_valid_frames(base, lstm_t_run(which, path, frames, chunks, packed=True, fill=True), "packed, padding filled")
        for k in range(chunks if chunks > 1 else 0):
            same_valid_frames({key: v[k:k + 1] for key, v in base.items()}, lstm_t_run(which, path, frames, chunks, packed=packed, only=k),
                              f"chunk {k} alone, packed {packed}")
    return base


@pytest.mark.parametrize("path", ["f32", "h2"])
@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
def test_time_lstm_0(frames, chunks, path):
    """The two-layer bottleneck LSTM (lstm_t2_kernel / lstm_t2h_kernel) with LayerNorm from a frame_stats pass, its output multiplied by
    its input: 10 / 20 / 30 bin groups at four per workgroup"""
    hold("lstm_t 0", functools.partial(lstm_t_case, 0), path, frames, chunks)
    lstm_t_properties(0, path, frames, chunks)


@pytest.mark.parametrize("chunks", CHUNKS)
@pytest.mark.parametrize("frames", FRAMES)
def test_time_lstm_1(frames, chunks):
    """The one-layer output LSTM (lstm_t_kernel: a loader wave four frames ahead): float32 MFMAs for every arithmetic"""
    hold("lstm_t 1", functools.partial(lstm_t_case, 1), "f32", frames, chunks)
    base = lstm_t_properties(1, "f32", frames, chunks)
    for path in ("split", "h2"):
        same_valid_frames(base, lstm_t_run(1, path, frames, chunks), path + " = f32")
