"""The 8 kHz Silero network's host side: weights, shape checks, the packed blob (CPU only, libvadx.so built)."""
import ctypes as C
import os

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, checkpoints, silero, weights

import _containers as CW

import _silero8k_ref as ref


def test_shape_check_and_resolve():
    w = weights.silero8k_synthetic(5)
    assert weights.silero_check(w, sample_rate=8000)
    with pytest.raises(ValueError):
        weights.silero_check(w)                                   # 16 kHz shapes
    with pytest.raises(ValueError):
        weights.silero_check(weights.silero_synthetic(5), sample_rate=8000)
    with pytest.raises(ValueError):
        weights.silero_check(w, sample_rate=22050)
    r = checkpoints.resolve("silero8k", "synthetic:5")
    assert set(r) == set(w) and all(np.array_equal(r[k], w[k]) for k in w)
    assert checkpoints.resolve("silero8k", w) is w
    with pytest.raises(ValueError):
        checkpoints.resolve("silero8k", None)
    b = weights.silero8k_stft_basis()
    assert b.shape == (130, 128) and b.dtype == np.float32
    n = np.arange(128)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / 128)
    assert np.allclose(b[5], np.cos(2 * np.pi * 5 * n / 128) * win, atol=1e-6)
    assert np.allclose(b[65 + 5], -np.sin(2 * np.pi * 5 * n / 128) * win, atol=1e-6)


def test_cfg_size_unchanged():
    assert C.sizeof(_lib.SileroCfg) == 16
    assert [f[0] for f in _lib.SileroCfg._fields_] == ["arithmetic", "sample_rate", "reserved"]


def _blob_offsets():
    """the packed-blob offsets, evaluated from the constexpr lines of csrc/silero_common.h (not copied by hand)"""
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "silero_common.h")).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (\w+) = ([^;]+);", src):
        env[name] = eval(expr.replace("/", "//"), {}, dict(env))
    return env


def test_pack_host_sr_shares_the_16k_sections():
    L = _lib.lib()
    assert L.vadx_silero_packed_floats_sr(8000) == L.vadx_silero_packed_floats() == L.vadx_silero_packed_floats_sr(16000)
    assert L.vadx_silero_packed_floats_sr(22050) == 0
    o = _blob_offsets()
    assert o["PACKED_FLOATS"] == L.vadx_silero_packed_floats()
    w16 = weights.silero_synthetic(3)
    w8 = dict(w16)
    w8["stft_basis"], w8["enc0_w"], w8["enc0_b"] = (weights.silero8k_stft_basis(), weights.silero8k_synthetic(3)["enc0_w"],
                                                     weights.silero8k_synthetic(3)["enc0_b"])
    p16, p8 = silero._pack(w16, 16000).view(np.uint32), silero._pack(w8, 8000).view(np.uint32)
    # the sections the 16 kHz and 8 kHz networks share are bitwise what the 16 kHz packer writes for the same tensors, in all three
    # layouts: f32 conv2 .. decoder [OFF_C2, OFF_SF), bf16 x 3 conv2 .. W_hh [OFF_Q2, OFF_QSF), fp16 x 2 conv2 .. W_hh [OFF_H2, OFF_HSF)
    for a, b in (("OFF_C2", "OFF_SF"), ("OFF_Q2", "OFF_QSF"), ("OFF_H2", "OFF_HSF")):
        lo, hi = o[a], o[b]
        assert hi > lo and np.array_equal(p8[lo:hi], p16[lo:hi]), (a, b)
        assert p8[lo:hi].any()
    assert p8[o["OFF_HFLAG"]] == p16[o["OFF_HFLAG"]] == np.float32(1.0).view(np.uint32)        # fp16 x 2 usable, both
    # the 8 kHz network's own conv1 bias at OFF_B1, the tag in the pad word behind OFF_FOLD (zero in a 16 kHz blob)
    assert np.array_equal(p8[o["OFF_B1"]:o["OFF_B1"] + 128].view(np.float32), w8["enc0_b"])
    tag = o["OFF_FOLD"] + 1
    assert p16[tag] == 0 and p8[tag].view(np.float32) == 8000.0
    # the 16 kHz network's own sections past OFF_B1 are left empty in an 8 kHz blob
    for a, b in (("OFF_SF", "OFF_FOLD"), ("OFF_Q1", "OFF_Q2"), ("OFF_QSF", "OFF_H1"), ("OFF_H1", "OFF_H2"), ("OFF_HSF", "OFF_HFLAG")):
        assert not p8[o[a]:o[b]].any(), (a, b)


def test_pack_host_sr_rejects_bad_rate():
    L = _lib.lib()
    w = weights.silero8k_synthetic(1)
    p = np.zeros(L.vadx_silero_packed_floats(), dtype=np.float32)
    hw = _lib.SileroWeightsHost()
    assert L.vadx_silero_pack_host_sr(22050, C.byref(hw), p.ctypes.data_as(C.c_void_p)) == -1
    assert L.vadx_silero_pack_host_sr(8000, None, p.ctypes.data_as(C.c_void_p)) == -1
    assert silero._pack(w, 8000)[-4] == 1.0


def test_restated_synthetic_clips_cross_both_thresholds():
    w = ref.weights64(weights.silero8k_synthetic(1234))
    audio = weights.burst_clips(4, 8000 * 6, seed=3, sample_rate=8000).astype(np.float32) * np.float32(0.000030517578)
    probs, _ = ref.clip_probs(w, audio)
    assert probs.shape == (4, (8000 * 6 + 255) // 256)
    for b in range(4):
        assert probs[b].max() > 0.5 and probs[b].min() < 0.35, (probs[b].min(), probs[b].max())


# ------------------------------------------------------------------ the 8 kHz branch of a .onnx file
def _branch(w, tag, lstm_node, stride, pad):
    """one Silero sub-graph in the layout of an exported silero_vad.onnx: reflect Pad -> STFT Conv -> |.| -> four Conv -> LSTM -> Conv"""
    inits = [(f"{tag}.stft.forward_basis_buffer", w["stft_basis"].reshape(w["stft_basis"].shape[0], 1, -1)),
             (f"{tag}.pads", np.array([0, 0, 0, pad], np.int64))]
    nodes = [CW.enc_node("Pad", ["x", f"{tag}.pads"], ["xp"], f"/{tag}/stft/Pad", attrs={"mode": b"reflect"}),
             CW.enc_node("Conv", ["xp", f"{tag}.stft.forward_basis_buffer"], ["spec"], f"/{tag}/stft/Conv", attrs={"strides": [stride]})]
    prev = "mag"
    for i in range(4):
        wn, bn = f"{tag}.encoder.{i}.reparam_conv.weight", f"onnx::Conv_{100 + i}_{tag}"
        inits += [(wn, w[f"enc{i}_w"], bool(i & 1)), (bn, w[f"enc{i}_b"], False)]
        nodes.append(CW.enc_node("Conv", [prev, wn, bn], [f"c{i}"], f"/{tag}/encoder.{i}/Conv"))
        prev = f"c{i}"
    H = 128
    if lstm_node:
        order = np.concatenate([np.arange(H) + H * gi for gi in (0, 3, 1, 2)])          # torch i,f,g,o -> ONNX i,o,f,c
        B = np.concatenate([w["lstm_b_ih"][order], w["lstm_b_hh"][order]])[None]
        inits += [(f"onnx::LSTM_{tag}_W", w["lstm_w_ih"][order][None]), (f"onnx::LSTM_{tag}_R", w["lstm_w_hh"][order][None]),
                  (f"onnx::LSTM_{tag}_B", B)]
        nodes.append(CW.enc_node("LSTM", [prev, f"onnx::LSTM_{tag}_W", f"onnx::LSTM_{tag}_R", f"onnx::LSTM_{tag}_B", "", "h0", "c0"],
                                 ["y", "hn", "cn"], f"/{tag}/decoder/rnn/LSTM", attrs={"hidden_size": H}))
    else:
        inits += [(f"{tag}.decoder.rnn.weight_ih", w["lstm_w_ih"]), (f"{tag}.decoder.rnn.weight_hh", w["lstm_w_hh"]),
                  (f"{tag}.decoder.rnn.bias_ih", w["lstm_b_ih"]), (f"{tag}.decoder.rnn.bias_hh", w["lstm_b_hh"])]
    inits += [(f"{tag}.decoder.decoder.2.weight", w["dec_w"].reshape(1, 128, 1)), (f"{tag}.decoder.decoder.2.bias", w["dec_b"])]
    nodes.append(CW.enc_node("Conv", ["relu_h", f"{tag}.decoder.decoder.2.weight", f"{tag}.decoder.decoder.2.bias"], ["logit"],
                             f"/{tag}/decoder/Conv"))
    return CW.enc_graph(nodes, inits, tag)


def _two_branch(path, w16, w8, lstm_node=True, stride8=64, pad8=32, with_8k=True):
    attrs = {"then_branch": ("graph", _branch(w16, "m16", lstm_node, 128, 64))}
    if with_8k:
        attrs["else_branch"] = ("graph", _branch(w8, "m8", lstm_node, stride8, pad8))
    top = CW.enc_graph([CW.enc_node("Equal", ["sr", "c16k"], ["is16"]), CW.enc_node("If", ["is16"], ["out", "stateN"], "If_0", attrs=attrs)],
                       [("c16k", np.array(16000, np.int64))])
    return CW.write_onnx(str(path), top)


def _same(got, want):
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("lstm_node", [True, False])
def test_silero_8k_onnx_loader(tmp_path, lstm_node):
    w16, w8 = weights.silero_synthetic(21), weights.silero8k_synthetic(21)
    path = _two_branch(tmp_path / "two.onnx", w16, w8, lstm_node)
    _same(checkpoints.silero_8k_from_onnx(path), w8)
    _same(checkpoints.resolve("silero8k", path), w8)
    _same(checkpoints.silero_from_onnx(path), w16)               # the 16 kHz reader still picks its own branch
    weights.silero_check(checkpoints.silero_8k_from_onnx(path), sample_rate=8000)
    # what SileroEngine / load_silero_vad load for an .onnx path: the file's 8 kHz branch; given weights_8k wins; no .onnx -> none
    _same(silero._weights_8k_spec(path, None), w8)
    _same(silero._weights_8k_spec(path, "synthetic:3"), weights.silero8k_synthetic(3))
    assert silero._weights_8k_spec("synthetic:3", None) is None


def test_silero_8k_onnx_loader_refuses_other_geometry(tmp_path):
    w16, w8 = weights.silero_synthetic(22), weights.silero8k_synthetic(22)
    with pytest.raises(ValueError, match="strides"):
        checkpoints.silero_8k_from_onnx(_two_branch(tmp_path / "s.onnx", w16, w8, stride8=128))
    with pytest.raises(ValueError, match="reflect Pad"):
        checkpoints.silero_8k_from_onnx(_two_branch(tmp_path / "p.onnx", w16, w8, pad8=64))
    with pytest.raises(ValueError, match="strides"):                # the engine's automatic load refuses it too
        silero._weights_8k_spec(str(tmp_path / "s.onnx"), None)


def test_silero_8k_onnx_loader_without_the_branch(tmp_path):
    path = _two_branch(tmp_path / "one.onnx", weights.silero_synthetic(23), None, with_8k=False)
    with pytest.raises(ValueError, match=r"8 kHz Silero tensors .*weight shapes present"):
        checkpoints.silero_8k_from_onnx(path)
    assert checkpoints.silero_8k_from_onnx(path, missing_ok=True) is None
    assert silero._weights_8k_spec(path, None) is None
    other = tmp_path / "x.bin"
    other.write_bytes(b"")
    with pytest.raises(ValueError, match="neither a .onnx"):
        checkpoints.resolve("silero8k", str(other))


# ------------------------------------------------------------------ every split section of both blobs, rebuilt from the weights
def _b3(w):
    """bf16 x 3 (csrc/split3.h): the three truncation-exact terms of w, w - t0, w - t0 - t1 as bf16 bit patterns [3][...]"""
    def top(x):
        return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    t0 = top(w)
    r1 = w - t0
    t1 = top(r1)
    return np.stack([(x.view(np.uint32) >> 16).astype(np.uint16) for x in (t0, t1, r1 - t1)])


def _h2(w):
    """fp16 x 2 (csrc/split2.h): h0 = RN16(w), h1 = RN16((w - h0) * 2^11) as fp16 bit patterns [2][...]"""
    h0 = w.astype(np.float16)
    h1 = ((w - h0.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return np.stack([h0, h1]).view(np.uint16)


def _section(view, split):
    """view [n0][n1][n2][16 rows][32 k] float32 -> the section [n0][n1][n2][plane][q][i][8] (k = 8 q + e) as 16-bit words"""
    v = np.ascontiguousarray(view, dtype=np.float32)
    planes = split(v).reshape((-1,) + v.shape[:3] + (16, 4, 8))             # plane, n0, n1, n2, i, q, e
    return planes.transpose(1, 2, 3, 0, 5, 4, 6).reshape(-1)


def _shared_views(w):
    """conv2 .. W_hh as [section order ..][16][32] (csrc/silero_common.h documents the order per offset)"""
    ih = w["lstm_w_ih"].reshape(4, 8, 16, 4, 32)                           # gate, unit tile, i, chunk, k
    hh = w["lstm_w_hh"].reshape(4, 8, 16, 4, 32)
    return {"2": w["enc1_w"].reshape(4, 16, 4, 32, 3).transpose(0, 2, 4, 1, 3),                  # [oc tile][chunk][tap]
            "3": w["enc2_w"][:, :, 1:].reshape(4, 16, 2, 32, 2).transpose(0, 4, 2, 1, 3),       # [oc tile][tap 1, 2][chunk]
            "4": w["enc3_w"][:, :, 1].reshape(8, 16, 2, 32).transpose(0, 2, 1, 3)[:, :, None],    # [oc tile][chunk], centre tap
            "IH": ih.transpose(1, 3, 0, 2, 4),                                                   # [unit tile][chunk][gate]
            "HH": hh.transpose(1, 0, 3, 2, 4)}                                                   # [unit tile][gate][chunk]


def _folded_stft_view(basis):
    """the folded 16 kHz STFT basis [5 bin tiles][E|O x re|im][2 chunks][16][32] in the packer's own float32 arithmetic: bins 0..63 symmetrised
    over the four table entries that must agree, bin 64 (tile 4, row 0) time-folded; pair m of a class = sample n = 2 m + 2 (E) / 2 m + 1 (O)"""
    re, im = basis[:129], basis[129:]
    q, h = np.float32(0.25), np.float32(0.5)
    out = np.zeros((80, 2, 2, 64), np.float32)                             # bin, class, re | im, pair
    k = np.arange(64)
    for cls in range(2):
        for m in range(64):
            n = 2 * m + 1 if cls else 2 * m + 2
            sg, nm = np.float32(-1.0 if n & 1 else 1.0), (256 - n) & 255
            c = q * (re[k, n] + re[k, nm] + sg * (re[128 - k, n] + re[128 - k, nm]))
            s = q * (im[k, n] - im[k, nm] - sg * (im[128 - k, n] - im[128 - k, nm]))
            out[:64, cls, 0, m] = h * c if n == 128 else c                 # n = 128 is its own mirror
            out[:64, cls, 1, m] = 0.0 if n == 128 else s
            out[64, cls, 0, m] = (h if n == 128 else np.float32(1.0)) * h * (re[64, n] + re[64, nm])
            out[64, cls, 1, m] = 0.0 if n == 128 else h * (im[64, n] - im[64, 256 - n])
    return out.reshape(5, 16, 4, 2, 32).transpose(0, 2, 3, 1, 4)


def _check_sections(blob, o, expected):
    """expected: (first offset name, next offset name, view) per section; both layouts of every view, bitwise, each filling its section"""
    words = blob.view(np.uint16)
    for lo, hi, view, split in expected:
        want = _section(view, split)
        assert want.size == 2 * (o[hi] - o[lo]), (lo, hi, want.size)
        got = words[2 * o[lo]:2 * o[hi]]
        assert got.any() and np.array_equal(got, want), (lo, hi)


def test_every_split_section_is_the_documented_layout_of_its_weights():
    """Every bf16 x 3 (OFF_Q*, OFF8_*Q) and fp16 x 2 (OFF_H*, OFF8_*H) section of the 16 kHz and the 8 kHz blob, rebuilt in numpy from the
    tensors it was packed from ([.. section order ..][plane][q][i][8], k = 8 q + e) and compared bitwise."""
    o = _blob_offsets()
    w16 = weights.silero_synthetic(3)
    order = np.array([s if s <= 64 else 192 - s for s in range(128)])      # conv1's input slots: the order the STFT pass leaves the bins in
    c1 = w16["enc0_w"][:, order].reshape(8, 16, 4, 32, 3).transpose(0, 2, 4, 1, 3)                # [oc tile][chunk][tap]
    sf = _folded_stft_view(w16["stft_basis"])
    sv = _shared_views(w16)
    expected = [("OFF_Q1", "OFF_Q1N", c1, _b3), ("OFF_QSF", "OFF_H1", sf[:4], _b3), ("OFF_H1", "OFF_H2", c1, _h2), ("OFF_HSF", "OFF_HFLAG", sf, _h2)]
    nxt = {"2": "3", "3": "4", "4": "IH", "IH": "HH"}
    for name, view in sv.items():
        expected += [(f"OFF_Q{name}", f"OFF_Q{nxt[name]}" if name in nxt else "OFF_QSF", view, _b3),
                     (f"OFF_H{name}", f"OFF_H{nxt[name]}" if name in nxt else "OFF_HSF", view, _h2)]
    assert len(expected) == 14
    _check_sections(silero._pack(w16, 16000), o, expected)

    w8 = weights.silero8k_synthetic(3)
    b = w8["stft_basis"]
    rows = np.zeros((144, 128), np.float32)                                # tiles 0..3 re of bins 0..63, 4..7 im, 8 = re / im of bin 64 in rows 0 / 1
    rows[:64], rows[64:128], rows[128], rows[129] = b[:64], b[65:129], b[64], b[129]
    st = rows.reshape(9, 16, 4, 32).transpose(0, 2, 1, 3)[:, :, None]                             # [row tile][chunk]
    c1 = w8["enc0_w"][:, :64].reshape(8, 16, 2, 32, 3).transpose(0, 4, 2, 1, 3)                   # [oc tile][tap][chunk]
    expected = [("OFF8_SQ", "OFF8_SH", st, _b3), ("OFF8_SH", "OFF8_C1F", st, _h2), ("OFF8_C1Q", "OFF8_C1H", c1, _b3), ("OFF8_C1H", "OFF8_C1N", c1, _h2)]
    for name, view in _shared_views(w8).items():
        expected += [(f"OFF_Q{name}", f"OFF_Q{nxt[name]}" if name in nxt else "OFF_QSF", view, _b3),
                     (f"OFF_H{name}", f"OFF_H{nxt[name]}" if name in nxt else "OFF_HSF", view, _h2)]
    assert len(expected) == 14
    _check_sections(silero._pack(w8, 8000), o, expected)
