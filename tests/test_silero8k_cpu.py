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
