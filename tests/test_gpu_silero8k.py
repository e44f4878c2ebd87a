"""GPU: the 8 kHz Silero network (csrc/silero8k.hip) on all three arithmetics, against the float64 restatement (tests/_silero8k_ref.py)
and against itself bit for bit across entry points."""
import ctypes

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, silero, weights
from oracle import postproc as opp

import _silero8k_ref as ref

pytestmark = pytest.mark.gpu
ATOL = 1e-4
SCALE = np.float32(0.000030517578)


@pytest.fixture(autouse=True, params=["f32", "split", "h2"])
def encoder(request):
    prev = silero.encoder_mode(request.param)
    yield request.param
    silero.encoder_mode(prev)


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234), weights_8k=weights.silero8k_synthetic(1234))


@pytest.fixture(scope="module")
def w64():
    return ref.weights64(weights.silero8k_synthetic(1234))


def _audio(B, n, seed=1):
    return weights.burst_clips(B, n, seed=seed, sample_rate=8000).astype(np.float32) * SCALE


@pytest.mark.parametrize("B,n", [(1, 100), (17, 256), (100, 257), (17, 44715), (1, 80000)])
def test_clips_against_restatement(engine, w64, B, n):
    a = _audio(B, n)
    probs, st = engine.clips(a, return_state=True, sampling_rate=8000)
    rp, rs = ref.clip_probs(w64, a)
    assert probs.shape == (B, (n + 255) // 256)
    np.testing.assert_allclose(probs.cpu().numpy(), rp, atol=ATOL, rtol=0)
    np.testing.assert_allclose(st.cpu().numpy(), rs, atol=ATOL, rtol=0)


@pytest.mark.parametrize("B", [1, 17, 100])
def test_step_against_restatement(engine, w64, B):
    rng = np.random.default_rng(B)
    x = (rng.standard_normal((B, 288)) * 0.1).astype(np.float32)
    s = (rng.standard_normal((2, B, 128)) * 0.3).astype(np.float32)
    out, sn = engine.step(x, s, sampling_rate=8000)
    ro, rs = ref.net_forward(w64, torch.from_numpy(x).double(), torch.from_numpy(s).double())
    np.testing.assert_allclose(out.cpu().numpy(), ro.numpy(), atol=ATOL, rtol=0)
    np.testing.assert_allclose(sn.cpu().numpy(), rs.numpy(), atol=ATOL, rtol=0)
    with pytest.raises(ValueError):
        engine.step(np.zeros((B, 576), np.float32), s, sampling_rate=8000)


def _gx(engine, audio, mode):
    B, N = audio.shape
    _, steps = engine.encode(audio, mode=mode, sampling_rate=8000)
    torch.cuda.synchronize()
    g = engine._ws[:_lib.lib().vadx_silero_workspace_bytes(B, steps)].view(torch.float32).clone()
    # [T][G][8 waves][4 gates][16 q*lanes...]: back to [T][B][512] in torch gate order
    G = (B + 15) // 16
    g = g.view(steps, G, 8, 4, 4, 16, 4).permute(0, 1, 5, 3, 2, 4, 6).reshape(steps, G * 16, 512)[:, :B]
    return g.cpu().double().numpy()


def test_encoder_error_against_float64(engine, w64, encoder):
    if encoder == "f32":
        pytest.skip("the yardstick itself")
    a = _audio(20, 256 * 12, seed=4)
    ad = torch.from_numpy(a).cuda()
    T = 12
    xp = np.zeros((20, 32 + T * 256))
    xp[:, 32:] = a
    want = np.stack([ref.input_projection(w64, torch.from_numpy(xp[:, t * 256:t * 256 + 288])).numpy() for t in range(T)])
    e_f32 = np.abs(_gx(engine, ad, "f32") - want).max()
    e = np.abs(_gx(engine, ad, encoder) - want).max()
    assert e <= 1.25 * e_f32, (e, e_f32)


def test_int16_spans_parts_are_bitwise(engine):
    pcm = weights.burst_clips(40, 20000, seed=7, sample_rate=8000)
    a = torch.from_numpy(pcm.astype(np.float32) * SCALE).cuda()
    p_f = engine.clips(a, sampling_rate=8000)
    p_i = engine.clips_pcm16(torch.from_numpy(pcm).cuda(), sampling_rate=8000)
    assert torch.equal(p_f, p_i)
    probs = torch.empty_like(p_f)
    engine.clips_spanned(a, 20000, probs, span=7, sampling_rate=8000)
    assert torch.equal(p_f, probs)
    # encode_pcm16_part over two slices == one launch
    L = _lib.lib()
    pd = torch.from_numpy(pcm).cuda()
    steps = (20000 + 255) // 256
    ws = torch.empty(L.vadx_silero_workspace_bytes(40, steps), dtype=torch.uint8, device="cuda")
    cfg = engine.cfg(None, 8000)
    for first, nb in ((0, 32), (32, 8)):
        _lib.check(L.vadx_silero_encode_pcm16_part(engine.packed_8k.data_ptr(), pd[first].data_ptr(), float(SCALE), nb, 20000, 20000,
                                                   first, 40, ws.data_ptr(), ws.numel(), _lib.stream_ptr(), cfg))
    out = torch.empty_like(p_f)
    _lib.check(L.vadx_silero_recur(engine.packed_8k.data_ptr(), ws.data_ptr(), ws.numel(), 40, steps, None, out.data_ptr(), None,
                                   _lib.stream_ptr(), cfg))
    if engine.mode(8000) == "h2":          # the whole-batch result above stood unrecomputed only if nothing left the fp16 range
        assert engine.range_flag(sampling_rate=8000)[0] == 0
    assert torch.equal(out, p_f)


def test_wrapper_per_window_equals_audio_forward(engine):
    a = _audio(3, 256 * 9 + 100, seed=9)
    wr = silero.OnnxWrapper(engine)
    full = wr.audio_forward(torch.from_numpy(a), 8000)
    wr.reset_states()
    xp = np.pad(a, ((0, 0), (0, (-a.shape[1]) % 256)))
    per = torch.cat([wr(torch.from_numpy(xp[:, i:i + 256]), 8000) for i in range(0, xp.shape[1], 256)], dim=1)
    assert torch.equal(full, per)
    ts = silero.get_speech_timestamps(torch.from_numpy(_audio(1, 8000 * 6)[0]), wr, sampling_rate=8000)
    assert isinstance(ts, list)


def test_segments_against_oracle(engine, w64):
    a = _audio(6, 8000 * 8, seed=11)
    res, probs = silero.get_speech_timestamps_batch(a, engine, sampling_rate=8000, return_probs=True)
    rp, _ = ref.clip_probs(w64, a)
    for b in range(6):
        want = opp.silero_segments(list(rp[b].astype(np.float32)), a.shape[1], sampling_rate=8000)
        if res[b] != want:
            near = np.min(np.minimum(np.abs(rp[b] - 0.5), np.abs(rp[b] - 0.35)))
            assert near < 2e-4, (b, res[b], want)


def test_iterator_batch_against_clips(engine):
    S, n = 5, 256 * 24
    a = _audio(S, n, seed=13)
    it = silero.VADIteratorBatch(engine, S, sampling_rate=8000)
    ps = []
    for lo, hi in ((0, 1), (1, 4), (4, 12), (12, 24)):
        _, _, p = it.step(a[:, lo * 256:hi * 256])
        ps.append(p)
    got = torch.cat(ps, 1)
    want = engine.clips(a, sampling_rate=8000)
    assert torch.equal(got, want)
    # events equal the host VADIterator over OnnxWrapper
    it2 = silero.VADIteratorBatch(engine, 1, sampling_rate=8000)
    dev = it2(a[:1])[0]
    host = silero.VADIterator(silero.OnnxWrapper(engine), sampling_rate=8000)
    hv = [host(torch.from_numpy(a[0, i:i + 256])) for i in range(0, n, 256)]
    assert dev == hv


def test_two_network_engine_16k_unchanged(engine):
    e16 = silero.SileroEngine(weights.silero_synthetic(1234))
    a = weights.burst_clips(20, 16000 * 3, seed=2).astype(np.float32) * SCALE
    assert torch.equal(engine.clips(a), e16.clips(a))
    assert engine.has_8k and not e16.has_8k


def test_range_protocol(encoder):
    """A loud gain on each arithmetic: fp16 x 2 raises the flag and the guarded call recomputes on bf16 x 3 (bitwise the bf16 x 3 result);
    unchecked fp16 x 2 gives NaN, never plausible scores; bf16 x 3 and f32 have float32's range and neither flag nor recompute."""
    a = _audio(16, 256 * 6, seed=5) * np.float32(3.0e4)
    e = silero.SileroEngine(weights.silero_synthetic(1234), weights_8k=weights.silero8k_synthetic(1234))
    e.range_flag(sampling_rate=8000)
    p = e.clips(a, sampling_rate=8000)
    if encoder != "h2":
        assert e.range_fallbacks == 0 and e.range_flag(sampling_rate=8000)[0] == 0
        assert torch.isfinite(p).all()
        return
    assert e.range_fallbacks == 1
    e.arithmetic = "split"
    assert torch.equal(p, e.clips(a, sampling_rate=8000))
    e.encode(torch.from_numpy(a).cuda(), mode="h2", sampling_rate=8000)
    out = torch.empty((16, 6), dtype=torch.float32, device="cuda")
    e.recur(16, 6, out, mode="h2", sampling_rate=8000)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert e.range_flag(sampling_rate=8000)[0] & 1


def test_bad_arguments(engine):
    L = _lib.lib()
    c = _lib.SileroCfg()
    c.sample_rate = 22050
    ws = torch.empty(L.vadx_silero_workspace_bytes(1, 1), dtype=torch.uint8, device="cuda")
    x = torch.zeros((1, 288), device="cuda")
    s = torch.zeros((2, 1, 128), device="cuda")
    out, sn = torch.empty((1, 1), device="cuda"), torch.empty((2, 1, 128), device="cuda")
    args = (x.data_ptr(), s.data_ptr())
    assert L.vadx_silero_step(engine.packed_8k.data_ptr(), *args, 22050, 1, out.data_ptr(), sn.data_ptr(), ws.data_ptr(), ws.numel(),
                              _lib.stream_ptr(), ctypes.byref(c)) == -1
    c.sample_rate = 8000
    assert L.vadx_silero_step(engine.packed_8k.data_ptr(), *args, 16000, 1, out.data_ptr(), sn.data_ptr(), ws.data_ptr(), ws.numel(),
                              _lib.stream_ptr(), ctypes.byref(c)) == -1
    # an 8 kHz launch on the 16 kHz blob: NaN and flag bit 2
    engine.range_flag()
    c.arithmetic = _lib.ARITH["split"]
    _lib.check(L.vadx_silero_encode(engine.packed.data_ptr(), x.data_ptr(), 1, 256, 288, ws.data_ptr(), ws.numel(), _lib.stream_ptr(),
                                    ctypes.byref(c)))
    torch.cuda.synchronize()
    assert torch.isnan(ws.view(torch.float32)).all()
    flag, _ = engine.range_flag()
    assert flag & 4
    # stream_run's sampling_rate must equal the cfg's
    p = _lib.SileroIterParams()
    p.threshold, p.sampling_rate, p.min_silence_duration_ms, p.speech_pad_ms = 0.5, 16000, 100.0, 30.0
    c.arithmetic = 0
    rec = [torch.zeros(L.vadx_silero_stream_state_bytes(1), dtype=torch.uint8, device="cuda") for _ in range(2)]
    sw = torch.empty(L.vadx_silero_stream_workspace_bytes(1, 1), dtype=torch.uint8, device="cuda")
    kind = torch.empty((1, 1), dtype=torch.int8, device="cuda")
    val = torch.empty((1, 1), dtype=torch.float64, device="cuda")
    assert L.vadx_silero_stream_run(engine.packed_8k.data_ptr(), ctypes.byref(p), x.data_ptr(), 0, 1.0, 256, 1, 1, None, None,
                                    rec[0].data_ptr(), rec[1].data_ptr(), out.data_ptr(), kind.data_ptr(), val.data_ptr(), sw.data_ptr(),
                                    sw.numel(), _lib.stream_ptr(), ctypes.byref(c)) == -1


def test_onnx_file_serves_both_rates(tmp_path, encoder):
    """load_silero_vad(path=<.onnx with both branches>) runs the file's 8 kHz branch at sr = 8000 and its 16 kHz branch at 16000"""
    from test_silero8k_cpu import _two_branch
    w16, w8 = weights.silero_synthetic(1234), weights.silero8k_synthetic(1234)
    path = _two_branch(tmp_path / "silero_vad.onnx", w16, w8)
    model = silero.load_silero_vad(path=path)
    assert model.engine.has_8k
    ref_engine = silero.SileroEngine(w16, weights_8k=w8)
    a8 = _audio(1, 8000 * 6, seed=17)[0]
    got = silero.get_speech_timestamps(torch.from_numpy(a8), model, sampling_rate=8000)
    want = silero.get_speech_timestamps(torch.from_numpy(a8), ref_engine, sampling_rate=8000)
    assert got == want and len(got) > 0
    a16 = weights.burst_clips(1, 16000 * 4, seed=17).astype(np.float32)[0] * SCALE
    assert silero.get_speech_timestamps(torch.from_numpy(a16), model) == silero.get_speech_timestamps(torch.from_numpy(a16), ref_engine)
