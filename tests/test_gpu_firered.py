"""GPU parity: FireRed DetectModel + device VadPostprocessor vs reference fixtures / oracle."""
import numpy as np
import pytest
from conftest import chain_or_threshold
import torch

import vadx  # noqa: F401
from vadx import firered, vadpost, weights
from oracle import firered as ofr
from oracle import postproc as opp

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["f32", "split", "h2"])
def gemm(request):
    """Every test of this file runs on both arithmetics of the point-wise pairs: exact-f32 MFMAs, bf16 x 3 split products and fp16 x 2 split products (the default)."""
    from vadx import _lib
    prev = _lib.gemm_mode(request.param)
    yield request.param
    _lib.gemm_mode(prev)
ATOL = 1e-4
LOGIT_ATOL = 4e-4          # ATOL restated at the sigmoid's steepest point (1e-4 / 0.25): not a new tolerance
CFGS = {1234: weights.FIRERED_CFG, 7: dict(weights.FIRERED_CFG, R=3, M=2, H=64, P=32, N1=8, S1=2, N2=4, S2=3),
        9: dict(weights.FIRERED_CFG, R=2, M=1, H=48, P=24, N1=5, S1=1, N2=0, S2=0, odim=3)}


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def assert_logits_close(got, want):
    """The fixture comparison in logit space, over every value where the fixture has 0 < p < 1 - 1e-3 (above that float32 resolves 1 - p too
    coarsely).  The seed-7 fixtures hold probabilities of 4e-9 .. 7e-6 only: against ATOL a kernel that returned zeros would pass."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    m = (want > 0) & (want < 1 - 1e-3)
    assert m.any()
    with np.errstate(divide="ignore"):
        np.testing.assert_allclose(np.log(got[m]) - np.log1p(-got[m]), np.log(want[m]) - np.log1p(-want[m]), rtol=0, atol=LOGIT_ATOL)


@pytest.mark.parametrize("seed", [1234, 7, 9])
def test_session_matches_reference_fixture(golden, seed):
    """The reference's own validate_export input (randint(-8000,8000), seed 1234) and two other
    architectures (dilated taps, no look-ahead, 3 output heads = AED)."""
    g = golden("firered_forward")
    sess = firered.FireRedSession(weights.firered_synthetic(seed, CFGS[seed]))
    assert sess.get_inputs()[0].name == "audio" and sess._inputs_meta[0].shape[-1] == 16000
    probs = sess.run([sess.get_outputs()[0].name], {"audio": g[f"s{seed}_audio"]})[0]
    assert probs.shape == g[f"s{seed}_probs"].shape
    np.testing.assert_allclose(probs, g[f"s{seed}_probs"], rtol=0, atol=ATOL)
    assert_logits_close(probs, g[f"s{seed}_probs"])
    with pytest.raises(ValueError):
        sess.run(None, {"audio": g[f"s{seed}_audio"].astype(np.float32)})


@pytest.mark.parametrize("a,b", [("fc1", "fc2_w"), ("blk1_fc1", "blk1_fc2_w"), ("blk7_fc1", "blk7_fc2_w"), ("dnn0", "out_w")])
@pytest.mark.parametrize("shift", [14, -12])
def test_rescaled_network_and_lsb_audio(gemm, a, b, shift):
    """layer a (weights and bias) x 2^-shift and the layer behind its ReLU x 2^shift is the same network; pack_host
    rebalances the pair by exact powers of two (csrc/rebalance.h).  float32 MFMAs and bf16 x 3 return the original network's
    probabilities bit for bit, fp16 x 2 to 2e-6, on silence, 1 - 3 LSB noise, an LSB-level tone and ordinary bursts; all within the
    oracle's tolerance."""
    w0 = weights.firered_synthetic(1234)
    w1 = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in w0.items()}
    w1[a + "_w"] = w1[a + "_w"] * np.float32(2.0 ** -shift)
    w1[a + "_b"] = w1[a + "_b"] * np.float32(2.0 ** -shift)
    w1[b] = w1[b] * np.float32(2.0 ** shift)
    rng = np.random.default_rng(31)
    clips = weights.burst_clips(6, 16000, seed=79)
    clips[0] = 0
    clips[1] = rng.integers(-1, 2, 16000)
    clips[2] = rng.integers(-3, 4, 16000)
    clips[3] = np.round(2.4 * np.sin(2 * np.pi * 440.0 / 16000 * np.arange(16000)))
    clips = clips.astype(np.int16)
    e0, e1 = firered.FireRedEngine(w0), firered.FireRedEngine(w1)
    p0, p1 = e0.run(T(clips).cuda(), 1), e1.run(T(clips).cuda(), 1)
    assert e1.blobs.mode() == gemm and e1.blobs.range_fallbacks == 0
    if gemm in ("f32", "split"):
        assert torch.equal(p0, p1)
    else:
        assert float((p0 - p1).abs().max()) <= 2e-6
    fe = ofr.Frontend()
    want = ofr.forward(fe, {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in w0.items()}, T(clips).unsqueeze(1))
    np.testing.assert_allclose(p1.cpu().numpy().reshape(want.shape), want.numpy(), rtol=0, atol=ATOL)


def test_vadpostprocessor_matches_reference(golden):
    g = golden("vadpost")
    n_cases = int(g["n_cases"])
    for c, cfg in enumerate(g["cfgs_f"]):
        pp = vadpost.VadPostprocessor(int(cfg[0]), float(cfg[1]), *[int(v) for v in cfg[2:7]])
        for i in range(n_cases):
            dec = pp.process(g[f"probs_{i}"])
            assert np.array_equal(dec, g[f"f{c}_dec_{i}"]), (c, i)
            wav = float(g[f"f{c}_wav_{i}"])
            seg = pp.decision_to_segment(dec, None if wav < 0 else wav)
            assert np.array_equal(np.array(seg, dtype=np.float64).reshape(-1, 2), g[f"f{c}_seg_{i}"]), (c, i)
    for c, cfg in enumerate(g["cfgs_m"]):
        pp = vadpost.VadPostprocessor(int(cfg[0]), float(cfg[1]), *[int(v) for v in cfg[2:7]],
                                      frame_shift_s=float(cfg[7]), frame_length_s=None)
        for i in range(n_cases):
            dec = pp.process(g[f"probs_{i}"])
            assert np.array_equal(dec, g[f"m{c}_dec_{i}"]), (c, i)
            wav = float(g[f"m{c}_wav_{i}"])
            seg = pp.decision_to_segment(dec, None if wav < 0 else wav)
            assert np.array_equal(np.array(seg, dtype=np.float64).reshape(-1, 2), g[f"m{c}_seg_{i}"]), (c, i)
    # ragged batch in one launch == the single-track results
    tracks = [g[f"probs_{i}"] for i in range(n_cases) if len(g[f"probs_{i}"])]
    S = max(len(p) for p in tracks)
    batch = np.zeros((len(tracks), S), np.float32)
    for k, p in enumerate(tracks):
        batch[k, :len(p)] = p
    pp = vadpost.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0)
    dec, segs, counts = pp.process_batch(batch, [len(p) for p in tracks], cap=1)
    for k, p in enumerate(tracks):
        want = opp.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0).process(p)
        assert np.array_equal(dec[k, :len(p)].cpu().numpy(), want), k


@pytest.mark.parametrize("n", [160000, 89431, 5000, 300])
def test_whole_clip_segments(n):
    eng = firered.FireRedEngine(weights.firered_synthetic(1234))
    fe = ofr.Frontend()
    ow = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in weights.firered_synthetic(1234).items()}
    B = 3
    clips = weights.burst_clips(B, n, seed=n)
    noise = np.random.default_rng(4).standard_normal((B, 20000))
    got, track, dec = eng.detect(clips, pad_noise=noise, return_probs=True) if firered.valid_frame_count(n) else (eng.detect(clips, pad_noise=noise), None, None)
    full_chain = 0
    for b in range(B):
        want_seg, want_p, want_dec = ofr.run_clip(fe, ow, clips[b], noise[b])
        if track is not None:
            np.testing.assert_allclose(track[b].cpu().numpy(), want_p, rtol=0, atol=ATOL)
            # decisions bit-exact when the device scores are post-processed by the oracle too
            d2 = opp.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0).process(track[b].cpu().numpy())
            assert np.array_equal(dec[b].cpu().numpy(), d2)
            assert got[b] == opp.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0).decision_to_segment(d2, n / 16000)
            if chain_or_threshold(opp.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0), track[b].cpu().numpy(), want_p, d2, want_dec, got[b], want_seg):
                full_chain += 1
                assert [(int(s * 16000), int(e * 16000)) for s, e in got[b]] == [(int(s * 16000), int(e * 16000)) for s, e in want_seg]
        else:
            assert got[b] == want_seg == []
    assert track is None or full_chain >= 1          # of three clips at least one took the whole chain (a clip may sit on a threshold)


def test_full_size_config5_properties():
    """BASELINE config 5 (FireRed half): B=2048 x 10 s -- batch-position invariance + oracle spot check."""
    import time
    eng = firered.FireRedEngine(weights.firered_synthetic(1234))
    base = weights.burst_clips(32, 160000, seed=321)
    big = np.tile(base, (64, 1))                                   # 2048 clips
    t0 = time.perf_counter()
    got, track, dec = eng.detect(big, return_probs=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert track.shape == (2048, 980)
    tr = track.view(64, 32, -1)
    assert torch.equal(tr[0], tr[41]) and torch.equal(tr[0], tr[63])
    assert got[5] == got[32 * 7 + 5]
    fe = ofr.Frontend()
    ow = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in weights.firered_synthetic(1234).items()}
    want_seg, want_p, want_dec = ofr.run_clip(fe, ow, base[5], np.zeros(10))
    np.testing.assert_allclose(track[5].cpu().numpy(), want_p, rtol=0, atol=ATOL)
    print(f"FireRed config-5 pass (incl. host pad/upload): {dt * 1e3:.1f} ms for 2048 x 10 s")


_ORACLE_C5 = {}


def test_config5_scores_and_segments_against_the_oracle(gemm):
    """BASELINE config 5 (FireRed half) on the bench's OWN batch (bench_models.synth_pcm16, seed 1505: 2048 unique 10 s clips): 64 clips spread
    over the batch against oracle.firered.run_clip on the same int16 samples -- scores within 1e-4, segment lists equal unless a smoothed
    frame sits on the threshold (conftest.chain_or_threshold).  Three arithmetics."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench_models as bm
    w = weights.firered_synthetic(1234)
    eng = firered.FireRedEngine(w)
    audio = bm.synth_pcm16(torch, torch.device("cuda:0"), 2048, 160000, seed=1505).cpu().numpy()
    got, track, dec = eng.detect(audio, return_probs=True)
    assert eng.blobs.mode() == gemm and eng.blobs.range_fallbacks == 0
    idx = [int(k * 32 + (k * 5) % 32) for k in range(64)]
    if "ref" not in _ORACLE_C5:
        fe = ofr.Frontend()
        ow = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _ORACLE_C5["ref"] = [ofr.run_clip(fe, ow, audio[b], np.zeros(10)) for b in idx]
    full = 0
    for b, (want_seg, want_p, want_dec) in zip(idx, _ORACLE_C5["ref"]):
        tr = track[b].cpu().numpy()
        assert tr.shape[0] == want_p.shape[0]
        np.testing.assert_allclose(tr, want_p, rtol=0, atol=ATOL)
        d2 = opp.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0).process(tr)          # the oracle's post-processor on the DEVICE scores
        assert np.array_equal(dec[b].cpu().numpy(), d2)
        if chain_or_threshold(opp.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0), tr, want_p, d2, want_dec, got[b], want_seg):
            full += 1
            assert [(int(s * 16000), int(e * 16000)) for s, e in got[b]] == [(int(s * 16000), int(e * 16000)) for s, e in want_seg]
    assert full >= len(idx) - 2, full


# ------------------------------------------------------------------ Stream-VAD (cache-carrying chunk kernel)
STREAM_CFGS = {1234: dict(weights.FIRERED_CFG, N2=0, S2=0),
               7: dict(weights.FIRERED_CFG, R=3, M=2, H=64, P=32, N1=8, S1=2, N2=0, S2=0)}


@pytest.mark.parametrize("seed", [1234, 7])
def test_stream_session_matches_reference_fixture(golden, seed):
    """The reference's chunk loop (2560-sample chunks, caches fed back, short tail zero-padded) through the
    session boundary, against probabilities / caches produced by the reference modules."""
    g = golden("firered_stream")
    cfg = STREAM_CFGS[seed]
    sess = firered.FireRedStreamSession(weights.firered_synthetic(seed, cfg))
    names = [m.name for m in sess.get_inputs()], [m.name for m in sess.get_outputs()]
    assert names == (["audio", "caches_in"], ["probs", "caches_out"])
    clip = g[f"s{seed}_clip"]
    n = len(clip)
    caches = np.zeros(sess._inputs_meta[1].shape, np.float32)
    probs, pos = [], 0
    while pos < n:
        end = min(pos + 2560, n)
        chunk = clip[pos:end]
        if len(chunk) < 400:
            chunk = np.pad(chunk, (0, 400 - len(chunk)), mode="constant")
        pr, caches = sess.run(["probs", "caches_out"], {"audio": chunk.reshape(1, 1, -1), "caches_in": caches})
        if pos == 0:
            np.testing.assert_allclose(caches, g[f"s{seed}_caches_first"], rtol=0, atol=1e-3)
        probs.append(pr[0, 0])
        pos = end
    got = np.concatenate(probs)
    assert got.shape == g[f"s{seed}_probs"].shape
    np.testing.assert_allclose(got, g[f"s{seed}_probs"], rtol=0, atol=ATOL)
    assert_logits_close(got, g[f"s{seed}_probs"])
    np.testing.assert_allclose(caches, g[f"s{seed}_caches_last"], rtol=0, atol=1e-3)
    with pytest.raises(ValueError):
        sess.run(None, {"audio": clip[:2560].reshape(1, 1, -1), "caches_in": caches[:, :, :, :-1]})
    with pytest.raises(ValueError):
        sess.run(None, {"audio": clip[:300].reshape(1, 1, -1), "caches_in": caches})


def test_stream_detect_batch_vs_oracle():
    """Many streams advance together, one chunk per launch: probabilities within 1e-4 of the oracle loop run
    clip by clip, identical segments, and every stream independent of its neighbours."""
    cfg = STREAM_CFGS[1234]
    wts = weights.firered_synthetic(1234, cfg)
    eng = firered.FireRedEngine(wts, firered.STREAM_CHUNK_SAMPLES)
    n = 3 * 16000 + 777
    clips = weights.burst_clips(5, n, seed=31)
    post = (5, 0.3, 5, 8, 2000, 20)      # the look-back-only synthetic net sits lower than the calibrated one
    segs, track = eng.stream_detect(clips, post=post, return_probs=True)
    fe = ofr.Frontend()
    wt = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in wts.items()}
    for b in range(clips.shape[0]):
        oseg, oprobs = ofr.run_clip_stream(fe, wt, clips[b], post=post)
        assert track[b].shape == oprobs.shape
        np.testing.assert_allclose(track[b], oprobs, rtol=0, atol=ATOL)
        csum = np.concatenate([[0.0], np.cumsum(oprobs, dtype=np.float64)])
        k = np.arange(1, len(oprobs) + 1)
        smooth = (csum[k] - csum[np.maximum(k - 5, 0)]) / np.minimum(k, 5)
        if np.min(np.abs(smooth - 0.3)) > 1e-3:          # no smoothed frame within tolerance of the threshold
            assert segs[b] == oseg, b
    solo, solo_track = eng.stream_detect(clips[2:3], post=post, return_probs=True)
    assert np.array_equal(solo_track[0], track[2]) and solo[0] == segs[2]
    assert any(len(s) for s in segs)


def test_device_stream_postprocessor_matches_reference_fixture(golden):
    """StreamVadPostprocessorBatch (vadx_stream_vadpost: one thread per stream, state in a device record) against the segments the
    REFERENCE class produced (fixture): whole tracks, tracks fed 14 frames at a time with the state carried, reset -- bit-exact."""
    from vadx import vadpost
    g = golden("firered_stream")
    for c, cfg in enumerate(g["post_cfgs"]):
        args = (int(cfg[0]), float(cfg[1]), *[int(v) for v in cfg[2:]])
        for i in range(int(g["post_n"])):
            p = g[f"post_probs_{i}"]
            if len(p) == 0:
                continue
            pp = vadpost.StreamVadPostprocessorBatch(*args, streams=1)
            seg = np.array(pp.process_batch(p[None, :])[0], dtype=np.float64).reshape(-1, 2)
            assert np.array_equal(seg, g[f"post{c}_seg_{i}"]), (c, i)
            pp.reset()
            pieces = [np.array(pp.process_batch(p[None, k:k + 14])[0], dtype=np.float64).reshape(-1, 2) for k in range(0, len(p), 14)]
            assert np.array_equal(np.concatenate(pieces), g[f"post{c}_chunked_{i}"]), (c, i)
            pp.reset()
            again = np.array(pp.process_batch(p[None, :])[0], dtype=np.float64).reshape(-1, 2)
            assert np.array_equal(again, g[f"post{c}_seg_{i}"]), (c, i)


@pytest.mark.parametrize("cfg", [(5, 0.4, 5, 8, 2000, 20), (3, 0.5, 2, 4, 60, 6), (1, 0.5, 0, 1, 25, 1), (16, 0.35, 20, 3, 40, 9)])
def test_device_stream_postprocessor_many_streams_equals_the_host_class(cfg):
    """300 streams in one launch per chunk (ragged chunk sizes), every stream identical to the host class fed the same chunks."""
    from vadx import vadpost
    rng = np.random.default_rng(sum(int(v * 10) for v in cfg))
    S, n = 300, 700
    tracks = rng.random((S, n), dtype=np.float32)
    tracks[1] = 0.0                                                # never speech
    tracks[2] = 0.99                                               # one segment, split at max_speech
    for s_ in range(3, S, 3):                                      # bursty tracks: long runs either side of the threshold
        edges = np.sort(rng.integers(0, n, 12))
        for a, b in zip(edges[::2], edges[1::2]):
            tracks[s_, a:b] = 0.6 + 0.4 * tracks[s_, a:b]
        tracks[s_] = np.where(tracks[s_] > 0.6, tracks[s_], 0.3 * tracks[s_]).astype(np.float32)
    tracks[4, 100:110] = np.float32(cfg[1])                        # frames exactly on the threshold
    dev = vadpost.StreamVadPostprocessorBatch(*cfg, streams=S)
    host = [vadpost.StreamVadPostprocessor(*cfg) for _ in range(S)]
    pos = 0
    for size in (1, 13, 160, 7, 256, 263):
        got = dev.process_batch(torch.from_numpy(tracks[:, pos:pos + size]).cuda())
        for s_ in range(S):
            assert got[s_] == host[s_].process_batch(tracks[s_, pos:pos + size].copy()), (s_, pos)
        pos += size
    assert pos == n and any(len(x) for x in got)


def test_whole_config_decision_record():
    """BASELINE config 5 (FireRed half) at full size: segment lists of the default arithmetic against float32 MFMAs + dense float32 front-end."""
    import decision_records
    r = decision_records.firered_c5(torch, torch.device("cuda", 0))
    print(r)
    assert r["compared"] == 2048 and r["unexcused"] == 0, r
