"""GPU, through the engine: DFSMN clip pairs of any lengths as ONE ragged batch (DfsmnEngine.ragged / scores_ragged / flags_ragged /
detect(list)) and as live streams (DfsmnStreamBatch, stream_detect) -- both against the rectangular path the engine already had and against
the oracle's restatement of the reference driver; the near-end-only model, the two script-level drivers, and the launches each path issues.

One engine for the file (it also carries near-only constants: the two-channel path does not read them), one batch, one set of scores."""
import os
import wave

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, audio_io, dfsmn, drivers, weights
from oracle import dfsmn as od

pytestmark = pytest.mark.gpu

# near lengths: shorter than a window, exactly one, a second window that is nearly all padding, exactly two with no padding, a third;
# the far side differs by a few hundred samples either way (the one shorter far keeps its pair below a window: 1, 1, 2, 2, 3 windows)
NEAR_LEN = (300, 16001, 16002, 26882, 26883)
FAR_LEN = (100, 16301, 16202, 27282, 27033)
WINDOWS = (1, 1, 2, 2, 3)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.fixture(scope="module")
def eng():
    e = dfsmn.DfsmnEngine(weights.dfsmn_synthetic(1234))
    e.set_near_only_constants(*weights.dfsmn_near_only_constants(1234))
    return e


@pytest.fixture(scope="module")
def pairs():
    near = [weights.burst_clips(1, n, seed=21 + 2 * b)[0].astype(np.float32) for b, n in enumerate(NEAR_LEN)]
    far = [weights.burst_clips(1, n, seed=22 + 2 * b)[0].astype(np.float32) for b, n in enumerate(FAR_LEN)]
    rng = np.random.default_rng(5)
    return near, far, rng.standard_normal((5, 20000)), rng.standard_normal((5, 20000))


@pytest.fixture(scope="module")
def batch(eng, pairs):
    """(RaggedPairs on the device, its scores [9, 51]) -- computed once, read by every test below"""
    rp = eng.ragged(*pairs)
    assert tuple(rp.windows.tolist()) == WINDOWS
    return rp, eng.scores_ragged(rp)


def gap_threshold(scores, q):
    """The midpoint of the widest gap between neighbours of the sorted scores within +-10 ranks of the q quantile, and half that gap."""
    s = np.sort(np.asarray(scores, dtype=np.float64).reshape(-1))
    r = int(round(q * (len(s) - 1)))
    lo, hi = max(r - 10, 0), min(r + 10, len(s) - 1)
    gaps = s[lo + 1:hi + 1] - s[lo:hi]
    i = int(np.argmax(gaps))
    return float(0.5 * (s[lo + i] + s[lo + i + 1])), float(0.5 * gaps[i])


@pytest.fixture(scope="module")
def thresholds(batch):
    """(speaking, silence) inside the synthetic head's score range, so that both vote branches fire (most of its scores are saturated:
    0.5 / 0.5 alone would test little), each at least 2e-4 -- twice the suite's 1e-4 device-to-oracle score tolerance -- away from every
    score of the batch: a flag cannot flip on arithmetic, neither between the device paths nor against the oracle."""
    vad = batch[1].cpu().numpy()
    (hi, gap_hi), (lo, gap_lo) = gap_threshold(vad, 0.7), gap_threshold(vad, 0.3)
    print(f"thresholds: speaking {hi:.6f} (half-gap {gap_hi:.3g}), silence {lo:.6f} (half-gap {gap_lo:.3g})")
    assert gap_hi >= 2e-4 and gap_lo >= 2e-4, (gap_hi, gap_lo)
    return hi, lo


def test_scores_ragged_are_the_rectangular_scores(eng, batch):
    rp, vad = batch
    _, stride = eng.grid()
    assert vad.shape == (9, 51)
    rows_near, rows_far = [], []
    for b in range(len(rp)):
        pn, pf = rp.padded(b)
        first, W = int(rp.win_first_host[b]), int(rp.windows[b])
        ref = eng.run(pn[None, :], pf[None, :], W, stride)
        err = float((vad[first:first + W] - ref).abs().max())
        print(f"clip {b}: max |ragged - alone| = {err:.3g}")
        # the project's bound for different sub-batch cuts (tests/test_gpu_dfsmn.py: the summation order of the fused LayerNorm statistics)
        torch.testing.assert_close(vad[first:first + W], ref, rtol=0, atol=2e-6)
        rows_near += [pn[k * stride:k * stride + eng.L] for k in range(W)]
        rows_far += [pf[k * stride:k * stride + eng.L] for k in range(W)]
    assert torch.equal(vad, eng.run(np.stack(rows_near), np.stack(rows_far), 1))      # the same rows stacked rectangular: bitwise


def test_flags_ragged_are_the_rectangular_vote_per_clip(eng, batch, thresholds):
    rp, vad = batch
    hi, lo = thresholds
    lb, _ = eng.grid()
    flags, nflags = eng.flags_ragged(rp, hi, lo, vad=vad)
    got = flags.cpu().numpy()
    assert nflags.tolist() == [w * (51 - lb) + lb for w in WINDOWS]
    for b in range(len(rp)):
        first, W = int(rp.win_first_host[b]), int(rp.windows[b])
        one = torch.empty((1, int(nflags[b])), dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib().vadx_dfsmn_vote(vad[first:first + W].data_ptr(), 1, W, 51, lb, hi, lo, one.data_ptr(), _lib.stream_ptr()))
        assert np.array_equal(got[b, :nflags[b]], one.cpu().numpy()[0]) and (got[b, nflags[b]:] == 255).all(), b


def test_detect_of_a_list_and_stream_detect_agree_and_match_the_oracle_driver(eng, pairs, batch, thresholds):
    near, far, nz_near, nz_far = pairs
    rp, vad = batch
    hi, lo = thresholds
    flags, nflags = eng.flags_ragged(rp, hi, lo, vad=vad)
    fl = flags.cpu().numpy()
    saved = [fl[b, :nflags[b]] for b in range(len(rp))]
    assert {0, 1} == set(np.concatenate(saved).tolist())                  # both states occur: both vote branches fired
    w = {k: T(v) for k, v in weights.dfsmn_synthetic(1234).items()}
    w["mask.shift"] = w["mask.shift"] + torch.log(torch.tensor(32768 ** 2, dtype=torch.float32))
    fe = od.Frontend()
    oracle = [od.run_clip(fe, w, near[b], far[b], nz_near[b], nz_far[b], weights.DFSMN_MASK["layers"], speaking=hi, silence_score=lo)
              for b in range(len(rp))]
    for b, (_, osaved) in enumerate(oracle):
        assert np.array_equal(saved[b].astype(bool), np.array(osaved, dtype=bool)), b
    want = [ts for ts, _ in oracle]
    assert eng.detect(list(near), list(far), nz_near, nz_far, speaking_score=hi, silence_score=lo) == want
    host = eng.ragged(near, far, nz_near, nz_far, device=None)
    for k in (1, 2):
        streamed = eng.stream_flags(host, k, hi, lo)                      # DfsmnStreamBatch.step, tick by tick
        for b in range(len(rp)):
            assert np.array_equal(streamed[b], saved[b]), (k, b)
        assert eng.stream_detect(near, far, nz_near, nz_far, windows_per_tick=k, speaking_score=hi, silence_score=lo) == want, k


def test_near_only_list_equals_each_clip_alone(eng, pairs, monkeypatch):
    near, _, nz_near, _ = pairs
    got = eng.detect(list(near), None, nz_near, None)
    alone = [eng.detect(near[b][None, :], None, nz_near[b][None, :], None)[0] for b in range(len(near))]
    assert got == alone
    assert eng.stream_detect(list(near), None, nz_near, None, windows_per_tick=2) == alone
    monkeypatch.delattr(eng, "pow_far")                                  # an engine without the export's baked constants
    with pytest.raises(ValueError):
        dfsmn.DfsmnStreamBatch(eng, 2, near_only=True)


def test_drivers_take_a_list_of_files_as_one_ragged_batch(eng, tmp_path):
    """The reference's example pair and a cut of it, as a list through both drivers: what the two single-file calls return, `.k` files
    written."""
    near_p, far_p = os.path.join(GOLD, "dfsmn_nearend_mic.wav"), os.path.join(GOLD, "dfsmn_farend_speech.wav")
    cut = []
    for name, src, n in (("near_cut.wav", near_p, 30000), ("far_cut.wav", far_p, 30400)):
        pth = str(tmp_path / name)
        with wave.open(pth, "wb") as wv:
            wv.setnchannels(1); wv.setsampwidth(2); wv.setframerate(16000); wv.writeframes(audio_io.load_wav(src)[:n].tobytes())
        cut.append(pth)
    rng = np.random.default_rng(8)
    nz1, nz2 = rng.standard_normal((2, 20000)), rng.standard_normal((2, 20000))
    quiet = lambda *_: None                                                     # noqa: E731
    sec, idx = str(tmp_path / "s.txt"), str(tmp_path / "i.txt")
    many = drivers.inference_dfsmn([near_p, cut[0]], [far_p, cut[1]], eng, sec, idx, pad_noise_near=nz1, pad_noise_far=nz2, echo=quiet)
    assert len(many) == 2 and all(os.path.exists(f"{p}.{k}") for p in (sec, idx) for k in (0, 1))
    for k, (pn, pf) in enumerate(((near_p, far_p), cut)):
        one = drivers.inference_dfsmn(pn, pf, eng, str(tmp_path / "s1.txt"), str(tmp_path / "i1.txt"), pad_noise_near=nz1[k:k + 1],
                                      pad_noise_far=nz2[k:k + 1], echo=quiet)
        assert many[k] == one, k
        assert open(f"{idx}.{k}").read() == open(str(tmp_path / "i1.txt")).read()
    many = drivers.inference_dfsmn_near_only([near_p, cut[0]], eng, sec + "n", idx + "n", pad_noise=nz1, echo=quiet)
    assert len(many) == 2 and all(os.path.exists(f"{p}n.{k}") for p in (sec, idx) for k in (0, 1))
    for k, pn in enumerate((near_p, cut[0])):
        assert many[k] == drivers.inference_dfsmn_near_only(pn, eng, str(tmp_path / "s1.txt"), str(tmp_path / "i1.txt"), pad_noise=nz1[k:k + 1],
                                                            echo=quiet), k


# what `detect` of a [2, 24 000] array pair (two windows per clip, one sub-batch) issued at the commit before the ragged path existed
PARENT_DETECT_CALLS = {
    "vadx_frontend_stft_ft": 2, "vadx_dfsmn_alpha_scale": 1, "vadx_dfsmn_ft_repack": 2, "vadx_dfsmn_lstm_f": 11, "vadx_dfsmn_pw_conv": 3,
    "vadx_dfsmn_stats_merge": 10, "vadx_dfsmn_frame_stats": 1, "vadx_dfsmn_cfb_front": 10, "vadx_dfsmn_cfb_back": 10,
    "vadx_dfsmn_lstm_t_ex": 2, "vadx_dfsmn_istft": 1, "vadx_frontend_logmel_ex": 3, "vadx_dfsmn_mask_net": 1, "vadx_dfsmn_vote": 1}


def test_launches(eng, pairs, batch, monkeypatch):
    near, far, nz_near, nz_far = pairs
    rp, _ = batch
    rect_n, rect_f = weights.burst_clips(2, 24000, seed=3), weights.burst_clips(2, 24000, seed=4)
    with _lib.trace() as tr:
        eng.detect(rect_n, rect_f, nz_near[:2], nz_far[:2])
    assert tr.calls == PARENT_DETECT_CALLS                               # the array form goes the way it always went
    rows = torch.zeros((9, eng.L), dtype=torch.int16, device="cuda")
    with _lib.trace() as net:
        eng.run(rows, rows, 1)
    with _lib.trace() as tr:
        eng.detect(list(near), list(far), nz_near, nz_far)
    assert tr.calls == dict(net.calls, vadx_windows_gather_any=2, vadx_dfsmn_vote_ragged=1) and "vadx_dfsmn_vote" not in tr.calls
    # a stream tick with one of three streams inactive hands the network 2 * k rows
    seen = []
    run = eng.run
    monkeypatch.setattr(eng, "run", lambda a, b, w: seen.append((tuple(a.shape), tuple(b.shape), w)) or run(a, b, w))
    sb = dfsmn.DfsmnStreamBatch(eng, 3)
    k = 2
    n = int(sb.samples_needed(k).max())
    smp = weights.burst_clips(3, n, seed=9)
    with _lib.trace() as tr:
        flags, tail = sb.step(smp, smp, k, active=[True, False, True])
    assert seen == [((2 * k, eng.L), (2 * k, eng.L), 1)]
    assert tr.calls == dict(net.calls, vadx_dfsmn_stream_windows=1, vadx_dfsmn_stream_vote=1)
    assert (flags[1] == 255).all() and (tail[1] == 255).all() and sb.windows_done.tolist() == [k, 0, k]
