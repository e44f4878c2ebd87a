"""GPU, kernels alone on plain tensors (no network): vadx_windows_gather_any copies any window from any sample offset and nothing else, and
vadx_dfsmn_vote_ragged gives every clip of a ragged batch the flags of the reference loop -- bit for bit the oracle's, and vadx_dfsmn_vote's
on that clip's rows alone -- whatever its neighbours' window counts are, and survives a lying window table."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib
from oracle import dfsmn as od
from oracle import postproc as opp

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- gather ---------------------------------------------------------------------------------------------------------------------------
PCM_LEN, GUARD = 40001, 64


def _gather(pcm, src, wl):
    """-> (rows int16 [n, wl], guard int16 [GUARD]) of one vadx_windows_gather_any call into a buffer with a sentinel behind it"""
    n = len(src)
    buf = torch.full((n * wl + GUARD,), 0x5A5A, dtype=torch.int16, device="cuda")
    _lib.check(_lib.lib().vadx_windows_gather_any(pcm.data_ptr(), pcm.numel(), dev(np.asarray(src, dtype=np.int64)).data_ptr(), n, wl,
                                                  buf.data_ptr(), _lib.stream_ptr()))
    out = buf.cpu().numpy()
    return out[:n * wl].reshape(n, wl), out[n * wl:]


def _want(pcm, src, wl):
    rows = np.zeros((len(src), wl), dtype=np.int16)
    for w, s in enumerate(src):
        if 0 <= s and s + wl <= len(pcm):
            rows[w] = pcm[s:s + wl]
    return rows


@pytest.mark.parametrize("wl", [1, 7, 8, 16001])
def test_gather_any_copies_every_window_and_nothing_else(wl):
    rng = np.random.default_rng(wl)
    pcm = rng.integers(-32768, 32768, PCM_LEN).astype(np.int16)
    pcm[pcm == 0] = 1                                                    # a zero row is then a refused window, not audio
    pcm_d = dev(pcm)
    last = PCM_LEN - wl                                                   # the window that ends exactly at pcm_len
    special = [0, 1, 2, 10881, 10882, last, last + 1, -1, -2, PCM_LEN, PCM_LEN + 5]      # odd and even, the edge, past it, negative
    src = special + rng.integers(0, last + 1, 300 - len(special)).tolist()
    rows, guard = _gather(pcm_d, src, wl)
    assert np.array_equal(rows, _want(pcm, src, wl))
    assert (rows[[5]] != 0).all() and not rows[[6, 7, 8, 9, 10]].any()  # the edge window is audio, its neighbours are zeros
    assert (guard == 0x5A5A).all()
    for s in special:                                                     # n_windows = 1
        rows, guard = _gather(pcm_d, [s], wl)
        assert np.array_equal(rows, _want(pcm, [s], wl)) and (guard == 0x5A5A).all(), s


def test_gather_any_with_a_window_longer_than_the_audio_writes_zeros():
    pcm = dev(np.arange(1, 101, dtype=np.int16))
    rows, guard = _gather(pcm, [0, 3], 101)
    assert not rows.any() and (guard == 0x5A5A).all()


# ---- ragged vote ----------------------------------------------------------------------------------------------------------------------
def oracle_saved(scores, lb, spk, sil):
    """The reference loop (Inference_DFSMN_VAD_ONNX.py:231-273) over one clip's scores [W, frames] -> its `saved` list as uint8"""
    frames, silence, saved = scores.shape[1], True, []
    for w in range(scores.shape[0]):
        f, silence = opp.lookahead_vote(scores[w], frames - lb, lb, spk, sil, silence, thresholds=(spk, sil))
        saved += f
    saved += od.tail_flags(scores[-1], frames - lb, frames, silence, spk, sil)[0]
    return np.array(saved, dtype=np.uint8)


def vote_ragged(scores_d, win_first, n_windows, max_windows, frames, lb, spk, sil, pad=3):
    B = len(win_first) - 1
    stride = max_windows * (frames - lb) + lb + pad                      # a stride wider than needed: the slack must read 255 too
    flags = torch.zeros((B, stride), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vadx_dfsmn_vote_ragged(scores_d.data_ptr(), B, n_windows, max_windows, dev(np.asarray(win_first, dtype=np.int32)).data_ptr(),
                                                 frames, lb, float(spk), float(sil), flags.data_ptr(), stride, _lib.stream_ptr()))
    return flags.cpu().numpy()


def vote_alone(rows_d, frames, lb, spk, sil):
    W = rows_d.shape[0]
    flags = torch.empty((1, W * (frames - lb) + lb), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vadx_dfsmn_vote(rows_d.data_ptr(), 1, W, frames, lb, float(spk), float(sil), flags.data_ptr(), _lib.stream_ptr()))
    return flags


def scores_on_thresholds(rng, shape, spk, sil):
    """random float32 scores, about a tenth of them exactly float32(threshold)"""
    s = rng.random(shape, dtype=np.float32)
    pick = rng.random(shape)
    s[pick < 0.05], s[pick > 0.95] = np.float32(spk), np.float32(sil)
    return s


@pytest.mark.parametrize("batch", [1, 65])           # 65: the second 64-lane workgroup has one live lane
@pytest.mark.parametrize("frames,lb", [(51, 15), (4, 1), (4, 3)])
def test_vote_ragged_is_the_oracle_loop_and_the_rectangular_vote_per_clip(golden, frames, lb, batch):
    rng = np.random.default_rng(100 * frames + 10 * lb + batch)
    for spk, sil in golden("hostloop_thresholds")["pairs"]:
        for W in ([np.array([1]), np.array([5])] if batch == 1 else [np.concatenate([[1, 5], rng.integers(1, 6, batch - 2)])]):
            win_first = np.concatenate([[0], np.cumsum(W)])
            n, mw = int(win_first[-1]), int(W.max())
            scores = scores_on_thresholds(rng, (n, frames), spk, sil)
            sd = dev(scores)
            got = vote_ragged(sd, win_first, n, mw, frames, lb, spk, sil)
            alone = [vote_alone(sd[win_first[b]:win_first[b + 1]], frames, lb, spk, sil) for b in range(batch)]
            for b in range(batch):
                nf = int(W[b]) * (frames - lb) + lb
                want = oracle_saved(scores[win_first[b]:win_first[b + 1]], lb, float(spk), float(sil))
                assert np.array_equal(got[b, :nf], want), (spk, sil, b)
                assert np.array_equal(got[b, :nf], alone[b].cpu().numpy()[0]), (spk, sil, b)
                assert (got[b, nf:] == 255).all(), (spk, sil, b)


def test_vote_ragged_replays_the_reference_loop_on_prefixes_of_its_scores(golden):
    """The scores the REFERENCE loop was run on, as three clips of 6, 4 and 1 windows in one batch: the whole one is the fixture's `saved`
    list, every prefix of whole windows the oracle loop on that prefix."""
    g = golden("hostloop_thresholds")
    for c, (spk, sil) in enumerate(g["pairs"]):
        scores = g[f"dfsmn_scores_{c}"]
        W = [scores.shape[0], 4, 1]
        rows = np.concatenate([scores[:w] for w in W])
        win_first = np.concatenate([[0], np.cumsum(W)])
        got = vote_ragged(dev(rows), win_first, len(rows), max(W), 51, 15, spk, sil)
        assert np.array_equal(got[0, :W[0] * 36 + 15].astype(bool), g[f"dfsmn_saved_{c}"]), c
        for b, w in enumerate(W):
            assert np.array_equal(got[b, :w * 36 + 15], oracle_saved(scores[:w], 15, float(spk), float(sil))), (c, b)
            assert (got[b, w * 36 + 15:] == 255).all()


@pytest.mark.parametrize("table,n_windows,liar", [
    ([0, 2, 2, 4, 5], 8, 1),          # W_1 = 0
    ([0, 2, 6, 7, 8], 8, 1),          # W_1 = 4 > max_windows
    ([-1, 2, 4, 6, 8], 8, 0),         # win_first[0] < 0
    ([0, 2, 4, 6, 9], 8, 3),          # win_first[B] > n_windows: the score tensor ends after row 7
])
def test_vote_ragged_with_a_lying_table_entry_leaves_that_row_255_and_its_neighbours_right(table, n_windows, liar):
    frames, lb, mw, spk, sil = 51, 15, 3, 0.7, 0.3
    scores = scores_on_thresholds(np.random.default_rng(liar + n_windows), (n_windows, frames), spk, sil)
    got = vote_ragged(dev(scores), table, n_windows, mw, frames, lb, spk, sil)
    for b in range(4):
        first, last = table[b], table[b + 1]
        if b == liar:
            assert first < 0 or last > n_windows or not 0 < last - first <= mw
            assert (got[b] == 255).all()
        else:
            nf = (last - first) * (frames - lb) + lb
            assert np.array_equal(got[b, :nf], oracle_saved(scores[first:last], lb, spk, sil)) and (got[b, nf:] == 255).all(), b
