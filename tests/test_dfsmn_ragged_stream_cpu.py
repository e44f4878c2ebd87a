"""CPU: DFSMN's ragged-batch and live-stream entry points (vadx_windows_gather_any, vadx_dfsmn_vote_ragged, vadx_dfsmn_stream_state_bytes,
vadx_dfsmn_stream_windows, vadx_dfsmn_stream_vote) exist under the unchanged ABI number, size the stream record as documented and refuse bad
arguments on the host before any device call; vadx.ragged.RaggedPairs packs near / far pairs of any lengths exactly as `detect` prepares
each pair alone; and the two host restatements the GPU tests lean on hold: the timeline rule (carry ++ new samples -> windows, new carry)
cuts a clip that arrives in pieces into the windows of the whole-clip grid, and the oracle's vote chained over ticks is the reference's
`saved` list."""
import ctypes as C
import re

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, clips, ragged, timestamps
from vadx.dfsmn import SHDR_WORDS
from oracle import dfsmn as od
from oracle import postproc as opp

L, T, FRAME, LB = 16001, 51, 320, 15
CARRY = (LB + 1) * FRAME                 # 5 120 samples two consecutive windows share
STRIDE = L - CARRY                       # 10 881
NAMES = ("vadx_windows_gather_any", "vadx_dfsmn_vote_ragged", "vadx_dfsmn_stream_state_bytes", "vadx_dfsmn_stream_windows",
         "vadx_dfsmn_stream_vote")
# near lengths: shorter than a window, exactly one, a second window that is nearly all padding, exactly two with no padding, a third;
# the far side differs by a few hundred samples either way (the one shorter far keeps its pair below a window: 1, 1, 2, 2, 3 windows)
NEAR_LEN = (300, 16001, 16002, 26882, 26883)
FAR_LEN = (100, 16301, 16202, 27282, 27033)
WINDOWS = (1, 1, 2, 2, 3)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_signatures_and_abi(lib):
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    assert lib.vadx_abi_version() == 10 == _lib.ABI_VERSION
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert len(re.findall(r"\b%s\b" % name, text)) >= 2, name        # declared, and recorded in the ABI history comment
        decl = re.search(r"^(?:int|size_t)\s+%s\(([^;]*)\);" % name, text, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name   # one ctypes argument per declared parameter


@pytest.mark.parametrize("channels", [1, 2])
def test_state_bytes(lib, channels):
    one = lib.vadx_dfsmn_stream_state_bytes(1, L, LB, channels)
    assert one == SHDR_WORDS * 4 + channels * CARRY * 2                  # the header DfsmnStreamBatch reads, then the carries
    for S in (1, 3, 64, 4097):
        n = lib.vadx_dfsmn_stream_state_bytes(S, L, LB, channels)
        assert n % 16 == 0 and n == S * one                              # aligned, linear in S
        assert n >= S * channels * CARRY * 2                             # the carry of every channel fits
    bytes_ = lib.vadx_dfsmn_stream_state_bytes
    assert bytes_(0, L, LB, channels) == 0 and bytes_(-1, L, LB, channels) == 0
    assert bytes_(4, L, 0, channels) == 0 and bytes_(4, L, -1, channels) == 0
    assert bytes_(4, 0, LB, channels) == 0 and bytes_(4, CARRY, LB, channels) == 0       # no stride left
    assert bytes_(4, CARRY + 1, LB, channels) > 0
    assert bytes_(4, L, LB, 0) == 0 and bytes_(4, L, LB, 3) == 0


def test_bad_arguments_are_refused_on_the_host(lib):
    """Every refusal the header lists comes back as VADX_EINVAL with the function's and the argument's name in vadx_last_error() -- before
    any HIP call (there is no device here; the pointers below are host memory nothing may touch)."""
    nb = lib.vadx_dfsmn_stream_state_bytes(2, L, LB, 2)
    buf = (C.c_char * (2 * nb + 64))()
    ptr = (C.addressof(buf) + 15) & ~15
    rec_a, rec_b = ptr, ptr + nb
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731

    def refused(call, name, **bad):
        return call(**bad) == -1 and name in err() and all(k.encode() in err() for k in bad)

    gather = lambda **kw: lib.vadx_windows_gather_any(*[kw.get(k, v) for k, v in (                                     # noqa: E731
        ("pcm", ptr), ("pcm_len", 16001), ("win_src", ptr), ("n_windows", 1), ("window_len", L), ("window_buf", ptr), ("stream", None))])
    for k in ("pcm", "win_src", "window_buf"):
        assert refused(gather, b"vadx_windows_gather_any", **{k: None}) and b"NULL" in err(), k
    for k, bad in (("n_windows", 0), ("n_windows", -3), ("pcm_len", 0), ("pcm_len", -1), ("window_len", 0), ("window_len", -8)):
        assert refused(gather, b"vadx_windows_gather_any", **{k: bad}), (k, bad)

    slide = T - LB
    vote = lambda **kw: lib.vadx_dfsmn_vote_ragged(*[kw.get(k, v) for k, v in (                                        # noqa: E731
        ("vad", ptr), ("batch", 2), ("n_windows", 5), ("max_windows", 4), ("win_first", ptr), ("frames", T), ("look_backward", LB),
        ("speaking", 0.5), ("silence", 0.5), ("flags", ptr), ("flag_stride", 4 * slide + LB), ("stream", None))])
    for k in ("vad", "win_first", "flags"):
        assert refused(vote, b"vadx_dfsmn_vote_ragged", **{k: None}) and b"NULL" in err(), k
    for k in ("batch", "n_windows", "max_windows", "frames"):
        for bad in (0, -1):
            assert refused(vote, b"vadx_dfsmn_vote_ragged", **{k: bad}), (k, bad)
    assert refused(vote, b"vadx_dfsmn_vote_ragged", flag_stride=4 * slide + LB - 1) and refused(vote, b"vadx_dfsmn_vote_ragged", flag_stride=0)
    for bad in (0, -1, T, T + 7):
        assert refused(vote, b"vadx_dfsmn_vote_ragged", look_backward=bad), bad

    win = lambda **kw: lib.vadx_dfsmn_stream_windows(*[kw.get(k, v) for k, v in (                                      # noqa: E731
        ("near", ptr), ("far", ptr), ("row_stride", L), ("streams", 2), ("n_slots", 2), ("windows", 1), ("window_len", L), ("look_backward", LB),
        ("slot", None), ("reset", None), ("state_in", rec_a), ("state_out", rec_b), ("near_buf", ptr), ("far_buf", ptr), ("stream", None))])
    name = b"vadx_dfsmn_stream_windows"
    for k in ("near", "state_in", "state_out", "near_buf", "far", "far_buf"):      # far without far_buf, and the reverse
        assert refused(win, name, **{k: None}) and b"NULL" in err(), k
    for k in ("streams", "n_slots", "windows"):
        for bad in (0, -1):
            assert refused(win, name, **{k: bad}), (k, bad)
    for bad in (0, -1, T - 1, T):                                         # T - 1: (lb + 1) * 320 > window_len, no stride left
        assert refused(win, name, look_backward=bad), bad
    assert refused(win, name, window_len=0) and refused(win, name, window_len=CARRY)
    assert refused(win, name, row_stride=STRIDE - 1)
    assert win(state_out=rec_a) == -1 and name in err() and b"overlap" in err()
    assert win(state_out=rec_a + nb - 16) == -1 and b"overlap" in err()
    assert win(state_in=rec_b, state_out=rec_b - 16) == -1 and b"overlap" in err()

    vt = lambda **kw: lib.vadx_dfsmn_stream_vote(*[kw.get(k, v) for k, v in (                                          # noqa: E731
        ("vad", ptr), ("streams", 2), ("n_slots", 2), ("windows", 1), ("frames", T), ("look_backward", LB), ("channels", 2), ("speaking", 0.5),
        ("silence", 0.5), ("slot", None), ("reset", None), ("state_in", rec_a), ("state_out", rec_b), ("flags", ptr), ("tail", ptr),
        ("stream", None))])
    name = b"vadx_dfsmn_stream_vote"
    for k in ("vad", "state_in", "state_out", "flags", "tail"):
        assert refused(vt, name, **{k: None}) and b"NULL" in err(), k
    for k in ("streams", "n_slots", "windows", "frames"):
        for bad in (0, -1):
            assert refused(vt, name, **{k: bad}), (k, bad)
    for bad in (0, -1, T, T + 7):
        assert refused(vt, name, look_backward=bad), bad
    assert refused(vt, name, channels=0) and refused(vt, name, channels=3)
    assert vt(state_out=rec_a) == -1 and name in err() and b"overlap" in err()
    assert vt(state_out=rec_a + 16) == -1 and b"overlap" in err()


def _pairs():
    rng = np.random.default_rng(3)
    near = [rng.integers(-9000, 9000, n).astype(np.float32) for n in NEAR_LEN]
    far = [rng.integers(-5000, 5000, n).astype(np.float32) for n in FAR_LEN]
    nz_near, nz_far = rng.standard_normal((len(near), 2 * L)), rng.standard_normal((len(near), 2 * L))
    return near, far, nz_near, nz_far


@pytest.mark.parametrize("near_only", [False, True])
def test_ragged_pairs_host_tables_and_padding(near_only):
    near, far, nz_near, nz_far = _pairs()
    if near_only:
        far = None
    prep = lambda a: timestamps.normalize_to_int16(np.asarray(a).astype(np.float32))      # noqa: E731
    rp = ragged.RaggedPairs.from_clips(near, far, L, STRIDE, nz_near, nz_far, prep=prep, device=None)
    cut = [len(a) for a in near] if near_only else [min(len(a), len(f)) for a, f in zip(near, far)]
    want_w = [1 if n <= L else -(-(n - L) // STRIDE) + 1 for n in cut]
    if not near_only:
        assert tuple(want_w) == WINDOWS
    assert len(rp) == len(near) and rp.device is None
    assert rp.lengths.tolist() == cut and rp.windows.tolist() == want_w
    assert rp.padded_lengths.tolist() == [(w - 1) * STRIDE + L for w in want_w]
    assert rp.clip_off.tolist() == np.concatenate([[0], np.cumsum(rp.padded_lengths)[:-1]]).tolist()      # end to end, no filler
    assert rp.win_first.dtype == np.int32 and rp.win_first.tolist() == np.concatenate([[0], np.cumsum(want_w)]).tolist()
    assert rp.win_src.dtype == np.int64 and rp.n_windows == sum(want_w) and rp.max_windows == max(want_w)
    assert rp.win_src.tolist() == [int(rp.clip_off[b]) + k * STRIDE for b in range(len(near)) for k in range(want_w[b])]
    assert rp.near.dtype == np.int16 and rp.near.shape == (int(rp.padded_lengths.sum()),)
    assert (rp.far is None) if near_only else (rp.far.dtype == np.int16 and rp.far.shape == rp.near.shape)
    for b, n in enumerate(cut):
        got_near, got_far = rp.padded(b)
        assert np.array_equal(got_near, clips.pad_to_window_grid(prep(near[b][:n]), L, STRIDE, nz_near[b]))
        if near_only:
            assert got_far is None
        else:
            assert np.array_equal(got_far, clips.pad_to_window_grid(prep(far[b][:n]), L, STRIDE, nz_far[b]))
    with pytest.raises(ValueError):
        rp.gather()                                                      # host-only
    with pytest.raises(ValueError):
        ragged.RaggedPairs.from_clips(near, [near[0]], L, STRIDE, prep=prep, device=None)
    with pytest.raises(ValueError):
        ragged.RaggedPairs.from_clips([], None, L, STRIDE, device=None)


def timeline_model(carry, new, k):
    """The documented rule: timeline = carry ++ new samples (no carry before the first tick); window j = timeline[j*stride : j*stride + L];
    the new carry = the last (lb + 1) * 320 samples.  Returns (windows [k, L], carry)."""
    need = k * STRIDE if carry is not None else L + (k - 1) * STRIDE
    assert len(new) == need
    tl = np.concatenate([carry, new]) if carry is not None else np.asarray(new)
    assert len(tl) == L + (k - 1) * STRIDE
    return np.stack([tl[j * STRIDE:j * STRIDE + L] for j in range(k)]), tl[len(tl) - CARRY:]


@pytest.mark.parametrize("sched", [(1, 1, 1), (2, 1), (3,)])
def test_timeline_rule_reproduces_the_window_grid(lib, sched):
    assert lib.vadx_dfsmn_stream_state_bytes(1, L, LB, 1) - SHDR_WORDS * 4 == 2 * CARRY      # the carry the record holds is the model's
    W = sum(sched)
    padded = np.random.default_rng(W).integers(-32768, 32768, (W - 1) * STRIDE + L).astype(np.int16)
    carry, pos, j0 = None, 0, 0
    for k in sched:
        need = k * STRIDE if carry is not None else L + (k - 1) * STRIDE
        wins, carry = timeline_model(carry, padded[pos:pos + need], k)
        pos += need
        for j in range(k):
            assert np.array_equal(wins[j], padded[(j0 + j) * STRIDE:(j0 + j) * STRIDE + L]), (sched, j0 + j)
        j0 += k
        assert np.array_equal(carry, padded[pos - CARRY:pos])
    assert pos == len(padded) and j0 == W                                 # the whole clip is consumed, nothing twice


def chained_vote(scores, sched, speaking, silence_score, lb=LB):
    """The host reference of the stream path: oracle.postproc.lookahead_vote window by window, its returned `silence` carried from tick to
    tick, and oracle.dfsmn.tail_flags on a copy of it after each tick.  scores [W, frames] -> (flags per tick, tail per tick)."""
    frames, silence, w0 = scores.shape[1], True, 0
    ticks, tails = [], []
    for k in sched:
        fl = []
        for w in range(w0, w0 + k):
            f, silence = opp.lookahead_vote(scores[w], frames - lb, lb, speaking, silence_score, silence, thresholds=(speaking, silence_score))
            fl += f
        w0 += k
        ticks.append(np.array(fl, dtype=bool))
        tails.append(np.array(od.tail_flags(scores[w0 - 1], frames - lb, frames, silence, speaking, silence_score)[0], dtype=bool))
    return ticks, tails


def test_chained_oracle_vote_is_the_whole_clip_list(golden):
    """On the scores the REFERENCE loop was run on (asymmetric thresholds, scores exactly on float32(threshold) included): the ticks of any
    schedule laid end to end, plus the last tick's tail, are the reference's `saved` list."""
    g = golden("hostloop_thresholds")
    for c, (spk, sil) in enumerate(g["pairs"]):
        scores, saved = g[f"dfsmn_scores_{c}"], g[f"dfsmn_saved_{c}"]
        W = scores.shape[0]
        for sched in ((1,) * W, (W,), (2,) + (1,) * (W - 2), (1,) * (W - 2) + (2,)):
            ticks, tails = chained_vote(scores, sched, float(spk), float(sil))
            assert np.array_equal(np.concatenate(ticks + [tails[-1]]), saved), (c, sched)
