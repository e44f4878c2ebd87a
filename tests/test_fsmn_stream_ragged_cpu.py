"""CPU: the ragged-tick entry points of the FSMN streams exist under ABI 10 and refuse bad arguments on the host before any device call;
the host plan of a tick (vadx.ragged.window_stream_plan: cumsum, repeat, counting sort) against plain numpy; and samples_needed_ragged
against a restatement of the timeline rule: any ragged schedule over a clip cuts exactly the windows of pad_to_window_grid."""
import ctypes as C

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, fsmn, ragged, weights

L, T, HOP = 16000, 101, 160


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_ragged_symbols_abi_and_cap(lib):
    for name in ("vadx_fsmn_stream_ragged_max_windows", "vadx_fsmn_stream_windows_ragged", "vadx_fsmn_stream_run_ragged"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.vadx_abi_version() == 10 == _lib.ABI_VERSION
    assert lib.vadx_fsmn_stream_ragged_max_windows() == 256 == ragged.STREAM_MAX_WINDOWS


def _dims():
    w = weights.fsmn_synthetic(1234)
    d = _lib.FsmnDims()
    d.input_affine_dim, d.linear_dim = w["in1_w"].shape[0], w["in2_w"].shape[0]
    d.output_affine_dim, d.output_dim = w["out1_w"].shape[0], w["out2_w"].shape[0]
    d.frames, d.speech_2_noise_ratio, d.arithmetic = T, 1.0, _lib.ARITH["split"]
    return d


def _loop_params(lb=30):
    lp = _lib.FsmnLoopParams()
    lp.look_backward, lp.one_minus_speech_threshold, lp.noise_db_init, lp.snr_threshold = lb, 1.0, 4.0, 1.0
    lp.speaking_score, lp.silence_score = 0.5, 0.5
    return lp


def test_bad_arguments_are_refused_on_the_host(lib):
    """Every VADX_EINVAL of the contract, with the argument's name in vadx_last_error -- before any HIP call (there is no device here; the
    pointers below are host memory nothing may touch)."""
    S, lb, stride = 2, 30, L - 31 * HOP
    nb = lib.vadx_fsmn_stream_state_bytes(S, lb)
    buf = (C.c_char * (2 * nb + 64))()
    base = (C.addressof(buf) + 15) & ~15
    rec_a, rec_b, ptr = base, base + nb, base
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731
    win = lambda **kw: lib.vadx_fsmn_stream_windows_ragged(*[kw.get(k, v) for k, v in (                               # noqa: E731
        ("samples", ptr), ("row_stride", 4 * stride), ("streams", S), ("n_windows", 3), ("max_windows", 4), ("window_len", L),
        ("look_backward", lb), ("counts", ptr), ("win_first", ptr), ("win_stream", ptr), ("reset", None), ("state_in", rec_a),
        ("state_out", rec_b), ("window_buf", ptr), ("status", ptr), ("stream", None))])
    d, lp = _dims(), _loop_params(lb)
    run = lambda **kw: lib.vadx_fsmn_stream_run_ragged(*[kw.get(k, v) for k, v in (                                   # noqa: E731
        ("dims", C.byref(d)), ("packed", ptr), ("logmel", ptr), ("db", ptr), ("streams", S), ("n_windows", 3), ("max_windows", 4),
        ("lp", C.byref(lp)), ("counts", ptr), ("win_first", ptr), ("order", None), ("reset", None), ("state_in", rec_a), ("state_out", rec_b),
        ("flags", ptr), ("tail", ptr), ("noise_trace", None), ("status", ptr), ("stream", None))])
    cases = [(win, b"vadx_fsmn_stream_windows_ragged", ("samples", "counts", "win_first", "win_stream", "state_in", "state_out", "window_buf", "status")),
             (run, b"vadx_fsmn_stream_run_ragged", ("dims", "packed", "logmel", "db", "lp", "counts", "win_first", "state_in", "state_out", "flags",
                                                    "tail", "status"))]
    for call, who, pointers in cases:
        for k in pointers:
            assert call(**{k: None}) == -1 and who in err() and b"NULL " + k.encode() in err(), k
        for k in ("streams", "n_windows", "max_windows"):
            assert call(**{k: 0}) == -1 and who in err() and k.encode() + b"=0" in err(), k
            assert call(**{k: -3}) == -1 and k.encode() + b"=-3" in err(), k
        assert call(max_windows=257) == -1 and who in err() and b"max_windows=257" in err()
        assert call(state_out=rec_a) == -1 and who in err() and b"overlap" in err()
        assert call(state_out=rec_a + nb - 16) == -1 and b"overlap" in err()
        assert call(state_in=rec_a + 4) == -1 and who in err() and b"aligned" in err()
    for bad in (-1, T, T - 2):                                           # T - 2: (lb + 1) * 160 == window_len, no stride left
        assert win(look_backward=bad) == -1 and b"vadx_fsmn_stream_windows_ragged" in err() and b"look_backward" in err(), bad
        assert run(lp=C.byref(_loop_params(bad))) == -1 and b"vadx_fsmn_stream_run_ragged" in err() and b"look_backward" in err(), bad
    assert win(row_stride=4 * stride - 8) == -1 and b"row_stride" in err()       # below max_windows * stride
    assert win(row_stride=4 * stride + 4) == -1 and b"row_stride" in err()       # not a multiple of 8
    assert win(samples=ptr + 2) == -1 and b"aligned" in err()


def patterns(S, mw, rng):
    ramp = np.arange(S) % (mw + 1)
    one = np.zeros(S, np.int64)
    one[S // 2] = mw
    return {"all zero": np.zeros(S, np.int64), "all equal": np.full(S, 3), "one active": one, "ramp": ramp, "ramp down": ramp[::-1].copy(),
            "random": rng.integers(0, mw + 1, S), "sparse": rng.integers(0, mw + 1, S) * (rng.random(S) < 0.2), "all at the cap": np.full(S, mw)}


@pytest.mark.parametrize("S", [1, 2, 3, 16, 17, 255, 256, 1024, 1025])
def test_host_plan_against_numpy(S):
    rng = np.random.default_rng(S)
    for mw in (4, 256):
        for name, counts in patterns(S, mw, rng).items():
            first, win_stream, order = ragged.window_stream_plan(counts, mw)
            assert first.dtype == np.int64 and win_stream.dtype == order.dtype == np.int32, name
            assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)])), name
            want = np.concatenate([np.full(int(c), s) for s, c in enumerate(counts)] + [np.zeros(0, np.int64)])
            assert np.array_equal(win_stream, want), name
            assert np.array_equal(order, np.argsort(-np.asarray(counts), kind="stable")), name         # the counting sort IS the stable argsort
            idle = np.flatnonzero(np.asarray(counts) == 0)
            assert np.array_equal(order[S - len(idle):], idle), name                                       # idle streams last, in index order


def fake_batch(S, lb_s):
    """An FsmnStreamBatch on an engine that has no device side at all: any launch would raise AttributeError."""
    import torch
    eng = object.__new__(fsmn.FsmnEngine)
    eng.torch, eng.device, eng.L, eng.T, eng.long_windows = torch, torch.device("cpu"), L, T, False
    return fsmn.FsmnStreamBatch(eng, S, look_backward_s=lb_s)


@pytest.mark.parametrize("lb_s", [0.3, 0.0])
def test_ragged_schedules_reproduce_the_window_grid(lb_s):
    """samples_needed_ragged against the timeline rule restated in numpy: timeline = carry ++ new samples (no carry before the first tick
    or after a reset); window j = timeline[j * stride : j * stride + L]; the new carry = the stream's own last (lb + 1) * 160 samples.
    Any ragged schedule then cuts every clip into exactly the windows of its pad_to_window_grid, and consumes it once."""
    S, rng = 6, np.random.default_rng(5)
    it = fake_batch(S, lb_s)
    lb, stride = it.lb, it.stride
    Cn = (lb + 1) * HOP
    assert stride == L - Cn
    W = [1, 2, 3, 5, 8, 13]
    clips = [rng.integers(-32768, 32768, (w - 1) * stride + L - 123).astype(np.int16) for w in W]
    padded = [fsmn.pad_to_window_grid(c, L, stride, rng.standard_normal(200)) for c in clips]
    assert [(len(p) - L) // stride + 1 for p in padded] == W
    carry, pos, done, left = [None] * S, [0] * S, [0] * S, np.array(W)
    restarted = False
    while left.any():
        counts = np.minimum(rng.integers(0, 5, S), left)
        if not restarted and done[5] >= 4:                               # stream 5 is reset mid-clip: the request waits over a tick with count 0
            it.reset_states([5])
            idle = counts.copy()
            idle[5] = 0
            assert it.samples_needed_ragged(idle)[5] == 0
            carry[5], pos[5], done[5], left[5], restarted = None, 0, 0, W[5], True
            counts[5] = 2
        need = it.samples_needed_ragged(counts)
        for s in range(S):
            n = int(counts[s])
            if n == 0:
                assert need[s] == 0
                continue
            assert need[s] == (n * stride if carry[s] is not None else L + (n - 1) * stride)
            new = padded[s][pos[s]:pos[s] + need[s]]
            assert len(new) == need[s]
            tl = new if carry[s] is None else np.concatenate([carry[s], new])
            for j in range(n):
                assert np.array_equal(tl[j * stride:j * stride + L], padded[s][(done[s] + j) * stride:(done[s] + j) * stride + L]), (s, j)
            carry[s], pos[s], done[s] = tl[len(tl) - Cn:], pos[s] + int(need[s]), done[s] + n
        act = counts > 0
        it._begin(None, act, upload_active=False)
        it._end(act)
        left = left - counts
    assert restarted and pos == [len(p) for p in padded] and done == W
    # the lengths of a list ARE the counts
    assert np.array_equal(it._counts_of_lengths(it.samples_needed_ragged([0, 1, 2, 3, 4, 0])), [0, 1, 2, 3, 4, 0])
    with pytest.raises(ValueError, match=r"samples\[2\]"):
        it._counts_of_lengths([0, stride, 2 * stride + 1, 0, 0, 0])


def test_step_ragged_refuses_bad_counts_before_touching_an_engine():
    S = 5
    it = fake_batch(S, 0.3)
    x = np.zeros((S, 4 * L), np.int16)
    bad = [np.full(S, -1), np.array([0, 1, 2, 3, 5]), np.zeros(S, np.float32), np.zeros(S + 1, np.int64), np.zeros((S, 1), np.int64)]
    for counts in bad:
        with pytest.raises(ValueError):
            it.step_ragged(x, counts, max_windows=4)
    with pytest.raises(ValueError, match="max_windows"):
        it.step_ragged(x, np.zeros(S, np.int64), max_windows=257)
    with pytest.raises(ValueError, match="counts"):
        it.step_ragged(x)
    with pytest.raises(ValueError, match="samples_needed_ragged"):
        it.step_ragged(x[:, :L - 1], np.ones(S, np.int64))
    with pytest.raises(ValueError, match="int16"):
        it.step_ragged([np.zeros(L, np.float32)] + [np.zeros(0, np.int16)] * (S - 1))
    with pytest.raises(ValueError):
        it.samples_needed_ragged(np.full(S, 257))
    assert not it.record.any() and not it._pending.any() and not it._primed.any()
