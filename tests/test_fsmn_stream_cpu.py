"""CPU: the FSMN stream entry points (ABI 10) exist, size their record as documented and validate their arguments on the host before any
device call; and the timeline rule of vadx_fsmn_stream_windows (carry ++ new samples -> windows, new carry), restated in numpy, cuts a
stream that arrives in pieces into exactly the windows the whole-clip path cuts."""
import ctypes as C

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, fsmn, weights

L, T, HOP = 16000, 101, 160
CACHE_BYTES = 4 * 128 * 19 * 4


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_stream_symbols_and_abi(lib):
    for name in ("vadx_fsmn_stream_state_bytes", "vadx_fsmn_stream_windows", "vadx_fsmn_stream_run"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.vadx_abi_version() == 10 == _lib.ABI_VERSION


@pytest.mark.parametrize("lb", [0, 30, 97])
def test_state_bytes(lib, lb):
    one = lib.vadx_fsmn_stream_state_bytes(1, lb)
    for S in (1, 3, 64, 4097):
        n = lib.vadx_fsmn_stream_state_bytes(S, lb)
        assert n % 16 == 0 and n == S * one                              # aligned, linear in S
        assert n >= S * (CACHE_BYTES + 2 * (lb + 1) * HOP)                # the caches and the carry fit
    assert lib.vadx_fsmn_stream_state_bytes(0, lb) == 0 and lib.vadx_fsmn_stream_state_bytes(-1, lb) == 0
    assert lib.vadx_fsmn_stream_state_bytes(4, -1) == 0


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
    """NULL pointers, windows < 1, a look-back that leaves no stride and overlapping records come back as VADX_EINVAL with a message that
    names the function -- before any HIP call (there is no device here; the pointers below are host memory nothing may touch)."""
    S, lb = 2, 30
    nb = lib.vadx_fsmn_stream_state_bytes(S, lb)
    buf = (C.c_char * (2 * nb + 64))()
    base = (C.addressof(buf) + 15) & ~15
    rec_a, rec_b, ptr = base, base + nb, base                            # two disjoint aligned records
    win = lambda **kw: lib.vadx_fsmn_stream_windows(*[kw.get(k, v) for k, v in (                                      # noqa: E731
        ("samples", ptr), ("row_stride", 16000), ("streams", S), ("windows", 1), ("window_len", L), ("look_backward", lb), ("reset", None),
        ("active", None), ("state_in", rec_a), ("state_out", rec_b), ("window_buf", ptr), ("stream", None))])
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731
    for k in ("samples", "state_in", "state_out", "window_buf"):
        assert win(**{k: None}) == -1 and b"vadx_fsmn_stream_windows" in err() and b"NULL" in err(), k
    assert win(windows=0) == -1 and b"vadx_fsmn_stream_windows" in err() and b"windows=0" in err()
    for bad in (-1, T, T - 2):                                           # T - 2: (lb + 1) * 160 == window_len, no stride left
        assert win(look_backward=bad) == -1 and b"vadx_fsmn_stream_windows" in err() and b"look_backward" in err(), bad
    assert win(state_out=rec_a) == -1 and b"vadx_fsmn_stream_windows" in err() and b"overlap" in err()
    assert win(state_out=rec_a + nb - 16) == -1 and b"overlap" in err()
    assert win(state_in=rec_b, state_out=rec_b - 16) == -1 and b"overlap" in err()
    assert win(row_stride=11032) == -1 and b"row_stride" in err()        # fewer than windows * stride samples per row

    d, lp = _dims(), _loop_params(lb)
    run = lambda **kw: lib.vadx_fsmn_stream_run(*[kw.get(k, v) for k, v in (                                          # noqa: E731
        ("dims", C.byref(d)), ("packed", ptr), ("logmel", ptr), ("db", ptr), ("streams", S), ("windows", 1), ("lp", C.byref(lp)),
        ("reset", None), ("active", None), ("state_in", rec_a), ("state_out", rec_b), ("flags", ptr), ("tail", ptr), ("noise_trace", None),
        ("stream", None))])
    for k in ("dims", "packed", "logmel", "db", "lp", "state_in", "state_out", "flags", "tail"):
        assert run(**{k: None}) == -1 and b"vadx_fsmn_stream_run" in err() and b"NULL" in err(), k
    assert run(windows=0) == -1 and b"vadx_fsmn_stream_run" in err() and b"windows=0" in err()
    assert run(state_out=rec_a) == -1 and b"vadx_fsmn_stream_run" in err() and b"overlap" in err()
    assert run(state_out=rec_a + 16) == -1 and b"overlap" in err()
    for bad in (-1, T, T - 2):
        assert run(lp=C.byref(_loop_params(bad))) == -1 and b"vadx_fsmn_stream_run" in err() and b"look_backward" in err(), bad


def timeline_model(carry, new, k, lb):
    """The documented rule: timeline = carry ++ new samples (no carry before the first tick); window j = timeline[j*stride : j*stride + L];
    the new carry = the last (lb + 1) * 160 samples.  Returns (windows [k, L], carry)."""
    Cn = (lb + 1) * HOP
    stride = L - Cn
    need = k * stride if carry is not None else L + (k - 1) * stride
    assert len(new) == need
    tl = np.concatenate([carry, new]) if carry is not None else np.asarray(new)
    assert len(tl) == L + (k - 1) * stride
    return np.stack([tl[j * stride:j * stride + L] for j in range(k)]), tl[len(tl) - Cn:]


@pytest.mark.parametrize("lb,schedules", [(30, [(1, 1, 1, 1), (2, 1, 1), (4,)]), (0, [(1, 1, 1), (2, 1), (3,)])])
def test_timeline_rule_reproduces_the_window_grid(lb, schedules):
    stride = L - (lb + 1) * HOP
    W = sum(schedules[0])
    padded = np.random.default_rng(lb).integers(-32768, 32768, (W - 1) * stride + L).astype(np.int16)
    for sched in schedules:
        assert sum(sched) == W
        carry, pos, j0 = None, 0, 0
        for k in sched:
            need = k * stride if carry is not None else L + (k - 1) * stride
            wins, carry = timeline_model(carry, padded[pos:pos + need], k, lb)
            pos += need
            for j in range(k):
                assert np.array_equal(wins[j], padded[(j0 + j) * stride:(j0 + j) * stride + L]), (sched, j0 + j)
            j0 += k
            assert np.array_equal(carry, padded[pos - (lb + 1) * HOP:pos])
        assert pos == len(padded) and j0 == W                             # the whole clip is consumed, nothing twice


def test_stream_batch_needs_a_gpu_engine():
    """FsmnStreamBatch has no host path: it is built on an FsmnEngine, which refuses to exist without a device."""
    with pytest.raises(TypeError):
        fsmn.FsmnStreamBatch(object(), 4)
