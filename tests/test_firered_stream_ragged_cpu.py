"""CPU: the ragged-tick entry point of the FireRed streams exists under ABI 10 and refuses bad arguments on the host, by name, before any
device call; the column plan of a tick (vadx.ragged.column_stream_plan: a counting sort and a closed form per distinct count) against a
plain per-stream next-fit loop; and FireRedStreamBatch.step_ragged's refusals, which come before an engine is touched."""
import ctypes as C
import types

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, firered, ragged, weights

WHO = b"vadx_firered_stream_tick_ragged"


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def _cfg(frames=14, **kw):
    c = dict(weights.FIRERED_CFG, N2=0, S2=0, **kw)
    cfg = _lib.FireRedCfg()
    for k in ("idim", "R", "M", "H", "P", "N1", "S1", "N2", "S2", "odim"):
        setattr(cfg, k, int(c[k]))
    cfg.frames, cfg.arithmetic = frames, _lib.GEMM_MODES["split"]
    return cfg


def test_symbol_and_abi(lib):
    assert hasattr(lib, "vadx_firered_stream_tick_ragged") and "vadx_firered_stream_tick_ragged" in _lib.SIGNATURES
    assert lib.vadx_abi_version() == 10 == _lib.ABI_VERSION
    assert lib.vadx_firered_stream_group_max(14) == 8 == ragged.TICK_COLUMNS // 14


def test_bad_arguments_are_refused_on_the_host(lib):
    """Every VADX_EINVAL of the contract, with the argument's name in vadx_last_error -- before any HIP call (there is no device here; the
    pointers below are host memory nothing may touch)."""
    S = 2
    cfg = _cfg()
    nb = lib.vadx_firered_stream_state_bytes(C.byref(cfg), S)
    assert nb > 0
    buf = (C.c_char * (2 * nb + 128))()
    base = (C.addressof(buf) + 15) & ~15
    rec_a, rec_b, ptr = base, base + nb + 32, base
    post = _lib.StreamVadPostParams(5, 0.4, 5, 8, 2000, 20)
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731
    call = lambda **kw: lib.vadx_firered_stream_tick_ragged(*[kw.get(k, v) for k, v in (                              # noqa: E731
        ("cfg", C.byref(cfg)), ("packed", ptr), ("logmel", ptr), ("streams", S), ("n_rows", 3), ("counts", ptr), ("row_first", ptr),
        ("slot_stream", ptr), ("wg_first", ptr), ("n_wg", 1), ("post", C.byref(post)), ("reset", None), ("state_in", rec_a),
        ("state_out", rec_b), ("probs", ptr), ("segments", ptr), ("counts_out", ptr), ("cap", 4), ("open_start", ptr), ("status", ptr),
        ("stream", None))])
    for k in ("cfg", "packed", "logmel", "counts", "row_first", "slot_stream", "wg_first", "post", "state_in", "state_out", "probs", "segments",
              "counts_out", "open_start", "status"):
        assert call(**{k: None}) == -1 and WHO in err() and k.encode() + b" is NULL" in err(), k
    for k in ("streams", "n_rows", "n_wg", "cap"):
        assert call(**{k: 0}) == -1 and WHO in err() and k.encode() + b"=0" in err(), k
        assert call(**{k: -3}) == -1 and k.encode() + b"=-3" in err(), k
    for frames in (113, 0):
        assert call(cfg=C.byref(_cfg(frames))) == -1 and WHO in err() and b"frames=%d" % frames in err()
    bad = _cfg()
    bad.N2, bad.S2 = 2, 1
    assert call(cfg=C.byref(bad)) == -1 and WHO in err() and b"N2" in err()
    assert call(post=C.byref(_lib.StreamVadPostParams(17, 0.4, 5, 8, 2000, 20))) == -1 and WHO in err() and b"smooth_window_size" in err()
    assert call(state_out=rec_a) == -1 and WHO in err() and b"overlap" in err()
    assert call(state_out=rec_a + nb - 16) == -1 and b"overlap" in err()
    assert call(state_in=rec_a + 4) == -1 and WHO in err() and b"aligned" in err()
    assert call(state_out=rec_b + 8) == -1 and WHO in err() and b"aligned" in err()


def patterns(S, cap, rng):
    ramp = np.arange(S) % (cap + 1)
    one = np.zeros(S, np.int64)
    one[S // 2] = cap
    return {"all zero": np.zeros(S, np.int64), "all at the capacity": np.full(S, cap), "one active": one, "ramp": ramp, "ramp down": ramp[::-1].copy(),
            "random": rng.integers(0, cap + 1, S), "sparse": rng.integers(0, cap + 1, S) * (rng.random(S) < 0.2)}


def next_fit(counts, order, capacity, g):
    """A workgroup takes consecutive positions of the active prefix of `order` while its counts sum to <= capacity and it holds <= g streams"""
    wg, used, held = [0], 0, 0
    active = int(np.count_nonzero(counts))
    for pos in range(active):
        v = int(counts[order[pos]])
        if held and (used + v > capacity or held + 1 > g):
            wg.append(pos)
            used = held = 0
        used, held = used + v, held + 1
    return np.array(wg + [active] if active else [0])


@pytest.mark.parametrize("S", [1, 2, 3, 16, 17, 255, 256, 257, 1024, 1025])
def test_column_plan_against_a_plain_loop(S):
    rng = np.random.default_rng(S)
    for cap in (1, 2, 3, 8, 112):
        for name, counts in patterns(S, cap, rng).items():
            for group in (0, 1, cap):
                first, order, wg = ragged.column_stream_plan(counts, cap, group)
                what = (name, cap, group)
                assert first.dtype == np.int64 and order.dtype == wg.dtype == np.int32, what
                assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)])), what
                assert np.array_equal(order, np.argsort(-np.asarray(counts), kind="stable")), what
                active = int(np.count_nonzero(counts))
                g = group or min(max(active // 256, 1), cap)
                assert np.array_equal(wg, next_fit(counts, order, cap, g)), what
                assert wg[0] == 0 and wg[-1] == active and (np.diff(wg) >= 1).all() and (np.diff(wg) <= g).all(), what
                sums = np.add.reduceat(np.asarray(counts)[order[:active]], wg[:-1]) if active else np.zeros(0)
                assert (sums <= cap).all() and (sums >= 1).all(), what
                assert np.array_equal(np.sort(order[:active]), np.flatnonzero(counts)), what          # every active stream exactly once


def test_column_plan_refusals():
    for bad in (np.array([0, 9]), np.array([-1, 2]), np.zeros(2, np.float32), np.zeros((2, 1), np.int64)):
        with pytest.raises(ValueError):
            ragged.column_stream_plan(bad, 8)
    with pytest.raises(ValueError, match="group"):
        ragged.column_stream_plan(np.array([1, 2]), 8, group=9)
    with pytest.raises(ValueError, match="capacity"):
        ragged.column_stream_plan(np.array([1, 2]), 113)


def fake_batch(S):
    """A FireRedStreamBatch on an engine that has no device side at all: any launch would raise AttributeError."""
    import torch
    cfg = _cfg(firered.valid_frame_count(firered.STREAM_CHUNK_SAMPLES))
    c = dict(weights.FIRERED_CFG, N2=0, S2=0)
    eng = object.__new__(firered.FireRedEngine)
    eng.torch, eng.device, eng.L, eng.in_sample_rate, eng.odim = torch, torch.device("cpu"), firered.STREAM_CHUNK_SAMPLES, 16000, c["odim"]
    eng.cache_shape = (c["R"], 1, c["P"], (c["N1"] - 1) * c["S1"])
    eng.blobs = types.SimpleNamespace(get=lambda: (cfg, None))
    return firered.FireRedStreamBatch(eng, S)


def test_step_ragged_refuses_before_touching_an_engine(lib):
    S, n = 5, firered.STREAM_CHUNK_SAMPLES
    it = fake_batch(S)
    it.reset_states([1])
    x = np.zeros((S, 8 * n), np.int16)
    for counts in (np.full(S, -1), np.array([0, 1, 2, 3, 9]), np.zeros(S, np.float32), np.zeros(S + 1, np.int64), np.zeros((S, 1), np.int64)):
        with pytest.raises(ValueError):
            it.step_ragged(x, counts)
    with pytest.raises(ValueError, match="counts"):
        it.step_ragged(x)
    with pytest.raises(ValueError, match="samples must be"):
        it.step_ragged(x[:, :2 * n], np.array([0, 1, 3, 0, 0]))                  # three chunks asked of rows that hold two
    with pytest.raises(ValueError, match="int16"):
        it.step_ragged(x.astype(np.float32), np.ones(S, np.int64))
    with pytest.raises(ValueError, match="int16"):
        it.step_ragged([np.zeros(n, np.float32)] + [np.zeros(0, np.int16)] * (S - 1))
    with pytest.raises(ValueError, match=r"samples\[1\]"):
        it.step_ragged([np.zeros(n, np.int16), np.zeros(n + 1, np.int16)] + [np.zeros(0, np.int16)] * (S - 2))
    with pytest.raises(ValueError, match="lists 2 arrays"):
        it.step_ragged([np.zeros(n, np.int16)] * 2)
    with pytest.raises(ValueError, match="disagree"):
        it.step_ragged([np.zeros(n, np.int16)] * S, np.full(S, 2))
    with pytest.raises(ValueError, match="at least 400"):
        it.step_ragged(x, np.ones(S, np.int64), chunk=399)
    with pytest.raises(ValueError, match="at most 112 frames"):
        it.step_ragged(x, np.ones(S, np.int64), chunk=400 + 160 * 112)
    with pytest.raises(ValueError, match="group"):
        it.step_ragged(x, np.ones(S, np.int64), group=9)
    with pytest.raises(ValueError):
        it.step_ragged(x, np.full(S, 2), chunk=400 + 160 * 56)                   # 57 frames a chunk: one chunk per tick
    # a tick whose counts are all 0 launches nothing and leaves the record and the pending resets alone
    rec = it.record
    probs, events, first = it.step_ragged(x, np.zeros(S, np.int64))
    assert probs.shape == (1, 0) and events == [[] for _ in range(S)] and np.array_equal(first, np.zeros(S + 1))
    assert it.record is rec and not rec.any() and it._pending.tolist() == [False, True, False, False, False]
