"""CPU: the host half of the ragged Silero stream tick (vadx.ragged.stream_plan), the numpy mirror of the device planner, and what
vadx_silero_stream_plan / vadx_silero_stream_run_ragged and VADIteratorBatch.step_ragged refuse before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, ragged

SIZES = [1, 15, 16, 17, 37, 1025]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def patterns(S):
    rng = np.random.default_rng(S)
    every = np.arange(S) % 257                                   # every count 0 .. 256 (as far as S reaches)
    one = np.zeros(S, np.int64)
    one[S // 2] = 7
    inter = rng.integers(1, 40, S)
    inter[::2] = 0
    return {"equal": np.full(S, 5), "one active": one, "zeros interleaved": inter, "every count": every,
            "every count, shuffled": rng.permutation(every), "sorted up": np.sort(every), "sorted down": np.sort(every)[::-1].copy(),
            "jitter": rng.choice([0, 1, 3, 16], S)}


@pytest.mark.parametrize("window", [512, 256])
@pytest.mark.parametrize("S", SIZES)
def test_plan_agrees_with_the_ragged_batch_tables(S, window):
    """stream_plan (a histogram, no sort) against RaggedClips._set_tables (a stable argsort) over the active streams as clips of
    n_s * window samples.  The one intended difference: a stream's slot is its staged row [context | n_s windows], so grp_min_len of a
    full group is the batch's + cw."""
    sr = {512: 16000, 256: 8000}[window]
    for name, counts in patterns(S).items():
        p = ragged.stream_plan(counts, window)
        act = np.flatnonzero(counts > 0)
        assert p.active == len(act) and p.n_windows == int(counts.sum()) and p.max_windows == max(int(counts.max()), 1), name
        assert p.row == window // 8 + p.max_windows * window
        want_bf = np.array([(counts > c).sum() for c in range(p.max_windows + 2)])
        assert np.array_equal(p.bucket_first, want_bf) and p.bucket_first.dtype == np.int32, name
        if len(act) == 0:                                         # (S = 1: a lone stream with count 0)
            assert p.groups == 0
            continue
        ref = ragged.RaggedClips()
        ref._set_tables(counts[act] * window, np.zeros(len(act), np.int64), sr)
        assert p.groups == ref.groups and p.tiles == ref.tiles and p.n_runs == ref.n_runs, name
        assert np.array_equal(p.group_windows, ref.group_windows), name
        assert np.array_equal(p.gx_first, ref.gx_first_host) and p.gx_first.dtype == np.int32, name
        assert np.array_equal(p.wg_tab, ref.wg_tab_host) and p.wg_tab.dtype == np.int32, name
        assert np.array_equal(p.grp_min_len, np.where(ref.grp_min_len_host > 0, ref.grp_min_len_host + window // 8, 0)), name
        # with an explicit max_windows only the row, the bucket table's length and the default change
        q = ragged.stream_plan(counts, window, max_windows=256)
        assert q.row == window // 8 + 256 * window and len(q.bucket_first) == 258
        assert np.array_equal(q.bucket_first[:len(want_bf)], want_bf) and not q.bucket_first[len(want_bf):].any()
        assert np.array_equal(q.wg_tab, p.wg_tab) and np.array_equal(q.grp_min_len, p.grp_min_len)
        # one staging vector
        host, at = p.staging()
        assert host.dtype == np.int32 and np.array_equal(host[at["counts"]:at["counts"] + S], counts)
        assert np.array_equal(host[at["wg_tab"]:].reshape(-1, 2), p.wg_tab)


def test_plan_of_a_silent_tick_has_no_groups():
    p = ragged.stream_plan(np.zeros(40, np.int64), 512)
    assert p.groups == 0 and p.active == 0 and p.n_windows == 0 and not p.bucket_first.any()


@pytest.mark.parametrize("S", SIZES + [1023, 1024, 2049])
def test_mirror_of_the_device_plan_is_the_stable_argsort(S):
    for name, counts in patterns(S).items():
        p = ragged.stream_plan(counts, 512)
        if p.groups == 0:
            continue
        first, off, ln, clip, status = ragged.stream_slots_mirror(counts, p.bucket_first, p.groups, 512, p.max_windows)
        order = np.argsort(-counts, kind="stable")[:p.active]
        assert status == 0, name
        assert np.array_equal(clip[:p.active], order) and (clip[p.active:] == -1).all() and len(clip) == 16 * p.groups, name
        assert np.array_equal(off[:p.active], order * p.row) and not off[p.active:].any(), name
        assert np.array_equal(ln[:p.active], 64 + counts[order] * 512) and not ln[p.active:].any(), name
        assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)])) and first.dtype == np.int64, name
        # the tables are those of the ragged batch the tick is: every group's first slot has the group's window count
        assert np.array_equal((ln[::16] - 64) // 512, p.group_windows), name


def test_mirror_takes_bad_counts_as_zero():
    counts = np.array([3, -1, 2, 257, 2, 0, 9])
    clean = np.where((counts < 0) | (counts > 16), 0, counts)
    p = ragged.stream_plan(clean, 256, max_windows=16)
    got = ragged.stream_slots_mirror(counts, p.bucket_first, p.groups, 256, 16)
    want = ragged.stream_slots_mirror(clean, p.bucket_first, p.groups, 256, 16)
    assert got[4] == 2 and want[4] == 0
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4]))
    assert list(got[3][:5]) == [6, 0, 2, 4, -1]


# ------------------------------------------------------------------ refusals
def test_python_refuses_bad_counts():
    for bad in (np.zeros(39, np.int64), np.zeros((40, 1), np.int64), np.full(40, -1), np.full(40, 17), np.zeros(40, np.float32)):
        with pytest.raises(ValueError):
            ragged.stream_counts(bad, 40, 16)
    with pytest.raises(ValueError, match="256"):
        ragged.stream_counts(np.full(40, 257), 40)
    for mw in (0, 257):
        with pytest.raises(ValueError, match="max_windows"):
            ragged.stream_counts(np.zeros(40, np.int64), 40, mw)
    assert ragged.stream_counts(np.arange(40) % 17, 40, 16).dtype == np.int32
    with pytest.raises(ValueError):
        ragged.stream_plan(np.full(4, 5), 512, max_windows=4)
    with pytest.raises(ValueError):
        ragged.stream_plan(np.full(4, 5), 500)


def test_step_ragged_refuses_bad_counts_before_any_launch(monkeypatch):
    import torch
    from vadx import silero
    eng = object.__new__(silero.SileroEngine)
    eng.torch, eng.device = torch, torch.device("cpu")
    it = silero.VADIteratorBatch(eng, 5)

    def no_launch():
        raise AssertionError("a refused tick must not reach the library")
    monkeypatch.setattr(_lib, "lib", no_launch)
    x = np.zeros((5, 4 * 512), np.float32)
    for counts in ([1, 2, 3, 4], [1, 2, 3, 4, -1], [1, 2, 3, 4, 5], [0, 0, 0, 0, 257], [[1, 2, 3, 4, 0]], [1.0, 2.0, 0.0, 0.0, 0.0]):
        with pytest.raises(ValueError):
            it.step_ragged(x, np.array(counts))
    with pytest.raises(ValueError, match="max_windows"):
        it.step_ragged(x, np.array([1, 2, 3, 4, 0]), max_windows=3)
    with pytest.raises(ValueError, match="max_windows"):
        it.step_ragged(x, np.array([1, 2, 3, 4, 0]), max_windows=257)
    with pytest.raises(ValueError):
        it.step_ragged(x)                                             # an array needs counts
    with pytest.raises(ValueError):
        it.step_ragged([np.zeros(512, np.float32)] * 4)               # four rows for five streams
    with pytest.raises(ValueError, match="whole windows"):
        it.step_ragged([np.zeros(500, np.float32)] * 5)
    with pytest.raises(ValueError):
        it.step_ragged([np.zeros(512, np.float32)] * 4 + [np.zeros(512, np.int16)])
    with pytest.raises(ValueError):
        it.step_ragged([np.zeros(512, np.float32)] * 5, counts=np.ones(5, np.int64))
    with pytest.raises(ValueError):
        it.step_ragged(np.zeros((5, 512), np.int32), np.ones(5, np.int64))
    # a silent tick is a no-op that launches nothing and keeps the record and the pending resets
    it.reset_states([1, 3])
    before = it.record
    kind, value, probs, first = it.step_ragged(x, np.zeros(5, np.int64))
    assert kind.numel() == value.numel() == probs.numel() == 0 and not first.any() and first.shape == (6,)
    assert it.record is before and list(it._pending) == [False, True, False, True, False]
    assert it.call_ragged([np.zeros(0, np.float32)] * 5) == [[], [], [], [], []]


def _tick_args(lib, S=40, mw=4, tiles=9, groups=3, n_runs=4):
    """Arguments of a C-level ragged tick over host memory that nothing may dereference: every refusal below comes first."""
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 255) & ~255
    ptr = lambda i: base + 16 * i                                                    # noqa: E731
    rg = _lib.SileroRagged(*[ptr(20 + i) for i in range(8)], S, groups, n_runs, tiles)
    prm = _lib.SileroIterParams()
    prm.threshold, prm.sampling_rate, prm.min_silence_duration_ms, prm.speech_pad_ms = 0.5, 16000, 100, 30
    rec = lib.vadx_silero_stream_state_bytes(S)
    need = lib.vadx_silero_stream_ragged_workspace_bytes(S, mw, tiles)
    args = [ptr(0), C.byref(prm), ptr(1), 0, 1.0, mw * 512, S, mw, C.byref(rg), None, base + (1 << 20), base + (1 << 20) + rec, ptr(4), ptr(5),
            ptr(6), ptr(7), need - 1, None, None]
    return args, (buf, rg, prm), rec, need


def test_c_level_tick_refuses_before_any_hip_call(lib):
    run = lib.vadx_silero_stream_run_ragged
    args, keep, rec, need = _tick_args(lib)
    assert lib.vadx_silero_stream_ragged_max_windows() == 256
    assert need == (lib.vadx_silero_stream_plan_bytes(40, 4) + lib.vadx_silero_stream_workspace_bytes(40, 4)
                    - ((lib.vadx_silero_workspace_bytes(40, 4) + 255) & ~255) + 9 * 32768)
    # a workspace one byte short: every other argument is acceptable, so this is the last refusal but the alignment's
    assert run(*args) == -2 and b"workspace" in lib.vadx_last_error()
    for i in (0, 1, 2, 8, 10, 11, 12, 13, 14, 15):
        bad = list(args)
        bad[i] = None
        assert run(*bad) == -1 and b"NULL" in lib.vadx_last_error(), i
    for field in ("slot_off", "slot_len", "slot_clip", "gx_first", "grp_min_len", "wg_tab", "probs_first", "status"):
        a2, keep2, _, _ = _tick_args(lib)
        setattr(keep2[1], field, None)
        assert run(*a2) == -1 and b"NULL table" in lib.vadx_last_error(), field
    for mw in (0, 257, -1):
        bad = list(args)
        bad[7] = mw
        assert run(*bad) == -1 and b"max_windows" in lib.vadx_last_error(), mw
    bad = list(args)
    bad[11] = bad[10] + rec - 16                                                     # overlapping records
    assert run(*bad) == -1 and b"overlap" in lib.vadx_last_error()
    bad[11] = bad[10]
    assert run(*bad) == -1 and b"overlap" in lib.vadx_last_error()
    bad = list(args)
    bad[5] = 4 * 512 - 1                                                             # row_stride below max_windows windows
    assert run(*bad) == -1 and b"row_stride" in lib.vadx_last_error()
    # the rate: cfg against prm, both ways, and a rate that does not exist
    c8 = _lib.SileroCfg()
    c8.sample_rate = 8000
    bad = list(args)
    bad[18] = C.byref(c8)
    assert run(*bad) == -1 and b"8 kHz" in lib.vadx_last_error()
    keep[2].sampling_rate = 8000
    assert run(*args) == -1 and b"16 kHz" in lib.vadx_last_error()
    assert run(*bad) == -2                                                           # 8 kHz cfg, 8 kHz params: past the rate check
    keep[2].sampling_rate = 16000
    c8.sample_rate = 44100
    assert run(*bad) == -1 and b"44100" in lib.vadx_last_error()
    c8.sample_rate, c8.arithmetic = 0, 9
    assert run(*bad) == -1 and b"arithmetic" in lib.vadx_last_error()
    # table counts that cannot be one tick's
    for kw in (dict(groups=4), dict(groups=0), dict(tiles=2), dict(tiles=13), dict(n_runs=2)):
        a2, keep2, _, _ = _tick_args(lib, **kw)
        assert run(*a2) == -1 and b"counts of one tick" in lib.vadx_last_error(), kw
    a2, keep2, _, _ = _tick_args(lib)
    keep2[1].clips = 39
    assert run(*a2) == -1 and b"counts of one tick" in lib.vadx_last_error()
    assert lib.vadx_silero_stream_ragged_workspace_bytes(0, 4, 9) == 0 and lib.vadx_silero_stream_ragged_workspace_bytes(40, 257, 9) == 0
    assert lib.vadx_silero_stream_ragged_workspace_bytes(40, 4, 0) == 0


def test_c_level_planner_refuses_before_any_hip_call(lib):
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 255) & ~255
    ptr = lambda i: base + 16 * i                                                    # noqa: E731
    need = lib.vadx_silero_stream_plan_bytes(2000, 16)
    assert need >= 2 * (8 + 17 * 4) and lib.vadx_silero_stream_plan_bytes(2000, 257) == 0 and lib.vadx_silero_stream_plan_bytes(0, 4) == 0
    args = [ptr(0), ptr(1), 2000, 16, 512, 125, ptr(2), ptr(3), ptr(4), ptr(5), ptr(6), ptr(7), need - 1, None]
    plan = lib.vadx_silero_stream_plan
    assert plan(*args) == -2 and b"workspace" in lib.vadx_last_error()
    for i in (0, 1, 6, 7, 8, 9, 10, 11):
        bad = list(args)
        bad[i] = None
        assert plan(*bad) == -1 and b"NULL" in lib.vadx_last_error(), i
    for i, v, word in ((2, 0, b"streams"), (3, 0, b"max_windows"), (3, 257, b"max_windows"), (4, 500, b"window"), (5, 0, b"groups"),
                       (5, 126, b"groups")):
        bad = list(args)
        bad[i] = v
        assert plan(*bad) == -1 and word in lib.vadx_last_error(), (i, v)
