"""CPU: the host mirrors of vadx.tstable state Python's own arithmetic -- round(x, 3), round(x / sr, 1), vad_to_timestamps +
process_timestamps -- bit for bit, so the GPU tests may compare the device against either."""
import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import clips, tstable
from vadx import timestamps as ts


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("fs", [0.01, 0.02])
@pytest.mark.parametrize("length", [None, 0.025])
def test_round3_host_is_pythons_round_on_frame_products(fs, length):
    x = np.arange(400001, dtype=np.float32) * np.float32(fs)
    if length is not None:
        x = x + np.float32(length)
    assert x.dtype == np.float32
    want = np.array([round(v, 3) for v in x.tolist()])
    assert np.array_equal(bits(tstable.round3_host(x)), bits(want))


def test_round3_host_is_pythons_round_on_random_float32():
    x = (np.random.default_rng(3).random(200000) * 4000.0).astype(np.float32)
    want = np.array([round(v, 3) for v in x.tolist()])
    assert np.array_equal(bits(tstable.round3_host(x)), bits(want))


@pytest.mark.parametrize("sr", [16000, 8000])
def test_round1_host_is_pythons_round(sr):
    step = sr // 10
    rng = np.random.default_rng(sr)
    xs = np.concatenate([np.arange(300000, dtype=np.int64),                                   # every small index
                         step * np.arange(200000, dtype=np.int64) + step // 2,                # every tie
                         rng.integers(0, 1 << 40, 100000),                                    # anywhere
                         step * rng.integers(0, (1 << 40) // step, 100000) + step // 2])      # ties anywhere
    want = np.array([round(x / sr, 1) for x in xs.tolist()])
    assert np.array_equal(bits(tstable.round1_host(xs, sr)), bits(want))
    neg = -xs[:5000]
    assert np.array_equal(bits(tstable.round1_host(neg, sr)), bits(np.array([round(x / sr, 1) for x in neg.tolist()])))


def test_round1_host_refuses_other_rates():
    with pytest.raises(ValueError, match="16000 or 8000"):
        tstable.round1_host([1], 44100)


def _patterns(n, rng):
    yield np.zeros(n, np.uint8)                          # all speech
    yield np.ones(n, np.uint8)                           # all silence
    yield (np.arange(n) & 1).astype(np.uint8)            # alternating
    yield ((np.arange(n) + 1) & 1).astype(np.uint8)
    f = np.ones(n, np.uint8)
    f[n // 2:] = 0                                       # a run that ends exactly at n
    yield f
    for p in (0.5, 0.9, 0.98):
        yield (rng.random(n) < p).astype(np.uint8)
    yield np.repeat((rng.random(n // 7 + 1) < 0.5), 7)[:n].astype(np.uint8)


@pytest.mark.parametrize("fd", [0.01, 0.02])
@pytest.mark.parametrize("fusion,minimum", [(0.3, 0.2), (1.0, 0.5), (0, 0), (0.05, 0.03)])
def test_flags_host_is_flag_timestamps(fd, fusion, minimum):
    rng = np.random.default_rng(11)
    for n in (0, 1, 63, 64, 65, 127, 128, 129, 1095, 4097):
        for f in _patterns(n, rng):
            assert tstable.flags_host(f, fd, fusion, minimum) == clips.flag_timestamps(f, fd, fusion, minimum), (n, fd, fusion, minimum)
    f = np.full(300, 255, np.uint8)                       # filler counts as silence, as astype(bool) makes it
    f[10:50] = 0
    assert tstable.flags_host(f, fd, fusion, minimum) == clips.flag_timestamps(f, fd, fusion, minimum)


def test_fuse_host_is_process_timestamps_on_the_thresholds():
    """Rows whose durations and gaps sit on and beside 0.2 and 0.3 in double: one pass of the fuse is the reference's two."""
    fd = 0.01
    for a in range(0, 201, 7):
        for l1 in range(15, 36):
            for gap in range(25, 36):
                for l2 in (15, 19, 20, 21, 35):
                    b1, a2 = a + l1, a + l1 + gap
                    rows = [(a * fd, b1 * fd + fd), (a2 * fd, (a2 + l2) * fd + fd)]
                    assert tstable.fuse_host(rows, 0.3, 0.2) == ts.process_timestamps(rows, 0.3, 0.2)
    rng = np.random.default_rng(5)
    for _ in range(300):
        cuts = np.sort(rng.choice(4000, 40, replace=False)).reshape(-1, 2)
        rows = [(int(s) * fd, int(e) * fd + fd) for s, e in cuts]
        for fusion, minimum in ((0.3, 0.2), (1.0, 0.5), (0, 0), (0.05, 0.03)):
            assert tstable.fuse_host(rows, fusion, minimum) == ts.process_timestamps(rows, fusion, minimum)


def test_samples_host_is_the_two_existing_rules():
    from vadx import chunks
    rows = [(0.0, 0.57), (1.234, 2.5), (3.0000001, 4.99999)]
    assert tstable.samples_host(rows, 16000, "nearest") == chunks.from_seconds([rows], 16000)[0]
    assert tstable.samples_host(rows, 16000, "trunc") == ts.indices(rows, 16000)


def test_entry_points_validate_before_touching_the_device():
    """VADX_EINVAL for what the host can see, before any HIP call: this machine has no GPU, and the pointers below point nowhere."""
    import ctypes as C
    from vadx import _lib
    L, p = _lib.lib(), 0x10000
    bad = lambda: L.vadx_last_error().decode()                                    # noqa: E731
    prm = _lib.TsParams(frame_s=0.01, frame_shift=0.01, sampling_rate=16000)
    flags = lambda **k: L.vadx_timestamps_flags(C.byref(k.get("prm", prm)), k.get("flags", p), k.get("stride", 8), p, k.get("batch", 1),     # noqa: E731
                                                k.get("seconds", p), p, p, k.get("cap", 1), p, None)
    assert flags(cap=0) == -1 and "cap=0" in bad()
    assert flags(batch=0) == -1 and "batch=0" in bad()
    assert flags(flags=None) == -1 and "NULL" in bad()
    assert flags(seconds=p + 4) == -1 and "aligned" in bad()
    assert flags(stride=-1) == -1 and "stride=-1" in bad()
    assert flags(prm=_lib.TsParams(frame_s=0.0, sampling_rate=16000)) == -1 and "frame_s" in bad()
    assert flags(prm=_lib.TsParams(frame_s=0.01, sampling_rate=16000, sample_rule=2)) == -1 and "sample_rule=2" in bad()
    assert flags(prm=_lib.TsParams(frame_s=0.01, sampling_rate=16000, process=1, fusion_threshold=float("nan"))) == -1 and "NaN" in bad()
    assert flags(prm=_lib.TsParams(frame_s=0.01, sampling_rate=0)) == -1 and "sampling_rate=0" in bad()
    assert L.vadx_timestamps_frames(C.byref(prm), p, p, 0, p, p, 1, p, p, p, 1, p, None) == -1 and "cap_in=0" in bad()
    assert L.vadx_timestamps_frames(C.byref(_lib.TsParams(sampling_rate=16000)), p, p, 1, p, p, 1, p, p, p, 1, p, None) == -1 and "frame_shift" in bad()
    assert L.vadx_timestamps_samples(C.byref(prm), p, p, 0, p, 1, p, p, p, 1, p, None) == -1 and "cap_in=0" in bad()
    assert L.vadx_timestamps_samples(C.byref(_lib.TsParams(sampling_rate=44100)), p, p, 1, p, 1, p, p, p, 1, p, None) == -1 and "16000 or 8000" in bad()


def test_table_bytes_is_the_documented_layout():
    assert tstable.table_bytes(1, 1) == 64 and tstable.table_bytes(3, 5) == (16 + 32 * 15 + 12 + 15) // 16 * 16
