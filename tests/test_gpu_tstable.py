"""GPU: vadx.tstable against the host code it replaces, bit for bit -- the f64 seconds viewed as int64, the int64 sample rows, the counts.
Every table is built inside a canary-filled buffer with guard regions on both sides: the guards must be intact afterwards, and so must
every row the call had no business writing (rows past a clip's count, the rows of a refused clip)."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, chunks, clips, silero, tstable, vadpost, weights
from vadx import timestamps as ts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, CANARY = 256, 0xA5
CANARY64 = int(np.frombuffer(bytes([CANARY] * 8), dtype=np.int64)[0])
CASES = [(0.3, 0.2), (1.0, 0.5), (0, 0), (0.05, 0.03)]
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 1095, 4097)


class Guarded:
    """storage for a (batch, cap) table inside canaries; `read(table)` checks them and returns the host arrays"""

    def __init__(self, batch, cap):
        self.need = tstable.table_bytes(batch, cap)
        self.whole = torch.full((GUARD + self.need + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
        self.storage = self.whole[GUARD:GUARD + self.need]

    def read(self, table):
        host = self.whole.cpu().numpy()
        assert np.all(host[:GUARD] == CANARY) and np.all(host[GUARD + self.need:] == CANARY), "a guard region was written"
        sec, smp, cnt = table.seconds.cpu().numpy(), table.samples.cpu().numpy(), table.counts.cpu().numpy()
        for b in range(table.batch):                         # rows past the count (clamped to cap) were not touched
            c = min(max(int(cnt[b]), 0), table.cap)
            assert np.all(sec[b, c:].view(np.int64) == CANARY64) and np.all(smp[b, c:] == CANARY64), f"clip {b}: a row past its count was written"
        head = table._head_t.cpu().numpy()
        assert head[2] == 0 and head[3] == 0
        return sec, smp, cnt, (int(head[0]), int(head[1]))


def flag_matrix(rows, tail=255):
    """rows (1-D uint8 arrays) -> (uint8 [B, S] with `tail` behind every row, n_flags)"""
    n = np.asarray([len(r) for r in rows], dtype=np.int32)
    m = np.full((len(rows), max(int(n.max()), 1)), tail, dtype=np.uint8)
    for b, r in enumerate(rows):
        m[b, :len(r)] = r
    return m, n


def run_flags(rows, fd, fusion, minimum, rule, cap=None, tail=255):
    m, n = flag_matrix(rows, tail)
    cap = cap or max(1, (m.shape[1] + 1) // 2)
    g = Guarded(len(rows), cap)
    tab = tstable.from_flags(torch.from_numpy(m).to(DEV), n, fd, fusion, minimum, 16000, rule, cap=cap, retry=False, storage=g.storage)
    return g.read(tab)


def assert_rows(got, want_lists, rule, sr=16000):
    sec, smp, cnt, head = got
    assert cnt.tolist() == [len(w) for w in want_lists]
    assert head == (0, max([len(w) for w in want_lists] + [0]))
    for b, w in enumerate(want_lists):
        want = np.asarray(w, dtype=np.float64).reshape(-1, 2)
        assert np.array_equal(sec[b, :len(w)].view(np.int64), want.view(np.int64)), f"clip {b}: seconds differ"
        idx = chunks.from_seconds([w], sr)[0] if rule == "nearest" else ts.indices(w, sr)
        assert smp[b, :len(w)].tolist() == [list(r) for r in idx], f"clip {b}: sample rows differ"


def patterns(n, rng):
    idx = np.arange(n)
    yield np.zeros(n, np.uint8)                              # all speech
    yield np.ones(n, np.uint8)                               # all silence
    yield (idx & 1).astype(np.uint8)                         # alternating every frame: the most runs
    yield ((idx + 1) & 1).astype(np.uint8)
    f = np.ones(n, np.uint8)
    f[n // 2:] = 0                                           # a run that ends exactly at n
    yield f
    yield (((idx + 3) % 64) >= 6).astype(np.uint8)           # a run across every 64-frame step boundary: [64k - 3, 64k + 3)
    yield (((idx + 30) % 128) >= 60).astype(np.uint8)        # long runs across every other boundary
    for p in (0.5, 0.98):
        yield (rng.random(n) < p).astype(np.uint8)
    yield np.repeat(rng.random(n // 9 + 1) < 0.5, 9)[:n].astype(np.uint8)
    yield np.repeat(rng.random(n // 40 + 1) < 0.5, 40)[:n].astype(np.uint8)


@pytest.mark.parametrize("fd", [0.01, 0.02])
@pytest.mark.parametrize("fusion,minimum", CASES)
def test_flags_every_length_and_pattern(fd, fusion, minimum):
    rng = np.random.default_rng(17)
    rows = [f for n in LENGTHS for f in patterns(n, rng)]
    want = [clips.flag_timestamps(r, fd, fusion, minimum) for r in rows]
    assert sum(len(w) for w in want) >= 20
    for rule in ("nearest", "trunc"):
        assert_rows(run_flags(rows, fd, fusion, minimum, rule), want, rule)
    # what lies behind n_flags is never read as speech: zeros there (flag 0 = speech) change nothing
    assert_rows(run_flags(rows, fd, fusion, minimum, "nearest", tail=0), want, "nearest")
    assert want == [tstable.flags_host(r, fd, fusion, minimum) for r in rows]


def test_flags_without_process_are_the_raw_runs():
    rng = np.random.default_rng(2)
    rows = [f for n in (65, 1095) for f in patterns(n, rng)]
    want = [ts.vad_to_timestamps(r.astype(bool), 0.01) for r in rows]
    assert_rows(run_flags(rows, 0.01, None, None, "nearest"), want, "nearest")


def test_flags_long_window_row_and_the_retry():
    """one row of 60 001 frames (a long-window FSMN clip) beside short ones; cap = 64 is too small for it: the head says by how much,
    nothing past cap is written, and the retry gives the whole table"""
    rng = np.random.default_rng(23)
    long = np.repeat(rng.random(60001 // 23 + 1) < 0.5, 23)[:60001].astype(np.uint8)
    rows = [np.zeros(100, np.uint8), long, (rng.random(1095) < 0.9).astype(np.uint8)]
    want = [clips.flag_timestamps(r, 0.01, 0.3, 0.2) for r in rows]
    most = max(len(w) for w in want)
    assert most > 64
    sec, smp, cnt, head = run_flags(rows, 0.01, 0.3, 0.2, "nearest", cap=64)
    assert cnt.tolist() == [len(w) for w in want] and head == (tstable.ST_OVERFLOW, most)
    for b, w in enumerate(want):
        k = min(len(w), 64)
        assert np.array_equal(sec[b, :k].view(np.int64), np.asarray(w[:k], dtype=np.float64).reshape(-1, 2).view(np.int64))
    m, n = flag_matrix(rows)
    tab = tstable.from_flags(torch.from_numpy(m).to(DEV), n, 0.01, 0.3, 0.2, cap=64)
    assert tab.cap == most and tab.head() == (0, most) and tab.lists() == want
    with pytest.raises(_lib.VadxError, match="more segments"):
        tstable.from_flags(torch.from_numpy(m).to(DEV), n, 0.01, 0.3, 0.2, cap=64, retry=False).lists()


def _sweep(a, l1, gap=None, l2=None, width=320):
    """flags uint8 [N, width] on the device with one run [a, a + l1) or two, the second [a + l1 + gap, a + l1 + gap + l2)"""
    pos = torch.arange(width, device=DEV).unsqueeze(0)
    a, b1 = a.unsqueeze(1), (a + l1).unsqueeze(1)
    speech = (pos >= a) & (pos < b1)
    if gap is not None:
        a2 = (a.squeeze(1) + l1 + gap).unsqueeze(1)
        speech |= (pos >= a2) & (pos < a2 + l2.unsqueeze(1))
    return (~speech).to(torch.uint8)


def _expect_sweep(a, l1, gap, l2, fd, fusion, minimum):
    """numpy float64, one IEEE operation at a time as Python does them -> (counts [N], seconds [N, 2, 2])"""
    s1, e1 = a * fd, (a + l1) * fd + fd
    a2 = a + l1 + gap
    s2, e2 = a2 * fd, (a2 + l2) * fd + fd
    k1, k2 = (e1 - s1) >= minimum, (e2 - s2) >= minimum
    fuse = k1 & k2 & ((s2 - e1) <= fusion)
    cnt = np.where(fuse, 1, k1.astype(np.int64) + k2)
    rows = np.zeros((len(a), 2, 2))
    rows[:, 0, 0] = np.where(k1, s1, s2)
    rows[:, 0, 1] = np.where(fuse, e2, np.where(k1, e1, e2))
    rows[:, 1, 0], rows[:, 1, 1] = s2, e2
    return cnt, rows


def test_flags_threshold_sweep():
    """Durations and gaps ON and beside min_duration = 0.2 and fusion_threshold = 0.3 in double -- what an FMA in b * fd + fd, or a > for
    a >=, gets wrong: every single run (a, len), a = 0 .. 200, len = 15 .. 35, and every pair of such runs 25 .. 35 frames apart."""
    fd, fusion, minimum = 0.01, 0.3, 0.2
    g = np.meshgrid(np.arange(201), np.arange(15, 36), np.arange(25, 36), np.arange(15, 36), indexing="ij")
    a, l1, gap, l2 = (x.reshape(-1).astype(np.int64) for x in g)
    N = len(a)
    assert N == 201 * 21 * 11 * 21
    dev = lambda v: torch.from_numpy(v).to(DEV)                                   # noqa: E731
    flags = _sweep(dev(a), dev(l1), dev(gap), dev(l2))
    tab = tstable.from_flags(flags, None, fd, fusion, minimum, cap=2, retry=False)
    assert tab.head() == (0, 2)
    cnt, sec = tab.counts.cpu().numpy(), tab.seconds.cpu().numpy()
    want_cnt, want = _expect_sweep(a, l1, gap, l2, fd, fusion, minimum)
    assert set(np.unique(want_cnt).tolist()) == {0, 1, 2} and np.array_equal(cnt, want_cnt)
    for k in (0, 1):
        live = want_cnt > k
        assert np.array_equal(sec[live, k].view(np.int64), want[live, k].view(np.int64))
    # the vectorised expectation is the reference's own code: a strided sample of the cases, and every case on a threshold's edge
    edge = np.flatnonzero(((l1 == 19) | (l1 == 20)) & ((gap == 29) | (gap == 30)) & (l2 == 20) & (a % 10 == 7))
    pick = np.concatenate([np.arange(0, N, 9973), edge])
    for i, f in zip(pick.tolist(), flags[dev(pick)].cpu().numpy()):
        w = clips.flag_timestamps(f, fd, fusion, minimum)
        assert len(w) == want_cnt[i] and np.array_equal(np.asarray(w).reshape(-1, 2).view(np.int64), want[i, :len(w)].view(np.int64))
    # single runs
    a1, n1 = (x.reshape(-1).astype(np.int64) for x in np.meshgrid(np.arange(201), np.arange(15, 36), indexing="ij"))
    f1 = _sweep(dev(a1), dev(n1)).cpu().numpy()
    want1 = [clips.flag_timestamps(r, fd, fusion, minimum) for r in f1]
    assert {len(w) for w in want1} == {0, 1}
    assert_rows(run_flags(list(f1), fd, fusion, minimum, "trunc", cap=2), want1, "trunc")


def test_a_clip_is_itself_in_any_company():
    rng = np.random.default_rng(31)
    mine = np.repeat(rng.random(50) < 0.5, 23)[:1095].astype(np.uint8)
    others = [f for n in (64, 129, 4097) for f in patterns(n, rng)]
    want = clips.flag_timestamps(mine, 0.01, 0.3, 0.2)
    assert len(want) > 3
    for at in (0, 1, 3, 4, 5, len(others)):                                  # every lane of a workgroup, first and last of the batch
        rows = others[:at] + [mine] + others[at:]
        sec, smp, cnt, _ = run_flags(rows, 0.01, 0.3, 0.2, "nearest")
        assert cnt[at] == len(want) and np.array_equal(sec[at, :len(want)].view(np.int64), np.asarray(want).view(np.int64))
    sec, _, cnt, _ = run_flags([mine], 0.01, 0.3, 0.2, "nearest")
    assert cnt[0] == len(want) and np.array_equal(sec[0, :len(want)].view(np.int64), np.asarray(want).view(np.int64))


# ---- FRAMES ---------------------------------------------------------------------------------------------------------------------------
def _tracks(ns, seed):
    """seeded block tracks f32 [B, max n]: even rows end in speech (the last segment ends at n), odd rows in silence"""
    rng = np.random.default_rng(seed)
    S = max(ns)
    tr = np.repeat(rng.random((len(ns), S // 31 + 1)) < 0.5, 31, axis=1)[:, :S].astype(np.float32) * 0.9 + 0.05
    for b, n in enumerate(ns):
        tr[b, max(0, n - 45):n] = 0.95 if b % 2 == 0 else 0.05
        tr[b, n:] = 0.0
    return tr


@pytest.mark.parametrize("shift,length", [(0.01, 0.025), (0.02, None), (0.01, None), (0.02, 0.025)])
def test_frames_against_segments_to_seconds(shift, length):
    post = (5, 0.4, 20, 2000, 20, 5, 0) if shift == 0.01 else (3, 0.5, 10, 1000, 10, 3, 0)
    pp = vadpost.VadPostprocessor(*post, frame_shift_s=shift, frame_length_s=length, device=DEV)
    ns = [n for n in (1, 98, 559, 400000) for _ in range(6)]
    end = lambda n: float(np.float32(n) * np.float32(shift) + np.float32(length or 0))   # noqa: E731
    durs = [(None, None, end(n) - 0.003, end(n) - 0.003, end(n) + 1.0, end(n) + 1.0)[k % 6] for k, n in enumerate(ns)]
    _, segs, counts = pp.process_batch(torch.from_numpy(_tracks(ns, 41)).to(DEV), n_frames=ns)
    sg, cn = segs.cpu().numpy(), counts.cpu().numpy()
    at_n = [bool(cn[b]) and int(sg[b, cn[b] - 1, 1]) == ns[b] for b in range(len(ns))]
    assert any(at_n) and not all(a for a, n in zip(at_n, ns) if n > 98) and cn.max() > 64
    want = [pp.segments_to_seconds(sg[b, :cn[b]].tolist(), ns[b], durs[b]) for b in range(len(ns))]
    for rule in ("nearest", "trunc"):
        g = Guarded(len(ns), segs.shape[1])
        tab = tstable.from_frames(pp, segs, counts, ns, durs, 16000, rule, retry=False, storage=g.storage)
        assert_rows(g.read(tab), want, rule)
    assert tstable.from_frames(pp, segs, counts, ns, durs).lists() == want
    # a cap too small: the head's largest count is right, nothing past cap is written, the retry gives the full table
    g = Guarded(len(ns), 3)
    sec, _, cnt, head = g.read(tstable.from_frames(pp, segs, counts, ns, durs, cap=3, retry=False, storage=g.storage))
    assert head == (tstable.ST_OVERFLOW, int(cn.max())) and np.array_equal(cnt, cn)
    tab = tstable.from_frames(pp, segs, counts, ns, durs, cap=3)
    assert tab.cap == int(cn.max()) and tab.lists() == want
    # with the optional process_timestamps pass
    got = tstable.from_frames(pp, segs, counts, ns, durs, fusion_threshold=1.0, min_duration=0.5).lists()
    assert got == [ts.process_timestamps(w, 1.0, 0.5) for w in want] and got != want


def test_frames_of_a_clip_without_frames():
    pp = vadpost.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0, device=DEV)
    segs = torch.zeros((2, 4, 2), dtype=torch.int32, device=DEV)
    segs[:, 0, 1] = 30
    tab = tstable.from_frames(pp, segs, torch.tensor([1, 1], dtype=torch.int32), [0, 30], [1.0, None])
    assert tab.lists() == [[], pp.segments_to_seconds([(0, 30)], 30, None)]


# ---- SAMPLES --------------------------------------------------------------------------------------------------------------------------
def _sample_tables(sr):
    """int64 [64, 64, 2]: every tie sample step * m + step / 2 for m < 4096 as a start; ends random, on ties, and beyond the clip"""
    rng = np.random.default_rng(sr)
    step = sr // 10
    ties = (step * np.arange(4096, dtype=np.int64) + step // 2).reshape(64, 64)
    segs = np.zeros((64, 64, 2), np.int64)
    segs[:, :, 0] = ties
    segs[:, :, 1] = ties + np.where(rng.random((64, 64)) < 0.5, step * rng.integers(1, 50, (64, 64)), rng.integers(1, 80000, (64, 64)))
    segs[1::4] = np.sort(rng.integers(0, 1 << 40, (16, 64, 2)), axis=2)                 # anywhere below 2^40
    segs[2::4, :, :] += rng.integers(0, 3, (16, 64, 2)) - 1                             # beside the ties
    lens = segs[:, :, 1].max(axis=1) + 1000
    lens[::3] = segs[::3, 32, 1]                                                       # ends beyond len: capped by len / sr
    counts = rng.integers(0, 65, 64).astype(np.int32)
    counts[:2] = 64, 0
    return segs, counts, lens


@pytest.mark.parametrize("sr", [16000, 8000])
def test_samples_against_finish(sr):
    segs, counts, lens = _sample_tables(sr)
    sd, cd = torch.from_numpy(segs).to(DEV), torch.from_numpy(counts).to(DEV)
    want = silero._finish(sd, cd, lens, sr, True, 1, 1)
    pairs = [[(d["start"], d["end"]) for d in w] for w in want]
    g = Guarded(64, 64)
    tab = tstable.from_samples(sd, cd, lens, sr, retry=False, storage=g.storage)
    assert_rows(g.read(tab), pairs, "nearest", sr)
    assert tstable.from_samples(sd, cd, lens, sr).lists() == want
    # the mirror says the same
    flat = segs[0, :, 0]
    assert np.array_equal(tstable.round1_host(flat, sr).view(np.int64), np.array([round(x / sr, 1) for x in flat.tolist()]).view(np.int64))


@pytest.mark.parametrize("sr", [16000, 8000])
def test_samples_then_process_timestamps(sr):
    """sorted rows whose gaps and durations are multiples of half a tenth of a second: what the Silero driver fuses"""
    rng = np.random.default_rng(sr + 1)
    half = sr // 20
    edges = np.cumsum(rng.integers(1, 9, (32, 128)) * half + (rng.random((32, 128)) < 0.2), axis=1).astype(np.int64)
    segs = edges.reshape(32, 64, 2)
    counts = rng.integers(1, 65, 32).astype(np.int32)
    lens = edges[:, -1] + 5
    sd, cd = torch.from_numpy(segs).to(DEV), torch.from_numpy(counts).to(DEV)
    raw = silero._finish(sd, cd, lens, sr, True, 1, 1)
    for fusion, minimum in ((0.3, 0.25), (0.1, 0.1), (0, 0)):
        want = [ts.process_timestamps([(d["start"], d["end"]) for d in w], fusion, minimum) for w in raw]
        assert any(0 < len(w) < c for w, c in zip(want, counts)) or fusion == 0
        g = Guarded(32, 64)
        tab = tstable.from_samples(sd, cd, lens, sr, fusion, minimum, retry=False, storage=g.storage)
        assert_rows(g.read(tab), want, "nearest", sr)


def test_samples_refuse_another_time_resolution_by_name():
    sd, cd = torch.zeros((1, 1, 2), dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="time_resolution=2"):
        tstable.from_samples(sd, cd, [100], 16000, time_resolution=2)
    model = silero.load_silero_vad(onnx=True, use_cpu=True, path="synthetic:1234")
    with pytest.raises(ValueError, match="time_resolution=2"):
        silero.get_speech_timestamps_table(np.zeros((1, 16000), np.float32), model, time_resolution=2)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _refused(run, good_counts, bad):
    """`run(storage)` built a table in which the clips `bad` must be refused alone"""
    g = Guarded(len(good_counts), 8)
    sec, smp, cnt, head = g.read(run(g.storage))                # (read also checks that a clip with count 0 has no written row)
    assert head[0] == tstable.ST_BAD_CLIP
    for b, c in enumerate(good_counts):
        assert cnt[b] == (0 if b in bad else c)
    return sec, smp


def test_flags_refusals():
    rng = np.random.default_rng(3)
    rows = [np.repeat(rng.random(10) < 0.5, 30).astype(np.uint8) for _ in range(6)]
    rows[0][:40], rows[5][:40] = 0, 0
    m, n = flag_matrix(rows)
    want = [clips.flag_timestamps(r, 0.01, 0.3, 0.2) for r in rows]
    for bad_n in (-1, m.shape[1] + 1, -2 ** 31, 2 ** 31 - 1):
        nb = n.copy()
        nb[2], nb[4] = bad_n, bad_n
        sec, _ = _refused(lambda st: tstable.from_flags(torch.from_numpy(m).to(DEV), nb, 0.01, 0.3, 0.2, cap=8, retry=False, storage=st),
                          [len(w) for w in want], {2, 4})
        for b in (0, 1, 3, 5):
            assert np.array_equal(sec[b, :len(want[b])].view(np.int64), np.asarray(want[b]).reshape(-1, 2).view(np.int64))
    with pytest.raises(_lib.VadxError, match="outside its table"):
        tstable.from_flags(torch.from_numpy(m).to(DEV), nb, 0.01, 0.3, 0.2).lists()


def test_frames_and_samples_refusals():
    pp = vadpost.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0, device=DEV)
    segs = torch.tensor([[[10 * k, 10 * k + 5] for k in range(4)]] * 5, dtype=torch.int32, device=DEV)
    for counts, ns, bad in (([2, 5, 3, 4, 1], [100] * 5, {1}), ([2, -1, 3, 4, 1], [100] * 5, {1}), ([2, 4, 3, 4, 1], [100, 100, 100, -1, 100], {3})):
        sec, _ = _refused(lambda st: tstable.from_frames(pp, segs, torch.tensor(counts, dtype=torch.int32), ns, None, cap=8, retry=False, storage=st),
                          counts, bad)
        assert np.array_equal(sec[0, :2].view(np.int64), np.asarray(pp.segments_to_seconds([(0, 5), (10, 15)], 100)).view(np.int64))
    s64 = segs.to(torch.int64) * 1000
    for counts, lens, bad in (([2, 5, 3, 4, 1], [10 ** 6] * 5, {1}), ([2, 4, 3, -7, 1], [10 ** 6] * 5, {3}),
                              ([2, 4, 3, 4, 1], [10 ** 6, 10 ** 6, -1, 10 ** 6, 10 ** 6], {2})):
        cd = torch.tensor(counts, dtype=torch.int32, device=DEV)
        _, smp = _refused(lambda st: tstable.from_samples(s64, cd, lens, 16000, cap=8, retry=False, storage=st), counts, bad)
        assert smp[4, 0].tolist() == [0, 4800]                  # round(5000 / 16000, 1) = 0.3 s


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
LENS = (16000, 48000, 29000)


def _cut_equal(table, lists, audio_i16, lengths, sr=16000):
    pcm = torch.from_numpy(np.ascontiguousarray(audio_i16)).to(DEV)
    a, ao = chunks.collect_chunks_batch(table.chunks_table(), pcm, lengths=lengths)
    b, bo = chunks.collect_chunks_batch(chunks.from_seconds(lists, sr), pcm, lengths=lengths)
    assert torch.equal(a, b) and torch.equal(ao, bo)
    return int(a.numel())


def _padded(cl):
    out = np.zeros((len(cl), max(len(c) for c in cl)), np.int16)
    for b, c in enumerate(cl):
        out[b, :len(c)] = c
    return out


@pytest.mark.parametrize("name", ["fsmn", "firered", "marblenet", "dfsmn"])
def test_detect_table_is_detect(name):
    from vadx import dfsmn, firered, fsmn, marblenet
    cl = [weights.burst_clips(1, n, seed=700 + k)[0] for k, n in enumerate(LENS)]
    arr = weights.burst_clips(2, 32000, seed=710)
    nz, nz2 = np.random.default_rng(5).standard_normal((3, 20000)), np.random.default_rng(6).standard_normal((3, 20000))
    if name == "fsmn":
        eng = fsmn.FsmnEngine("synthetic:1234")
        calls = [((cl,), dict(pad_noise=nz)), ((arr,), dict(pad_noise=nz[:2]))]
    elif name == "firered":
        eng = firered.FireRedEngine("synthetic:1234")
        calls = [((cl,), dict(pad_noise=nz)), ((arr,), dict(pad_noise=nz[:2]))]
    elif name == "marblenet":
        eng = marblenet.MarbleNetEngine("synthetic:1234")
        calls = [((cl,), {}), ((arr,), {}), ((cl,), dict(window_len=16000, pad_noise=nz))]
    else:
        eng = dfsmn.DfsmnEngine("synthetic:1234")
        far = [weights.burst_clips(1, n, seed=720 + k)[0] for k, n in enumerate(LENS)]
        calls = [((cl, far, nz, nz2), {}), ((arr, weights.burst_clips(2, 32000, seed=730), nz[:2], nz2[:2]), {})]
    for args, kw in calls:
        want = eng.detect(*args, **kw)
        table = eng.detect_table(*args, **kw)
        assert table.lists() == want
        audio = args[0]
        lengths = [len(c) for c in audio]
        cut = _cut_equal(table, want, _padded(audio) if isinstance(audio, list) else audio, lengths)
        print(f"{name}: segments per clip {[len(w) for w in want]}, {cut} samples of speech")
        assert eng.detect_table(*args, sample_rule="trunc", **kw).samples[0, :len(want[0])].tolist() == [list(r) for r in ts.indices(want[0], 16000)]


def test_silero_table_is_the_batch_call_and_the_drivers_pass():
    model = silero.load_silero_vad(onnx=True, use_cpu=True, path="synthetic:1234")
    cl = [weights.burst_clips(1, n, seed=740 + k)[0] for k, n in enumerate(LENS)]
    pcm = _padded(cl)
    audio = pcm.astype(np.float32) / 32768.0
    lengths = [len(c) for c in cl]
    for a, ln in ((audio, lengths), (audio[:2, :16000], None)):
        want = silero.get_speech_timestamps_batch(a, model, lengths=ln, return_seconds=True)
        assert silero.get_speech_timestamps_table(a, model, lengths=ln).lists() == want
        fused = [ts.process_timestamps([(d["start"], d["end"]) for d in w], 0.3, 0.25) for w in want]
        table = silero.get_speech_timestamps_table(a, model, lengths=ln, fusion_threshold=0.3, min_duration=0.25)
        assert [[(d["start"], d["end"]) for d in w] for w in table.lists()] == fused
        _cut_equal(table, fused, pcm[:len(a), :a.shape[1]], ln or [a.shape[1]] * len(a))
    assert silero.get_speech_timestamps_table(np.zeros((2, 0), np.float32), model).lists() == [[], []]
