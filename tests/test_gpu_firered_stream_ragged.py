"""GPU: ragged ticks of the FireRed streams (FireRedStreamBatch.step_ragged over vadx_firered_stream_tick_ragged) on the three arithmetics.

Every comparison is bitwise.  The reference for a stream is always that stream ALONE in a FireRedStreamBatch(eng, 1, post), started from the
same record bytes (load_record) and advanced with the existing `step(chunks=c)`: probabilities, events, open_start, caches and the 32
header words.  Configs, weights, audio and record helpers are those of tests/test_gpu_firered_stream.py (imported, so the engines are
shared too)."""
import ctypes as C

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, audio_io, drivers, firered, ragged, weights
import test_gpu_firered_stream as base
from test_gpu_firered_stream import (CHUNK, DEFAULT, LONG_PAD, PADDED, POST, POST_G, SMALL, T, cfg_name, engine, gemm, oracle_decisions,  # noqa: F401
                                     random_record, samples, stream_audio)

pytestmark = pytest.mark.gpu
Batch = firered.FireRedStreamBatch


def stream_state(it, s=0):
    return it.caches[s].clone(), it.headers()[s].clone(), int(it.open_start[s])


def columns(probs, first, s, frames):
    return probs[:, int(first[s]) * frames:int(first[s + 1]) * frames]


def sub_record(it, rec, s, it1):
    """Stream s's bytes of `rec` (a record of `it`) as a record of the one-stream batch it1"""
    out = torch.zeros_like(it1.record)
    n = it._cache_floats // it.streams * 4
    out[:n] = rec[s * n:(s + 1) * n]
    out[it1._hdr_at:] = rec[it._hdr_at + s * 128:it._hdr_at + (s + 1) * 128]
    return out


def alone_from(eng, it, rec, s, audio_row, c, n, post):
    """Stream s alone from its bytes of `rec`, advanced by c chunks of n samples with `step`: (probs [odim, c * frames], events, state)"""
    it1 = Batch(eng, 1, post)
    it1.load_record(sub_record(it, rec, s, it1))
    p, ev = it1.step(audio_row[None, :c * n], c)
    return p[0].clone(), ev[0], stream_state(it1)


def check_stream(it, before, s, c, frames, probs, events, first, want):
    if c == 0:
        assert torch.equal(it.stream_bytes(it.record, s), it.stream_bytes(before, s)), s
        assert events[s] == [] and int(it.open_start[s]) == -1 and first[s] == first[s + 1], s
        return
    p, ev, (caches, hdr, opened) = want
    assert torch.equal(columns(probs, first, s, frames), p), s
    assert events[s] == ev and int(it.open_start[s]) == opened, s
    assert torch.equal(it.caches[s], caches) and torch.equal(it.headers()[s], hdr), s


# ------------------------------------------------------------------ one tick on random caches
TICK_COUNTS = {1: [112, 0, 100, 12, 50, 7, 3, 0, 1], 14: [8, 0, 6, 2, 5, 1, 0, 1], 15: [7, 0, 4, 3, 2, 1, 0, 1], 17: [6, 0, 4, 2, 3, 0, 2],
               37: [3, 0, 2, 1, 1, 0, 1], 56: [2, 0, 1, 1, 0, 1], 57: [1, 0, 1, 0, 1], 112: [1, 0, 1, 0, 1]}


def tick_case(key, frames, counts):
    eng, cap, n = engine(key), 112 // frames, samples(frames)
    counts = np.array(counts)
    S = len(counts)
    audio = stream_audio(S, int(counts.max()) * n, 77 + frames)
    it = Batch(eng, S, POST_G)
    rec = random_record(it, 5)[0]
    want = [alone_from(eng, it, rec, s, audio[s], int(c), n, POST_G) if c else None for s, c in enumerate(counts)]
    fallbacks = eng.blobs.range_fallbacks
    for group in (1, cap, 0):
        it = Batch(eng, S, POST_G)
        it.load_record(rec)
        probs, events, first = it.step_ragged(audio, counts, chunk=n, group=group)
        assert probs.shape == (eng.odim, int(counts.sum()) * frames) and bool(torch.isfinite(probs).all()), group
        assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)]))
        for s, c in enumerate(counts):
            check_stream(it, rec, s, int(c), frames, probs, events, first, want[s])
        assert np.array_equal(it.frames_done, counts * frames), group
    assert eng.blobs.range_fallbacks == fallbacks
    return want


@pytest.mark.parametrize("frames", sorted(TICK_COUNTS))
def test_one_ragged_tick_on_random_caches(gemm, frames):
    """A workgroup exactly full, one with a single stream, one mixing widths so that a stream starts on a column that is no multiple of
    16, an idle stream between two active ones, a partial last workgroup -- at group = 1, the capacity and 0."""
    counts, cap = np.array(TICK_COUNTS[frames]), 112 // frames
    _, order, wg = ragged.column_stream_plan(counts, cap, cap)
    sums = [int(counts[order[a:b]].sum()) for a, b in zip(wg[:-1], wg[1:])]
    starts = [int(counts[order[a:j]].sum()) * frames for a, b in zip(wg[:-1], wg[1:]) for j in range(a + 1, b)]
    assert cap in sums and 1 in np.diff(wg) and (counts[1:-1] == 0).any() and counts[0] and counts[-1]
    if cap >= 2:
        assert any(c % 16 for c in starts) and sums[-1] < cap, (sums, starts)
    want = tick_case(DEFAULT, frames, counts)
    if frames >= 14:
        assert any(w and (w[1] or w[2][2] >= 0) for w in want)               # the decisions that are compared say something


@pytest.mark.parametrize("frames", [14, 37])
@pytest.mark.parametrize("key", [SMALL, LONG_PAD, PADDED], ids=cfg_name)
def test_one_ragged_tick_at_other_widths(gemm, key, frames):
    tick_case(key, frames, TICK_COUNTS[frames])


# ------------------------------------------------------------------ a schedule
CHUNKS = [8, 8, 7, 6, 5, 4, 3, 2, 1]
PATTERN = np.array([[4, 0, 2, 1, 3, 0, 1, 2, 1],
                    [0, 3, 1, 2, 0, 4, 2, 0, 0],
                    [0, 0, 0, 0, 0, 0, 0, 0, 0],
                    [1, 2, 4, 0, 2, 0, 0, 0, 0],
                    [3, 0, 0, 3, 0, 0, 0, 0, 0]])
_ALONE = {}


def schedule_reference(gemm, eng, audio):
    """Each stream alone from the reset state through one-chunk `step` ticks"""
    if gemm not in _ALONE:
        ref = []
        for s, k in enumerate(CHUNKS):
            it1 = Batch(eng, 1, POST)
            parts, ev = [], []
            for j in range(k):
                p, e = it1.step(audio[s:s + 1, j * CHUNK:(j + 1) * CHUNK])
                parts.append(p[0])
                ev += e[0]
            ref.append((torch.cat(parts, dim=1), ev, it1.open_segments()[0], it1.stream_bytes(it1.record, 0).clone()))
        _ALONE[gemm] = ref
    return _ALONE[gemm]


@pytest.mark.parametrize("perm", [None, [3, 7, 0, 8, 1, 5, 2, 6, 4]], ids=["pattern", "permuted"])
def test_ragged_schedule(gemm, perm):
    eng, S = engine(DEFAULT), len(CHUNKS)
    audio = stream_audio(S, 8 * CHUNK, 6)
    ref = schedule_reference(gemm, eng, audio)
    pattern = PATTERN if perm is None else PATTERN[:, perm]
    it = Batch(eng, S, POST)
    left, pos = np.array(CHUNKS), np.zeros(S, np.int64)
    parts, events = [[] for _ in range(S)], [[] for _ in range(S)]
    seen = dict(zero=0, one=0, first_zero=False, fresh_many=False)
    taken = []
    for tick in range(40):
        if not left.any():
            break
        counts = np.minimum(pattern[tick % len(pattern)], left)
        taken.append(counts.copy())
        seen["first_zero"] |= tick == 0 and bool((counts == 0).any())
        seen["fresh_many"] |= bool(((pos == 0) & (counts > 1)).any())
        seen["zero"] += int(not counts.any())
        seen["one"] += int(np.count_nonzero(counts) == 1)
        rec = it.record
        x = np.zeros((S, 4 * CHUNK), np.int16)
        for s in range(S):
            x[s, :counts[s] * CHUNK] = audio[s, pos[s]:pos[s] + counts[s] * CHUNK]
        with _lib.trace() as tr:
            probs, ev, first = it.step_ragged(x, counts, chunk=CHUNK)
        if not counts.any():
            assert tr.calls == {} and it.record is rec and probs.shape == (1, 0)          # nothing launched, the record pointer unmoved
        for s in range(S):
            parts[s].append(columns(probs, first, s, 14))
            events[s] += ev[s]
        pos += counts * CHUNK
        left = left - counts
    assert not left.any()
    if perm is None:
        assert seen["first_zero"] and seen["fresh_many"] and seen["zero"] >= 1 and seen["one"] >= 1, seen
        last = np.array(taken)[:, 8]                                                 # the one-chunk stream: done in tick 0, idle to the end
        assert last[0] == 1 and len(last) >= 4 and not last[1:].any(), last
    opened = it.open_segments()
    closing = 0
    for s in range(S):
        p, ev, op, bytes_ = ref[s]
        got = torch.cat(parts[s], dim=1)
        assert torch.equal(got, p) and events[s] == ev and opened[s] == op, s
        assert torch.equal(it.stream_bytes(it.record, s), bytes_), s
        want, _, _ = oracle_decisions(got[0].cpu().numpy(), POST)
        assert events[s] + ([opened[s]] if opened[s] is not None else []) == want, s
        closing += bool(ev)
    print(f"ragged schedule: {closing} of {S} streams end a segment, {sum(o is not None for o in opened)} keep one open")
    assert 2 * closing >= S and any(o is not None for o in opened)
    assert np.array_equal(it.frames_done, np.array(CHUNKS) * 14)


# ------------------------------------------------------------------ interchange with `step`
def as_rect(probs, S):
    return probs.view(probs.shape[0], S, -1).permute(1, 0, 2)


@pytest.mark.parametrize("c", [1, 2, 4])
def test_equal_counts_are_step(gemm, c):
    eng, S = engine(DEFAULT), 9
    audio = stream_audio(S, 8 * CHUNK, 6)
    a, b = Batch(eng, S, POST), Batch(eng, S, POST)
    for j in range(2):
        x = audio[:, j * c * CHUNK:(j + 1) * c * CHUNK]
        pa, ea = a.step(x, c)
        pb, eb, first = b.step_ragged(x, np.full(S, c), chunk=CHUNK)
        assert torch.equal(as_rect(pb, S), pa) and ea == eb and torch.equal(a.open_start, b.open_start)
        assert torch.equal(a.record, b.record)


def test_step_and_step_ragged_interchange(gemm):
    eng, S = engine(DEFAULT), 9
    audio = stream_audio(S, 8 * CHUNK, 6)
    cut = lambda a, k: audio[:, a * CHUNK:(a + k) * CHUNK]                           # noqa: E731
    a, b, c = (Batch(eng, S, POST) for _ in range(3))
    want = [a.step(cut(0, 2), 2), a.step(cut(2, 1)), a.step(cut(3, 3), 3), a.step(cut(6, 1))]
    ones = lambda k: np.full(S, k)                                                  # noqa: E731
    got_b = [b.step(cut(0, 2), 2), b.step_ragged(cut(2, 1), ones(1), chunk=CHUNK), b.step(cut(3, 3), 3), b.step_ragged(cut(6, 1), ones(1), chunk=CHUNK)]
    got_c = [c.step_ragged(cut(0, 2), ones(2), chunk=CHUNK), c.step(cut(2, 1)), c.step_ragged(cut(3, 3), ones(3), chunk=CHUNK), c.step(cut(6, 1))]
    for got in (got_b, got_c):
        for w, g in zip(want, got):
            p = g[0] if len(g) == 2 else as_rect(g[0], S)
            assert torch.equal(p, w[0]) and g[1] == w[1]
    assert torch.equal(a.record, b.record) and torch.equal(a.record, c.record)
    assert a.open_segments() == b.open_segments() == c.open_segments()


# ------------------------------------------------------------------ idle streams and resets
def test_idle_streams_and_resets(gemm):
    eng, S = engine(DEFAULT), 3
    audio = stream_audio(S, 6 * CHUNK, 6)
    fresh = lambda s, a, k: alone_from(eng, Batch(eng, 1, POST), torch.zeros_like(Batch(eng, 1, POST).record), 0, audio[s, a * CHUNK:], k, CHUNK, POST)  # noqa: E731
    rows = lambda at, counts: [audio[s, at[s] * CHUNK:(at[s] + counts[s]) * CHUNK] for s in range(S)]       # noqa: E731
    it = Batch(eng, S, POST)
    # tick 1: stream 2 has no audio, and the explicit reset request for it is ignored
    probs, ev, first = it.step_ragged(rows([0, 0, 0], [2, 1, 0]), reset=[False, False, True], chunk=CHUNK)
    assert not bool(it.stream_bytes(it.record, 2).any()) and np.array_equal(it.frames_done, [28, 14, 0])
    assert torch.equal(columns(probs, first, 0, 14), fresh(0, 0, 2)[0])
    # a pending reset waits over a count of 0: stream 1 keeps its bytes ...
    it.reset_states([1])
    before = it.record.clone()
    probs, ev, first = it.step_ragged(rows([2, 1, 0], [1, 0, 3]), chunk=CHUNK)
    assert torch.equal(it.stream_bytes(it.record, 1), it.stream_bytes(before, 1)) and ev[1] == [] and int(it.open_start[1]) == -1
    assert torch.equal(columns(probs, first, 2, 14), fresh(2, 0, 3)[0]) and it._pending.tolist() == [False, True, False]
    # ... then applies: stream 1 hears its chunks 3 and 4 as a fresh stream
    before = it.record.clone()
    probs, ev, first = it.step_ragged(rows([3, 3, 3], [1, 2, 0]), chunk=CHUNK)
    p, e, (caches, hdr, opened) = fresh(1, 3, 2)
    assert torch.equal(columns(probs, first, 1, 14), p) and ev[1] == e and torch.equal(it.caches[1], caches) and torch.equal(it.headers()[1], hdr)
    assert torch.equal(it.stream_bytes(it.record, 2), it.stream_bytes(before, 2)) and not it._pending.any()
    assert np.array_equal(it.frames_done, [56, 28, 42])
    # a reset mid-run, requested with the tick
    probs, ev, first = it.step_ragged(rows([4, 5, 3], [2, 1, 1]), reset=[True, False, False], chunk=CHUNK)
    p, e, (caches, hdr, opened) = fresh(0, 4, 2)
    assert torch.equal(columns(probs, first, 0, 14), p) and ev[0] == e and torch.equal(it.caches[0], caches) and torch.equal(it.headers()[0], hdr)
    assert np.array_equal(it.frames_done, [28, 42, 56])


# ------------------------------------------------------------------ rectangle input against list input
def test_rectangle_and_list_inputs(gemm):
    eng, S = engine(DEFAULT), 6
    counts = np.array([3, 0, 1, 2, 0, 1])
    audio = stream_audio(S, 3 * CHUNK, 9)
    runs = []
    lst = [audio[s, :counts[s] * CHUNK] for s in range(S)]
    odd = torch.zeros((S, 3 * CHUNK + 1), dtype=torch.int16, device="cuda")
    odd[:, :3 * CHUNK] = T(audio).cuda()
    wide = T(audio).cuda()
    for x, cn, calls in ((lst, None, {}), (audio, counts, {"vadx_windows_gather": 1}), (wide, counts, {"vadx_windows_gather": 1}),
                         (odd[:, :3 * CHUNK], counts, {"vadx_windows_gather_any": 1})):
        it = Batch(eng, S, POST)
        it.load_record(random_record(it, 3)[0])
        with _lib.trace() as tr:
            probs, ev, first = it.step_ragged(x, cn, chunk=CHUNK)
        assert tr.calls == dict(calls, vadx_frontend_logmel=1, vadx_firered_stream_tick_ragged=1), tr.calls     # ONE net launch per tick
        runs.append((probs, ev, it.record.clone(), it.open_start.clone()))
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and r[1] == runs[0][1] and torch.equal(r[2], runs[0][2]) and torch.equal(r[3], runs[0][3])


# ------------------------------------------------------------------ range protocol, state_in
def test_range_protocol_and_state_in(gemm):
    """state_in is unchanged by a ragged tick; on fp16 x 2 a loud tick (test_gpu_firered_stream.py's recipe) counts one fallback and leaves
    what the same tick leaves on an engine pinned to bf16 x 3."""
    # (an engine of its own on fp16 x 2: the shared one's fallback count is asserted on by tests/test_gpu_firered_stream.py)
    eng, S = firered.FireRedEngine(base.weights_for(DEFAULT), CHUNK) if gemm == "h2" else engine(DEFAULT), 9
    counts = np.array([2, 1, 0, 3, 1, 0, 2, 1, 1])
    audio = stream_audio(S, 4 * CHUNK, 6)
    it = Batch(eng, S, POST)
    it.step(audio[:, :CHUNK])
    if gemm == "h2":
        it.caches[1, 0].fill_(3e5)
    src = it.record
    before = src.clone()
    fallbacks = eng.blobs.range_fallbacks
    probs, ev, first = it.step_ragged(audio[:, CHUNK:], counts, chunk=CHUNK)
    assert it.record is not src and torch.equal(src, before)
    if gemm != "h2":
        assert eng.blobs.range_fallbacks == fallbacks
        return
    assert eng.blobs.range_fallbacks == fallbacks + 1 and eng.blobs.mode() == "h2"
    eng_s = engine(DEFAULT, "split")
    other = Batch(eng_s, S, POST)
    other.load_record(before)
    probs_s, ev_s, _ = other.step_ragged(audio[:, CHUNK:], counts, chunk=CHUNK)
    assert eng_s.blobs.range_fallbacks == 0 and bool(torch.isfinite(probs).all())
    assert torch.equal(probs, probs_s) and ev == ev_s and torch.equal(it.open_start, other.open_start) and torch.equal(it.record, other.record)


# ------------------------------------------------------------------ the C entry point inside canary guards
GUARD = 256


class Guarded:
    """Device buffers of exact sizes inside one uint8 tensor of 0xA5 bytes, GUARD bytes around each"""

    def __init__(self, **sizes):
        self.at, n = {}, GUARD
        for k, b in sizes.items():
            self.at[k] = (n, b)
            n += (b + 15) // 16 * 16 + GUARD
        self.buf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        self.used = torch.zeros(n, dtype=torch.bool, device="cuda")
        for a, b in self.at.values():
            self.used[a:a + b] = True

    def view(self, k, dtype=torch.uint8):
        a, b = self.at[k]
        return self.buf[a:a + b].view(dtype)

    def ptr(self, k):
        return self.buf.data_ptr() + self.at[k][0]

    def guards_intact(self):
        return bool((self.buf[~self.used] == 0xA5).all())


def c_tick(eng, it, rec, logmel, frames, counts, row_first, slot_stream, wg_first, n_rows, post=POST_G):
    """vadx_firered_stream_tick_ragged on tables as given -> (Guarded outputs, status)"""
    S, odim = it.streams, eng.odim
    cap = 8 * frames
    g = Guarded(probs=odim * n_rows * frames * 4, segments=S * cap * 8, counts_out=S * 4, open_start=S * 4, record=rec.numel())
    tabs = [np.asarray(a, dtype=np.int32) for a in (counts, row_first, slot_stream, wg_first, [0])]
    tab = T(np.concatenate(tabs)).cuda()
    ptrs = [tab.data_ptr() + 4 * int(sum(len(a) for a in tabs[:i])) for i in range(5)]
    cfg, packed = eng.blobs.get()
    c = _lib.FireRedCfg.from_buffer_copy(cfg)
    c.frames = frames
    src = rec.clone()
    _lib.check(_lib.lib().vadx_firered_stream_tick_ragged(C.byref(c), packed.data_ptr(), logmel.data_ptr(), S, n_rows, ptrs[0], ptrs[1], ptrs[2],
                                                          ptrs[3], len(wg_first) - 1, C.byref(it._prm), None, src.data_ptr(), g.ptr("record"),
                                                          g.ptr("probs"), g.ptr("segments"), g.ptr("counts_out"), cap, g.ptr("open_start"),
                                                          ptrs[4], _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(src, rec) and g.guards_intact()
    return g, int(tab[-1].item())


class CCase:
    """S streams with `counts` chunks of `frames` frames on a random record: the log-mel rows, and every stream alone"""

    def __init__(self, eng, frames, counts, seed):
        self.eng, self.frames, self.counts, self.S = eng, frames, np.array(counts), len(counts)
        n = samples(frames)
        self.first = np.concatenate([[0], np.cumsum(self.counts)])
        self.n_rows = int(self.first[-1])
        audio = stream_audio(self.S, int(self.counts.max()) * n, seed)
        self.it = Batch(eng, self.S, POST_G)
        self.rec = random_record(self.it, 8)[0]
        self.want = [alone_from(eng, self.it, self.rec, s, audio[s], int(c), n, POST_G) if c else None for s, c in enumerate(self.counts)]
        rows = np.concatenate([audio[s, :self.counts[s] * n] for s in range(self.S)]).reshape(-1, n)
        self.logmel = eng._frontend_for(n).logmel(T(rows).cuda(), 1, n)

    def tick(self, slots, wg, counts=None, row_first=None):
        return c_tick(self.eng, self.it, self.rec, self.logmel, self.frames, self.counts if counts is None else counts,
                      self.first[:self.S] if row_first is None else row_first, slots, wg, self.n_rows)

    def check(self, g, live, copied):
        """streams `live` hold what they hold alone, `copied` their bytes of the record read; every other byte of every output is 0xA5"""
        it, rec, S = self.it, self.rec, self.S
        per, hdr_at = it._cache_floats // S * 4, it._hdr_at
        A5 = lambda t: bool((t == 0xA5).all())                                     # noqa: E731
        probs = g.view("probs", torch.float32).view(self.eng.odim, self.n_rows * self.frames)
        record, cnt, opened = g.view("record"), g.view("counts_out", torch.int32), g.view("open_start", torch.int32)
        segs = g.view("segments", torch.int32).view(S, -1, 2)
        for s in range(S):
            cols = columns(probs, self.first, s, self.frames)
            cache, hdr = record[s * per:(s + 1) * per], record[hdr_at + s * 128:hdr_at + (s + 1) * 128]
            if s in live:
                p, ev, (caches, h, op) = self.want[s]
                assert torch.equal(cols, p) and int(opened[s]) == op and int(cnt[s]) == len(ev), s
                assert [(int(a) * 0.01, int(b) * 0.01) for a, b in segs[s, :len(ev)].tolist()] == ev, s
                assert A5(segs[s, len(ev):].contiguous().view(torch.uint8)), s
                assert torch.equal(cache.view(torch.float32), caches.reshape(-1)) and torch.equal(hdr.view(torch.int32), h.reshape(-1)), s
                continue
            assert A5(cols.contiguous().view(torch.uint8)) and A5(segs[s].contiguous().view(torch.uint8)), s
            if s in copied:
                assert torch.equal(cache, rec[s * per:(s + 1) * per]) and torch.equal(hdr, rec[hdr_at + s * 128:hdr_at + (s + 1) * 128]), s
                assert int(cnt[s]) == 0 and int(opened[s]) == -1, s
            else:
                assert A5(cache) and A5(hdr) and A5(cnt[s:s + 1].view(torch.uint8)) and A5(opened[s:s + 1].view(torch.uint8)), s


def test_c_entry_point_in_canary_guards(gemm):
    S = 5
    case = CCase(engine(DEFAULT), 14, [2, 0, 3, 1, 2], 21)
    counts, first = case.counts, case.first
    everyone, plan = {0, 2, 3, 4}, ragged.column_stream_plan(counts, 8, 8)
    orders = {"identity": ([0, 2, 3, 4], [0, 2, 4]), "reversed": ([4, 3, 2, 0], [0, 3, 4]), "plan": (plan[1][:4].tolist(), plan[2].tolist()),
              "alone": ([0, 2, 3, 4], [0, 1, 2, 3, 4]), "one workgroup": ([2, 0, 3, 4], [0, 4])}
    for name, (slots, wg) in orders.items():
        g, status = case.tick(slots, wg)
        assert status == 0, name
        case.check(g, everyone, {1})
    # tables that lie: the slot is skipped, bit 1 raised, the neighbours right, nothing else written
    slots, wg = [0, 2, 3, 4], [0, 2, 4]
    for bad in (-1, 9):                                                             # a count below 0 and above the capacity: a stream without audio
        lie = counts.copy()
        lie[2] = bad
        g, status = case.tick(slots, wg, counts=lie)
        assert status == 2, bad
        case.check(g, everyone - {2}, {1, 2})
    lie = first[:S].copy()
    lie[3] = case.n_rows                                                            # rows past n_rows
    g, status = case.tick(slots, wg, row_first=lie)
    assert status == 2
    case.check(g, everyone - {3}, {1, 3})
    g, status = case.tick([0, S, 3, 4], wg)                                         # a slot_stream entry of S
    assert status == 2
    case.check(g, everyone - {2}, {1})                                              # stream 2 has audio and no slot: not written at all
    g, status = case.tick([0, 2, 3, 4], [0, 2, 1])                                  # a wg_first that runs backwards: the workgroup is skipped
    assert status == 2
    case.check(g, {0, 2}, {1})


def test_c_workgroup_of_113_columns(gemm):
    """Chunks of one frame: 56 + 56 + 1 chunks in one workgroup are 113 columns -- the third slot is skipped, the first two are right."""
    case = CCase(engine(DEFAULT), 1, [56, 0, 56, 1], 22)
    g, status = case.tick([0, 2, 3], [0, 3])
    assert status == 2
    case.check(g, {0, 2}, {1})
    g, status = case.tick([0, 2, 3], [0, 2, 3])
    assert status == 0
    case.check(g, {0, 2, 3}, {1})


# ------------------------------------------------------------------ stream_detect and the driver
DETECT_LENGTHS = [100, 399, 400, 2560, 2600, 2960, 5121, 12345, 2560 * 19 + 700]


def test_stream_detect_chunks_per_tick(gemm):
    eng = engine(DEFAULT)
    clips = [weights.burst_clips(1, n, seed=11 + n, sample_rate=4000)[0] for n in DETECT_LENGTHS]
    want, want_tracks = eng.stream_detect(clips, post=base.DETECT_POST, return_probs=True)
    assert [len(t) for t in want_tracks] == [0, 0, 1, 14, 14, 15, 29, 67, 19 * 14 + 2]      # per chunk, as the reference streams them
    for k in (3, 8):
        with _lib.trace() as tr:
            out, tracks = eng.stream_detect(clips, post=base.DETECT_POST, return_probs=True, chunks_per_tick=k)
        assert out == want, k
        assert all(np.array_equal(a, b) for a, b in zip(tracks, want_tracks)), k
        assert tr.calls["vadx_firered_stream_tick_ragged"] == -(-19 // k), (k, tr.calls)
    assert len(want[-1]) >= 2


def test_driver_chunks_per_tick(gemm, tmp_path):
    eng = engine(DEFAULT)
    files = []
    for k, n in enumerate([399, 2960, 12345, 2560 * 7 + 700]):
        files.append(str(tmp_path / f"c{k}.wav"))
        audio_io.save_wav(files[-1], weights.burst_clips(1, n, seed=11 + n, sample_rate=4000)[0], 16000)
    kw = dict(engine=eng, SMOOTH_WINDOW_SIZE=3, STREAM_VAD_THRESHOLD=0.36, PAD_START_FRAME=3, MIN_SPEECH_FRAME_STREAM=3,
              MAX_SPEECH_FRAME_STREAM=12, MIN_SILENCE_FRAME_STREAM=3, echo=lambda *a: None, batched=True)
    want = drivers.inference_firered_stream(files, **kw)
    assert drivers.inference_firered_stream(files, CHUNKS_PER_TICK=3, **kw) == want and any(want)
