"""GPU: ragged ticks of the Silero streams (vadx_silero_stream_plan / vadx_silero_stream_run_ragged / VADIteratorBatch.step_ragged): every
stream delivers its own number of windows.  The device planner is pinned bitwise to its numpy mirror; scores fed in ragged ticks must be
bit for bit what clips() gives for each stream's concatenated audio, on every arithmetic and at both rates; the two tick forms share one
record."""
import ctypes as C

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, ragged, silero, weights

pytestmark = pytest.mark.gpu
SCALE = np.float32(0.000030517578)
CYCLE = [0, 1, 3, 4, 5, 15, 16, 17, 33]      # the run of four, the 16-step flush block, groups that mix long and short streams
WIN = {16000: 512, 8000: 256}
CANARY = 0x5A


@pytest.fixture(autouse=True, params=["f32", "split", "h2"])
def encoder(request):
    """Every test of this file runs on the three kernel sets (exact-f32 MFMAs, bf16 x 3, fp16 x 2)."""
    prev = silero.encoder_mode(request.param)
    yield request.param
    silero.encoder_mode(prev)


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234), weights_8k=weights.silero8k_synthetic(1234))


def pcm(S, windows, seed, rate=16000):
    return weights.burst_clips(S, windows * WIN[rate], seed=seed)


def schedule(totals, shift, cycle=CYCLE, cap=None):
    """Per-tick counts: stream s takes cycle[(shift[s] + tick) % len] windows, as far as its audio (or its budget `cap`) reaches."""
    left = np.asarray(totals, dtype=np.int64).copy() if cap is None else np.minimum(totals, cap).astype(np.int64)
    out, j = [], 0
    while left.any():
        c = np.minimum(np.asarray(cycle)[(np.asarray(shift) + j) % len(cycle)], left)
        out.append(c)
        left -= c
        j += 1
    return out


def rows_at(audio, done, counts, win):
    """The tick's samples [S, max(counts) * win]: row s = the next counts[s] windows of stream s (zeros behind them are never read)."""
    x = np.zeros((audio.shape[0], max(int(counts.max()), 1) * win), dtype=audio.dtype)
    for s, (d, c) in enumerate(zip(done, counts)):
        x[s, :c * win] = audio[s, d * win:(d + c) * win]
    return x


def feed(it, audio, ticks, win, as_list=False):
    """Run `ticks` (lists of counts) over `audio` from window 0 -> per stream the concatenated (kind, value, probs)."""
    S = audio.shape[0]
    done = np.zeros(S, dtype=np.int64)
    got = [[] for _ in range(S)]
    for j, c in enumerate(ticks):
        if as_list and j % 2:
            x, cc = [audio[s, done[s] * win:(done[s] + c[s]) * win] for s in range(S)], None
        else:
            x, cc = rows_at(audio, done, c, win), c
            x = torch.from_numpy(x) if j % 3 == 0 else x
        kind, value, probs, first = it.step_ragged(x, cc)
        assert np.array_equal(first, np.concatenate([[0], np.cumsum(c)]))
        for s in range(S):
            got[s].append((kind[first[s]:first[s + 1]], value[first[s]:first[s + 1]], probs[first[s]:first[s + 1]]))
        done += c
    return [tuple(torch.cat([g[i] for g in got[s]]) for i in range(3)) for s in range(S)]


# ------------------------------------------------------------------ 1. the planner alone
def guarded(n, dtype):
    """A device vector of n elements between two guards of 64 elements, everything filled with the canary byte."""
    buf = torch.full(((n + 128) * torch.empty(0, dtype=dtype).element_size(),), CANARY, dtype=torch.uint8, device="cuda").view(dtype)
    return buf, buf[64:64 + n]


def guards_intact(buf, n):
    b = buf.view(torch.uint8)
    e = buf.element_size()
    return bool((b[:64 * e] == CANARY).all() and (b[(64 + n) * e:] == CANARY).all())


def plan_on_device(counts, p, window):
    L = _lib.lib()
    S, slots = len(counts), 16 * p.groups
    host, at = p.staging()
    host[at["counts"]:at["counts"] + S] = counts            # (bad counts included: the plan's tables come from the clean ones)
    dev = torch.from_numpy(host).cuda()
    bufs = dict(first=guarded(S + 1, torch.int64), off=guarded(slots, torch.int64), len=guarded(slots, torch.int32),
                clip=guarded(slots, torch.int32), status=guarded(1, torch.int32))
    bufs["status"][1].zero_()
    need = L.vadx_silero_stream_plan_bytes(S, p.max_windows)
    ws = torch.full((need + 256,), CANARY, dtype=torch.uint8, device="cuda")
    rc = L.vadx_silero_stream_plan(dev.data_ptr() + 4 * at["counts"], dev.data_ptr() + 4 * at["bucket_first"], S, p.max_windows, window,
                                   p.groups, bufs["first"][1].data_ptr(), bufs["off"][1].data_ptr(), bufs["len"][1].data_ptr(),
                                   bufs["clip"][1].data_ptr(), bufs["status"][1].data_ptr(), ws.data_ptr(), need, _lib.stream_ptr())
    _lib.check(rc)
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        assert guards_intact(buf, view.numel()), name
    assert (ws[need:] == CANARY).all()
    return tuple(bufs[k][1].cpu().numpy() for k in ("first", "off", "len", "clip")) + (int(bufs["status"][1].item()),)


def plan_patterns(S):
    rng = np.random.default_rng(S)
    every = np.arange(S) % 257
    inter = rng.integers(1, 40, S)
    inter[::2] = 0
    one = np.zeros(S, np.int64)
    one[S // 2] = 7
    return {"equal": np.full(S, 5), "one active": one, "zeros interleaved": inter, "every count, shuffled": rng.permutation(every),
            "sorted up": np.sort(every), "sorted down": np.sort(every)[::-1].copy(), "jitter": rng.choice([0, 1, 3, 16], S)}


ONCE = pytest.mark.parametrize("encoder", ["f32"], indirect=True)      # the planner has no arithmetic
H2_ONLY = pytest.mark.parametrize("encoder", ["h2"], indirect=True)     # the range protocol belongs to the fp16 x 2 kernels


@ONCE
@pytest.mark.parametrize("S", [1, 15, 16, 17, 37, 1023, 1024, 1025, 70000])
def test_planner_is_bitwise_its_mirror(S):
    for name, counts in plan_patterns(S).items():
        for window in (512, 256):
            p = ragged.stream_plan(counts, window)
            if p.groups == 0:
                continue
            want = ragged.stream_slots_mirror(counts, p.bucket_first, p.groups, window, p.max_windows)
            got = plan_on_device(counts, p, window)
            assert got[4] == want[4] == 0, name
            for g, w, what in zip(got, want, ("probs_first", "slot_off", "slot_len", "slot_clip")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (name, window, what)
            assert np.array_equal(got[3][:p.active], np.argsort(-counts, kind="stable")[:p.active]), name


@ONCE
@pytest.mark.parametrize("S", [37, 1025, 70000])
def test_planner_takes_bad_counts_as_zero(S):
    rng = np.random.default_rng(S + 1)
    clean = rng.integers(0, 17, S)
    bad = clean.copy()
    where = rng.choice(S, size=min(S, 9), replace=False)
    bad[where[::2]], bad[where[1::2]] = -1, 257
    bad[where[0]] = 17                                        # just above max_windows = 16
    clean[where] = 0
    p = ragged.stream_plan(clean, 512, max_windows=16)
    want = ragged.stream_slots_mirror(clean, p.bucket_first, p.groups, 512, 16)
    got = plan_on_device(bad, p, 512)
    assert got[4] == 2 and want[4] == 0                        # the status bit; and every table as if the bad counts were 0
    for g, w in zip(got[:4], want[:4]):
        assert np.array_equal(g, w)


# ------------------------------------------------------------------ 2. ragged ticks == whole clips, bit for bit
_reference = {}


def reference(engine, encoder, rate, S=37):
    """Per stream (its own total length) the scores and final state of clips() over all its audio: computed once per arithmetic and rate."""
    key = (encoder, rate)
    if key not in _reference:
        totals = 34 + (np.arange(S) * 11) % 53
        a = pcm(S, int(totals.max()), seed=7 + rate, rate=rate)
        f = a.astype(np.float32) * SCALE
        ref = []
        for s in range(S):
            probs, state = engine.clips(torch.from_numpy(f[s:s + 1, :totals[s] * WIN[rate]]).cuda(), return_state=True, sampling_rate=rate)
            ref.append((probs[0].clone(), state[:, 0].clone()))
        _reference[key] = (totals, a, f, ref)
    return _reference[key]


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "int16"])
@pytest.mark.parametrize("rate", [16000, 8000])
def test_ragged_ticks_are_bitwise_clips(engine, encoder, rate, dtype, perm):
    totals, a, f, ref = reference(engine, encoder, rate)
    S = len(totals)
    shift = np.random.default_rng(3).permutation(S) if perm else np.arange(S)
    ticks = schedule(totals, shift)
    assert {int(c) for t in ticks for c in t} >= set(CYCLE)
    it = silero.VADIteratorBatch(engine, S, sampling_rate=rate)
    got = feed(it, a if dtype == "int16" else f, ticks, WIN[rate], as_list=perm)
    torch.cuda.synchronize()
    for s in range(S):
        assert torch.equal(got[s][2], ref[s][0]), s
        assert torch.equal(it.state[:, s], ref[s][1]), s


# ------------------------------------------------------------------ 3. the two tick forms share the record
@pytest.mark.parametrize("rate", [16000, 8000])
def test_tick_forms_interchange(engine, rate):
    S, W, win = 37, 24, WIN[rate]
    f = pcm(S, W, seed=21, rate=rate).astype(np.float32) * SCALE
    totals = np.full(S, W)
    uni = silero.VADIteratorBatch(engine, S, sampling_rate=rate)
    want, half = [], None
    for w0 in range(0, W, 4):
        if w0 == 12:
            half = uni.record.clone()
        want.append(uni.step(f[:, w0 * win:(w0 + 4) * win]))
    want = [torch.cat([w[i] for w in want], dim=1) for i in range(3)]
    # the same audio in ragged ticks: the same record, byte for byte
    rag = silero.VADIteratorBatch(engine, S, sampling_rate=rate)
    got = feed(rag, f, schedule(totals, np.arange(S)), win)
    torch.cuda.synchronize()
    assert torch.equal(rag.record, uni.record)
    for s in range(S):
        for i in range(3):
            assert torch.equal(got[s][i], want[i][s]), (s, i)
    # ragged up to window 12, then uniform
    a = silero.VADIteratorBatch(engine, S, sampling_rate=rate)
    feed(a, f, schedule(totals, np.arange(S), cap=12), win)
    assert torch.equal(a.record, half)
    b = silero.VADIteratorBatch(engine, S, sampling_rate=rate)
    b.load_record(a.record)
    for w0 in range(12, W, 4):
        out = b.step(f[:, w0 * win:(w0 + 4) * win])
        for i in range(3):
            assert torch.equal(out[i], want[i][:, w0:w0 + 4])
    assert torch.equal(b.record, uni.record)
    # uniform up to window 12, then ragged
    c = silero.VADIteratorBatch(engine, S, sampling_rate=rate)
    c.load_record(half)
    got = feed(c, f[:, 12 * win:], schedule(totals - 12, np.arange(S)[::-1]), win)
    assert torch.equal(c.record, uni.record)
    for s in range(S):
        for i in range(3):
            assert torch.equal(got[s][i], want[i][s, 12:]), (s, i)


@pytest.mark.parametrize("k", [1, 4, 5])
def test_equal_counts_are_a_uniform_tick(engine, k):
    S = 37
    f = pcm(S, 3 + k, seed=30 + k).astype(np.float32) * SCALE
    its = [silero.VADIteratorBatch(engine, S) for _ in range(2)]
    for it in its:
        it.step(f[:, :3 * 512])
    x = f[:, 3 * 512:]
    kind, value, probs = its[0].step(x)
    rk, rv, rp, first = its[1].step_ragged(x, np.full(S, k))
    assert np.array_equal(first, np.arange(S + 1) * k)
    assert torch.equal(rk.view(S, k), kind) and torch.equal(rv.view(S, k), value) and torch.equal(rp.view(S, k), probs)
    assert not torch.isnan(probs).any()
    assert torch.equal(its[0].record, its[1].record)


# ------------------------------------------------------------------ 4. idle streams and resets
def fields(rec, S):
    """The record's per-stream parts as byte rows [S, 1300]: h, c, context, current_sample, temp_end, triggered."""
    b = rec[:S * 1300]
    hc = b[:S * 1024].view(2, S, 512)
    return torch.cat([hc[0], hc[1], b[S * 1024:S * 1280].view(S, 256), b[S * 1280:S * 1288].view(S, 8), b[S * 1288:S * 1296].view(S, 8),
                      b[S * 1296:].view(S, 4)], dim=1)


def test_idle_streams_and_resets(engine):
    S = 40
    f = pcm(S, 7, seed=5).astype(np.float32) * SCALE
    x = torch.from_numpy(f).cuda()
    it = silero.VADIteratorBatch(engine, S)
    it.step_ragged(x[:, :3 * 512], np.full(S, 3))
    r1 = it.record.clone()
    it.reset_states([1, 7, 20])
    idle = [0, 7, 39]
    counts = np.full(S, 2)
    counts[idle] = 0
    _, _, p2, first2 = it.step_ragged(x[:, 3 * 512:5 * 512], counts)
    torch.cuda.synchronize()
    assert torch.equal(fields(it.record, S)[idle], fields(r1, S)[idle])              # an idle stream keeps its record bytes ...
    assert list(np.flatnonzero(it._pending)) == [7]                                   # ... and its pending reset
    fresh = engine.clips(x[[1, 20], 3 * 512:5 * 512])
    for j, s in enumerate((1, 20)):                                                   # a reset stream starts over at this tick
        assert torch.equal(p2[first2[s]:first2[s + 1]], fresh[j])
    whole = engine.clips(x)
    keep = [s for s in range(S) if s not in (0, 1, 7, 20, 39)]
    for s in keep:
        assert torch.equal(p2[first2[s]:first2[s + 1]], whole[s, 3:5])
    # tick 3: everyone; stream 7's reset applies now, streams 0 and 39 continue behind their tick 1 as if tick 2 had not happened
    _, _, p3, first3 = it.step_ragged(x[:, 5 * 512:], np.full(S, 2))
    assert not it._pending.any()
    assert torch.equal(p3[first3[7]:first3[8]], engine.clips(x[7:8, 5 * 512:])[0])
    cont = engine.clips(torch.cat([x[[0, 39], :3 * 512], x[[0, 39], 5 * 512:]], dim=1))
    assert torch.equal(p3[first3[0]:first3[1]], cont[0, 3:]) and torch.equal(p3[first3[39]:first3[40]], cont[1, 3:])
    for s in keep:
        assert torch.equal(p3[first3[s]:first3[s + 1]], whole[s, 5:])


# ------------------------------------------------------------------ 5. the device machine == S host VADIterators on the device's scores
class _Replay:
    def __init__(self):
        self.q = []

    def reset_states(self):
        pass

    def __call__(self, x, sr):
        return torch.tensor([[self.q.pop(0)]])


def test_call_ragged_matches_host_iterators(engine):
    S, ticks = 1024, 14
    rng = np.random.default_rng(9)
    a = pcm(S, 7 * ticks, seed=17)
    n_events = 0
    for kw, ckw in ((dict(), dict()), (dict(threshold=0.45, speech_pad_ms=30.03, min_silence_duration_ms=0), dict(return_seconds=True))):
        dev, twin = silero.VADIteratorBatch(engine, S, **kw), silero.VADIteratorBatch(engine, S, **kw)
        reps = [_Replay() for _ in range(S)]
        host = [silero.VADIterator(m, **kw) for m in reps]
        done = np.zeros(S, dtype=np.int64)
        for j in range(ticks):
            counts = rng.integers(0, 8, S)
            rs = rng.random(S) < 0.03
            dev.reset_states(rs), twin.reset_states(rs)
            x = rows_at(a, done, counts, 512)
            _, _, probs, first = twin.step_ragged(x, counts)
            probs = probs.cpu().numpy()
            res = dev.call_ragged(x, counts, **ckw)
            pend = rs.copy() if j == 0 else pend | rs
            for s in range(S):
                if counts[s] == 0:
                    assert res[s] == []
                    continue
                if pend[s]:
                    host[s].reset_states()
                reps[s].q = [float(v) for v in probs[first[s]:first[s + 1]]]
                want = [host[s](torch.zeros(512), **ckw) for _ in range(counts[s])]
                assert res[s] == want, (s, j)
                n_events += sum(w is not None for w in want)
            pend &= counts == 0
            done += counts
    assert n_events > 100


# ------------------------------------------------------------------ C-level ticks
class CTick:
    """One C-level ragged tick: the tables from stream_plan + vadx_silero_stream_plan, a workspace of EXACTLY the required bytes with a
    canary behind it, the packed outputs and the output record between canaries."""

    def __init__(self, engine, x, counts, rin, rate=16000):
        L = _lib.lib()
        self.engine, self.x, self.rate, self.S = engine, x, rate, len(counts)
        S, win = self.S, WIN[rate]
        p = self.plan = ragged.stream_plan(counts, win)
        host, at = p.staging()
        self.dev = torch.from_numpy(host).cuda()
        slots = 16 * p.groups
        self.first, self.off = torch.empty(S + 1, dtype=torch.int64, device="cuda"), torch.empty(slots, dtype=torch.int64, device="cuda")
        self.len, self.clip = (torch.empty(slots, dtype=torch.int32, device="cuda") for _ in range(2))
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.need = L.vadx_silero_stream_ragged_workspace_bytes(S, p.max_windows, p.tiles)
        self.ws = torch.full((self.need + 4096,), CANARY, dtype=torch.uint8, device="cuda")
        base = self.dev.data_ptr()
        _lib.check(L.vadx_silero_stream_plan(base + 4 * at["counts"], base + 4 * at["bucket_first"], S, p.max_windows, win, p.groups,
                                             self.first.data_ptr(), self.off.data_ptr(), self.len.data_ptr(), self.clip.data_ptr(),
                                             self.status.data_ptr(), self.ws.data_ptr(), self.need, _lib.stream_ptr()))
        self.rg = _lib.SileroRagged(self.off.data_ptr(), self.len.data_ptr(), self.clip.data_ptr(), base + 4 * at["gx_first"],
                                    base + 4 * at["grp_min_len"], base + 4 * at["wg_tab"], self.first.data_ptr(), self.status.data_ptr(),
                                    S, p.groups, p.n_runs, p.tiles)
        n = p.n_windows
        self.bufs = dict(probs=guarded(n, torch.float32), kind=guarded(n, torch.int8), value=guarded(n, torch.float64),
                         rec=guarded(rin.numel(), torch.uint8))
        self.rin = rin
        self.prm = _lib.SileroIterParams()
        self.prm.threshold, self.prm.sampling_rate, self.prm.min_silence_duration_ms, self.prm.speech_pad_ms = 0.5, rate, 100, 30

    def run(self, mode, reset=None):
        L, b = _lib.lib(), self.bufs
        self.bufs["rec"][1].zero_()                    # (the record's padding bytes: a fresh record has zeros there)
        pcm16 = self.x.dtype == torch.int16
        _lib.check(L.vadx_silero_stream_run_ragged(
            self.engine.blob(self.rate).data_ptr(), C.byref(self.prm), self.x.data_ptr(), int(pcm16), float(SCALE), self.x.stride(0), self.S,
            self.plan.max_windows, C.byref(self.rg), None if reset is None else reset.data_ptr(), self.rin.data_ptr(),
            b["rec"][1].data_ptr(), b["probs"][1].data_ptr(), b["kind"][1].data_ptr(), b["value"][1].data_ptr(), self.ws.data_ptr(),
            self.need, _lib.stream_ptr(), self.engine.cfg(mode, self.rate)))
        torch.cuda.synchronize()
        for name, (buf, view) in b.items():
            assert guards_intact(buf, view.numel()), name
        assert (self.ws[self.need:] == CANARY).all()
        assert int(self.status.item()) == 0
        return b["kind"][1], b["value"][1], b["probs"][1], b["rec"][1]


# ------------------------------------------------------------------ 6. work follows the counts
@pytest.mark.parametrize("rate", [16000, 8000])
def test_exact_workspace_and_canaries(engine, encoder, rate):
    S, win = 70, WIN[rate]
    rng = np.random.default_rng(11)
    f = pcm(S, 3 + 33, seed=12, rate=rate).astype(np.float32) * SCALE
    it = silero.VADIteratorBatch(engine, S, sampling_rate=rate)
    it.step(f[:, :3 * win])
    before = it.record.clone()
    counts = rng.choice(CYCLE, S)
    counts[:3] = [33, 0, 1]
    x = torch.from_numpy(f[:, 3 * win:]).cuda()
    tick = CTick(engine, x, counts, before, rate)
    assert tick.need < _lib.lib().vadx_silero_stream_workspace_bytes(S, 33)          # less than the rectangle's
    engine.range_flag(sampling_rate=rate)
    kind, value, probs, rec = tick.run(encoder)
    assert engine.range_flag(sampling_rate=rate)[0] == 0
    k2, v2, p2, _ = it.step_ragged(x, counts)
    assert torch.equal(kind, k2) and torch.equal(value, v2) and torch.equal(probs, p2) and torch.equal(rec, it.record)
    assert not torch.isnan(probs).any()


# ------------------------------------------------------------------ 7. the fp16 range protocol
@H2_ONLY
def test_range_protocol_recomputes_the_ragged_tick(engine):
    """A loud ragged tick on "h2" is the "split" tick from the same record, counted once; quiet ticks stay on "h2"."""
    S = 48
    rng = np.random.default_rng(3)
    counts = rng.choice([0, 1, 3, 4, 5], S)
    quiet = [torch.from_numpy(pcm(S, 5, seed=40 + j).astype(np.float32) * SCALE).cuda() for j in range(3)]
    loud = torch.from_numpy((rng.standard_normal((S, 5 * 512)) * 3000).astype(np.float32)).cuda()
    engine.range_flag()
    it = silero.VADIteratorBatch(engine, S)
    n0 = engine.range_fallbacks
    for j, x in enumerate([quiet[0], loud, quiet[1], quiet[2]]):
        before = it.record.clone()
        kind, value, probs, _ = it.step_ragged(x, counts)
        assert engine.range_fallbacks == n0 + (j >= 1)
        if j == 1:
            k2, v2, p2, rec = CTick(engine, x, counts, before).run("split")
            assert torch.equal(kind, k2) and torch.equal(value, v2) and torch.equal(probs, p2) and torch.equal(it.record, rec)
        assert not torch.isnan(probs).any()


@H2_ONLY
def test_unchecked_f16x2_ragged_tick_reads_invalid(engine):
    """Without the flag read, NaN and -1 appear for exactly the streams of the poisoned group -- the sixteen the deterministic plan puts
    into one group, wherever they are in stream order -- and their h in the record is NaN."""
    S = 64
    rng = np.random.default_rng(4)
    counts = rng.choice([0, 1, 2, 3, 4, 5, 9], S)
    order = np.argsort(-counts, kind="stable")[:int((counts > 0).sum())]
    group = order[16:32]                                          # group 1 of the plan
    assert len(group) == 16 and len(set(counts[group])) > 1 and not np.array_equal(np.sort(group), np.arange(group.min(), group.min() + 16))
    x = torch.from_numpy(pcm(S, 9, seed=60).astype(np.float32) * SCALE).cuda()
    x[torch.from_numpy(group).cuda()] = torch.from_numpy((rng.standard_normal((16, 9 * 512)) * 3000).astype(np.float32)).cuda()
    engine.range_flag()
    rin = torch.zeros(_lib.lib().vadx_silero_stream_state_bytes(S), dtype=torch.uint8, device="cuda")
    kind, value, probs, rec = CTick(engine, x, counts, rin).run("h2")
    assert engine.range_flag()[0] & 1
    first = np.concatenate([[0], np.cumsum(counts)])
    bad = np.zeros(S, bool)
    bad[group] = True
    per_window = torch.from_numpy(np.repeat(bad, counts)).cuda()
    assert torch.equal(torch.isnan(probs), per_window) and torch.equal(kind == -1, per_window)
    h = rec[:2 * S * 128 * 4].view(torch.float32).view(2, S, 128)[0]
    assert torch.equal(torch.isnan(h).all(dim=1).cpu(), torch.from_numpy(bad)) and torch.equal(torch.isnan(h).any(dim=1).cpu(), torch.from_numpy(bad))
    assert first[-1] == probs.numel()
