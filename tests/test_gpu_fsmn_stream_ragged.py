"""GPU: ragged ticks of the FSMN streams (FsmnStreamBatch.step_ragged over vadx_fsmn_stream_windows_ragged / vadx_fsmn_stream_run_ragged)
against the whole-clip path (FsmnEngine.flags on each stream alone, bit for bit), the chained boundary calls (FsmnEngine.run, caches bit for
bit) and the rectangular tick (`step`, every byte of the record).  Eight streams of 1, 1, 2, 3, 4, 5, 7 and 9 windows of T = 101 frames (the
64 + 48-frame tile split); nothing depends on S beyond one workgroup per stream.  Every comparison is bitwise."""
import ctypes as C

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, drivers, fsmn, ragged, weights
from vadx import audio_io
from oracle import postproc as opp

pytestmark = pytest.mark.gpu
L, SEED = 16000, 1234
WS = (1, 1, 2, 3, 4, 5, 7, 9)
S = len(WS)
PATTERN = (0, 2, 1, 4, 0, 3, 1, 2)         # the fixed pattern over {0, 1, 2, 3, 4}: stream s reads it from position s (or perm[s])
PERM = (5, 0, 1, 4, 2, 6, 3, 7)
GUARD, FILL = 0xA5, 0x5A


@pytest.fixture(autouse=True, params=["f32", "split", "h2"])
def gemm(request):
    """Every test of this file runs on the three arithmetics of the dense layers: exact-f32 MFMAs, bf16 x 3 and fp16 x 2 split products (the default)."""
    prev = _lib.gemm_mode(request.param)
    yield request.param
    _lib.gemm_mode(prev)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


_CACHE = {}


def engine():
    if "eng" not in _CACHE:
        _CACHE["eng"] = fsmn.FsmnEngine(weights.fsmn_synthetic(SEED))
    return _CACHE["eng"]


def grid(lb_s):
    lb = int(lb_s * 16000 // 160)
    return lb, L - (lb + 1) * 160


def clips_for(lb_s):
    """(raw int16 clips, noise rows): clip s is 700 samples short of W_s windows of this grid, bursts of 0.25-1 s (burst_clips at half its
    segment lengths, so that one-second windows hold both kinds)."""
    _, stride = grid(lb_s)
    raw = [weights.burst_clips(1, (w - 1) * stride + L - 700, seed=SEED + 17 * s, sample_rate=8000)[0] for s, w in enumerate(WS)]
    noise = np.random.default_rng(9).standard_normal((S, 1000))
    return raw, noise


def audio(lb_s):
    """padded[s]: stream s's int16 audio, peak-normalised and padded to its own window grid: W_s windows"""
    if ("audio", lb_s) not in _CACHE:
        _, stride = grid(lb_s)
        raw, noise = clips_for(lb_s)
        padded = [fsmn.pad_to_window_grid(opp.normalize_to_int16(raw[s].astype(np.float32)), L, stride, noise[s]) for s in range(S)]
        assert [(len(p) - L) // stride + 1 for p in padded] == list(WS)
        _CACHE["audio", lb_s] = padded
    return _CACHE["audio", lb_s]


def reference(gemm, lb_s):
    """Per stream, on that stream ALONE through the whole-clip path: (flags u8 [W_s * slide + lb], trace f32 [W_s], caches 4 x [128, 19] after
    W_s chained run() calls with the noise floor fed back from the trace).  Computed once per (arithmetic, look-back) and never written."""
    if ("ref", gemm, lb_s) not in _CACHE:
        eng, padded = engine(), audio(lb_s)
        _, stride = grid(lb_s)
        out = []
        for s in range(S):
            f, tr = eng.flags(T(padded[s][None]), WS[s], look_backward_s=lb_s, return_noise=True)
            out.append([f[0].clone(), tr[0].clone(), None])
        assert eng.blobs.mode() == gemm
        caches = [torch.zeros(S, 128, 19) for _ in range(4)]
        res = [c.clone().to(eng.device) for c in caches]
        noise_in = torch.full((S,), float(np.float32(30.0 + 10.0) * np.float32(0.1)))
        for j in range(max(WS)):
            live = [s for s in range(S) if WS[s] > j]
            x = np.stack([padded[s][j * stride:j * stride + L] for s in live])
            _, cout, _ = eng.run(T(x), [res[l][live] for l in range(4)], np.ones(len(live), np.float32), noise_in[live])
            for l in range(4):
                res[l][live] = cout[l]
            for s in live:
                noise_in[s] = out[s][1][j]
        for s in range(S):
            out[s][2] = [res[l][s].clone() for l in range(4)]
        _CACHE["ref", gemm, lb_s] = out
    return _CACHE["ref", gemm, lb_s]


def schedule(perm=None, zero_tick=2):
    """Ticks of per-stream counts: PATTERN read from the stream's own position, clipped to the windows left, until everyone is through;
    one tick in which every count is 0 is put in at `zero_tick`."""
    left, ticks, t = np.array(WS), [], 0
    while left.any():
        c = np.array([min(PATTERN[(t + (s if perm is None else perm[s])) % len(PATTERN)], left[s]) for s in range(S)])
        t += 1
        if not c.any():
            continue
        ticks.append(c)
        left = left - c
    ticks.insert(zero_tick, np.zeros(S, dtype=np.int64))
    return ticks


def tick(it, rows, pos, counts, reset=None, as_list=False, extra=0, device=False):
    """One ragged tick: stream s gets its next samples_needed_ragged samples of rows[s] from pos[s] on."""
    counts = np.asarray(counts)
    need = it.samples_needed_ragged(counts, reset)
    if as_list:
        x = [np.ascontiguousarray(rows[s][pos[s]:pos[s] + need[s]]) for s in range(it.streams)]
    else:
        x = np.zeros((it.streams, int(need.max()) + extra), np.int16)
        for s in range(it.streams):
            x[s, :need[s]] = rows[s][pos[s]:pos[s] + need[s]]
        if device:
            x = T(x).to(it.engine.device)
    for s in range(it.streams):
        pos[s] += int(need[s])
    return it.step_ragged(x, None if as_list else counts, reset=reset)


def test_schedule_covers_the_cases():
    """The properties the schedules are there for (no device work)."""
    for perm in (None, PERM):
        ticks = np.stack(schedule(perm))
        assert ticks.min() >= 0 and ticks.max() == 4 and np.array_equal(ticks.sum(0), WS)
        first = [ticks[:, s][np.flatnonzero(ticks[:, s])[0]] for s in range(S)]
        assert (ticks[0] == 0).any()                                       # a stream whose first tick is 0
        assert max(first) > 1                                              # a fresh stream starting with n > 1
        last = [np.flatnonzero(ticks[:, s])[-1] for s in range(S)]
        assert min(last) < len(ticks) - 2                                  # one finishes while others go on, and sits at 0 to the end
        assert (ticks.sum(1) == 0).any()                                   # a tick in which every count is 0
        assert ((ticks > 0).sum(1) == 1).any()                             # a tick in which only one stream has audio


@pytest.mark.parametrize("lb_s", [0.3, 0.0])
@pytest.mark.parametrize("perm", [None, PERM])
def test_ragged_schedules_are_bitwise_flags(gemm, lb_s, perm):
    eng, padded, ref = engine(), audio(lb_s), reference(gemm, lb_s)
    lb, stride = grid(lb_s)
    slide = eng.T - lb
    fallbacks = eng.blobs.range_fallbacks
    it = fsmn.FsmnStreamBatch(eng, S, look_backward_s=lb_s)
    pos, got, tails, traces = [0] * S, [[] for _ in range(S)], [None] * S, [[] for _ in range(S)]
    for counts in schedule(perm):
        before = it.record
        flags, tail, first = tick(it, padded, pos, counts)
        n = int(counts.sum())
        assert flags.shape == (n, slide) and tail.shape == (S, lb) and flags.dtype == tail.dtype == torch.uint8
        assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)])) and it.noise_trace.shape == (n,)
        if n == 0:
            assert it.record is before and bool((tail == 255).all())        # nothing was launched, the record stays where it is
        for s in range(S):
            if counts[s]:
                got[s].append(flags[first[s]:first[s + 1]].reshape(-1))
                traces[s].append(it.noise_trace[first[s]:first[s + 1]])
                tails[s] = tail[s].clone()
            else:
                assert bool((tail[s] == 255).all())
    assert pos == [len(p) for p in padded]
    assert np.array_equal(it.windows_done, WS)
    for s in range(S):
        assert torch.equal(torch.cat(got[s] + [tails[s]]), ref[s][0]), s
        assert torch.equal(torch.cat(traces[s]), ref[s][1]), s
        for l in range(4):
            assert torch.equal(it.caches[s, l], ref[s][2][l]), (s, l)
    assert eng.blobs.range_fallbacks == fallbacks and eng.blobs.mode() == gemm


def test_reference_is_not_vacuous(gemm):
    """Each flag value makes up at least 10 % of the reference flags, and at least five streams' rows hold both: a wrong carry or a frozen
    vote cannot hide in all-silence rows."""
    for lb_s in (0.3, 0.0):
        ref = reference(gemm, lb_s)
        allf = torch.cat([r[0] for r in ref]).cpu().numpy()
        ones = float(allf.mean())
        both = sum(1 for r in ref if 0 < int(r[0].sum()) < r[0].numel())
        print(f"lb_s={lb_s}: flags {allf.size}, silence {ones:.3f}, streams with both values {both}")
        assert set(np.unique(allf)) == {0, 1} and 0.10 <= ones <= 0.90 and both >= 5


LONG = [s for s in range(S) if WS[s] >= 4]            # the streams that can do four windows in uniform ticks


@pytest.mark.parametrize("lb_s", [0.3, 0.0])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_equal_counts_equal_step(gemm, lb_s, k):
    eng, padded = engine(), audio(lb_s)
    rows, n = [padded[s] for s in LONG], len(LONG)
    a, b = fsmn.FsmnStreamBatch(eng, n, look_backward_s=lb_s), fsmn.FsmnStreamBatch(eng, n, look_backward_s=lb_s)
    pa, pb = [0] * n, [0] * n
    for _ in range(4 // k):
        need = a.samples_needed(k)
        x = np.stack([rows[s][pa[s]:pa[s] + need[s]] for s in range(n)])
        pa = [pa[s] + int(need[s]) for s in range(n)]
        f1, t1 = a.step(x, k)
        f2, t2, first = tick(b, rows, pb, np.full(n, k))
        assert pa == pb and np.array_equal(first, np.arange(n + 1) * k)
        assert torch.equal(f1.reshape(n * k, -1), f2) and torch.equal(t1, t2) and torch.equal(a.noise_trace.reshape(-1), b.noise_trace)
        assert torch.equal(a.record, b.record)


def test_the_two_tick_forms_interchange(gemm):
    """step -> step_ragged -> step and step_ragged -> step -> step_ragged over the same audio end with the record of four uniform ticks."""
    eng, padded = engine(), audio(0.3)
    rows, n = [padded[s] for s in LONG], len(LONG)

    def run(forms):
        it, pos = fsmn.FsmnStreamBatch(eng, n), [0] * n
        for form, k in forms:
            if form == "step":
                need = it.samples_needed(k)
                x = np.stack([rows[s][pos[s]:pos[s] + need[s]] for s in range(n)])
                pos = [pos[s] + int(need[s]) for s in range(n)]
                it.step(x, k)
            else:
                tick(it, rows, pos, np.full(n, k))
        assert np.array_equal(it.windows_done, np.full(n, 4))
        return it.record
    want = run([("step", 1)] * 4)
    assert torch.equal(run([("step", 1), ("ragged", 2), ("step", 1)]), want)
    assert torch.equal(run([("ragged", 1), ("step", 2), ("ragged", 1)]), want)


def test_idle_streams_and_resets(gemm):
    eng, padded, ref = engine(), audio(0.3), reference(gemm, 0.3)
    lb, stride = grid(0.3)
    slide = eng.T - lb
    it = fsmn.FsmnStreamBatch(eng, S)
    pos = [0] * S
    tick(it, padded, pos, [1, 1, 1, 1, 1, 1, 1, 1])
    # a stream with count 0 keeps every byte; its tail reads 255
    before = it.record.clone()
    _, tail, _ = tick(it, padded, pos, [0, 0, 1, 0, 1, 1, 0, 1])
    for s in (0, 1, 3, 6):
        assert torch.equal(it.stream_bytes(it.record, s), it.stream_bytes(before, s)) and bool((tail[s] == 255).all()), s
    assert not torch.equal(it.stream_bytes(it.record, 2), it.stream_bytes(before, 2))
    # reset_states on stream 6, then a tick with count 0 (the request waits, the record stays), then one with count 2: from its start again
    it.reset_states([6])
    before = it.record.clone()
    assert it.samples_needed_ragged([0] * 6 + [0, 1])[6] == 0 and it.samples_needed_ragged([0] * 6 + [2, 0])[6] == L + stride
    tick(it, padded, pos, [0, 0, 0, 0, 0, 0, 0, 1])
    assert torch.equal(it.stream_bytes(it.record, 6), it.stream_bytes(before, 6))
    pos[6] = 0
    flags, _, first = tick(it, padded, pos, [0, 0, 0, 0, 0, 0, 2, 0])
    assert torch.equal(flags[first[6]:first[7]].reshape(-1), ref[6][0][:2 * slide])
    assert it.windows_done[6] == 2
    # a reset on a stream with n > 0 mid-run: stream 7 hears stream 5's audio from its start; an explicit request on idle stream 4 is ignored
    rows = list(padded)
    rows[7], pos[7] = padded[5], 0
    mask = np.zeros(S, bool)
    mask[[4, 7]] = True
    before = it.record.clone()
    flags, _, first = tick(it, rows, pos, [0, 0, 0, 0, 0, 0, 0, 3], reset=mask)
    assert torch.equal(flags[first[7]:first[8]].reshape(-1), ref[5][0][:3 * slide])
    assert torch.equal(it.stream_bytes(it.record, 4), it.stream_bytes(before, 4))
    flags, tail, first = tick(it, rows, pos, [0, 0, 0, 0, 1, 0, 0, 2])
    assert torch.equal(torch.cat([flags[first[7]:first[8]].reshape(-1), tail[7]]), ref[5][0][3 * slide:])
    assert torch.equal(flags[first[4]:first[5]].reshape(-1), ref[4][0][2 * slide:3 * slide])          # stream 4 went on where it was
    assert np.array_equal(it.windows_done, [1, 1, 2, 1, 3, 2, 2, 5])


def test_sample_layouts_give_the_same_bytes(gemm):
    """Samples as a host array, a device tensor, rows of odd length (the 16-byte staging copy) and a list of arrays."""
    eng, padded = engine(), audio(0.3)
    plans = [[1, 0, 1, 3, 1, 0, 4, 2], [0, 1, 1, 0, 3, 2, 0, 4]]
    outs = []
    for kw in (dict(), dict(device=True), dict(extra=3), dict(as_list=True)):
        it, pos, res = fsmn.FsmnStreamBatch(eng, S), [0] * S, []
        for counts in plans:
            flags, tail, first = tick(it, padded, pos, counts, **kw)
            res += [flags, tail, it.noise_trace, T(first)]
        outs.append(res + [it.record])
    for o in outs[1:]:
        assert all(torch.equal(x, y) for x, y in zip(o, outs[0]))
    it = fsmn.FsmnStreamBatch(eng, S)
    need = it.samples_needed_ragged(plans[0])
    rows = [padded[s][:need[s]] for s in range(S)]
    rows[3] = padded[3][:need[3] - 1]
    with pytest.raises(ValueError, match=r"samples\[3\]"):
        it.step_ragged(rows)
    assert not bool(it.record.any())


# ---- the C level: one tick with every buffer inside guard regions ---------------------------------------------------------------------------
def c_tick(eng, lb_s, rec_in, rows, counts, *, true_counts=None, win_first=None, order=None, n_windows=None, max_windows=None):
    """One ragged tick through the C entry points.  Every buffer the two new calls read or write lies in one arena of GUARD bytes, each
    region of exactly its documented size with GUARD bytes on both sides; outputs start as FILL.  -> dict of host arrays + status.  The
    samples and sizes follow `true_counts` (default: counts), the tables hold `counts` / `win_first` as given."""
    t, dev = torch, eng.device
    lb, stride = grid(lb_s)
    slide, S_ = eng.T - lb, len(rows)
    true_counts = np.asarray(counts if true_counts is None else true_counts, dtype=np.int64)
    honest_first = np.concatenate([[0], np.cumsum(true_counts)])
    n = int(honest_first[-1]) if n_windows is None else n_windows
    mw = int(true_counts.max()) if max_windows is None else max_windows
    row = (max(len(r) for r in rows) + 7) // 8 * 8
    nb = _lib.lib().vadx_fsmn_stream_state_bytes(S_, lb)
    sizes = dict(samples=S_ * row * 2, counts=4 * S_, win_first=4 * (S_ + 1), win_stream=4 * n, order=4 * S_, status=4, wbuf=n * L * 2,
                 flags=n * slide, tail=S_ * lb, trace=4 * n, rec_in=nb, rec_out=nb)
    at, off = {}, 256
    for k, v in sizes.items():
        at[k] = off
        off += (v + 255) // 256 * 256 + 256
    arena = t.full((off,), GUARD, dtype=t.uint8, device=dev)
    inside, orig = np.zeros(off, bool), {}

    def put(name, host_bytes):
        a = np.frombuffer(np.ascontiguousarray(host_bytes).tobytes(), np.uint8)
        assert a.size == sizes[name], name
        orig[name] = a
        arena[at[name]:at[name] + a.size] = T(a.copy()).to(dev)
        inside[at[name]:at[name] + a.size] = True
    x = np.zeros((S_, row), np.int16)
    for s in range(S_):
        x[s, :len(rows[s])] = rows[s]
    put("samples", x)
    put("counts", np.asarray(counts, np.int32))
    put("win_first", np.asarray(honest_first if win_first is None else win_first, np.int32))
    put("win_stream", np.repeat(np.arange(S_), true_counts).astype(np.int32)[:n])
    put("order", np.asarray(np.arange(S_) if order is None else order, np.int32))
    put("status", np.zeros(1, np.int32))
    put("rec_in", rec_in.cpu().numpy())
    for name in ("wbuf", "flags", "tail", "trace", "rec_out"):
        put(name, np.full(sizes[name], FILL, np.uint8))
    p = {k: arena.data_ptr() + v for k, v in at.items()}
    Lb = _lib.lib()
    lp = fsmn._loop_params(lb)
    with t.cuda.device(dev):
        _lib.check(Lb.vadx_fsmn_stream_windows_ragged(p["samples"], row, S_, n, mw, L, lb, p["counts"], p["win_first"], p["win_stream"], None,
                                                      p["rec_in"], p["rec_out"], p["wbuf"], p["status"], _lib.stream_ptr()))
        wbuf = arena[at["wbuf"]:at["wbuf"] + sizes["wbuf"]].view(t.int16).view(n, L)
        logmel, db = eng.features(wbuf, 1, L)
        dims, packed = eng.blobs.get(eng.blobs.mode())
        _lib.check(Lb.vadx_fsmn_stream_run_ragged(C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), S_, n, mw, C.byref(lp),
                                                  p["counts"], p["win_first"], None if order is None else p["order"], None, p["rec_in"],
                                                  p["rec_out"], p["flags"], p["tail"] if lb else None, p["trace"], p["status"],
                                                  _lib.stream_ptr()))
    host = arena.cpu().numpy()
    assert bool((host[~inside] == GUARD).all()), "a guard byte was written"
    out = {k: host[at[k]:at[k] + sizes[k]].copy() for k in sizes}
    for k in ("samples", "counts", "win_first", "win_stream", "order", "rec_in"):      # the inputs are read-only
        assert np.array_equal(out[k], orig[k]), k
    out["status"] = int(out["status"].view(np.uint32)[0])
    out["flags"] = out["flags"].reshape(n, slide)
    out["tail"] = out["tail"].reshape(S_, lb)
    out["first"] = honest_first
    return out


def rec_of(it, rec_bytes, s):
    """stream s's bytes of a host record"""
    return it.stream_bytes(T(rec_bytes), s).numpy()


def primed_record(eng, padded, pos):
    """A record in which every stream has done one window (a Python tick), so that the C-level ticks below start from carries"""
    it = fsmn.FsmnStreamBatch(eng, S)
    tick(it, padded, pos, np.ones(S, np.int64))
    return it, it.record.clone()


def c_rows(it, padded, pos, counts):
    need = it.samples_needed_ragged(counts)
    return [padded[s][pos[s]:pos[s] + need[s]] for s in range(S)]


def test_c_level_order_neighbours_and_guards(gemm):
    """The same tick with order = identity (NULL), reversed and the plan's: bytewise equal outputs and records, every guard intact; and
    a stream's bytes equal those of a batch holding that stream alone."""
    eng, padded = engine(), audio(0.3)
    lb, _ = grid(0.3)
    pos = [0] * S
    it, rec = primed_record(eng, padded, pos)
    counts = np.array([0, 0, 1, 2, 0, 4, 3, 2])
    rows = c_rows(it, padded, pos, counts)
    base = c_tick(eng, 0.3, rec, rows, counts)
    assert base["status"] == 0 and not (base["flags"] == FILL).any() and not (base["wbuf"] == FILL).all()
    _, _, plan = ragged.window_stream_plan(counts)
    for order in (np.arange(S)[::-1], plan):
        o = c_tick(eng, 0.3, rec, rows, counts, order=order)
        for k in ("wbuf", "flags", "tail", "trace", "rec_out", "status"):
            assert np.array_equal(o[k], base[k]), k
    # the Python tick is this tick
    flags, tail, _ = it.step_ragged(np.stack([np.pad(r, (0, max(map(len, rows)) - len(r))) for r in rows]), counts)
    assert np.array_equal(flags.cpu().numpy(), base["flags"]) and np.array_equal(tail.cpu().numpy(), base["tail"])
    assert np.array_equal(it.record.cpu().numpy(), base["rec_out"])
    # one stream alone, from a zero record: its flags, tail, trace and record bytes are those it has among seven neighbours
    zero = torch.zeros_like(rec)
    fresh = fsmn.FsmnStreamBatch(eng, S)
    counts = np.array([1, 0, 2, 1, 0, 3, 1, 4])
    rows = [padded[s][:n] for s, n in enumerate(fresh.samples_needed_ragged(counts))]
    full = c_tick(eng, 0.3, zero, rows, counts)
    one = fsmn.FsmnStreamBatch(eng, 1)
    for s in (2, 7):
        alone = c_tick(eng, 0.3, torch.zeros_like(one.record), [rows[s]], counts[s:s + 1])
        a, b = full["first"][s], full["first"][s + 1]
        assert np.array_equal(alone["flags"], full["flags"][a:b]) and np.array_equal(alone["tail"][0], full["tail"][s])
        assert np.array_equal(alone["trace"], full["trace"][4 * a:4 * b])
        assert np.array_equal(rec_of(one, alone["rec_out"], 0), rec_of(fresh, full["rec_out"], s))


def test_c_level_lying_tables_are_harmless(gemm):
    """Counts of -1 and max_windows + 1, a win_first that points past n_windows and an order entry of S reach the device only through the C
    ABI.  The kernels' own checks make them harmless: the status bit is set, the lying stream counts as 0 (record copied bit for bit, tail
    255, no flag row written), every other stream's bytes are the honest tick's and every guard is intact.  (A stream that no order entry
    names is not served: the run kernel writes nothing of it.)"""
    eng, padded = engine(), audio(0.3)
    lb, _ = grid(0.3)
    pos = [0] * S
    it, rec = primed_record(eng, padded, pos)
    true = np.array([0, 0, 1, 1, 0, 3, 1, 2])
    rows = c_rows(it, padded, pos, true)
    honest = c_tick(eng, 0.3, rec, rows, true)
    first, n, mw = honest["first"], int(true.sum()), int(true.max())
    assert honest["status"] == 0

    def others_equal(o, liar):
        for s in range(S):
            if s == liar:
                continue
            a, b = first[s], first[s + 1]
            assert np.array_equal(o["flags"][a:b], honest["flags"][a:b]) and np.array_equal(o["tail"][s], honest["tail"][s]), s
            assert np.array_equal(o["trace"][4 * a:4 * b], honest["trace"][4 * a:4 * b]), s
            assert np.array_equal(rec_of(it, o["rec_out"], s), rec_of(it, honest["rec_out"], s)), s

    lies = []
    for bad in (-1, mw + 1):
        c = true.copy()
        c[2] = bad
        lies.append((2, dict(counts=c)))
    wf = first.copy()
    wf[S] = n + 1
    lies.append((S - 1, dict(counts=true, win_first=wf)))
    for liar, kw in lies:
        o = c_tick(eng, 0.3, rec, rows, kw.pop("counts"), true_counts=true, **kw)
        assert o["status"] & 2
        a, b = first[liar], first[liar + 1]
        assert np.array_equal(rec_of(it, o["rec_out"], liar), rec_of(it, rec.cpu().numpy(), liar))
        assert (o["tail"][liar] == 255).all() and (o["flags"][a:b] == FILL).all() and (o["trace"][4 * a:4 * b] == FILL).all()
        others_equal(o, liar)
    order = np.arange(S)
    order[5] = S
    o = c_tick(eng, 0.3, rec, rows, true, order=order)
    assert o["status"] & 2
    a, b = first[5], first[5 + 1]
    assert (o["tail"][5] == FILL).all() and (o["flags"][a:b] == FILL).all()
    others_equal(o, 5)


def test_range_protocol_per_ragged_tick(gemm):
    """fp16 x 2 only; the loud tick of tests/test_gpu_fsmn_stream.py::test_range_protocol_per_tick (a primed stream's layer-0 FIR cache at
    3e5).  The ragged tick counts one fallback and leaves every output and record byte of the same tick on an engine pinned to bf16 x 3."""
    if gemm != "h2":
        pytest.skip("the range protocol belongs to fp16 x 2")
    eng, padded = engine(), audio(0.3)
    if "eng_split" not in _CACHE:
        _CACHE["eng_split"] = fsmn.FsmnEngine(weights.fsmn_synthetic(SEED))
        _CACHE["eng_split"].blobs.arithmetic = "split"
    eng_s = _CACHE["eng_split"]
    it, pos = fsmn.FsmnStreamBatch(eng, S), [0] * S
    tick(it, padded, pos, [0, 0, 1, 1, 1, 1, 1, 1])
    it.caches[5, 0].fill_(3e5)
    other = fsmn.FsmnStreamBatch(eng_s, S)
    other.load_record(it.record)
    pos_s, counts = list(pos), [1, 0, 0, 2, 1, 3, 0, 2]
    fallbacks = eng.blobs.range_fallbacks
    flags, tail, _ = tick(it, padded, pos, counts)
    assert eng.blobs.range_fallbacks == fallbacks + 1 and eng.blobs.mode() == "h2"
    flags_s, tail_s, _ = tick(other, padded, pos_s, counts)
    assert eng_s.blobs.mode() == "split" and eng_s.blobs.range_fallbacks == 0
    assert torch.equal(flags, flags_s) and torch.equal(tail, tail_s) and torch.equal(it.noise_trace, other.noise_trace)
    assert torch.equal(it.record, other.record)
    tick(it, padded, pos, [0, 0, 0, 0, 1, 0, 1, 1])
    assert eng.blobs.range_fallbacks == fallbacks + 1


@pytest.mark.parametrize("wpt", [1, 3])
def test_stream_detect_and_the_driver(gemm, wpt, tmp_path):
    """Clips of four lengths -- one window, on the grid, off the grid, the longest -- as the streams of one batch: the lists `detect(list)`
    and `inference_fsmn` give."""
    eng = engine()
    _, stride = grid(0.3)
    lens = [L - 3000, L + 2 * stride, L + stride + 777, L + 5 * stride - 100]
    clips = [weights.burst_clips(1, n, seed=77 + k, sample_rate=8000)[0] for k, n in enumerate(lens)]
    noise = np.random.default_rng(3).standard_normal((len(clips), stride + 8))
    want = eng.detect(clips, pad_noise=noise)
    assert eng.stream_detect(clips, windows_per_tick=wpt, pad_noise=noise) == want and any(want)
    files = []
    for k, c in enumerate(clips):
        files.append(str(tmp_path / f"c{k}.wav"))
        audio_io.save_wav(files[-1], c, 16000)
    kw = dict(engine=eng, pad_noise=noise, echo=lambda *_: None)
    a = drivers.inference_fsmn(files, save_timestamps_second=str(tmp_path / "a_s"), save_timestamps_indices=str(tmp_path / "a_i"), **kw)
    b = drivers.inference_fsmn_stream(files, save_timestamps_second=str(tmp_path / "b_s"), save_timestamps_indices=str(tmp_path / "b_i"),
                                      windows_per_tick=wpt, **kw)
    assert a == b == want
    for k in range(len(files)):
        for kind in ("s", "i"):
            assert (tmp_path / f"a_{kind}.{k}").read_text() == (tmp_path / f"b_{kind}.{k}").read_text()
