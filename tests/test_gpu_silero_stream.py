"""GPU: the Silero stream path (vadx_silero_stream_run / vadx.silero.VADIteratorBatch) against whole-clip runs, the host VADIterator and
the reference fixture.  Scores fed tick by tick must be bit for bit what clips() gives for the concatenated audio, on every arithmetic,
and so must the final LSTM state."""
import ctypes as C

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, silero, weights

pytestmark = pytest.mark.gpu
SCALE = np.float32(0.000030517578)
TICKS = [1, 3, 16, 7, 2, 5, 11, 4]


@pytest.fixture(autouse=True, params=["f32", "split", "h2"])
def encoder(request):
    """Every test of this file runs on the three kernel sets (exact-f32 MFMAs, bf16 x 3, fp16 x 2)."""
    prev = silero.encoder_mode(request.param)
    yield request.param
    silero.encoder_mode(prev)


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234))


@pytest.fixture(scope="module")
def golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silero_iterator.npz"))


def ticks_of(windows, sizes=TICKS):
    out, i = [], 0
    while sum(out) < windows:
        out.append(min(sizes[i % len(sizes)], windows - sum(out)))
        i += 1
    return out


def pcm(S, windows, seed):
    return weights.burst_clips(S, windows * 512, seed=seed)


def prm(threshold=0.5, sampling_rate=16000, min_silence_duration_ms=100, speech_pad_ms=30):
    p = _lib.SileroIterParams()
    p.threshold, p.sampling_rate, p.min_silence_duration_ms, p.speech_pad_ms = threshold, sampling_rate, min_silence_duration_ms, speech_pad_ms
    return p


class Tick:
    """Buffers of one C-level tick for S streams x k windows."""

    def __init__(self, S, k):
        L = _lib.lib()
        self.S, self.k = S, k
        self.rec = [torch.zeros(L.vadx_silero_stream_state_bytes(S), dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.ws = torch.empty(L.vadx_silero_stream_workspace_bytes(S, k), dtype=torch.uint8, device="cuda")
        self.probs = torch.empty((S, k), dtype=torch.float32, device="cuda")
        self.kind = torch.empty((S, k), dtype=torch.int8, device="cuda")
        self.value = torch.empty((S, k), dtype=torch.float64, device="cuda")

    def run(self, engine, x, rin, rout, reset=None, active=None, cfg=None, p=None, ws_bytes=None, row_stride=None):
        pcm16 = x.dtype == torch.int16
        return _lib.lib().vadx_silero_stream_run(
            engine.packed.data_ptr(), C.byref(p or prm()), x.data_ptr(), int(pcm16), float(SCALE),
            row_stride if row_stride is not None else x.stride(0), self.S, self.k,
            None if reset is None else reset.data_ptr(), None if active is None else active.data_ptr(),
            rin.data_ptr(), rout.data_ptr(), self.probs.data_ptr(), self.kind.data_ptr(), self.value.data_ptr(), self.ws.data_ptr(),
            self.ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_ptr(), cfg if cfg is not None else engine.cfg())


def hc(rec, S):
    return rec[:2 * S * 128 * 4].view(torch.float32).view(2, S, 128)


# ------------------------------------------------------------------ 1. tick by tick == whole clips, bit for bit
@pytest.mark.parametrize("S,windows,sizes", [(1, 40, TICKS), (37, 320, TICKS), (300, 100, TICKS), (16, 10, TICKS), (4096, 32, [1])])
@pytest.mark.parametrize("dtype", ["f32", "int16"])
def test_ticks_are_bitwise_clips(engine, S, windows, sizes, dtype):
    a = pcm(S, windows, seed=S + windows)
    f = a.astype(np.float32) * SCALE
    want, st_want = engine.clips(torch.from_numpy(f).cuda(), return_state=True)
    if dtype == "int16":
        want = engine.clips_pcm16(torch.from_numpy(a).cuda())
    src = a if dtype == "int16" else f
    it = silero.VADIteratorBatch(engine, S)
    got, w0 = [], 0
    for k in ticks_of(windows, sizes):
        x = src[:, w0 * 512:(w0 + k) * 512]
        _, _, p = it.step(torch.from_numpy(x) if k % 2 else x)          # numpy and torch, host memory
        got.append(p)
        w0 += k
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(got, dim=1), want)
    assert torch.equal(it.state, st_want)


# ------------------------------------------------------------------ 2. the record
def test_record_carry(engine):
    S, k = 40, 6
    a = pcm(S, 4 * k, seed=5).astype(np.float32) * SCALE
    x = torch.from_numpy(a).cuda()
    t = Tick(S, k)
    # an all-zero record is S fresh streams; state_in is never written
    rin = torch.zeros_like(t.rec[0])
    rout = torch.full_like(t.rec[1], 7)
    _lib.check(t.run(engine, x[:, :k * 512], rin, rout))
    torch.cuda.synchronize()
    assert not rin.any()
    assert torch.equal(t.probs, engine.clips(x[:, :k * 512]))
    # inactive streams: bitwise copy of the record, kind 0, NaN probs; reset streams restart from their audio at this tick
    r1 = rout.clone()
    rout2 = torch.full_like(rout, 3)
    active = torch.ones(S, dtype=torch.uint8, device="cuda")
    active[[0, 7, 39]] = 0
    reset = torch.zeros(S, dtype=torch.uint8, device="cuda")
    reset[[1, 7, 20]] = 1                                       # 7 is inactive: its reset is ignored
    _lib.check(t.run(engine, x[:, k * 512:2 * k * 512], r1, rout2, reset=reset, active=active))
    torch.cuda.synchronize()
    assert torch.equal(r1, rout)                                # state_in untouched
    p2, rec2 = t.probs.clone(), rout2.clone()
    a_ = torch.tensor([0, 7, 39])
    assert (t.kind[a_] == 0).all() and torch.isnan(t.probs[a_]).all()
    assert torch.equal(hc(rout2, S)[:, a_], hc(r1, S)[:, a_])
    # a tick with every stream inactive hands back the whole record, bit for bit (S = 40: the record has no padding bytes)
    rcopy = torch.full_like(r1, 5)
    _lib.check(t.run(engine, x[:, :k * 512], r1, rcopy, active=torch.zeros_like(active)))
    torch.cuda.synchronize()
    assert r1.numel() == S * 1300 and torch.equal(rcopy, r1)
    # run the remaining ticks; the reset streams must equal clips() of their audio from the reset tick on
    r = [rout2, torch.empty_like(rout2)]
    probs = [p2]
    for j in (2, 3):
        _lib.check(t.run(engine, x[:, j * k * 512:(j + 1) * k * 512], r[0], r[1]))
        probs.append(t.probs.clone())
        r.reverse()
    torch.cuda.synchronize()
    got = torch.cat(probs, dim=1)
    fresh = engine.clips(x[[1, 20], k * 512:])
    assert torch.equal(got[[1, 20]], fresh)
    whole = engine.clips(x)
    keep = [s for s in range(S) if s not in (0, 1, 7, 20, 39)]
    assert torch.equal(got[keep], whole[keep, k:])
    # the inactive streams' records carried their context too: tick 2 rerun with everyone active continues them seamlessly
    t2 = Tick(S, k)
    _lib.check(t2.run(engine, x[:, k * 512:2 * k * 512], rec2, torch.empty_like(rec2)))
    torch.cuda.synchronize()
    assert torch.equal(t2.probs[a_], whole[a_, k:2 * k])


# ------------------------------------------------------------------ 3. the device machine == S host VADIterators on the device's scores
class _Replay:
    def __init__(self):
        self.q = []

    def reset_states(self):
        pass

    def __call__(self, x, sr):
        return torch.tensor([[self.q.pop(0)]])


def test_device_machine_matches_host_iterators(engine, encoder):
    S, W = 1024, 300
    rng = np.random.default_rng(9)
    a = pcm(S, W, seed=17)
    sizes = ticks_of(W, [16, 1, 7, 30, 4, 2, 12])
    actives = [rng.random(S) > 0.15 for _ in sizes]
    resets = [rng.random(S) < 0.03 for _ in sizes]
    params = [dict(), dict(threshold=0.6, min_silence_duration_ms=250), dict(threshold=0.45, speech_pad_ms=30.03, min_silence_duration_ms=0)]
    n_events = 0
    for kw in params:
        dev = silero.VADIteratorBatch(engine, S, **kw)
        reps = [_Replay() for _ in range(S)]
        host = [silero.VADIterator(m, **kw) for m in reps]
        w0 = 0
        for k, act, rs in zip(sizes, actives, resets):
            dev.reset_states(rs)
            kind, value, probs = dev.step(a[:, w0 * 512:(w0 + k) * 512], active=act)
            kind, value, probs = kind.cpu().numpy(), value.cpu().numpy(), probs.cpu().numpy()
            for s in range(S):
                if rs[s]:
                    host[s].reset_states()
                if not act[s]:
                    assert (kind[s] == 0).all() and np.isnan(probs[s]).all()
                    continue
                reps[s].q = [float(v) for v in probs[s]]
                for t in range(k):
                    r = host[s](torch.zeros(512))
                    want = (0, None) if r is None else ((1, r["start"]) if "start" in r else (2, r["end"]))
                    got = (int(kind[s, t]), None if kind[s, t] == 0 else int(value[s, t]))
                    assert got == want, (s, t)
                    n_events += kind[s, t] != 0
            w0 += k
    assert n_events > 1000


def test_call_returns_what_k_reference_calls_return(engine):
    """__call__: per stream the k results of k VADIterator calls (dict or None, samples or rounded seconds); [] when inactive."""
    S, k = 3, 4
    a = pcm(S, 60, seed=2).astype(np.float32) * SCALE
    act = np.array([True, False, True])
    for kw in (dict(), dict(return_seconds=True, time_resolution=3)):
        dev = silero.VADIteratorBatch(engine, S)
        reps = [_Replay() for _ in range(S)]
        host = [silero.VADIterator(m) for m in reps]
        twin = silero.VADIteratorBatch(engine, S)
        for w0 in range(0, 60, k):
            x = a[:, w0 * 512:(w0 + k) * 512]
            probs = twin.step(x, active=act)[2].cpu().numpy()
            res = dev(x, active=act, **kw)
            assert res[1] == []
            for s in (0, 2):
                reps[s].q = [float(v) for v in probs[s]]
                assert res[s] == [host[s](torch.zeros(512), **kw) for _ in range(k)]


# ------------------------------------------------------------------ 4. the reference fixture through the device
def _excused(p, thr=0.5):
    return (np.abs(p - thr) < 2e-4) | (np.abs(p - (thr - 0.15)) < 2e-4)


def _check_against_fixture(golden, probs, kinds, values, state):
    excused = 0
    for c in range(2):
        ref = golden[f"b{c}_probs"]
        np.testing.assert_allclose(probs[c], ref, rtol=0, atol=1e-4)
        ex = _excused(ref)
        if ex.any():                                         # a score on a threshold may fall either side: compare up to it only
            first = int(np.argmax(ex))
            excused += 1
        else:
            first = len(ref)
        assert np.array_equal(kinds[c][:first], golden[f"b{c}_kind"][:first])
        m = golden[f"b{c}_kind"][:first] != 0
        assert np.array_equal(np.asarray(values[c][:first])[m], golden[f"b{c}_samples"][:first][m])
        np.testing.assert_allclose(state[:, c], golden[f"b{c}_state"][:, 0], rtol=0, atol=1e-4)
    assert excused <= 1


def test_reference_fixture_through_the_device(engine, golden):
    audio = golden["b_audio"]
    it = silero.VADIteratorBatch(engine, 2)
    ks, vs, ps, w0 = [], [], [], 0
    for k in ticks_of(150):
        kind, value, probs = it.step(audio[:, w0 * 512:(w0 + k) * 512])
        ks.append(kind.cpu().numpy()), vs.append(value.cpu().numpy()), ps.append(probs.cpu().numpy())
        w0 += k
    assert sum(int((golden[f"b{c}_kind"] != 0).sum()) for c in range(2)) >= 4
    _check_against_fixture(golden, np.concatenate(ps, 1), np.concatenate(ks, 1), np.concatenate(vs, 1), it.state.cpu().numpy())


def test_reference_fixture_through_the_host_iterator(engine, golden):
    audio = golden["b_audio"]
    ps, ks, vs, st = [], [], [], []
    for c in range(2):
        m = silero.OnnxWrapper(engine)
        probs = []

        class Tap:
            def reset_states(self):
                m.reset_states()

            def __call__(self, x, sr):
                o = m(x, sr)
                probs.append(float(o.reshape(-1)[0]))
                return o
        vi = silero.VADIterator(Tap())
        kind, val = np.zeros(150, np.int8), np.full(150, np.nan)
        for i in range(150):
            r = vi(torch.from_numpy(audio[c, i * 512:(i + 1) * 512].copy()))
            if r is not None:
                kind[i], val[i] = (1 if "start" in r else 2), r.get("start", r.get("end"))
        ps.append(probs), ks.append(kind), vs.append(val), st.append(m._state.cpu().numpy()[:, 0])
    _check_against_fixture(golden, np.array(ps, dtype=np.float32), ks, vs, np.stack(st, 1))


# ------------------------------------------------------------------ 5. the fp16 range protocol
def test_range_protocol_recomputes_the_tick(engine, encoder):
    """A tick whose activations leave the fp16 range is recomputed on "split" from the same record: its scores, events and record are
    bit for bit a "split" tick from that record, and range_fallbacks counts it.  In-range ticks stay on "h2"."""
    if encoder != "h2":
        pytest.skip("the range protocol belongs to the fp16 x 2 kernels")
    S, k = 48, 4
    rng = np.random.default_rng(3)
    quiet = [torch.from_numpy(pcm(S, k, seed=40 + j).astype(np.float32) * SCALE).cuda() for j in range(3)]
    loud = torch.from_numpy((rng.standard_normal((S, k * 512)) * 3000).astype(np.float32)).cuda()
    engine.range_flag()
    it = silero.VADIteratorBatch(engine, S)
    n0 = engine.range_fallbacks
    t = Tick(S, k)
    for j, x in enumerate([quiet[0], loud, quiet[1], quiet[2]]):
        before = it.record.clone()
        kind, value, probs = it.step(x)
        assert engine.range_fallbacks == n0 + (j >= 1)
        want = torch.empty_like(before)
        _lib.check(t.run(engine, x, before, want, cfg=engine.cfg("split")))
        torch.cuda.synchronize()
        if j == 1:                                             # the loud tick IS the split tick from the same record
            assert torch.equal(kind, t.kind) and torch.equal(value, t.value) and torch.equal(probs, t.probs)
            assert torch.equal(it.record, want)
        assert not torch.isnan(probs).any()


def test_unchecked_f16x2_tick_reads_invalid(engine, encoder):
    if encoder != "h2":
        pytest.skip("the range protocol belongs to the fp16 x 2 kernels")
    S, k = 64, 4
    rng = np.random.default_rng(4)
    x = [torch.from_numpy(pcm(S, k, seed=60 + j).astype(np.float32) * SCALE).cuda() for j in range(4)]
    x[1][16:32] = torch.from_numpy((rng.standard_normal((16, k * 512)) * 3000).astype(np.float32)).cuda()       # one whole clip group
    t = Tick(S, k)
    cfg = engine.cfg("h2")
    engine.range_flag()
    r = [t.rec[0], t.rec[1]]
    kinds, probs = [], []
    for j in range(4):
        reset = None
        if j == 3:
            reset = torch.zeros(S, dtype=torch.uint8, device="cuda")
            reset[16:24] = 1
        _lib.check(t.run(engine, x[j], r[0], r[1], reset=reset, cfg=cfg))
        kinds.append(t.kind.clone()), probs.append(t.probs.clone())
        r.reverse()
    flag, _ = engine.range_flag()
    assert flag & 1
    kind, p = torch.cat(kinds, 1).cpu().numpy(), torch.cat(probs, 1).cpu().numpy()
    assert np.array_equal(kind == -1, np.isnan(p))                    # -1 exactly where the score is not a number
    bad = np.zeros(S, bool)
    bad[16:32] = True
    assert (kind[bad, k:3 * k] == -1).all()                            # from the loud tick on ...
    assert (kind[16:24, 3 * k:] != -1).all() and (kind[24:32, 3 * k:] == -1).all()    # ... until reset
    assert not (kind[~bad] == -1).any()


def test_blob_that_cannot_run_on_fp16_reads_invalid(encoder):
    if encoder != "h2":
        pytest.skip("the range protocol belongs to the fp16 x 2 kernels")
    w = weights.silero_synthetic(1234)
    w["enc1_w"] = w["enc1_w"].copy()
    w["enc1_w"][3, 5, 1] = 1.0e5
    eng = silero.SileroEngine(w)
    assert not eng.h2_ok
    S, k = 20, 3
    x = torch.from_numpy(pcm(S, k, seed=8).astype(np.float32) * SCALE).cuda()
    t = Tick(S, k)
    rout = torch.full_like(t.rec[1], 0x3f)                          # 0.74...: stale numbers that must not survive
    t.probs.fill_(0.9)
    auto = _lib.SileroCfg()
    _lib.check(t.run(eng, x, t.rec[0], rout, cfg=C.byref(auto)))
    assert eng.range_flag()[0] == 2
    assert (t.kind == -1).all() and torch.isnan(t.probs).all() and torch.isnan(hc(rout, S)).all()


# ------------------------------------------------------------------ 6. bad arguments
def test_bad_arguments(engine):
    S, k = 20, 2
    x = torch.zeros((S, k * 512), dtype=torch.float32, device="cuda")
    t = Tick(S, k)
    a, b = t.rec
    L = _lib.lib()
    run = t.run
    assert run(engine, x, a, b) == 0
    assert run(engine, x, a, b, p=prm(sampling_rate=8000)) == -1 and b"16 kHz" in L.vadx_last_error()
    assert run(engine, x, a, a) == -1 and b"overlap" in L.vadx_last_error()
    assert run(engine, x, a[512:], a[512 + 1024:]) == -1
    assert run(engine, x, a, b, row_stride=k * 512 - 1) == -1
    assert run(engine, x, a, b, ws_bytes=t.ws.numel() - 1) == -2
    bad = _lib.SileroCfg()
    bad.arithmetic = 9
    assert run(engine, x, a, b, cfg=C.byref(bad)) == -1
    args = [engine.packed.data_ptr(), C.byref(prm()), x.data_ptr(), 0, 1.0, k * 512, S, k, None, None, a.data_ptr(), b.data_ptr(),
            t.probs.data_ptr(), t.kind.data_ptr(), t.value.data_ptr(), t.ws.data_ptr(), t.ws.numel(), _lib.stream_ptr(), None]
    for i in (0, 1, 2, 10, 11, 12, 13, 14, 15):
        bad_args = list(args)
        bad_args[i] = None
        assert L.vadx_silero_stream_run(*bad_args) == -1, i
    for i, v in ((6, 0), (7, 0), (6, -3), (7, -1)):
        bad_args = list(args)
        bad_args[i] = v
        assert L.vadx_silero_stream_run(*bad_args) == -1, (i, v)
    assert L.vadx_silero_stream_workspace_bytes(0, 1) == 0 and L.vadx_silero_stream_state_bytes(0) == 0
    torch.cuda.synchronize()
    it = silero.VADIteratorBatch(engine, S)
    for shape in ((S, 500), (S + 1, 512), (S,), (S, 0)):
        with pytest.raises(ValueError):
            it.step(np.zeros(shape, dtype=np.float32))
    with pytest.raises(ValueError):
        it.step(np.zeros((S, 512), dtype=np.int32))
    with pytest.raises(ValueError):
        it.step(np.zeros((S, 512), dtype=np.float32), active=np.ones(S + 1, bool))
    with pytest.raises(ValueError, match="does not support sampling rates"):
        silero.VADIteratorBatch(engine, S, sampling_rate=44100)
    with pytest.raises(ValueError, match="16 kHz"):
        silero.VADIteratorBatch(engine, S, sampling_rate=8000)
