"""GPU: MarbleNet over live streams (vadx.marblenet.MarbleNetStreamBatch, vadx_marblenet_stream_tick).

The contract: a stream is the audio of one virtual clip arriving in pieces, and after its final tick the emitted scores, in order, are
BIT FOR BIT `MarbleNetEngine.run(clip[None])[:, :n // 320]` -- whatever the tick size, the schedule, the neighbours in the batch, on
float32 and on fp16 x 2.  Every test runs on both arithmetics (the `gemm` fixture), on synthetic weights whose decoder is re-centred as
tests/test_gpu_marblenet_shapes.py re-centres it (on the float64 logits of the pooled clips below, from the device's own log-mel), so
that the float64 comparison of item 2 reads probabilities where an error shows.

FINDING: the whole-clip call itself is not one function of the audio at the last bit.  Its front-end computes the
clip's LAST F mod 64 log-mel frames (when that is 1 .. 48; F = n // 160 + 1) in a tail-tile variant in which the compiler contracts
re * re + im * im into an FMA, and every other frame in the full tile, where it does not: the same frame comes out one float32 ulp
apart depending on where the clip happens to end.  A stream cannot know where its clip will end when it computes a frame, so it
computes every frame in the full-tile form.  Hence: score frame j is BITWISE the whole-clip call's wherever it reads none of those
tail-tile frames (2 j + 145 < 64 (F // 64), or no tail tile at all: `bitwise_frames`), and the frames that do read them are held to the
float64 bound of item 2 in the bitwise assertion's place (item 2 runs over ALL frames of all clips).  Two clips whose whole-clip call has
no tail tile (F = 256 and F = 64 * 3 + 50) are added to the issue's lengths: they are bitwise to the last frame.  Everything that does
not involve the whole-clip call -- schedules, neighbours, resets, the range protocol against a float32 stream -- is bitwise throughout.

Seeds: weights 1234, clips numpy default_rng(77), amplitude 8000; the clip of 320 * 74 samples is all zeros, the one of 320 * 140 + 7 is
silence then noise.  Checked on the CPU before the GPU run (float64 net on the ORACLE's log-mel of the same clips, same re-centring):
the pooled reference keeps 96.8 % of its probabilities in (0.02, 0.98); the test asserts >= 90 % on the reference it compares with.

Float64 bound (item 2): e = max |z - z_ref| / sd(z_ref) over the in-range values of the pooled clips, z = log s1 - log s0; the float32
torch oracle's own error e32 on the same log-mel; e <= 2 * R * e32 with R the pinned ratios tests/test_gpu_marblenet_shapes.py
records (profiles/marblenet_shapes_errors.txt): 0.69 fused float32, 0.60 fused fp16 x 2.  Probabilities within 1e-4."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, marblenet, weights
from test_gpu_marblenet_shapes import logit_error, net, score_logit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
HOP = 320
LENGTHS = (0, 1, 319, 320, 321, 320 * 73, 320 * 73 + 319, 320 * 74, 320 * 74 + 1, 320 * 75 + 161, 320 * 140 + 7, 320 * 200 + 77,
           160 * 255, 160 * (64 * 3 + 49) + 3)               # the last two: F = 256 and 242, no tail tile in the whole-clip front-end
ZERO_CLIP, HALF_SILENT = 320 * 74, 320 * 140 + 7
R_ARITH = {"f32": 0.69, "h2": 0.60}
SENTINEL = np.float32(-7.0e37)


@pytest.fixture(autouse=True, params=["f32", "h2"])
def gemm(request):
    prev = _lib.gemm_mode(request.param)
    yield request.param
    _lib.gemm_mode(prev)


def make_clips():
    rng = np.random.default_rng(77)
    clips = []
    for n in LENGTHS:
        c = np.clip(np.rint(rng.standard_normal(n) * 8000), -32768, 32767).astype(np.int16)
        if n == ZERO_CLIP:
            c[:] = 0
        if n == HALF_SILENT:
            c[:n // 2] = 0
        clips.append(c)
    return clips


_S = {}


def setup():
    """Engine (re-centred weights), clips, the device's log-mel per clip and both oracles on it: built once, shared, never changed."""
    if not _S:
        clips = make_clips()
        plain = marblenet.MarbleNetEngine(weights.marblenet_synthetic(SEED))
        feats = {b: plain.frontend(len(c)).logmel(c[None]).cpu().numpy() for b, c in enumerate(clips) if len(c)}
        w0 = weights.marblenet_synthetic(SEED)
        blocks = tuple(weights.MARBLENET_BLOCKS)
        z_all = np.concatenate([net(w0, f, blocks, torch.float64)[0][0, :len(clips[b]) // HOP] for b, f in feats.items()])
        s, mu = 1.5 / z_all.std(), z_all.mean()
        dw, db = w0["dec_w"].astype(np.float64), w0["dec_b"].astype(np.float64)
        dw[1] = dw[0] + s * (dw[1] - dw[0])
        db[1] = db[0] + s * (db[1] - db[0]) - s * mu
        w = dict(w0, dec_w=dw.astype(np.float32), dec_b=db.astype(np.float32))
        ref = {}
        for b, f in feats.items():
            nf = len(clips[b]) // HOP
            z64, s64, _ = net(w, f, blocks, torch.float64)
            _, s32, _ = net(w, f, blocks, torch.float32)
            ref[b] = dict(z=z64[0, :nf], p=s64[0, :nf, 1], s32=s32[0, :nf])
        zr = np.concatenate([r["z"] for r in ref.values()])
        pr = np.concatenate([r["p"] for r in ref.values()])
        z32 = np.concatenate([score_logit(r["s32"][:, 0], r["s32"][:, 1]) for r in ref.values()])
        sd = float(zr.std())
        _S.update(clips=clips, w=w, plain=plain, eng=marblenet.MarbleNetEngine(w), ref=ref, whole={}, streamed={}, sd=sd, zr=zr, pr=pr,
                  e32=logit_error(z32, zr, pr, sd))
    return _S


def whole_clip(gemm, b):
    """engine.run(clip[None])[:, :n // 320] for clip b on this arithmetic (empty for a clip shorter than one score frame), once"""
    S = setup()
    if (gemm, b) not in S["whole"]:
        c = S["clips"][b]
        nf = len(c) // HOP
        if nf == 0:
            S["whole"][(gemm, b)] = (np.zeros(0, np.float32), np.zeros(0, np.float32))
        else:
            before = S["eng"].range_fallbacks
            s0, s1, slen = S["eng"].run(c[None])
            assert slen == nf and S["eng"].range_fallbacks == before
            S["whole"][(gemm, b)] = (s0[0, :nf].cpu().numpy(), s1[0, :nf].cpu().numpy())
    return S["whole"][(gemm, b)]


def bitwise_frames(n):
    """Score frames of an n-sample clip that read no log-mel frame of the whole-clip front-end's tail tile (see FINDING above)"""
    F = n // 160 + 1
    if F % 64 == 0 or F % 64 > 48:
        return n // HOP
    return min(n // HOP, max(0, (64 * (F // 64) - 145 + 1) // 2))


def float64_reference(clip):
    """(z, p, z32) on the device's own log-mel of `clip`, re-centred weights, the n // 320 score frames: the float64 oracle's logit
    and probability, and the float32 torch oracle's logit (for the case's own e32)"""
    S = setup()
    nf = len(clip) // HOP
    f = S["plain"].frontend(len(clip)).logmel(clip[None]).cpu().numpy()
    blocks = tuple(weights.MARBLENET_BLOCKS)
    z64, s64, _ = net(S["w"], f, blocks, torch.float64)
    _, s32, _ = net(S["w"], f, blocks, torch.float32)
    return z64[0, :nf], s64[0, :nf, 1], score_logit(s32[0, :nf, 0], s32[0, :nf, 1])


def held_to_float64(gemm, s0, s1, z_ref, p_ref, e32, what):
    """The float64 bound of item 2 in a bitwise assertion's place (FINDING above): probabilities within 1e-4 and the logit error,
    normalised by the weight set's sd(z), within 2 R e32 -- R the pinned ratio of this arithmetic, e32 the float32 oracle's own error
    AT THE CASE the frames belong to (all frames of that case's clips pooled, as item 2 pools this file's)."""
    S = setup()
    assert float(np.abs(np.asarray(s1, dtype=np.float64) - p_ref).max()) <= 1e-4, what
    if ((p_ref > 0.02) & (p_ref < 0.98)).any():
        e = logit_error(score_logit(s0, s1), z_ref, p_ref, S["sd"])
        print(f"marblenet stream {gemm} {what}: e {e:.2e} e32 {e32:.2e} bound {2.0 * R_ARITH[gemm] * e32:.2e}")
        assert e <= 2.0 * R_ARITH[gemm] * e32, (what, e, e32)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_streams(eng, clips, schedule, sb=None, on_tick=None):
    """Every clip one stream of one batch; tick i feeds schedule[i % len] frames to every stream that still has that much audio, a
    stream's first tick with less is its final one, then it idles.  -> per clip (s0, s1, n_out per tick), the batch object."""
    S = len(clips)
    sb = sb or marblenet.MarbleNetStreamBatch(eng, S)
    at, done = [0] * S, [False] * S
    out = [([], [], []) for _ in range(S)]
    i = 0
    while not all(done):
        k = schedule[i % len(schedule)]
        row = k * HOP
        host, n, fin = np.zeros((S, row), np.int16), np.zeros(S, np.int64), np.zeros(S, bool)
        for s, c in enumerate(clips):
            if done[s]:
                continue
            left = len(c) - at[s]
            take = row if left >= row else left
            fin[s] = left < row
            host[s, :take], n[s] = c[at[s]:at[s] + take], take
            at[s] += take
            done[s] = bool(fin[s])
        s0, s1, n_out = sb.step(host, n, final=fin)
        cnt = n_out.cpu().numpy()
        assert s0.shape == s1.shape == (S, k + 73)
        h0, h1 = s0.cpu().numpy(), s1.cpu().numpy()
        for s in range(S):
            assert np.isnan(h0[s, cnt[s]:]).all() and np.isnan(h1[s, cnt[s]:]).all()
            assert np.isfinite(h0[s, :cnt[s]]).all() and np.isfinite(h1[s, :cnt[s]]).all()
            out[s][0].append(h0[s, :cnt[s]]); out[s][1].append(h1[s, :cnt[s]]); out[s][2].append(int(cnt[s]))
        if on_tick:
            on_tick(i, sb)
        i += 1
    return [(np.concatenate(a), np.concatenate(b), c) for a, b, c in out], sb


def streamed(gemm, k):
    """The clips of LENGTHS as the streams of one batch at k frames per tick, once per arithmetic"""
    S = setup()
    if (gemm, k) not in S["streamed"]:
        before = S["eng"].range_fallbacks
        res, sb = run_streams(S["eng"], S["clips"], [k])
        assert S["eng"].range_fallbacks == before and S["eng"].mode() == gemm
        assert not sb.record.any() and not sb.fed.any() and not sb.emitted.any()        # every stream has had its final tick
        S["streamed"][(gemm, k)] = res
    return S["streamed"][(gemm, k)]


# ---- 1. whole-clip equality
@pytest.mark.parametrize("k", [1, 3, 32, 33])
def test_streamed_scores_are_bitwise_the_whole_clip_call(gemm, k):
    S = setup()
    res = streamed(gemm, k)
    for b, c in enumerate(S["clips"]):
        n = len(c)
        want0, want1 = whole_clip(gemm, b)
        s0, s1, per_tick = res[b]
        assert s0.shape == (n // HOP,), (b, n)
        m = bitwise_frames(n)
        assert same_bytes(s0[:m], want0[:m]) and same_bytes(s1[:m], want1[:m]), (k, b, n)
        if m < n // HOP:        # frames behind m read the whole-clip call's tail-tile log-mel: float64 bound in the bitwise assertion's place
            r = S["ref"][b]
            held_to_float64(gemm, s0[m:], s1[m:], r["z"][m:], r["p"][m:], S["e32"], (k, b, n))
        else:
            assert same_bytes(s0, want0) and same_bytes(s1, want1), (k, b, n)
        for kk in (1, 3, 32, 33):                             # and the streams agree with each other to the last bit, whatever k
            other = streamed(gemm, kk)[b]                     # (computed here if no other case has: no pair depends on test order)
            assert same_bytes(other[0], s0) and same_bytes(other[1], s1), (k, kk, b)
        # counts: nothing before the look-ahead is covered, everything by the final tick
        q = n // (k * HOP)                                  # the stream's own ticks: q whole rows, then its final tick; idle after it
        own, idle = per_tick[:q + 1], per_tick[q + 1:]
        want_counts = np.maximum(np.arange(1, q + 1) * k - 73, 0)
        assert np.array_equal(np.cumsum(own)[:-1], want_counts), (k, b)
        assert sum(own) == n // HOP and not any(idle)
        if n < 320 * 74:
            assert sum(own[:-1]) == 0                                                    # shorter than the look-ahead: all on the final tick


# ---- 2. against float64
def test_streamed_scores_against_float64(gemm):
    S = setup()
    res = streamed(gemm, 3)
    z = np.concatenate([score_logit(res[b][0], res[b][1]) for b in S["ref"]])
    p1 = np.concatenate([res[b][1].astype(np.float64) for b in S["ref"]])
    zr, pr, sd, e32 = S["zr"], S["pr"], S["sd"], S["e32"]
    inside = float(((pr > 0.02) & (pr < 0.98)).mean())
    assert inside >= 0.9, inside
    e, p = logit_error(z, zr, pr, sd), float(np.abs(p1 - pr).max())
    bound = 2.0 * R_ARITH[gemm] * e32
    line = f"marblenet stream {gemm}: frames {len(zr)} inside {inside:.3f} p {p:.2e} e {e:.2e} e32 {e32:.2e} bound {bound:.2e} ratio {e / bound:.3f}"
    print(line)
    if os.environ.get("VADX_WRITE_PROFILES"):
        with open(os.path.join(ROOT, "profiles", "marblenet_stream_errors.txt"), "a") as fh:
            fh.write(line + "\n")
    assert p <= 1e-4, line
    assert e <= bound, line


# ---- 3. schedule independence
def test_schedule_does_not_matter(gemm):
    S = setup()
    eng = S["eng"]
    rng = np.random.default_rng(78)
    clip = np.rint(rng.standard_normal(45000) * 8000).astype(np.int16)
    head, rest = clip[:128 * HOP], clip[128 * HOP:]
    schedules = ([1] * 128, [64, 64], [1, 33, 2, 32, 31, 5, 24])
    outs, records = [], []
    for sched in schedules:
        assert sum(sched) == 128
        sb = marblenet.MarbleNetStreamBatch(eng, 1)
        a0, a1, at = [], [], 0
        for k in sched:
            s0, s1, n_out = sb.step(head[None, at * HOP:(at + k) * HOP])
            m = int(n_out[0])
            a0.append(s0[0, :m].cpu().numpy()); a1.append(s1[0, :m].cpu().numpy())
            at += k
        assert sb.fed.tolist() == [128 * HOP] and sb.emitted.tolist() == [128 - 73]
        records.append(sb.record.cpu().numpy().copy())
        row = np.zeros((1, 64 * HOP), np.int16)
        row[0, :len(rest)] = rest
        s0, s1, n_out = sb.step(row, [len(rest)], final=[True])
        m = int(n_out[0])
        a0.append(s0[0, :m].cpu().numpy()); a1.append(s1[0, :m].cpu().numpy())
        outs.append((np.concatenate(a0), np.concatenate(a1)))
        assert not sb.record.any()
    for o, r in zip(outs[1:], records[1:]):
        assert same_bytes(o[0], outs[0][0]) and same_bytes(o[1], outs[0][1])
        assert same_bytes(r, records[0])
    assert records[0].any() and outs[0][0].shape == (45000 // HOP,)
    s0, s1, _ = eng.run(clip[None])
    m = bitwise_frames(45000)
    assert 0 < m < 45000 // HOP
    assert same_bytes(outs[0][1][:m], s1[0, :m].cpu().numpy()) and same_bytes(outs[0][0][:m], s0[0, :m].cpu().numpy())
    z_ref, p_ref, z32 = float64_reference(clip)              # behind m: the float64 bound in the bitwise assertion's place
    held_to_float64(gemm, outs[0][0][m:], outs[0][1][m:], z_ref[m:], p_ref[m:], logit_error(z32, z_ref, p_ref, S["sd"]), "schedule clip")


# ---- 4. neighbours, masks, record
def test_neighbours_masks_and_record(gemm):
    S = setup()
    eng, k = S["eng"], 16
    rng = np.random.default_rng(79)
    lengths = (320 * 90 + 5, 320 * 30, 320 * 120 + 100, 320 * 80, 320 * 100 + 319)
    clips = [np.rint(rng.standard_normal(n) * 8000).astype(np.int16) for n in lengths]
    fresh = np.rint(rng.standard_normal(320 * 85 + 11) * 8000).astype(np.int16)       # what stream 3 is fed after its reset
    row = k * HOP
    sb = marblenet.MarbleNetStreamBatch(eng, 5)
    got = [([], []) for _ in range(5)]
    at = [0] * 5
    src = [clips[0], clips[1], clips[2], clips[3], clips[4]]
    done = [False] * 5
    tick = 0
    while not all(done):
        host, n, fin, rs = np.zeros((5, row), np.int16), np.zeros(5, np.int64), np.zeros(5, bool), np.zeros(5, bool)
        for s in range(5):
            if done[s] or (s == 1 and tick in (1, 2)):             # stream 1 gets no audio on ticks 1 and 2
                continue
            if s == 3 and tick == 3:                               # stream 3 restarts on another clip, mid-call
                rs[s], src[s], at[s], got[s] = True, fresh, 0, ([], [])
            left = len(src[s]) - at[s]
            take = row if left >= row else left
            fin[s] = left < row
            host[s, :take], n[s] = src[s][at[s]:at[s] + take], take
            at[s] += take
            done[s] = bool(fin[s])
        before = sb.record.clone()
        before_ptr = sb.record.data_ptr()
        s0, s1, n_out = sb.step(host, n, reset=rs, final=fin)
        cnt = n_out.cpu().numpy()
        assert sb.record.data_ptr() != before_ptr and torch.equal(sb._rec[1 - sb._cur], before)      # state_in: byte-identical after the tick
        for s in range(5):
            if n[s] == 0 and not fin[s]:
                assert cnt[s] == 0 and torch.equal(sb.stream_bytes(s), sb.stream_bytes(s, before)), (tick, s)
                assert torch.isnan(s0[s]).all() and torch.isnan(s1[s]).all()
            elif fin[s]:
                assert not sb.stream_bytes(s).any(), (tick, s)                              # final: the record is zero bytes again
            elif n[s]:
                assert not torch.equal(sb.stream_bytes(s), sb.stream_bytes(s, before)), (tick, s)
            got[s][0].append(s0[s, :cnt[s]].cpu().numpy()); got[s][1].append(s1[s, :cnt[s]].cpu().numpy())
        tick += 1
    assert tick > 6
    for s in range(5):
        alone, _ = run_streams(eng, [src[s]], [k])
        g0, g1 = np.concatenate(got[s][0]), np.concatenate(got[s][1])
        assert g0.shape == (len(src[s]) // HOP,)
        assert same_bytes(g0, alone[0][0]) and same_bytes(g1, alone[0][1]), s


# ---- 5. range protocol
@pytest.mark.parametrize("scale", [3e4, 1600.0])
def test_range_protocol_recomputes_a_flagged_tick_from_the_untouched_record(gemm, scale):
    """The prologue's 1x1 weights scaled as tests/test_gpu_marblenet_ragged.py::test_range_protocol_covers_the_whole_ragged_batch scales
    them.  At 3e4 every operand behind the prologue is far past 65504 (that test's docstring: 8 - 43 x), so every tick that runs a tile
    flags; at 1600 only silence does (1.5e5 against 2.8e4 for loud noise), so a stream of silence then 3.4 s of noise flags while the
    silence is inside some launch's reach and stops flagging behind it.  Either way a flagged tick counts once and the stream's scores
    are the float32 engine's stream, bit for bit, across the flagged ticks and the ones after.  On float32 the same weights and audio
    raise no flag, count nothing, and give those bytes too."""
    w = dict(weights.marblenet_synthetic(7))
    w["b0r0_pw"] = np.asarray(w["b0r0_pw"]) * scale
    rng = np.random.default_rng(80)
    clip = np.concatenate([np.zeros(5000, np.int16), np.rint(rng.standard_normal(320 * 170) * 8000).astype(np.int16)])
    eng = marblenet.MarbleNetEngine(w)
    assert eng.mode() == gemm
    flagged = []

    def on_tick(i, sb, state={"last": eng.range_fallbacks}):
        flagged.append(eng.range_fallbacks - state["last"])
        state["last"] = eng.range_fallbacks
        assert int(eng._flag[0].item()) == 0

    before = eng.range_fallbacks
    got, _ = run_streams(eng, [clip], [16], on_tick=on_tick)
    print(f"stream ticks recomputed on float32 at scale {scale:g} ({gemm}):", flagged)
    assert sum(flagged) == eng.range_fallbacks - before
    if gemm == "f32":                   # float32 has float32's range: the same weights raise no flag and nothing is recomputed
        assert not any(flagged) and eng.range_fallbacks == 0
    else:
        assert set(flagged) <= {0, 1} and flagged[0] == 1
        if scale == 3e4:
            assert all(flagged)
        else:
            assert flagged[-1] == 0 and 0 < sum(flagged) < len(flagged)
    ref = marblenet.MarbleNetEngine(w)
    ref.arithmetic = "f32"
    want, _ = run_streams(ref, [clip], [16])
    assert ref.range_fallbacks == 0 and int(ref._flag[0].item()) == 0
    assert same_bytes(got[0][0], want[0][0]) and same_bytes(got[0][1], want[0][1]) and got[0][2] == want[0][2]


# ---- 6. guards: bad n_samples straight to the C entry
@pytest.mark.parametrize("bad", [-320, 8 * 320 + 320, 161])
def test_bad_sample_counts_leave_the_stream_untouched(gemm, bad):
    S = setup()
    eng, k, n_streams = S["eng"], 8, 5
    dev, t = eng.device, torch
    rng = np.random.default_rng(81)
    sb = marblenet.MarbleNetStreamBatch(eng, n_streams)
    warm = np.rint(rng.standard_normal((n_streams, 80 * HOP)) * 8000).astype(np.int16)
    sb.step(warm)                                                         # every stream 80 frames in: the tick below emits
    x = t.from_numpy(np.rint(rng.standard_normal((n_streams, k * HOP)) * 8000).astype(np.int16)).to(dev)
    words, cap = marblenet.STREAM_RECORD_WORDS, k + 73
    mode = eng.mode()

    def tick(n_host):
        """state_out / scores / n_out with one sentinel row on either side; -> host copies of the padded buffers"""
        rec = t.full((n_streams + 2, words), float(SENTINEL), dtype=t.float32, device=dev)
        s0 = t.full((n_streams + 2, cap), float(SENTINEL), dtype=t.float32, device=dev)
        s1 = t.full((n_streams + 2, cap), float(SENTINEL), dtype=t.float32, device=dev)
        n_out = t.full((n_streams + 2,), -77, dtype=t.int32, device=dev)
        n_dev = t.from_numpy(np.asarray(n_host, dtype=np.int32)).to(dev)
        src = sb.record.clone()
        sb.tick_raw(x, n_dev, None, None, k, sb.record, rec[1:-1].view(t.uint8).view(-1), s0[1:-1], s1[1:-1], n_out[1:-1], mode)
        t.cuda.synchronize()
        assert torch.equal(src, sb.record)
        if mode == "h2":
            assert int(eng._flag[0].item()) == 0
        return rec.cpu().numpy(), s0.cpu().numpy(), s1.cpu().numpy(), n_out.cpu().numpy()

    good = tick([k * HOP] * n_streams)
    n = [k * HOP] * n_streams
    n[2] = bad
    got = tick(n)
    sent = SENTINEL.view(np.uint32)
    for g, w_ in zip(got[:3], good[:3]):
        g, w_ = g.view(np.uint32), w_.view(np.uint32)
        assert (g[0] == sent).all() and (g[-1] == sent).all()              # the rows around the buffers
        assert (g[1 + 2] == sent).all()                                    # the refused stream: record and score rows as they were filled
        keep = [1 + s for s in range(n_streams) if s != 2]
        assert np.array_equal(g[keep], w_[keep])                          # everyone else: what the good tick gives
        assert not (w_[1 + 2] == sent).all()
    assert got[3][0] == got[3][-1] == -77 and got[3][3] == -77
    assert np.array_equal(np.delete(got[3], 3), np.delete(good[3], 3)) and (good[3][1:-1] == k).all()


# ---- 7. stream_detect
def test_stream_detect_equals_detect(gemm):
    S = setup()
    eng = S["eng"]
    lengths = (100, 320 + 5, 320 * 74 + 17, 320 * 75, 320 * 300 + 100)       # F = 1, 3, 149, 151, 601: every whole-clip call has a tail tile
    clips = [weights.burst_clips(1, n, seed=90 + i)[0] for i, n in enumerate(lengths)]
    want, wtrack, wdec, wnf = eng.detect(clips, return_probs=True)
    got, track, dec, nf = eng.stream_detect(clips, chunk_frames=16, return_probs=True)
    assert nf.tolist() == wnf.tolist() == [0, 1, 74, 75, 300]
    assert got == want == eng.stream_detect(clips, chunk_frames=16)
    assert torch.equal(dec, wdec) and track.shape == wtrack.shape
    both, _ = run_streams(eng, clips, [16])                  # a track holds score_active only: the same streams with both scores
    refs = [float64_reference(c) for c in clips]
    e32 = logit_error(*(np.concatenate([r[i] for r in refs]) for i in (2, 0, 1)), S["sd"])      # the case = these five clips, pooled
    for b, n in enumerate(lengths):                          # bit for bit where `detect` read no tail-tile log-mel frame (FINDING above)
        m = bitwise_frames(n)
        assert torch.equal(track[b, :m], wtrack[b, :m]) and not track[b, nf[b]:].any(), b
        assert same_bytes(track[b, :nf[b]].cpu().numpy(), both[b][1]), b
        if m < nf[b]:                                        # behind m: the float64 bound in the bitwise assertion's place
            z_ref, p_ref, _ = refs[b]
            held_to_float64(gemm, both[b][0][m:], both[b][1][m:], z_ref[m:], p_ref[m:], e32, ("stream_detect", b))
    assert bitwise_frames(lengths[4]) == 216 and any(want)
    full = [weights.burst_clips(1, n, seed=95 + i)[0] for i, n in enumerate((160 * 255, 160 * 511 + 9))]      # F = 256, 512: no tail tile
    want, wtrack, wdec, wnf = eng.detect(full, return_probs=True)
    got, track, dec, nf = eng.stream_detect(full, chunk_frames=16, return_probs=True)
    assert got == want and torch.equal(track, wtrack) and torch.equal(dec, wdec) and nf.tolist() == wnf.tolist() == [127, 255]


def test_refusals_on_the_device_path(gemm):
    S = setup()
    eng = S["eng"]
    sb = marblenet.MarbleNetStreamBatch(eng, 2)
    x = np.zeros((2, 4 * HOP), np.int16)
    for kw, match in ((dict(n_samples=[161, 320]), "not a multiple of 320"), (dict(n_samples=[5 * 320, 320]), r"outside \[0, k \* 320"),
                      (dict(n_samples=[-320, 320]), r"outside \[0, k \* 320")):
        with pytest.raises(ValueError, match=match):
            sb.step(x, **kw)
    with pytest.raises(ValueError, match=r"\[2, k \* 320\]"):
        sb.step(np.zeros((2, 100), np.int16))
    with pytest.raises(ValueError, match=r"outside \[1, 256\]"):
        sb.step(np.zeros((2, 257 * HOP), np.int16))
    assert not sb.record.any()
    lib = _lib.lib()
    assert lib.vadx_marblenet_stream_cap(16) == 89 and lib.vadx_marblenet_stream_max_frames() == marblenet.STREAM_MAX_FRAMES
    assert lib.vadx_marblenet_stream_state_bytes(3) == 3 * 4 * marblenet.STREAM_RECORD_WORDS
    assert C.sizeof(_lib.MarbleNetStreamWeights) == 34 * C.sizeof(C.c_void_p)
