"""GPU: FireRed Stream-VAD for S live streams (vadx.firered.FireRedStreamBatch over vadx_firered_stream_tick) on the three arithmetics.

What is held, and against what:
  - grouping: every stream's probabilities, segments, counts, open_start and record bytes are bitwise those of the same stream run alone,
    whatever the group, S and the neighbours; on float32 the probabilities and caches are bitwise `FireRedEngine.stream_run`;
  - any split of the same chunks into ticks gives the same bytes, and the events + the open segment are exactly what
    oracle.firered.StreamVadPostprocessor makes of the probabilities the ticks returned;
  - five carried ticks against oracle.firered.detect_model_stream in float64 on the device's own log-mel: probabilities within 1e-4, caches
    within 1e-3 (the file-wide bounds of tests/test_gpu_firered*.py), the normalised logit error e and the largest per-layer relative cache
    error c no more than FACTOR = 2 x the larger of what `stream_run` (the float32 MFMA stream kernel) and the float32 torch oracle show on
    the same case -- both measured here, neither the code under test; 2 is the project's factor for the noise of a max over few values;
  - masks (staggered starts, an inactive stream, a reset), state_in read only, the fp16 x 2 range protocol per tick, one net launch per
    tick, `stream_detect` over a list of clips, and the reference's own streaming run (tests/golden/firered_stream.npz).

A random net's sigmoid saturates, so the weights' output head is re-centred (per channel, logits of mean 0 and standard deviation 1.5) on
the float64 logits of the unmodified weights, as tests/test_gpu_firered_shapes.py does -- here once per config, on the CPU oracle's log-mel of
a fixed clip set, so the weights of a config are the same in every test and can be examined without a device.  The helpers below are copies
of that file's.  Set VADX_STREAM_ERRORS=<path> to have the float64 test write its worst figures per arithmetic there
(profiles/firered_stream_errors.txt keeps one run's)."""
import os

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, firered, weights
from oracle import firered as ofr

pytestmark = pytest.mark.gpu
ATOL, CACHE_ATOL, FACTOR = 1e-4, 1e-3, 2.0
INSIDE, LO, HI = 0.9, 0.02, 0.98
CHUNK = firered.STREAM_CHUNK_SAMPLES


@pytest.fixture(autouse=True, params=["f32", "split", "h2"])
def gemm(request):
    """Every test of this file runs on the three arithmetics of the point-wise layers: exact-f32 MFMAs, bf16 x 3 and fp16 x 2 split products."""
    prev = _lib.gemm_mode(request.param)
    yield request.param
    _lib.gemm_mode(prev)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def K(**kw):
    return tuple(kw.items())


# the stream configs and seeds of tests/test_gpu_firered_shapes.py (STREAM_CFGS / STREAM_SEEDS)
DEFAULT, SMALL, TWO_TAPS, LONG_PAD, PADDED = (K(N2=0, S2=0), K(H=64, P=32, R=3, M=2, N1=8, S1=2, N2=0, S2=0), K(N1=2, N2=0, S2=0),
                                              K(N1=32, S1=3, R=2, N2=0, S2=0), K(H=250, P=120, N2=0, S2=0))
SEEDS = {DEFAULT: 1234, SMALL: 2, TWO_TAPS: 31, LONG_PAD: 9, PADDED: 7}
RAGGED = [14, 1, 33, 19, 2]              # frames per chunk of the carried case


def make_cfg(key):
    return dict(weights.FIRERED_CFG, **dict(key))


def cfg_name(key):
    return ",".join(f"{k}={v}" for k, v in key)


def split_eligible(cfg):
    return (cfg["H"] + 15) // 16 * 16 == 256 and (cfg["P"] + 15) // 16 * 16 == 128


def samples(frames):
    return 400 + 160 * (frames - 1)


def logit(p):
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(p) - np.log1p(-p)


def model(w, feats, caches, dtype):
    """The stream oracle in `dtype` on log-mel chunks [B, 80, T_i], carrying `caches` [R, B, P, pad]: (probs [B, odim, sum T_i], caches after every chunk)"""
    wt = {k: (T(v).to(dtype) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    with torch.no_grad():
        c, probs, after = T(caches).to(dtype), [], []
        for f in feats:
            p, c = ofr.detect_model_stream(wt, T(f).to(dtype), c)
            probs.append(p.numpy())
            after.append(c.numpy())
    return np.concatenate(probs, axis=2), after


def logit_error(p, ref):
    """max |z - z_ref| / sd(z_ref) over the values where the reference lies in (LO, HI)"""
    m = (ref > LO) & (ref < HI)
    zr = logit(ref)[m]
    return float(np.abs(logit(p)[m] - zr).max() / zr.std())


def cache_errors(got, ref):
    """per chunk and layer max |c - c_ref| -> (largest absolute error, per layer the largest error / max |c_ref| over the chunks)"""
    err = np.array([[np.abs(g[r].astype(np.float64) - c[r]).max() for r in range(c.shape[0])] for g, c in zip(got, ref)])
    top = np.array([[np.abs(c[r]).max() for r in range(c.shape[0])] for c in ref])
    return float(err.max()), (err / top).max(axis=0)


def ragged_clips(B, seed):
    """B burst clips cut into chunks of RAGGED frames, the first half of clip 0 digital silence: (clips [B, n], chunk lengths)"""
    lens = [samples(f) for f in RAGGED]
    clips = weights.burst_clips(B, sum(lens), seed=sum(lens) + seed)
    clips[0, :sum(lens) // 2] = 0
    return clips, lens


_CACHE = {}


def weights_for(key):
    """The synthetic weights of config `key` with the output head re-centred on the float64 logits z of the weights themselves over the
    carried case (CPU oracle, its own log-mel, zero caches): out_w *= 1.5 / sd(z), out_b = (out_b - mean(z)) * 1.5 / sd(z), as float32."""
    if ("w", key) not in _CACHE:
        cfg, seed = make_cfg(key), SEEDS[key]
        w = weights.firered_synthetic(seed, cfg)
        clips, lens = ragged_clips(4, seed)
        fe = ofr.Frontend()
        feats = [ofr.log_mel(fe, T(clips[:, sum(lens[:i]):sum(lens[:i + 1])]).reshape(4, 1, -1)).numpy() for i in range(len(lens))]
        c0 = np.zeros((cfg["R"], 4, cfg["P"], (cfg["N1"] - 1) * cfg["S1"]), np.float32)
        probe = dict(w, out_w=w["out_w"] * np.float32(2.0 ** -10), out_b=w["out_b"] * np.float32(2.0 ** -10))
        z = logit(model(probe, feats, c0, torch.float64)[0]) * 2.0 ** 10
        mu, s = z.mean(axis=(0, 2)), 1.5 / z.std(axis=(0, 2))
        _CACHE["w", key] = dict(w, out_w=(w["out_w"].astype(np.float64) * s[:, None]).astype(np.float32),
                                out_b=((w["out_b"].astype(np.float64) - mu) * s).astype(np.float32))
    return _CACHE["w", key]


def engine(key, pinned=None):
    """One engine per config for the file (its blobs are per arithmetic, the arithmetic is the module default the `gemm` fixture sets);
    pinned = an engine of its own held to that arithmetic."""
    if ("eng", key, pinned) not in _CACHE:
        eng = firered.FireRedEngine(weights_for(key), CHUNK)
        eng.blobs.arithmetic = pinned
        _CACHE["eng", key, pinned] = eng
    return _CACHE["eng", key, pinned]


def random_record(it, seed, first=0):
    """A record of it.streams streams in their reset state except for caches 0.3 N(0, 1), stream s drawn from (seed, first + s) alone"""
    rec = torch.zeros_like(it.record)
    R, _, P, pad = it.engine.cache_shape
    c = np.stack([np.random.default_rng((seed, first + s)).standard_normal((R, P, pad)) * 0.3 for s in range(it.streams)]).astype(np.float32)
    rec[:c.size * 4] = T(c).view(torch.uint8).reshape(-1).cuda()
    return rec, c


def stream_audio(S, n, seed, rate=2500):
    """int16 [S, n]: loud / quiet bursts of 0.5 .. 2 s at `rate` samples per second, i.e. a few frames each at 16 kHz, row s drawn from
    (seed, s) alone"""
    return np.concatenate([weights.burst_clips(1, n, seed=seed * 1000 + s, sample_rate=rate) for s in range(S)])


POST = (3, 0.3, 2, 3, 12, 3)             # short windows and a forced split after 12 frames: events inside ticks of a few frames
POST_G = (3, 0.2, 2, 3, 12, 3)           # on random caches the net sits lower (median 0.22 .. 0.32 on the CPU oracle): a threshold below it


def one_tick(eng, S, audio, seed, group, post=POST_G):
    it = firered.FireRedStreamBatch(eng, S, post)
    rec, c0 = random_record(it, seed)
    it.load_record(rec)
    probs, events = it.step(audio[:S], group=group)
    return it, c0, probs, events


# ------------------------------------------------------------------ grouping and independence
GROUP_FRAMES = [1, 14, 15, 16, 17, 37, 56, 57, 112]


def grouping_case(gemm, key, frames):
    cfg = make_cfg(key)
    eng = engine(key)
    G = 112 // frames
    assert _lib.lib().vadx_firered_stream_group_max(frames) == G
    Smax, n = 2 * G + 1, samples(frames)
    audio = stream_audio(Smax, n, 77 + frames)
    fallbacks = eng.blobs.range_fallbacks
    alone = []
    for s in range(Smax):
        it = firered.FireRedStreamBatch(eng, 1, POST_G)
        it.load_record(random_record(it, 5, first=s)[0])
        probs, events = it.step(audio[s:s + 1])
        alone.append((probs[0].clone(), events[0], int(it.open_start[0]), it.caches[0].clone(), it.headers()[0].clone()))
    a_probs, a_caches, a_hdr = (torch.stack([a[i] for a in alone]) for i in (0, 3, 4))
    a_open = np.array([a[2] for a in alone])
    assert bool(torch.isfinite(a_probs).all()) and np.array_equal(it.frames_done, [frames])
    for S in (G + 1, 2 * G + 1):
        for group in (1, G, 0):
            it, c0, probs, events = one_tick(eng, S, audio, 5, group)
            assert probs.shape == (S, cfg["odim"], frames)
            assert torch.equal(probs, a_probs[:S]), (S, group)
            assert events == [a[1] for a in alone[:S]], (S, group)
            assert np.array_equal(it.open_start.cpu().numpy(), a_open[:S]), (S, group)
            assert torch.equal(it.caches, a_caches[:S]) and torch.equal(it.headers(), a_hdr[:S]), (S, group)
            assert np.array_equal(it.frames_done, np.full(S, frames))
    assert eng.blobs.range_fallbacks == fallbacks                                  # the equality is not a fallback's
    assert eng.cfg.arithmetic == _lib.GEMM_MODES[gemm if split_eligible(cfg) else "f32"]
    if eng.cfg.arithmetic == _lib.GEMM_MODES["f32"]:
        # float32: the parent's stream kernel on the same chunk and caches, bit for bit
        S = 2 * G + 1
        p, cout = eng.stream_run(T(audio).cuda(), T(c0).cuda().permute(1, 0, 2, 3).contiguous())
        assert torch.equal(probs, p) and torch.equal(it.caches, cout.permute(1, 0, 2, 3))
    return alone


@pytest.mark.parametrize("frames", GROUP_FRAMES)
def test_grouping_is_invisible(gemm, frames):
    """Default config, one tick of `frames` frames on random caches: S = G + 1 and 2 G + 1 streams (G = 112 // frames) at group = 1, G and 0
    against every stream alone; on float32 against `stream_run`."""
    alone = grouping_case(gemm, DEFAULT, frames)
    if frames >= 14:                       # (CPU oracle, same audio and caches: at least 10 segments ended and 3 open over the 2 G + 1 streams)
        assert any(a[1] for a in alone) and any(a[2] >= 0 for a in alone)          # the outputs that are compared say something


@pytest.mark.parametrize("frames", [14, 37])
@pytest.mark.parametrize("key", [SMALL, LONG_PAD, PADDED], ids=cfg_name)
def test_grouping_is_invisible_at_other_widths(gemm, key, frames):
    """The non-resident float32 pair with two dnn layers (whatever arithmetic is asked for), a cache of 93 frames (longer than the
    tick), and widths only the zero padding of the split fragments supplies."""
    grouping_case(gemm, key, frames)


# ------------------------------------------------------------------ any split into ticks
def run_schedule(eng, audio, sched, post=POST, group=0):
    """sched = [(chunks, samples per chunk)]: -> (probs [S, odim, sum F], events per stream, open segments, record)"""
    S = audio.shape[0]
    it = firered.FireRedStreamBatch(eng, S, post)
    pos, probs, events = 0, [], [[] for _ in range(S)]
    for k, n in sched:
        p, ev = it.step(audio[:, pos:pos + k * n], k, group=group)
        pos += k * n
        probs.append(p)
        for s in range(S):
            events[s] += ev[s]
    assert pos == audio.shape[1]
    return torch.cat(probs, dim=2), events, it.open_segments(), it.record.clone(), it


def oracle_decisions(track, post):
    """oracle.firered.StreamVadPostprocessor over one track: (its process_batch result, segments closed, forced splits)"""
    pp = ofr.StreamVadPostprocessor(*post)
    out = pp.process_batch(track)
    closed = len(out) - (1 if pp.last_start > 0 else 0)
    one, forced = ofr.StreamVadPostprocessor(*post), 0
    for v in track:
        one.process_batch(np.array([v], np.float32))
        forced += int(one.hit_max)
    return out, closed, forced


def test_any_split_into_ticks(gemm):
    """Default config, S = 9, 8 chunks of 14 frames as 8 x 1, 1 x 8 and (3, 1, 4) chunks per tick: the same probabilities and the same
    final record, bit for bit; events + open segment == the oracle's decisions over the probabilities returned, every stream closing at
    least two segments and one by a forced split (on the CPU oracle, same weights and audio: at least 6 and 4)."""
    eng = engine(DEFAULT)
    S = 9
    audio = stream_audio(S, 8 * CHUNK, 6)
    runs = [run_schedule(eng, audio, [(k, CHUNK) for k in ks]) for ks in ([1] * 8, [8], [3, 1, 4])]
    probs, events, opened, rec, it = runs[0]
    assert probs.shape == (S, 1, 112) and np.array_equal(it.frames_done, np.full(S, 112))
    for p2, ev2, op2, rec2, _ in runs[1:]:
        assert torch.equal(p2, probs) and torch.equal(rec2, rec) and ev2 == events and op2 == opened
    tracks = probs[:, 0].cpu().numpy()
    for s in range(S):
        want, closed, forced = oracle_decisions(tracks[s], POST)
        assert events[s] + ([opened[s]] if opened[s] is not None else []) == want, s
        assert len(events[s]) == closed and closed >= 2 and forced >= 1, (s, closed, forced)
    # group = 1 and the library's choice: the same bytes
    p1, ev1, op1, rec1, _ = run_schedule(eng, audio, [(1, CHUNK)] * 8, group=1)
    assert torch.equal(p1, probs) and torch.equal(rec1, rec) and ev1 == events


def test_ragged_single_chunk_ticks(gemm):
    """Chunks of 14 + 1 + 33 + 19 + 2 frames in single-chunk ticks, S = 9: events + open segment == the oracle's decisions, at the
    library's grouping and at one stream per workgroup, the same bytes."""
    eng = engine(DEFAULT)
    S = 9
    lens = [samples(f) for f in RAGGED]
    audio = stream_audio(S, sum(lens), 8)
    probs, events, opened, rec, it = run_schedule(eng, audio, [(1, n) for n in lens])
    assert probs.shape == (S, 1, sum(RAGGED)) and np.array_equal(it.frames_done, np.full(S, sum(RAGGED)))
    tracks = probs[:, 0].cpu().numpy()
    for s in range(S):
        want, _, _ = oracle_decisions(tracks[s], POST)
        assert events[s] + ([opened[s]] if opened[s] is not None else []) == want, s
    assert any(events)
    p1, ev1, op1, rec1, _ = run_schedule(eng, audio, [(1, n) for n in lens], group=1)
    assert torch.equal(p1, probs) and torch.equal(rec1, rec) and ev1 == events and op1 == opened


# ------------------------------------------------------------------ float64
_WORST = {}


def write_errors():
    path = os.environ.get("VADX_STREAM_ERRORS")
    if not path:
        return
    with open(path, "w") as fh:
        fh.write("FireRed stream tick (tests/test_gpu_firered_stream.py::test_carried_ticks_against_float64), one MI355X: five carried ticks of "
                 "14 + 1 + 33 + 19 + 2 frames, B = 4 streams,\nagainst the float64 oracle on the device's own log-mel.  p = max |p - p_ref| "
                 "(bound 1e-4), cache = max |c - c_ref| (bound 1e-3), e = logit error / sd(z_ref),\nc = largest per-layer cache error / max "
                 "|c_ref|; bounds of e and c = 2 x max(stream_run's figure, the float32 torch oracle's figure).\n\n")
        for (arith, name), r in sorted(_WORST.items()):
            fh.write(f"{arith:5s} {name:32s} p {r['p']:.2e} cache {r['c_abs']:.2e} e {r['e']:.2e} (stream_run {r['e_parent']:.2e}, float32 oracle "
                     f"{r['e32']:.2e}) c {r['c']:.2e} (stream_run {r['c_parent']:.2e}, float32 oracle {r['c32']:.2e})\n")


@pytest.mark.parametrize("key", [DEFAULT, LONG_PAD], ids=cfg_name)
def test_carried_ticks_against_float64(gemm, key):
    """Five ticks of 14, 1, 33, 19 and 2 frames from the reset state, the device carrying its record and the float64 net its caches."""
    cfg, B = make_cfg(key), 4
    eng = engine(key)
    clips, lens = ragged_clips(B, SEEDS[key])
    chunks = [T(clips[:, sum(lens[:i]):sum(lens[:i + 1])]).cuda() for i in range(len(lens))]
    if ("ref", key) not in _CACHE:
        feats = [np.ascontiguousarray(eng._frontend_for(n).logmel(a, 1, n).cpu().numpy().transpose(0, 2, 1)) for a, n in zip(chunks, lens)]
        c0 = np.zeros((cfg["R"], B, cfg["P"], (cfg["N1"] - 1) * cfg["S1"]), np.float32)
        w = weights_for(key)
        p64, c64 = model(w, feats, c0, torch.float64)
        p32, c32 = model(w, feats, c0, torch.float32)
        # the parent's route: stream_run (float32 MFMAs whatever the arithmetic) carrying its own caches
        caches, pp, cp = eng.new_caches(B), [], []
        for a in chunks:
            p, caches = eng.stream_run(a, caches)
            pp.append(p.cpu().numpy().astype(np.float64))
            cp.append(caches.cpu().numpy())
        pp = np.concatenate(pp, axis=2)
        _CACHE["ref", key] = dict(p=p64, c=c64, e32=logit_error(p32, p64), c32=float(cache_errors(c32, c64)[1].max()),
                                  e_parent=logit_error(pp, p64), c_parent=float(cache_errors(cp, c64)[1].max()),
                                  inside=float(((p64 > LO) & (p64 < HI)).mean()))
    ref = _CACHE["ref", key]
    assert ref["inside"] >= INSIDE, ref["inside"]          # a saturated sigmoid tests nothing
    it = firered.FireRedStreamBatch(eng, B)
    probs, after = [], []
    for a in chunks:
        p, _ = it.step(a)
        probs.append(p.cpu().numpy().astype(np.float64))
        after.append(it.caches.permute(1, 0, 2, 3).cpu().numpy())
    got = np.concatenate(probs, axis=2)
    assert got.shape == ref["p"].shape == (B, cfg["odim"], sum(RAGGED)) and np.isfinite(got).all()
    c_abs, c_rel = cache_errors(after, ref["c"])
    r = dict(p=float(np.abs(got - ref["p"]).max()), e=logit_error(got, ref["p"]), c_abs=c_abs, c=float(c_rel.max()),
             **{k: ref[k] for k in ("e32", "c32", "e_parent", "c_parent")})
    print(f"firered stream tick {gemm} {cfg_name(key)}: p {r['p']:.2e} cache {r['c_abs']:.2e} e {r['e']:.2e} (stream_run {r['e_parent']:.2e}, "
          f"float32 oracle {r['e32']:.2e}) c {r['c']:.2e} (stream_run {r['c_parent']:.2e}, float32 oracle {r['c32']:.2e}) per layer "
          + " ".join(f"{v:.1e}" for v in c_rel) + f" inside {ref['inside']:.3f}")
    _WORST[gemm, cfg_name(key)] = r
    write_errors()
    assert r["p"] <= ATOL and r["c_abs"] <= CACHE_ATOL, r
    assert r["e"] <= FACTOR * max(r["e_parent"], r["e32"]), r
    assert r["c"] <= FACTOR * max(r["c_parent"], r["c32"]), r
    assert eng.blobs.range_fallbacks == 0


# ------------------------------------------------------------------ masks
def test_staggered_inactive_and_reset_streams(gemm):
    eng = engine(DEFAULT)
    S = 3
    audio = stream_audio(S, 4 * CHUNK, 6)
    # what each stream gives alone, chunk by chunk, from the reset state
    want = []
    for s in range(S):
        it1 = firered.FireRedStreamBatch(eng, 1, POST)
        want.append([(lambda r: (r[0][0].clone(), r[1][0]))(it1.step(audio[s:s + 1, j * CHUNK:(j + 1) * CHUNK])) for j in range(4)])
    chunk = lambda rows: np.stack([audio[s, j * CHUNK:(j + 1) * CHUNK] if j is not None else np.zeros(CHUNK, np.int16)      # noqa: E731
                                   for s, j in enumerate(rows)])
    it = firered.FireRedStreamBatch(eng, S, POST)
    assert not bool(it.record.any())
    # tick 1: streams 0 and 1 start; stream 2 has no audio yet (and its reset request is ignored)
    probs, ev = it.step(chunk([0, 0, None]), active=[True, True, False], reset=[False, False, True])
    assert torch.equal(probs[0], want[0][0][0]) and torch.equal(probs[1], want[1][0][0]) and ev[0] == want[0][0][1]
    assert bool(torch.isnan(probs[2]).all()) and ev[2] == [] and int(it.open_start[2]) == -1
    assert not bool(it.stream_bytes(it.record, 2).any())                          # still the all-zero record
    assert np.array_equal(it.frames_done, [14, 14, 0])
    # tick 2: stream 2 starts (from the all-zero record: the reset state), stream 1 pauses
    before = it.record.clone()
    probs, ev = it.step(chunk([1, None, 0]), active=[True, False, True], reset=[False, True, False])
    assert torch.equal(probs[0], want[0][1][0]) and torch.equal(probs[2], want[2][0][0]) and ev[2] == want[2][0][1]
    assert bool(torch.isnan(probs[1]).all()) and ev[1] == [] and int(it.open_start[1]) == -1
    assert torch.equal(it.stream_bytes(it.record, 1), it.stream_bytes(before, 1))          # bit for bit, the reset request ignored
    assert not torch.equal(it.stream_bytes(it.record, 0), it.stream_bytes(before, 0))
    # tick 3: stream 1 goes on where it was; stream 0 is reset and hears its audio from the start again
    probs, ev = it.step(chunk([0, 1, 1]), reset=[True, False, False])
    assert torch.equal(probs[0], want[0][0][0]) and ev[0] == want[0][0][1]
    assert torch.equal(probs[1], want[1][1][0]) and ev[1] == want[1][1][1]
    assert torch.equal(probs[2], want[2][1][0]) and ev[2] == want[2][1][1]
    assert np.array_equal(it.frames_done, [14, 28, 28])
    # after its reset stream 0 is a fresh stream: its bytes are those of a stream that ran this one chunk from the zero record
    fresh = firered.FireRedStreamBatch(eng, 1, POST)
    fresh.step(audio[0:1, :CHUNK])
    assert torch.equal(it.stream_bytes(it.record, 0), fresh.stream_bytes(fresh.record, 0))
    # reset_states: pending until the stream is active
    it.reset_states([2])
    probs, ev = it.step(chunk([1, 2, None]), active=[True, True, False])
    assert np.array_equal(it.frames_done, [28, 42, 28]) and torch.equal(probs[0], want[0][1][0]) and torch.equal(probs[1], want[1][2][0])
    probs, ev = it.step(chunk([2, 3, 0]))
    assert np.array_equal(it.frames_done, [42, 56, 14]) and torch.equal(probs[2], want[2][0][0]) and torch.equal(probs[1], want[1][3][0])
    assert eng.blobs.mode() == gemm


def test_state_in_is_read_only_and_a_tick_can_be_recomputed(gemm):
    eng = engine(DEFAULT)
    S = 9
    audio = stream_audio(S, 3 * CHUNK, 6)
    it = firered.FireRedStreamBatch(eng, S, POST)
    it.step(audio[:, :2 * CHUNK], 2)
    src = it.record                                              # the tensor the next tick reads
    before = src.clone()
    probs, ev = it.step(audio[:, 2 * CHUNK:])
    assert it.record is not src and torch.equal(src, before)     # byte for byte untouched
    again = firered.FireRedStreamBatch(eng, S, POST)
    again.load_record(before)
    probs2, ev2 = again.step(audio[:, 2 * CHUNK:])
    assert torch.equal(probs, probs2) and ev == ev2 and torch.equal(it.open_start, again.open_start)
    assert torch.equal(it.record, again.record)


def test_range_protocol_per_tick(gemm):
    """fp16 x 2 only.  Recipe (tests/test_gpu_fsmn_stream.py::test_range_protocol_per_tick): one stream's whole layer-0 FIR cache is set to
    3e5; the FIR + skip of layer 0 then puts 3e5 * (sum of a channel's taps) on the activation the next point-wise pair splits, beyond
    65504 for most channels.  The tick must count one fallback and leave, for ALL streams, the results and the record of the same tick on
    an engine pinned to bf16 x 3."""
    if gemm != "h2":
        pytest.skip("the range protocol belongs to fp16 x 2")
    eng, eng_s = engine(DEFAULT), engine(DEFAULT, "split")
    S = 9
    audio = stream_audio(S, 3 * CHUNK, 6)
    it = firered.FireRedStreamBatch(eng, S, POST)
    it.step(audio[:, :CHUNK])
    it.caches[1, 0].fill_(3e5)
    other = firered.FireRedStreamBatch(eng_s, S, POST)
    other.load_record(it.record)
    fallbacks = eng.blobs.range_fallbacks
    probs, ev = it.step(audio[:, CHUNK:2 * CHUNK])
    assert eng.blobs.range_fallbacks == fallbacks + 1 and eng.blobs.mode() == "h2"
    probs_s, ev_s = other.step(audio[:, CHUNK:2 * CHUNK])
    assert eng_s.blobs.mode() == "split" and eng_s.blobs.range_fallbacks == 0
    assert torch.equal(probs, probs_s) and ev == ev_s and torch.equal(it.open_start, other.open_start) and torch.equal(it.record, other.record)
    assert bool(torch.isfinite(probs).all())
    # the next tick is an ordinary one again (the cache of 19 frames has been pushed out by 14 new ones only in part: reset the stream)
    it.step(audio[:, 2 * CHUNK:], reset=[s == 1 for s in range(S)])
    assert eng.blobs.range_fallbacks == fallbacks + 1


def test_one_net_launch_per_tick(gemm):
    eng = engine(DEFAULT)
    S = 9
    audio = T(stream_audio(S, 4 * CHUNK, 6)).cuda()
    it = firered.FireRedStreamBatch(eng, S, POST)
    it.step(audio[:, :CHUNK].contiguous())
    for k in (1, 3):
        with _lib.trace() as tr:
            it.step(audio[:, CHUNK:(k + 1) * CHUNK].contiguous(), k)
        assert tr.calls == {"vadx_frontend_logmel": 1, "vadx_firered_stream_tick": 1}, tr.calls


def test_bad_arguments(gemm):
    if gemm != "h2":
        pytest.skip("independent of the arithmetic")
    eng = engine(DEFAULT)
    S = 3
    it = firered.FireRedStreamBatch(eng, S)
    x = np.zeros((S, CHUNK), np.int16)
    with _lib.trace() as tr:
        with pytest.raises(ValueError, match="int16"):
            it.step(x.astype(np.float32))
        with pytest.raises(ValueError, match="at least 400"):
            it.step(x[:, :399])
        with pytest.raises(ValueError, match="at most 112 frames"):
            it.step(np.zeros((S, 9 * CHUNK), np.int16), 9)
        with pytest.raises(ValueError, match="at most 112 frames"):
            it.step(np.zeros((S, samples(113)), np.int16))
        with pytest.raises(ValueError, match="chunks"):
            it.step(x, 0)
        with pytest.raises(ValueError, match="chunks"):
            it.step(x, 3)                                        # 2 560 is no multiple of 3
        with pytest.raises(ValueError, match="group"):
            it.step(x, group=9)
        with pytest.raises(ValueError, match="active"):
            it.step(x, active=[True, False])
        with pytest.raises(ValueError, match="reset"):
            it.step(x, reset=np.zeros(S + 1, bool))
        with pytest.raises(ValueError):
            it.step(x[:2])
    assert tr.calls == {}
    with pytest.raises(ValueError):
        firered.FireRedStreamBatch(eng, 0)
    with pytest.raises(ValueError, match="smooth_window_size"):
        firered.FireRedStreamBatch(eng, 2, post=(17, 0.4, 5, 8, 2000, 20))
    with pytest.raises(ValueError, match="N2"):
        firered.FireRedStreamBatch(firered.FireRedEngine(weights.firered_synthetic(1234), CHUNK), 2)
    assert np.array_equal(it.frames_done, np.zeros(S)) and not bool(it.record.any())      # nothing ran
    assert it.open_segments() == [None] * S


# ------------------------------------------------------------------ stream_detect over a list of clips
DETECT_LENGTHS = [100, 399, 400, 2560, 2600, 2960, 5120 + 1, 12345]
# threshold 0.36 at a smoothing window of 3: on the float32 CPU oracle (oracle.firered.run_clip_stream, these weights and clips) no smoothed
# probability of any clip lies within 1.1e-2 of it, and the two longest clips have 2 and 3 segments
DETECT_POST = (3, 0.36, 3, 3, 12, 3)


def test_stream_detect_over_a_list_of_clips(gemm):
    """Clips under one window, of exactly one, of one chunk, one chunk + 40 samples (the padded last chunk's frame lies beyond the valid
    count: skipped), + 400, two chunks + 1 sample, and 12 345 samples, as the streams of one batch: each clip's track and segments are
    those of `stream_detect(clip[None, :])` on a float32-mode engine."""
    eng, eng32 = engine(DEFAULT), engine(DEFAULT, "f32")
    clips = [weights.burst_clips(1, n, seed=11 + n, sample_rate=4000)[0] for n in DETECT_LENGTHS]
    out, tracks = eng.stream_detect(clips, post=DETECT_POST, return_probs=True)
    assert len(out) == len(tracks) == len(clips)
    assert [len(t) for t in tracks] == [0, 0, 1, 14, 14, 15, 29, 67]
    thr, ws = np.float32(DETECT_POST[1]), DETECT_POST[0]
    for b, c in enumerate(clips):
        want, want_track = eng32.stream_detect(c[None, :], post=DETECT_POST, return_probs=True)
        assert tracks[b].shape == want_track[0].shape, b
        np.testing.assert_allclose(tracks[b], want_track[0], rtol=0, atol=ATOL)
        if gemm == "f32":
            assert np.array_equal(tracks[b], want_track[0]), b
        csum = np.concatenate([[0.0], np.cumsum(want_track[0], dtype=np.float64)])
        k = np.arange(1, len(want_track[0]) + 1)
        smooth = (csum[k] - csum[np.maximum(k - ws, 0)]) / np.minimum(k, ws)
        assert len(smooth) == 0 or np.min(np.abs(smooth - thr)) > 1e-3, b          # the threshold was chosen for this
        assert out[b] == want[0], b
    assert len(out[-1]) >= 2 and len(out[-2]) >= 1 and out[0] == out[1] == []
    assert eng.stream_detect(clips, post=DETECT_POST) == out
    assert eng.stream_detect([], post=DETECT_POST) == []
    assert eng32.blobs.mode() == "f32" and eng.blobs.mode() == gemm


# ------------------------------------------------------------------ the reference's own streaming run
GOLDEN_CFGS = {1234: dict(weights.FIRERED_CFG, N2=0, S2=0), 7: dict(weights.FIRERED_CFG, R=3, M=2, H=64, P=32, N1=8, S1=2, N2=0, S2=0)}


@pytest.mark.parametrize("seed", [1234, 7])
def test_reference_fixture_one_chunk_per_tick(golden, gemm, seed):
    """tests/golden/firered_stream.npz (probabilities and caches the reference modules produced over its chunk loop) through
    FireRedStreamBatch, one chunk per tick, with the tolerances tests/test_gpu_firered.py holds the session to on that fixture."""
    g = golden("firered_stream")
    eng = firered.FireRedEngine(weights.firered_synthetic(seed, GOLDEN_CFGS[seed]), CHUNK)
    it = firered.FireRedStreamBatch(eng, 1)
    clip = g[f"s{seed}_clip"]
    probs, pos = [], 0
    while pos < len(clip):
        chunk = clip[pos:pos + CHUNK]
        if len(chunk) < 400:
            chunk = np.pad(chunk, (0, 400 - len(chunk)), mode="constant")
        pr, _ = it.step(chunk[None, :])
        if pos == 0:
            np.testing.assert_allclose(it.caches.permute(1, 0, 2, 3).cpu().numpy(), g[f"s{seed}_caches_first"], rtol=0, atol=1e-3)
        probs.append(pr[0, 0].cpu().numpy())
        pos += CHUNK
    got, want = np.concatenate(probs), g[f"s{seed}_probs"]
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    m = (want > 0) & (want < 1 - 1e-3)                           # the fixture comparison in logit space (LOGIT_ATOL = ATOL / 0.25)
    assert m.any()
    np.testing.assert_allclose(logit(got[m]), logit(want[m]), rtol=0, atol=4e-4)
    np.testing.assert_allclose(it.caches.permute(1, 0, 2, 3).cpu().numpy(), g[f"s{seed}_caches_last"], rtol=0, atol=1e-3)
    assert int(it.frames_done[0]) == len(got)
