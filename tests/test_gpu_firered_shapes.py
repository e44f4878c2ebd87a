"""GPU parity: the FireRed DFSMN at every tile size of the window walk, at layer widths other than the checkpoint's and at every FIR tap shape,
compared in logit space.

tests/test_gpu_firered.py runs one window length (16 000 samples, T = 98 frames), one stream chunk (T = 14, and a T = 1 tail) and one width per
kernel path (256 / 128 on the split-product and register-resident kernels, 64 / 32 and 48 / 24 on `layer<>`).  Here the window length sweeps
every tile sequence of `pointwise_pair` / `pair_tile_resident` (32-frame tiles and a 16-frame half tile), every remainder of the 16-frame walk
of `pointwise_pair_split` and the 14-frame segments of `fsmn_memory_fast`; the widths sweep the zero padding of the split fragments
(H 241 .. 256, P 113 .. 128), the `M > 1` tail, R = 1 and 16, odim = 4 and the wide non-resident pair; the tap shapes leave the fast FIR one
step at a time (21 taps, dilation, a reach beyond the window); the stream kernel runs chunks shorter and longer than its cache, of one tile
and of several, with caches carried over five ragged chunks.

The reference is oracle.firered.detect_model / detect_model_stream in float64 on the DEVICE's own log-mel, so that only the net is measured
(the front-end is pinned by tests/test_gpu_frontend.py).  A random net's sigmoid saturates (tests/golden's seed-7 probabilities are all below
1e-5, where any kernel passes an absolute tolerance), so every case re-centres its output head from the float64 logits of the unmodified
weights -- per channel mean 0, standard deviation 1.5 -- and asserts on the reference that at least 90 % of its values lie in (0.02, 0.98).
Errors are taken in logit space over those values and divided by sd(z_ref), which makes them independent of the head's scale.

The bound on that error e is measured, not chosen: with e_dev(pinned) the device's error at the pinned shape (default config, T = 98, seed
1234) on the same arithmetic in the same session, e_32 the float32 torch oracle's error against the float64 one on the same input, and
R_arith = e_dev(pinned) / e_32(pinned), every case must hold e_dev(case) <= 2 max(e_dev(pinned), R_arith e_32(case)): the kernels claim
float32 grade, depth and width legitimately move the float32 error, so each case is held to the float32 reference's own error at that case,
scaled by the ratio seen at the pinned shape, with a factor 2 for the max-over-few-values noise of both terms.  The stream kernel runs float32
MFMAs whatever the arithmetic, so its probabilities take the float32 figures; the non-stream net has no caches, so `caches_out` (error / max
|reference| per layer) takes the same form from the stream's own pinned shape (default config without look-ahead, T = 14).

N1 = 1 is left out of the stream cases on purpose: its cache is empty, and the oracle's `seq[:, :, -0:]` is the whole sequence, not a cache.
"""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, firered, weights
from vadx import frontend as vfe
from oracle import firered as ofr

pytestmark = pytest.mark.gpu
ATOL = 1e-4                    # probabilities: the file-wide ATOL of tests/test_gpu_firered.py
CACHE_ATOL = 1e-3              # caches_out: the absolute bound of test_stream_session_matches_reference_fixture
FACTOR = 2.0
INSIDE, LO, HI = 0.9, 0.02, 0.98
B = 4
BASE_SEED, BASE_T, STREAM_BASE_T = 1234, 98, 14
WIDTH_SEED = 7
ARITHS = ["f32", "split", "h2"]


@pytest.fixture(autouse=True)
def gemm(request):
    """The arithmetic the engines are asked for: the three of them where `three_arithmetics` parametrises the test, the package default
    (fp16 x 2) otherwise -- a config the split kernels do not take must then fall back to float32 MFMAs by itself, and runs once."""
    mode = getattr(request, "param", "h2")
    prev = _lib.gemm_mode(mode)
    yield mode
    _lib.gemm_mode(prev)


three_arithmetics = pytest.mark.parametrize("gemm", ARITHS, indirect=True)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def make_cfg(key):
    return dict(weights.FIRERED_CFG, **dict(key))


def split_eligible(cfg):
    """csrc/firered.hip: the split-product kernels run where the widths pad to 256 / 128"""
    return (cfg["H"] + 15) // 16 * 16 == 256 and (cfg["P"] + 15) // 16 * 16 == 128


def samples(frames):
    return 400 + 160 * (frames - 1)


def clips_for(L, seed):
    """B burst windows, the first half of clip 0 digital silence"""
    clips = weights.burst_clips(B, L, seed=L + seed)
    clips[0, :L // 2] = 0
    return clips


def logit(p):
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(p) - np.log1p(-p)


def model(w, feats, caches, dtype):
    """The oracle in `dtype` on log-mel chunks [B, 80, T_i]: (probs [B, odim, sum T_i], caches after every chunk); caches = None is the
    non-stream net (one chunk), otherwise the stream net carries `caches` [R, B, P, pad] from chunk to chunk."""
    wt = {k: (T(v).to(dtype) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    with torch.no_grad():
        if caches is None:
            return ofr.detect_model(wt, T(feats[0]).to(dtype)).numpy(), []
        c, probs, after = T(caches).to(dtype), [], []
        for f in feats:
            p, c = ofr.detect_model_stream(wt, T(f).to(dtype), c)
            probs.append(p.numpy())
            after.append(c.numpy())
    return np.concatenate(probs, axis=2), after


def recentred(w, feats, caches):
    """`w` with its output head re-centred per channel on the float64 logits z of `w` itself: out_w *= 1.5 / sd(z),
    out_b = (out_b - mean(z)) * 1.5 / sd(z), stored as float32.  (z is read through a head scaled by 2^-10, where the sigmoid is invertible
    to full precision whatever the unmodified head's scale.)"""
    probe = dict(w, out_w=w["out_w"] * np.float32(2.0 ** -10), out_b=w["out_b"] * np.float32(2.0 ** -10))
    z = logit(model(probe, feats, caches, torch.float64)[0]) * 2.0 ** 10
    mu, s = z.mean(axis=(0, 2)), 1.5 / z.std(axis=(0, 2))
    return dict(w, out_w=(w["out_w"].astype(np.float64) * s[:, None]).astype(np.float32),
                out_b=((w["out_b"].astype(np.float64) - mu) * s).astype(np.float32))


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


_REF = {}          # case -> the device log-mel, the re-centred weights and both oracles on them: computed once, shared by the arithmetics
_BASE = {}         # arithmetic (or "stream") -> the figures of the pinned shape


def reference(name, w0, feats, caches):
    hit = _REF.get(name)
    if hit is None:
        w = recentred(w0, feats, caches)
        p64, c64 = model(w, feats, caches, torch.float64)
        p32, c32 = model(w, feats, caches, torch.float32)
        hit = dict(feats=feats, w=w, p=p64, c=c64, e32=logit_error(p32, p64), p32=float(np.abs(p32 - p64).max()),
                   c32=cache_errors(c32, c64)[1].max() if caches is not None else None,
                   inside=float(((p64 > LO) & (p64 < HI)).mean()))
        _REF[name] = hit
    # a saturated sigmoid tests nothing: the reference itself must sit where an error shows
    assert hit["inside"] >= INSIDE, (name, hit["inside"])
    return hit


def logmel_of(fe, audio, L):
    """the device's log-mel [B, T, 80] as the oracle's feature layout [B, 80, T] (host)"""
    return np.ascontiguousarray(fe.logmel(audio, 1, L).cpu().numpy().transpose(0, 2, 1))


def run_case(gemm, key, frames, seed):
    """One launch of B windows of `frames` frames on config `key` and its float64 reference -> the case's figures; what holds for every
    shape is asserted here."""
    cfg, L = make_cfg(key), samples(frames)
    audio = T(clips_for(L, seed)).cuda()
    name = ("window", key, frames, seed)
    feats = _REF[name]["feats"] if name in _REF else [logmel_of(vfe.Frontend("firered", L), audio, L)]
    ref = reference(name, weights.firered_synthetic(seed, cfg), feats, None)
    eng = firered.FireRedEngine(ref["w"], L)
    assert eng.T == frames
    assert np.array_equal(logmel_of(eng.fe, audio, L), ref["feats"][0])         # the reference saw what the net sees
    probs = eng.run(audio, 1)
    # `blobs.mode()` is the REQUESTED arithmetic; the cfg the launch used says which kernel ran
    want = gemm if split_eligible(cfg) else "f32"
    assert eng.cfg.arithmetic == _lib.GEMM_MODES[want], (eng.cfg.arithmetic, want)
    assert eng.blobs.range_fallbacks == 0
    got = probs.cpu().numpy().astype(np.float64)
    assert got.shape == ref["p"].shape == (B, cfg["odim"], frames)
    assert np.isfinite(got).all()
    out = dict(arith=want, p=float(np.abs(got - ref["p"]).max()), e=logit_error(got, ref["p"]), e32=ref["e32"], p32=ref["p32"], inside=ref["inside"])
    print(f"firered shapes window {want} T={frames} {cfg_name(key)}: p {out['p']:.2e} e {out['e']:.2e} e32 {out['e32']:.2e} "
          f"p32 {out['p32']:.2e} inside {out['inside']:.3f}")
    assert out["p"] <= ATOL, out
    return out


def cfg_name(key):
    return "default" if not key else ",".join(f"{k}={v}" for k, v in key)


def pinned(arith):
    """the pinned shape's figures on `arith`, measured once per session: (e_dev, R_arith = e_dev / e_32)"""
    if arith not in _BASE:
        prev = _lib.gemm_mode(arith)
        try:
            r = run_case(arith, (), BASE_T, BASE_SEED)
        finally:
            _lib.gemm_mode(prev)
        _BASE[arith] = (r["e"], r["e"] / r["e32"])
        print(f"firered shapes pinned {arith}: e {r['e']:.2e} e32 {r['e32']:.2e} R_arith {_BASE[arith][1]:.3f}")
    return _BASE[arith]


def assert_float32_grade(arith, e, e32, what):
    e_pin, ratio = pinned(arith)
    bound = FACTOR * max(e_pin, ratio * e32)
    print(f"    e {e:.2e} bound {bound:.2e} (pinned {e_pin:.2e}, R_arith {ratio:.3f}, e32 {e32:.2e})")
    assert e <= bound, (what, e, bound, e_pin, ratio, e32)


def window_case(gemm, key, frames, seed):
    r = run_case(gemm, key, frames, seed)
    assert_float32_grade(r["arith"], r["e"], r["e32"], (key, frames))


# every float32 tile sequence (half only; full; full + half; full + partial full; three full + half at MAX_T), every remainder class of the
# 16-frame split walk, the 14-frame FIR segment edges, and T = 1, which takes the generic FIR
LENGTHS = [1, 2, 14, 15, 16, 17, 29, 31, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 111, 112]


@three_arithmetics
@pytest.mark.parametrize("frames", LENGTHS)
def test_window_length_sweep(gemm, frames):
    """Default config at every tile sequence: probabilities within 1e-4 of the float64 net, logits at float32 grade."""
    window_case(gemm, (), frames, BASE_SEED)


def K(**kw):
    return tuple(kw.items())


WIDTHS_SPLIT = [K(H=250, P=120), K(H=241, P=113), K(M=2), K(M=4, odim=4), K(R=16), K(R=1)]
WIDTHS_F32 = [K(H=256, P=112), K(H=240, P=128), K(H=16, P=16, R=2), K(H=17, P=1, R=2), K(H=48, P=24, M=4, odim=4), K(H=64, P=32, R=3, M=2)]


@three_arithmetics
@pytest.mark.parametrize("frames", [98, 41])
@pytest.mark.parametrize("key", WIDTHS_SPLIT, ids=cfg_name)
def test_width_sweep_split_eligible(gemm, key, frames):
    """Widths the split kernels take (Hp = 256, Pp = 128): rows and k-groups that only `pack::split`'s zero padding and the padded biases
    supply, the `M > 1` tail behind the resident dnn[0], the deepest and the shallowest stack, four output channels."""
    window_case(gemm, key, frames, WIDTH_SEED)


@pytest.mark.parametrize("frames", [98, 41])
@pytest.mark.parametrize("key", WIDTHS_F32, ids=cfg_name)
def test_width_sweep_float32_only(gemm, key, frames):
    """Widths the split kernels do not take: the engine, asked for the default fp16 x 2, packs and runs float32 MFMAs (run_case asserts the
    cfg's arithmetic) -- wide but non-resident (256 / 112, 240 / 128), one n-tile, a one-channel trunk, `layer<>` with M = 4 and odim = 4."""
    window_case(gemm, key, frames, WIDTH_SEED)


# the weights' seed where 1234 leaves the re-centred float64 reference with heavy tails (88 % inside (0.02, 0.98) at one tap a side; found on
# the CPU, float64 net on the oracle's log-mel: seed 4 keeps 98 %)
TAP_SEEDS = {(1, 1, 1, 1): 4}
TAPS = [(21, 1, 20, 1), (20, 1, 21, 1), (20, 1, 20, 2), (1, 1, 1, 1), (3, 1, 0, 0), (32, 4, 32, 4), (8, 2, 4, 3)]


@three_arithmetics
@pytest.mark.parametrize("frames", [98, 41, 20])
@pytest.mark.parametrize("taps", TAPS, ids=lambda t: "-".join(map(str, t)))
def test_tap_shape_sweep(gemm, taps, frames):
    """(N1, S1, N2, S2) at default widths: 21 taps on either side (the first shapes to leave the fast FIR), a dilated look-ahead, one tap,
    no look-ahead, a reach of 124 frames (beyond every window here; R = 2), the dilated pair of tests/golden's seed 7."""
    n1, s1, n2, s2 = taps
    key = K(N1=n1, S1=s1, N2=n2, S2=s2) + (K(R=2) if n1 == 32 else ())
    window_case(gemm, key, frames, TAP_SEEDS.get(taps, BASE_SEED))


# ------------------------------------------------------------------ the stream kernel (one arithmetic: float32 MFMAs)
STREAM_CFGS = [K(N2=0, S2=0), K(H=64, P=32, R=3, M=2, N1=8, S1=2, N2=0, S2=0), K(N1=2, N2=0, S2=0), K(N1=32, S1=3, R=2, N2=0, S2=0),
               K(H=250, P=120, N2=0, S2=0)]
# the weights' seed per config: the one of a few tried (CPU, float64 net on the oracle's log-mel) whose re-centred reference keeps at least 95 %
# of its values inside (0.02, 0.98) at every chunk length below; the tests assert 90 % on the reference they compare with.  N1 = 2 (taps of
# 0.35 on a gain of 1 + w, eight blocks deep) is badly conditioned at most seeds: the float32 ORACLE's own e_32 then moves by 3 x (seed 1234)
# to 25 x (seed 39) between chunk lengths, which the bound's factor 2 for max-over-few-values noise cannot absorb; seed 31 is the one of
# 1234, 4, 12 .. 39 where it stays within 2.3 x (1.84e-6 .. 4.23e-6 at seed 19 is as good, with 95.3 % inside against 98.1 %)
STREAM_SEEDS = dict(zip(STREAM_CFGS, [BASE_SEED, 2, 31, 9, WIDTH_SEED]))
STREAM_FRAMES = [1, 2, 13, 14, 16, 17, 19, 20, 32, 33, 64, 65, 112]


def run_stream(key, chunk_frames, seed, random_caches):
    """Chunks of `chunk_frames` frames for B streams through `stream_run`, the device carrying its own caches and the reference its own."""
    cfg = make_cfg(key)
    R, P, pad = cfg["R"], cfg["P"], (cfg["N1"] - 1) * cfg["S1"]
    lens = [samples(f) for f in chunk_frames]
    clips = clips_for(sum(lens), seed)
    chunks = [T(clips[:, sum(lens[:i]):sum(lens[:i + 1])]).cuda() for i in range(len(lens))]
    rng = np.random.default_rng(seed + sum(chunk_frames))
    c0 = (rng.standard_normal((R, B, P, pad)) * 0.3 if random_caches else np.zeros((R, B, P, pad))).astype(np.float32)
    name = ("stream", key, tuple(chunk_frames), seed)
    feats = _REF[name]["feats"] if name in _REF else [logmel_of(vfe.Frontend("firered", n), a, n) for a, n in zip(chunks, lens)]
    ref = reference(name, weights.firered_synthetic(seed, cfg), feats, c0)
    eng = firered.FireRedEngine(ref["w"], firered.STREAM_CHUNK_SAMPLES)
    caches, probs, after = T(c0).cuda(), [], []
    for a, n, f in zip(chunks, lens, ref["feats"]):
        assert np.array_equal(logmel_of(eng._frontend_for(n), a, n), f)
        keep = caches.clone()
        p, cout = eng.stream_run(a, caches)
        assert torch.equal(caches, keep)                                      # caches_in is read only
        assert cout.shape == caches.shape and cout.data_ptr() != caches.data_ptr()
        probs.append(p.cpu().numpy().astype(np.float64))
        after.append(cout.cpu().numpy())
        caches = cout
    got = np.concatenate(probs, axis=2)
    assert got.shape == ref["p"].shape == (B, cfg["odim"], sum(chunk_frames))
    assert np.isfinite(got).all() and all(np.isfinite(c).all() for c in after)
    c_abs, c_rel = cache_errors(after, ref["c"])
    out = dict(p=float(np.abs(got - ref["p"]).max()), e=logit_error(got, ref["p"]), e32=ref["e32"], c_abs=c_abs, c=float(c_rel.max()), c32=float(ref["c32"]))
    print(f"firered shapes stream f32 T={'+'.join(map(str, chunk_frames))} {cfg_name(key)}: p {out['p']:.2e} e {out['e']:.2e} e32 {out['e32']:.2e} "
          f"cache {out['c_abs']:.2e} rel {out['c']:.2e} rel32 {out['c32']:.2e} per layer " + " ".join(f"{v:.1e}" for v in c_rel) + f" inside {ref['inside']:.3f}")
    assert out["p"] <= ATOL, out
    assert out["c_abs"] <= CACHE_ATOL, out
    return out


def stream_pinned():
    """the stream's pinned shape (default config without look-ahead, one 14-frame chunk): (c_dev, c_dev / c_32) of `caches_out`"""
    if "stream" not in _BASE:
        r = run_stream(STREAM_CFGS[0], [STREAM_BASE_T], BASE_SEED, True)
        _BASE["stream"] = (r["c"], r["c"] / r["c32"])
        print(f"firered shapes pinned stream: cache rel {r['c']:.2e} rel32 {r['c32']:.2e} R_cache {_BASE['stream'][1]:.3f}")
    return _BASE["stream"]


def stream_case(key, chunk_frames, seed, random_caches):
    r = run_stream(key, chunk_frames, seed, random_caches)
    assert_float32_grade("f32", r["e"], r["e32"], (key, chunk_frames))
    c_pin, ratio = stream_pinned()
    bound = FACTOR * max(c_pin, ratio * r["c32"])
    print(f"    cache rel {r['c']:.2e} bound {bound:.2e} (pinned {c_pin:.2e}, R_cache {ratio:.3f}, rel32 {r['c32']:.2e})")
    assert r["c"] <= bound, (key, chunk_frames, r["c"], bound)


@pytest.mark.parametrize("frames", STREAM_FRAMES)
@pytest.mark.parametrize("key", STREAM_CFGS, ids=cfg_name)
def test_stream_chunk_sweep(gemm, key, frames):
    """One chunk on random caches 0.3 N(0, 1): chunks shorter than the cache (pad = 19, 14, 1, 93), as long, longer (no entry of the new cache
    comes from the old one), of one tile and of several up to 112 frames; probabilities and `caches_out` against float64."""
    stream_case(key, [frames], STREAM_SEEDS[key], True)


@pytest.mark.parametrize("key", STREAM_CFGS[:2], ids=cfg_name)
def test_stream_carried_over_ragged_chunks(gemm, key):
    """Five chunks of 14, 1, 33, 19 and 2 frames from zero caches: every chunk's probabilities and caches against the float64 net carrying
    its own."""
    stream_case(key, [14, 1, 33, 19, 2], STREAM_SEEDS[key], False)


# ------------------------------------------------------------------ limits
def test_more_than_112_frames_is_refused_before_any_launch(gemm):
    """T = 113 (18 320 samples) does not fit the kernels' LDS rows: the engine and `stream_run` refuse it by name, and no entry point of the
    library was called on the way."""
    with _lib.trace() as tr:
        with pytest.raises(ValueError, match="at most 112 frames"):
            firered.FireRedEngine(weights.firered_synthetic(BASE_SEED), 18320)
    assert tr.calls == {}
    eng = firered.FireRedEngine(weights.firered_synthetic(BASE_SEED, make_cfg(STREAM_CFGS[0])), firered.STREAM_CHUNK_SAMPLES)
    caches = eng.new_caches(1)
    audio = torch.zeros((1, 18320), dtype=torch.int16, device="cuda")
    with _lib.trace() as tr:
        with pytest.raises(ValueError, match="at most 112 frames"):
            eng.stream_run(audio, caches)
    assert tr.calls == {}
    probs, _ = eng.stream_run(audio[:, :samples(112)].contiguous(), caches)     # 112 frames is the longest chunk, and runs
    assert probs.shape == (1, 1, 112) and bool(torch.isfinite(probs).all())
