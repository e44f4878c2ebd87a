"""GPU parity: MarbleNet at every tile edge of its three fused kernel families, on the per-sub-block launches they replace, and on layouts other
than the published 3x2x64 (the generic `sepconv_block_kernel<0,0,0>`, `frame_classifier_kernel` at C != 128), compared in logit space.

tests/test_gpu_marblenet.py holds softmax probabilities of a few long clips to 1e-4; here the score-frame count T' (frames after block 1's
stride 2) sweeps one frame, the 32-frame tile and its multiples with their neighbours, the 2 PAD = 12 / 14 / 16-frame halo of the fused
blocks, the 28-frame halo of the tail and the 48-column sub-block-0 tile, each at T = 2 T' - 1 and some at T = 2 T' (both parities in front
of the stride-2 prologue), on three paths: the fused launches on float32 MFMAs, the fused launches on fp16 x 2 split products, and the ten
per-sub-block launches (compile-time FIRs 11/1/2, 13, 15, 17, 29/2).  Other layouts run the generic kernel: runtime k / dilation / stride,
channel counts that pad to 16, residual blocks of one and three sub-blocks and with cin != cout, a plain block in the middle.

The reference is oracle.marblenet.encoder + the decoder Linear in float64 on the DEVICE's own log-mel, fed through
`MarbleNetEngine.run_features` (the front-end is pinned by tests/test_gpu_frontend.py); the array the device was fed is asserted equal to
the one the reference saw.  Windows of fewer than 6 frames (800 samples is the shortest window the front-end's own tests run) are the first T
frames of a one-second window's log-mel.

A random net's softmax saturates (seed 7 at L = 16000: 63 % of the probabilities inside (0.02, 0.98)), and an absolute tolerance on a
saturated probability checks next to nothing.  So every weight set's decoder is re-centred in `_MARBLENET_DEC_CALIB`'s form -- row 0 kept,
row 1 = row 0 + s (row 1 - row 0), bias 1 shifted by -s mean(z) -- from the float64 logits z = z1 - z0 of the unmodified weights on the
pinned input (B one-second burst clips, T = 101), so that z has mean 0 and sd 1.5 there; every case asserts ON THE REFERENCE that at least
90 % of its probabilities lie in (0.02, 0.98).  The device logit is log(s1) - log(s0) of the two float32 scores, in double; the error e is
max |z - z_ref| over the in-range values divided by sd(z_ref) of the weight set's pinned input.  (tests/test_gpu_marblenet.py's four session cases come
here too, through `run` with the front-end in it; each is one window, and its head is centred on that window's own log-mel.)

The bound is measured, not chosen: with e_dev(pinned) the device's error at the pinned shape (seed 1234, published layout, T = 101, T' = 51)
on the same path in the same session, e_32 the float32 torch oracle's error against the float64 one on the same input, and R_arith =
e_dev(pinned) / e_32(pinned), every case holds e_dev(case) <= 2 max(e_dev(pinned), R_arith e_32(case)); the factor 2 covers the
max-over-few-values noise of both terms.  profiles/marblenet_shapes_errors.txt keeps one run's table.  The absolute 1e-4 on probabilities
stays as a second, unconditional assert.

Seeds.  Weights: 1234 on the published layout, 7 on the others.  Clips: weights.burst_clips(seed = samples + 1234), the first half of clip 0
digital silence.  They were checked on the CPU (float64 net on the oracle's log-mel) against the 90 % condition for every case below; a case
whose reference keeps less than 95 % there takes the clip seed named in CLIP_SEEDS.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vadx  # noqa: F401
from vadx import _lib, marblenet, weights
from oracle import marblenet as omb

pytestmark = pytest.mark.gpu
ATOL = 1e-4                    # probabilities: the file-wide ATOL of tests/test_gpu_marblenet.py
FACTOR = 2.0
INSIDE, LO, HI = 0.9, 0.02, 0.98
BASE_SEED, WIDTH_SEED, BASE_T = 1234, 7, 101
MIN_FRONTEND_T = 6             # shorter windows are cut from a BASE_T-frame window's log-mel
PUBLISHED = tuple(weights.MARBLENET_BLOCKS)
PATHS = ["f32", "h2", "unfused"]                                   # fused launches on either arithmetic; per-sub-block launches (float32)
# (layout name, T) -> clip seed where BASE_SEED's clips leave the float64 reference with less than 95 % in range on the CPU (82 .. 94 %: mostly
# T = 37, where half of clip 0 -- an eighth of the case -- is digital silence and one long loud or quiet stretch fills a whole clip): the
# first seed of 1235, 1236, ... that keeps 95 %.  The tests assert the 90 % on the reference they compare with.
CLIP_SEEDS = {
    ("published", 257): 1237, ("k1", 37): 1235, ("k8", 37): 1236, ("k7s3", 65): 1236, ("k7s3", 37): 1235, ("k69", 65): 1236,
    ("f1", 65): 1236, ("f1", 37): 1239, ("f2", 65): 1236, ("f2", 37): 1239, ("f17", 65): 1236, ("f17", 37): 1239, ("f128", 37): 1241,
    ("res40to100", 65): 1236, ("res40to100", 37): 1239, ("last2", 37): 1239, ("last17", 65): 1236, ("last17", 37): 1239,
}


def T_(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def samples(frames):
    return 160 * (frames - 1)


def clips_for(n, L, seed):
    """n burst windows, the first half of clip 0 digital silence"""
    clips = weights.burst_clips(n, L, seed=L + seed)
    clips[0, :L // 2] = 0
    return clips


def net(w, feats, blocks, dtype):
    """The oracle in `dtype` on log-mel [N, T, 80]: (z = z1 - z0 from the logits, scores [N, T', 2], T'), all float64 numpy"""
    wt = {k: T_(v).to(dtype) for k, v in w.items()}
    with torch.no_grad():
        enc, length = omb.encoder(wt, T_(feats.transpose(0, 2, 1)).to(dtype), blocks)
        logits = F.linear(enc.transpose(1, 2), wt["dec_w"], wt["dec_b"])
        s = torch.softmax(logits, dim=-1)
    logits, s = logits.double().numpy(), s.double().numpy()
    assert logits.shape[1] == length
    return logits[..., 1] - logits[..., 0], s, int(length)


def score_logit(s0, s1):
    """log(s1) - log(s0) of two float32 scores, in double"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(s1, dtype=np.float64)) - np.log(np.asarray(s0, dtype=np.float64))


def recentred(w, blocks, pin_feats):
    """`w` with its decoder re-centred on the float64 logits z of `w` itself on the pinned input: mean 0, sd 1.5 (float32 storage)"""
    z = net(w, pin_feats, blocks, torch.float64)[0]
    s, mu = 1.5 / z.std(), z.mean()
    dw, db = w["dec_w"].astype(np.float64), w["dec_b"].astype(np.float64)
    dw[1] = dw[0] + s * (dw[1] - dw[0])
    db[1] = db[0] + s * (db[1] - db[0]) - s * mu
    return dict(w, dec_w=dw.astype(np.float32), dec_b=db.astype(np.float32))


def logit_error(z, z_ref, p_ref, sd):
    """max |z - z_ref| / sd over the values where the reference probability lies in (LO, HI)"""
    m = (p_ref > LO) & (p_ref < HI)
    return float(np.abs(z[m] - z_ref[m]).max() / sd)


_PIN = {}          # "feats" -> the pinned input (device log-mel of the pinned clips, host copy)
_SETS = {}         # (layout name, seed) -> the weight set: blocks, re-centred weights, sd(z_ref) on the pinned input, its engine
_REF = {}          # case -> the device log-mel it was fed and both oracles on it: computed once, shared by the paths
_BASE = {}         # path -> the figures of the pinned shape


def device_logmel(eng, frames, seed, n):
    """[n, frames, 80] on the device: the engine's own log-mel of n burst windows, or, for windows the front-end is not run at, the first
    frames of a BASE_T-frame window's"""
    take = frames if frames >= MIN_FRONTEND_T else BASE_T
    L = samples(take)
    x = eng.frontend(L).logmel(T_(clips_for(n, L, seed)).cuda(), 1, L)
    assert x.shape == (n, take, 80)
    return x[:, :frames].contiguous()


def weight_set(name, blocks, seed, pin=None):
    """The weight set `name`: marblenet_synthetic(seed, blocks) with its decoder re-centred on `pin` (default: the pinned input)"""
    key = (name, seed)
    if key not in _SETS:
        if pin is None:
            if "feats" not in _PIN:
                eng = marblenet.MarbleNetEngine(weights.marblenet_synthetic(BASE_SEED))
                _PIN["feats"] = device_logmel(eng, BASE_T, BASE_SEED, 4).cpu().numpy()
            pin = _PIN["feats"]
        w = recentred(weights.marblenet_synthetic(seed, blocks), blocks, pin)
        _SETS[key] = dict(blocks=blocks, w=w, sd=float(net(w, pin, blocks, torch.float64)[0].std()), eng=marblenet.MarbleNetEngine(w, blocks=blocks))
    return _SETS[key]


def reference(case, ws, feats):
    hit = _REF.get(case)
    if hit is None:
        z64, s64, frames = net(ws["w"], feats, ws["blocks"], torch.float64)
        _, s32, _ = net(ws["w"], feats, ws["blocks"], torch.float32)
        p64 = s64[..., 1]
        hit = dict(feats=feats, z=z64, p=p64, frames=frames, inside=float(((p64 > LO) & (p64 < HI)).mean()))
        if hit["inside"] > 0:
            hit["e32"] = logit_error(score_logit(s32[..., 0], s32[..., 1]), z64, p64, ws["sd"])
        hit["p32"] = float(np.abs(s32 - s64).max())
        _REF[case] = hit
    # a saturated softmax tests nothing: the reference itself must sit where an error shows
    assert hit["inside"] >= INSIDE, (case, hit["inside"])
    return hit


def run_case(path, name, blocks, frames, wseed):
    """One launch sequence of B windows of `frames` log-mel frames on layout `blocks` and its float64 reference -> the case's figures"""
    ws = weight_set(name, blocks, wseed)
    n = 8 if (frames + 1) // 2 <= 4 else 4
    cseed = CLIP_SEEDS.get((name, frames), BASE_SEED)
    case = (name, wseed, frames, cseed)
    x = T_(_REF[case]["feats"]).cuda() if case in _REF else device_logmel(ws["eng"], frames, cseed, n)
    return compare(path, f"{name} T={frames}", case, ws, x, lambda eng: eng.run_features(x))


def compare(path, label, case, ws, x, launch):
    """`launch(engine)` on `path` against the float64 reference on the log-mel `x` it is fed; what holds for every shape is asserted here"""
    eng, published = ws["eng"], ws["blocks"] == PUBLISHED
    ref = reference(case, ws, x.cpu().numpy())
    prev = _lib.gemm_mode("h2" if path == "h2" else "f32")
    try:
        assert eng.fused == published                                         # another layout has no fused form
        eng.fused = published and path != "unfused"
        s0, s1, slen = launch(eng)
        assert eng.mode() == ("h2" if path == "h2" else "f32")
        assert eng.range_fallbacks == 0
    finally:
        eng.fused = published
        _lib.gemm_mode(prev)
    assert np.array_equal(x.cpu().numpy(), ref["feats"])                          # the reference saw what the net was fed
    s0, s1 = s0.cpu().numpy(), s1.cpu().numpy()
    assert s0.dtype == s1.dtype == np.float32
    assert s0.shape == s1.shape == ref["p"].shape == (x.shape[0], ref["frames"]) and slen == ref["frames"] - 1
    assert np.isfinite(s0).all() and np.isfinite(s1).all()
    assert float(np.abs(s0.astype(np.float64) + s1 - 1.0).max()) <= 1e-5
    z = score_logit(s0, s1)
    out = dict(p=float(np.abs(s1.astype(np.float64) - ref["p"]).max()), e=logit_error(z, ref["z"], ref["p"], ws["sd"]), e32=ref["e32"],
               p32=ref["p32"], inside=ref["inside"])
    print(f"marblenet shapes {path} {label} T'={ref['frames']}: p {out['p']:.2e} e {out['e']:.2e} e32 {out['e32']:.2e} "
          f"p32 {out['p32']:.2e} inside {out['inside']:.3f}")
    assert np.isfinite(out["e"]), out
    assert out["p"] <= ATOL, out
    assert float(np.abs(s0.astype(np.float64) - (1.0 - ref["p"])).max()) <= ATOL
    return out


def pinned(path):
    """the pinned shape's figures on `path`, measured once per session: (e_dev, R_arith = e_dev / e_32)"""
    if path not in _BASE:
        r = run_case(path, "published", PUBLISHED, BASE_T, BASE_SEED)
        _BASE[path] = (r["e"], r["e"] / r["e32"])
        print(f"marblenet shapes pinned {path}: e {r['e']:.2e} e32 {r['e32']:.2e} R_arith {_BASE[path][1]:.3f}")
    return _BASE[path]


def assert_float32_grade(path, r, what):
    e_pin, ratio = pinned(path)
    bound = FACTOR * max(e_pin, ratio * r["e32"])
    print(f"    e {r['e']:.2e} bound {bound:.2e} ratio {r['e'] / bound:.3f} (pinned {e_pin:.2e}, R_arith {ratio:.3f}, e32 {r['e32']:.2e})")
    assert r["e"] <= bound, (path, what, r["e"], bound, e_pin, ratio, r["e32"])


def shape_case(path, name, blocks, frames, wseed):
    assert_float32_grade(path, run_case(path, name, blocks, frames, wseed), (name, frames))


def session_case(path, seed, audio):
    """tests/test_gpu_marblenet.py's session cases in logit space: int16 [1, L] through `run` (front-end included) on the published layout
    with the decoder re-centred on this window's own device log-mel (one window: the head is centred where it is read), held to the
    float64 net on that log-mel at the bound measured at the pinned shape."""
    L = audio.shape[-1]
    a = T_(audio.reshape(1, L)).cuda()
    x = marblenet.MarbleNetEngine(weights.marblenet_synthetic(seed)).frontend(L).logmel(a, 1, L)
    ws = weight_set(f"session L={L}", PUBLISHED, seed, pin=x.cpu().numpy())
    assert_float32_grade(path, compare(path, f"session seed {seed} L={L}", ("session", seed, L), ws, x, lambda eng: eng.run(a)), (seed, L))


# T': one frame; the first score frames whose halo reaches the clip start (1 .. 9: PAD = 6 / 7 / 8 of the fused blocks); their 2 PAD = 12 /
# 14 / 16-frame input halo and its neighbours (14 .. 17); the tail's PAD = 28 halo (27 .. 29); the 32-frame tile, its multiples and their
# neighbours (31 .. 33, 63 .. 65, 96 / 97, 128 / 129); the 48-column sub-block-0 tile (47 .. 49); 56 / 57 = 2 PAD of the tail, where its
# second tile's halo begins at frame 4 and the `lane + 64 h` stage read first crosses the clip end
SCORE_FRAMES = [1, 2, 3, 6, 7, 8, 9, 14, 15, 16, 17, 27, 28, 29, 31, 32, 33, 47, 48, 49, 56, 57, 63, 64, 65, 96, 97, 128, 129]
EVEN_T = [1, 8, 32, 33, 64]                                        # T = 2 T': the other parity in front of the stride-2 prologue
FRAMES = sorted([2 * t - 1 for t in SCORE_FRAMES] + [2 * t for t in EVEN_T])


@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("path", PATHS)
def test_frame_count_sweep(path, frames):
    """Published layout at every tile edge: probabilities within 1e-4 of the float64 net, logits at float32 grade, on the fused launches of
    both arithmetics and on the per-sub-block launches -- each held to the oracle, not to each other."""
    shape_case(path, "published", PUBLISHED, frames, BASE_SEED)


def stack(first=(128, 1, 11, 2, 1, False, True), mid=((64, 2, 13, 1, 1, True, True),), last=(128, 1, 1, 1, 1, False, False)):
    """A small Jasper stack: a first block on the time-major log-mel, residual block(s), a plain 1x1 block in front of the decoder"""
    return (first,) + tuple(mid) + (last,)


def first_k(k, stride=1, dil=1):
    return stack(first=(128, 1, k, stride, dil, False, True))


def first_filters(f):
    return stack(first=(f, 1, 11, 2, 1, False, True))


LAYOUTS = {
    # the generic FIR at stride 1: no taps to loop over (k = 1), fewer than a vector (3, 5), an even kernel (pad 3 of 7: T - 1 frames
    # leave the block), a window of 62 frames across the tile (31)
    **{f"k{k}": first_k(k) for k in (1, 3, 5, 8, 31)},
    # dilation: `row[kk * dil]` with pad 6 and 16
    "k5d3": first_k(5, dil=3), "k9d4": first_k(9, dil=4),
    # stride 3: `row + m * stride`, `tin0 = t0 * stride - pad`; with k = 7 the tile's receptive field is 31 * 3 + 6 + 1 = 100, the largest
    # the launcher admits (in_ld = 108), as is k = 69 at stride 1 (31 + 68 + 1)
    "k7s3": first_k(7, stride=3), "k69": first_k(69),
    # filters F as the first block's cout and the residual block's cin and cres.  1 and 2: one row tile with 15 / 14 padded rows, one
    # k-group of one / two live channels (`cc = cin - 1` clamps, the `ch < c.cin` select).  17: a second row tile and k-group for ONE
    # channel.  40: cinp = 48 = one 32-channel loader pass + a leftover pass of 16, three row tiles on eight waves (the item loop).
    # 100: cinp = 112 = three loader passes + the leftover, seven row tiles.  128: four loader passes, eight row tiles = the paired
    # whole-tile rounds of `layer<>`, no remainder anywhere
    **{f"f{f}": first_filters(f) for f in (1, 2, 17, 40, 100, 128)},
    # residual blocks: three sub-blocks (the branch only behind the last), cin != cout both ways (RIN / ROUT carved at cresp != coutp),
    # one sub-block (first and last at once: the branch reads the sub-block's own input)
    "rep3": stack(mid=((64, 3, 13, 1, 1, True, True),)),
    "res40to100": stack(first=(40, 1, 11, 2, 1, False, True), mid=((100, 2, 13, 1, 1, True, True),)),
    "res100to40": stack(first=(100, 1, 11, 2, 1, False, True), mid=((40, 2, 13, 1, 1, True, True),)),
    "res1": stack(mid=((64, 1, 13, 1, 1, True, True),)),
    # a plain 1x1 block in the middle: no depthwise stage, IN feeds the GEMM at row stride A_LD, no out_alias
    "plain_mid": stack(mid=((48, 1, 1, 1, 1, False, False), (64, 2, 13, 1, 1, True, True))),
    # the last block's width = the decoder's C: `frame_classifier_kernel` at C = 2, 17, 64 (its loop bound; 128 runs everywhere above)
    **{f"last{c}": stack(last=(c, 1, 1, 1, 1, False, False)) for c in (2, 17, 64)},
}


@pytest.mark.parametrize("frames", [65, 37])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_other_layouts(name, frames):
    """Layouts the fused kernels do not take: the generic per-sub-block kernel and the stand-alone classifier, float32, against the float64
    net on the same layout.  The bound's pinned shape is the published layout on the per-sub-block launches."""
    assert LAYOUTS[name] != PUBLISHED
    shape_case("unfused", name, LAYOUTS[name], frames, WIDTH_SEED)


REFUSED = {
    "one past the receptive field (k 70)": (first_k(70), "receptive field"),
    "one past the receptive field (k 8 stride 3)": (first_k(8, stride=3), "receptive field"),
    "129 channels": (first_filters(129), r"\[1, 128\]"),
    "129 channels in a residual block": (stack(mid=((129, 2, 13, 1, 1, True, True),)), r"\[1, 128\]"),
    "a plain conv with k 3": (stack(last=(128, 1, 3, 1, 1, False, False)), "1x1"),
    "a residual block with a stride": (stack(mid=((64, 2, 13, 2, 1, True, True),)), "frame count"),
    "a residual block with an even kernel": (stack(mid=((64, 2, 12, 1, 1, True, True),)), "frame count"),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_layouts_outside_the_kernels_limits_are_refused_before_any_launch(what):
    """The engine refuses by name what vadx_sepconv_block cannot run, and a residual block whose input and output frames differ (the kernel
    would add the wrong frames); no entry point of the library was called on the way."""
    blocks, match = REFUSED[what]
    w = weights.marblenet_synthetic(WIDTH_SEED, blocks)
    with _lib.trace() as tr:
        with pytest.raises(ValueError, match=match):
            marblenet.MarbleNetEngine(w, blocks=blocks)
    assert tr.calls == {}
