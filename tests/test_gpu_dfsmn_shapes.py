"""GPU parity: the DFSMN kernels at every frame-tile edge, chunk count and head width, stage by stage against float64, the head in logit space.

tests/test_gpu_dfsmn.py holds the whole network to 2e-4 x scale on the AEC waveform and 1e-4 on a sigmoid at ONE shape (101 STFT frames, 51
score frames, head 128 / 256 / 4 / 20).  Here every stage is run on its own, through the product's launch code, over the shapes where its
tiling changes:

  a. ICCRN spectrum   `Iccrn.forward(x4, chunks, T, pack)`: quad edges of the time LSTMs' loader wave and T = 1, the packed strides 8 / 24 / 40 /
                      104 / 136 against tile-aligned ones, 1 / 2 / 3 chunks (10 / 20 / 30 work units of the two-layer LSTM: a partial, a full,
                      a partial last workgroup) and 40 chunks; paths f32 / split / h2, each packed and unpacked (equal bit for bit).
  b. ISTFT            `DfsmnEngine.istft` at T = 1 .. 200 (the window_sum_inv table's frame count; 201 is refused before any launch).
  c. mask net         `DfsmnEngine.mask_net` at T = 1 .. 64, around the FIR's 19-frame history, and at hidden / fsmn_hidden / layers / lorder
                      other than 128 / 256 / 4 / 20.
  d. input, features  `vadx_frontend_stft_ft` x 2 + `vadx_dfsmn_alpha_scale` (both forms) and the three `vadx_frontend_logmel_ex` calls at
                      window lengths 160 (T - 1) + 1.

Reference: oracle.dfsmn in float64 -- the reference's own float32 table bits and float32 weights evaluated in double -- chunk by chunk, on the
array the device was fed (asserted equal).  Nothing is compared with the code under test, except where bitwise equality is the claim
(packed vs unpacked, a chunk in a batch vs alone).

The bound is measured, not chosen, and the same for every stage: with e_dev the device's error against float64, e_32 the float32 torch
oracle's error against float64 on the same input, and R = e_dev(pinned) / e_32(pinned) at the stage's pinned shape on the same path in the
same session, every case holds e_dev(case) <= 2 max(e_dev(pinned), R e_32(case)); the factor 2 (FACTOR of the other shape tests) covers
the max-over-few-values noise of both terms.  The project's absolute tolerances stay as a second, unconditional assert: 2e-4 x max(1, scale)
on spectra and waveforms, 1e-4 on probabilities, `assert_features_close`'s 2e-4 (log domain, bands within e^-7 of the frame's peak) and 2e-5
(linear domain relative to that peak, every band) on features.  profiles/dfsmn_shapes_errors.txt keeps one run's table.

Errors.  Spectra, waveforms, x4: max |y - y64| / max |y64| over every value of every chunk.  Head: the device logit is log(p) - log1p(-p) of
the float32 score, in double; e = max |z - z64| / sd over the values whose reference probability lies in (0.02, 0.98), sd the standard
deviation of z64 on the weight set's pinned input.  A random head saturates, so every weight set's linear3 is re-centred, weight and bias,
from its own float64 logits on the pinned input (mean 0, sd 1.5 there), and every case asserts ON THE REFERENCE that at least 90 % of its
probabilities lie in that interval.

Seeds.  ICCRN / ISTFT / input stages: weights.dfsmn_synthetic(1234).  ICCRN input: torch.randn (seed 1234 + 1000 chunks + T) x 0.5, the first
third of chunk 0's frames x 0.01, the last chunk all zeros (digital silence on both streams: the LayerNorms see bias-driven tensors); the
one-chunk cases keep their chunk.  The 40-chunk case repeats the three chunks of the 3-chunk case of the same T, whose references it shares.
ISTFT: torch.randn (seed 77 + T).  Head: the default head is seed 1234, the other widths seed 7; features -34 + 3 N(window) + 2 N(window,
frame) + 1.5 N(window, frame, band) from numpy's default_rng(1234 + T), 8 windows (64 where T <= 4); pinned input 8 windows at T = 51 from
default_rng(1234).  Input stage: weights.burst_clips(3, L, seed 1234 + T) / (seed 4321 + T), the first half of clip 0 digital silence.

The input stage also holds two parts of x4 on their own, each relative to the part's own maximum: the two far channels alpha_scale
multiplies, and their frames 0 .. 8, whose history taps reach before the chunk's first frame (in the two-stream form 1 / 500 of the tensor's
maximum: an error there does not show in the tensor's figure).  They are held to the stage's bound, not to a ratio of their own: 8640 values
whose pinned error is below one float32 ulp (near-only form: 8.9e-8 < 2^-23) are no yardstick -- against such a ratio the near-only T = 16
case read 2.26e-7 (1.9 ulp; float32 oracle 9.2e-8) for a bound of 1.79e-7, from a kernel that sums the same ten float32 taps in another order.

Measured on one MI355X (profiles/dfsmn_shapes_errors.txt has every case), pinned shapes: e_dev, e_32, R
  iccrn (3 chunks, T = 101, packed = unpacked)   f32 1.89e-06 1.97e-06 0.959   split 2.00e-06 1.97e-06 1.015   h2 2.60e-06 1.97e-06 1.322
  istft (3 chunks, T = 101)                      5.27e-07 5.27e-07 1.000
  head (default head, 8 windows, T = 51)         3.77e-06 2.59e-06 1.459
  alpha (3 windows, T = 101)                     two-stream 8.98e-07 4.71e-07 1.905   near-only 2.71e-07 1.76e-07 1.539
  features (3 windows, T = 101, T_A = 51)        log 2.12e-06 1.74e-06 1.218   lin 1.15e-06 6.79e-07 1.688
Largest e / bound: iccrn 0.776 (f32, T = 5) / 0.885 (split, T = 104) / 0.691 (h2, T = 104), istft 0.621 (T = 32), head 0.496 (lorder 1,
T = 64), alpha 0.633 (two-stream, T = 17), features 0.580 (T = 33).  Lowest share of a head reference inside (0.02, 0.98): 96.3 % (hidden = 1,
T = 51); no case needed another feature seed.  The sweep found no kernel bug: every case of every path passed on the library as it was.
That it notices one was checked once on a library with three one-line changes: the ISTFT's overlap-add one sample short per frame edge (all
20 ISTFT cases failed), alpha_scale's history tap at frame 0 skipped (12 of 14 input cases; the two others start on a quiet stretch), the
head's FIR window one frame early at frame 63 (all 12 cases with a FIR at T = 64).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, dfsmn, frontend, weights
from oracle import dfsmn as od

pytestmark = pytest.mark.gpu
FACTOR = 2.0
SCALE_TOL = 2e-4               # spectra and waveforms, x max(1, scale): tests/test_gpu_dfsmn.py
PROB_ATOL = 1e-4               # probabilities: tests/test_gpu_dfsmn.py
FEAT_ATOL, FEAT_LIN = 2e-4, 2e-5          # features: assert_features_close of tests/test_gpu_frontend.py
INSIDE, LO, HI = 0.9, 0.02, 0.98
SEED, WIDTH_SEED = 1234, 7
PIN_T, PIN_CHUNKS, PIN_TA = 101, 3, 51
PATHS = ["f32", "split", "h2"]


def T_(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@contextlib.contextmanager
def arithmetic(path):
    """The arithmetic of the kernels that have more than one, set for the block and restored"""
    prev = _lib.gemm_mode(path)
    try:
        yield
    finally:
        _lib.gemm_mode(prev)


def rel_error(y, y64):
    """(max |y - y64| / max |y64|, max |y64|)"""
    scale = float(np.abs(y64).max())
    return float(np.abs(y.astype(np.float64) - y64).max()) / scale, scale


# ---- the measured bound, shared by the stages ------------------------------------------------------------------------------------------
_PIN = {}          # (stage, path) -> {metric: (e_dev, R)} of the stage's pinned shape, measured once per session
_PINNED_RUN = {}   # stage -> function(path) -> {metric: (e_dev, e_32)}


def pinned(stage, path):
    if (stage, path) not in _PIN:
        figs = _PINNED_RUN[stage](path)
        _PIN[(stage, path)] = {m: (e, e / e32) for m, (e, e32) in figs.items()}
        for m, (e, e32) in figs.items():
            print(f"dfsmn shapes pinned {stage} {path} {m}: e {e:.2e} e32 {e32:.2e} R {e / e32:.3f}")
    return _PIN[(stage, path)]


def assert_float32_grade(stage, path, figs, what, parts=None):
    """figs {metric: (e_dev, e_32)} of one case against the bound measured at the stage's pinned shape.  parts {name: e_dev}: errors of parts of
    the tensor, each relative to the part's own maximum, held to the bound of the metric "all"."""
    for m, (e, e32) in figs.items():
        e_pin, ratio = pinned(stage, path)[m]
        bound = FACTOR * max(e_pin, ratio * e32)
        print(f"    {m}: e {e:.2e} bound {bound:.2e} ratio {e / bound:.3f} (pinned {e_pin:.2e}, R {ratio:.3f}, e32 {e32:.2e})")
        assert e <= bound, (stage, path, m, what, e, bound, e_pin, ratio, e32)
        for name, ep in (parts or {}).items() if m == "all" else ():
            print(f"    {name}: e {ep:.2e} bound {bound:.2e} ratio {ep / bound:.3f}")
            assert ep <= bound, (stage, path, name, what, ep, bound)


# ---- shared, built once ----------------------------------------------------------------------------------------------------------------
_W = {}            # "np" -> the seed-1234 weights, torch.float32 / torch.float64 -> the oracle's copies
_TABLES = {}       # dtype -> od.Frontend(200, dtype) (its .tb are the ICCRN's tables)
_ENG = {}          # weight set name -> DfsmnEngine


def base_weights(dtype=None):
    if "np" not in _W:
        _W["np"] = weights.dfsmn_synthetic(SEED)
    if dtype is None:
        return _W["np"]
    if dtype not in _W:
        _W[dtype] = {k: T_(v).to(dtype) for k, v in _W["np"].items()}
    return _W[dtype]


def iccrn_weights(dtype):
    key = ("iccrn", dtype)
    if key not in _W:
        _W[key] = {k[len("iccrn."):]: v for k, v in base_weights(dtype).items() if k.startswith("iccrn.")}
    return _W[key]


def tables(dtype):
    if dtype not in _TABLES:
        _TABLES[dtype] = od.Frontend(dfsmn.ISTFT_MAX_FRAMES, dtype)
    return _TABLES[dtype]


def engine(name="default", w=None):
    if name not in _ENG:
        _ENG[name] = dfsmn.DfsmnEngine(base_weights() if w is None else w)
    return _ENG[name]


def range_flag(net):
    words = net.range_flag.cpu().numpy()
    return int(words[0]), float(words[1:].view(np.float32)[0])


# ======================================================================================================================================
# a. ICCRN spectrum
# ======================================================================================================================================
_SPEC = {}         # (frames, chunks) -> the input and both oracles' spectra on it


def iccrn_input(frames, chunks):
    g = torch.Generator().manual_seed(SEED + 1000 * chunks + frames)
    x = torch.randn(chunks, 4, od.F_BINS, frames, generator=g) * 0.5
    x[0, :, :, :frames // 3] *= 0.01
    if chunks > 1:
        x[-1] = 0.0
    return x.numpy()


def oracle_spectrum(x, dtype):
    """[chunks, 4, 160, T] float32 -> the oracle's spectrum in `dtype`, chunk by chunk, as float64 numpy [chunks, 2, 160, T]"""
    w, tb = iccrn_weights(dtype), tables(dtype).tb
    with torch.no_grad():
        return torch.cat([od.iccrn_spectrum(T_(x[k:k + 1]).to(dtype), w, tb) for k in range(x.shape[0])], 0).double().numpy()


def spectrum_reference(frames, chunks):
    key = (frames, chunks)
    if key not in _SPEC:
        x = iccrn_input(frames, chunks)
        y64 = oracle_spectrum(x, torch.float64)
        assert np.isfinite(y64).all()
        _SPEC[key] = dict(x=x, y64=y64, e32=rel_error(oracle_spectrum(x, torch.float32), y64)[0])
    return _SPEC[key]


def spectrum_case(path, frames, chunks):
    """One ICCRN pass of `chunks` windows of `frames` frames on `path`, packed and unpacked -> {metric: (e_dev, e_32)}"""
    net = engine().iccrn
    if chunks <= 3:
        ref = spectrum_reference(frames, chunks)
        x, y64 = ref["x"], ref["y64"]
    else:                                          # the 3-chunk case's chunks, repeated: its references serve
        ref = spectrum_reference(frames, 3)
        pick = np.arange(chunks) % 3
        x, y64 = ref["x"][pick], ref["y64"][pick]
    x4 = dfsmn.to_ft(torch, T_(x), net.device)
    assert np.array_equal(dfsmn.from_ft(x4, chunks).cpu().numpy(), x)                  # the reference saw what the net is fed
    with arithmetic(path):
        assert net.arithmetic is None and net.lstm_t_h2
        out = {pack: dfsmn.from_ft(net.forward(x4, chunks, frames, pack=pack), chunks).cpu().numpy() for pack in (True, False)}
        flag = range_flag(net)
    assert flag == (0, 0.0), (path, flag)                                                # in-range operands never raise the fp16 x 2 flag
    assert out[True].dtype == np.float32 and out[True].shape == y64.shape and np.isfinite(out[False]).all()
    assert np.array_equal(out[True], out[False])                                         # packed frame layout: bit for bit the unpacked one
    figs = {}
    for pack in (True, False):
        e, scale = rel_error(out[pack], y64)
        print(f"dfsmn shapes iccrn {path} {'packed' if pack else 'unpacked'} T={frames} chunks={chunks} stride={dfsmn.packed_stride(frames)}: "
              f"e {e:.2e} e32 {ref['e32']:.2e} scale {scale:.2f}")
        assert e * scale <= SCALE_TOL * max(1.0, scale), (path, pack, frames, chunks, e, scale)
        figs["packed" if pack else "unpacked"] = (e, ref["e32"])
    return figs


_PINNED_RUN["iccrn"] = lambda path: spectrum_case(path, PIN_T, PIN_CHUNKS)

# T: quad edges of the loader wave (1 .. 5, 7 .. 9), T = 1 = the single step of layer 1, tile edges (15 .. 17, 31 .. 33, 48 / 49), the packed
# strides 8 (T <= 8) / 24 (17, 24) / 40 (33, 40) / 104 (101, 104) / 136 (129) against tile-aligned ones (9 .. 16, 25 .. 32, 41 .. 48, 105)
ICCRN_FRAMES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 101, 104, 105, 129]


@pytest.mark.parametrize("frames", ICCRN_FRAMES)
@pytest.mark.parametrize("path", PATHS)
def test_iccrn_frame_count_sweep(path, frames):
    """Three chunks (30 work units of the two-layer time LSTM: the last workgroup has two dead slots; with an odd chunk count the last packed
    tile is half empty) at every frame count above, the last chunk digital silence."""
    assert_float32_grade("iccrn", path, spectrum_case(path, frames, 3), (frames, 3))


@pytest.mark.parametrize("chunks", [1, 2, 3, 40])
@pytest.mark.parametrize("frames", [17, 101])
@pytest.mark.parametrize("path", PATHS)
def test_iccrn_chunk_count_sweep(path, frames, chunks):
    """1 / 2 / 3 chunks = 10 / 20 / 30 units of the two-layer LSTM (NTILE = 4 per workgroup: partial, exact, partial); 40 chunks at packed
    strides 24 / 104: every second chunk starts mid-tile."""
    assert_float32_grade("iccrn", path, spectrum_case(path, frames, chunks), (frames, chunks))


# ======================================================================================================================================
# b. ISTFT
# ======================================================================================================================================
def istft_case(path, frames, chunks):
    eng = engine()
    g = torch.Generator().manual_seed(77 + frames)
    spec = torch.randn(chunks, 2, od.F_BINS, frames, generator=g)
    with torch.no_grad():
        ref = {dt: torch.cat([od.istft(spec[k:k + 1].to(dt), tables(dt).tb)[0] for k in range(chunks)], 0)[:, 0].double().numpy()
               for dt in (torch.float64, torch.float32)}
    y_ft = dfsmn.to_ft(torch, spec, eng.device)
    assert torch.equal(dfsmn.from_ft(y_ft, chunks).cpu(), spec)
    out = eng.istft(y_ft.data, chunks, frames).cpu().numpy()
    assert out.dtype == np.float32 and out.shape == ref[torch.float64].shape == (chunks, (frames - 1) * 160 + 1)
    assert np.isfinite(out).all()
    (e, scale), e32 = rel_error(out, ref[torch.float64]), rel_error(ref[torch.float32], ref[torch.float64])[0]
    print(f"dfsmn shapes istft T={frames} chunks={chunks}: e {e:.2e} e32 {e32:.2e} scale {scale:.3f}")
    assert e * scale <= SCALE_TOL * max(1.0, scale), (frames, chunks, e, scale)
    return {"wave": (e, e32)}


_PINNED_RUN["istft"] = lambda path: istft_case(path, PIN_T, PIN_CHUNKS)


@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("frames", [1, 2, 15, 16, 17, 32, 33, 101, 129, 200])
def test_istft_frame_count_sweep(frames, chunks):
    """`t < T` per 16-frame tile of the GEMM, the overlap-add's first and last frame, a one-sample output at T = 1, the last entry of the
    window_sum_inv table at T = 200."""
    assert_float32_grade("istft", "f32", istft_case("f32", frames, chunks), (frames, chunks))


def test_istft_refuses_more_frames_than_its_table_covers():
    eng = engine()
    frames = dfsmn.ISTFT_MAX_FRAMES + 1
    y_ft = dfsmn.FT(torch, eng.device, 1, frames, 2, od.F_BINS)
    with _lib.trace() as tr:
        with pytest.raises(ValueError, match="window_sum_inv"):
            eng.istft(y_ft.data, 1, frames)
    assert tr.calls == {}


# ======================================================================================================================================
# c. mask net, in logit space
# ======================================================================================================================================
_HEADS = {}        # weight set name -> dict(w, sd, eng)
_HEAD_REF = {}     # (weight set name, frames) -> features and both oracles on them


def head_features(frames, seed=None, n=None):
    rng = np.random.default_rng(SEED + frames if seed is None else seed)
    n = (64 if frames <= 4 else 8) if n is None else n
    f = -34.0 + 3.0 * rng.standard_normal((n, 1, 1)) + 2.0 * rng.standard_normal((n, frames, 1)) + 1.5 * rng.standard_normal((n, frames, 240))
    return f.astype(np.float32)


def head_logits(w, feat, dtype):
    """oracle.dfsmn.mask_head in `dtype` on features [n, T, 240], window by window -> (logits, sigmoid of them), float64 numpy [n, T]"""
    wt = {k: T_(v).to(dtype) for k, v in w.items() if k.startswith("mask.")}
    wt["mask.shift"] = T_(w["mask.shift"] + np.float32(np.log(np.float32(32768.0 ** 2)))).to(dtype)      # float32, as the engine loads it
    with torch.no_grad():
        z = torch.cat([od.mask_head(T_(feat[k:k + 1]).to(dtype), wt) for k in range(feat.shape[0])], 0)[..., 0]
        return z.double().numpy(), torch.sigmoid(z).double().numpy()


def p_logit(p):
    with np.errstate(divide="ignore"):
        p = np.asarray(p, dtype=np.float64)
        return np.log(p) - np.log1p(-p)


def head_set(name, seed=SEED, mask=None):
    """The weight set `name`: dfsmn_synthetic(seed, mask) with linear3 re-centred on its own float64 logits on the pinned input"""
    if name not in _HEADS:
        w = dict(weights.dfsmn_synthetic(seed, mask=mask))
        pin = head_features(PIN_TA, seed=SEED, n=8)
        z = head_logits(w, pin, torch.float64)[0]
        s, mu = 1.5 / z.std(), z.mean()
        w3, b3 = w["mask.linear3.weight"].astype(np.float64), w["mask.linear3.bias"].astype(np.float64)
        w["mask.linear3.weight"], w["mask.linear3.bias"] = (s * w3).astype(np.float32), (s * b3 - s * mu).astype(np.float32)
        _HEADS[name] = dict(w=w, sd=float(head_logits(w, pin, torch.float64)[0].std()), eng=engine("head " + name, w))
    return _HEADS[name]


def logit_error(z, z64, p64, sd):
    m = (p64 > LO) & (p64 < HI)
    return float(np.abs(z[m] - z64[m]).max() / sd)


def head_case(name, frames, pinned_input=False, **set_args):
    hs = head_set(name, **set_args)
    key = (name, frames, pinned_input)
    if key not in _HEAD_REF:
        feat = head_features(frames, seed=SEED, n=8) if pinned_input else head_features(frames)
        z64, p64 = head_logits(hs["w"], feat, torch.float64)
        p32 = head_logits(hs["w"], feat, torch.float32)[1].astype(np.float32)          # the float32 oracle's SCORES, as the device's are read
        inside = float(((p64 > LO) & (p64 < HI)).mean())
        _HEAD_REF[key] = dict(feat=feat, z=z64, p=p64, inside=inside, e32=logit_error(p_logit(p32), z64, p64, hs["sd"]) if inside else None)
    ref = _HEAD_REF[key]
    assert ref["inside"] >= INSIDE, (key, ref["inside"])                                 # a saturated sigmoid tests nothing
    eng, n = hs["eng"], ref["feat"].shape[0]
    x = T_(ref["feat"]).to(eng.device)
    p = eng.mask_net(x, n, frames)
    alone = eng.mask_net(x[n - 1:].contiguous(), 1, frames)
    assert np.array_equal(x.cpu().numpy(), ref["feat"])
    assert torch.equal(p[n - 1:], alone)                                                 # a chunk of a batch = the same chunk alone, bit for bit
    p = p.cpu().numpy()
    assert p.dtype == np.float32 and p.shape == ref["p"].shape == (n, frames) and np.isfinite(p).all()
    dp, e = float(np.abs(p.astype(np.float64) - ref["p"]).max()), logit_error(p_logit(p), ref["z"], ref["p"], hs["sd"])
    print(f"dfsmn shapes head {name} T={frames} windows={n}: p {dp:.2e} e {e:.2e} e32 {ref['e32']:.2e} inside {ref['inside']:.3f}")
    assert np.isfinite(e) and dp <= PROB_ATOL, (name, frames, dp, e)
    return {"logit": (e, ref["e32"])}


_PINNED_RUN["head"] = lambda path: head_case("default", PIN_TA, pinned_input=True)


# 19 / 20 / 21 straddle the FIR's full history (lorder - 1 = 19 frames); 64 is the kernel's limit; 15 .. 17, 31 .. 33, 48 / 49: 16-frame tiles
@pytest.mark.parametrize("frames", [1, 2, 15, 16, 17, 19, 20, 21, 31, 32, 33, 48, 49, 51, 63, 64])
def test_head_frame_count_sweep(frames):
    assert_float32_grade("head", "f32", head_case("default", frames), frames)


HEAD_DIMS = {
    # hidden: one live row in a tile, a second tile for one row, seven tiles
    **{f"hidden{h}": dict(hidden=h) for h in (1, 17, 100)},
    **{f"fsmn_hidden{h}": dict(fsmn_hidden=h) for h in (1, 17, 250)},
    **{f"layers{n}": dict(layers=n) for n in (0, 1, 8)},
    # lorder 1: no taps to loop over
    **{f"lorder{n}": dict(lorder=n) for n in (1, 2, 19)},
}


@pytest.mark.parametrize("frames", [51, 17, 64])
@pytest.mark.parametrize("name", list(HEAD_DIMS))
def test_head_other_dimensions(name, frames):
    """Head dimensions other than 128 / 256 / 4 / 20, rows padded to 16; the bound's pinned shape is the default head."""
    assert_float32_grade("head", "f32", head_case(name, frames, seed=WIDTH_SEED, mask=dict(weights.DFSMN_MASK, **HEAD_DIMS[name])), (name, frames))


@pytest.mark.parametrize("what,mask,match", [("hidden 129", dict(hidden=129), "hidden"), ("fsmn_hidden 257", dict(fsmn_hidden=257), "fsmn_hidden"),
                                             ("layers 9", dict(layers=9), "layers"), ("lorder 21", dict(lorder=21), "lorder")])
def test_head_dimensions_outside_the_kernels_limits_are_refused_before_any_launch(what, mask, match):
    w = weights.dfsmn_synthetic(WIDTH_SEED, mask=dict(weights.DFSMN_MASK, **mask))
    with _lib.trace() as tr:
        with pytest.raises(ValueError, match=match + " = "):
            dfsmn.DfsmnEngine(w)
    assert tr.calls == {}


# ======================================================================================================================================
# d. input and feature stages
# ======================================================================================================================================
_FE = {}           # (preset key, L) -> frontend.Frontend
_INPUT = {}        # (T, near_only) -> everything the two tests of one case share


def fe_for(key, L):
    if (key, L) not in _FE:
        _FE[(key, L)] = frontend.Frontend(dfsmn.STFT_B_PRESET if key == "b" else dfsmn.STFT_A_PRESETS[key], L)
    return _FE[(key, L)]


def near_only_constants():
    if "no" not in _W:
        _W["no"] = weights.dfsmn_near_only_constants(SEED)
    return _W["no"]


def input_stage(frames, near_only):
    """STFT-B of both streams into an FT tensor + alpha_scale, on the device and in both oracles, for 3 windows of 160 (frames - 1) + 1 samples"""
    key = (frames, near_only)
    if key in _INPUT:
        return _INPUT[key]
    eng, n, L = engine(), 3, 160 * (frames - 1) + 1
    near, far = weights.burst_clips(n, L, seed=SEED + frames), weights.burst_clips(n, L, seed=4321 + frames)
    near[0, :L // 2] = 0
    far[0, :L // 2] = 0
    consts = near_only_constants() if near_only else None
    ref = {}
    for dt in (torch.float64, torch.float32):
        fe, w = tables(dt), base_weights(dt)
        no = None if consts is None else tuple(T_(c).to(dt) for c in consts)
        with torch.no_grad():
            rows = [od.scaled_input(fe, w, T_(near[k]).reshape(1, 1, -1), None if near_only else T_(far[k]).reshape(1, 1, -1), no) for k in range(n)]
        ref[dt] = dict(near=[r[0] for r in rows], x4=torch.cat([r[1] for r in rows], 0).double().numpy())
    t, lib, st = torch, _lib.lib(), _lib.stream_ptr()
    feb, nt = fe_for("b", L), dfsmn.ft_tiles(frames)
    assert feb.frames == frames
    xraw, x4 = dfsmn.FT(t, eng.device, n, frames, 4, od.F_BINS), dfsmn.FT(t, eng.device, n, frames, 4, od.F_BINS)
    d_near, d_far = T_(near).to(eng.device), T_(far).to(eng.device)
    mean_near, mean_far = (t.empty((n,), dtype=t.float32, device=eng.device) for _ in range(2))
    for src, means, coff in ((d_near, mean_near, 0), (None if near_only else d_far, mean_far, 2)):
        if src is None:
            far_ft = dfsmn.to_ft(t, T_(consts[1][:, :, :frames]).unsqueeze(0), eng.device).data                # [nt, 2, 160, 16]
            xraw.data.view(n, nt, 4, od.F_BINS, 16)[:, :, 2:4] = far_ft.unsqueeze(0)
            continue
        _lib.check(lib.vadx_frontend_stft_ft(C.byref(feb.cfg), feb.packed.data_ptr(), src.data_ptr(), _lib.row_stride(src), L, n, 1,
                                             means.data_ptr(), xraw.data.data_ptr(), 4, coff, st))
    pow_far = T_(consts[0][:, :frames, :]).to(eng.device).contiguous() if near_only else None
    _lib.check(lib.vadx_dfsmn_alpha_scale(xraw.data.data_ptr(), x4.data.data_ptr(), n, nt, *[a.data_ptr() for a in eng.alpha],
                                          None if pow_far is None else pow_far.data_ptr(), frames, st))
    assert np.array_equal(d_near.cpu().numpy(), near) and np.array_equal(d_far.cpu().numpy(), far)
    _INPUT[key] = dict(n=n, L=L, near=near, d_near=d_near, mean_near=mean_near, x4=x4, ref=ref)
    return _INPUT[key]


def alpha_case(path, frames, near_only):
    c = input_stage(frames, near_only)
    got, y64, y32 = dfsmn.from_ft(c["x4"], c["n"]).cpu().numpy(), c["ref"][torch.float64]["x4"], c["ref"][torch.float32]["x4"]
    assert got.shape == y64.shape == (c["n"], 4, od.F_BINS, frames) and np.isfinite(got).all()
    figs, parts = {}, {}
    # all: every value, the stage's error.  far: the two channels alpha_scale multiplies; head: their first nine frames, the taps with zero
    # history -- in the two-stream form 1 / 500 of the tensor's maximum, so an error there does not show in "all": each part's error is
    # taken relative to the part's own maximum and held to the stage's bound (the same ten taps and one product make every frame)
    for m, sel in (("all", np.s_[:]), ("far", np.s_[:, 2:]), ("head", np.s_[:, 2:, :, :9])):
        scale = float(np.abs(y64[sel]).max())
        e, e32 = float(np.abs(got[sel] - y64[sel]).max()) / scale, float(np.abs(y32[sel] - y64[sel]).max()) / scale
        print(f"dfsmn shapes alpha {'near-only' if near_only else 'two-stream'} T={frames} {m}: e {e:.2e} e32 {e32:.2e} scale {scale:.3f}")
        assert e * scale <= SCALE_TOL * max(1.0, scale), (frames, near_only, m, e, scale)
        if m == "all":
            figs[m] = (e, e32)
        else:
            parts[m] = e
    return figs, parts


_PINNED_RUN["alpha"] = lambda path: alpha_case(path, PIN_T, False)[0]
_PINNED_RUN["alpha near-only"] = lambda path: alpha_case(path, PIN_T, True)[0]
# 5: the shortest window whose AEC waveform (641 samples) exceeds STFT-A's 512-sample centre pad; 9 / 10: the last frame with a zero-history
# tap and the first without; 16 / 17 / 33: tile edges
INPUT_FRAMES = [5, 9, 10, 16, 17, 33, 101]


@pytest.mark.parametrize("near_only", [False, True])
@pytest.mark.parametrize("frames", INPUT_FRAMES)
def test_stft_b_and_alpha_scale(frames, near_only):
    """x4 = [mix re, mix im, |alpha| far re, |alpha| far im] from two int16 streams (or one and the near-end-only model's constants) against
    oracle.dfsmn.scaled_input in float64; the frames whose ten history taps reach before the chunk's first frame are held on their own."""
    stage = "alpha near-only" if near_only else "alpha"
    figs, parts = alpha_case("f32", frames, near_only)
    assert_float32_grade(stage, "f32", figs, (frames, near_only), parts)


def features_case(path, frames):
    """The three vadx_frontend_logmel_ex calls on the DEVICE's own AEC waveform of the two-stream input stage, against float64 features of
    that same waveform"""
    c = input_stage(frames, False)
    eng, n, L, t = engine(), c["n"], c["L"], torch
    with arithmetic("f32"):
        aec = eng.istft(eng.iccrn.forward(c["x4"], n, frames).data, n, frames)
    frames_a = L // od.HOP_A + 1
    feat = t.empty((n, frames_a, 240), dtype=t.float32, device=eng.device)
    near = c["d_near"]
    for prep, off in ((3, 0), (4, 80), (5, 160)):
        fe = fe_for(prep, L)
        assert fe.frames == frames_a
        _lib.check(_lib.lib().vadx_frontend_logmel_ex(C.byref(fe.cfg), fe.packed.data_ptr(), fe.mel_kb.ctypes.data,
                                                      None if prep == 4 else near.data_ptr(), _lib.row_stride(near), L, n, 1,
                                                      None if prep == 4 else c["mean_near"].data_ptr(),
                                                      None if prep == 3 else aec.data_ptr(), 240, off, feat.data_ptr(), _lib.stream_ptr()))
    got, wave = feat.cpu().numpy().astype(np.float64), aec.cpu()
    assert wave.shape == (n, L) and np.isfinite(got).all()
    ref = {}
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            ref[dt] = torch.cat([od.features(tables(dt), c["ref"][dt]["near"][k], wave[k].reshape(1, 1, -1).to(dt)) for k in range(n)], 0).double().numpy()
    assert ref[torch.float64].shape == got.shape
    per_stream = lambda a: a.reshape(n, frames_a, 3, 80)      # noqa: E731
    want = per_stream(ref[torch.float64])
    peak = want.max(axis=-1, keepdims=True)
    big = want > peak - 7.0
    figs = {}
    for m, err in (("log", lambda a: np.abs(per_stream(a) - want)[big].max()), ("lin", lambda a: np.abs(np.exp(per_stream(a) - peak) - np.exp(want - peak)).max())):
        figs[m] = (float(err(got)), float(err(ref[torch.float32])))
    print(f"dfsmn shapes features T={frames} T_A={frames_a}: log {figs['log'][0]:.2e} (e32 {figs['log'][1]:.2e}) lin {figs['lin'][0]:.2e} (e32 {figs['lin'][1]:.2e})")
    assert figs["log"][0] < FEAT_ATOL and figs["lin"][0] < FEAT_LIN, (frames, figs)
    return figs


_PINNED_RUN["features"] = lambda path: features_case(path, PIN_T)


@pytest.mark.parametrize("frames", INPUT_FRAMES)
def test_feature_streams(frames):
    """Preps 3 / 4 / 5 (near, AEC, echo) at windows of 641 .. 16001 samples: the log-domain error within e^-7 of the frame's strongest band
    and the linear-domain error of every band relative to that peak."""
    assert_float32_grade("features", "f32", features_case("f32", frames), frames)
