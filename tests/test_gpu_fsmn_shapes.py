"""GPU parity: the FSMN-VAD net at every tile size of the window walk and at layer widths other than the checkpoint's.

tests/test_gpu_fsmn.py runs one window length (16 000 samples, T = 101 frames: a 64-frame tile, then a 48-frame one) and one set of widths
(140 / 250 / 140 / 248).  Here the window length sweeps every tile sequence `run_chunk` (csrc/fsmn.hip) can take -- 16, 32, 48, 64 frames,
full and partial, one tile and two, a second tile that keeps most of the old FIR history -- and the widths sweep `qlayer`'s work splits
(csrc/layers_split.h: fewer n-tiles than waves, a full round + leftover tiles, an odd number of 32-k chunks, a width that is no multiple
of 32).  The reference is float64 on the CPU, fed the DEVICE's own log-mel, so that only the net is measured (the front-end is pinned by
tests/test_gpu_frontend.py): LFR edge replication as oracle.fsmn.features, CMVN, oracle.fsmn.encoder with weights and caches in double.
"""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, fsmn, weights
from oracle import fsmn as ofs
from oracle import postproc as opp

pytestmark = pytest.mark.gpu
# the tolerances of tests/test_gpu_fsmn.py: P(silence), the FIR caches, and how close to a threshold a frame must sit for its gate output to differ
ATOL, CACHE_ATOL, NEAR = 1e-4, 5e-4, 2e-4
# float32 torch against the same float64 reference (on the oracle's own log-mel of the inputs below) puts NO frame of any case within NEAR
# of a threshold and reaches 7.0e-6 on P(silence), 2.2e-5 on the caches: no gate output may differ
MAX_EXCUSED = 0
# error / max |reference| per tensor, against the same figure at the pinned shape (L = 16 000, default widths) on the same arithmetic in the
# same session: no width or K here exceeds the default's by more than 3 %, so the summation error has no reason to grow
REL_FACTOR, REL_FLOOR = 2.0, 1e-6
B = 4
BASE_L, BASE_SEED = 16000, 1234
# seeds of the inputs: with these the float64 reference keeps every frame of every case more than 1e-3 (lengths) / 5e-3 (widths) from the
# score threshold and 1.5 from the energy threshold, so that MAX_EXCUSED = 0 asks nothing of chance
LEN_SEED, WIDTH_SEED = 8, 5


@pytest.fixture(autouse=True, params=["f32", "split", "h2"])
def gemm(request):
    """Every test of this file runs on the three arithmetics of the dense layers: float32 MFMAs, bf16 x 3 and fp16 x 2 split products."""
    prev = _lib.gemm_mode(request.param)
    yield request.param
    _lib.gemm_mode(prev)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def make_dims(A, L, A2, O):
    return dict(weights.FSMN_DIMS, input_affine_dim=A, linear_dim=L, output_affine_dim=A2, output_dim=O)


# (A, L, A2, O) -> what to add to out2_b[0]: weights.fsmn_synthetic tunes the silence bias for O = 248; these offsets (found on the CPU, float64
# net on the oracle's features of the inputs below: the mid-range of the silence logit's margin over both window lengths) put P(silence) on
# both sides of the gate for each set.  The tests assert the spread on the reference they compare with.
WIDTHS = {
    (100, 200, 48, 2): -17.5,
    (64, 96, 128, 130): 4.5,
    (16, 16, 16, 5): -10.0,
    (144, 256, 144, 256): 4.0,
}


def width_weights(key):
    w = weights.fsmn_synthetic(7, make_dims(*key))
    w["out2_b"] = w["out2_b"].copy()
    w["out2_b"][0] += np.float32(WIDTHS[key])
    return w


def inputs(L, seed):
    """B burst windows (clip 0 starts in digital silence), random FIR caches 0.3 N(0,1), noise floors, thresholds."""
    rng = np.random.default_rng(seed)
    clips = weights.burst_clips(B, L, seed=L + seed)
    clips[0, :L // 2] = 0
    caches = [(rng.standard_normal((B, 128, 19)) * 0.3).astype(np.float32) for _ in range(4)]
    noise = rng.uniform(1.0, 1.4, B).astype(np.float32)
    thr = np.full(B, 1.0, np.float32)
    return clips, caches, noise, thr


def energy_f64(clips, L, frames):
    """The gate's energy term (oracle.fsmn.forward) in float64: log10 of the 512-sample frame power of the prepped window, last value repeated."""
    a = torch.from_numpy(clips.astype(np.float64))
    a = a - a.mean(dim=-1, keepdim=True)
    y = torch.cat([a[:, :1], a[:, 1:] - 0.97 * a[:, :-1]], dim=-1) * (1.0 / (np.sqrt(float(L)) * 2e-5))
    idx = torch.arange(512).unsqueeze(0) + torch.arange(0, L - 512 + 1, 160).unsqueeze(-1)
    p = torch.log10((y[:, idx] ** 2).sum(-1) + 0.00002)
    return torch.cat((p, p[:, -1:].expand(-1, frames - p.shape[-1])), dim=-1).numpy()


def reference_f64(w, logmel, caches, L):
    """float64 net on a given log-mel [B, T, 80]: (P(silence) [B, T], new caches 4 x [B, 128, 19])."""
    fe = ofs.Frontend(L)
    m = torch.as_tensor(np.asarray(logmel, dtype=np.float64))
    padded = torch.cat((m[:, :1, :].expand(-1, fe.lfr_half, -1), m), dim=1)       # oracle.fsmn.features' LFR edge replication
    lfr = padded[:, fe.idx_mel].reshape(m.shape[0], fe.T_lfr, -1)
    w64 = {k: T(v).double() for k, v in w.items()}
    p, c = ofs.encoder(w64, (lfr + w64["cmvn_means"]) * w64["cmvn_vars"], [T(x).double().unsqueeze(-1) for x in caches])
    return p.numpy(), [x[..., 0].numpy() for x in c]


_REF = {}          # (L, widths key or None, seed) -> (device log-mel, reference), computed once per shape and shared by the three arithmetics
_BASE = {}         # arithmetic -> normalised errors at the pinned shape


def run_case(gemm, w, L, seed, key):
    """One boundary call on the device and its float64 reference -> (errors, normalised errors, reference P(silence)); the assertions that
    hold for every shape are made here."""
    eng = fsmn.FsmnEngine(w, input_audio_length=L)
    clips, caches, noise, thr = inputs(L, seed)
    a = T(clips)
    logmel, _ = eng.features(a.cuda(), 1, L)
    logmel = logmel.cpu().numpy()
    hit = _REF.get((L, key, seed))
    if hit is None or not np.array_equal(hit[0], logmel):
        hit = (logmel, reference_f64(w, logmel, caches, L), energy_f64(clips, L, eng.T))
        _REF[(L, key, seed)] = hit
    _, (rp, rc), rdb = hit
    score, cout, noisy, psil = eng.run(a, [T(c) for c in caches], thr, noise, return_psil=True)
    assert eng.blobs.mode() == gemm and eng.blobs.range_fallbacks == 0
    got_p = psil.cpu().numpy().astype(np.float64)
    got_c = [c.cpu().numpy().astype(np.float64) for c in cout]
    assert got_p.shape == rp.shape == (B, L // 160 + 1)
    assert np.isfinite(got_p).all() and all(np.isfinite(c).all() for c in got_c)
    err = {"psil": float(np.abs(got_p - rp).max())}
    rel = {"psil": err["psil"] / float(np.abs(rp).max())}
    for i in range(4):
        err[f"cache{i}"] = float(np.abs(got_c[i] - rc[i]).max())
        rel[f"cache{i}"] = err[f"cache{i}"] / float(np.abs(rc[i]).max())
    print(f"fsmn shapes {gemm} L={L} widths={key or 'default'}: " + " ".join(f"{k} {err[k]:.2e} (rel {rel[k]:.2e})" for k in err))
    assert err["psil"] <= ATOL, err
    assert max(err[f"cache{i}"] for i in range(4)) <= CACHE_ATOL, err
    # the uint8 score against the float64 gate (oracle.fsmn.forward: score = 2 P(silence) <= thr and energy >= noise floor)
    want = ((rp + rp) <= thr[:, None].astype(np.float64)) & (rdb >= noise[:, None].astype(np.float64))
    got = score.cpu().numpy().astype(bool)
    bad = list(zip(*np.nonzero(got != want)))
    for b, i in bad:
        assert abs(2.0 * rp[b, i] - float(thr[b])) < NEAR or abs(rdb[b, i] - float(noise[b])) < NEAR, (b, i, rp[b, i], rdb[b, i], noise[b])
    assert len(bad) <= MAX_EXCUSED, bad
    if not bad:
        want_noisy = np.array([rdb[b][~want[b]].mean() if (~want[b]).any() else np.nan for b in range(B)])
        np.testing.assert_allclose(noisy.cpu().numpy(), want_noisy, rtol=0, atol=ATOL, equal_nan=True)
    return err, rel, rp


def baseline(gemm):
    if gemm not in _BASE:
        _BASE[gemm] = run_case(gemm, weights.fsmn_synthetic(BASE_SEED), BASE_L, LEN_SEED, None)[1]
    return _BASE[gemm]


def assert_no_worse_than_the_pinned_shape(gemm, rel, what):
    base = baseline(gemm)
    for k, v in rel.items():
        bound = max(REL_FACTOR * base[k], REL_FLOOR)
        print(f"    {k}: rel {v:.2e}, pinned shape {base[k]:.2e}, bound {bound:.2e}")
        assert v <= bound, (what, k, v, base[k])


# L -> T = L // 160 + 1 and the tiles run_chunk walks
LENGTHS = [
    800,        # T =   6: 16-frame tile, nvalid = 6
    2400,       # T =  16: 16-frame tile, full
    2560,       # T =  17: 32-frame tile
    4960,       # T =  32: 32-frame tile, full
    5120,       # T =  33: 48-frame tile
    7520,       # T =  48: 48-frame tile, full
    7680,       # T =  49: 64-frame tile
    10080,      # T =  64: 64-frame tile, full
    10240,      # T =  65: 64 + 16, nvalid = 1 (the new cache is 18 frames of the first tile's + 1)
    12800,      # T =  81: 64 + 32
    17760,      # T = 112: 64 + 48, the limit of the clips / ragged / stream entry points
    20320,      # T = 128: 64 + 64, the limit of the score scratch
]


@pytest.mark.parametrize("L", LENGTHS)
def test_window_length_sweep(gemm, L):
    """Default widths at every tile sequence: P(silence) within 1e-4 and the four output caches within 5e-4 of the float64 net, the uint8
    score equal to the float64 gate, and no tensor's normalised error above twice the pinned shape's."""
    err, rel, rp = run_case(gemm, weights.fsmn_synthetic(BASE_SEED), L, LEN_SEED, None)
    assert_no_worse_than_the_pinned_shape(gemm, rel, L)


@pytest.mark.parametrize("L", [2560, 12800])
@pytest.mark.parametrize("key", list(WIDTHS), ids=lambda k: "-".join(map(str, k)))
def test_width_sweep(gemm, key, L):
    """Other layer widths (A, L, A2, O), one tile and two:
    100/200/48/2     7 n-tiles on 8 waves, 13 = 8 + 5 leftover, an odd number of L-wide 32-k chunks whose last one is half beyond Lp, one-tile head
    64/96/128/130    A2 > A, a 9-tile head (8 + 1 leftover), three L-wide chunks
    16/16/16/5       one n-tile and half a chunk everywhere
    144/256/144/256  the largest accepted
    The silence bias is set per width set so that the reference P(silence) lies on both sides of the gate: a saturated softmax tests nothing."""
    err, rel, rp = run_case(gemm, width_weights(key), L, WIDTH_SEED, key)
    assert rp.min() < 0.2 and rp.max() > 0.8, (float(rp.min()), float(rp.max()))
    assert_no_worse_than_the_pinned_shape(gemm, rel, (key, L))


_CLIPS = {}        # L -> the oracle's (timestamps, flags) per clip


@pytest.mark.parametrize("L", [7680, 17760])
def test_whole_clips_at_other_window_lengths(gemm, L):
    """`detect` and `flags` on another window grid -- L = 7680: T = 49, slide 19, stride 2720, one 64-frame tile per window; L = 17760: T = 112,
    the longest window the clip loop takes -- against oracle.fsmn.run_clip with the same Frontend(L): the `saved` flags and the final
    (start, end) pairs are the oracle's, as tests/test_gpu_fsmn.py::test_whole_clip_flags_and_timestamps asserts at L = 16 000."""
    seed, n, nclips = BASE_SEED, 48000, 2
    w = weights.fsmn_synthetic(seed)
    eng = fsmn.FsmnEngine(w, input_audio_length=L)
    lb, stride = eng.grid()
    assert (lb, stride) == (30, L - 31 * 160) and eng.T - lb == L // 160 - 29
    clips = weights.burst_clips(nclips, n, seed=seed + L)
    noise = np.random.default_rng(9).standard_normal((nclips, 20000))
    got = eng.detect(clips, pad_noise=noise)
    assert eng.blobs.mode() == gemm and eng.blobs.range_fallbacks == 0
    if L not in _CLIPS:
        fe = ofs.Frontend(L)
        ow = {k: T(v) for k, v in w.items()}
        _CLIPS[L] = [ofs.run_clip(fe, ow, opp.normalize_to_int16(clips[b].astype(np.float32)), noise[b]) for b in range(nclips)]
    for b in range(nclips):
        a = opp.normalize_to_int16(clips[b].astype(np.float32))
        want_ts, want_flags = _CLIPS[L][b]
        padded = fsmn.pad_to_window_grid(a, L, stride, noise[b])
        W = (padded.shape[0] - L) // stride + 1
        flags, trace = eng.flags(torch.from_numpy(padded[None]), W, return_noise=True)
        flags = flags.cpu().numpy()[0].astype(bool)
        assert flags.shape[0] == len(want_flags) == W * (eng.T - lb) + lb
        mism = np.flatnonzero(flags != np.array(want_flags, bool))
        assert len(mism) == 0, (b, mism[:10])
        assert got[b] == want_ts
        assert [(int(s * 16000), int(e * 16000)) for s, e in got[b]] == [(int(s * 16000), int(e * 16000)) for s, e in want_ts]
    assert eng.blobs.range_fallbacks == 0


def test_window_longer_than_the_score_scratch_is_refused(gemm):
    """T = 129 frames (20 480 samples) would write P(silence) past the kernel's 128-entry scratch: the engine refuses it by name before
    anything is packed or launched; 20 320 samples (T = 128) is the longest session and runs."""
    w = weights.fsmn_synthetic(BASE_SEED)
    with pytest.raises(ValueError, match="at most 128"):
        fsmn.FsmnSession(w, input_audio_length=20480)
    with pytest.raises(ValueError, match="112"):
        fsmn.FsmnEngine(w, input_audio_length=20480)
    sess = fsmn.FsmnSession(w, input_audio_length=20320)
    assert sess._inputs_meta[0].shape[-1] == 20320 and sess._outputs_meta[0].shape[-1] == 128
    z = np.zeros((1, 128, 19, 1), np.float32)
    res = sess.run(None, {"audio": weights.burst_clips(1, 20320, seed=1).reshape(1, 1, -1), "cache_0": z, "cache_1": z, "cache_2": z, "cache_3": z,
                          "one_minus_speech_threshold": np.array([1.0], np.float32), "noise_average_dB": np.array([4.0], np.float32)})
    assert res[0].dtype == np.uint8 and res[0].shape == (128,) and res[1].shape == (1, 128, 19, 1)
    assert sess.engine.blobs.mode() == gemm and sess.engine.blobs.range_fallbacks == 0
    # the clip loop's own limit is 112 frames: `flags` at T = 128 is refused by the library, not run
    with pytest.raises(ValueError, match="frames=128 unsupported"):
        sess.engine.flags(torch.zeros((1, 20320), dtype=torch.int16), 1)
