"""GPU: FSMN-VAD windows of any length behind `long_windows=True` (vadx_fsmn_window_stats_long, vadx_fsmn_run_long, vadx_fsmn_clips_long).

An export of FSMN/Export_FSMN_VAD.py with a long INPUT_AUDIO_LENGTH scores a whole clip as one window; the default entry points keep a
window's scores in LDS and stop at 128 / 112 frames.  The long path keeps them in a global workspace.  Checked here, on the three
arithmetics: bit for bit the default engine where both run (a long engine uses the long entry points at EVERY length); the float64 net on
the device's own log-mel beyond 128 frames, in the style and with the bounds of tests/test_gpu_fsmn_shapes.py (helpers restated); the
long stats kernels against the two-kernel fallback; whole clips against oracle.fsmn.run_clip; ragged batches; refusals; the session."""
import ctypes as C

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, fsmn, weights
from oracle import fsmn as ofs
from oracle import postproc as opp

pytestmark = pytest.mark.gpu
# the bounds of tests/test_gpu_fsmn_shapes.py: P(silence), the FIR caches, how close to a threshold a frame must sit for its gate output to
# differ, no excused frame, and no tensor's normalised error above twice the pinned shape's (L = 16 000, default widths, same arithmetic)
ATOL, CACHE_ATOL, NEAR = 1e-4, 5e-4, 2e-4
MAX_EXCUSED = 0
REL_FACTOR, REL_FLOOR = 2.0, 1e-6
BASE_L, BASE_SEED, BASE_INPUT_SEED = 16000, 1234, 8
# Seeds of the inputs, chosen on the CPU (float32 oracle and float64 net on the oracle's own log-mel of `inputs`): with them the float32
# oracle's gate equals the float64 gate on EVERY frame, and the float64 reference keeps every frame at least 2.1 from the energy threshold
# and, from the score threshold, more than 1e-3 up to T = 257 (5e-3 at the other widths), 5.3e-4 at T = 1 001 and 3.9e-4 at T = 12 001
# (the more frames, the closer the closest).  The device's P(silence) is held to ATOL, i.e. its score to 2e-4 = NEAR, so no frame's gate
# output can differ while that bound holds: MAX_EXCUSED = 0 asks nothing of chance.
#   L -> (T, tiles, input seed)
LENGTHS = {
    20480: (129, "64 + 64 + a 16-frame tile with one valid frame", 9),
    25600: (161, "64 + 64 + 48", 10),
    30720: (193, "3 x 64 + 16 (1 valid)", 10),
    40960: (257, "4 x 64 + 16 (1 valid)", 8),
    160000: (1001, "15 x 64 + 48: the 10 s clip as one window", 10),
}
LONGEST, LONGEST_SEED = 1920000, 14         # T = 12 001, B = 1: two minutes as one window
WIDTH_L, WIDTH_SEED = 25600, 5


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


# (A, L, A2, O) -> what to add to out2_b[0], as tests/test_gpu_fsmn_shapes.py::WIDTHS: the smallest and the largest accepted widths
WIDTHS = {
    (16, 16, 16, 5): -10.0,
    (144, 256, 144, 256): 4.0,
}


def width_weights(key):
    w = weights.fsmn_synthetic(7, make_dims(*key))
    w["out2_b"] = w["out2_b"].copy()
    w["out2_b"][0] += np.float32(WIDTHS[key])
    return w


def inputs(L, seed, B=4):
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
    p = torch.log10((y.unfold(-1, 512, 160) ** 2).sum(-1) + 0.00002)
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
_ENG = {}          # (weights key, L, long) -> engine: its blobs are per arithmetic


def engine(L, long, key=None):
    if (key, L, long) not in _ENG:
        w = weights.fsmn_synthetic(BASE_SEED) if key is None else width_weights(key)
        _ENG[key, L, long] = (fsmn.FsmnEngine(w, input_audio_length=L, long_windows=long), w)
    return _ENG[key, L, long]


def run_case(gemm, L, seed, key, B=4):
    """One boundary call of a LONG engine and its float64 reference -> (errors, normalised errors, reference P(silence)); the
    assertions that hold for every shape are made here (tests/test_gpu_fsmn_shapes.py::run_case, on the long entry points)."""
    eng, w = engine(L, True, key)
    clips, caches, noise, thr = inputs(L, seed, B)
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
    print(f"fsmn long {gemm} L={L} widths={key or 'default'}: " + " ".join(f"{k} {err[k]:.2e} (rel {rel[k]:.2e})" for k in err))
    assert err["psil"] <= ATOL, err
    assert max(err[f"cache{i}"] for i in range(4)) <= CACHE_ATOL, err
    # the uint8 score against the float64 gate (oracle.fsmn.forward: score = 2 P(silence) <= thr and energy >= noise floor); the energies
    # of the long stats kernel are checked through it, against energy_f64
    want = ((rp + rp) <= thr[:, None].astype(np.float64)) & (rdb >= noise[:, None].astype(np.float64))
    got = score.cpu().numpy().astype(bool)
    bad = list(zip(*np.nonzero(got != want)))
    for b, i in bad:
        assert abs(2.0 * rp[b, i] - float(thr[b])) < NEAR or abs(rdb[b, i] - float(noise[b])) < NEAR, (b, i, rp[b, i], rdb[b, i], noise[b])
    assert len(bad) <= MAX_EXCUSED, bad
    assert want.any() and not want.all()                                   # both gate outputs occur
    want_noisy = np.array([rdb[b][~want[b]].mean() if (~want[b]).any() else np.nan for b in range(B)])
    np.testing.assert_allclose(noisy.cpu().numpy(), want_noisy, rtol=0, atol=ATOL, equal_nan=True)
    return err, rel, rp


def assert_no_worse_than_the_pinned_shape(gemm, rel, what):
    if gemm not in _BASE:
        _BASE[gemm] = run_case(gemm, BASE_L, BASE_INPUT_SEED, None)[1]
    base = _BASE[gemm]
    for k, v in rel.items():
        bound = max(REL_FACTOR * base[k], REL_FLOOR)
        print(f"    {k}: rel {v:.2e}, pinned shape {base[k]:.2e}, bound {bound:.2e}")
        assert v <= bound, (what, k, v, base[k])


# ------------------------------------------------------------------------------------------ bit for bit the default path where both run
@pytest.mark.parametrize("L", [800, 10240, 17760, 20320])
def test_run_is_bitwise_the_default_engine(gemm, L):
    """T = 6, 65, 112 and 128: score, the four caches, noisy_dB and P(silence) of one boundary call."""
    (short, _), (long, _) = engine(L, False), engine(L, True)
    clips, caches, noise, thr = inputs(L, 8)
    want = short.run(T(clips), [T(c) for c in caches], thr, noise, return_psil=True)
    got = long.run(T(clips), [T(c) for c in caches], thr, noise, return_psil=True)
    assert short.blobs.mode() == long.blobs.mode() == gemm and short.blobs.range_fallbacks == long.blobs.range_fallbacks == 0
    assert torch.equal(got[0], want[0]) and got[0].dtype == torch.uint8
    for i in range(4):
        assert torch.equal(got[1][i], want[1][i]), i
    assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32))           # bits: NaN = NaN
    assert torch.equal(got[3], want[3])
    assert 0 < int(want[0].sum()) < want[0].numel()


@pytest.mark.parametrize("L", [7680, 17760])
def test_flags_and_detect_are_bitwise_the_default_engine(gemm, L):
    """48 000-sample clips on the grids of T = 49 and T = 112: `flags` with the noise trace, and `detect`."""
    (short, _), (long, _) = engine(L, False), engine(L, True)
    nclips, n = 3, 48000
    clips = weights.burst_clips(nclips, n, seed=BASE_SEED + L)
    noise = np.random.default_rng(9).standard_normal((nclips, 20000))
    lb, stride = long.grid()
    padded, W = fsmn.pad_batch(clips, L, stride, noise, fsmn._prep(True))
    assert W > 1
    want, want_trace = short.flags(T(padded), W, return_noise=True)
    got, got_trace = long.flags(T(padded), W, return_noise=True)
    assert got.shape == (nclips, W * (long.T - lb) + lb) and torch.equal(got, want) and torch.equal(got_trace, want_trace)
    assert 0 < int(want.sum()) < want.numel() and int(want.max()) == 1
    assert long.detect(clips, pad_noise=noise) == short.detect(clips, pad_noise=noise)
    assert long.detect(list(clips), pad_noise=noise) == short.detect(list(clips), pad_noise=noise)
    assert short.blobs.mode() == long.blobs.mode() == gemm and long.blobs.range_fallbacks == 0


# ------------------------------------------------------------------------------------- the float64 net on the device's own log-mel
@pytest.mark.parametrize("L", list(LENGTHS))
def test_long_windows_against_float64(gemm, L):
    """Default widths beyond the 128-frame scratch: P(silence) within 1e-4 and the four output caches within 5e-4 of the float64 net, the
    uint8 score equal to the float64 gate, and no tensor's normalised error above twice the pinned shape's."""
    frames, _, seed = LENGTHS[L]
    assert L // 160 + 1 == frames
    err, rel, rp = run_case(gemm, L, seed, None)
    assert_no_worse_than_the_pinned_shape(gemm, rel, L)


@pytest.mark.parametrize("key", list(WIDTHS), ids=lambda k: "-".join(map(str, k)))
def test_long_window_width_sweep(gemm, key):
    """T = 161 at the smallest and the largest layer widths; the silence bias puts the reference P(silence) on both sides of the gate."""
    err, rel, rp = run_case(gemm, WIDTH_L, WIDTH_SEED, key)
    assert rp.min() < 0.2 and rp.max() > 0.8, (float(rp.min()), float(rp.max()))
    assert_no_worse_than_the_pinned_shape(gemm, rel, (key, WIDTH_L))


def test_two_minutes_as_one_window(gemm):
    """T = 12 001 frames, one stream: 188 tiles by one workgroup with the caches carried through all of them."""
    err, rel, rp = run_case(gemm, LONGEST, LONGEST_SEED, None, B=1)
    assert_no_worse_than_the_pinned_shape(gemm, rel, LONGEST)


# ------------------------------------------------------------------------------------------------------------- long-window energies
@pytest.mark.parametrize("L", [20480, 25608, 160000])
def test_window_stats_long_against_the_two_kernels(gemm, L):
    """vadx_fsmn_window_stats_long against the fallback vadx_fsmn_window_stats takes above 16 384 samples (vadx_frontend_window_means +
    vadx_fsmn_energy): the means bit for bit (exact integer sum, one rounding); the dB values within 8e-6, the bound under which the
    one-pass kernel is accepted against the same pair (tests/test_gpu_fsmn.py::test_window_stats_one_pass_equals_the_two_kernels: a few
    float32 ulps of values around 15, another summation order).  On silence, +-1 LSB noise, full-scale noise and bursts; an overlapping
    grid, and rows that start off every alignment (25 608 is no multiple of 32)."""
    Lb = _lib.lib()                        # (independent of the dense-layer arithmetic: cheap enough to run under each)
    rng = np.random.default_rng(41)
    frames = L // 160 + 1
    for B, W, stride, pad in ((4, 2, L - 4960, 0), (4, 1, L, 3)):
        n = (W - 1) * stride + L
        clips = weights.burst_clips(B, n + pad, seed=B + W)
        clips[0] = 0
        clips[1] = rng.integers(-1, 2, n + pad)
        clips[2] = rng.integers(-32768, 32768, n + pad)
        a = torch.from_numpy(clips).cuda()
        view = a[:, pad:] if pad else a
        m0 = torch.empty(B * W, dtype=torch.float32, device="cuda"); d0 = torch.empty((B * W, frames), dtype=torch.float32, device="cuda")
        m1 = torch.full_like(m0, float("nan")); d1 = torch.full_like(d0, float("nan"))
        ws = torch.empty(Lb.vadx_fsmn_long_workspace_bytes(B * W, frames), dtype=torch.uint8, device="cuda")
        st = _lib.stream_ptr()
        _lib.check(Lb.vadx_frontend_window_means(view.data_ptr(), a.stride(0), stride, B, W, L, C.c_float(1.0), m0.data_ptr(), st))
        _lib.check(Lb.vadx_fsmn_energy(view.data_ptr(), a.stride(0), stride, B, W, L, frames, m0.data_ptr(), d0.data_ptr(), st))
        _lib.check(Lb.vadx_fsmn_window_stats_long(view.data_ptr(), a.stride(0), stride, B, W, L, frames, m1.data_ptr(), d1.data_ptr(),
                                                  ws.data_ptr(), st))
        assert torch.equal(m0, m1)
        assert bool(torch.isfinite(d1).all())
        assert float((d0 - d1).abs().max()) <= 8e-6, (L, pad, float((d0 - d1).abs().max()))


# ------------------------------------------------------------------------------------------------------ whole clips against the oracle
def oracle_clip(fe, w, audio_i16, pad_noise, lb_s):
    """oracle.fsmn.run_clip restated to ALSO return the noise floor after each window (float32, as the reference loop carries it)."""
    L, frame = fe.L, 160
    lb = int(lb_s * ofs.SR // frame)
    stride, slide = L - (lb + 1) * frame, fe.T - lb
    audio, _ = opp.pad_to_window_grid(audio_i16, L, stride, pad_noise)
    caches = [torch.zeros(1, ofs.PROJ, ofs.LORDER - 1, 1) for _ in range(4)]
    noise_dB = np.array([30.0 + 10.0], dtype=np.float32) * np.float32(0.1)
    thr = np.array([1.0], dtype=np.float32)
    silence, saved, trace, s, score = True, [], [], 0, None
    while s + L <= audio.shape[0]:
        sc, caches, noisy = ofs.forward(fe, w, torch.from_numpy(audio[s:s + L].copy()).reshape(1, 1, -1), caches, thr, noise_dB)
        score = sc[0].numpy()
        flags, silence = opp.lookahead_vote(score, slide, lb if lb else 1, 0.5, 0.5, silence)
        saved += flags
        nd = noisy.numpy()[0]
        if nd > 0.0:
            noise_dB = 0.5 * (noise_dB + nd + 10.0 * 0.1)
        trace.append(float(np.asarray(noise_dB).reshape(-1)[0]))
        s += stride
    flags, silence = opp.tail_flags_fsmn(score, slide, fe.T, silence)
    saved += flags
    return opp.process_timestamps(opp.vad_to_timestamps(saved, frame / ofs.SR), 0.3, 0.2), saved, trace


# (L, clip samples, look_backward_s) -> seed of the clips, chosen on the CPU: the oracle's float32 and float64 flags agree on every frame
CLIP_CASES = {
    (48000, 48000, 0.3): 3,         # W = 1: slide = T - 30, a tail of 30
    (32000, 80000, 0.3): 3,         # W = 3: the noise floor and `silence` carried between long windows
    (32000, 80000, 0.0): 3,         # look_backward 0: slide = T, a one-frame vote, no tail
}
_CLIPS = {}


@pytest.mark.parametrize("L,n,lb_s", list(CLIP_CASES), ids=lambda v: str(v))
def test_whole_clips_against_the_oracle(gemm, L, n, lb_s):
    """`flags` (with the noise trace) and `detect` of a long engine against oracle.fsmn.run_clip with Frontend(L): every flag of the `saved`
    list and the same (start, end) pairs; the noise floor after each window within 1e-4 (the file's bound on noisy_dB, which it averages)."""
    seed, nclips = CLIP_CASES[L, n, lb_s], 2
    eng, w = engine(L, True)
    lb, stride = eng.grid(lb_s)
    assert lb == int(lb_s * 100) and stride == L - (lb + 1) * 160
    clips = weights.burst_clips(nclips, n, seed=seed + L)
    noise = np.random.default_rng(9).standard_normal((nclips, 40000))
    got = eng.detect(clips, pad_noise=noise, look_backward_s=lb_s)
    if (L, n, lb_s) not in _CLIPS:
        fe, ow = ofs.Frontend(L), {k: T(v) for k, v in w.items()}
        rows = []
        for b in range(nclips):
            a = opp.normalize_to_int16(clips[b].astype(np.float32))
            rows.append(oracle_clip(fe, ow, a, noise[b], lb_s))
            assert rows[-1][:2] == ofs.run_clip(fe, ow, a, noise[b], look_backward_s=lb_s)        # the restatement is the oracle
        _CLIPS[L, n, lb_s] = rows
    for b in range(nclips):
        a = opp.normalize_to_int16(clips[b].astype(np.float32))
        want_ts, want_flags, want_trace = _CLIPS[L, n, lb_s][b]
        padded = fsmn.pad_to_window_grid(a, L, stride, noise[b])
        W = (padded.shape[0] - L) // stride + 1
        assert W == len(want_trace) == (1 if n <= L else 3)
        flags, trace = eng.flags(torch.from_numpy(padded[None]), W, return_noise=True, look_backward_s=lb_s)
        flags = flags.cpu().numpy()[0]
        assert flags.shape[0] == len(want_flags) == W * (eng.T - lb) + lb and int(flags.max()) <= 1
        mism = np.flatnonzero(flags.astype(bool) != np.array(want_flags, bool))
        assert len(mism) == 0, (b, mism[:10])
        assert 0 < int(flags.sum()) < flags.shape[0]
        np.testing.assert_allclose(trace.cpu().numpy()[0], np.array(want_trace, np.float32), rtol=0, atol=ATOL)
        assert got[b] == want_ts
    assert eng.blobs.mode() == gemm and eng.blobs.range_fallbacks == 0


# ---------------------------------------------------------------------------------------------------------------------------- ragged
RAGGED_L = 32000
RAGGED_N = (8000, 32000, 59040, 100000, 144000)        # 0.5 s .. 9 s: W = 1, 1, 2, 4, 6 on the stride of 27 040


def ragged_batch():
    if "rb" not in _CLIPS:
        eng, _ = engine(RAGGED_L, True)
        clips = [weights.burst_clips(1, n, seed=700 + k)[0] for k, n in enumerate(RAGGED_N)]
        noise = np.random.default_rng(11).standard_normal((5, 40000))
        rb = eng.ragged(clips, noise)
        assert rb.stride == 27040 and rb.windows.tolist() == [1, 1, 2, 4, 6] and rb.order_host.tolist() == [4, 3, 2, 0, 1]
        _CLIPS["rb"] = rb
    return _CLIPS["rb"]


def ragged_reference(gemm):
    """`flags` of the long engine on each padded clip ALONE, once per arithmetic: [(flags u8 [nflags_b], noise trace f32 [W_b])]"""
    if ("ref", gemm) not in _CLIPS:
        eng, rb = engine(RAGGED_L, True)[0], ragged_batch()
        ref = []
        for b in range(len(rb)):
            flags, trace = eng.flags(T(rb.padded(b)[None, :]), int(rb.windows[b]), return_noise=True)
            ref.append((flags[0].clone(), trace[0].clone()))
        assert eng.blobs.mode() == gemm
        _CLIPS["ref", gemm] = ref
    return _CLIPS["ref", gemm]


def test_flags_ragged_is_bitwise_the_per_clip_path(gemm):
    """Five clips from 0.5 s to 9 s on the L = 32 000 grid (T = 201): row b is `flags(padded_b[None], W_b)` followed by 255s, with the
    longest clip first and with clip b on workgroup b."""
    eng, rb, ref = engine(RAGGED_L, True)[0], ragged_batch(), ragged_reference(gemm)
    lb, _ = eng.grid()
    for order in (None, "identity"):
        flags, nflags, trace = eng.flags_ragged(rb, order=order, return_noise=True)
        assert flags.shape == (5, rb.max_windows * (eng.T - lb) + lb) and flags.dtype == torch.uint8 and trace.shape == (rb.n_windows,)
        assert nflags.tolist() == [201, 201, 372, 714, 1056]
        for b in range(5):
            want, want_trace = ref[b]
            assert torch.equal(flags[b, :nflags[b]], want), (order, b)
            assert bool((flags[b, nflags[b]:] == 255).all()), (order, b)
            assert torch.equal(trace[rb.win_first_host[b]:rb.win_first_host[b + 1]], want_trace), (order, b)
    assert eng.blobs.mode() == gemm and eng.blobs.range_fallbacks == 0


def test_lying_table_entries_leave_their_rows_at_255(gemm):
    """A clip that claims more windows than max_windows and one that claims none: those rows stay all 255, their neighbours are the
    per-clip result.  Bounds-guard checks on table VALUES, as tests/test_gpu_ragged.py has them: the buffers are sized so that even an
    unguarded kernel would stay inside them."""
    eng, rb, ref = engine(RAGGED_L, True)[0], ragged_batch(), ragged_reference(gemm)
    lb, _ = eng.grid()
    slide, B, nwin, maxw = eng.T - lb, 5, rb.n_windows, rb.max_windows
    logmel, db = eng.features(rb.gather(), 1, RAGGED_L)
    spare = 8                                                             # clip 4 claims windows 8 .. 21: the buffers hold them
    logmel = torch.cat([logmel, torch.zeros((spare, eng.T, 80), device=logmel.device)])
    db = torch.cat([db, torch.zeros((spare, eng.T), device=db.device)])
    stride_f = (maxw + spare) * slide + lb                                # a row holds the flags of the longest claim
    lp = fsmn._loop_params(lb)
    cache = torch.empty((B, 4, 128, 19), dtype=torch.float32, device=eng.device)
    ws = eng._workspace(B)

    def run(win_first, n_windows):
        flags = torch.zeros((B + 2, stride_f), dtype=torch.uint8, device=eng.device)          # two spare rows behind the last clip
        wf = T(np.asarray(win_first, np.int32)).to(eng.device)

        def launch(mode, dims, packed):
            _lib.check(_lib.lib().vadx_fsmn_clips_long(C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), B, n_windows,
                                                       maxw, wf.data_ptr(), None, C.byref(lp), cache.data_ptr(), flags.data_ptr(), stride_f,
                                                       None, ws.data_ptr(), _lib.stream_ptr()))
            return flags
        return eng.blobs.guarded(launch)

    def check(flags, dead):
        for b in range(B):
            if b in dead:
                assert bool((flags[b] == 255).all()), b
            else:
                n = ref[b][0].numel()
                assert torch.equal(flags[b, :n], ref[b][0]) and bool((flags[b, n:] == 255).all()), b
        assert not bool(flags[B:].any())                                 # nothing behind the batch's rows was written

    assert rb.win_first_host.tolist() == [0, 1, 2, 4, 8, 14]
    check(run([0, 1, 2, 4, 8, 22], nwin + spare), {4})                   # W_4 = 14 > max_windows = 6
    check(run([0, 1, 2, 4, 3, 14], nwin), {3, 4})                        # W_3 = -1, W_4 = 11 > max_windows
    assert eng.blobs.mode() == gemm


def test_driver_takes_a_long_engine(gemm, tmp_path):
    """drivers.inference_fsmn with a long engine object and a list of two files of different lengths: the engine's own `detect` of the list."""
    import wave
    from vadx import drivers
    eng, _ = engine(RAGGED_L, True)
    clips = [weights.burst_clips(1, n, seed=600 + k)[0] for k, n in enumerate((80000, 48000))]
    paths = []
    for k, a in enumerate(clips):
        paths.append(str(tmp_path / f"c{k}.wav"))
        with wave.open(paths[-1], "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000); wf.writeframes(a.tobytes())          # noqa: E702
    noise = np.random.default_rng(13).standard_normal((2, 40000))
    got = drivers.inference_fsmn(paths, eng, str(tmp_path / "s.txt"), str(tmp_path / "i.txt"), pad_noise=noise, echo=lambda *_: None)
    assert got == eng.detect(clips, pad_noise=noise) and all(len(ts) >= 1 for ts in got)
    assert eng.blobs.mode() == gemm


# -------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_by_name(gemm):
    w = weights.fsmn_synthetic(BASE_SEED)
    with pytest.raises(ValueError, match="input_audio_length=9600160"):
        fsmn.FsmnEngine(w, input_audio_length=9600160, long_windows=True)
    with pytest.raises(ValueError, match="input_audio_length=500"):
        fsmn.FsmnEngine(w, input_audio_length=500, long_windows=True)
    eng, _ = engine(20480, True)
    assert eng.T == 129
    with pytest.raises(ValueError, match="FsmnStreamBatch.*129 frames"):
        fsmn.FsmnStreamBatch(eng, 2)
    with pytest.raises(ValueError, match="look_backward_s=1.3"):          # 130 frames >= T - 1: no stride left
        eng.flags(torch.zeros((1, 20480), dtype=torch.int16), 1, look_backward_s=1.3)
    odd = fsmn.FsmnEngine(w, input_audio_length=25604, long_windows=True)
    with pytest.raises(ValueError, match="input_audio_length=25604 must be a multiple of 8"):
        odd.ragged([np.zeros(30000, np.int16)])
    # the opt-in is explicit: the default engine and session still refuse the same length, with the phrases they had
    with pytest.raises(ValueError, match="112"):
        fsmn.FsmnEngine(w, input_audio_length=20480)
    with pytest.raises(ValueError, match="at most 128"):
        fsmn.FsmnSession(w, input_audio_length=20480)
    with pytest.raises(ValueError, match="long_windows=True"):
        fsmn.FsmnEngine(w, input_audio_length=20480, long_windows=False)


# --------------------------------------------------------------------------------------------------------------------------- session
def test_long_session(gemm):
    """FsmnSession(w, 160000, long_windows=True): `[1,1,160000]` and `[1001]`; a batch of two streams run twice with the caches fed back
    equals engine.run on the same inputs; io_dtype="float16" rounds once at the boundary, as the short session does."""
    L, frames = 160000, 1001
    w = weights.fsmn_synthetic(BASE_SEED)
    s32 = fsmn.FsmnSession(w, L, long_windows=True)
    s16 = fsmn.FsmnSession(w, L, io_dtype="float16", long_windows=True)
    for s in (s32, s16):
        assert s._inputs_meta[0].shape == [1, 1, L] and s._inputs_meta[0].type == "tensor(int16)" and s._outputs_meta[0].shape == [frames]
    assert "float16" in s16._inputs_meta[1].type and "float16" in s16._outputs_meta[5].type and "float16" not in s32._inputs_meta[1].type
    rng = np.random.default_rng(5)
    audio = weights.burst_clips(2, 2 * L, seed=21)
    c16 = [(rng.standard_normal((2, 128, 19, 1)) * 0.3).astype(np.float16) for _ in range(4)]
    c32 = [c.astype(np.float32) for c in c16]
    ceng = [T(c[..., 0]) for c in c32]
    thr16, nz16 = np.array([1.0, 1.0], np.float16), np.array([4.0, 1.25], np.float16)
    for k in range(2):
        a = audio[:, k * L:(k + 1) * L].reshape(2, 1, -1)
        feeds16 = {"audio": a, "one_minus_speech_threshold": thr16, "noise_average_dB": nz16, **{f"cache_{i}": c16[i] for i in range(4)}}
        feeds32 = {"audio": a, "one_minus_speech_threshold": thr16.astype(np.float32), "noise_average_dB": nz16.astype(np.float32),
                   **{f"cache_{i}": c32[i] for i in range(4)}}
        o32, o16 = s32.run(None, feeds32), s16.run(None, feeds16)
        score, cout, noisy = s32.engine.run(T(a[:, 0]), ceng, thr16.astype(np.float32), nz16.astype(np.float32))
        assert o32[0].dtype == np.uint8 and o32[0].shape == (2, frames) and np.array_equal(o32[0], score.cpu().numpy())
        assert 0 < int(o32[0].sum()) < o32[0].size
        for i in range(4):
            assert o32[1 + i].shape == (2, 128, 19, 1) and np.array_equal(o32[1 + i][..., 0], cout[i].cpu().numpy())
        assert np.array_equal(o32[5], noisy.cpu().numpy(), equal_nan=True)
        if k == 0:                                                         # same float16-representable feeds: one rounding at the boundary
            assert np.array_equal(o16[0], o32[0])
            for i in range(1, 6):
                assert o16[i].dtype == np.float16 and np.array_equal(o16[i], o32[i].astype(np.float16), equal_nan=True)
        c32, ceng = o32[1:5], cout                                          # the caches fed back
        c16 = o16[1:5]
    assert s32.engine.blobs.mode() == gemm and s32.engine.blobs.range_fallbacks == 0
