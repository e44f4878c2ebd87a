"""GPU: ragged batches (vadx.ragged.RaggedBatch; vadx_windows_gather, vadx_fsmn_clips_ragged, vadx_tracks_gather) against the paths
that take one clip at a time -- FsmnEngine.flags bit for bit, FireRedEngine.detect / detect_events tracks bit for bit -- and against the
CPU oracle's restatement of the reference loop.  Five FSMN clips (shorter than a window, exactly one window, exactly on the grid, and two
that need padding: W = 1, 1, 2, 3, 4) and four FireRed clips (W = 1, 1, 2, 3): every per-clip bound differs, T = 101 frames per window
already takes the 64 + 48-frame tile split, and nothing depends on the batch beyond one workgroup per clip."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, drivers, firered, fsmn, ragged, weights
from oracle import fsmn as ofs
from oracle import postproc as opp

pytestmark = pytest.mark.gpu
L, SEED = 16000, 1234
FSMN_N = (9000, 16000, 27040, 30000, 45000)
FIRERED_N = (9000, 16000, 25000, 40000)


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
    """One engine for the file: its blobs are per arithmetic, the arithmetic is the module default the `gemm` fixture sets."""
    if "eng" not in _CACHE:
        _CACHE["eng"] = fsmn.FsmnEngine(weights.fsmn_synthetic(SEED))
    return _CACHE["eng"]


def fsmn_audio():
    """(raw clips, peak-normalised clips, padding noise [5, 20000])"""
    if "audio" not in _CACHE:
        clips = [weights.burst_clips(1, n, seed=700 + k)[0] for k, n in enumerate(FSMN_N)]
        norm = [opp.normalize_to_int16(c.astype(np.float32)) for c in clips]
        _CACHE["audio"] = (clips, norm, np.random.default_rng(11).standard_normal((5, 20000)))
    return _CACHE["audio"]


def batch(lb_s):
    """The packed batch at one look-back, on the device; at 0.3 s the layout the fixture is known to give is asserted first."""
    if ("rb", lb_s) not in _CACHE:
        clips, norm, noise = fsmn_audio()
        rb = engine().ragged(clips, noise, look_backward_s=lb_s)
        if lb_s == 0.3:
            assert rb.stride == 11040 and rb.padded_lengths.tolist() == [16000, 16000, 27040, 38080, 49120]
            assert rb.windows.tolist() == [1, 1, 2, 3, 4] and rb.win_first_host.tolist() == [0, 1, 2, 4, 7, 11]
            assert rb.order_host.tolist() == [4, 3, 2, 0, 1]
        for b in range(5):
            assert np.array_equal(rb.padded(b), fsmn.pad_to_window_grid(norm[b], L, rb.stride, noise[b])), b
        _CACHE["rb", lb_s] = rb
    return _CACHE["rb", lb_s]


def per_clip_reference(gemm, lb_s):
    """The existing path on each clip ALONE, once per (arithmetic, look-back): [(flags u8 [nflags_b], noise trace f32 [W_b])]"""
    if ("ref", gemm, lb_s) not in _CACHE:
        rb, eng = batch(lb_s), engine()
        ref = []
        for b in range(len(rb)):
            flags, trace = eng.flags(T(rb.padded(b)[None, :]), int(rb.windows[b]), look_backward_s=lb_s, return_noise=True)
            ref.append((flags[0].clone(), trace[0].clone()))
        assert eng.blobs.mode() == gemm
        _CACHE["ref", gemm, lb_s] = ref
    return _CACHE["ref", gemm, lb_s]


# ---------------------------------------------------------------------------------------------------------------------------- gather
def gather(pcm, win_src, window):
    wbuf = torch.full((win_src.numel(), window), 12345, dtype=torch.int16, device=pcm.device)
    _lib.check(_lib.lib().vadx_windows_gather(pcm.data_ptr(), pcm.numel(), win_src.data_ptr(), win_src.numel(), window, wbuf.data_ptr(),
                                              _lib.stream_ptr()))
    return wbuf.cpu().numpy()


@pytest.mark.parametrize("stride", [11040, L, 15840])
def test_windows_gather_is_numpy_slicing(stride):
    clips, norm, noise = fsmn_audio()
    rb = ragged.RaggedBatch.from_clips(norm, L, stride, noise)
    got = rb.gather().cpu().numpy()
    assert got.shape == (rb.n_windows, L)
    for w, src in enumerate(rb.win_src_host):
        assert np.array_equal(got[w], rb.pcm_host[src:src + L]), w
    # offsets that leave [0, pcm_len): windows of zeros, every other window as before
    total = rb.pcm_host.shape[0]
    bad = {0: total + 8, 2: -8, 3: total - L + 8, rb.n_windows - 1: total}
    src = rb.win_src_host.copy()
    for w, v in bad.items():
        src[w] = v
    got2 = gather(rb.pcm, T(src).to(rb.pcm.device), L)
    for w in range(rb.n_windows):
        assert np.array_equal(got2[w], np.zeros(L, np.int16) if w in bad else got[w]), w


# ------------------------------------------------------------------------------------------------------------------------------ FSMN
@pytest.mark.parametrize("lb_s", [0.3, 0.0])
def test_flags_ragged_is_bitwise_the_per_clip_path(gemm, lb_s):
    eng, rb = engine(), batch(lb_s)
    ref = per_clip_reference(gemm, lb_s)
    lb, _ = eng.grid(lb_s)
    fallbacks = eng.blobs.range_fallbacks
    first = None
    for order in (None, "identity", rb.order_host, rb.order_host[::-1].copy()):
        flags, nflags, trace = eng.flags_ragged(rb, order=order, return_noise=True, look_backward_s=lb_s)
        assert flags.shape == (5, rb.max_windows * (eng.T - lb) + lb) and flags.dtype == torch.uint8 and trace.shape == (rb.n_windows,)
        assert np.array_equal(nflags, rb.windows * (eng.T - lb) + lb)
        for b in range(5):
            want, want_trace = ref[b]
            assert nflags[b] == want.numel()
            assert torch.equal(flags[b, :nflags[b]], want), (order, b)
            assert bool((flags[b, nflags[b]:] == 255).all()), (order, b)
            assert torch.equal(trace[rb.win_first_host[b]:rb.win_first_host[b + 1]], want_trace), (order, b)
        if first is None:
            first = flags.clone()
        assert torch.equal(flags, first)
    assert eng.blobs.mode() == gemm and eng.blobs.range_fallbacks == fallbacks        # the equality is not a fallback's
    if lb_s == 0.3:
        assert nflags.tolist() == [101, 101, 172, 243, 314]


def test_every_clip_against_the_oracle(gemm):
    """oracle.fsmn.run_clip on each clip with its padding noise: every flag of the `saved` list (no excused frames: the oracle's closest
    frame lies 2.4e-2 from its deciding threshold, two orders above the 1e-4 score bound) and the same (start, end) pairs."""
    eng, rb = engine(), batch(0.3)
    clips, norm, noise = fsmn_audio()
    if "oracle" not in _CACHE:
        ow = {k: T(v) for k, v in weights.fsmn_synthetic(SEED).items()}
        _CACHE["oracle"] = [ofs.run_clip(ofs.Frontend(), ow, norm[b], noise[b]) for b in range(5)]
    flags, nflags = eng.flags_ragged(rb)
    flags = flags.cpu().numpy()
    got_ts = eng.detect(clips, pad_noise=noise)
    assert [len(ts) for ts, _ in _CACHE["oracle"]] == [1, 1, 1, 1, 2]
    for b, (want_ts, want_flags) in enumerate(_CACHE["oracle"]):
        assert nflags[b] == len(want_flags), b
        assert np.array_equal(flags[b, :nflags[b]].astype(bool), np.array(want_flags, bool)), b
        assert got_ts[b] == want_ts, b
        assert got_ts[b] == eng.detect(clips[b][None, :], pad_noise=noise[b:b + 1])[0], b
    assert eng.blobs.mode() == gemm


def test_bad_table_entries_leave_their_rows_at_255(gemm):
    """One clip with W_b > max_windows, then an order naming clips that do not exist: those rows are all 255, the others unchanged.
    (The buffers are sized so that even an unguarded kernel would stay inside them.)"""
    eng, rb = engine(), batch(0.3)
    ref = per_clip_reference(gemm, 0.3)
    lb, _ = eng.grid(0.3)
    slide, B, nwin, maxw = eng.T - lb, 5, rb.n_windows, rb.max_windows
    logmel, db = eng.features(rb.gather(), 1, L)
    grown = nwin + 5                                                    # clip 4 claims windows 7 .. 15: W = 9 > max_windows = 4
    logmel = torch.cat([logmel, torch.zeros((5, eng.T, 80), device=logmel.device)])
    db = torch.cat([db, torch.zeros((5, eng.T), device=db.device)])
    stride_f = maxw * slide + lb
    lp = fsmn._loop_params(lb)
    cache = torch.empty((B, 4, 128, 19), dtype=torch.float32, device=eng.device)

    def run(win_first, order, n_windows):
        flags = torch.zeros((B + 3, stride_f), dtype=torch.uint8, device=eng.device)          # three spare rows behind the last clip
        wf = T(np.asarray(win_first, np.int32)).to(eng.device)
        od = None if order is None else T(np.asarray(order, np.int32)).to(eng.device)

        def launch(mode, dims, packed):
            _lib.check(_lib.lib().vadx_fsmn_clips_ragged(C.byref(dims), packed.data_ptr(), logmel.data_ptr(), db.data_ptr(), B, n_windows,
                                                         maxw, wf.data_ptr(), None if od is None else od.data_ptr(), C.byref(lp),
                                                         cache.data_ptr(), flags.data_ptr(), stride_f, None, _lib.stream_ptr()))
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

    check(run([0, 1, 2, 4, 7, 16], None, grown), {4})                    # W_4 = 9 > max_windows
    check(run([0, 1, 2, 4, 7, 16], None, nwin), {4})                     # ... and past n_windows
    check(run([0, 1, 2, 2, 7, 11], None, nwin), {2, 3})                  # W_2 = 0, W_3 = 5
    check(run([0, 1, 2, 4, 3, 11], None, nwin), {3, 4})                  # W_3 = -1, W_4 = 8
    check(run(rb.win_first_host, [3, 2, 99, 1, -1], nwin), {0, 4})       # order entries outside [0, batch)
    assert eng.blobs.mode() == gemm


# --------------------------------------------------------------------------------------------------------------------------- FireRed
def firered_audio():
    if "fr_audio" not in _CACHE:
        clips = [weights.burst_clips(1, n, seed=800 + k)[0] for k, n in enumerate(FIRERED_N)]
        _CACHE["fr_audio"] = (clips, np.random.default_rng(11).standard_normal((4, 20000)))
    return _CACHE["fr_audio"]


def firered_engine(odim):
    if ("fr", odim) not in _CACHE:
        _CACHE["fr", odim] = firered.FireRedEngine(weights.firered_synthetic(SEED, dict(weights.FIRERED_CFG, odim=odim)))
    return _CACHE["fr", odim]


def test_firered_detect_list_equals_one_clip_at_a_time(gemm):
    eng = firered_engine(1)
    clips, noise = firered_audio()
    rb = eng.ragged(clips, noise)
    assert rb.windows.tolist() == [1, 1, 2, 3] and eng.T == 98
    assert firered.valid_frame_count(40000) == 248 < 3 * eng.T
    probs = eng.run_ragged(rb)
    assert probs.shape == (7, 1, 98)
    out, tracks, decs = eng.detect(clips, pad_noise=noise, return_probs=True)
    assert [t.numel() for t in tracks] == [54, 98, 154, 248]
    for k, c in enumerate(clips):
        one, track, dec = eng.detect(c[None, :], pad_noise=noise[k:k + 1], return_probs=True)
        assert out[k] == one[0], k
        assert torch.equal(tracks[k], track[0]) and torch.equal(decs[k], dec[0]), k
    assert eng.detect(clips, pad_noise=noise) == out
    assert eng.blobs.mode() == gemm


def test_firered_detect_events_list_equals_one_clip_at_a_time(gemm):
    eng = firered_engine(3)
    clips, noise = firered_audio()
    out, tracks = eng.detect_events(clips, pad_noise=noise, return_probs=True)
    for k, c in enumerate(clips):
        one, tr = eng.detect_events(c[None, :], pad_noise=noise[k:k + 1], return_probs=True)
        assert out[k] == one[0], k
        assert tracks[k].shape == tr[0].shape and torch.equal(tracks[k], tr[0]), k
    assert eng.detect_events(clips, pad_noise=noise) == out


def test_event_ratio_product_is_torchs_device_mean():
    """detect_events on a list counts the frames over threshold and multiplies by the float32 reciprocal of the frame count; the one-clip
    path takes torch's mean of the 0 / 1 values on the device.  Bitwise the same for every count at every frame count up to three windows."""
    for n in range(1, 3 * 98 + 1):
        ones = torch.tril(torch.ones((n + 1, n), device="cuda"), diagonal=-1)          # row c holds c ones
        want = (ones >= 0.5).float().mean(dim=1).cpu().numpy()
        got = np.arange(n + 1).astype(np.float32) * (np.float32(1.0) / np.float32(n))
        assert np.array_equal(got, want), n


def test_tracks_gather_against_numpy():
    rng = np.random.default_rng(5)
    odim, fpw, stride = 3, 98, 300
    win_first = np.array([0, 1, 2, 4, 7, 7, 9], np.int32)               # W = 1, 1, 2, 3, 0, 2
    n_frames = np.array([54, 98, 500, 248, 10, -3], np.int32)           # inside, exact, more than W * fpw, inside, no windows, negative
    probs = rng.random((9, odim, fpw), dtype=np.float32)
    pd, wf, nf = T(probs).cuda(), T(win_first).cuda(), T(n_frames).cuda()
    for ch in range(odim):
        got = torch.full((6, stride), -1.0, device="cuda")
        _lib.check(_lib.lib().vadx_tracks_gather(pd.data_ptr(), odim * fpw, ch * fpw, fpw, wf.data_ptr(), nf.data_ptr(), 6, got.data_ptr(),
                                                 stride, _lib.stream_ptr()))
        want = np.zeros((6, stride), np.float32)
        for b in range(6):
            full = probs[win_first[b]:win_first[b + 1], ch].reshape(-1)
            n = max(0, min(int(n_frames[b]), full.shape[0], stride))
            want[b, :n] = full[:n]
        assert np.array_equal(got.cpu().numpy(), want), ch
    # a track narrower than the clip's frames is cut, not overrun
    got = torch.full((6, 100), -1.0, device="cuda")
    _lib.check(_lib.lib().vadx_tracks_gather(pd.data_ptr(), odim * fpw, 0, fpw, wf.data_ptr(), nf.data_ptr(), 6, got.data_ptr(), 100,
                                             _lib.stream_ptr()))
    assert np.array_equal(got[3].cpu().numpy(), probs[4:7, 0].reshape(-1)[:100])


# --------------------------------------------------------------------------------------------------------------------------- drivers
def test_drivers_hand_a_file_list_over_as_one_ragged_batch(tmp_path, gemm):
    paths, lens = [], [40000, 25000, 40000, 16000]
    for k, n in enumerate(lens):
        pth = str(tmp_path / f"c{k}.wav")
        with wave.open(pth, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(weights.burst_clips(1, n, seed=500 + k)[0].tobytes())
        paths.append(pth)
    noise = np.random.default_rng(77).standard_normal((len(paths), 20000))
    quiet = lambda *_: None                                                     # noqa: E731
    files = (str(tmp_path / "s.txt"), str(tmp_path / "i.txt"))
    seen = []
    for eng in (engine(), firered_engine(1)):
        ragged_call = eng.flags_ragged if eng is engine() else eng.run_ragged
        run = drivers.inference_fsmn if eng is engine() else drivers.inference_firered
        spy = lambda *a, _f=ragged_call, **kw: (seen.append(len(a[0])), _f(*a, **kw))[1]      # noqa: E731
        setattr(eng, ragged_call.__name__, spy)
        try:
            many = run(paths, eng, *files, pad_noise=noise, echo=quiet)
            assert seen == [len(paths)]                                  # one ragged batch of all four files
            for k, pth in enumerate(paths):
                assert many[k] == run(pth, eng, *files, pad_noise=noise[k:k + 1], echo=quiet), (run.__name__, k)
            assert seen == [len(paths)]                                  # a single file goes the way it always went
        finally:
            delattr(eng, ragged_call.__name__)
        seen.clear()
    aed = firered_engine(3)
    many = drivers.inference_firered_aed(paths, aed, pad_noise=noise, echo=quiet)
    assert len(many) == len(paths)
    for k, pth in enumerate(paths):
        assert many[k] == drivers.inference_firered_aed(pth, aed, pad_noise=noise[k:k + 1], echo=quiet), k
