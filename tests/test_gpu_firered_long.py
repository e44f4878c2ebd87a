"""GPU: FireRed windows of any length (FireRedEngine(long_windows=True), vadx_firered_run_long, vadx_frontend_logmel_ragged_snip).

1. Where the default engine applies too (T <= 112 frames) the long engine returns the same bytes: every tile edge of the 64-frame walk, at the
   published widths on the three arithmetics, and on float32 at other widths, depths and FIR tap shapes.
2. Beyond 112 frames the long engine is held to the float64 net on the device's own log-mel, with the bounds, the re-centred head and the
   pinned-shape ratio of tests/test_gpu_firered_shapes.py (its helpers are imported, so the two files share one cache of references).
3. A clip of a dynamic list -- or of a static long grid through `run_ragged` -- gets the log-mel and the probabilities of the one-clip call,
   bit for bit, in any order; at the C level inside canary guards with buffers of exactly the required bytes; and in a batch whose workspace
   planes pass 2^32 bytes.
4. Table entries that lie leave their rows untouched and every other clip's bytes right.
5. The fp16 x 2 range protocol: a loud log-mel raises the flag once and the call returns the bf16 x 3 result.
6. End to end: detect / detect_table / detect_events on a dynamic engine against oracle.firered.run_clip(window=len(clip)) under thresholds
   placed in a score gap; the drivers on wav files; the session's dynamic shapes; collect_chunks_batch -> from_packed -> detect.

VADX_FIRERED_LONG_ERRORS=<path> appends the figures of item 2 to that file (profiles/firered_long_errors.txt is such a run).
"""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, chunks, drivers, firered, ragged, weights
from vadx import frontend as vfe
from oracle import firered as ofr
from oracle import postproc as opp

from test_gpu_firered_shapes import (ATOL, B, BASE_SEED, TAP_SEEDS, WIDTH_SEED, K, T, assert_float32_grade, cfg_name, clips_for,  # noqa: F401
                                     gemm, logit_error, logmel_of, make_cfg, reference, samples, split_eligible, three_arithmetics)

pytestmark = pytest.mark.gpu

SAME_T = [1, 2, 19, 20, 21, 63, 64, 65, 84, 85, 98, 111, 112]
LONG_T = [113, 127, 128, 129, 148, 149, 192, 193, 257, 998, 6001]
WIDTHS = [K(H=250, P=120), K(M=4, odim=4), K(R=1)]
TAPS = [(21, 1, 20, 1), (20, 1, 20, 2), (1, 1, 1, 1), (3, 1, 0, 0), (32, 4, 32, 4), (8, 2, 4, 3)]


def tap_key(taps):
    n1, s1, n2, s2 = taps
    return K(N1=n1, S1=s1, N2=n2, S2=s2) + (K(R=2) if n1 == 32 else ())


def tap_seed(taps):
    return TAP_SEEDS.get(taps, BASE_SEED)


SETS = [(k, WIDTH_SEED) for k in WIDTHS] + [(tap_key(t), tap_seed(t)) for t in TAPS]


def centred_weights(key, seed, frames=98):
    """`key`'s synthetic weights with the head re-centred on the float64 logits of a T = `frames` batch (the shapes file's own case, shared
    with it): probabilities spread over (0, 1), so equal bytes mean equal logits and not two saturated sigmoids."""
    cfg, L = make_cfg(key), samples(frames)
    audio = T(clips_for(L, seed)).cuda()
    name = ("window", key, frames, seed)
    feats = [logmel_of(vfe.Frontend("firered", L), audio, L)]         # (`reference` keeps the first it saw under `name`)
    return reference(name, weights.firered_synthetic(seed, cfg), feats, None)["w"]


# ------------------------------------------------------------------ 1. the same bytes where both engines apply
def same_bytes(key, seed):
    w, bad = centred_weights(key, seed), []
    for frames in SAME_T:
        L = samples(frames)
        audio = T(clips_for(L, seed)).cuda()
        short, long_ = firered.FireRedEngine(w, L), firered.FireRedEngine(w, L, long_windows=True)
        a, b = short.run(audio, 1), long_.run(audio, 1)
        assert a.shape == b.shape == (B, make_cfg(key)["odim"], frames) and bool(torch.isfinite(b).all())
        assert short.cfg.arithmetic == long_.cfg.arithmetic and short.blobs.range_fallbacks == long_.blobs.range_fallbacks == 0
        if not torch.equal(a, b):
            bad.append((frames, float((a - b).abs().max())))
        # (two windows per clip: the rectangular tables at more than one window per row)
        if frames == 65:
            two = T(np.concatenate([clips_for(L, seed), clips_for(L, seed + 1)], axis=1)).cuda()
            assert torch.equal(short.run(two, 2), long_.run(two, 2))
    assert not bad, (cfg_name(key), bad)


@three_arithmetics
def test_same_bytes_as_the_default_engine_published_widths(gemm):
    """T on every edge of the 64-frame tile walk and of the default kernel's own walks, published widths, three arithmetics: torch.equal."""
    same_bytes((), BASE_SEED)


@pytest.mark.parametrize("gemm", ["f32"], indirect=True)
@pytest.mark.parametrize("key,seed", SETS, ids=[cfg_name(k) for k, _ in SETS])
def test_same_bytes_as_the_default_engine_other_shapes(gemm, key, seed):
    """float32 at widths that pad (250 / 120), the M = 4 / odim = 4 tail, R = 1, and the tap shapes: 21 taps, a dilated look-ahead, one tap,
    no look-ahead, a reach of 124 / 128 frames, the dilated pair (8, 2, 4, 3)."""
    same_bytes(key, seed)


# ------------------------------------------------------------------ 2. beyond 112 frames, against float64
_WORST = {}
ERRORS_HEADER = ("FireRed long path (FireRedEngine(long_windows=True), vadx_firered_run_long) against the float64 net on the device's own log-mel, head\n"
                 "re-centred per case; written by tests/test_gpu_firered_long.py under VADX_FIRERED_LONG_ERRORS, one line per case in run order.\n"
                 "p: max |prob - ref| (bound 1e-4); e: max logit error / sd(z_ref), held to 2 * max(e_pinned, R_arith * e32); e32: the float32 torch\n"
                 "oracle's own e; inside: share of the reference in (0.02, 0.98); B = 4 windows per case; the last line's `worst so far` is the file's.\n\n")


def long_case(gemm, key, frames, seed):
    cfg, L = make_cfg(key), samples(frames)
    audio = T(clips_for(L, seed)).cuda()
    name = ("long", key, frames, seed)
    feats = [logmel_of(vfe.Frontend("firered", L), audio, L)]         # (`reference` keeps the first it saw under `name`)
    ref = reference(name, weights.firered_synthetic(seed, cfg), feats, None)        # asserts >= 90 % of the reference in (0.02, 0.98)
    eng = firered.FireRedEngine(ref["w"], L, long_windows=True)
    assert eng.T == frames
    assert np.array_equal(logmel_of(eng.fe, audio, L), ref["feats"][0])             # the reference saw what the net sees
    probs = eng.run(audio, 1)
    want = gemm if split_eligible(cfg) else "f32"
    assert eng.cfg.arithmetic == _lib.GEMM_MODES[want] and eng.blobs.range_fallbacks == 0
    got = probs.cpu().numpy().astype(np.float64)
    assert got.shape == ref["p"].shape == (B, cfg["odim"], frames) and np.isfinite(got).all()
    p, e = float(np.abs(got - ref["p"]).max()), logit_error(got, ref["p"])
    line = f"firered long {want} T={frames} {cfg_name(key)}: p {p:.2e} e {e:.2e} e32 {ref['e32']:.2e} p32 {ref['p32']:.2e} inside {ref['inside']:.3f}"
    print(line)
    worst = _WORST.setdefault("all", dict(p=0.0, e=0.0, ratio=0.0))
    worst.update(p=max(worst["p"], p), e=max(worst["e"], e), ratio=max(worst["ratio"], e / ref["e32"]))
    path = os.environ.get("VADX_FIRERED_LONG_ERRORS")
    if path:
        new = not os.path.exists(path)
        with open(path, "a") as fh:
            if new:
                fh.write(ERRORS_HEADER)
            fh.write(f"{line} | worst so far: p {worst['p']:.2e} e {worst['e']:.2e} e/e32 {worst['ratio']:.2f}\n")
    assert p <= ATOL, (key, frames, p)
    assert_float32_grade(want, e, ref["e32"], (key, frames))


@three_arithmetics
@pytest.mark.parametrize("frames", LONG_T)
def test_long_window_against_float64(gemm, frames):
    """Default config from the first frame count the default engine refuses to 60 s: one tile more than a window held (113), tile edges
    (127 .. 129, 192, 193, 257), 148 / 149 (a tail of 20 / 21 frames: the look-ahead's reach), 10 s and 60 s."""
    long_case(gemm, (), frames, BASE_SEED)


@pytest.mark.parametrize("gemm", ["f32"], indirect=True)
@pytest.mark.parametrize("frames", [113, 200])
@pytest.mark.parametrize("key,seed", SETS, ids=[cfg_name(k) for k, _ in SETS])
def test_long_window_other_shapes_against_float64(gemm, key, seed, frames):
    long_case(gemm, key, frames, seed)


# ------------------------------------------------------------------ 3. ragged equals the clip alone
EDGE_T = SAME_T + [113, 127, 128, 129, 148, 149, 192, 193, 257, 998]


def edge_clips(seed=5):
    """Clips whose frame counts sit on every edge above, with sample counts off the hop grid, and one clip of 399 samples (no frame)"""
    rng = np.random.default_rng(seed)
    lens = [samples(f) + int(rng.integers(0, 160)) for f in EDGE_T]
    clips = [weights.burst_clips(1, n, seed=n + seed)[0] for n in lens]
    clips.insert(7, weights.burst_clips(1, 399, seed=3)[0])
    return clips


def dynamic_engine(w=None, **kw):
    return firered.FireRedEngine(w if w is not None else centred_weights((), BASE_SEED), None, long_windows=True, **kw)


@three_arithmetics
def test_dynamic_list_equals_each_clip_alone(gemm):
    eng, clips = dynamic_engine(), edge_clips()
    alone = [eng.run_packed(eng.pack([c]), return_logmel=True) for c in clips]
    rng = np.random.default_rng(11)
    for order in (np.arange(len(clips)), rng.permutation(len(clips))):
        pc = eng.pack([clips[i] for i in order])
        probs, logmel = eng.run_packed(pc, return_logmel=True)
        assert probs.shape == (1, pc.n_frames) and bool(torch.isfinite(probs).all())
        for k, i in enumerate(order):
            f0, f1 = int(pc.frame_first_host[k]), int(pc.frame_first_host[k + 1])
            assert f1 - f0 == firered.valid_frame_count(len(clips[i])) == alone[i][0].shape[1]
            assert torch.equal(logmel[f0:f1], alone[i][1]), (gemm, i)
            assert torch.equal(probs[:, f0:f1], alone[i][0]), (gemm, i)
    assert eng.blobs.range_fallbacks == 0 and eng.blobs.mode() == gemm
    # the dynamic window IS one window of that length: the static long engine at L = len(clip) gives the same probabilities
    i = EDGE_T.index(148)
    c = clips[i if i < 7 else i + 1]
    static = firered.FireRedEngine(centred_weights((), BASE_SEED), len(c), long_windows=True)
    assert torch.equal(static.run(T(c[None, :]).cuda(), 1)[0], eng.run_packed(eng.pack([c])))


@three_arithmetics
def test_static_long_grid_run_ragged_equals_each_clip_alone(gemm):
    """A RaggedBatch on a static long grid (L = 24 000 samples, 148 frames a window) through `run_ragged`: clip b's windows are those of
    `run` on its own padded row."""
    L = 24000
    eng = firered.FireRedEngine(centred_weights((), BASE_SEED), L, long_windows=True)
    clips = [weights.burst_clips(1, n, seed=n)[0] for n in (50000, 300, 24000, 24001, 71999)]
    noise = np.random.default_rng(2).standard_normal((len(clips), L))
    rb = eng.ragged(clips, noise)
    probs = eng.run_ragged(rb)
    assert probs.shape == (rb.n_windows, 1, 148)
    for b in range(len(clips)):
        row = T(rb.padded(b)[None, :]).cuda()
        assert torch.equal(probs[int(rb.win_first_host[b]):int(rb.win_first_host[b + 1])], eng.run(row, int(rb.windows[b]))), b


GUARD = 4096          # bytes of canary on either side of every buffer
CANARY = 0xA5


class Guarded:
    """`nbytes` device bytes between two canary zones, the buffer itself prefilled with `fill`"""

    def __init__(self, nbytes, fill=0x3C):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.raw[GUARD:GUARD + self.n] = fill
        self.ptr = self.raw.data_ptr() + GUARD

    def floats(self):
        return self.raw[GUARD:GUARD + self.n].view(torch.float32)

    def intact(self):
        return bool((self.raw[:GUARD] == CANARY).all()) and bool((self.raw[GUARD + self.n:] == CANARY).all())


def c_call(eng, pc, tables=None, lm=None, probs=None, ws=None, frontend=True, fe_tabs=None):
    """The two C entry points on PackedClips `pc` with buffers of exactly the required bytes inside canaries -> (logmel, probs, workspace)"""
    Lb, n = _lib.lib(), pc.n_frames
    cfg, blob = eng.blobs.get()
    lm = lm or Guarded(n * 80 * 4)
    probs = probs or Guarded(eng.odim * n * 4)
    need = Lb.vadx_firered_long_workspace_bytes(C.byref(cfg), n)
    assert need == 3 * eng._cfg0.P * n * 4
    ws = ws or Guarded(need)
    if frontend:
        ff, tf, tc = fe_tabs or (pc.frame_first, pc.tile_first, pc.tile_clip)
        _lib.check(Lb.vadx_frontend_logmel_ragged_snip(C.byref(eng.fe.cfg), eng.fe.packed.data_ptr(), eng.fe.mel_kb.ctypes.data, pc.pcm.data_ptr(),
                                                       int(pc.pcm.numel()), pc.clip_off.data_ptr(), pc.clip_len.data_ptr(), ff.data_ptr(),
                                                       tf.data_ptr(), tc.data_ptr(), len(pc), pc.n_tiles, n, lm.ptr, _lib.stream_ptr()))
    tabs = tables if tables is not None else pc.tables()
    _lib.check(Lb.vadx_firered_run_long(C.byref(cfg), blob.data_ptr(), lm.ptr, C.byref(tabs), probs.ptr, ws.ptr, ws.n, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert lm.intact() and probs.intact() and ws.intact()
    return lm, probs, ws


@three_arithmetics
def test_c_entry_points_inside_canaries(gemm):
    """Buffers of exactly the required bytes, canaries on both sides of the log-mel, the probabilities and the workspace: nothing outside is
    written, every float inside is, and the result is the engine's."""
    eng = dynamic_engine()
    eng.blobs.arithmetic = gemm
    pc = eng.pack(edge_clips())
    lm, probs, ws = c_call(eng, pc)
    want_p, want_lm = eng.run_packed(pc, return_logmel=True)
    assert torch.equal(lm.floats().view(-1, 80), want_lm) and torch.equal(probs.floats().view(1, -1), want_p)
    # workspace smaller by one byte: refused by name, nothing launched
    cfg, blob = eng.blobs.get()
    with pytest.raises(_lib.VadxError, match="workspace_bytes"):
        _lib.check(_lib.lib().vadx_firered_run_long(C.byref(cfg), blob.data_ptr(), lm.ptr, C.byref(pc.tables()), probs.ptr, ws.ptr, ws.n - 1,
                                                    _lib.stream_ptr()))


def test_planes_beyond_four_gib(gemm):
    """8 500 clips of 10 s generated on the device: every workspace plane is 128 x 8 483 000 floats = 4.3 GB, so a 32-bit offset wraps inside
    it.  The last three clips, which lie beyond 2^32 bytes in every plane, equal the one-clip call bit for bit."""
    n, clip = 8500, 160000
    eng = dynamic_engine()
    g = torch.Generator(device="cuda").manual_seed(17)
    base = (torch.randn((100, clip), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    base *= (torch.arange(clip, device="cuda") // 8000 % 3 != 0).to(torch.int16)[None, :]          # bursts: a third of every clip is silence
    pcm = base.repeat(n // 100, 1).reshape(-1)                                                        # 8 500 clips, 100 of them distinct
    del base
    pc = ragged.PackedClips.from_packed(pcm, np.arange(n, dtype=np.int64) * clip, np.full(n, clip, dtype=np.int64))
    assert pc.n_frames == n * 998 and eng.workspace_bytes(pc.n_frames) // 3 > 2 ** 32
    probs = eng.run_packed(pc)
    for b in (n - 3, n - 2, n - 1):
        one = eng.run_packed(ragged.PackedClips.from_packed(pcm, np.array([b * clip]), np.array([clip])))
        assert torch.equal(probs[:, b * 998:(b + 1) * 998], one), b
    assert float(probs[:, -998:].std()) > 0
    with pytest.raises(ValueError, match="workspace_cap"):
        dynamic_engine(workspace_cap=1 << 30).run_packed(pc)
    eng.release_workspace()


# ------------------------------------------------------------------ 4. lying tables
def lying_case(eng, pc, true, lie_clips, mutate):
    """Run with tables `mutate` has changed; the clips in `lie_clips` keep the sentinel in every row, all other clips are bitwise right."""
    ff, tf, tc = (pc.frame_first_host.copy(), pc.tile_first_host.copy(), pc.tile_clip_host.copy())
    own = mutate(ff, tf, tc)          # frame ranges [(f0, f1)] that must stay untouched (None: all frames of lie_clips)
    dev = [torch.from_numpy(a).cuda() for a in (ff, tf, tc)]
    tabs = _lib.FireRedLongTables(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), len(pc), pc.n_tiles, pc.n_frames)
    lm = Guarded(pc.n_frames * 80 * 4)
    lm.floats().copy_(true[0].floats())
    probs = Guarded(pc.n_frames * 4, fill=0x3C)
    sentinel = probs.floats().clone()
    _, probs, _ = c_call(eng, pc, tables=tabs, lm=lm, probs=probs, frontend=False)
    got, want = probs.floats(), true[1].floats()
    F = pc.frame_first_host
    for b in range(len(pc)):
        a, z = int(F[b]), int(F[b + 1])
        if b in lie_clips:
            for f0, f1 in (own or [(a, z)]):
                assert torch.equal(got[f0:f1], sentinel[f0:f1]), (b, f0, f1)
        else:
            assert torch.equal(got[a:z], want[a:z]), b


@three_arithmetics
def test_lying_tables_leave_their_rows_and_the_neighbours_alone(gemm):
    eng = dynamic_engine()
    eng.blobs.arithmetic = gemm
    frames = [70, 64, 64, 130, 20, 64]
    pc = eng.pack([weights.burst_clips(1, samples(f), seed=f + k)[0] for k, f in enumerate(frames)])
    true = c_call(eng, pc)
    F, TF = pc.frame_first_host, pc.tile_first_host

    def clip_below(ff, tf, tc):            # a clip outside [0, B): the first tile of clip 3
        tc[TF[3]] = -1
        return [(int(F[3]), int(F[3]) + 64)]

    def clip_above(ff, tf, tc):
        tc[TF[3] + 1] = len(frames)
        return [(int(F[3]) + 64, int(F[3]) + 128)]

    def tile_outside_its_clip(ff, tf, tc):  # clip 0's second tile claims clip 4, whose tiles lie elsewhere
        tc[TF[0] + 1] = 4
        return [(int(F[0]) + 64, int(F[1]))]

    def decreasing_prefix(ff, tf, tc):      # clip 1 ends before it starts; clip 2 (64 frames, one tile) then spans two tiles' worth
        ff[2] = ff[1] - 1

    def beyond_the_total(ff, tf, tc):
        ff[len(frames)] = pc.n_frames + 64

    def tile_count_disagrees(ff, tf, tc):   # clip 4 (20 frames) claims two tiles
        tf[5] += 1

    lying_case(eng, pc, true, {3}, clip_below)
    lying_case(eng, pc, true, {3}, clip_above)
    lying_case(eng, pc, true, {0}, tile_outside_its_clip)
    lying_case(eng, pc, true, {1, 2}, decreasing_prefix)
    lying_case(eng, pc, true, {5}, beyond_the_total)
    lying_case(eng, pc, true, {4, 5}, tile_count_disagrees)
    # the front-end's guard: a lying tile writes no log-mel row
    tc = pc.tile_clip_host.copy()
    tc[TF[3]] = -1
    lm = Guarded(pc.n_frames * 80 * 4)
    before = lm.floats().clone()
    Lb = _lib.lib()
    _lib.check(Lb.vadx_frontend_logmel_ragged_snip(C.byref(eng.fe.cfg), eng.fe.packed.data_ptr(), eng.fe.mel_kb.ctypes.data, pc.pcm.data_ptr(),
                                                   int(pc.pcm.numel()), pc.clip_off.data_ptr(), pc.clip_len.data_ptr(), pc.frame_first.data_ptr(),
                                                   pc.tile_first.data_ptr(), torch.from_numpy(tc).cuda().data_ptr(), len(pc), pc.n_tiles,
                                                   pc.n_frames, lm.ptr, _lib.stream_ptr()))
    torch.cuda.synchronize()
    a, z = int(F[3]) * 80, (int(F[3]) + 64) * 80
    got, want = lm.floats(), true[0].floats()
    assert lm.intact() and torch.equal(got[a:z], before[a:z]) and torch.equal(got[:a], want[:a]) and torch.equal(got[z:], want[z:])


# ------------------------------------------------------------------ 5. the range protocol
def test_range_protocol_on_the_long_path():
    """A log-mel of 1e6 leaves the fp16 range in the first split: the fp16 x 2 call raises the flag once and returns the bf16 x 3 result."""
    w, frames = centred_weights((), BASE_SEED), 200
    rng = np.random.default_rng(3)
    logmel = T((rng.standard_normal((2, frames, 80)) * 1e6).astype(np.float32)).cuda()
    eng = firered.FireRedEngine(w, samples(frames), long_windows=True)
    eng.blobs.arithmetic = "h2"
    other = firered.FireRedEngine(w, samples(frames), long_windows=True)
    other.blobs.arithmetic = "split"
    got, want = eng._run_logmel(logmel), other._run_logmel(logmel)
    assert eng.blobs.range_fallbacks == 1 and eng.blobs.mode() == "h2" and other.blobs.range_fallbacks == 0
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    quiet = T(rng.standard_normal((2, frames, 80)).astype(np.float32)).cuda()
    eng._run_logmel(quiet)
    assert eng.blobs.range_fallbacks == 1                    # the flag was cleared; an ordinary input does not raise it


# ------------------------------------------------------------------ 6. end to end
E2E_LENGTHS = [48000, 30123, 160000, 5000]
_E2E = {}


def gap_threshold(tracks, smooth, lo=0.2, hi=0.8):
    """The middle of the widest gap, inside (lo, hi), between the oracle scores of all clips, raw (the AED ratio counts them) and
    smoothed (the decisions compare them): no value within half that gap of the threshold, so the device's scores (within 1e-4) fall on
    the same side of it as the oracle's, frame by frame"""
    pp = opp.VadPostprocessor(smooth, 0.5, 20, 2000, 20, 5, 0)
    v = np.sort(np.concatenate([np.asarray(pp.smooth(np.asarray(t, dtype=np.float32)), dtype=np.float64) for t in tracks if len(t)] +
                               [np.asarray(t, dtype=np.float64) for t in tracks] + [[lo, hi]]))
    v = v[(v >= lo) & (v <= hi)]
    k = int(np.argmax(np.diff(v)))
    assert v[k + 1] - v[k] > 20 * ATOL, "no score gap to put a threshold in"
    return float(np.float32((v[k] + v[k + 1]) / 2))


def e2e(odim):
    if odim not in _E2E:
        cfg = dict(weights.FIRERED_CFG, odim=odim)
        clips = [weights.burst_clips(1, n, seed=n)[0] for n in E2E_LENGTHS]
        fe = ofr.Frontend()
        feats = [ofr.log_mel(fe, torch.from_numpy(clips[0].copy()).reshape(1, 1, -1)).numpy()]
        from test_gpu_firered_shapes import recentred
        w = recentred(weights.firered_synthetic(BASE_SEED, cfg), feats, None)
        ow = {k: (T(v) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
        if odim == 1:
            tracks = [ofr.run_clip(fe, ow, c, None, window=len(c))[1] for c in clips]
            thr = [gap_threshold(tracks, 5)]
        else:
            allp = [ofr.run_clip_aed(fe, ow, c, None, window=len(c))[2] for c in clips]
            thr = [gap_threshold([p[k] for p in allp], 5) for k in range(3)]
        _E2E[odim] = (w, ow, fe, clips, thr)
    return _E2E[odim]


@three_arithmetics
def test_detect_on_a_dynamic_engine_against_the_oracle(gemm, tmp_path):
    w, ow, fe, clips, (thr,) = e2e(1)
    post = (5, thr, 20, 2000, 20, 5, 0)
    want = [ofr.run_clip(fe, ow, c, None, window=len(c), post=post) for c in clips]
    assert any(len(s) for s, _, _ in want)
    eng = dynamic_engine(w)
    got, tracks, decs = eng.detect(clips, post=post, return_probs=True)
    for b, (seg, p, dec) in enumerate(want):
        np.testing.assert_allclose(tracks[b].cpu().numpy(), p, rtol=0, atol=ATOL)
        assert np.array_equal(decs[b].cpu().numpy(), dec) and got[b] == seg, b
    assert eng.detect(clips, post=post) == got and eng.detect_table(clips, post=post).lists() == got
    assert eng.detect(clips[1][None, :], post=post) == [got[1]]                       # an array [1, N]: one clip of that length
    # the drivers on wav files: a list is one packed batch, a single file a [1, N] array
    files = []
    for k, c in enumerate(clips):
        files.append(str(tmp_path / f"c{k}.wav"))
        with wave.open(files[-1], "wb") as fh:
            fh.setnchannels(1), fh.setsampwidth(2), fh.setframerate(16000), fh.writeframes(c.tobytes())
    kw = dict(engine=eng, SPEAKING_SCORE=thr, echo=lambda *_: None, save_timestamps_second=str(tmp_path / "s.txt"),
              save_timestamps_indices=str(tmp_path / "i.txt"))
    assert drivers.inference_firered(files, **kw) == got
    assert drivers.inference_firered(files[0], **kw) == got[0]
    assert drivers.inference_firered(files, device_ingest=True, **kw) == got
    # collect_chunks_batch -> from_packed -> detect equals the host route over the same chunks
    src = eng.pack(clips)
    table = eng.detect_table(src, post=post)
    pcm, offs = chunks.collect_chunks_batch(table.chunks_table(), src.pcm, lengths=src.clip_len, clip_offsets=src.clip_off)
    offs = offs.cpu().numpy()
    keep = [(int(offs[b]), int(offs[b + 1] - offs[b])) for b in range(len(clips)) if offs[b + 1] > offs[b]]
    assert keep and sum(n for _, n in keep) == pcm.numel()
    host = [pcm[o:o + n].cpu().numpy() for o, n in keep]
    pc = eng.ragged_packed(pcm, np.array([o for o, _ in keep]), np.array([n for _, n in keep]))
    assert pc.pcm.data_ptr() == pcm.data_ptr()                                        # tables only: the speech is not copied
    assert eng.detect(pc, post=post) == eng.detect(host, post=post)


@three_arithmetics
def test_detect_events_on_a_dynamic_engine_against_the_oracle(gemm, tmp_path):
    w, ow, fe, clips, thr = e2e(3)
    post = (5, 20, 2000, 20, 5, 0)
    want = [ofr.run_clip_aed(fe, ow, c, None, window=len(c), thresholds=thr, post=post) for c in clips]
    eng = dynamic_engine(w)
    got, tracks = eng.detect_events(clips, thresholds=thr, post=post, return_probs=True)
    for b, (ts, ratio, allp) in enumerate(want):
        np.testing.assert_allclose(tracks[b].cpu().numpy(), allp, rtol=0, atol=ATOL)
        assert got[b][0] == ts and got[b][1] == ratio, b
    assert eng.detect_events(np.stack([clips[0], clips[0]]), thresholds=thr, post=post) == [got[0], got[0]]
    files = []
    for k, c in enumerate(clips):
        files.append(str(tmp_path / f"c{k}.wav"))
        with wave.open(files[-1], "wb") as fh:
            fh.setnchannels(1), fh.setsampwidth(2), fh.setframerate(16000), fh.writeframes(c.tobytes())
    kw = dict(engine=eng, SPEAKING_SCORE=thr[0], SINGING_THRESHOLD=thr[1], MUSIC_THRESHOLD=thr[2], echo=lambda *_: None)
    assert drivers.inference_firered_aed(files, **kw) == got
    assert drivers.inference_firered_aed(files[2], **kw) == got[2]


def test_session_reports_the_dynamic_shapes():
    w = centred_weights((), BASE_SEED)
    sess = firered.FireRedSession(w, None, long_windows=True)
    assert sess.get_inputs()[0].shape == [1, 1, "audio_len"] and sess.get_outputs()[0].shape == [1, 1, "n_frames"]
    eng = sess.engine
    for n in (400, 16000, 18320, 50001):
        clip = weights.burst_clips(1, n, seed=n)
        out, = sess.run(None, {"audio": clip.reshape(1, 1, n)})
        assert out.shape == (1, 1, firered.valid_frame_count(n))
        assert np.array_equal(out[0], eng.run_packed(eng.pack([clip[0]])).cpu().numpy())
    with pytest.raises(ValueError, match="audio"):
        sess.run(None, {"audio": np.zeros((1, 1, 399), np.int16)})
    static = firered.FireRedSession(w, 18320, long_windows=True)                      # T = 113: a static long export
    assert static.get_inputs()[0].shape == [1, 1, 18320] and static.get_outputs()[0].shape == [1, 1, 113]
    clip = weights.burst_clips(1, 18320, seed=1)
    assert np.array_equal(static.run(None, {"audio": clip.reshape(1, 1, -1)})[0][0], eng.run_packed(eng.pack([clip[0]])).cpu().numpy())


def test_one_hour_in_one_window_static_and_dynamic():
    """3600 s, the reference driver's cap (359 998 frames, 5 625 tiles): the rectangular front-end takes it as one window, and the static
    long engine at that length returns the dynamic engine's bytes."""
    n = 3600 * 16000
    g = torch.Generator(device="cuda").manual_seed(23)
    pcm = (torch.randn((n,), generator=g, device="cuda") * 3000).clamp_(-32768, 32767).to(torch.int16)
    pcm *= (torch.arange(n, device="cuda") // 8000 % 3 != 0).to(torch.int16)
    w = centred_weights((), BASE_SEED)
    static, dyn = firered.FireRedEngine(w, n, long_windows=True), dynamic_engine(w)
    assert static.T == 359998 <= firered.LONG_MAX_FRAMES
    a = static.run(pcm[None, :], 1)
    b = dyn.run_packed(ragged.PackedClips.from_packed(pcm, np.array([0]), np.array([n])))
    assert a.shape == (1, 1, 359998) and torch.equal(a[0], b) and bool(torch.isfinite(a).all()) and float(a.std()) > 0
    assert static.blobs.range_fallbacks == dyn.blobs.range_fallbacks == 0
