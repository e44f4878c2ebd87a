"""GPU: the FSMN stream path (vadx.fsmn.FsmnStreamBatch over vadx_fsmn_stream_windows / vadx_fsmn_stream_run) against the whole-clip path
(FsmnEngine.flags, bit for bit), the chained boundary calls (FsmnEngine.run, caches bit for bit) and the CPU oracle's restatement of the
reference loop.  S = 3 streams x 4 windows (3 at look_backward = 0): T = 101 frames per window already takes the 64 + 48-frame tile split,
and nothing depends on S beyond one workgroup per stream."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, fsmn, weights
from oracle import fsmn as ofs
from oracle import postproc as opp

pytestmark = pytest.mark.gpu
S, N, L, SEED = 3, 45000, 16000, 1234


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


def audio(lb_s):
    """(clips int16 [S, N] peak-normalised, explicit padding noise [S, 20000], padded [S, (W-1)*stride + L], W)"""
    if ("audio", lb_s) not in _CACHE:
        lb, stride = engine().grid(lb_s)
        clips = weights.burst_clips(S, N, seed=SEED + N)
        noise = np.random.default_rng(9).standard_normal((S, 20000))
        norm = [opp.normalize_to_int16(clips[b].astype(np.float32)) for b in range(S)]
        padded = np.stack([fsmn.pad_to_window_grid(norm[b], L, stride, noise[b]) for b in range(S)])
        W = (padded.shape[1] - L) // stride + 1
        assert W == (4 if lb else 3) and padded.shape[1] == (49120 if lb else 47680)
        _CACHE["audio", lb_s] = (norm, noise, padded, W)
    return _CACHE["audio", lb_s]


def reference(gemm, lb_s):
    """FsmnEngine.flags over the whole padded clips, once per (arithmetic, look-back): (flags u8 [S, W*slide + lb], noise trace f32 [S, W])"""
    if ("ref", gemm, lb_s) not in _CACHE:
        _, _, padded, W = audio(lb_s)
        flags, trace = engine().flags(T(padded), W, look_backward_s=lb_s, return_noise=True)
        assert engine().blobs.mode() == gemm
        _CACHE["ref", gemm, lb_s] = (flags.clone(), trace.clone())
    return _CACHE["ref", gemm, lb_s]


def feed(it, rows, pos, k, reset=None, active=None, extra=0):
    """One tick: every active stream s gets its next samples_needed samples of rows[s] from pos[s] on (rows of inactive streams stay zero)."""
    need = it.samples_needed(k, reset)
    act = np.ones(it.streams, bool) if active is None else np.asarray(active, bool)
    x = np.zeros((it.streams, int(need[act].max()) + extra), np.int16)
    for s in range(it.streams):
        if act[s]:
            x[s, :need[s]] = rows[s][pos[s]:pos[s] + need[s]]
            pos[s] += int(need[s])
    return it.step(x, k, reset=reset, active=active)


@pytest.mark.parametrize("lb_s,sched", [(0.3, (1, 1, 1, 1)), (0.3, (2, 1, 1)), (0.3, (4,)), (0.0, (1, 1, 1)), (0.0, (2, 1)), (0.0, (3,))])
def test_ticks_are_bitwise_flags(gemm, lb_s, sched):
    """Any tick schedule over the same audio: concatenated flags + the last tick's tail == flags(); noise floor after every window ==
    flags(return_noise=True)'s trace; the caches in the record's documented prefix == those after W chained run() calls.  All bitwise."""
    eng = engine()
    _, _, padded, W = audio(lb_s)
    want, want_trace = reference(gemm, lb_s)
    fallbacks = eng.blobs.range_fallbacks
    it = fsmn.FsmnStreamBatch(eng, S, look_backward_s=lb_s)
    lb, stride = eng.grid(lb_s)
    assert (it.lb, it.stride, it.carry) == (lb, stride, (lb + 1) * 160) and sum(sched) == W
    pos, got, traces = [0] * S, [], []
    for k in sched:
        flags, tail = feed(it, padded, pos, k, extra=3 if sched[0] == 2 else 0)      # odd row lengths take the 16-byte staging copy
        assert flags.shape == (S, k * (eng.T - lb)) and tail.shape == (S, lb) and flags.dtype == tail.dtype == torch.uint8
        got.append(flags)
        traces.append(it.noise_trace)
    assert pos == [padded.shape[1]] * S
    assert torch.equal(torch.cat(got + [tail], dim=1), want)
    assert torch.equal(torch.cat(traces, dim=1), want_trace)
    assert np.array_equal(it.windows_done, np.full(S, W))
    # the four FIR caches: W chained boundary calls, the noise floor fed back from the trace as the reference loop feeds it
    caches = [torch.zeros(S, 128, 19) for _ in range(4)]
    noise_in = torch.full((S,), float(np.float32(30.0 + 10.0) * np.float32(0.1)))
    for j in range(W):
        _, caches, _ = eng.run(T(padded[:, j * stride:j * stride + L]), caches, np.ones(S, np.float32), noise_in)
        noise_in = want_trace[:, j]
    for l in range(4):
        assert torch.equal(it.caches[:, l], caches[l]), l
    assert eng.blobs.range_fallbacks == fallbacks and eng.blobs.mode() == gemm        # the equality is not a fallback's


def test_one_stream_against_the_oracle(gemm):
    """One stream against oracle.fsmn.run_clip on the same clip and padding
    noise: every flag of the `saved` list, no excused frames, and the same (start, end) pairs."""
    eng = engine()
    norm, noise, padded, W = audio(0.3)
    if "oracle" not in _CACHE:
        ow = {k: T(v) for k, v in weights.fsmn_synthetic(SEED).items()}
        _CACHE["oracle"] = ofs.run_clip(ofs.Frontend(), ow, norm[0], noise[0])
    want_ts, want_flags = _CACHE["oracle"]
    it = fsmn.FsmnStreamBatch(eng, 1)
    pos, got = [0], []
    for k in (1, 2, 1):
        flags, tail = feed(it, padded[:1], pos, k)
        got.append(flags[0])
    saved = torch.cat(got)
    full = torch.cat([saved, tail[0]]).cpu().numpy().astype(bool)
    assert full.shape[0] == len(want_flags) and np.array_equal(full, np.array(want_flags, bool))
    assert it.timestamps(saved, tail[0]) == want_ts
    assert eng.blobs.mode() == gemm


def test_reset_inactive_and_staggered_streams(gemm):
    eng = engine()
    _, _, padded, W = audio(0.3)
    want, _ = reference(gemm, 0.3)
    lb, stride = eng.grid(0.3)
    slide = eng.T - lb
    refw = want[:, :W * slide].reshape(S, W, slide)              # voted flags per window
    ref_tail = want[:, W * slide:]
    it = fsmn.FsmnStreamBatch(eng, S)
    first = lambda k: L + (k - 1) * stride                        # noqa: E731
    for k in (1, 2, 3):
        assert np.array_equal(it.samples_needed(k), np.full(S, first(k)))
    rows, pos = [padded[0], padded[1], padded[2]], [0, 0, 0]
    # tick 1: everyone's first window
    flags, _ = feed(it, rows, pos, 1)
    assert torch.equal(flags, refw[:, 0])
    for k in (1, 2, 3):
        assert np.array_equal(it.samples_needed(k), np.full(S, k * stride))
        assert np.array_equal(it.samples_needed(k, reset=[False, True, False]), [k * stride, first(k), k * stride])
    # tick 2: stream 1 is reset and from here on hears clip 0 from its start; stream 2 has no audio
    rows[1], pos[1] = padded[0], 0
    before = it.record.clone()
    flags, tail = feed(it, rows, pos, 1, reset=[False, True, False], active=[True, True, False])
    assert torch.equal(flags[0], refw[0, 1]) and torch.equal(flags[1], refw[0, 0])
    assert bool((flags[2] == 255).all()) and bool((tail[2] == 255).all()) and bool(torch.isnan(it.noise_trace[2]).all())
    assert torch.equal(it.stream_bytes(it.record, 2), it.stream_bytes(before, 2))
    assert not torch.equal(it.stream_bytes(it.record, 0), it.stream_bytes(before, 0))
    # tick 3: everyone; stream 2 never saw the gap
    flags, _ = feed(it, rows, pos, 1)
    assert torch.equal(flags[0], refw[0, 2]) and torch.equal(flags[1], refw[0, 1]) and torch.equal(flags[2], refw[2, 1])
    # tick 4: a reset request on the inactive stream 2 is ignored
    before = it.record.clone()
    flags, tail = feed(it, rows, pos, 1, reset=[False, False, True], active=[True, True, False])
    assert torch.equal(flags[0], refw[0, 3]) and torch.equal(tail[0], ref_tail[0]) and torch.equal(flags[1], refw[0, 2])
    assert bool((flags[2] == 255).all()) and bool((tail[2] == 255).all())
    assert torch.equal(it.stream_bytes(it.record, 2), it.stream_bytes(before, 2))
    assert np.array_equal(it.samples_needed(1), np.full(S, stride))
    # tick 5: stream 0 is through; stream 1 ends clip 0, stream 2 goes on where it was
    flags, tail = feed(it, rows, pos, 1, active=[False, True, True])
    assert torch.equal(flags[1], refw[0, 3]) and torch.equal(tail[1], ref_tail[0]) and torch.equal(flags[2], refw[2, 2])
    assert np.array_equal(it.windows_done, [4, 4, 3])
    it.reset_states([1])
    assert np.array_equal(it.samples_needed(2), [2 * stride, first(2), 2 * stride])
    assert eng.blobs.mode() == gemm


def test_state_in_is_read_only_and_a_tick_can_be_recomputed(gemm):
    eng = engine()
    _, _, padded, _ = audio(0.3)
    it = fsmn.FsmnStreamBatch(eng, S)
    pos = [0] * S
    feed(it, padded, pos, 2)
    src = it.record                                              # the tensor the next tick reads
    before = src.clone()
    pos2 = list(pos)
    flags, tail = feed(it, padded, pos, 1)
    assert it.record is not src and torch.equal(src, before)     # byte for byte untouched
    again = fsmn.FsmnStreamBatch(eng, S)
    again.load_record(before)
    flags2, tail2 = feed(again, padded, pos2, 1)
    assert torch.equal(flags, flags2) and torch.equal(tail, tail2) and torch.equal(it.noise_trace, again.noise_trace)
    assert torch.equal(it.record, again.record)


def test_range_protocol_per_tick(gemm):
    """fp16 x 2 only.  Recipe: one primed stream's whole layer-0 FIR cache (the record's documented prefix) is set to 3e5.  The FIR + skip of
    layer 0 then puts 3e5 * (sum of a channel's taps) on the activation that tile_split splits next (`SC::split4(o[t], pp, amax)`), beyond
    65504 for every channel whose taps sum to more than 0.22 in magnitude -- most of the synthetic checkpoint's 128.  The tick must count one
    fallback and leave the flags, tail and record of the same tick on an engine pinned to bf16 x 3."""
    if gemm != "h2":
        pytest.skip("the range protocol belongs to fp16 x 2")
    eng = engine()
    if "eng_split" not in _CACHE:
        _CACHE["eng_split"] = fsmn.FsmnEngine(weights.fsmn_synthetic(SEED))
        _CACHE["eng_split"].blobs.arithmetic = "split"
    eng_s = _CACHE["eng_split"]
    _, _, padded, _ = audio(0.3)
    it = fsmn.FsmnStreamBatch(eng, S)
    pos = [0] * S
    feed(it, padded, pos, 1)
    it.caches[1, 0].fill_(3e5)
    other = fsmn.FsmnStreamBatch(eng_s, S)
    other.load_record(it.record)
    pos_s = list(pos)
    fallbacks = eng.blobs.range_fallbacks
    flags, tail = feed(it, padded, pos, 1)
    assert eng.blobs.range_fallbacks == fallbacks + 1 and eng.blobs.mode() == "h2"
    flags_s, tail_s = feed(other, padded, pos_s, 1)
    assert eng_s.blobs.mode() == "split" and eng_s.blobs.range_fallbacks == 0
    assert torch.equal(flags, flags_s) and torch.equal(tail, tail_s) and torch.equal(it.record, other.record)
    # the next tick is an ordinary one again
    feed(it, padded, pos, 1)
    assert eng.blobs.range_fallbacks == fallbacks + 1


def test_bad_arguments(gemm):
    if gemm != "h2":
        pytest.skip("independent of the dense-layer arithmetic")
    eng = engine()
    it = fsmn.FsmnStreamBatch(eng, S)
    x = np.zeros((S, L), np.int16)
    with pytest.raises(ValueError, match="int16"):
        it.step(x.astype(np.float32))
    with pytest.raises(ValueError, match="samples_needed"):
        it.step(x[:, :L - 1])
    with pytest.raises(ValueError, match="samples_needed"):
        it.step(x, 2)
    with pytest.raises(ValueError, match="windows"):
        it.step(x, 0)
    with pytest.raises(ValueError, match="windows"):
        it.samples_needed(0)
    with pytest.raises(ValueError, match="active"):
        it.step(x, active=[True, False])
    with pytest.raises(ValueError, match="reset"):
        it.step(x, reset=np.zeros(S + 1, bool))
    with pytest.raises(ValueError):
        it.step(x[:2])
    with pytest.raises(ValueError):
        fsmn.FsmnStreamBatch(eng, 0)
    assert np.array_equal(it.windows_done, np.zeros(S)) and not bool(it.record.any())      # nothing ran
