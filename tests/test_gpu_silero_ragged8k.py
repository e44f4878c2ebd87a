"""Silero's ragged batch on the 8 kHz network (csrc/silero8k.hip: silero8k_encode_kernel<Sch, SampleT, true>; the _8k entry points of
include/vadx.h) and ragged batches above the workspace cap, run as parts of consecutive groups at either rate.
The yardstick throughout is the existing code: engine.clips(clip[None], return_state=True, sampling_rate=rate) on one clip alone, in the
same arithmetic -- every comparison is torch.equal, bit for bit, on float32 / bf16 x 3 / fp16 x 2 (a tile's numbers do not depend on the
workgroup that computes it, and the columns of an MFMA are independent: no tolerance anywhere).

The 37 clips (tests/test_silero_ragged8k_cpu.py: LENGTHS8K_37): group 0 mixes T_b = 33, 32, 31, 17, 16, 15, 9, 8, 5, 4, 3, 2, 2, 2, 2, 1
(lengths 256 k - 50 / 256 k / 256 k + 1 in turn and 257, 287, 288, 289, 255 around the reflect pad and the window edge), group 1 is
sixteen clips of one window (1, 3, 4, 31, 32, 33, 255, 206, 256 samples: around the vector-load minimum and the 32-sample context),
group 2 the last five (partial)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, audio_io, drivers, ragged, silero, weights
from test_silero_ragged8k_cpu import LENGTHS8K_37

pytestmark = pytest.mark.gpu
MODES = ["f32", "split", "h2"]
SCALE = np.float32(0.000030517578)
WIN = 256
TILE = 32768


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234), weights_8k=weights.silero8k_synthetic(1234))


@pytest.fixture(scope="module")
def pcm37():
    """int16 burst clips cut to LENGTHS8K_37"""
    full = weights.burst_clips(37, 33 * WIN, seed=91, sample_rate=8000)
    return [np.ascontiguousarray(full[b, :n]) for b, n in enumerate(LENGTHS8K_37)]


@pytest.fixture(scope="module")
def clips37(pcm37):
    return [c.astype(np.float32) * SCALE for c in pcm37]


def alone(engine, clip, mode, rate=8000):
    """(probs [T], state [2, 128]) of one clip through the rectangular path, in `mode`"""
    engine.arithmetic = mode
    p, s = engine.clips(torch.from_numpy(np.ascontiguousarray(clip))[None].cuda(), return_state=True, sampling_rate=rate)
    return p[0].clone(), s[:, 0].clone()


def reference_of(engine, clips, rate):
    """per arithmetic, per clip: the rectangular path on that clip alone -- computed once, asserted finite, never changed"""
    ref = {}
    for mode in MODES:
        before = engine.range_fallbacks
        ref[mode] = [alone(engine, c, mode, rate) for c in clips]
        assert engine.range_fallbacks == before
        for p, s in ref[mode]:
            assert torch.isfinite(p).all() and torch.isfinite(s).all()
    engine.arithmetic = None
    return ref


@pytest.fixture(scope="module")
def reference(engine, clips37):
    return reference_of(engine, clips37, 8000)


def run(engine, batch, mode, **kw):
    engine.arithmetic = mode
    before = engine.range_fallbacks
    out = engine.clips_ragged(batch, return_state=True, **kw)
    assert engine.range_fallbacks == before
    return out


def assert_rows(probs, first, state, ref, order=None, skip=()):
    first = first.cpu().tolist()
    for k in range(len(first) - 1):
        if k in skip:
            continue
        p, s = ref[k if order is None else order[k]]
        assert first[k + 1] - first[k] == p.shape[0]
        assert torch.equal(probs[first[k]:first[k + 1]], p), k
        if state is not None:
            assert torch.equal(state[:, k], s), k


# ---- 1. per clip, bit for bit, scores and state
@pytest.mark.parametrize("mode", MODES)
def test_every_clip_equals_the_clip_alone(engine, clips37, reference, mode):
    batch = ragged.RaggedClips.from_clips(clips37, sampling_rate=8000)
    assert batch.group_windows.tolist() == [33, 1, 1] and batch.tiles == 35 and batch.window == WIN
    probs, first, state = run(engine, batch, mode)
    assert probs.shape == (sum((n + WIN - 1) // WIN for n in LENGTHS8K_37),) and state.shape == (2, 37, 128)
    assert_rows(probs, first, state, reference[mode])
    batch.check()
    # the list form, and the rate a RaggedClips carries against an explicit one
    probs2, first2, state2 = run(engine, clips37, mode, sampling_rate=8000)
    assert torch.equal(probs2, probs) and torch.equal(first2, first) and torch.equal(state2, state)
    with pytest.raises(ValueError, match="8000"):
        engine.clips_ragged(batch, sampling_rate=16000)
    with pytest.raises(ValueError, match="44100"):
        engine.clips_ragged(clips37, sampling_rate=44100)


# ---- 2. neighbours and order
@pytest.mark.parametrize("mode", MODES)
def test_order_and_neighbours_do_not_matter(engine, clips37, reference, mode):
    perm = np.random.default_rng(5).permutation(37).tolist()
    probs, first, state = run(engine, [clips37[k] for k in perm], mode, sampling_rate=8000)
    assert_rows(probs, first, state, reference[mode], order=perm)
    for k in (0, 3, 4, 5, 15, 20):                     # T_b = 33, 17, 16, 15, 1, 1: the group's own T_g at the flush block's edges
        probs, first, state = run(engine, [clips37[k]], mode, sampling_rate=8000)
        assert_rows(probs, first, state, [reference[mode][k]])
    sub = [2, 3, 4, 7, 11, 30]                         # a partial group alone
    probs, first, state = run(engine, [clips37[k] for k in sub], mode, sampling_rate=8000)
    assert_rows(probs, first, state, reference[mode], order=sub)


# ---- 3. source forms
@pytest.mark.parametrize("mode", MODES)
def test_int16_source_equals_the_scaled_float32(engine, pcm37, reference, mode):
    for c16, c32 in zip(pcm37[:3], [c.astype(np.float32) * SCALE for c in pcm37[:3]]):
        assert np.array_equal(torch.from_numpy(c16).float().numpy() * np.float32(engine.PCM16_SCALE), c32)
    probs, first, state = run(engine, pcm37, mode, sampling_rate=8000)
    assert_rows(probs, first, state, reference[mode])


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("mode", MODES)
def test_any_element_residue_equals_the_aligned_clip(engine, pcm37, clips37, reference, mode, dtype):
    """two clips (T_b = 5 and one of 33 samples), each starting at element residues 0 ... 7 of the packed vector"""
    src = pcm37 if dtype == "int16" else clips37
    ids = [8, 21]
    assert LENGTHS8K_37[8] == 256 * 4 + 1 and LENGTHS8K_37[21] == 33
    offs, lens, which, pos = [], [], [], 0
    for r in range(8):
        for k in ids:
            pos = (pos + 7) // 8 * 8 + r
            offs.append(pos)
            lens.append(len(src[k]))
            which.append(k)
            pos += len(src[k])
    vec = np.zeros(pos + 3, dtype=src[0].dtype)
    for o, k in zip(offs, which):
        vec[o:o + len(src[k])] = src[k]
    assert sorted(set(o % 8 for o in offs)) == list(range(8))
    batch = ragged.RaggedClips.from_packed(torch.from_numpy(vec).cuda(), offs, lens, sampling_rate=8000)
    probs, first, state = run(engine, batch, mode)
    assert_rows(probs, first, state, reference[mode], order=which)
    batch.check()


# ---- 4. canary guards, through the C entry point
@pytest.mark.parametrize("mode", MODES)
def test_nothing_is_written_outside_scores_and_workspace(engine, clips37, reference, mode):
    batch = ragged.RaggedClips.from_clips(clips37, sampling_rate=8000)
    engine.arithmetic = mode
    L, G = _lib.lib(), 4096
    need = L.vadx_silero_ragged_workspace_bytes(batch.tiles)
    assert need == batch.workspace_bytes == 35 * TILE
    ws = torch.full((need + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    pr = torch.full((batch.n_windows + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((2 * 37 * 128 + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
    tab = batch.tables()
    engine.range_flag(sampling_rate=8000)
    _lib.check(L.vadx_silero_clips_ragged_8k(engine.packed_8k.data_ptr(), batch.pcm.data_ptr(), 0, 1.0, batch.pcm.numel(), tab,
                                             pr.data_ptr() + 4 * G, st.data_ptr() + 4 * G, ws.data_ptr() + G, need, _lib.stream_ptr(),
                                             engine.cfg(mode, 8000)))
    torch.cuda.synchronize()
    assert (ws[:G] == 0x5A).all() and (ws[G + need:] == 0x5A).all()
    assert (pr[:G] == -7.0).all() and (pr[G + batch.n_windows:] == -7.0).all()
    assert (st[:G] == -7.0).all() and (st[G + 2 * 37 * 128:] == -7.0).all()
    body = pr[G:G + batch.n_windows]
    assert (body != -7.0).all()                                           # every score entry is written
    assert_rows(body, batch.probs_first, st[G:G + 2 * 37 * 128].view(2, 37, 128), reference[mode])
    assert engine.range_flag(sampling_rate=8000)[0] == 0
    # a workspace one byte short is refused, by name
    rc = L.vadx_silero_clips_ragged_8k(engine.packed_8k.data_ptr(), batch.pcm.data_ptr(), 0, 1.0, batch.pcm.numel(), tab,
                                       pr.data_ptr() + 4 * G, None, ws.data_ptr() + G, need - 1, _lib.stream_ptr(), engine.cfg(mode, 8000))
    assert rc == -2 and b"workspace" in L.vadx_last_error() and b"vadx_silero_clips_ragged_8k" in L.vadx_last_error()


# ---- 5. lying tables: the device refuses a slot before indexing through it
@pytest.mark.parametrize("lie", ["offset past the end", "negative offset", "length past the end", "huge offset"])
@pytest.mark.parametrize("mode", MODES)
def test_a_slot_outside_the_source_is_refused_on_the_device(engine, clips37, reference, mode, lie):
    batch = ragged.RaggedClips.from_clips(clips37, sampling_rate=8000)
    n_src = int(batch.pcm.numel())
    slot = 3                                                              # clip 3 (T_b = 17) in the mixed group
    assert batch.slot_clip_host[slot] == 3
    n = int(batch.slot_len_host[slot])
    if lie == "offset past the end":
        batch.slot_off[slot] = n_src - n + 1                              # the last sample would be element n_src
    elif lie == "negative offset":
        batch.slot_off[slot] = -8
    elif lie == "huge offset":
        batch.slot_off[slot] = 2 ** 62
    else:
        batch.slot_len[slot] = n_src + 1
    probs, first, state = run(engine, batch, mode)
    f = first.cpu().tolist()
    assert torch.isnan(probs[f[3]:f[4]]).all() and f[4] - f[3] == 17
    assert int(batch.status.item()) & 1
    assert_rows(probs, first, state, reference[mode], skip={3})
    with pytest.raises(ValueError, match="outside the packed vector"):
        batch.check()


# ---- 6. range protocol (fp16 x 2 is the arithmetic that has one)
def test_range_protocol(engine, clips37, reference):
    loud = [c.copy() for c in clips37]
    assert LENGTHS8K_37[3] == 17 * WIN - 50
    loud[3][16 * WIN:] *= np.float32(1.0e6)                               # clip 3's last window, far outside +-1 (and the fp16 range)
    engine.range_flag(sampling_rate=8000)
    # unchecked: the halves on fp16 x 2
    batch = ragged.RaggedClips.from_clips(loud, sampling_rate=8000)
    engine.encode_ragged(batch, mode="h2")
    state = torch.empty((2, 37, 128), dtype=torch.float32, device="cuda")
    probs = engine.recur_ragged(batch, state_n=state, mode="h2")
    flag, amax = engine.range_flag(sampling_rate=8000)
    assert flag == 1 and amax > 65504.0
    f = batch.probs_first_host.tolist()
    ref = reference["h2"]
    for k in range(37):
        row, (p, s) = probs[f[k]:f[k + 1]], ref[k]
        if k < 16 and row.shape[0] > 16:                                  # group 0, still running at window 16: NaN from there on
            assert torch.equal(row[:16], p[:16]) and torch.isnan(row[16:]).all(), k
        else:                                                             # ended before it, or another group: untouched
            assert torch.equal(row, p) and torch.equal(state[:, k], s), k
    # guarded: the batch is recomputed on bf16 x 3
    engine.arithmetic = "split"
    want = engine.clips_ragged(loud, return_state=True, sampling_rate=8000)
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[2]).all()
    engine.arithmetic = "h2"
    before = engine.range_fallbacks
    got = engine.clips_ragged(loud, return_state=True, sampling_rate=8000)
    assert engine.range_fallbacks == before + 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert engine.range_flag(sampling_rate=8000)[0] == 0


# ---- 7. the wrong blob, the wrong cfg
@pytest.mark.parametrize("mode", MODES)
def test_a_16_khz_blob_gives_nan_and_the_flag_bit(engine, clips37, mode):
    batch = ragged.RaggedClips.from_clips(clips37[:5], sampling_rate=8000)
    L = _lib.lib()
    ws = torch.zeros(batch.workspace_bytes, dtype=torch.uint8, device="cuda")
    pr = torch.zeros(batch.n_windows, dtype=torch.float32, device="cuda")
    engine.range_flag()
    _lib.check(L.vadx_silero_clips_ragged_8k(engine.packed.data_ptr(), batch.pcm.data_ptr(), 0, 1.0, batch.pcm.numel(), batch.tables(),
                                             pr.data_ptr(), None, ws.data_ptr(), ws.numel(), _lib.stream_ptr(), engine.cfg(mode, 8000)))
    torch.cuda.synchronize()
    assert torch.isnan(pr).all()
    assert engine.range_flag()[0] & 4


def test_the_8k_calls_refuse_another_rate_by_name(engine, clips37):
    batch = ragged.RaggedClips.from_clips(clips37[:5], sampling_rate=8000)
    L = _lib.lib()
    ws = torch.zeros(batch.workspace_bytes, dtype=torch.uint8, device="cuda")
    pr = torch.zeros(batch.n_windows, dtype=torch.float32, device="cuda")
    blob, src, n, tab, st = engine.packed_8k.data_ptr(), batch.pcm.data_ptr(), batch.pcm.numel(), batch.tables(), _lib.stream_ptr()
    pcm16 = torch.zeros(n, dtype=torch.int16, device="cuda")
    for rate in (16000, 0):
        cfg = _lib.SileroCfg()
        cfg.sample_rate = rate
        c = ctypes.byref(cfg)
        calls = {
            "vadx_silero_encode_ragged_8k": lambda: L.vadx_silero_encode_ragged_8k(blob, src, n, tab, ws.data_ptr(), ws.numel(), st, c),
            "vadx_silero_encode_ragged_8k_pcm16": lambda: L.vadx_silero_encode_ragged_8k_pcm16(blob, pcm16.data_ptr(), 1.0, n, tab, ws.data_ptr(),
                                                                                               ws.numel(), st, c),
            "vadx_silero_recur_ragged_8k": lambda: L.vadx_silero_recur_ragged_8k(blob, ws.data_ptr(), ws.numel(), n, tab, pr.data_ptr(), None, st, c),
            "vadx_silero_clips_ragged_8k": lambda: L.vadx_silero_clips_ragged_8k(blob, src, 0, 1.0, n, tab, pr.data_ptr(), None, ws.data_ptr(),
                                                                                 ws.numel(), st, c),
        }
        for name, call in calls.items():
            assert call() == -1
            msg = L.vadx_last_error()
            assert name.encode() in msg and b"8000" in msg, (name, msg)
    assert L.vadx_silero_clips_ragged_8k(blob, src, 0, 1.0, n, tab, pr.data_ptr(), None, ws.data_ptr(), ws.numel(), st, None) == -1
    torch.cuda.synchronize()
    assert (pr == 0).all()                                                # nothing ran
    # an engine without the 8 kHz network says so
    e16 = silero.SileroEngine(weights.silero_synthetic(1234))
    with pytest.raises(ValueError, match="8000"):
        e16.clips_ragged(clips37[:5], sampling_rate=8000)
    with pytest.raises(ValueError, match="8000"):
        e16.clips_ragged(batch)
    with pytest.raises(ValueError, match="no 8 kHz weights"):
        silero.get_speech_timestamps_batch(clips37[:5], e16, sampling_rate=8000)


# ---- 8. segments and drop-ins at 8000
KW = [dict(), dict(threshold=0.45, max_speech_duration_s=0.9, min_speech_duration_ms=100, min_silence_duration_ms=60, speech_pad_ms=20)]


@pytest.fixture(scope="module")
def speech():
    """nine clips of 0.2 - 2.4 s with loud and quiet stretches"""
    full = weights.burst_clips(9, 19000, seed=23, sample_rate=2000).astype(np.float32) * SCALE
    lens = [19000, 1650, 8192, 12501, 6000, 15555, 3500, 10240, 256]
    return [np.ascontiguousarray(full[b, :n]) for b, n in enumerate(lens)]


@pytest.mark.parametrize("kw", KW)
@pytest.mark.parametrize("mode", MODES)
def test_list_form_of_the_batch_entry_points(engine, speech, mode, kw):
    engine.arithmetic = mode
    lens = [len(c) for c in speech]
    got, rows = silero.get_speech_timestamps_batch(speech, engine, sampling_rate=8000, return_probs=True, **kw)
    assert sum(len(r) for r in got) > 5
    rect = np.zeros((len(speech), max(lens)), np.float32)
    for b, c in enumerate(speech):
        rect[b, :len(c)] = c
    want, rprobs = silero.get_speech_timestamps_batch(rect, engine, lengths=lens, sampling_rate=8000, return_probs=True, **kw)
    assert got == want
    assert isinstance(rows, list) and [r.shape[0] for r in rows] == [(n + WIN - 1) // WIN for n in lens]
    for b, r in enumerate(rows):
        assert torch.equal(r, rprobs[b, :r.shape[0]])
    sec = silero.get_speech_timestamps_batch(speech, engine, sampling_rate=8000, return_seconds=True, **kw)
    assert sec == silero.get_speech_timestamps_batch(rect, engine, lengths=lens, sampling_rate=8000, return_seconds=True, **kw)
    batch = ragged.RaggedClips.from_clips(speech, sampling_rate=8000)
    assert silero.get_speech_timestamps_batch(batch, engine, sampling_rate=8000, **kw) == got
    with pytest.raises(ValueError, match="8000"):                          # a batch built for the other rate
        silero.get_speech_timestamps_batch(batch, engine, **kw)
    # the segmenter on the packed scores, against the rows
    probs, first = engine.clips_ragged(batch)
    segs, counts = engine.segments_ragged(probs, first, lens, sampling_rate=8000, **kw)
    f = first.cpu().tolist()
    for b in range(len(speech)):
        s1, c1 = engine.segments(probs[f[b]:f[b + 1]][None], [lens[b]], sampling_rate=8000, **kw)
        assert int(c1[0]) == int(counts[b]) and torch.equal(s1[0, :int(c1[0])], segs[b, :int(counts[b])])
    # the table and the audio variants
    tab = silero.get_speech_timestamps_table(speech, engine, sampling_rate=8000, **kw)
    assert tab.lists() == silero.get_speech_timestamps_table(rect, engine, lengths=lens, sampling_rate=8000, **kw).lists() == sec
    for drop in (False, True):
        p1, o1, t1 = silero.get_speech_audio_batch(speech, engine, drop=drop, sampling_rate=8000, **kw)
        p2, o2, t2 = silero.get_speech_audio_batch(rect, engine, lengths=lens, drop=drop, sampling_rate=8000, **kw)
        assert t1 == t2 == got and torch.equal(o1, o2) and torch.equal(p1, p2) and p1.numel() > 0


def test_driver_runs_a_list_of_8_khz_files_as_one_ragged_batch(engine, tmp_path, monkeypatch):
    from conftest import GOLDEN
    engine.arithmetic = None
    pcm = audio_io.load_wav(os.path.join(GOLDEN, "vad_sample.wav"), 8000)
    files = []
    for k, n in enumerate([len(pcm), 15000, 30617, 4000]):
        files.append(str(tmp_path / f"cut{k}.wav"))
        audio_io.save_wav(files[-1], pcm[:n], 8000)
    model = silero.OnnxWrapper(engine)
    quiet = lambda *_: None      # noqa: E731
    seen = []
    real = silero.SileroEngine.clips_ragged
    monkeypatch.setattr(silero.SileroEngine, "clips_ragged", lambda self, batch, *a, **k: (seen.append(batch), real(self, batch, *a, **k))[1])
    for fp16 in (False, True):
        del seen[:]
        many = drivers.inference_silero(files, model, str(tmp_path / "s.txt"), str(tmp_path / "i.txt"), SAMPLE_RATE=8000, use_fp16=fp16, echo=quiet)
        assert len(seen) == 1 and seen[0].sampling_rate == 8000 and len(seen[0]) == 4      # one ragged batch on the 8 kHz network
        one = [drivers.inference_silero(f, model, str(tmp_path / "s1.txt"), str(tmp_path / "i1.txt"), SAMPLE_RATE=8000, use_fp16=fp16, echo=quiet)
               for f in files]
        assert len(seen) == 1
        assert many == one and sum(len(r) for r in many) >= 1


# ---- 9. above the workspace cap: parts of consecutive groups, at both rates
PART_TG = [9, 5, 3, 2, 1, 1]                      # T_g of the six groups (the last one partial): 21 tiles
PART_CAPS = {9: [(0, 1), (1, 3), (3, 6)],         # the smallest feasible cap, T_g[0] tiles: the most parts
             20: [(0, 5), (5, 6)],                # sum(T_g) - 1 tiles: two parts
             64: [(0, 6)]}                        # above the batch: the two launches of an uncapped call


def part_lengths(win):
    """87 clips whose sorted groups have T_g = PART_TG, in a shuffled order; lengths on both sides of the window edges"""
    rng = np.random.default_rng(77)
    counts = [9, 9, 8, 8, 8, 7, 7, 7, 7, 6, 6, 6, 6, 6, 6, 6] + [5] * 4 + [4] * 12 + [3] * 10 + [2] * 6 + [2] * 9 + [1] * 7 + [1] * 16 + [1] * 7
    assert len(counts) == 87
    lens = [t * win - int(rng.integers(0, win)) for t in counts]
    lens[0], lens[16], lens[32] = 9 * win, 5 * win - win + 1, 3 * win - 1
    return [lens[k] for k in rng.permutation(87).tolist()]


@pytest.fixture(scope="module", params=[16000, 8000])
def part_set(request, engine):
    rate = request.param
    win = 512 if rate == 16000 else 256
    lens = part_lengths(win)
    full = weights.burst_clips(87, 9 * win, seed=33, sample_rate=rate)
    clips = [np.ascontiguousarray(full[b, :n]).astype(np.float32) * SCALE for b, n in enumerate(lens)]
    return rate, win, clips, reference_of(engine, clips, rate)


@pytest.mark.parametrize("mode", MODES)
def test_a_batch_above_the_cap_runs_in_parts(engine, part_set, mode, monkeypatch):
    rate, win, clips, ref = part_set
    batch = ragged.RaggedClips.from_clips(clips, sampling_rate=rate)
    assert batch.group_windows.tolist() == PART_TG and batch.tiles == 21 and batch.groups == 6
    assert int(batch.slot_clip_host[-1]) == -1                             # the last group is partial
    uncapped = run(engine, batch, mode)
    assert_rows(*uncapped, ref[mode])
    for cap_tiles, want_parts in PART_CAPS.items():
        monkeypatch.setattr(silero, "WORKSPACE_CAP_BYTES", cap_tiles * TILE)
        assert batch.parts(silero.WORKSPACE_CAP_BYTES) == want_parts
        engine._ws = None
        probs, first, state = run(engine, batch, mode)
        assert engine._ws.numel() <= silero.WORKSPACE_CAP_BYTES
        assert engine._ws.numel() == max(sum(PART_TG[a:b]) for a, b in want_parts) * TILE
        assert_rows(probs, first, state, ref[mode])
        assert torch.equal(probs, uncapped[0]) and torch.equal(first, uncapped[1]) and torch.equal(state, uncapped[2])
        batch.check()
        # the list form builds the same batch
        probs, first, state = run(engine, clips, mode, sampling_rate=rate)
        assert torch.equal(probs, uncapped[0]) and torch.equal(state, uncapped[2])
    monkeypatch.setattr(silero, "WORKSPACE_CAP_BYTES", (PART_TG[0] - 1) * TILE)
    with pytest.raises(ValueError, match="WORKSPACE_CAP_BYTES"):
        engine.clips_ragged(batch)
    monkeypatch.setattr(silero, "WORKSPACE_CAP_BYTES", PART_TG[0] * TILE)
    with pytest.raises(ValueError, match="WORKSPACE_CAP_BYTES"):         # the separate halves keep the whole batch's gx
        engine.encode_ragged(batch, mode=mode)


def test_range_protocol_across_parts(engine, part_set, monkeypatch):
    rate, win, clips, ref = part_set
    batch0 = ragged.RaggedClips.from_clips(clips, sampling_rate=rate)
    k = int(batch0.slot_clip_host[16])                                    # the first slot of group 1: the second part's longest clip
    assert batch0.windows[k] == 5
    loud = [c.copy() for c in clips]
    loud[k][2 * win:] *= np.float32(1.0e6)
    monkeypatch.setattr(silero, "WORKSPACE_CAP_BYTES", PART_TG[0] * TILE)
    assert ragged.RaggedClips.from_clips(loud, sampling_rate=rate).parts(silero.WORKSPACE_CAP_BYTES) == PART_CAPS[9]
    engine.range_flag(sampling_rate=rate)
    engine.arithmetic = "split"
    want = engine.clips_ragged(loud, return_state=True, sampling_rate=rate)
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[2]).all()
    engine.arithmetic = "h2"
    before = engine.range_fallbacks
    got = engine.clips_ragged(loud, return_state=True, sampling_rate=rate)
    assert engine.range_fallbacks == before + 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert engine.range_flag(sampling_rate=rate)[0] == 0
    # the clips of the other parts are what they were
    f = got[1].cpu().tolist()
    monkeypatch.undo()
    engine.arithmetic = "split"
    for b in (int(batch0.slot_clip_host[0]), int(batch0.slot_clip_host[40]), int(batch0.slot_clip_host[80])):
        p, s = alone(engine, clips[b], "split", rate)
        assert torch.equal(got[0][f[b]:f[b + 1]], p) and torch.equal(got[2][:, b], s)
    engine.arithmetic = None
