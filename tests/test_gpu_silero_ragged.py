"""Silero over a ragged batch (vadx.ragged.RaggedClips, SileroEngine.clips_ragged; include/vadx.h "Silero over a RAGGED batch").
The yardstick throughout is the existing code: engine.clips(clip[None], return_state=True) on one clip alone, in the same arithmetic --
every comparison is torch.equal, bit for bit, on float32 / bf16 x 3 / fp16 x 2.

The 37 clips (tests/test_silero_ragged_cpu.py: LENGTHS_37): group 0 mixes T_b = 33, 32, 31, 17, 16, 15, 9, 8, 5, 4, 3, 2, 2, 2, 2, 1 (every
count of valid encoder slots of a run of four, both sides of the 16-step flush block, lengths 512 k - 100 / 512 k / 512 k + 1 in turn and
513, 575, 576, 577, 511 around the reflect pad and the window edge), group 1 is sixteen clips of one window (uniform; lengths 1, 3, 4, 63,
64, 65, 511, 412, 512 around the vector-load minimum), group 2 the last five (partial)."""
import ctypes

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, audio_io, chunks, drivers, ragged, silero, weights
from test_silero_ragged_cpu import LENGTHS_37

pytestmark = pytest.mark.gpu
MODES = ["f32", "split", "h2"]
SCALE = np.float32(0.000030517578)
WIN = 512


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234))


@pytest.fixture(scope="module")
def pcm37():
    """int16 burst clips cut to LENGTHS_37"""
    full = weights.burst_clips(37, 33 * WIN, seed=91)
    return [np.ascontiguousarray(full[b, :n]) for b, n in enumerate(LENGTHS_37)]


@pytest.fixture(scope="module")
def clips37(pcm37):
    return [c.astype(np.float32) * SCALE for c in pcm37]


def alone(engine, clip, mode):
    """(probs [T], state [2, 128]) of one clip through the rectangular path, in `mode`"""
    engine.arithmetic = mode
    p, s = engine.clips(torch.from_numpy(np.ascontiguousarray(clip))[None].cuda(), return_state=True)
    return p[0].clone(), s[:, 0].clone()


@pytest.fixture(scope="module")
def reference(engine, clips37):
    """per arithmetic, per clip: the rectangular path on that clip alone -- computed once, asserted finite, never changed"""
    ref = {}
    for mode in MODES:
        before = engine.range_fallbacks
        ref[mode] = [alone(engine, c, mode) for c in clips37]
        assert engine.range_fallbacks == before
        for p, s in ref[mode]:
            assert torch.isfinite(p).all() and torch.isfinite(s).all()
    engine.arithmetic = None
    return ref


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
    batch = ragged.RaggedClips.from_clips(clips37)
    assert batch.group_windows.tolist() == [33, 1, 1] and batch.tiles == 35
    probs, first, state = run(engine, batch, mode)
    assert probs.shape == (sum((n + WIN - 1) // WIN for n in LENGTHS_37),) and state.shape == (2, 37, 128)
    assert_rows(probs, first, state, reference[mode])
    batch.check()


# ---- 2. neighbours and order
@pytest.mark.parametrize("mode", MODES)
def test_order_and_neighbours_do_not_matter(engine, clips37, reference, mode):
    perm = np.random.default_rng(5).permutation(37).tolist()
    probs, first, state = run(engine, [clips37[k] for k in perm], mode)
    assert_rows(probs, first, state, reference[mode], order=perm)
    for k in (0, 3, 4, 5, 15, 20):                     # T_b = 33, 17, 16, 15, 1, 1: the group's own T_g at the flush block's edges
        probs, first, state = run(engine, [clips37[k]], mode)
        assert_rows(probs, first, state, [reference[mode][k]])
    sub = [2, 3, 4, 7, 11, 30]                         # a partial group alone
    probs, first, state = run(engine, [clips37[k] for k in sub], mode)
    assert_rows(probs, first, state, reference[mode], order=sub)


# ---- 3. source forms
@pytest.mark.parametrize("mode", MODES)
def test_int16_source_equals_the_scaled_float32(engine, pcm37, reference, mode):
    for c16, c32 in zip(pcm37[:3], [c.astype(np.float32) * SCALE for c in pcm37[:3]]):
        assert np.array_equal(torch.from_numpy(c16).float().numpy() * np.float32(engine.PCM16_SCALE), c32)
    probs, first, state = run(engine, pcm37, mode)
    assert_rows(probs, first, state, reference[mode])


@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("mode", MODES)
def test_any_element_residue_equals_the_aligned_clip(engine, pcm37, clips37, reference, mode, dtype):
    """two clips (T_b = 5 and one of 65 samples), each starting at element residues 0 ... 7 of the packed vector"""
    src = pcm37 if dtype == "int16" else clips37
    ids = [8, 21]
    assert LENGTHS_37[8] == 512 * 4 + 1 and LENGTHS_37[21] == 65
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
    batch = ragged.RaggedClips.from_packed(torch.from_numpy(vec).cuda(), offs, lens)
    probs, first, state = run(engine, batch, mode)
    assert_rows(probs, first, state, reference[mode], order=which)
    batch.check()


@pytest.mark.parametrize("mode", MODES)
def test_cascade_from_collect_chunks(engine, mode):
    """cut the speech out on the device, re-score the cut clips where they lie: from_packed over collect_chunks_batch's output"""
    engine.arithmetic = mode
    audio = torch.from_numpy(weights.burst_clips(6, 14000, seed=20, sample_rate=4000).astype(np.float32) * SCALE).cuda()
    lens = [14000, 9000, 13001, 5000, 12000, 7777]
    probs = engine.clips(audio)
    segs, counts = engine.segments(probs, lens)
    packed, offsets, plan = chunks.collect_chunks_batch((segs, counts), audio, lengths=lens, align=1, return_plan=True)
    n = plan.lengths.cpu().numpy()
    keep = [b for b in range(6) if n[b] > 0]
    assert len(keep) >= 3                                                 # (the test's own precondition: clips with speech to cut)
    off = offsets.cpu().numpy()[:-1]
    batch = ragged.RaggedClips.from_packed(packed, off[keep], n[keep])
    assert batch.pcm.data_ptr() == packed.data_ptr()                      # no copy
    got, first, state = run(engine, batch, mode)
    ref = []
    for b in keep:
        cut = packed[int(off[b]):int(off[b] + n[b])]
        p, s = engine.clips(cut[None].clone(), return_state=True)
        assert torch.isfinite(p).all()
        ref.append((p[0], s[:, 0]))
    assert_rows(got, first, state, ref)


# ---- 4. canary guards
@pytest.mark.parametrize("mode", MODES)
def test_nothing_is_written_outside_scores_and_workspace(engine, clips37, reference, mode):
    batch = ragged.RaggedClips.from_clips(clips37)
    engine.arithmetic = mode
    L, G = _lib.lib(), 4096
    need = L.vadx_silero_ragged_workspace_bytes(batch.tiles)
    assert need == batch.workspace_bytes == 35 * 32768
    ws = torch.full((need + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    pr = torch.full((batch.n_windows + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
    st = torch.full((2 * 37 * 128 + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
    tab = batch.tables()
    _lib.check(L.vadx_silero_clips_ragged(engine.packed.data_ptr(), batch.pcm.data_ptr(), 0, 1.0, batch.pcm.numel(), tab,
                                          pr.data_ptr() + 4 * G, st.data_ptr() + 4 * G, ws.data_ptr() + G, need, _lib.stream_ptr(),
                                          engine.cfg(mode)))
    torch.cuda.synchronize()
    assert (ws[:G] == 0x5A).all() and (ws[G + need:] == 0x5A).all()
    assert (pr[:G] == -7.0).all() and (pr[G + batch.n_windows:] == -7.0).all()
    assert (st[:G] == -7.0).all() and (st[G + 2 * 37 * 128:] == -7.0).all()
    body = pr[G:G + batch.n_windows]
    assert (body != -7.0).all()                                           # every score entry is written
    assert_rows(body, batch.probs_first, st[G:G + 2 * 37 * 128].view(2, 37, 128), reference[mode])
    assert engine.range_flag()[0] == 0
    # a workspace one byte short is refused, by name
    rc = L.vadx_silero_clips_ragged(engine.packed.data_ptr(), batch.pcm.data_ptr(), 0, 1.0, batch.pcm.numel(), tab, pr.data_ptr() + 4 * G,
                                    None, ws.data_ptr() + G, need - 1, _lib.stream_ptr(), engine.cfg(mode))
    assert rc == -2 and b"workspace" in L.vadx_last_error()


# ---- 5. lying tables: the device refuses a slot before indexing through it
@pytest.mark.parametrize("lie", ["offset past the end", "negative offset", "length past the end", "huge offset"])
@pytest.mark.parametrize("mode", MODES)
def test_a_slot_outside_the_source_is_refused_on_the_device(engine, clips37, reference, mode, lie):
    batch = ragged.RaggedClips.from_clips(clips37)
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
    with pytest.raises(ValueError, match="outside the packed vector"):    # the host refuses what it can see
        ragged.RaggedClips.from_packed(batch.pcm, [0, n_src - 4], [8, 5])


# ---- 6. range protocol (fp16 x 2 is the arithmetic that has one)
def test_range_protocol(engine, clips37, reference):
    loud = [c.copy() for c in clips37]
    assert LENGTHS_37[3] == 17 * WIN - 100
    loud[3][16 * WIN:] *= np.float32(1.0e6)                               # clip 3's last window, far outside +-1 (and the fp16 range)
    engine.range_flag()
    # unchecked: the halves on fp16 x 2
    batch = ragged.RaggedClips.from_clips(loud)
    engine.encode_ragged(batch, mode="h2")
    state = torch.empty((2, 37, 128), dtype=torch.float32, device="cuda")
    probs = engine.recur_ragged(batch, state_n=state, mode="h2")
    flag, amax = engine.range_flag()
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
    want = engine.clips_ragged(loud, return_state=True)
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[2]).all()
    engine.arithmetic = "h2"
    before = engine.range_fallbacks
    got = engine.clips_ragged(loud, return_state=True)
    assert engine.range_fallbacks == before + 1
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert engine.range_flag()[0] == 0


# ---- 7. segments and drop-ins
KW = [dict(), dict(threshold=0.45, max_speech_duration_s=0.9, min_speech_duration_ms=100, min_silence_duration_ms=60, speech_pad_ms=20)]


@pytest.fixture(scope="module")
def speech():
    """nine clips of 0.2 - 2.4 s with loud and quiet stretches"""
    full = weights.burst_clips(9, 38000, seed=23, sample_rate=4000).astype(np.float32) * SCALE
    lens = [38000, 3300, 16384, 25001, 12000, 31111, 7000, 20480, 512]
    return [np.ascontiguousarray(full[b, :n]) for b, n in enumerate(lens)]


@pytest.mark.parametrize("mode", MODES)
def test_segments_ragged_equals_segments_on_the_rows(engine, speech, mode):
    engine.arithmetic = mode
    probs, first = engine.clips_ragged(speech)
    lens = [len(c) for c in speech]
    total = 0
    for kw in KW:
        segs, counts = engine.segments_ragged(probs, first, lens, **kw)
        f = first.cpu().tolist()
        for b in range(len(speech)):
            s1, c1 = engine.segments(probs[f[b]:f[b + 1]][None], [lens[b]], **kw)
            assert int(c1[0]) == int(counts[b]) and torch.equal(s1[0, :int(c1[0])], segs[b, :int(counts[b])])
            total += int(c1[0])
    assert total > 10


@pytest.mark.parametrize("kw", KW)
@pytest.mark.parametrize("mode", MODES)
def test_list_form_of_the_batch_entry_points(engine, speech, mode, kw):
    engine.arithmetic = mode
    lens = [len(c) for c in speech]
    got, rows = silero.get_speech_timestamps_batch(speech, engine, return_probs=True, **kw)
    assert sum(len(r) for r in got) > 5
    assert got == [silero.get_speech_timestamps(torch.from_numpy(c), engine, **kw) for c in speech]
    rect = np.zeros((len(speech), max(lens)), np.float32)
    for b, c in enumerate(speech):
        rect[b, :len(c)] = c
    want, rprobs = silero.get_speech_timestamps_batch(rect, engine, lengths=lens, return_probs=True, **kw)
    assert got == want
    assert isinstance(rows, list) and [r.shape[0] for r in rows] == [(n + WIN - 1) // WIN for n in lens]
    for b, r in enumerate(rows):
        assert torch.equal(r, rprobs[b, :r.shape[0]])
    sec = silero.get_speech_timestamps_batch(speech, engine, return_seconds=True, **kw)
    assert sec == silero.get_speech_timestamps_batch(rect, engine, lengths=lens, return_seconds=True, **kw)
    assert silero.get_speech_timestamps_batch(ragged.RaggedClips.from_clips(speech), engine, **kw) == got
    # the table and the audio variants
    tab = silero.get_speech_timestamps_table(speech, engine, **kw)
    assert tab.lists() == silero.get_speech_timestamps_table(rect, engine, lengths=lens, **kw).lists() == sec
    for drop in (False, True):
        p1, o1, t1 = silero.get_speech_audio_batch(speech, engine, drop=drop, **kw)
        p2, o2, t2 = silero.get_speech_audio_batch(rect, engine, lengths=lens, drop=drop, **kw)
        assert t1 == t2 == got and torch.equal(o1, o2) and torch.equal(p1, p2) and p1.numel() > 0


def test_driver_runs_a_list_of_files_as_one_ragged_batch(tmp_path):
    from conftest import GOLDEN
    import os
    pcm = audio_io.load_wav(os.path.join(GOLDEN, "vad_sample.wav"))
    files = []
    for k, n in enumerate([len(pcm), 30000, 61234, 8000]):
        files.append(str(tmp_path / f"cut{k}.wav"))
        audio_io.save_wav(files[-1], pcm[:n], 16000)
    model = silero.load_silero_vad(onnx=True, use_cpu=True, path="synthetic:1234")
    quiet = lambda *_: None      # noqa: E731
    for fp16 in (False, True):
        many = drivers.inference_silero(files, model, str(tmp_path / "s.txt"), str(tmp_path / "i.txt"), use_fp16=fp16, echo=quiet)
        one = [drivers.inference_silero(f, model, str(tmp_path / "s1.txt"), str(tmp_path / "i1.txt"), use_fp16=fp16, echo=quiet) for f in files]
        assert many == one and sum(len(r) for r in many) >= 1


# ---- 8. refusals by name
def test_refusals(engine, speech, monkeypatch):
    engine.arithmetic = None
    with pytest.raises(ValueError, match="8000"):
        silero.get_speech_timestamps_batch(speech, engine, sampling_rate=8000)
    with pytest.raises(ValueError, match="32000"):
        silero.get_speech_timestamps_batch(speech, engine, sampling_rate=32000)
    with pytest.raises(ValueError, match="dtype"):
        engine.clips_ragged([c.astype(np.float64) for c in speech])
    with pytest.raises(ValueError, match="dtype"):
        ragged.RaggedClips.from_packed(torch.zeros(64, dtype=torch.float64, device="cuda"), [0], [64])
    monkeypatch.setattr(silero, "WORKSPACE_CAP_BYTES", 10 * 32768)
    with pytest.raises(ValueError, match="WORKSPACE_CAP_BYTES"):
        engine.clips_ragged(speech)
    monkeypatch.undo()
    # the C ABI: the 8 kHz network has no ragged encoder
    batch = ragged.RaggedClips.from_clips(speech)
    engine._ragged_workspace(batch, "test")
    cfg = _lib.SileroCfg()
    cfg.sample_rate = 8000
    L = _lib.lib()
    probs = torch.empty(batch.n_windows, dtype=torch.float32, device="cuda")
    rc = L.vadx_silero_clips_ragged(engine.packed.data_ptr(), batch.pcm.data_ptr(), 0, 1.0, batch.pcm.numel(), batch.tables(), probs.data_ptr(),
                                    None, engine._ws.data_ptr(), engine._ws.numel(), _lib.stream_ptr(), ctypes.byref(cfg))
    assert rc == -1 and b"8000" in L.vadx_last_error()
