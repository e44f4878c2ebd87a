"""GPU: vadx.chunks -- the batched collect_chunks / drop_chunks (Silero/modeling_modified/utils_vad.py:588-682) on the device.

Every comparison is BITWISE against tests/_chunks_ref.py (pinned to the reference's own functions by tests/test_chunks_cpu.py) on RAMP
audio: a sample's value is its own index in its clip, so a misplaced element names where it came from.  The destination is wrapped in
canary-filled guard regions of 64 elements on both sides and pre-filled with the canary itself: the guards must be intact afterwards and
every alignment gap must have been written as zero."""
import os

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, audio_io, chunks, drivers, silero, weights

import _chunks_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
DTYPES = {"i16": np.int16, "f32": np.float32}
CANARY = {"i16": np.int16(0x5A5B), "f32": np.float32(-7777.25)}
WAV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vad_sample.wav")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ramp(n, tag):
    return np.arange(n, dtype=DTYPES[tag])


def pack_source(clips, starts=None, tail=0):
    """clips laid into one vector at `starts` (default: end to end, each on a multiple of 8 elements), the rest filled with a value no
    ramp holds; `tail` extra elements after the last clip."""
    lens = np.asarray([len(c) for c in clips], dtype=np.int64)
    if starts is None:
        starts = np.concatenate([[0], np.cumsum((lens + 7) // 8 * 8)])[:-1]
    starts = np.asarray(starts, dtype=np.int64)
    total = int((starts + lens).max()) + tail if len(clips) else tail
    flat = np.full(total, -3, dtype=clips[0].dtype)
    for s, c in zip(starts, clips):
        flat[s:s + len(c)] = c
    return flat, starts, lens


def run_device(mode, table, flat, starts, lens, align, tag, shrink=0):
    """Plan + copy into a guarded destination.  `table` is a host list or a device pair.  -> (out [total] numpy or None when the copy
    refused, offsets, lengths, status, plan); asserts that the guards are intact."""
    src = T(flat)
    if isinstance(table, tuple):
        segs, counts = table
    else:
        segs, counts = (T(a) for a in chunks.table_of(table))
    plan = chunks.ChunkPlan(segs, counts, T(lens), mode, align)
    total = plan.total
    room = max(total - shrink, 0)
    whole = torch.full((GUARD + room + GUARD,), float(CANARY[tag]) if tag == "f32" else int(CANARY[tag]), dtype=src.dtype, device=DEV)
    plan.copy(src, T(starts), whole[GUARD:GUARD + room])
    torch.cuda.synchronize()
    host = whole.cpu().numpy()
    assert np.all(host[:GUARD] == CANARY[tag]) and np.all(host[GUARD + room:] == CANARY[tag]), "a guard region was written"
    return host[GUARD:GUARD + room], plan.clip_offsets.cpu().numpy(), plan.lengths.cpu().numpy(), plan.status, plan


def check(mode, tables, clips, align, tag, starts=None, tail=0):
    flat, starts, lens = pack_source(clips, starts, tail)
    got, offsets, lengths, status, plan = run_device(mode, tables, flat, starts, lens, align, tag)
    want, woff, wlen = ref.packed(mode, tables, clips, align)
    assert status == 0
    assert np.array_equal(offsets, woff) and np.array_equal(lengths, wlen)
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
    return got, offsets, lengths, plan


def random_rows(rng, n, k):
    """k rows over a clip of n samples: mostly inside, some negative, past the end, reversed or empty"""
    rows = []
    for _ in range(k):
        a, b = sorted(int(v) for v in rng.integers(0, n + 1, 2))
        kind = int(rng.integers(0, 8))
        if kind == 0:
            a, b = a - n - 1, b                    # a negative start
        elif kind == 1:
            b = b + n + 3                          # an end past the end
        elif kind == 2:
            a, b = b, a                            # reversed
        elif kind == 3:
            b = a                                  # empty
        rows.append((a, b))
    return rows


LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000]


@pytest.mark.parametrize("align", [1, 8, 64])
@pytest.mark.parametrize("mode", ["collect", "drop"])
@pytest.mark.parametrize("tag", ["i16", "f32"])
def test_every_clip_length(tag, mode, align):
    rng = np.random.default_rng(11 + align)
    clips = [ramp(n, tag) for n in LENGTHS]
    tables = [random_rows(rng, n, 1 + i % 4) for i, n in enumerate(LENGTHS)]
    tables[3] = sorted(tables[3])
    check(mode, tables, clips, align, tag)
    check(mode, [[(0, n)] for n in LENGTHS], clips, align, tag)            # whole clips: collect copies all, drop leaves nothing


@pytest.mark.parametrize("mode", ["collect", "drop"])
@pytest.mark.parametrize("tag", ["i16", "f32"])
def test_piece_starts_at_every_residue(tag, mode):
    """A piece of every length in {0, 1, 7, 8, 9, 33} starting at every residue of a 16-byte vector (mod 8 for int16, mod 4 for float32),
    in a clip of its own and all in one clip -- so that every source shift meets every destination residue."""
    vec = 8 if tag == "i16" else 4
    sizes = [0, 1, 7, 8, 9, 33]
    clips, tables = [], []
    for r in range(vec):
        for first in range(len(sizes)):                                    # rotate: every length leads once, at destination residue 0
            order = sizes[first:] + sizes[:first]
            rows = [(r + 48 * j, r + 48 * j + n) for j, n in enumerate(order)]
            tables.append(rows)
            clips.append(ramp(48 * len(sizes) + 5, tag))
    tables.append([(r + 16 * k, r + 16 * k + n) for k, (r, n) in enumerate((r, n) for r in range(vec) for n in sizes)])
    clips.append(ramp(16 * vec * len(sizes) + 40, tag))
    for align in (1, 8):
        check(mode, tables, clips, align, tag)


@pytest.mark.parametrize("tag", ["i16", "f32"])
def test_seams_inside_one_vector(tag):
    """Two misaligned pieces meeting inside one 16-byte destination vector; 64 pieces of length 1 in one clip (every element a seam)."""
    check("collect", [[(3, 8), (21, 40)]], [ramp(50, tag)], 1, tag)
    check("collect", [[(3, 5), (9, 10), (21, 60)], [(1, 2)]], [ramp(70, tag), ramp(4, tag)], 8, tag)
    ones = [(2 * i + 1, 2 * i + 2) for i in range(64)]
    got, _, lengths, _ = check("collect", [ones], [ramp(200, tag)], 1, tag)
    assert lengths.tolist() == [64] and got.tolist() == list(range(1, 129, 2))
    check("drop", [ones], [ramp(200, tag)], 1, tag)


@pytest.mark.parametrize("mode", ["collect", "drop"])
@pytest.mark.parametrize("tag", ["i16", "f32"])
def test_long_piece_spans_tiles(tag, mode):
    """One piece of 20 000 elements (three int16 tiles, five float32 tiles) from a misaligned start, beside a short neighbour."""
    rows = [(37, 20037)] if mode == "collect" else [(0, 37), (20037, 20100)]
    check(mode, [[(2, 5)], rows, [(1, 3)]], [ramp(9, tag), ramp(20100, tag), ramp(6, tag)], 8, tag)


@pytest.mark.parametrize("tag", ["i16", "f32"])
def test_source_ends_at_the_last_element_of_src(tag):
    """The last clip ends exactly where src ends, src is not a whole number of 16-byte vectors, and the piece runs to the end from a
    misaligned start: the aligned vector pair around its tail would reach past src, so the tail goes element by element."""
    for n in (61, 64, 67, 1003):
        clips = [ramp(40, tag), ramp(n, tag)]
        for start in (n - 21, n - 16, n - 9, 0):
            for starts in ([0, 40], [0, 43]):
                check("collect", [[(0, 40)], [(start, n)]], clips, 1, tag, starts=starts)
                check("drop", [[(0, 40)], [(0, start)]], clips, 8, tag, starts=starts)


@pytest.mark.parametrize("cap", [1, 3, 64, 65, 130])
def test_table_capacities(cap):
    """count = 0 and count = cap at table widths on both sides of the 64-lane round of the plan kernel."""
    n = 3 * cap + 10
    full = [(3 * k + 1, 3 * k + 1 + (k % 3) + 1) for k in range(cap)]
    tables = [full, [], full[::-1], []]
    clips = [ramp(n, "i16") for _ in tables]
    segs, counts = chunks.table_of(tables, cap=cap)
    assert counts.tolist() == [cap, 0, cap, 0]
    for mode in ("collect", "drop"):
        flat, starts, lens = pack_source(clips)
        got, offsets, lengths, status, plan = run_device(mode, (T(segs), T(counts)), flat, starts, lens, 8, "i16")
        want, woff, wlen = ref.packed(mode, tables, clips, 8)
        assert status == 0 and np.array_equal(got, want) and np.array_equal(offsets, woff) and np.array_equal(lengths, wlen)
        host = chunks.plan_host(segs, counts, lens, mode, 8)
        assert np.array_equal(plan.piece_offsets.cpu().numpy(), host["piece_dst"])
        assert np.array_equal(plan.piece_src.cpu().numpy(), host["piece_src"])
        assert np.array_equal(plan.n_pieces.cpu().numpy(), host["n_pieces"]) and plan.total == host["total"]


@pytest.mark.parametrize("mode", ["collect", "drop"])
def test_bad_clips_are_refused_alone(mode):
    """count = cap + 1, count = -1 and clip_len = -1: the status bit is set, the clip's output is empty, its rows (2^62 everywhere) are
    never used and its neighbours come out as they do without it."""
    cap = 3
    good = [(2, 9), (11, 30)]
    tables = [good, good, good, good, good, good, good]
    clips = [ramp(40, "i16") for _ in tables]
    segs, counts = chunks.table_of(tables, cap=cap)
    flat, starts, lens = pack_source(clips)
    for b in (1, 3, 5):
        segs[b] = 1 << 62
    counts[1], counts[3] = cap + 1, -1
    lens_bad = lens.copy()
    lens_bad[5] = -1
    got, offsets, lengths, status, plan = run_device(mode, (T(segs), T(counts)), flat, starts, lens_bad, 8, "i16")
    assert status == chunks.ST_BAD_CLIP
    assert plan.n_pieces.cpu().numpy().tolist() == [2 + (mode == "drop"), -1] * 3 + [2 + (mode == "drop")]
    assert lengths[[1, 3, 5]].tolist() == [0, 0, 0]
    with pytest.raises(_lib.VadxError, match="segment count"):
        plan.check()
    keep = [0, 2, 4, 6]
    want, woff, wlen = ref.packed(mode, [tables[b] for b in keep], [clips[b] for b in keep], 8)
    assert np.array_equal(got, want) and np.array_equal(lengths[keep], wlen) and np.array_equal(offsets[keep], woff[:-1])
    assert np.array_equal(plan.piece_src.cpu().numpy()[[1, 3, 5]], np.zeros((3, cap + 1, 2), np.int64))
    with pytest.raises(_lib.VadxError, match="segment count"):           # the allocating call reads the status with the total
        chunks.collect_chunks_batch((T(segs), T(counts)), T(flat), lengths=lens_bad, clip_offsets=starts)


@pytest.mark.parametrize("B", [1, 2, 1025, 70000])
def test_batch_sizes_cross_every_round_of_the_prefix(B):
    """Clips of 0 - 9 samples, one or two rows each: B = 1025 and 70 000 cross the 1024-clip rounds of the cross-clip prefix, and a
    destination tile holds thousands of clips."""
    rng = np.random.default_rng(B)
    n = rng.integers(0, 10, B)
    clips = [ramp(int(v), "i16") for v in n]
    a = rng.integers(0, 10, (B, 2, 2))
    tables = [[tuple(r) for r in a[b, :1 + b % 2].tolist()] for b in range(B)]
    for mode, align in (("collect", 1), ("drop", 8)):
        check(mode, tables, clips, align, "i16")


@pytest.mark.parametrize("tag", ["i16", "f32"])
def test_rectangle_and_packed_sources_give_the_same_bytes(tag):
    """A [B, N] rectangle (clip_src = b * N, aligned or not as N is), a packed vector with 16-byte clip starts and one with odd clip
    starts: one result.  And a clip's bytes do not depend on its neighbours or on B."""
    rng = np.random.default_rng(5)
    lens = [100, 37, 64, 1, 90]
    clips = [ramp(n, tag) for n in lens]
    tables = [random_rows(rng, n, 3) for n in lens]
    for mode in ("collect", "drop"):
        want, woff, wlen = ref.packed(mode, tables, clips, 1)
        for N in (104, 101):
            rect = np.full((len(lens), N), -3, dtype=DTYPES[tag])
            for b, c in enumerate(clips):
                rect[b, :len(c)] = c
            got, off = (chunks.collect_chunks_batch if mode == "collect" else chunks.drop_chunks_batch)(tables, T(rect), lengths=lens)
            assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(off.cpu().numpy(), woff)
        for starts in (None, [1, 131, 201, 301, 303]):
            check(mode, tables, clips, 1, tag, starts=starts, tail=3)
        for b in range(len(lens)):
            alone, _, _, _ = check(mode, [tables[b]], [clips[b]], 1, tag)
            assert np.array_equal(alone, want[woff[b]:woff[b] + wlen[b]])
        pair, _, _, _ = check(mode, tables[1:3], clips[1:3], 1, tag)
        assert np.array_equal(pair, want[woff[1]:woff[3]])


def test_out_too_small_by_one_element_writes_nothing():
    clips = [ramp(300, "i16"), ramp(50, "i16")]
    tables = [[(5, 205)], [(0, 33)]]
    flat, starts, lens = pack_source(clips)
    got, _, _, status, plan = run_device("collect", tables, flat, starts, lens, 1, "i16", shrink=1)
    assert plan.total == 233 and got.shape == (232,)
    assert status == chunks.ST_OVERFLOW and np.all(got == CANARY["i16"])
    with pytest.raises(_lib.VadxError, match="does not fit"):
        plan.check()
    out = torch.full((240,), 9, dtype=torch.int16, device=DEV)            # and the public call with a large enough `out`: no status
    packed, off, plan = chunks.collect_chunks_batch(tables, T(flat), lengths=lens, clip_offsets=starts, out=out, return_plan=True)
    plan.check()
    assert packed is out and np.array_equal(out.cpu().numpy()[:233], ref.packed("collect", tables, clips)[0]) and np.all(out.cpu().numpy()[233:] == 9)
    small = torch.full((232,), 9, dtype=torch.int16, device=DEV)
    _, _, plan = chunks.collect_chunks_batch(tables, T(flat), lengths=lens, clip_offsets=starts, out=small, return_plan=True)
    with pytest.raises(_lib.VadxError, match="does not fit"):
        plan.check()
    assert np.all(small.cpu().numpy() == 9)


def test_a_source_that_its_offsets_do_not_describe_is_not_read():
    """clip_src / lengths pointing past src: nothing outside src is read, those samples are zeros and the status says so."""
    flat = ramp(64, "i16")
    got, _, lengths, status, _ = run_device("collect", [[(0, 40)]], flat, np.asarray([40]), np.asarray([40]), 1, "i16")
    assert status == chunks.ST_SRC_RANGE and lengths.tolist() == [40]
    assert got.tolist() == list(range(40, 64)) + [0] * 16


@pytest.fixture(scope="module")
def model():
    return silero.load_silero_vad(onnx=True, use_cpu=True, path="synthetic:1234", device=DEV)


SEG_KW = dict(threshold=0.5, max_speech_duration_s=20, min_speech_duration_ms=250, min_silence_duration_ms=250)


def test_device_pair_from_the_segmenter_equals_the_host_list(model):
    """(segs, counts) as SileroEngine.segments returns them, handed over on the device, against the same timestamps as a host list --
    and both against the numpy reference."""
    pcm = weights.burst_clips(3, 48000, seed=5)
    audio = pcm.astype(np.float32) * np.float32(0.000030517578)
    eng = model.engine
    probs = eng.clips(audio)
    segs, counts = eng.segments(probs, 48000, **SEG_KW)
    tables = [[tuple(r) for r in segs[b, :int(counts[b])].cpu().numpy().tolist()] for b in range(3)]
    assert sum(len(t) for t in tables) >= 3
    for mode, fn in (("collect", chunks.collect_chunks_batch), ("drop", chunks.drop_chunks_batch)):
        for src in (T(pcm), T(audio)):
            a, oa = fn((segs, counts), src, align=8)
            b, ob = fn(tables, src, align=8)
            want, woff, _ = ref.packed(mode, tables, list(src.cpu().numpy()), 8)
            assert torch.equal(a, b) and torch.equal(oa, ob)
            assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(oa.cpu().numpy(), woff)


def test_get_speech_audio_batch_equals_the_per_clip_calls(model):
    pcm = weights.burst_clips(3, 40000, seed=8)
    audio = pcm.astype(np.float32) * np.float32(0.000030517578)
    lens = [40000, 33333, 25000]
    for b, n in enumerate(lens):
        audio[b, n:] = 0
    ts = silero.get_speech_timestamps_batch(audio, model, lengths=lens, **SEG_KW)
    assert sum(len(t) for t in ts) >= 3
    for drop in (False, True):
        packed, offsets, got_ts = silero.get_speech_audio_batch(audio, model, lengths=lens, drop=drop, **SEG_KW)
        assert got_ts == ts and packed.dtype == torch.float32 and offsets.cpu().numpy()[0] == 0
        off = offsets.cpu().numpy()
        for b, n in enumerate(lens):
            wav = T(audio[b, :n])
            if drop or ts[b]:
                one = (silero.drop_chunks if drop else silero.collect_chunks)(ts[b], wav)
                assert torch.equal(packed[off[b]:off[b + 1]], one)
            else:
                assert off[b + 1] == off[b]
    secs = silero.get_speech_audio_batch(audio, model, lengths=lens, return_seconds=True, **SEG_KW)[2]
    assert secs == silero.get_speech_timestamps_batch(audio, model, lengths=lens, return_seconds=True, **SEG_KW)


def test_drop_ins_reproduce_the_reference(golden):
    """Every row of tests/golden/chunks.npz -- the reference's own functions on ramps -- including its ValueErrors."""
    g = golden("chunks")
    seen = 0
    for name in g["names"].tolist():
        seconds, sr = g[f"{name}_seconds"].tolist()
        tss = [{"start": s, "end": e} if seconds else {"start": int(s), "end": int(e)} for s, e in g[f"{name}_rows"].tolist()]
        for fn, call in (("collect", silero.collect_chunks), ("drop", silero.drop_chunks)):
            for tag, dt in (("i16", torch.int16), ("f32", torch.float32)):
                wav = torch.arange(int(g[f"{name}_len"]), dtype=dt, device=DEV)
                err = str(g[f"{name}_{fn}_chunks_{tag}_error"])
                kw = dict(seconds=True, sampling_rate=sr or None) if seconds else {}
                if err:
                    assert err == "ValueError"
                    with pytest.raises(ValueError):
                        call(tss, wav, **kw)
                    continue
                got = call(tss, wav, **kw)
                want = g[f"{name}_{fn}_chunks_{tag}"]
                assert got.dtype == dt and got.dim() == 1 and got.device == wav.device
                assert np.array_equal(got.cpu().numpy(), want), (name, fn, tag)
                seen += 1
    assert seen >= 50


def test_driver_writes_the_collected_speech(model, tmp_path):
    out = str(tmp_path / "speech.wav")
    got = drivers.inference_silero(WAV, model, str(tmp_path / "s.txt"), str(tmp_path / "i.txt"), echo=lambda *_: None, save_speech_audio=out)
    assert got == drivers.inference_silero(WAV, model, str(tmp_path / "s2.txt"), str(tmp_path / "i2.txt"), echo=lambda *_: None)
    assert len(got) >= 1
    pcm = audio_io.load_wav(WAV)
    want = silero.collect_chunks([{"start": s, "end": e} for s, e in chunks.from_seconds([got], 16000)[0]], T(pcm)).cpu().numpy()
    assert want.dtype == np.int16 and 0 < len(want) <= len(pcm)
    assert np.array_equal(audio_io.load_wav(out), want)
    assert np.array_equal(want, ref.collect(chunks.from_seconds([got], 16000)[0], pcm))
    many = drivers.inference_silero([WAV, WAV], model, str(tmp_path / "s3.txt"), str(tmp_path / "i3.txt"), echo=lambda *_: None,
                                    save_speech_audio=out)
    assert many == [got, got]
    for k in range(2):
        assert np.array_equal(audio_io.load_wav(f"{out}.{k}"), want)
