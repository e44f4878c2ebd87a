"""GPU: vadx.prepare -- ragged batches normalised, padded and packed on the device (csrc/prepare.hip), and the ragged ingest before them.

Everything is compared BITWISE: the packed vector and every table against `RaggedBatch.from_clips(..., device=None)` of the same clips
(tests/_prepare_cases.py: every length where a path changes, four kinds of signal, every source residue), the per-clip records against
the host mirror (vadx.prepare.prepare_host, pinned by tests/test_prepare_cpu.py).  Every output lies between canary-filled guards."""
import wave

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, audio_io, chunks, clips as vclips, drivers, firered, fsmn, marblenet, prepare, ragged, timestamps, weights

import _prepare_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
CANARY = 0x5A5B


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def guarded(total):
    """(whole, view): an int16 buffer of canaries, `total` elements of it between two guards (the view starts on a 16-byte boundary)"""
    whole = torch.full((GUARD + total + GUARD,), CANARY, dtype=torch.int16, device=DEV)
    return whole, whole[GUARD:GUARD + total]


def guards_intact(whole, total):
    host = whole.cpu().numpy()
    return bool(np.all(host[:GUARD] == CANARY) and np.all(host[GUARD + total:] == CANARY))


def packed(clips, window, stride, noise, mode, lead=0, **kw):
    """from_packed of `clips` laid into one source vector at every residue, into a guarded output -> (batch, packed vector on the host)"""
    flat, starts, lens = pc.pack_source(clips, lead)
    total = int(sum(n + vclips.pad_count(int(n), window, stride) for n in lens))
    whole, out = guarded(total)
    rb = ragged.RaggedBatch.from_packed(T(flat), starts, lens, window, stride, noise, mode, out=out, **kw)
    torch.cuda.synchronize()
    assert guards_intact(whole, total), "a guard region was written"
    assert rb.pcm.data_ptr() == out.data_ptr() and rb.pcm.numel() == total and rb.pcm_host is None
    return rb, rb.pcm.cpu().numpy()


_MIRROR = {}


def mirror(grid, mode):
    if (grid, mode) not in _MIRROR:
        _MIRROR[grid, mode] = prepare.prepare_host(pc.clips_of(grid), *pc.GRIDS[grid], pc.noise_of(grid), mode)
    return _MIRROR[grid, mode]


def same_records(rb, m):
    rec = rb.records.cpu().numpy()
    assert rec[:, 0].tobytes() == m.scales.tobytes(), (rec[:, 0], m.scales)
    assert rec[:, 1].tobytes() == m.tail_rms.tobytes(), (rec[:, 1], m.tail_rms)
    assert not rb.prepared.status().any()


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("grid", list(pc.GRIDS))
def test_from_packed_is_from_clips(grid, mode):
    window, stride = pc.GRIDS[grid]
    want = pc.reference(grid, mode)
    rb, got = packed(pc.clips_of(grid), window, stride, pc.noise_of(grid), mode)
    pc.same_tables(rb, want)
    assert pc.first_difference(got, want.pcm_host) is None, pc.first_difference(got, want.pcm_host)
    same_records(rb, mirror(grid, mode))
    for name in ("win_first", "win_src", "order"):
        assert np.array_equal(getattr(rb, name).cpu().numpy(), getattr(want, name + "_host")), name
    assert np.array_equal(rb.padded(3), want.padded(3))
    rb.check()


@pytest.mark.parametrize("lead", [1, 5])
def test_every_clip_from_every_residue(lead):
    """the clips shifted so that each meets other source residues than in the test above, from an unaligned VIEW of the source, with the
    tables given as device tensors (read back once)"""
    window, stride = pc.GRIDS["small"]
    clips, want = pc.clips_of("small"), pc.reference("small", "rms")
    flat, starts, lens = pc.pack_source(clips, lead)
    big = T(np.concatenate([np.full(3, pc.JUNK), flat]))
    whole, out = guarded(int(want.padded_lengths.sum()))
    rb = ragged.RaggedBatch.from_packed(big[3:], T(starts), T(lens), window, stride, T(pc.noise_of("small")), "rms", out=out)
    torch.cuda.synchronize()
    assert guards_intact(whole, out.numel())
    assert pc.first_difference(rb.pcm.cpu().numpy(), want.pcm_host) is None
    pc.same_tables(rb, want)
    same_records(rb, mirror("small", "rms"))


@pytest.mark.parametrize("grid", ["fsmn", "small"])
def test_the_three_forms_of_pad_noise(grid):
    window, stride = pc.GRIDS[grid]
    clips = pc.clips_of(grid)
    np.random.seed(4321)
    want = ragged.RaggedBatch.from_clips(clips, window, stride, None, pc.PREP["peak"], device=None)
    np.random.seed(4321)
    _, got = packed(clips, window, stride, None, "peak")
    assert pc.first_difference(got, want.pcm_host) is None                # None: numpy's global RNG, the reference's own draws
    ref = pc.reference(grid, "peak")
    z = pc.noise_of(grid)
    _, got = packed(clips, window, stride, [row for row in z], "peak")   # host rows
    assert pc.first_difference(got, ref.pcm_host) is None
    _, got = packed(clips, window, stride, T(z), "peak")                  # a device matrix [B, >= max pad], where it lies
    assert pc.first_difference(got, ref.pcm_host) is None
    one = ragged.RaggedBatch.from_clips(clips, window, stride, np.repeat(z[:1], len(clips), axis=0), pc.PREP["peak"], device=None)
    _, got = packed(clips, window, stride, T(z[:1]), "peak")              # one device row for every clip
    assert pc.first_difference(got, one.pcm_host) is None


def test_a_clip_does_not_depend_on_its_neighbours_or_its_place():
    window, stride = pc.GRIDS["fsmn"]
    clips, z, want = pc.clips_of("fsmn"), pc.noise_of("fsmn"), pc.reference("fsmn", "rms")
    for pick in (list(range(len(clips)))[::-1], [7, 0, 31, 16, 16, 25], [25]):
        rb, got = packed([clips[b] for b in pick], window, stride, z[pick], "rms", lead=2)
        for k, b in enumerate(pick):
            assert np.array_equal(got[rb.clip_off[k]:rb.clip_off[k] + rb.padded_lengths[k]], want.padded(b)), (pick, k)


def test_a_lying_offset_is_refused_and_reads_nothing():
    """clips whose tables point outside the source: a status bit each, zeros for their samples AND their fill (nothing was read, so the
    tail RMS is zero) although the memory around the source view is full of non-zero samples; every other clip as before"""
    window, stride = pc.GRIDS["small"]
    clips, z = pc.clips_of("small"), pc.noise_of("small")
    want = pc.reference("small", "peak")
    flat, starts, lens = pc.pack_source(clips)
    around = T(np.concatenate([np.full(4096, 12345, dtype=np.int16), flat, np.full(4096, 12345, dtype=np.int16)]))
    src = around[4096:4096 + len(flat)]
    lies = {2: -1, 9: -600, 13: len(flat) - int(lens[13]) + 1, 20: len(flat) + 64, 27: 2 ** 40}
    bad_starts = starts.copy()
    for b, v in lies.items():
        bad_starts[b] = v
    whole, out = guarded(int(want.padded_lengths.sum()))
    rb = ragged.RaggedBatch.from_packed(src, bad_starts, lens, window, stride, z, "peak", out=out)
    torch.cuda.synchronize()
    assert guards_intact(whole, out.numel())
    st = rb.prepared.status()
    assert st.tolist() == [prepare.ST_SRC_RANGE if b in lies else 0 for b in range(len(clips))]
    with pytest.raises(ValueError, match="clip 2"):
        rb.check()
    got = rb.pcm.cpu().numpy()
    for b in range(len(clips)):
        mine = got[rb.clip_off[b]:rb.clip_off[b] + rb.padded_lengths[b]]
        assert (not mine.any()) if b in lies else np.array_equal(mine, want.padded(b)), b


def test_guarded_workspace_and_the_raw_launches():
    """prepare_device with a workspace of exactly vadx_prepare_workspace_bytes between guards"""
    window, stride = pc.GRIDS["firered"]
    clips, want = pc.clips_of("firered"), pc.reference("firered", "rms")
    flat, starts, lens = pc.pack_source(clips, 6)
    tiles = int(prepare.chunk_tables(lens)[0][-1])
    need = _lib.lib().vadx_prepare_workspace_bytes(len(clips), tiles)
    ws_whole = torch.full((256 + need + 256,), 0x5B, dtype=torch.uint8, device=DEV)
    pads = want.padded_lengths - want.lengths
    noise, noise_off = prepare.device_noise(pads, pc.noise_of("firered"), torch.device(DEV))
    whole, out = guarded(int(want.padded_lengths.sum()))
    dst_off = np.concatenate([want.clip_off, [want.padded_lengths.sum()]])
    got = prepare.prepare_device(T(flat), starts, lens, dst_off, window, stride, "rms", 8192.0, noise, noise_off, out=out, workspace=ws_whole[256:256 + need])
    torch.cuda.synchronize()
    assert guards_intact(whole, out.numel())
    assert bool((ws_whole[:256] == 0x5B).all()) and bool((ws_whole[256 + need:] == 0x5B).all())
    assert pc.first_difference(got.pcm.cpu().numpy(), want.pcm_host) is None
    assert not got.status().any()


@pytest.mark.parametrize("mode", [None, "rms"])
def test_ragged_frames_from_packed_is_from_clips(mode):
    clips = pc.clips_of("small")
    want = ragged.RaggedFrames.from_clips([c if mode is None else timestamps.normalise_audio(c) for c in clips], device=None)
    flat, starts, lens = pc.pack_source(clips, 3)
    whole, out = guarded(int(lens.sum()))
    rf = ragged.RaggedFrames.from_packed(T(flat), starts, lens, mode, out=out)
    torch.cuda.synchronize()
    assert guards_intact(whole, out.numel())
    for name in ragged.RaggedFrames.TABLES:
        assert np.array_equal(getattr(rf, name).cpu().numpy(), getattr(want, name + "_host")), name
    assert rf.pcm_host is None and (rf.n_mel, rf.n_enc, rf.n_fe_tiles, rf.n_enc_tiles) == (want.n_mel, want.n_enc, want.n_fe_tiles, want.n_enc_tiles)
    assert not rf.prepared.status().any()


# ---- end to end, on the synthetic weights the other suites use --------------------------------------------------------------------------
SEED = 1234
_ENG = {}


def engine(kind):
    if kind not in _ENG:
        _ENG[kind] = {"fsmn": lambda: fsmn.FsmnEngine(weights.fsmn_synthetic(SEED)),
                      "firered": lambda: firered.FireRedEngine(weights.firered_synthetic(SEED, dict(weights.FIRERED_CFG, odim=1))),
                      "marblenet": lambda: marblenet.MarbleNetEngine(weights.marblenet_synthetic(SEED))}[kind]()
    return _ENG[kind]


def speech(lengths, seed):
    return [weights.burst_clips(1, n, seed=seed + k)[0] for k, n in enumerate(lengths)]


def on_device(clips):
    flat, starts, lens = pc.pack_source(clips, 1)
    return T(flat), starts, lens


@pytest.mark.parametrize("gemm", ["f32", "split", "h2"])
def test_fsmn_flags_from_packed_are_the_host_paths(gemm):
    prev = _lib.gemm_mode(gemm)
    try:
        eng = engine("fsmn")
        clips, noise = speech((9000, 16000, 27041, 30000), 700), np.random.default_rng(11).standard_normal((4, 20000))
        want_flags, want_n = eng.flags_ragged(eng.ragged(clips, noise))
        rb = eng.ragged_packed(*on_device(clips), pad_noise=noise)
        flags, n = eng.flags_ragged(rb)
        assert np.array_equal(n, want_n) and torch.equal(flags, want_flags)
        assert eng.detect(rb) == eng.detect(clips, pad_noise=noise)
        assert eng.detect_table(rb).lists() == eng.detect_table(clips, pad_noise=noise).lists()
        assert eng.blobs.mode() == gemm
    finally:
        _lib.gemm_mode(prev)


def test_firered_detect_from_packed_is_the_host_paths():
    eng = engine("firered")
    clips, noise = speech((9000, 16000, 25001, 40000), 800), np.random.default_rng(11).standard_normal((4, 20000))
    want, wtracks, wdecs = eng.detect(clips, pad_noise=noise, return_probs=True)
    got, tracks, decs = eng.detect(eng.ragged_packed(*on_device(clips), pad_noise=noise), return_probs=True)
    assert got == want
    for a, b in zip(tracks + decs, wtracks + wdecs):
        assert torch.equal(a, b)
    assert eng.detect_table(eng.ragged_packed(*on_device(clips), pad_noise=noise)).lists() == want


@pytest.mark.parametrize("window_len", [None, 8000])
def test_marblenet_detect_from_packed_is_the_host_paths(window_len):
    eng = engine("marblenet")
    clips, noise = speech((9000, 16000, 25001, 4000), 900), np.random.default_rng(11).standard_normal((4, 20000))
    want, wtrack, wdec, wnf = eng.detect(clips, window_len=window_len, pad_noise=noise, return_probs=True)
    batch = eng.ragged_packed(*on_device(clips), window_len=window_len, pad_noise=noise)
    assert isinstance(batch, ragged.RaggedFrames if window_len is None else ragged.RaggedBatch)
    got, track, dec, nf = eng.detect(batch, return_probs=True)
    assert got == want and np.array_equal(nf, wnf) and torch.equal(track, wtrack) and torch.equal(dec, wdec)
    assert eng.detect_table(batch).lists() == want


def test_cascade_cut_then_rescore_without_the_host():
    """collect_chunks_batch's packed output goes into from_packed as it is (device offsets and lengths), then FSMN: the result is the host
    path's on the downloaded chunks"""
    eng = engine("fsmn")
    clips = speech((48000, 30000, 52000), 300)
    tables = [[(1000, 20000), (30001, 47000)], [(5, 17003)], [(0, 9000), (20000, 52000)]]
    flat, starts, lens = pc.pack_source(clips)
    segs, counts = (T(a) for a in chunks.table_of(tables))
    cut, offsets, plan = chunks.collect_chunks_batch((segs, counts), T(flat), lengths=T(lens), clip_offsets=T(starts), return_plan=True)
    noise = np.random.default_rng(5).standard_normal((3, 20000))
    got = eng.detect(eng.ragged_packed(cut, offsets[:-1], plan.lengths, pad_noise=noise))
    host, off, n = cut.cpu().numpy(), offsets.cpu().numpy(), plan.lengths.cpu().numpy()
    pieces = [host[off[b]:off[b] + n[b]] for b in range(3)]
    assert [len(p) for p in pieces] == [35999, 16998, 41000]
    assert got == eng.detect(pieces, pad_noise=noise)


# ---- ragged ingest -------------------------------------------------------------------------------------------------------------------
def write_wav(path, samples, channels, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(samples, dtype="<i2").tobytes())
    return str(path)


INGEST_SPEC = [(48000, 2, 1), (48000, 2, 2), (48000, 2, 3), (48000, 2, 1000), (16000, 1, 1), (16000, 1, 1000), (8000, 1, 1), (8000, 1, 2), (8000, 1, 3),
               (8000, 1, 1000), (44100, 2, 4411), (16000, 2, 2049), (48000, 1, 30000)]


def test_ingest_ragged_is_load_wav_per_file(tmp_path):
    rng = np.random.default_rng(8)
    paths = [write_wav(tmp_path / f"c{k}.wav", rng.integers(-32768, 32768, n * ch).astype(np.int16), ch, rate)
             for k, (rate, ch, n) in enumerate(INGEST_SPEC)]
    raws = [audio_io.read_wav_raw(p) for p in paths]
    pcm, offs, lens, status = audio_io.ingest_ragged([r[0] for r in raws], [r[1] for r in raws], [r[2] for r in raws], 16000, DEV, return_status=True)
    host = pcm.cpu().numpy()
    assert not status.cpu().numpy().any()
    mirror_pcm, moffs, mlens = audio_io.ingest_ragged_host([r[0] for r in raws], [r[1] for r in raws], [r[2] for r in raws], 16000)
    assert np.array_equal(offs, moffs) and np.array_equal(lens, mlens) and np.array_equal(host, mirror_pcm)
    for p, o, n in zip(paths, offs, lens):
        want = audio_io.load_wav(p, 16000)
        assert n == len(want) and np.array_equal(host[o:o + n], want), p


def test_ingest_ragged_refuses_per_clip():
    """the C entry point with tables the Python layer would not build: a refused clip is zeros and says so, its neighbours are untouched"""
    rng = np.random.default_rng(9)
    raws = [rng.integers(-3000, 3000, n).astype(np.int16) for n in (2000, 1000, 3000, 500)]
    good, offs, lens = audio_io.ingest_ragged(raws, [1, 2, 1, 1], [8000, 48000, 16000, 44100], 16000, DEV)
    want = good.cpu().numpy()
    B = 4
    src = T(np.concatenate(raws))
    src_off = np.concatenate([[0], np.cumsum([len(r) for r in raws])[:-1]]).astype(np.int64)
    frames = np.asarray([2000, 500, 3000, 500], dtype=np.int64)
    chans, rates = np.asarray([1, 3, 1, 1], dtype=np.int32), np.asarray([8000, 48000, 16000, 44100], dtype=np.int32)
    src_off[2] = len(src) - 2999                                                # one sample past the end
    per = np.maximum((lens + 1023) // 1024, 1)
    i64 = T(np.concatenate([src_off, frames, offs]))
    i32 = T(np.concatenate([chans, rates, np.concatenate([[0], np.cumsum(per)]), np.repeat(np.arange(B), per)]).astype(np.int32))
    whole, out = guarded(int(want.shape[0]))
    out.zero_()
    status = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    p64, p32 = i64.data_ptr(), i32.data_ptr()
    _lib.check(_lib.lib().vadx_ingest_pcm16_ragged(src.data_ptr(), int(src.numel()), p64, p64 + 8 * B, p32, p32 + 4 * B, 16000, p64 + 16 * B, p32 + 8 * B,
                                                   p32 + 4 * (3 * B + 1), B, int(per.sum()), out.data_ptr(), int(out.numel()), status.data_ptr(),
                                                   _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(whole, out.numel())
    assert status.cpu().tolist() == [0, 1, 2, 0]
    got = out.cpu().numpy()
    for b in range(B):
        mine = got[offs[b]:offs[b] + lens[b]]
        assert (not mine.any()) if b in (1, 2) else np.array_equal(mine, want[offs[b]:offs[b] + lens[b]]), b


def test_drivers_with_device_ingest_return_what_the_default_path_returns(tmp_path):
    rng = np.random.default_rng(3)
    spec = [(16000, 1, 40000), (48000, 2, 75000), (8000, 1, 12500), (16000, 1, 16000)]
    paths = []
    for k, (rate, ch, n) in enumerate(spec):
        mono = weights.burst_clips(1, n, seed=500 + k)[0]
        x = mono if ch == 1 else np.stack([mono, (mono // 2 + rng.integers(-50, 50, n)).astype(np.int16)], axis=1).reshape(-1)
        paths.append(write_wav(tmp_path / f"d{k}.wav", x, ch, rate))
    noise = np.random.default_rng(77).standard_normal((len(paths), 20000))
    quiet = lambda *_: None                                                     # noqa: E731
    files = (str(tmp_path / "s.txt"), str(tmp_path / "i.txt"))
    runs = [(drivers.inference_fsmn, engine("fsmn"), {}), (drivers.inference_firered, engine("firered"), {}),
            (drivers.inference_firered, engine("firered"), dict(NORMALIZE_AUDIO=True)), (drivers.inference_marblenet, engine("marblenet"), {}),
            (drivers.inference_marblenet, engine("marblenet"), dict(NORMALIZE_AUDIO=True, INPUT_AUDIO_LENGTH=8000))]
    for run, eng, kw in runs:
        want = run(paths, eng, *files, pad_noise=noise, echo=quiet, **kw)
        got = run(paths, eng, *files, pad_noise=noise, echo=quiet, device_ingest=True, **kw)
        assert got == want and any(want), (run.__name__, kw)
    one = drivers.inference_fsmn(paths[1], engine("fsmn"), *files, pad_noise=noise[1:2], echo=quiet, device_ingest=True)
    assert one == drivers.inference_fsmn(paths[1], engine("fsmn"), *files, pad_noise=noise[1:2], echo=quiet)
