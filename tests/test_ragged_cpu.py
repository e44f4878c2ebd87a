"""CPU: the ragged-batch entry points (vadx_windows_gather, vadx_fsmn_clips_ragged, vadx_tracks_gather) exist under the unchanged ABI
number and refuse bad arguments on the host before any device call; vadx.ragged.RaggedBatch packs clips of any lengths exactly as
`pad_to_window_grid` pads each of them, on 16-byte boundaries, with the window tables the header documents."""
import ctypes as C
import re

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, clips, fsmn, ragged, timestamps, weights

L, T = 16000, 101
NAMES = ("vadx_windows_gather", "vadx_fsmn_clips_ragged", "vadx_tracks_gather")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_and_abi(lib):
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    header = int(re.search(r"^#define\s+VADX_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M).group(1))
    assert lib.vadx_abi_version() == header == _lib.ABI_VERSION
    for name in NAMES:                                                   # declared, and recorded in the ABI history comment
        assert len(re.findall(r"\b%s\b" % name, text)) >= 2, name


def _dims():
    w = weights.fsmn_synthetic(1234)
    d = _lib.FsmnDims()
    d.input_affine_dim, d.linear_dim = w["in1_w"].shape[0], w["in2_w"].shape[0]
    d.output_affine_dim, d.output_dim = w["out1_w"].shape[0], w["out2_w"].shape[0]
    d.frames, d.speech_2_noise_ratio, d.arithmetic = T, 1.0, _lib.ARITH["split"]
    return d


def _loop_params(lb=30):
    lp = _lib.FsmnLoopParams()
    lp.look_backward, lp.one_minus_speech_threshold, lp.noise_db_init, lp.snr_threshold = lb, 1.0, 4.0, 1.0
    lp.speaking_score, lp.silence_score = 0.5, 0.5
    return lp


def test_bad_arguments_are_refused_on_the_host(lib):
    """Every refusal the header lists comes back as VADX_EINVAL with the function's name in vadx_last_error() -- before any HIP call
    (there is no device here; the pointers below are host memory nothing may touch)."""
    buf = (C.c_char * 256)()
    ptr = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731

    gather = lambda **kw: lib.vadx_windows_gather(*[kw.get(k, v) for k, v in (                                         # noqa: E731
        ("pcm", ptr), ("pcm_len", 16000), ("win_src", ptr), ("n_windows", 1), ("window_len", L), ("window_buf", ptr), ("stream", None))])
    for k in ("pcm", "win_src", "window_buf"):
        assert gather(**{k: None}) == -1 and b"vadx_windows_gather" in err() and b"NULL" in err(), k
    for k, bad in (("n_windows", 0), ("n_windows", -3), ("pcm_len", 0), ("window_len", 0), ("window_len", -8), ("window_len", 16004),
                   ("pcm", ptr + 2), ("window_buf", ptr + 8), ("win_src", ptr + 4)):
        assert gather(**{k: bad}) == -1 and b"vadx_windows_gather" in err(), (k, bad)

    d, lp, slide = _dims(), _loop_params(30), T - 30
    run = lambda **kw: lib.vadx_fsmn_clips_ragged(*[kw.get(k, v) for k, v in (                                         # noqa: E731
        ("dims", C.byref(d)), ("packed", ptr), ("logmel", ptr), ("db", ptr), ("batch", 2), ("n_windows", 5), ("max_windows", 4),
        ("win_first", ptr), ("order", None), ("lp", C.byref(lp)), ("cache_ws", ptr), ("flags", ptr), ("flag_stride", 4 * slide + 30),
        ("noise_trace", None), ("stream", None))])
    for k in ("dims", "packed", "logmel", "db", "win_first", "lp", "cache_ws", "flags"):
        assert run(**{k: None}) == -1 and b"vadx_fsmn_clips_ragged" in err() and b"NULL" in err(), k
    for k in ("batch", "n_windows", "max_windows"):
        for bad in (0, -1):
            assert run(**{k: bad}) == -1 and b"vadx_fsmn_clips_ragged" in err() and k.encode() in err(), (k, bad)
    assert run(flag_stride=4 * slide + 29) == -1 and b"vadx_fsmn_clips_ragged" in err() and b"flag_stride" in err()
    assert run(flag_stride=0) == -1 and b"flag_stride" in err()
    for bad in (-1, T, T + 7):
        assert run(lp=C.byref(_loop_params(bad))) == -1 and b"vadx_fsmn_clips_ragged" in err() and b"look_backward" in err(), bad
    # look-back 0: slide = T, no tail -> max_windows * T flags
    assert run(lp=C.byref(_loop_params(0)), flag_stride=4 * T - 1) == -1 and b"flag_stride" in err()

    tracks = lambda **kw: lib.vadx_tracks_gather(*[kw.get(k, v) for k, v in (                                          # noqa: E731
        ("probs", ptr), ("win_floats", 3 * 98), ("chan_offset", 98), ("frames_per_window", 98), ("win_first", ptr), ("n_frames", ptr),
        ("batch", 2), ("tracks", ptr), ("track_stride", 248), ("stream", None))])
    for k in ("probs", "win_first", "n_frames", "tracks"):
        assert tracks(**{k: None}) == -1 and b"vadx_tracks_gather" in err() and b"NULL" in err(), k
    for k, bad in (("batch", 0), ("track_stride", 0), ("frames_per_window", 0), ("chan_offset", -1), ("chan_offset", 2 * 98 + 1),
                   ("win_floats", 97)):
        assert tracks(**{k: bad}) == -1 and b"vadx_tracks_gather" in err(), (k, bad)


LENGTHS = (9000, 16000, 27040, 30000, 45000, 16001, 72345)


def _clips():
    return [weights.burst_clips(1, n, seed=700 + k)[0] for k, n in enumerate(LENGTHS)]


@pytest.mark.parametrize("window,stride,prep", [(L, 11040, True), (L, 15840, True), (L, L, False)])
def test_packing_against_numpy(window, stride, prep):
    """Host mode (device=None): the tables are numpy arrays, nothing is uploaded."""
    clips = _clips()
    noise = np.random.default_rng(11).standard_normal((len(clips), 20000))
    fn = (lambda a: timestamps.normalize_to_int16(a.astype(np.float32))) if prep else None
    rb = ragged.RaggedBatch.from_clips(clips, window, stride, noise, fn, device=None)
    want = [fsmn.pad_to_window_grid(fn(c) if fn else c, window, stride, noise[b]) for b, c in enumerate(clips)]
    assert len(rb) == len(clips) and rb.device is None and rb.pcm.dtype == np.int16 and rb.pcm.ndim == 1
    assert np.array_equal(rb.lengths, LENGTHS)
    W = np.array([(len(p) - window) // stride + 1 for p in want])
    assert np.array_equal(rb.windows, W) and rb.windows.dtype == np.int32
    assert rb.n_windows == W.sum() and rb.max_windows == W.max()
    end = 0
    for b, p in enumerate(want):
        off = int(rb.clip_off[b])
        assert off % 8 == 0 and off >= end, b                            # 16-byte boundary, no overlap with the previous clip
        assert np.array_equal(rb.pcm[off:off + len(p)], p) and np.array_equal(rb.padded(b), p), b
        end = off + len(p)
    assert end <= rb.pcm.shape[0]
    assert rb.win_first.dtype == np.int32 and np.array_equal(rb.win_first, np.concatenate([[0], np.cumsum(W)]))
    assert rb.win_src.dtype == np.int64 and rb.win_src.shape == (W.sum(),)
    for b in range(len(clips)):
        for k in range(W[b]):
            src = int(rb.win_src[rb.win_first[b] + k])
            assert src == rb.clip_off[b] + k * stride and src % 8 == 0 and src + window <= rb.pcm.shape[0]
            assert np.array_equal(rb.pcm[src:src + window], want[b][k * stride:k * stride + window])
    # longest first, ties in input order
    assert rb.order.dtype == np.int32 and sorted(rb.order.tolist()) == list(range(len(clips)))
    keyed = sorted(range(len(clips)), key=lambda b: (-W[b], b))
    assert rb.order.tolist() == keyed


def test_packing_takes_noise_rows_as_a_list_and_refuses_bad_input():
    clips = _clips()[:3]
    rows = [np.random.default_rng(k).standard_normal(7000 + 1000 * k) for k in range(3)]      # ragged rows, each >= its clip's pad
    rb = ragged.RaggedBatch.from_clips(clips, L, L, rows, device=None)
    for b, c in enumerate(clips):
        assert np.array_equal(rb.padded(b), fsmn.pad_to_window_grid(c, L, L, rows[b])), b
    with pytest.raises(ValueError, match="multiples of 8"):
        ragged.RaggedBatch.from_clips(clips, 16001, 16001, rows, device=None)
    with pytest.raises(ValueError, match="at least one"):
        ragged.RaggedBatch.from_clips([], L, L, device=None)
    with pytest.raises(ValueError, match="int16"):
        ragged.RaggedBatch.from_clips([c.astype(np.float32) for c in clips], L, L, rows, device=None)
    with pytest.raises(ValueError, match="empty"):
        ragged.RaggedBatch.from_clips([clips[0][:0]], L, L, rows, device=None)
    with pytest.raises(ValueError, match="rows"):
        ragged.RaggedBatch.from_clips(clips, L, L, rows[:2], device=None)
    with pytest.raises(ValueError, match="host-only"):
        rb.gather()


# ------------------------------------------------------------------------------------------------------- the whole-clip host pipeline
@pytest.mark.parametrize("window,stride,prep", [(L, 11040, True), (L, 11040, False), (L, L, False), (8000, 8000, False)])
@pytest.mark.parametrize("n", [9000, 16000, 27040, 30000])
def test_pad_batch_is_the_stack_of_padded_rows(window, stride, prep, n):
    """A clip shorter than the window, of exactly one window, exactly on the FSMN grid (16000 + 11040) and with a remainder; the FSMN
    grid with and without its peak normalisation, an L, L grid; a given noise matrix."""
    batch = weights.burst_clips(3, n, seed=900 + n % 7)
    noise = np.random.default_rng(12).standard_normal((3, 20000))
    fn = (lambda a: timestamps.normalize_to_int16(a.astype(np.float32))) if prep else None
    padded, W = clips.pad_batch(batch, window, stride, noise, fn)
    want = np.stack([fsmn.pad_to_window_grid(fn(batch[b]) if fn else batch[b], window, stride, noise[b]) for b in range(3)])
    assert padded.dtype == np.int16 and np.array_equal(padded, want)
    assert W == (padded.shape[1] - window) // stride + 1 == max(0, -(-(n - window) // stride)) + 1
    assert (W - 1) * stride + window == padded.shape[1]                  # the last window ends with the padded clip
    assert np.array_equal(padded[:, :n], np.stack([fn(batch[b]) for b in range(3)]) if fn else batch)
    with pytest.raises(ValueError):
        clips.pad_batch(batch[0], window, stride, noise)                 # one 1-D clip is not a batch


def test_pad_batch_without_noise_draws_like_the_reference():
    batch = weights.burst_clips(2, 9000, seed=3)
    np.random.seed(5)
    padded, W = clips.pad_batch(batch, L, L)
    np.random.seed(5)
    assert W == 1 and np.array_equal(padded, np.stack([fsmn.pad_to_window_grid(batch[b], L, L) for b in range(2)]))


def test_the_moved_names_still_resolve():
    from vadx import session
    assert fsmn.pad_to_window_grid is clips.pad_to_window_grid and ragged.pad_to_window_grid is clips.pad_to_window_grid
    assert fsmn._Meta is session._Meta
    assert not hasattr(ragged, "fsmn")
    assert session.io_types("float16") == (np.float16, "tensor(float16)") and session.io_types("float32") == (np.float32, "tensor(float)")
    with pytest.raises(ValueError, match="io_dtype must be 'float32' or 'float16'"):
        session.io_types("bfloat16")


class _StubEngine:
    """Stands where an engine stands in a driver call: records what `detect` receives; a clip's result names its first sample and the
    first value of the noise row it was given, so a result that lost its clip or its noise row shows."""

    def __init__(self):
        self.seen = []

    def detect(self, audio, pad_noise=None, **kw):
        self.seen.append((audio, pad_noise, kw))
        return [[(float(abs(int(c[0]))), float(abs(int(c[0]))) + abs(float(pad_noise[b][0])))] for b, c in enumerate(audio)]


def _wavs(tmp_path, lengths):
    import wave
    paths = []
    for k, n in enumerate(lengths):
        pth = str(tmp_path / f"c{k}.wav")
        a = weights.burst_clips(1, n, seed=600 + k)[0]
        a[0] = 100 + k                                                    # the first sample names the clip
        with wave.open(pth, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(a.tobytes())         # noqa: E702
        paths.append(pth)
    return paths


@pytest.mark.parametrize("driver,kw", [("inference_fsmn", {}), ("inference_firered", {}), ("inference_marblenet", {}),
                                       ("inference_marblenet", {"INPUT_AUDIO_LENGTH": 8000})])
def test_driver_skeleton_with_a_stub_engine(tmp_path, driver, kw):
    from vadx import drivers
    run = getattr(drivers, driver)
    lengths = [4000, 2500, 4000]
    paths = _wavs(tmp_path, lengths)
    noise = np.random.default_rng(13).standard_normal((3, 50))
    files = (str(tmp_path / "s.txt"), str(tmp_path / "i.txt"))
    quiet = lambda *_: None                                                                                               # noqa: E731
    # a list of three files of different lengths reaches detect once, as a list
    eng = _StubEngine()
    many = run(paths, eng, *files, pad_noise=noise, echo=quiet, **kw)
    assert len(eng.seen) == 1
    audio, nz, passed = eng.seen[0]
    assert isinstance(audio, list) and [a.shape for a in audio] == [(n,) for n in lengths] and nz is noise
    assert [int(a[0]) for a in audio] == [100, 101, 102]
    assert passed.get("window_len", None) == kw.get("INPUT_AUDIO_LENGTH")
    assert [m[0][0] for m in many] == [100.0, 101.0, 102.0]
    assert [m[0][1] - m[0][0] for m in many] == pytest.approx(np.abs(noise[:, 0]))
    # a single path reaches detect as a [1, N] array, its noise as one row; the result is the clip's, not a list of one
    for k, pth in enumerate(paths):
        eng = _StubEngine()
        one = run(pth, eng, *files, pad_noise=noise[k:k + 1], echo=quiet, **kw)
        audio, nz, _ = eng.seen[0]
        assert len(eng.seen) == 1 and isinstance(audio, np.ndarray) and audio.shape == (1, lengths[k]) and nz.shape == (1, 50)
        assert one == many[k]                                             # two equal-length files one at a time: the same, in input order
    # the length groups of `_grouped`: clips 0 and 2 share one [2, N] batch, their noise rows follow them; results in input order
    eng = _StubEngine()
    loaded = drivers._load(paths)
    got = drivers._detect_files(lambda c, z: eng.detect(c, pad_noise=z), loaded, False, [noise[0], noise[1][:30], noise[2][:40]])
    assert got == many and [s[0].shape for s in eng.seen] == [(2, 4000), (1, 2500)]
    assert [s[1].shape for s in eng.seen] == [(2, 40), (1, 30)]           # ragged rows are trimmed to the group's shortest
    assert np.array_equal(eng.seen[0][1], np.stack([noise[0][:40], noise[2][:40]]))
    assert drivers._detect_files(lambda c, z: eng.detect(c, pad_noise=z), loaded, True, noise) == many
    assert drivers._engine_of(dict, eng) is eng and drivers._engine_of(dict, {"a": 1}) == {"a": 1}
