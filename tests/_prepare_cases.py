"""The input set tests/test_prepare_cpu.py and tests/test_gpu_prepare.py share: clips at every length where vadx.prepare takes another path,
four kinds of signal, laid into one source vector at every residue of a 16-byte vector -- and the host reference every comparison is made
against, `RaggedBatch.from_clips(..., device=None)`, built once per (grid, mode)."""
import functools

import numpy as np

import vadx  # noqa: F401
from vadx import ragged, timestamps

GRIDS = {"fsmn": (16000, 11040), "firered": (16000, 16000), "small": (512, 256)}
MODES = [None, "peak", "rms"]
PREP = {None: None, "peak": lambda a: timestamps.normalize_to_int16(a.astype(np.float32)), "rms": timestamps.normalise_audio}
JUNK = np.int16(-3)                    # what lies between the clips of a packed source


def lengths_of(window, stride):
    """1, 7, 8, 9, 127 .. 129 and the grid's edges; window + 1 has a pad of stride - 1 samples taken from its own tail, which on the two
    16000-sample grids crosses an 8192 chunk; 8191 .. 8193, 16385, 24577: the chunk edges of the whole-clip sums."""
    edge = [window - 1, window, window + 1, window + stride - 1, window + stride, window + stride + 1]
    return [1, 7, 8, 9, 127, 128, 129] + edge + [8191, 8192, 8193, 16385, 24577]


def signal(kind, n, rng):
    if kind == "silence":
        return np.zeros(n, dtype=np.int16)
    if kind == "lone":
        x = np.zeros(n, dtype=np.int16)
        x[n // 2] = -32768
        return x
    if kind == "quiet":
        return rng.integers(-30, 31, n).astype(np.int16)
    return rng.integers(-32768, 32768, n).astype(np.int16)           # full scale


KINDS = ["full", "quiet", "silence", "lone"]


@functools.lru_cache(maxsize=None)
def clips_of(grid):
    """every length with a full-scale and a quiet signal, silence and the lone -32768 at a few"""
    window, stride = GRIDS[grid]
    rng = np.random.default_rng(20240 + window + stride)
    clips = []
    for i, n in enumerate(lengths_of(window, stride)):
        clips.append(signal("full", n, rng))
        clips.append(signal(KINDS[1 + i % 3], n, rng))
    return clips


@functools.lru_cache(maxsize=None)
def noise_of(grid):
    """standard-normal rows [B, max(window, stride)], two samples pushed out to +-40 so that the fill wraps around int16"""
    window, stride = GRIDS[grid]
    z = np.random.default_rng(77 + window).standard_normal((len(clips_of(grid)), max(window, stride)))
    z[:, 3], z[:, 5] = 40.0, -39.5
    return z


def pack_source(clips, lead=0):
    """The clips in one vector, clip i starting at residue (lead + i) % 8 of a 16-byte vector, JUNK between them and at both ends.
    -> (flat int16, starts int64, lengths int64)"""
    starts, at = [], 8 + lead
    for i, c in enumerate(clips):
        at += (lead + i - at) % 8
        starts.append(at)
        at += len(c) + 1
    flat = np.full(at + 11, JUNK, dtype=np.int16)
    for s, c in zip(starts, clips):
        flat[s:s + len(c)] = c
    return flat, np.asarray(starts, dtype=np.int64), np.asarray([len(c) for c in clips], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def reference(grid, mode):
    """RaggedBatch.from_clips(device=None) of the grid's clips with the grid's noise: never changed by a test"""
    window, stride = GRIDS[grid]
    rb = ragged.RaggedBatch.from_clips(clips_of(grid), window, stride, noise_of(grid), PREP[mode], device=None)
    rb.pcm_host.setflags(write=False)
    return rb


TABLES = ("lengths", "padded_lengths", "windows", "clip_off", "win_first_host", "win_src_host", "order_host")


def same_tables(a, b):
    for name in TABLES:
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert (a.window, a.stride, a.n_windows, a.max_windows) == (b.window, b.stride, b.n_windows, b.max_windows)


def first_difference(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(got != want)
    return None if bad.size == 0 else f"{bad.size} elements differ, first at {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"
