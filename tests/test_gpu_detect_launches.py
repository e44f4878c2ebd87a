"""GPU: the library calls behind every whole-clip `detect`, pinned per path.  FSMN, FireRed (VAD and the AED events) and MarbleNet
(dynamic axis and an 8000-sample window) each run a rectangular [2, 24 000] batch and a list of three clips under `_lib.trace()`; the
entry points called and how often must equal the literal tables below, which `record()` printed at the commit BEFORE the host pipeline
moved into vadx.clips -- so a rectangular batch that got routed through the gather kernels, a launch issued twice or a dropped one
shows here, whatever the results are (the engines are warmed up first: building a front-end table is no part of the sequence).
The list clips are the smallest that take every route: 300 samples (shorter than a FireRed frame: no valid frame; MarbleNet: two
log-mel frames, one encoder frame, which is the dropped last one), 16 000 (exactly one window) and 16 001 (a second window, nearly all
padding).  In passing: clip b of the list result is the [1, N] result of that clip alone, bitwise -- segments, and the return_probs
tensors cut to the clip's frame count."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, firered, fsmn, marblenet, weights

pytestmark = pytest.mark.gpu
SEED, ARITH = 1234, "h2"
LIST_N, RECT = (300, 16000, 16001), (2, 24000)

# printed by record() at the parent commit: {case: (calls of the [2, 24 000] batch, calls of the three-clip list)}
EXPECTED = {
    'fsmn': ({'vadx_frontend_logmel_means': 1, 'vadx_fsmn_clips': 1, 'vadx_fsmn_window_stats': 1},
        {'vadx_frontend_logmel_means': 1, 'vadx_fsmn_clips_ragged': 1, 'vadx_fsmn_window_stats': 1, 'vadx_windows_gather': 1}),
    'firered': ({'vadx_firered_run': 1, 'vadx_frontend_logmel': 1, 'vadx_vadpost': 1},
        {'vadx_firered_run': 1, 'vadx_frontend_logmel': 1, 'vadx_tracks_gather': 1, 'vadx_vadpost': 1, 'vadx_windows_gather': 1}),
    'firered_events': ({'vadx_firered_run': 1, 'vadx_frontend_logmel': 1, 'vadx_vadpost': 3},
        {'vadx_firered_run': 1, 'vadx_frontend_logmel': 1, 'vadx_tracks_gather': 3, 'vadx_vadpost': 3, 'vadx_windows_gather': 1}),
    'marblenet_dynamic': ({'vadx_frontend_logmel': 1, 'vadx_marblenet_block2': 3, 'vadx_marblenet_tail': 1, 'vadx_sepconv_block': 1, 'vadx_vadpost': 1},
        {'vadx_frontend_logmel_ragged': 1, 'vadx_marblenet_block2_ragged': 3, 'vadx_marblenet_tail_ragged': 1, 'vadx_sepconv_block_ragged': 1, 'vadx_tracks_gather': 1, 'vadx_vadpost': 1}),
    'marblenet_8000': ({'vadx_frontend_logmel': 1, 'vadx_marblenet_block2': 3, 'vadx_marblenet_tail': 1, 'vadx_sepconv_block': 1, 'vadx_vadpost': 1},
        {'vadx_frontend_logmel': 1, 'vadx_marblenet_block2': 3, 'vadx_marblenet_tail': 1, 'vadx_sepconv_block': 1, 'vadx_tracks_gather': 1, 'vadx_vadpost': 1, 'vadx_windows_gather': 1}),
}

_CACHE = {}


def _engine(kind):
    if kind not in _CACHE:
        _CACHE[kind] = {"fsmn": lambda: fsmn.FsmnEngine(weights.fsmn_synthetic(SEED)),
                        "firered": lambda: firered.FireRedEngine(weights.firered_synthetic(SEED)),
                        "events": lambda: firered.FireRedEngine(weights.firered_synthetic(SEED, dict(weights.FIRERED_CFG, odim=3))),
                        "marblenet": lambda: marblenet.MarbleNetEngine(weights.marblenet_synthetic(SEED))}[kind]()
    return _CACHE[kind]


def _audio():
    """(rectangular int16 [2, 24 000], the three list clips, padding noise [3, 20 000])"""
    if "audio" not in _CACHE:
        _CACHE["audio"] = (weights.burst_clips(RECT[0], RECT[1], seed=40),
                           [weights.burst_clips(1, n, seed=41 + k)[0] for k, n in enumerate(LIST_N)],
                           np.random.default_rng(42).standard_normal((3, 20000)))
    return _CACHE["audio"]


# case -> (engine kind, detect(engine, clips, pad_noise) with every result the path can return)
CASES = {
    "fsmn": ("fsmn", lambda e, c, nz: e.detect(c, pad_noise=nz)),
    "firered": ("firered", lambda e, c, nz: e.detect(c, pad_noise=nz, return_probs=True)),
    "firered_events": ("events", lambda e, c, nz: e.detect_events(c, pad_noise=nz, return_probs=True)),
    "marblenet_dynamic": ("marblenet", lambda e, c, nz: e.detect(c, pad_noise=nz, return_probs=True)),
    "marblenet_8000": ("marblenet", lambda e, c, nz: e.detect(c, window_len=8000, pad_noise=nz, return_probs=True)),
}


def _traced(case):
    """((calls, result) of the rectangular batch, (calls, result) of the list) on one arithmetic"""
    kind, detect = CASES[case]
    eng, (rect, clips, noise) = _engine(kind), _audio()
    prev = _lib.gemm_mode(ARITH)
    try:
        out = []
        for audio, nz in ((rect, noise[:2]), (clips, noise)):
            detect(eng, audio, nz)              # builds and caches the per-length front-end tables, outside the trace
            with _lib.trace() as tr:
                res = detect(eng, audio, nz)
            out.append((dict(sorted(tr.calls.items())), res))
        return out
    finally:
        _lib.gemm_mode(prev)


def record():
    """Prints the EXPECTED table of the tree it runs in."""
    print("EXPECTED = {")
    for case in CASES:
        (rect, _), (lst, _) = _traced(case)
        print(f"    {case!r}: ({rect!r},\n        {lst!r}),")
    print("}")


def _cut(case, res, b):
    """Clip b of a detect result as (segments or events, [tensors cut to the clip's frames]): the list forms and the [B, N] forms of
    every model brought to one shape."""
    if case == "fsmn":
        return res[b], []
    out, rest = res[0], res[1:]
    if case == "firered_events":                       # list: per clip [odim, n_b]; array: [B, odim, n]
        return out[b], [rest[0][b]]
    if case == "firered":                              # list: per-clip lists; array: [B, n] tensors (no decisions without a valid frame)
        return out[b], [r[b] for r in rest]
    n = int(rest[2][b]) if len(rest) == 3 else rest[0].shape[1]        # MarbleNet's list form carries n_frames
    return out[b], [r[b, :n] for r in rest[:2]]


@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence_and_one_clip_identity(case):
    kind, detect = CASES[case]
    (rect_calls, rect_res), (list_calls, list_res) = _traced(case)
    print(case, rect_calls, list_calls)
    assert (rect_calls, list_calls) == EXPECTED[case]
    assert len(rect_res if case == "fsmn" else rect_res[0]) == RECT[0]
    eng, (_, clips, noise) = _engine(kind), _audio()
    prev = _lib.gemm_mode(ARITH)
    try:
        for b, c in enumerate(clips):
            alone = detect(eng, c[None, :], noise[b:b + 1])
            got, want = _cut(case, list_res, b), _cut(case, alone, 0)
            assert got[0] == want[0], b
            assert len(got[1]) >= len(want[1]) > 0 or case == "fsmn", b
            for g, w in zip(got[1], want[1]):
                assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), b
    finally:
        _lib.gemm_mode(prev)
