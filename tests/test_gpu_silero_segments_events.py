"""The device segmenter feeds its state machine only the windows at which it can act (csrc/silero.hip: silero_segments_kernel, one clip per
wave, the threshold masks from ballots).  Every segment table must still be exactly what the plain loop over all windows gives:
oracle.postproc.silero_segments, compared without tolerance over track kinds and parameters chosen to reach every branch of the state machine
and every edge of the walk (chunks of 64 windows, clips shorter than the score rows, tables that overflow their capacity)."""
import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import silero, weights
from oracle import postproc as opp

pytestmark = pytest.mark.gpu

B = 70
STEPS = [1, 63, 64, 65, 129, 313, 400]          # around the 64-window chunk, the benchmark's 313, and test_device_segmenter_batch_and_capacity's 400
INF = float("inf")
PARAMS = [
    dict(),
    dict(min_speech_duration_ms=30, min_silence_duration_ms=30, max_speech_duration_s=3),
    dict(max_speech_duration_s=0.2, speech_pad_ms=0),
    dict(max_speech_duration_s=0.2, speech_pad_ms=200, min_silence_duration_ms=0),          # max_speech below zero: every window is past it
    dict(max_speech_duration_s=1, use_max_poss_sil_at_max_speech=False, min_silence_duration_ms=0, min_speech_duration_ms=0),
    dict(max_speech_duration_s=1, min_silence_duration_ms=500, min_silence_at_max_speech=30, speech_pad_ms=0),
    dict(max_speech_duration_s=2, use_max_poss_sil_at_max_speech=False, min_silence_duration_ms=2000, min_silence_at_max_speech=64),
    dict(max_speech_duration_s=1.5, use_max_poss_sil_at_max_speech=False, min_silence_duration_ms=700, speech_pad_ms=200),
    dict(neg_threshold=0.5),                                                                  # neg_threshold at the threshold
    dict(neg_threshold=0.7, max_speech_duration_s=1.5, min_silence_duration_ms=60),           # ... and above it
    dict(min_silence_duration_ms=2000, speech_pad_ms=200),
    dict(threshold=0.3, min_speech_duration_ms=0, speech_pad_ms=200, max_speech_duration_s=0.5, use_max_poss_sil_at_max_speech=False),
    dict(threshold=0.8, neg_threshold=0.8, min_silence_duration_ms=0, min_speech_duration_ms=0, speech_pad_ms=0),
    dict(max_speech_duration_s=3, min_silence_duration_ms=300, min_silence_at_max_speech=0),
]
KINDS = ["noise", "bursts", "ulp", "alternating", "nan", "slow"]


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234))


def _bursts(rng, n):
    out = np.empty(0, dtype=np.float32)
    hi = bool(rng.integers(0, 2))
    while out.shape[0] < n:
        m = int(rng.integers(1, 41))
        seg = rng.uniform(0.75, 1.0, m) if hi else rng.uniform(0.0, 0.2, m)
        out = np.concatenate((out, seg.astype(np.float32)))
        hi = not hi
    return out[:n]


def _tracks(rng, steps, thr, neg):
    """[B, steps] float32 scores: rows 0..2 all zero / all one / all NaN, then the kinds in turn"""
    p = np.empty((B, steps), dtype=np.float32)
    t32, n32 = np.float32(thr), np.float32(neg)
    edge = np.array([np.nextafter(t32, np.float32(-1)), t32, np.nextafter(t32, np.float32(2)),
                     np.nextafter(n32, np.float32(-1)), n32, np.nextafter(n32, np.float32(2)), 0.0, 1.0], dtype=np.float32)
    kinds = []
    for b in range(B):
        kind = ["zero", "one", "allnan"][b] if b < 3 else KINDS[(b - 3) % len(KINDS)]
        kinds.append(kind)
        if kind == "zero":
            p[b] = 0.0
        elif kind == "one":
            p[b] = 1.0
        elif kind == "allnan":
            p[b] = np.nan
        elif kind == "noise":
            p[b] = rng.uniform(0, 1, steps)
        elif kind == "bursts":
            p[b] = _bursts(rng, steps)
        elif kind == "ulp":                      # one ulp either side of both thresholds, in runs of 1..6 windows
            p[b] = np.repeat(edge[rng.integers(0, edge.shape[0], steps)], rng.integers(1, 7, steps))[:steps]
        elif kind == "alternating":
            p[b] = np.where((np.arange(steps) + b) % 2 == 0, 0.9, 0.1)
        elif kind == "nan":
            p[b] = _bursts(rng, steps)
            p[b, rng.uniform(0, 1, steps) < 0.15] = np.nan
        else:                                    # long stretches of speech with dips that stay above / fall below neg_threshold
            p[b] = np.clip(0.8 + 0.25 * np.sin(np.arange(steps) * rng.uniform(0.02, 0.3) + b) + rng.normal(0, 0.12, steps), 0, 1)
    return p, kinds


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("case", range(len(PARAMS)))
def test_event_walk_is_the_plain_loop(engine, case, steps):
    kw = dict(PARAMS[case])
    sr = 8000 if case % 3 == 2 else 16000        # a third of the parameter sets on the 8 kHz window (256 samples)
    kw["sampling_rate"] = sr
    win = 512 if sr == 16000 else 256
    thr = kw.get("threshold", 0.5)
    neg = kw.get("neg_threshold", max(thr - 0.15, 0.01))
    rng = np.random.default_rng(1000 * case + steps)
    probs, kinds = _tracks(rng, steps, thr, neg)
    lens = rng.integers(1, steps * win + 1, B)   # clips may end anywhere in the score row: windows past the clip's end are not read
    lens[:12] = steps * win - rng.integers(0, win, 12)
    segs, counts = engine.segments(probs, lens, cap=2, **kw)     # cap too small on purpose: counts keep counting, the engine re-runs
    got = silero._finish(segs, counts, lens, sr, False, 1, 1)
    for b in range(B):
        nwin = min(steps, (int(lens[b]) + win - 1) // win)
        want = opp.silero_segments([float(v) for v in probs[b, :nwin]], int(lens[b]), **kw)
        assert got[b] == [{"start": d["start"], "end": d["end"]} for d in want], (b, kinds[b], int(lens[b]), kw)
    assert got[0] == [] and got[2] == []
