"""vadx.silero.VADIterator (host drop-in for the reference's stream iterator, utils_vad.py:494-586) against what the REFERENCE iterator
returned on scripted scores (tests/golden/silero_iterator.npz, part (a)): call for call, in samples and in seconds, across a reset.  No
GPU: the model is a stand-in that replays the scores."""
import os

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import silero

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silero_iterator.npz")


class Replay:
    def __init__(self, probs):
        self.probs, self.i, self.resets = probs, 0, 0

    def reset_states(self):
        self.resets += 1

    def __call__(self, chunk, sr):
        v = self.probs[self.i]
        self.i += 1
        return torch.tensor([[v]], dtype=torch.float32)


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def run_track(g, i, **kw):
    p = g[f"a{i}_probs"]
    thr, min_sil, pad = g[f"a{i}_params"].tolist()
    reset_at = int(g[f"a{i}_reset_at"])
    model = Replay([float(v) for v in p])
    vi = silero.VADIterator(model, threshold=thr, sampling_rate=16000, min_silence_duration_ms=min_sil, speech_pad_ms=pad)
    res = []
    for n in range(len(p)):
        if n == reset_at:
            vi.reset_states()
        res.append(vi(torch.zeros(512), **kw))
    return res, model


def table(res):
    kind = np.array([0 if r is None else (1 if "start" in r else 2) for r in res], dtype=np.int8)
    val = np.array([np.nan if r is None else r.get("start", r.get("end")) for r in res])
    return kind, val


@pytest.mark.parametrize("tag,kw", [("samples", {}), ("s1", dict(return_seconds=True, time_resolution=1)),
                                    ("s3", dict(return_seconds=True, time_resolution=3))])
def test_host_iterator_matches_reference_calls(g, tag, kw):
    n_tracks = int(g["a_tracks"])
    assert n_tracks >= 16
    events = 0
    for i in range(n_tracks):
        res, model = run_track(g, i, **kw)
        kind, val = table(res)
        assert np.array_equal(kind, g[f"a{i}_kind"]), i
        assert np.array_equal(val, g[f"a{i}_{tag}"], equal_nan=True), i
        if tag == "samples":                       # int() positions, as the reference returns them
            assert all(type(v) is int for r in res if r for v in r.values())
        assert model.resets == 1 + (int(g[f"a{i}_reset_at"]) >= 0)
        events += int((kind != 0).sum())
    assert events > 100


def test_fixture_covers_the_edges(g):
    """The tracks hold scores at both thresholds, a reset, a non-integral pad (non-integral positions before int())."""
    pads = {float(g[f"a{i}_params"][2]) for i in range(int(g["a_tracks"]))}
    assert 0.0 in pads and 30.03 in pads
    assert any(int(g[f"a{i}_reset_at"]) >= 0 for i in range(int(g["a_tracks"])))
    for i in range(int(g["a_tracks"])):
        thr = float(g[f"a{i}_params"][0])
        p = g[f"a{i}_probs"]
        assert (p == np.float32(thr)).any() and (p == np.float32(thr - 0.15)).any()


def test_host_iterator_errors():
    m = Replay([0.0])
    with pytest.raises(ValueError, match="does not support sampling rates"):
        silero.VADIterator(m, sampling_rate=44100)
    vi = silero.VADIterator(m)
    with pytest.raises(TypeError, match="Audio cannot be casted to tensor"):
        vi(object())
    # 8000 Hz is accepted by the iterator itself (the model decides), windows of 256 samples
    vi8 = silero.VADIterator(Replay([0.9, 0.0]), sampling_rate=8000, min_silence_duration_ms=0)
    assert vi8(np.zeros(256, dtype=np.float32)) == {"start": 0}
    assert vi8(np.zeros(256, dtype=np.float32)) == {"end": 512 + 240 - 256}     # temp_end = 512, pad 240, window 256
