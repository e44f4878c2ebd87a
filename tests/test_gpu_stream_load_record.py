"""GPU: `load_record` as Silero's and MarbleNet's stream batches inherit it from vadx.stream.StreamBatch.  Their records hold all of a
stream's state, so a fresh batch that loads a copy taken mid-stream must go on exactly as the batch the copy was taken from: the same
outputs and the same record after the next tick, byte for byte (the pattern of test_gpu_fsmn_stream.py's recomputed tick)."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import marblenet, silero, weights

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_silero_continues_from_a_loaded_record():
    S, k = 17, 2                                                          # one full group of sixteen streams and one more
    eng = silero.SileroEngine(weights.silero_synthetic(1234))
    x = weights.burst_clips(S, 3 * k * 512, seed=11)
    ticks = [x[:, j * k * 512:(j + 1) * k * 512] for j in range(3)]
    it = silero.VADIteratorBatch(eng, S)
    it.step(ticks[0])
    it.step(ticks[1])
    saved = it.record.clone()
    want = it.step(ticks[2])
    again = silero.VADIteratorBatch(eng, S)
    assert saved.any() and not again.record.any()
    again.reset_states([3])                                               # a request from before the load does not outlive it
    again.load_record(saved)
    got = again.step(ticks[2])
    torch.cuda.synchronize()
    assert torch.isfinite(want[2]).all()
    assert all(same_bytes(a, b) for a, b in zip(want, got))               # kind, value, probs
    assert torch.equal(it.record, again.record) and torch.equal(it.state, again.state)
    assert not torch.equal(it.record, saved)


def test_marblenet_continues_from_a_loaded_record():
    S, k = 2, 4
    eng = marblenet.MarbleNetEngine(weights.marblenet_synthetic(1234))
    rng = np.random.default_rng(5)
    ticks = [np.clip(np.rint(rng.standard_normal((S, k * 320)) * 8000), -32768, 32767).astype(np.int16) for _ in range(3)]
    sb = marblenet.MarbleNetStreamBatch(eng, S)
    sb.step(ticks[0])
    sb.step(ticks[1])
    assert sb.fed.tolist() == [2 * k * 320] * S and sb.emitted.tolist() == [0] * S      # mid-stream: audio in, no stream final yet
    saved = sb.record.clone().cpu().numpy()                               # a host copy, as a caller would keep it
    want = sb.step(ticks[2], final=[True, False])
    again = marblenet.MarbleNetStreamBatch(eng, S)
    again.reset_states()
    again.load_record(saved)
    assert again.fed.tolist() == [2 * k * 320] * S
    got = again.step(ticks[2], final=[True, False])
    torch.cuda.synchronize()
    assert want[2].tolist() == [3 * k, 0]                                 # stream 0 ends: all of its 12 frames; stream 1 is still behind its audio
    assert torch.isfinite(want[0][0, :3 * k]).all()
    assert all(same_bytes(a, b) for a, b in zip(want, got))               # score_silence, score_active (NaN behind n_out), n_out
    assert torch.equal(sb.record, again.record)
    assert same_bytes(sb.stream_bytes(1), again.stream_bytes(1)) and sb.fed.tolist() == again.fed.tolist() == [0, 3 * k * 320]
