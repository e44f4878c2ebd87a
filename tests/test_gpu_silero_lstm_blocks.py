"""silero_lstm_h2_kernel keeps the decoder's partial sums in an LDS ring and writes the scores in blocks of 16 steps (csrc/silero_h2.hip).
Clip lengths on either side of a block, batches on either side of a 16-clip group; the scores against the oracle at test_gpu_silero.py's
tolerance, bitwise against the span-by-span schedule (which flushes after every span and carries the state between launches), and the
NaN overwrite of a clip group that left the fp16 range, which must land after the last block of scores."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, silero, weights
from oracle import silero as osil

pytestmark = pytest.mark.gpu
ATOL = 1e-4                                      # test_gpu_silero.py::test_clips_match_oracle
STEPS = [1, 15, 16, 17, 33, 47]
BATCHES = [1, 16, 37]
SPANS = [1, 5, 16, 17]
WIN = 512


@pytest.fixture(autouse=True)
def h2_arithmetic():
    prev = silero.encoder_mode("h2")
    yield
    silero.encoder_mode(prev)


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234))


@pytest.fixture(scope="module")
def clips():
    return weights.burst_clips(max(BATCHES), max(STEPS) * WIN, seed=47).astype(np.float32) * np.float32(0.000030517578)


@pytest.fixture(scope="module")
def reference(clips):
    """The oracle's scores of the longest clips, computed once: a window's score depends on nothing behind that window, so the first T
    columns of the first B rows are the scores of B clips cut to T whole windows."""
    w = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.silero_synthetic(1234).items()}
    return osil.OnnxWrapperOracle(w).audio_forward(torch.from_numpy(clips), 16000).numpy()


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("batch", BATCHES)
def test_block_flush_matches_oracle_and_spans(engine, clips, reference, batch, steps):
    assert engine.mode() == "h2"
    n = steps * WIN
    a = torch.from_numpy(np.ascontiguousarray(clips[:batch, :n])).cuda()
    probs, state = engine.clips(a, return_state=True)
    assert engine.range_fallbacks == 0
    assert tuple(probs.shape) == (batch, steps)
    np.testing.assert_allclose(probs.cpu().numpy(), reference[:batch, :steps], rtol=0, atol=ATOL)
    for span in SPANS:
        got = torch.full((batch, steps), -1.0, dtype=torch.float32, device="cuda")
        st = engine.clips_spanned(a, n, got, span=span)
        assert torch.equal(got, probs) and torch.equal(st, state), span


def _recur_h2(engine, batch, steps, state0):
    """the recurrent kernel alone over the engine's workspace, fp16 x 2, no range protocol around it"""
    probs = torch.full((batch, steps), -1.0, dtype=torch.float32, device="cuda")
    ws = engine._ws
    _lib.check(_lib.lib().vadx_silero_recur_span(engine.packed.data_ptr(), ws.data_ptr(), ws.numel(), batch, steps,
                                                 None if state0 is None else state0.data_ptr(), probs.data_ptr(), steps, None,
                                                 _lib.stream_ptr(), engine.cfg("h2")))
    torch.cuda.synchronize()
    return probs.cpu().numpy()


def test_group_outside_the_fp16_range_is_all_nan(engine, clips, reference):
    """T = 17 is one full block of scores and a remainder of one.  The second of three clip groups leaves the fp16 range, once through its audio
    (the encoder poisons its gx) and once through a caller-supplied state (the kernel overwrites the group's scores with NaN at its end, after
    both flushes have written numbers there): every score of that group is NaN, the other groups' are the oracle's, the flag is up."""
    batch, steps = 37, 17
    n = steps * WIN
    engine.range_flag()
    loud = clips[:batch, :n].copy()
    loud[16:32] = (np.random.default_rng(3).standard_normal((16, n)) * 3000).astype(np.float32)
    engine.encode(torch.from_numpy(loud).cuda(), mode="h2")
    got = _recur_h2(engine, batch, steps, None)
    flag, amax = engine.range_flag()
    assert flag == 1 and amax > 65504.0
    assert np.isnan(got[16:32]).all()
    np.testing.assert_allclose(got[:16], reference[:16, :steps], rtol=0, atol=ATOL)
    np.testing.assert_allclose(got[32:], reference[32:batch, :steps], rtol=0, atol=ATOL)

    engine.encode(torch.from_numpy(np.ascontiguousarray(clips[:batch, :n])).cuda(), mode="h2")
    assert engine.range_flag() == (0, 0.0)
    state0 = torch.zeros((2, batch, 128), dtype=torch.float32, device="cuda")
    state0[0, 16:32] = 1.0e5                     # h beyond the largest finite fp16
    got = _recur_h2(engine, batch, steps, state0)
    flag, amax = engine.range_flag()
    assert flag == 1 and amax > 65504.0
    assert np.isnan(got[16:32]).all()
    np.testing.assert_allclose(got[:16], reference[:16, :steps], rtol=0, atol=ATOL)
    np.testing.assert_allclose(got[32:], reference[32:batch, :steps], rtol=0, atol=ATOL)
