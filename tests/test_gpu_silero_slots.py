"""The fp16 x 2 encoder's workgroup slots (csrc/silero_h2.hip): a workgroup encodes up to four consecutive windows of one clip group,
and the slots past a clip's last window are skipped.  Every count of valid slots (T = 1 .. 9, spans of 1, 2, 3 and 5 windows) must give
the one-launch result bit for bit, and a workgroup with skipped slots must still raise the range flag and poison its gx."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, silero, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    return silero.SileroEngine(weights.silero_synthetic(1234))


@pytest.fixture(autouse=True)
def h2_mode():
    prev = silero.encoder_mode("h2")
    yield
    silero.encoder_mode(prev)


def _clips(batch, n, seed):
    return torch.from_numpy(weights.burst_clips(batch, n, seed=seed).astype(np.float32) * np.float32(0.000030517578)).cuda()


def _one_launch(engine, a, n):
    batch = int(a.shape[0])
    steps = (n + 511) // 512
    ws = engine._workspace(batch, steps)
    probs = torch.empty((batch, steps), dtype=torch.float32, device="cuda")
    state = torch.empty((2, batch, 128), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().vadx_silero_clips(engine.packed.data_ptr(), a.data_ptr(), batch, n, _lib.row_stride(a), probs.data_ptr(),
                                            state.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(), engine.cfg()))
    torch.cuda.synchronize()
    return probs, state


def _spanned(engine, a, n, span):
    steps = (n + 511) // 512
    probs = torch.full((int(a.shape[0]), steps), -1.0, dtype=torch.float32, device="cuda")
    state = engine.clips_spanned(a, n, probs, span=span)
    torch.cuda.synchronize()
    return probs, state


@pytest.mark.parametrize("steps", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_every_valid_slot_count_matches_single_window_launches(engine, steps):
    """T = 1 .. 9 covers T = 1, 2, 3, 0 (mod 4) with and without full workgroups in front; against span = 1, where every workgroup
    holds one valid slot.  37 clips: the last clip group is partial too."""
    n = 512 * steps - 100
    a = _clips(37, n, seed=100 + steps)
    want, st_want = _one_launch(engine, a, n)
    got, st = _spanned(engine, a, n, 1)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want) and torch.equal(st, st_want)


@pytest.mark.parametrize("span", [1, 2, 3, 5])
def test_spans_of_one_to_five_windows(engine, span):
    """Spans whose window count leaves 1, 2, 3 or 0 slots of the last workgroup row valid, over an 11-window clip."""
    n = 512 * 11 - 7
    a = _clips(21, n, seed=7 + span)
    want, st_want = _one_launch(engine, a, n)
    got, st = _spanned(engine, a, n, span)
    assert torch.equal(got, want) and torch.equal(st, st_want)


def test_range_flag_and_poison_in_a_workgroup_with_skipped_slots(engine):
    """T = 5: window 4 sits alone in its workgroup (three slots skipped).  Audio far outside +-1 in that window only (from its sample
    128 on, which no earlier window reaches): the flag is raised, that window's gx is NaN (its scores are NaN without the range
    protocol), the windows in front are untouched, and the protocol recomputes the batch on bf16 x 3."""
    n = 5 * 512
    x = _clips(16, n, seed=3)
    x[:, 4 * 512 + 128:] = torch.from_numpy((np.random.default_rng(9).standard_normal((16, 384)) * 3000).astype(np.float32)).cuda()
    engine.range_flag()                                                           # clear
    B, steps = engine.encode(x)
    probs = engine.recur(B, steps, torch.empty((B, steps), dtype=torch.float32, device="cuda"))
    flag, amax = engine.range_flag()
    assert flag == 1 and amax > 65504.0
    p = probs.cpu()
    assert torch.isfinite(p[:, :4]).all() and torch.isnan(p[:, 4]).all()
    prev = silero.encoder_mode("split")
    want = engine.clips(x)
    silero.encoder_mode("h2")
    n0 = engine.range_fallbacks
    got = engine.clips(x)
    assert engine.range_fallbacks == n0 + 1 and torch.equal(got, want)
    silero.encoder_mode(prev)
