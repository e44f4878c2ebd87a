"""GPU, kernels alone on plain tensors (no network): vadx_dfsmn_stream_windows + vadx_dfsmn_stream_vote advance S = 3 live streams so that,
whatever the tick schedule, the assembled windows are the slices of the concatenated audio and the flags of the ticks followed by the last
tail are vadx_dfsmn_vote over the whole score tensor; a reset restarts one stream only, an inactive stream passes through bit for bit and
owns no window row, and state_in is never written."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib
from vadx.dfsmn import SH_DONE, SH_PRIMED, SHDR_WORDS

pytestmark = pytest.mark.gpu

L, T, LB, S, W = 16001, 51, 15, 3, 4
CARRY = (LB + 1) * 320
STRIDE = L - CARRY
SLIDE = T - LB
SPK, SIL = 0.7, 0.3
GUARD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


class Streams:
    """The two entry points around plain tensors: two ping-ponged records, one tick = windows call + vote call on given scores."""

    def __init__(self, channels):
        self.ch = channels
        nb = _lib.lib().vadx_dfsmn_stream_state_bytes(S, L, LB, channels)
        assert nb and nb % 16 == 0
        self.rec = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.cur = 0

    def header(self, rec):
        return rec[:S * SHDR_WORDS * 4].view(torch.int32).view(S, SHDR_WORDS).cpu().numpy()

    def carries(self, rec):
        return rec[S * SHDR_WORDS * 4:].view(torch.int16).view(self.ch, S, CARRY).cpu().numpy()

    def done(self, rec):
        return rec[:S * SHDR_WORDS * 4].view(torch.int64).view(S, SHDR_WORDS // 2)[:, SH_DONE // 2].cpu().numpy()

    def stream_bytes(self, rec, s):
        return np.concatenate([self.header(rec)[s].view(np.uint8)] + [self.carries(rec)[c, s].view(np.uint8) for c in range(self.ch)])

    def tick(self, samples, scores, k, slot=None, reset=None, n_slots=S, swap=True):
        """samples: per channel int16 [S, n]; scores f32 [n_slots * k, T] -> (window rows per channel [n_slots * k, L], flags, tail)"""
        src, dst = self.rec[self.cur], self.rec[1 - self.cur]
        xs = [dev(x) for x in samples]
        bufs = [torch.full((n_slots * k * L + GUARD,), 0x5A5A, dtype=torch.int16, device="cuda") for _ in xs]
        slot_d = None if slot is None else dev(np.asarray(slot, dtype=np.int32))
        reset_d = None if reset is None else dev(np.asarray(reset, dtype=np.uint8))
        flags = torch.zeros((S, k * SLIDE), dtype=torch.uint8, device="cuda")
        tail = torch.zeros((S, LB), dtype=torch.uint8, device="cuda")
        two = self.ch == 2
        lib = _lib.lib()
        _lib.check(lib.vadx_dfsmn_stream_windows(ptr(xs[0]), ptr(xs[1]) if two else None, xs[0].shape[1], S, n_slots, k, L, LB, ptr(slot_d),
                                                 ptr(reset_d), src.data_ptr(), dst.data_ptr(), ptr(bufs[0]), ptr(bufs[1]) if two else None,
                                                 _lib.stream_ptr()))
        _lib.check(lib.vadx_dfsmn_stream_vote(dev(scores).data_ptr(), S, n_slots, k, T, LB, self.ch, SPK, SIL, ptr(slot_d), ptr(reset_d),
                                              src.data_ptr(), dst.data_ptr(), flags.data_ptr(), tail.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        if swap:
            self.cur = 1 - self.cur
        for b in bufs:
            assert (b[n_slots * k * L:] == 0x5A5A).all()                 # nothing written behind the window rows
        return [b[:n_slots * k * L].view(n_slots * k, L).cpu().numpy() for b in bufs], flags.cpu().numpy(), tail.cpu().numpy()


def make(seed, channels, windows=W):
    """-> (audio int16 [channels, S, (windows-1)*stride + L], scores f32 [S, windows, T] with a tenth exactly on the thresholds)"""
    rng = np.random.default_rng(seed)
    audio = rng.integers(-32768, 32768, (channels, S, (windows - 1) * STRIDE + L)).astype(np.int16)
    scores = rng.random((S, windows, T), dtype=np.float32)
    pick = rng.random(scores.shape)
    scores[pick < 0.05], scores[pick > 0.95] = np.float32(SPK), np.float32(SIL)
    return audio, scores


def whole_vote(scores):
    """vadx_dfsmn_vote over [B, W', T] scores -> flags u8 [B, W' * SLIDE + LB]"""
    B, w = scores.shape[0], scores.shape[1]
    flags = torch.empty((B, w * SLIDE + LB), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vadx_dfsmn_vote(dev(scores).data_ptr(), B, w, T, LB, SPK, SIL, flags.data_ptr(), _lib.stream_ptr()))
    return flags.cpu().numpy()


def need(k, fresh):
    return L + (k - 1) * STRIDE if fresh else k * STRIDE


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("sched", [(1, 1, 1, 1), (2, 1, 1), (4,)])
def test_any_schedule_gives_the_whole_clip_windows_and_flags(channels, sched):
    audio, scores = make(sum(sched) * 10 + channels, channels)
    st = Streams(channels)
    pos, j0, got = 0, 0, []
    for k in sched:
        n = need(k, pos == 0)
        rows, flags, tail = st.tick([audio[c, :, pos:pos + n] for c in range(channels)], scores[:, j0:j0 + k].reshape(S * k, T), k)
        pos += n
        for c in range(channels):
            for s in range(S):
                for j in range(k):
                    at = (j0 + j) * STRIDE
                    assert np.array_equal(rows[c][s * k + j], audio[c, s, at:at + L]), (c, s, j0 + j)
            assert np.array_equal(st.carries(st.rec[st.cur])[c], audio[c, :, pos - CARRY:pos])
        j0 += k
        got.append(flags)
        assert (st.done(st.rec[st.cur]) == j0).all() and (st.header(st.rec[st.cur])[:, SH_PRIMED] == 1).all()
        # the tail after j0 windows is the tail of the clip that ends there
        assert np.array_equal(tail, whole_vote(scores[:, :j0])[:, j0 * SLIDE:])
    assert pos == audio.shape[2] and j0 == W
    assert np.array_equal(np.concatenate(got + [tail], axis=1), whole_vote(scores))


@pytest.mark.parametrize("channels", [1, 2])
def test_state_in_is_never_written_and_a_repeated_tick_writes_the_same_bytes(channels):
    audio, scores = make(7 + channels, channels)
    st = Streams(channels)
    st.tick([audio[c, :, :L] for c in range(channels)], scores[:, 0], 1)
    before = st.rec[st.cur].clone()
    args = ([audio[c, :, L:L + 2 * STRIDE] for c in range(channels)], scores[:, 1:3].reshape(S * 2, T), 2)
    first = st.tick(*args, swap=False)
    out = st.rec[1 - st.cur].clone()
    assert torch.equal(st.rec[st.cur], before)
    st.rec[1 - st.cur].fill_(0xEE)
    again = st.tick(*args, swap=False)
    assert torch.equal(st.rec[st.cur], before) and torch.equal(st.rec[1 - st.cur], out)      # every byte of state_out is written again
    for a, b in zip(first[0] + list(first[1:]), again[0] + list(again[1:])):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("channels", [1, 2])
def test_a_reset_mid_stream_restarts_that_stream_only(channels):
    audio, scores = make(20 + channels, channels)
    other, other_scores = make(30 + channels, channels, windows=2)
    st = Streams(channels)
    _, f0, _ = st.tick([audio[c, :, :L] for c in range(channels)], scores[:, 0], 1)
    # tick 2: stream 1 starts over on `other` (a whole first window), streams 0 and 2 go on
    smp = [audio[c, :, L:2 * L].copy() for c in range(channels)]
    sc = scores[:, 1].copy()
    for c in range(channels):
        smp[c][1] = other[c, 1, :L]
    sc[1] = other_scores[1, 0]
    rows, f1, _ = st.tick(smp, sc, 1, reset=[0, 1, 0])
    assert st.done(st.rec[st.cur]).tolist() == [2, 1, 2]
    for c in range(channels):
        assert np.array_equal(rows[c][1], other[c, 1, :L]) and np.array_equal(rows[c][0], audio[c, 0, STRIDE:STRIDE + L])
        assert np.array_equal(st.carries(st.rec[st.cur])[c, 1], other[c, 1, L - CARRY:L])
    # tick 3: everybody goes on
    smp = [audio[c, :, L + STRIDE:L + 2 * STRIDE].copy() for c in range(channels)]
    sc = scores[:, 2].copy()
    for c in range(channels):
        smp[c][1] = other[c, 1, L:L + STRIDE]
    sc[1] = other_scores[1, 1]
    rows, f2, tail = st.tick(smp, sc, 1)
    assert st.done(st.rec[st.cur]).tolist() == [3, 2, 3]
    for c in range(channels):
        assert np.array_equal(rows[c][1], other[c, 1, STRIDE:STRIDE + L]) and np.array_equal(rows[c][2], audio[c, 2, 2 * STRIDE:2 * STRIDE + L])
    want = whole_vote(scores[:, :3])
    got = np.concatenate([f0, f1, f2, tail], axis=1)
    assert np.array_equal(got[[0, 2]], want[[0, 2]])
    assert np.array_equal(np.concatenate([f1[1], f2[1], tail[1]]), whole_vote(other_scores[1:2])[0])


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("slot", [[0, -1, 1], [1, 7, 0], [0, -5, 1]])      # a slot outside [-1, n_slots) is inactive too
def test_an_inactive_stream_passes_through_and_owns_no_row(channels, slot):
    audio, scores = make(40 + channels, channels)
    st = Streams(channels)
    _, f0, _ = st.tick([audio[c, :, :L] for c in range(channels)], scores[:, 0], 1)
    before = st.rec[st.cur].clone()
    k, live = 2, [s for s in range(S) if 0 <= slot[s] < 2]
    sc = np.zeros((2 * k, T), dtype=np.float32)
    for s in live:
        sc[slot[s] * k:slot[s] * k + k] = scores[s, 1:3]
    # two slots for three streams; the inactive stream asks for a reset, which is ignored
    rows, f1, tail = st.tick([audio[c, :, L:L + k * STRIDE] for c in range(channels)], sc, k, slot=slot, reset=[0, 1, 0], n_slots=2)
    after = st.rec[st.cur]
    assert np.array_equal(st.stream_bytes(after, 1), st.stream_bytes(before, 1))
    assert (f1[1] == 255).all() and (tail[1] == 255).all()
    assert st.done(after).tolist() == [3, 1, 3]
    for c in range(channels):
        assert rows[c].shape == (2 * k, L)
        for s in live:
            for j in range(k):
                assert np.array_equal(rows[c][slot[s] * k + j], audio[c, s, (1 + j) * STRIDE:(1 + j) * STRIDE + L]), (c, s, j)
    want = whole_vote(scores[:, :3])
    assert np.array_equal(np.concatenate([f0, f1, tail], axis=1)[live], want[live])
    # the stream that sat out goes on from where it was
    smp = [audio[c, :, L:L + STRIDE] for c in range(channels)]
    _, f2, tail = st.tick(smp, np.stack([scores[1, 1]]), 1, slot=[-1, 0, -1], n_slots=1)
    assert np.array_equal(np.concatenate([f0[1], f2[1], tail[1]]), whole_vote(scores[1:2, :2])[0])
    assert st.done(st.rec[st.cur]).tolist() == [3, 2, 3]
