"""CPU: the bookkeeping every live-stream batch inherits from vadx.stream.StreamBatch -- which reset requests a tick applies and which
wait, the mask arguments, the ping-pong of the two records, save / restore -- on an engine stand-in that is torch on the CPU.  No library
call is involved: the base touches `engine.torch` and `engine.device` only."""
import types

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import dfsmn, firered, fsmn, marblenet, silero, stream

S, NB = 5, 64
ENGINE = types.SimpleNamespace(torch=torch, device="cpu")


class Probe(stream.StreamBatch):
    loaded = 0

    def _record_loaded(self):
        self.loaded += 1


def mask(*on):
    m = np.zeros(S, dtype=bool)
    m[list(on)] = True
    return m


def test_constructor():
    b = stream.StreamBatch(ENGINE, S, NB)
    assert b.streams == S and b._cur == 0 and not b._pending.any() and b._pending.shape == (S,)
    assert [(r.dtype, tuple(r.shape), int(r.sum())) for r in b._rec] == [(torch.uint8, (NB,), 0)] * 2
    assert b._rec[0].data_ptr() != b._rec[1].data_ptr() and b.record is b._rec[0]
    for bad in (0, -3):
        with pytest.raises(ValueError, match=f"streams={bad} must be positive"):
            stream.StreamBatch(ENGINE, bad, NB)


@pytest.mark.parametrize("arg, want", [
    (None, mask(0, 1, 2, 3, 4)),
    ([1, 3], mask(1, 3)),
    (torch.tensor([4, 0]), mask(0, 4)),
    (np.int32(2), mask(2)),
    (mask(0, 2), mask(0, 2)),
    (torch.from_numpy(mask(1, 4)), mask(1, 4)),
    ([False, False, False, True, False], mask(3)),
    (mask(2, 3).reshape(S, 1), mask(2, 3)),                  # any shape that flattens to [S]: every model, Silero included
    (torch.from_numpy(mask(0)).reshape(1, S), mask(0)),
])
def test_reset_states_names_exactly_these_streams(arg, want):
    b = stream.StreamBatch(ENGINE, S, NB)
    b.reset_states(arg)
    assert np.array_equal(b._pending, want)
    b.reset_states([1])                                      # requests add up
    assert np.array_equal(b._pending, want | mask(1))


def test_a_mask_of_the_wrong_length_is_refused_by_name():
    b = stream.StreamBatch(ENGINE, S, NB)
    with pytest.raises(ValueError, match=r"reset mask must have shape \(5,\), got \(4,\)"):
        b.reset_states(np.zeros(4, dtype=bool))
    with pytest.raises(ValueError, match=r"reset mask must have shape \(5,\), got \(10,\)"):
        b.reset_states(np.zeros((S, 2), dtype=bool))
    with pytest.raises(ValueError, match=r"active must have shape \(5,\), got \(6,\)"):
        b._begin(None, torch.zeros(6, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"reset must have shape \(5,\), got \(1,\)"):
        b._begin([True], None)
    assert not b._pending.any() and b._cur == 0


# (reset_states() argument before the tick or "-", the tick's reset, the tick's active)
SCRIPT = [
    ("-", None, None),                                        # a plain tick
    ([1, 3], None, mask(0, 1, 4)),                            # 1 is active: applied; 3 is not: waits
    ("-", mask(0), mask()),                                   # nobody is active: the explicit reset of 0 is dropped, 3 still waits
    ([2], None, [True, False, False, False, False]),          # 2 asked between two of its inactive ticks: waits; 0 is NOT reset (dropped above)
    ("-", torch.from_numpy(mask(4)), torch.from_numpy(mask(2, 3, 4))),      # 2 and 3 come back: applied, with 4's explicit one
    ("-", mask(0, 1, 2, 3, 4), None),                         # everybody is reset
    (None, None, mask(1)),                                    # reset_states(): only 1 is served now
    ("-", None, None),                                        # the other four, at their next active tick
    ("-", None, None),                                        # nothing left
]


def test_which_requests_a_tick_applies_and_which_wait():
    b = stream.StreamBatch(ENGINE, S, NB)
    waiting = [False] * S                                     # the rule, restated stream by stream
    seen_none = seen_all = 0
    for asked, reset, active in SCRIPT:
        if not isinstance(asked, str):
            b.reset_states(asked)
            for s in (range(S) if asked is None else asked):
                waiting[s] = True
        act_w = [True] * S if active is None else [bool(v) for v in active]
        explicit = [False] * S if reset is None else [bool(v) for v in reset]
        req_w = [False] * S
        for s in range(S):
            if act_w[s]:                                      # an active stream takes its waiting or explicit request now
                req_w[s], waiting[s] = waiting[s] or explicit[s], False
            # an inactive one: its waiting request goes on waiting, an explicit one is dropped and not remembered
        before = b._pending.copy()
        act, req, reset_d, act_d, src, dst = b._begin(reset, active)
        assert act.dtype == bool and act.tolist() == act_w and req.dtype == bool and req.tolist() == req_w
        assert np.array_equal(b._pending, before)             # the head of a tick changes nothing
        assert (reset_d is None) == (not any(req_w)) and (act_d is None) == (active is None)
        if reset_d is not None:
            assert reset_d.dtype == torch.uint8 and reset_d.tolist() == [int(v) for v in req_w]
        if act_d is not None:
            assert act_d.dtype == torch.uint8 and act_d.tolist() == [int(v) for v in act_w]
        assert b._begin(reset, active, upload_active=False)[3] is None
        assert src is b.record and dst is b._rec[1 - b._cur]
        b._end(act)
        assert b._pending.tolist() == waiting
        seen_none += not any(act_w)
        seen_all += all(req_w)
    assert seen_none and seen_all and not any(waiting)


def test_the_records_alternate_and_the_one_read_is_left_alone():
    b = stream.StreamBatch(ENGINE, S, NB)
    ptrs = [r.data_ptr() for r in b._rec]
    for tick in range(1, 5):
        act, _, _, _, src, dst = b._begin()
        assert src.data_ptr() == ptrs[(tick - 1) % 2] and dst.data_ptr() == ptrs[tick % 2]
        kept = src.clone()
        dst.fill_(tick)                                       # what a kernel would do
        b._end(act)
        assert b.record is dst and int(b.record[0]) == tick and b.record.data_ptr() == ptrs[tick % 2]
        assert torch.equal(src, kept) and int(src[0]) == tick - 1


@pytest.mark.parametrize("as_numpy", [False, True])
def test_load_record(as_numpy):
    b = Probe(ENGINE, S, NB)
    b._end(np.ones(S, dtype=bool))                            # mid-stream: the second tensor is current
    b.reset_states([0, 2])
    saved = torch.arange(NB, dtype=torch.uint8)
    other = b._rec[1 - b._cur].clone()
    b.load_record(saved.numpy() if as_numpy else saved.view(4, 16))      # any shape of the right size
    assert torch.equal(b.record, saved) and b.record is b._rec[1] and torch.equal(b._rec[0], other)
    assert not b._pending.any() and b.loaded == 1
    for bad, what in ((saved[:-1], r"torch.uint8 \[63\]"), (torch.zeros(NB + 16, dtype=torch.uint8), r"torch.uint8 \[80\]"),
                      (saved.to(torch.int8), r"torch.int8 \[64\]"), (np.zeros(NB // 4, dtype=np.float32), r"torch.float32 \[16\]")):
        b.reset_states([3])
        with pytest.raises(ValueError, match=r"record must be uint8 \[64\], got " + what):
            b.load_record(bad)
        assert torch.equal(b.record, saved) and b._pending.tolist() == mask(3).tolist() and b.loaded == 1      # a refusal changes nothing


def test_samples_are_taken_where_they_are_and_refused_by_name():
    b = stream.StreamBatch(ENGINE, S, NB)
    x = np.zeros((S, 7), dtype=np.int16)
    assert b._samples(x).dtype == torch.int16 and tuple(b._samples(x[:, ::2]).shape) == (S, 4)
    xt = torch.from_numpy(x)
    assert b._samples(xt) is xt
    with pytest.raises(ValueError, match="samples must be int16, got torch.float32"):
        b._samples(x.astype(np.float32))
    with pytest.raises(ValueError, match=r"samples must be \[5, n\], got \(4, 7\)"):
        b._samples(x[:4])
    with pytest.raises(ValueError, match=r"samples must be \[5, n\], got \(35,\)"):
        b._samples(x.reshape(-1))
    with pytest.raises(ValueError, match=r"samples must be \[5, k\*2\], got \(5, 7\) here"):
        b._samples(x, "[5, k*2]", lambda v: v.shape[1] % 2, where=" here")
    assert b._samples(x.astype(np.float64), floats=True).dtype == torch.float32
    with pytest.raises(ValueError, match="samples must be float32 or int16, got torch.int32"):
        b._samples(x.astype(np.int32), floats=True)


class Windows(stream.WindowStreamBatch):
    """L = 100 samples per window, 30 apart; the record's first S int32 words are the streams' "has a carry" words."""
    stride, frame_s = 30, 0.01

    def _primed_words(self):
        return self.record[:4 * S].view(torch.int32)


def test_window_streams_mirror_who_has_a_carry():
    b = Windows(types.SimpleNamespace(torch=torch, device="cpu", L=100), S, NB)
    assert b.samples_needed(2).tolist() == [130] * S
    b._end(b._begin(None, mask(0, 1, 2))[0])                  # only the active streams get a carry
    assert b.samples_needed(2).tolist() == [60, 60, 60, 130, 130]
    assert b.samples_needed(1, reset=mask(0)).tolist() == [100, 30, 30, 100, 100]
    b.reset_states([1])
    assert b.samples_needed(1).tolist() == [30, 100, 30, 100, 100]
    with pytest.raises(ValueError, match="windows=0 must be at least 1"):
        b.samples_needed(0)
    saved = torch.zeros(NB, dtype=torch.uint8)
    saved[:4 * S].view(torch.int32)[3] = 1                    # a record in which stream 3 alone has a carry
    b.load_record(saved)
    assert b._primed.tolist() == mask(3).tolist() and b.samples_needed(1).tolist() == [100, 100, 100, 30, 100]
    assert b.timestamps(np.array([1, 1, 0, 0, 0, 0], np.uint8), torch.tensor([1, 1], dtype=torch.uint8), 0.0, 0.0) == \
        fsmn.flag_timestamps(np.array([1, 1, 0, 0, 0, 0, 1, 1], np.uint8), 0.01, 0.0, 0.0)


CLASSES = [silero.VADIteratorBatch, fsmn.FsmnStreamBatch, firered.FireRedStreamBatch, dfsmn.DfsmnStreamBatch, marblenet.MarbleNetStreamBatch]


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_the_five_classes_inherit_the_bookkeeping(cls):
    assert issubclass(cls, stream.StreamBatch)
    for name in ("_mask", "reset_states", "record", "load_record", "_begin", "_end", "_samples"):
        assert name not in cls.__dict__, name
    assert cls.record is stream.StreamBatch.record and cls.load_record is stream.StreamBatch.load_record
    if cls in (fsmn.FsmnStreamBatch, dfsmn.DfsmnStreamBatch):
        assert issubclass(cls, stream.WindowStreamBatch) and "_primed_words" in cls.__dict__
        for name in ("samples_needed", "timestamps", "_record_loaded"):
            assert name not in cls.__dict__, name
