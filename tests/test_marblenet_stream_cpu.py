"""CPU: the MarbleNet streaming definition, its counts and its refusals -- no GPU.

1. tests/_marblenet_stream_ref.py (the torch restatement of the streaming definition: per-stage histories, global-index masking, the
   `final` cascade) is pinned to the oracle on whole clips.  WHICH bound: torch's conv1d / matmul on this CPU are NOT order-stable (a
   frame's float32 bits change with the length of the tensor it is computed in -- in the front-end's DFT and in the encoder's convs
   alike; at k = 33 the float32 streamed logits of the clips below equal the oracle's bit for bit, at k = 1 they differ by 7e-6 sd(z)),
   so the pin is not bitwise.  It is split where the rounding enters:
     - the encoder + decoder in float64 on the ORACLE'S OWN log-mel (oracle.marblenet.log_mel -> encoder -> Linear, the pieces of
       `forward`), streamed against whole: 1e-6 in logit space, max |z - z_ref| / sd(z_ref), z = z1 - z0 (measured: 1e-14);
     - the streamed front-end's frames against the oracle's log-mel of the whole clip: 1e-3 in the log domain.  A 512-tap float32 dot
       product of white noise carries a relative rounding error of at most 512 * 2^-24 * sum|x w| / |sum x w| ~ 3e-5 * sqrt(512) =
       7e-4 whatever the order of its terms (measured: 2e-5); silence is exact (log 1e-7 in every band);
     - end to end in float32, the probabilities: 1e-4, the suite's tolerance on MarbleNet scores (tests/test_gpu_marblenet.py).
2. vadx.marblenet.stream_counts against the closed forms and against brute force: which frames of a prefix's oracle output no later
   audio can change.
3. Refusals, by name, of everything reachable without a device."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vadx  # noqa: F401
from vadx import _lib, marblenet, weights
from oracle import marblenet as omb

import _marblenet_stream_ref as sref

HOP = 320
TOTALS = (0, 1, 319, 320, 321, 320 * 73, 320 * 73 + 319, 320 * 74, 320 * 74 + 1, 320 * 75 + 161, 320 * 140 + 7)
TICKS = (1, 2, 3, 31, 32, 33, 64)
_W = {}


def w():
    if not _W:
        _W.update(weights.marblenet_synthetic(1234))
    return _W


def clip_of(n, seed=5):
    rng = np.random.default_rng(seed + n)
    c = np.clip(np.rint(rng.standard_normal(n) * 8000), -32768, 32767).astype(np.int16)
    if n == 320 * 74:
        c[:n // 2] = 0                          # silence then noise
    return c


def oracle_logits(clip, dtype):
    """oracle.marblenet.forward's pieces on the whole clip: (log-mel [80, F] float32, logits [n // 320, 2] in `dtype`)"""
    wt = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w().items()}
    with torch.no_grad():
        lm = omb.log_mel(omb.Frontend(), torch.from_numpy(clip).reshape(1, 1, -1))
        enc, length = omb.encoder(wt, lm.to(dtype))
        logits = F.linear(enc.transpose(1, 2), wt["dec_w"], wt["dec_b"])[0]
    assert length - 1 == clip.size // HOP                                  # the session's signal_len - 1
    return lm[0], logits[:clip.size // HOP]


# ---- 1. the reference
@pytest.mark.parametrize("n", [n for n in TOTALS if n >= 320])
def test_reference_encoder_is_the_oracle_on_whole_clips(n):
    clip = clip_of(n)
    lm, want = oracle_logits(clip, torch.float64)
    z = (want[:, 1] - want[:, 0]).numpy()
    sd = float(z.std()) if n // HOP > 1 else 1.0
    for k in (1, 3, 33):
        got, per_tick = sref.stream_clip(w(), clip, k, torch.float64, mel=lm)
        assert got.shape == want.shape and sum(per_tick) == n // HOP
        e = float(np.abs((got[:, 1] - got[:, 0]).numpy() - z).max() / sd)
        assert e <= 1e-6, (n, k, e)


@pytest.mark.parametrize("n", [1, 319, 320 * 74, 320 * 75 + 161])
def test_reference_front_end_frames_are_the_oracles(n):
    clip = clip_of(n)
    lm, _ = oracle_logits(clip, torch.float32)
    for k in (1, 5, 64):
        ref = sref.StreamRef(w())
        at, row, seen = 0, k * HOP, 0
        with torch.no_grad():
            while True:
                final = n - at < row
                ref.feed(clip[at:at + row] if not final else clip[at:], final=final)
                a, b = ref.last_mel_range
                assert a == max(2 * (at // HOP) - 1, -1) and ref.last_mel.shape[1] == b - a
                got = ref.last_mel[:, max(0, -a):]
                assert float((got - lm[:, max(a, 0):b]).abs().max()) <= 1e-3, (n, k, at)
                seen = b
                at += row
                if final:
                    break
        assert seen == lm.shape[1] == n // 160 + 1


@pytest.mark.parametrize("n", [320, 320 * 74 + 1, 320 * 140 + 7])
def test_reference_end_to_end_float32(n):
    clip = clip_of(n)
    _, want = oracle_logits(clip, torch.float32)
    fwd = omb.forward(omb.Frontend(), {k: torch.as_tensor(np.asarray(v)) for k, v in w().items()}, torch.from_numpy(clip).reshape(1, 1, -1))
    assert int(fwd[2]) == n // HOP
    for k in (1, 32):
        got, _ = sref.stream_clip(w(), clip, k)
        p = torch.softmax(got, dim=-1)
        assert float((p[:, 1] - fwd[1][0, :n // HOP, 0]).abs().max()) <= 1e-4
        assert float((p[:, 0] - fwd[0][0, :n // HOP, 0]).abs().max()) <= 1e-4
        assert float((got - want).abs().max()) <= 1e-3


def test_final_is_not_feeding_silence():
    """The right edge: every layer pads ITS OWN input with zeros.  Feeding 1.5 s of digital silence instead of `final` gives other
    numbers for the last frames (log-mel of silence is log 1e-7, not 0) -- the reference must tell the two apart."""
    n = 320 * 90
    clip = clip_of(n)
    _, want = oracle_logits(clip, torch.float64)
    ref = sref.StreamRef(w(), torch.float64)
    with torch.no_grad():
        a = ref.feed(clip)
        b = ref.feed(np.zeros(74 * HOP, np.int16))
    fed_silence = torch.cat([a, b])[:n // HOP]
    assert fed_silence.shape == want.shape
    assert float((fed_silence[:n // HOP - 73] - want[:n // HOP - 73]).abs().max()) <= 1e-4       # far from the edge: the same (float32 log-mel)
    assert float((fed_silence[-20:] - want[-20:]).abs().max()) > 1e-2                          # at the edge: another function


# ---- 2. counts
def closed_form(n_total_before, n_after, final):
    J0, J1 = n_total_before // HOP, n_after // HOP
    before = (max(2 * J0 - 1, 0), max(J0 - 3, 0), max(J0 - 73, 0))
    after = (n_after // 160 + 1, n_after // HOP + 1, n_after // HOP) if final else (max(2 * J1 - 1, 0), max(J1 - 3, 0), max(J1 - 73, 0))
    return tuple(a - b for a, b in zip(after, before))


@pytest.mark.parametrize("k", TICKS)
def test_stream_counts_closed_forms(k):
    for n in TOTALS:
        fed, sums = 0, np.zeros(3, np.int64)
        row = k * HOP
        while n - fed >= row:
            got = marblenet.stream_counts(fed, row, False)
            assert tuple(int(v) for v in got) == closed_form(fed, fed + row, False), (n, k, fed)
            sums += np.array([int(v) for v in got])
            fed += row
        assert sums[2] == max(0, fed // HOP - 73) and sums[0] == max(0, 2 * (fed // HOP) - 1)       # after N = 320 J samples, no final
        got = marblenet.stream_counts(fed, n - fed, True)
        assert tuple(int(v) for v in got) == closed_form(fed, n, True), (n, k, fed)
        sums += np.array([int(v) for v in got])
        assert sums.tolist() == [n // 160 + 1, n // HOP + 1, n // HOP], (n, k)
    m, e, s = marblenet.stream_counts([0, 320 * 80, 320 * 80], [k * HOP, 0, 7], [False, False, True])
    assert m.shape == (3,) and e[1] == 0 and s[1] == 0 and s[2] == 73


def test_stream_counts_against_brute_force():
    """Which leading frames are final once N = 320 J samples are in: the oracle on the whole clip against the oracle on the same clip with
    EVERYTHING FROM SAMPLE N ON replaced by other noise -- the leading log-mel / encoder-output / score frames that stay bit-identical
    are exactly the counts, the next one differs.  (Same length on both sides on purpose: against a bare prefix torch's float32 DFT
    rounds every frame differently, see the module docstring, and the influence of the last samples under the window's tail is too
    small for any tolerance that forgives that.)  Float64 net on the float32 log-mel.
    Which N: a non-final count depends on the samples fed alone, and the boundaries the issue's totals visit at its tick sizes are the
    multiples of 320 k up to each total -- with k = 1 among the tick sizes, every J = 1 .. 140.  All of them are checked, on the longest
    total's clip.  `final` counts are the oracle's own frame counts on the prefix, at every total of the issue's list."""
    n = 320 * 140 + 7
    clip = clip_of(n, seed=11)
    other = clip_of(n, seed=12)
    wt = {k: torch.as_tensor(np.asarray(v)).double() for k, v in w().items()}
    fe = omb.Frontend()

    def stages(a):
        with torch.no_grad():
            lm = omb.log_mel(fe, torch.from_numpy(a.copy()).reshape(1, 1, -1))
            x = lm.double()
            pro = F.relu(omb._bn(F.conv1d(F.conv1d(x, wt["b0r0_dw"].unsqueeze(1), stride=2, padding=5, groups=80), wt["b0r0_pw"].unsqueeze(-1)), wt, "b0r0"))
            enc, _ = omb.encoder(wt, x)
            z = F.linear(enc.transpose(1, 2), wt["dec_w"], wt["dec_b"])
        return lm[0].t().numpy(), pro[0].t().numpy(), z[0].numpy()

    whole = stages(clip)

    def stable(a, b):
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        return int(bad[0]) if len(bad) else len(a)

    visited = sorted({fed // HOP for total in TOTALS for k in TICKS for fed in range(k * HOP, total + 1, k * HOP)})
    assert visited == list(range(1, 141)) and n == max(TOTALS)
    for J in visited:
        changed = clip.copy()
        changed[J * HOP:] = other[J * HOP:]
        part = stages(changed)
        counts = [int(v) for v in marblenet.stream_counts(0, J * HOP, False)]
        got = [stable(p, q) for p, q in zip(part, whole)]
        assert got == counts == [max(2 * J - 1, 0), max(J - 3, 0), max(J - 73, 0)], (J, got, counts)
    for total in TOTALS:                                         # final: the counts are the whole-clip call's own frame counts
        if total == 0:                                           # (the oracle takes no empty clip: one log-mel frame of padding, no score)
            assert [int(v) for v in marblenet.stream_counts(0, 0, True)] == [1, 1, 0]
            continue
        part = stages(clip[:total])
        fin = [int(v) for v in marblenet.stream_counts(0, total, True)]
        assert fin == [part[0].shape[0], part[1].shape[0], part[2].shape[0] - 1] == [total // 160 + 1, total // HOP + 1, total // HOP]


# ---- 3. refusals
def test_step_arguments_are_refused_by_name():
    ok = marblenet.check_stream_step
    ok(1, [320, 0], [False, False]); ok(64, [64 * 320, 161], [False, True]); ok(256, [0], [True])
    with pytest.raises(ValueError, match=r"k=0 frames per tick is outside \[1, 256\]"):
        ok(0, [0], [False])
    with pytest.raises(ValueError, match=r"k=257 frames per tick is outside \[1, 256\]"):
        ok(257, [320], [False])
    with pytest.raises(ValueError, match="n_samples=161 is not a multiple of 320 on a stream that is not final"):
        ok(4, [320, 161], [False, False])
    with pytest.raises(ValueError, match=r"n_samples=1600 is outside \[0, k \* 320 = 1280\]"):
        ok(4, [1600, 320], [False, True])
    with pytest.raises(ValueError, match=r"n_samples=-320 is outside"):
        ok(4, [-320], [False])
    with pytest.raises(ValueError, match="multiple of 320"):
        marblenet.stream_counts(100, 320, False)
    with pytest.raises(ValueError, match="multiple of 320"):
        marblenet.stream_counts(0, 100, False)


def test_engines_the_stream_path_is_not_built_for_are_refused_by_name():
    with pytest.raises(ValueError, match="in_sample_rate is 8000, not 16000"):
        marblenet.MarbleNetStreamBatch(types.SimpleNamespace(in_sample_rate=8000, fused=True), 4)
    with pytest.raises(ValueError, match="another `blocks` layout"):
        marblenet.MarbleNetStreamBatch(types.SimpleNamespace(in_sample_rate=16000, fused=False), 4)
    with pytest.raises(ValueError, match="streams=0 must be at least 1"):
        marblenet.MarbleNetStreamBatch(types.SimpleNamespace(in_sample_rate=16000, fused=True), 0)


def test_c_entry_refuses_before_any_hip_call():
    """vadx_marblenet_stream_tick and vadx_frontend_logmel_stream check their arguments before the first HIP call, so the refusals run
    on a machine without a GPU: every pointer below is a host buffer no kernel ever sees."""
    lib = _lib.lib()
    assert lib.vadx_abi_version() == 10
    assert lib.vadx_marblenet_stream_max_frames() == marblenet.STREAM_MAX_FRAMES == 256 >= 64
    assert lib.vadx_marblenet_stream_cap(1) == 74 and lib.vadx_marblenet_stream_cap(0) == 0 and lib.vadx_marblenet_stream_cap(257) == 0
    assert lib.vadx_marblenet_stream_state_bytes(2) == 2 * 46048 and lib.vadx_marblenet_stream_state_bytes(0) == 0
    assert lib.vadx_marblenet_stream_workspace_bytes(4, 0) == 0 and lib.vadx_marblenet_stream_workspace_bytes(0, 4) == 0
    need = lib.vadx_marblenet_stream_workspace_bytes(2, 4)
    assert need > 0 and need % 256 == 0
    from vadx import frontend
    _, cfg, _, _, _ = frontend.host_tables("marblenet", 16000)
    cfg.fold = frontend.KIND_SPLIT_H2
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    p = (base + 255) & ~255                     # an aligned, non-NULL stand-in for every pointer
    wts = _lib.MarbleNetStreamWeights()
    for name, typ in wts._fields_:
        setattr(wts, name, p if typ is C.c_void_p else (C.c_void_p * 3)(p, p, p))
    flag = _lib.MarbleNetCfg(_lib.ARITH["h2"], 0, p)

    def tick(cfg=cfg, w=wts, samples=p, stride=4 * 320, n=p, streams=2, k=4, sin=p, sout=p + 512, ws=p, ws_bytes=need, mc=flag):
        rc = lib.vadx_marblenet_stream_tick(C.byref(cfg), p, p, C.byref(w), samples, stride, n, None, None, streams, k, sin, sout, p, p, p, ws,
                                            ws_bytes, None, C.byref(mc) if mc is not None else None)
        return rc, lib.vadx_last_error().decode()

    for kw, match in ((dict(k=0), "k=0 frames per tick is outside [1, 256]"), (dict(k=257), "k=257 frames per tick is outside [1, 256]"),
                      (dict(streams=0), "streams=0 must be at least 1"), (dict(samples=None), "NULL argument"), (dict(n=None), "NULL argument"),
                      (dict(stride=100), "sample_stride=100 is shorter"), (dict(sout=p), "second record"),
                      (dict(ws_bytes=need - 1), "workspace of"), (dict(ws=p + 4), "16-byte aligned"),
                      (dict(mc=_lib.MarbleNetCfg(_lib.ARITH["split"], 0, p)), "arithmetic 2 is not built"),
                      (dict(mc=_lib.MarbleNetCfg(_lib.ARITH["h2"], 0, None)), "F16X2 needs cfg->range_flag")):
        rc, msg = tick(**kw)
        assert rc == -1 and match in msg, (kw, rc, msg)
    bad_w = _lib.MarbleNetStreamWeights.from_buffer_copy(wts)
    bad_w.b_rw[1] = None
    rc, msg = tick(w=bad_w)
    assert rc == -1 and "NULL weight of block 3" in msg
    for field, value, match in (("fold", frontend.KIND_DENSE, "DFT product kind 0 is not built for streams"),
                                ("fold", frontend.KIND_FOLD_TF, "DFT product kind 3 is not built for streams"),
                                ("prep", 0, "front-end prep 0"), ("hop", 80, "hop 80"), ("in_window_len", 8000, "in_window_len 8000")):
        bad = _lib.FrontendCfg.from_buffer_copy(cfg)
        setattr(bad, field, value)
        rc, msg = tick(cfg=bad)
        assert rc == -1 and match in msg, (field, rc, msg)
        rc = lib.vadx_frontend_logmel_stream(C.byref(bad), p, p, p, 1697, p, p, 2, 10, p, 20, 10, None)
        msg = lib.vadx_last_error().decode()
        assert rc == -1 and "vadx_frontend_logmel_stream" in msg and ("is not built for streams" in msg), (field, msg)
    rc = lib.vadx_frontend_logmel_stream(C.byref(cfg), p, p, p, 1697, p, p, 2, 10, p, 19, 10, None)
    assert rc == -1 and "do not fit" in lib.vadx_last_error().decode()
    rc = lib.vadx_frontend_logmel_stream(C.byref(cfg), p, p, None, 1697, p, p, 2, 10, p, 20, 10, None)
    assert rc == -1 and "NULL argument" in lib.vadx_last_error().decode()


def test_a_non_published_layout_has_no_stream_entry():
    """The C entry takes the published 3x2x64 weights by name (prologue, blocks 2 - 4, tail): there is no `blocks` argument to get wrong;
    the Python class refuses an engine built on another layout (above), and vadx.marblenet.check_blocks still decides what an engine takes."""
    fields = [n for n, _ in _lib.MarbleNetStreamWeights._fields_]
    assert fields[:3] == ["p_dw", "p_pw", "p_pb"] and fields[-2:] == ["dec_w", "dec_b"] and len(fields) == 18
    assert C.sizeof(_lib.MarbleNetStreamWeights) == 34 * C.sizeof(C.c_void_p)
