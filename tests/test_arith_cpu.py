"""CPU, no library load: the one fp16 x 2 range guard (_lib.range_guarded) driven by fake launches and flag readers, through the bare
function and through the engines' own wiring of it, and the one default-arithmetic parser behind both environment variables."""
import pytest

import vadx  # noqa: F401
from vadx import _lib, silero


class _Owner:
    range_fallbacks = 0


class _Fakes:
    """run(mode) -> a result naming the mode; read_flag() -> `raised` once, clearing it (as every engine's reader does)"""

    def __init__(self, raised):
        self.raised, self.runs, self.reads = raised, [], 0

    def run(self, mode, *extra):
        self.runs.append(mode)
        return ("out", mode) + extra

    def read_flag(self, *_):
        self.reads += 1
        was, self.raised = self.raised, False
        return was


def test_guard_h2_with_a_clear_flag_runs_once():
    o, f = _Owner(), _Fakes(False)
    assert _lib.range_guarded(o, "h2", f.run, f.read_flag, "split") == ("out", "h2")
    assert f.runs == ["h2"] and f.reads == 1 and o.range_fallbacks == 0


@pytest.mark.parametrize("fallback", ["split", "f32", None])       # Silero / FSMN / FireRed, MarbleNet, the DFSMN session
def test_guard_h2_with_a_raised_flag_returns_the_fallback_run(fallback):
    o, f = _Owner(), _Fakes(True)
    o.range_fallbacks = 3
    assert _lib.range_guarded(o, "h2", f.run, f.read_flag, fallback) == ("out", fallback)
    assert f.runs == ["h2", fallback] and f.reads == 1 and o.range_fallbacks == 4


@pytest.mark.parametrize("mode", ["split", "f32"])
def test_guard_never_reads_the_flag_off_h2(mode):
    o, f = _Owner(), _Fakes(True)
    assert _lib.range_guarded(o, mode, f.run, f.read_flag, "split") == ("out", mode)
    assert f.runs == [mode] and f.reads == 0 and o.range_fallbacks == 0


def test_arith_blobs_guarded_is_that_guard():
    """ArithBlobs hands run() the (cfg, blob) of the mode it runs, reads the flag of the "h2" blob, and falls back to "split"."""
    f = _Fakes(True)
    built = []

    def build(mode):
        built.append(mode)
        return "cfg-" + mode, "blob-" + mode
    b = _lib.ArithBlobs(build, lambda cfg, blob: (int(f.read_flag()), 7.0e4) if (cfg, blob) == ("cfg-h2", "blob-h2") else None)
    b.arithmetic = "h2"
    assert b.guarded(f.run) == ("out", "split", "cfg-split", "blob-split")
    assert f.runs == ["h2", "split"] and f.reads == 1 and b.range_fallbacks == 1 and built == ["h2", "split"]
    assert b.guarded(f.run) == ("out", "h2", "cfg-h2", "blob-h2") and f.reads == 2 and b.range_fallbacks == 1     # the flag was cleared
    b.arithmetic = "f32"
    assert b.guarded(f.run) == ("out", "f32", "cfg-f32", "blob-f32") and f.reads == 2


def test_silero_engine_guarded_is_that_guard():
    """SileroEngine._guarded (every clips* entry and the stream tick go through it): the engine's own flag reader for the network of the
    sampling rate, "split" as the fallback, and "h2" only where that network's blob has its fp16 x 2 section."""
    f = _Fakes(True)
    e = silero.SileroEngine.__new__(silero.SileroEngine)
    e.arithmetic, e.h2_ok, e.h2_ok_8k, e.range_fallbacks = "h2", True, False, 0
    rates = []
    e.range_flag = lambda reset=True, sampling_rate=16000: (rates.append(sampling_rate), (int(f.read_flag()), 7.0e4))[1]
    assert e._guarded(f.run, 16000) == ("out", "split") and e.range_fallbacks == 1 and rates == [16000]
    assert e._guarded(f.run, 16000) == ("out", "h2") and e.range_fallbacks == 1 and f.reads == 2
    assert e._guarded(f.run, 8000) == ("out", "split") and f.reads == 2               # no fp16 x 2 section at 8 kHz: bf16 x 3, unguarded


def test_marblenet_run_is_that_guard(monkeypatch):
    """MarbleNetEngine.run: its own two flag words (read, and cleared when raised), float32 as the fallback"""
    import types
    import torch
    from vadx import marblenet
    monkeypatch.setattr(_lib, "lib", lambda: None)
    e = marblenet.MarbleNetEngine.__new__(marblenet.MarbleNetEngine)
    e.torch, e.device, e.fused, e.arithmetic, e.h2_ok, e.range_fallbacks = torch, torch.device("cpu"), True, "h2", True, 0
    e._flag = torch.tensor([1, 0x47800000], dtype=torch.int32)
    e.frontend = lambda L: types.SimpleNamespace(logmel=lambda a, w, n: torch.zeros(2, 5, 80))
    runs = []
    e._run_fused = lambda x, N, T, mode: (runs.append(mode), ("out", mode))[1]
    audio = torch.zeros(2, 800, dtype=torch.int16)
    assert e.run(audio) == ("out", "f32") and runs == ["h2", "f32"] and e.range_fallbacks == 1 and e._flag.tolist() == [0, 0]
    assert e.run(audio) == ("out", "h2") and runs == ["h2", "f32", "h2"] and e.range_fallbacks == 1
    e.arithmetic, e._flag[0] = "f32", 1
    assert e.run(audio) == ("out", "f32") and e._flag.tolist() == [1, 0] and e.range_fallbacks == 1            # flag not read off "h2"


def test_dfsmn_session_run_is_that_guard():
    """DfsmnEngine.run: the net's flag words, and as the fallback the same sweep with the LSTMs' fp16 x 2 forms off -- for that sweep only,
    and never switching on what the caller had switched off."""
    import types
    import torch
    from vadx import dfsmn
    e = dfsmn.DfsmnEngine.__new__(dfsmn.DfsmnEngine)
    e.torch, e.device, e.L, e.T_A, e.sub_batch, e.range_fallbacks = torch, torch.device("cpu"), 160, 3, 2, 0
    net = e.iccrn = types.SimpleNamespace(arithmetic="h2", range_flag=torch.tensor([1, 0x47800000], dtype=torch.int32), lstm_t_h2=True)
    seen = []

    def run_sub(near, far, W, ws):
        seen.append((near.shape[0], net.lstm_t_h2))
        return torch.full((near.shape[0] * W, e.T_A), float(len(seen))), None
    e._run_sub = run_sub
    near = torch.zeros(3, 160, dtype=torch.int16)
    vad = e.run(near, near)
    assert seen == [(2, True), (1, True), (2, False), (1, False)] and vad[:, 0].tolist() == [3.0, 3.0, 4.0]
    assert e.range_fallbacks == 1 and net.range_flag.tolist() == [0, 0] and net.lstm_t_h2 is True
    del seen[:]
    e.run(near, near)
    assert seen == [(2, True), (1, True)] and e.range_fallbacks == 1
    del seen[:]
    net.lstm_t_h2 = False                                              # a caller's own switch stays as it is
    e.run(near, near)
    assert seen == [(2, False), (1, False)] and net.lstm_t_h2 is False
    del seen[:]
    net.arithmetic, net.lstm_t_h2, net.range_flag[0] = "split", True, 1
    e.run(near, near)
    assert seen == [(2, True), (1, True)] and net.range_flag.tolist() == [1, 0] and e.range_fallbacks == 1      # flag not read off "h2"


@pytest.mark.parametrize("env,fn,store,what", [("VADX_GEMM", _lib.gemm_mode, _lib._gemm_default, "gemm"),
                                               ("VADX_SILERO_ENCODER", silero.encoder_mode, silero._default_mode, "encoder")])
def test_default_arithmetic_from_the_environment(monkeypatch, env, fn, store, what):
    saved = store[0]
    try:
        _check_default(monkeypatch, env, fn, store, what)
    finally:
        store[0] = saved


def _check_default(monkeypatch, env, fn, store, what):
    other = "VADX_SILERO_ENCODER" if env == "VADX_GEMM" else "VADX_GEMM"
    monkeypatch.setenv(other, "fp8")                                  # each default reads its own variable only
    for text, want in (("0", "f32"), ("1", "split"), ("2", "h2"), ("bf16x3", "split"), ("f16x2", "h2"),
                       ("f32", "f32"), ("split", "split"), ("h2", "h2"), (" F16X2 ", "h2"), ("", "h2")):
        store[0] = None
        monkeypatch.setenv(env, text)
        assert fn() == want and fn() == want
    store[0] = None
    monkeypatch.delenv(env)
    assert fn() == "h2"
    store[0] = None
    monkeypatch.setenv(env, "fp8")
    with pytest.raises(ValueError) as ei:
        fn()
    assert str(ei.value) == f"{env} must be one of ['f32', 'h2', 'split'], got 'fp8'"
    # the setter: returns the previous value, keeps its own stored default, and validates with its own wording
    store[0] = None
    monkeypatch.setenv(env, "1")
    assert fn("f32") == "split" and fn() == "f32" and fn("h2") == "f32"
    with pytest.raises(ValueError) as ei:
        fn("bf16x3")
    assert str(ei.value) == f"{what} mode must be one of ['f32', 'h2', 'split'], got 'bf16x3'"
    assert fn() == "h2"


def test_one_arithmetic_table():
    assert _lib.GEMM_MODES == {"f32": _lib.ARITH["f32"], "split": _lib.ARITH["split"], "h2": _lib.ARITH["h2"]}
    assert (_lib.ARITH["auto"], _lib.ARITH["f32"], _lib.ARITH["bf16x3"], _lib.ARITH["f16x2"]) == (0, 1, 2, 3)      # include/vadx.h: VADX_ARITH_*
