"""CPU: the long-window FSMN entry points (vadx_fsmn_long_workspace_bytes, vadx_fsmn_window_stats_long, vadx_fsmn_run_long,
vadx_fsmn_clips_long) exist under the unchanged ABI number, are declared in the header, and refuse bad arguments on the host, by name,
before any device call (there is no device here; the pointers below are host memory nothing may touch)."""
import ctypes as C
import re

import pytest

import vadx  # noqa: F401
from vadx import _lib, build, weights

L, T = 160000, 1001
LONG_MAX = 60001
NAMES = ("vadx_fsmn_long_workspace_bytes", "vadx_fsmn_window_stats_long", "vadx_fsmn_run_long", "vadx_fsmn_clips_long")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_header_and_abi(lib):
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    header = int(re.search(r"^#define\s+VADX_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M).group(1))
    assert lib.vadx_abi_version() == header == _lib.ABI_VERSION == 10
    for name in NAMES:                                                   # declared, and recorded in the ABI history comment
        assert len(re.findall(r"\b%s\b" % name, text)) >= 2, name
    assert int(re.search(r"^#define\s+VADX_FSMN_LONG_MAX_FRAMES\s+(\d+)\s*$", text, flags=re.M).group(1)) == LONG_MAX
    # each new entry point cites the reference seam it replaces
    for name, seam in (("vadx_fsmn_run_long", "Inference_FSMN_VAD_ONNX.py:177-187"), ("vadx_fsmn_clips_long", "Inference_FSMN_VAD_ONNX.py:176-234")):
        decl = text.index("int %s(" % name)
        assert seam in text[text.rindex("/*", 0, decl):decl], name


def test_workspace_bytes(lib):
    ws = lib.vadx_fsmn_long_workspace_bytes
    assert ws(0, T) == 0 and ws(-1, T) == 0 and ws(1, 0) == 0 and ws(1, -5) == 0 and ws(1, LONG_MAX + 1) == 0
    assert ws(1, 1) > 0 and ws(1, LONG_MAX) >= 2 * 4 * LONG_MAX
    frames = (1, 6, 64, 65, 101, 112, 113, 128, 129, 1001, 12001, LONG_MAX)
    for rows in (1, 2, 5, 4096):
        sizes = [ws(rows, f) for f in frames]
        assert sizes == sorted(sizes) and all(s >= rows * 8 * f for s, f in zip(sizes, frames)), rows     # a float of P(silence) and one gate bit per frame
    for f in frames:
        sizes = [ws(rows, f) for rows in (1, 2, 3, 64, 4096)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), f
        assert ws(4096, f) >= 8 * 4096                                   # also covers the stats call's 8 bytes per window


def _dims(frames=T):
    w = weights.fsmn_synthetic(1234)
    d = _lib.FsmnDims()
    d.input_affine_dim, d.linear_dim = w["in1_w"].shape[0], w["in2_w"].shape[0]
    d.output_affine_dim, d.output_dim = w["out1_w"].shape[0], w["out2_w"].shape[0]
    d.frames, d.speech_2_noise_ratio, d.arithmetic = frames, 1.0, _lib.ARITH["split"]
    return d


def _loop_params(lb=30):
    lp = _lib.FsmnLoopParams()
    lp.look_backward, lp.one_minus_speech_threshold, lp.noise_db_init, lp.snr_threshold = lb, 1.0, 4.0, 1.0
    lp.speaking_score, lp.silence_score = 0.5, 0.5
    return lp


def test_bad_arguments_are_refused_on_the_host(lib):
    buf = (C.c_char * 256)()
    ptr = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731
    four = (C.c_void_p * 4)(ptr, ptr, ptr, ptr)

    who = b"vadx_fsmn_window_stats_long"
    stats = lambda **kw: lib.vadx_fsmn_window_stats_long(*[kw.get(k, v) for k, v in (                                  # noqa: E731
        ("audio", ptr), ("row_stride", 2 * L), ("win_stride", L), ("batch", 3), ("windows_per_clip", 2), ("window_len", L), ("frames", T),
        ("means", ptr), ("db", ptr), ("workspace", ptr), ("stream", None))])
    for k in ("audio", "means", "db", "workspace"):
        assert stats(**{k: None}) == -1 and who in err() and b"NULL" in err() and k.encode() in err(), k
    assert stats(workspace=ptr + 4) == -1 and who in err() and b"workspace" in err()
    for k, bad in (("batch", 0), ("batch", -2), ("windows_per_clip", 0), ("window_len", 511), ("window_len", 9600160), ("frames", 0),
                   ("frames", LONG_MAX + 1), ("row_stride", 2 * L - 1), ("row_stride", -1)):
        assert stats(**{k: bad}) == -1 and who in err() and k.encode() in err(), (k, bad)

    who = b"vadx_fsmn_run_long"
    d = _dims()
    run = lambda **kw: lib.vadx_fsmn_run_long(*[kw.get(k, v) for k, v in (                                             # noqa: E731
        ("dims", C.byref(d)), ("packed", ptr), ("logmel", ptr), ("db", ptr), ("cache_in", C.byref(four)), ("cache_out", C.byref(four)),
        ("thr", ptr), ("noise_db", ptr), ("batch", 2), ("score", ptr), ("noisy_db", ptr), ("psil", None), ("workspace", ptr), ("stream", None))])
    for k in ("dims", "packed", "logmel", "db", "cache_in", "cache_out", "thr", "noise_db", "score", "noisy_db", "workspace"):
        assert run(**{k: None}) == -1 and who in err() and b"NULL" in err() and k.encode() in err(), k
    hole = (C.c_void_p * 4)(ptr, ptr, None, ptr)
    assert run(cache_in=C.byref(hole)) == -1 and who in err() and b"cache" in err()
    assert run(cache_out=C.byref(hole)) == -1 and who in err() and b"cache" in err()
    for bad in (0, -1, LONG_MAX + 1):
        assert run(dims=C.byref(_dims(bad))) == -1 and who in err() and b"frames" in err(), bad
    for bad in (0, -4):
        assert run(batch=bad) == -1 and who in err() and b"batch" in err(), bad
    assert run(workspace=ptr + 2) == -1 and who in err() and b"workspace" in err()

    who = b"vadx_fsmn_clips_long"
    lp, slide = _loop_params(30), T - 30
    clips = lambda **kw: lib.vadx_fsmn_clips_long(*[kw.get(k, v) for k, v in (                                         # noqa: E731
        ("dims", C.byref(d)), ("packed", ptr), ("logmel", ptr), ("db", ptr), ("batch", 2), ("n_windows", 5), ("max_windows", 4),
        ("win_first", ptr), ("order", None), ("lp", C.byref(lp)), ("cache_ws", ptr), ("flags", ptr), ("flag_stride", 4 * slide + 30),
        ("noise_trace", None), ("workspace", ptr), ("stream", None))])
    for k in ("dims", "packed", "logmel", "db", "lp", "cache_ws", "flags", "workspace"):
        assert clips(**{k: None}) == -1 and who in err() and b"NULL" in err() and k.encode() in err(), k
    for bad in (0, LONG_MAX + 1):
        assert clips(dims=C.byref(_dims(bad))) == -1 and who in err() and b"frames" in err(), bad
    for k in ("batch", "n_windows", "max_windows"):
        for bad in (0, -1):
            assert clips(**{k: bad}) == -1 and who in err() and k.encode() in err(), (k, bad)
    # counts that do not fit each other: a ragged batch gives every clip 1 .. max_windows windows, a rectangular one exactly max_windows
    for kw in (dict(n_windows=1), dict(n_windows=9), dict(win_first=None, n_windows=5), dict(win_first=None, n_windows=7)):
        assert clips(**kw) == -1 and who in err() and b"n_windows" in err(), kw
    assert clips(flag_stride=4 * slide + 29) == -1 and who in err() and b"flag_stride" in err()
    assert clips(win_first=None, n_windows=8, flag_stride=4 * slide + 29) == -1 and b"flag_stride" in err()
    # the windows of a grid must advance: look_backward >= frames - 1 leaves no stride
    for bad in (-1, T - 1, T, T + 7):
        assert clips(lp=C.byref(_loop_params(bad))) == -1 and who in err() and b"look_backward" in err(), bad
    assert clips(lp=C.byref(_loop_params(0)), flag_stride=4 * T - 1) == -1 and b"flag_stride" in err()      # look-back 0: max_windows * T flags
    assert clips(workspace=ptr + 1) == -1 and who in err() and b"workspace" in err()
