"""CPU: the FireRed stream-tick entry points (added under ABI 10) exist, size their record as documented, report the group limit, and refuse
every bad argument on the host with a message that names the function -- before any device call (there is no device here; the pointers
below are host memory nothing may touch)."""
import ctypes as C

import pytest

import vadx  # noqa: F401
from vadx import _lib, build, firered, weights

T = 14                                   # frames of the reference's 2 560-sample chunk


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def cfg_of(arith="f32", frames=T, **over):
    c = dict(dict(weights.FIRERED_CFG, N2=0, S2=0), **over)
    cfg = _lib.FireRedCfg()
    for k in ("idim", "R", "M", "H", "P", "N1", "S1", "N2", "S2", "odim"):
        setattr(cfg, k, int(c[k]))
    cfg.frames, cfg.arithmetic = frames, _lib.ARITH[arith]
    return cfg, c


def test_symbols_and_abi(lib):
    for name in ("vadx_firered_stream_state_bytes", "vadx_firered_stream_group_max", "vadx_firered_stream_tick"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.vadx_abi_version() == 10 == _lib.ABI_VERSION
    assert hasattr(firered, "FireRedStreamBatch")


def test_group_max(lib):
    for F in (1, 14, 15, 56, 57, 112):
        assert lib.vadx_firered_stream_group_max(F) == 112 // F, F
    assert lib.vadx_firered_stream_group_max(0) == 0 and lib.vadx_firered_stream_group_max(113) == 0
    assert lib.vadx_firered_stream_group_max(-3) == 0


@pytest.mark.parametrize("over", [{}, dict(N1=32, S1=3, R=2), dict(H=17, P=1, R=2), dict(N1=2)], ids=str)
def test_state_bytes(lib, over):
    cfg, c = cfg_of(**over)
    cache = c["R"] * c["P"] * (c["N1"] - 1) * c["S1"] * 4
    for S in (1, 3, 64, 4097):
        n = lib.vadx_firered_stream_state_bytes(C.byref(cfg), S)
        assert n % 16 == 0 and n >= S * cache + S * 8 and n <= S * (cache + 128) + 16, (S, n)
    cfg.frames = 999                     # the record does not depend on the chunk length
    assert lib.vadx_firered_stream_state_bytes(C.byref(cfg), 3) == 3 * cache + (-3 * cache) % 16 + 3 * 128
    for S in (0, -1):
        assert lib.vadx_firered_stream_state_bytes(C.byref(cfg), S) == 0
    assert lib.vadx_firered_stream_state_bytes(None, 4) == 0
    bad, _ = cfg_of(H=300)
    assert lib.vadx_firered_stream_state_bytes(C.byref(bad), 4) == 0


def test_bad_arguments_are_refused_on_the_host(lib):
    S = 3
    cfg, _ = cfg_of()
    nb = lib.vadx_firered_stream_state_bytes(C.byref(cfg), S)
    buf = (C.c_char * (2 * nb + 64))()
    base = (C.addressof(buf) + 15) & ~15
    rec_a, rec_b, ptr = base, base + nb, base                            # two disjoint aligned records
    post = _lib.StreamVadPostParams(5, 0.4, 5, 8, 2000, 20)
    tick = lambda **kw: lib.vadx_firered_stream_tick(*[kw.get(k, v) for k, v in (                                     # noqa: E731
        ("cfg", C.byref(cfg)), ("packed", ptr), ("logmel", ptr), ("streams", S), ("chunks", 1), ("group", 0), ("post", C.byref(post)),
        ("reset", None), ("active", None), ("state_in", rec_a), ("state_out", rec_b), ("probs", ptr), ("segments", ptr), ("counts", ptr),
        ("cap", 4), ("open_start", ptr), ("stream", None))])
    err = lambda: lib.vadx_last_error()                                                                                # noqa: E731
    name = b"vadx_firered_stream_tick"
    for k in ("cfg", "packed", "logmel", "post", "state_in", "state_out", "probs", "segments", "counts", "open_start"):
        assert tick(**{k: None}) == -1 and name in err() and b"NULL" in err(), k
    for k in ("streams", "chunks", "cap"):
        for bad in (0, -2):
            assert tick(**{k: bad}) == -1 and name in err() and (k + "=" + str(bad)).encode() in err(), (k, bad)
    assert tick(chunks=9) == -1 and name in err() and b"126" in err() and b"112" in err()        # 9 chunks of 14 frames
    assert tick(chunks=8, group=2) == -1 and name in err() and b"group=2" in err()               # F = 112: one stream per workgroup
    for bad in (-1, 9):                                                                          # F = 14: 1 .. 8 streams, or 0
        assert tick(group=bad) == -1 and name in err() and b"group=%d" % bad in err(), bad
    la, _ = cfg_of(N2=2, S2=1)
    assert tick(cfg=C.byref(la)) == -1 and name in err() and b"N2" in err()
    wide = _lib.StreamVadPostParams(17, 0.4, 5, 8, 2000, 20)
    assert tick(post=C.byref(wide)) == -1 and name in err() and b"smooth_window_size 17" in err()
    assert tick(state_out=rec_a) == -1 and name in err() and b"overlap" in err()
    assert tick(state_out=rec_a + nb - 16) == -1 and b"overlap" in err()
    assert tick(state_in=rec_b, state_out=rec_b - 16) == -1 and b"overlap" in err()
    # a split arithmetic on widths the split kernels do not take, and a config outside the limits
    for arith in ("split", "h2"):
        narrow, _ = cfg_of(arith, H=64, P=32)
        assert tick(cfg=C.byref(narrow)) == -1 and name in err() and b"unsupported config" in err(), arith
    long_chunk, _ = cfg_of(frames=113)
    assert tick(cfg=C.byref(long_chunk)) == -1 and name in err()


def test_stream_batch_needs_a_gpu_engine():
    """FireRedStreamBatch has no host path: it is built on a FireRedEngine, which refuses to exist without a device."""
    with pytest.raises(TypeError):
        firered.FireRedStreamBatch(object(), 4)
