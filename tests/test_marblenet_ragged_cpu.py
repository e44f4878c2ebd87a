"""CPU: MarbleNet's ragged-batch entry points (vadx_frontend_logmel_ragged, vadx_sepconv_block_ragged, vadx_marblenet_block2_ragged,
vadx_marblenet_tail_ragged) exist under the unchanged ABI number and refuse bad arguments on the host before any device call;
vadx.ragged.RaggedFrames lays clips of any lengths end to end with the frame prefixes and tile tables the header documents."""
import ctypes as C
import re

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, frontend, marblenet, ragged, weights

NAMES = ("vadx_frontend_logmel_ragged", "vadx_sepconv_block_ragged", "vadx_marblenet_block2_ragged", "vadx_marblenet_tail_ragged")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_symbols_and_abi(lib):
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    header = int(re.search(r"^#define\s+VADX_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M).group(1))
    assert lib.vadx_abi_version() == header == _lib.ABI_VERSION == 10
    for name in NAMES + ("vadx_marblenet_ragged",):                      # declared, and recorded in the ABI history comment
        assert len(re.findall(r"\b%s\b" % name, text)) >= 2, name
    assert hasattr(ragged, "RaggedFrames") and hasattr(marblenet.MarbleNetEngine, "run_ragged")
    assert hasattr(frontend.Frontend, "logmel_ragged")


LENGTHS = (1, 159, 160, 161, 319, 320, 2560, 10079, 10080, 10240, 16000, 20481, 72345)


def _clips(lengths=LENGTHS):
    rng = np.random.default_rng(3)
    return [rng.integers(-3000, 3000, n).astype(np.int16) for n in lengths]


def test_tables_against_numpy():
    """Host mode (device=None): the tables are numpy arrays, nothing is uploaded."""
    clips = _clips()
    rf = ragged.RaggedFrames.from_clips(clips, device=None)
    n = np.array(LENGTHS, dtype=np.int64)
    F = n // 160 + 1
    T1 = (F - 1) // 2 + 1
    assert len(rf) == len(clips) and rf.device is None
    assert rf.pcm.dtype == np.int16 and rf.pcm.ndim == 1 and rf.pcm.shape[0] == n.sum()
    assert rf.clip_off.dtype == np.int64 and np.array_equal(rf.clip_off, np.concatenate([[0], np.cumsum(n)[:-1]]))
    assert rf.clip_len.dtype == np.int32 and np.array_equal(rf.clip_len, n)
    for b, c in enumerate(clips):                                         # end to end: no padding, no filler
        assert np.array_equal(rf.pcm[rf.clip_off[b]:rf.clip_off[b] + rf.clip_len[b]], c), b
    assert np.array_equal(rf.mel_frames, F) and np.array_equal(rf.enc_frames, T1)
    for got, per_clip, tile in ((rf.mel_first, F, None), (rf.enc_first, T1, None), (rf.fe_tile_first, F, 64), (rf.enc_tile_first, T1, 32)):
        counts = per_clip if tile is None else -(-per_clip // tile)
        assert got.dtype == np.int32 and np.array_equal(got, np.concatenate([[0], np.cumsum(counts)])), tile
    assert rf.n_mel == F.sum() and rf.n_enc == T1.sum()
    for clip_of, first, per_clip, tile, total in ((rf.fe_tile_clip, rf.fe_tile_first, F, 64, rf.n_fe_tiles),
                                                  (rf.enc_tile_clip, rf.enc_tile_first, T1, 32, rf.n_enc_tiles)):
        assert clip_of.dtype == np.int32 and clip_of.shape == (total,) and total == first[-1]
        want = np.concatenate([np.full(-(-int(f) // tile), b) for b, f in enumerate(per_clip)])
        assert np.array_equal(clip_of, want)
        for g, b in enumerate(clip_of):                                   # what a workgroup derives: its tile lies inside its clip
            k = g - first[b]
            assert 0 <= k and k * tile < per_clip[b] and g < first[b + 1]
    # the tail m-tiles of the front-end's 64-frame tiling: all four widths occur
    assert {int(-(-(f % 64) // 16)) for f in F} >= {0, 1}
    with pytest.raises(ValueError, match="host-only"):
        rf.encoder_tables()


def test_bad_clips_are_refused():
    clips = _clips()[:3]
    with pytest.raises(ValueError, match="at least one"):
        ragged.RaggedFrames.from_clips([], device=None)
    with pytest.raises(ValueError, match="empty"):
        ragged.RaggedFrames.from_clips([clips[0], clips[1][:0]], device=None)
    with pytest.raises(ValueError, match="int16"):
        ragged.RaggedFrames.from_clips([c.astype(np.float32) for c in clips], device=None)
    with pytest.raises(ValueError, match="int16"):
        ragged.RaggedFrames.from_clips([clips[0], clips[1].astype(np.int32)], device=None)
    with pytest.raises(ValueError, match="int32"):
        ragged._prefix(np.array([2 ** 30, 2 ** 30], dtype=np.int64), "frames")


def _fe_cfg(kind=frontend.KIND_SPLIT_H2):
    _, cfg, cos, sin, fb = frontend.host_tables("marblenet", 16000)
    cfg.fold = kind
    return cfg


def test_bad_arguments_are_refused_on_the_host(lib):
    """Every refusal the header lists comes back as VADX_EINVAL with the function's name in vadx_last_error() -- before any HIP call
    (there is no device here; the pointers below are host memory nothing may touch)."""
    buf = (C.c_char * 256)()
    ptr = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731

    cfg = _fe_cfg()
    fe = lambda **kw: lib.vadx_frontend_logmel_ragged(*[kw.get(k, v) for k, v in (                                      # noqa: E731
        ("cfg", C.byref(cfg)), ("packed", ptr), ("mel_kb", ptr), ("pcm", ptr), ("pcm_len", 40000), ("clip_off", ptr), ("clip_len", ptr),
        ("mel_first", ptr), ("tile_first", ptr), ("tile_clip", ptr), ("clips", 3), ("n_tiles", 5), ("mel_total", 253), ("out", ptr),
        ("stream", None))])
    name = b"vadx_frontend_logmel_ragged"
    for k in ("cfg", "packed", "mel_kb", "pcm", "clip_off", "clip_len", "mel_first", "tile_first", "tile_clip", "out"):
        assert fe(**{k: None}) == -1 and name in err() and b"NULL" in err(), k
    for k, bad in (("clips", 0), ("clips", -1), ("n_tiles", 0), ("mel_total", 0), ("pcm_len", 0), ("clips", 6), ("n_tiles", 254),
                   ("mel_total", 5 * 64 + 1), ("n_tiles", 3)):
        assert fe(**{k: bad}) == -1 and name in err(), (k, bad)
    for kind in (frontend.KIND_DENSE, frontend.KIND_FOLD_SYM, frontend.KIND_FOLD_PER, frontend.KIND_FOLD_TF, 9):
        bad = _fe_cfg(kind)
        assert fe(cfg=C.byref(bad)) == -1 and name in err() and b"kind %d" % kind in err(), kind
    for prep in (0, 2, 6, 7):
        bad = _fe_cfg()
        bad.prep = prep
        assert fe(cfg=C.byref(bad)) == -1 and name in err() and b"prep %d" % prep in err(), prep
    nopad = _fe_cfg()
    nopad.center_pad = 0
    assert fe(cfg=C.byref(nopad)) == -1 and name in err() and b"centre pad 0" in err()

    rt = _lib.MarbleNetRagged(ptr, ptr, ptr, ptr, 3, 5, 130, 253)

    def tables(**kw):
        t = _lib.MarbleNetRagged(rt.tile_first, rt.tile_clip, rt.frame_first, rt.src_first, rt.clips, rt.n_tiles, rt.frames_total, rt.src_total)
        for k, v in kw.items():
            setattr(t, k, v)
        return C.byref(t)

    f32 = _lib.MarbleNetCfg(_lib.ARITH["f32"], 0, None)
    h2_noflag = _lib.MarbleNetCfg(_lib.ARITH["h2"], 0, None)
    bf16 = _lib.MarbleNetCfg(_lib.ARITH["split"], 0, ptr)
    sc = _lib.SepConvCfg(80, 128, 11, 2, 1, 1, 0, 1)
    pro = lambda **kw: lib.vadx_sepconv_block_ragged(*[kw.get(k, v) for k, v in (                                       # noqa: E731
        ("cfg", C.byref(sc)), ("dw_w", ptr), ("pw_w", ptr), ("pw_b", ptr), ("x", ptr), ("xs_t", 80), ("y", ptr), ("rt", tables()),
        ("stream", None), ("mcfg", C.byref(f32)))])
    blk = lambda **kw: lib.vadx_marblenet_block2_ragged(*[kw.get(k, v) for k, v in (                                    # noqa: E731
        ("cin", 128), ("kernel", 13), ("dw0", ptr), ("pw0", ptr), ("b0", ptr), ("dw1", ptr), ("pw1", ptr), ("b1", ptr), ("res_w", ptr),
        ("res_b", ptr), ("x", ptr), ("y", ptr), ("rt", tables()), ("stream", None), ("cfg", C.byref(f32)))])
    tail = lambda **kw: lib.vadx_marblenet_tail_ragged(*[kw.get(k, v) for k, v in (                                     # noqa: E731
        ("dw", ptr), ("pw", ptr), ("pb", ptr), ("w6", ptr), ("b6", ptr), ("dec_w", ptr), ("dec_b", ptr), ("x", ptr), ("score0", ptr),
        ("score1", ptr), ("rt", tables()), ("stream", None), ("cfg", C.byref(f32)))])
    cases = ((pro, b"vadx_sepconv_block_ragged", ("cfg", "dw_w", "pw_w", "pw_b", "x", "y"), "mcfg", True),
             (blk, b"vadx_marblenet_block2_ragged", ("dw0", "pw0", "b0", "dw1", "pw1", "b1", "res_w", "res_b", "x", "y"), "cfg", False),
             (tail, b"vadx_marblenet_tail_ragged", ("dw", "pw", "pb", "w6", "b6", "dec_w", "dec_b", "x", "score0", "score1"), "cfg", False))
    for fn, name, pointers, cfg_key, with_src in cases:
        for k in pointers + ("rt",):
            assert fn(**{k: None}) == -1 and name in err() and b"NULL" in err(), (name, k)
        for k in ("tile_first", "tile_clip", "frame_first") + (("src_first",) if with_src else ()):
            assert fn(rt=tables(**{k: None})) == -1 and name in err() and b"NULL" in err(), (name, k)
        for k, bad in (("clips", 0), ("clips", -2), ("n_tiles", 0), ("frames_total", 0), ("frames_total", -1),
                       ("clips", 6), ("n_tiles", 131), ("frames_total", 5 * 32 + 1), ("n_tiles", 4)):
            assert fn(rt=tables(**{k: bad})) == -1 and name in err(), (name, k, bad)
        assert fn(**{cfg_key: C.byref(bf16)}) == -1 and name in err() and b"arithmetic" in err(), name        # bf16 x 3: no such form
        assert fn(**{cfg_key: C.byref(h2_noflag)}) == -1 and name in err() and b"range_flag" in err(), name
    for bad in (129, 2 * 130 + 1):                                        # sum T1 <= sum F <= 2 sum T1
        assert pro(rt=tables(src_total=bad)) == -1 and b"src_total" in err(), bad
    for field, bad in (("kernel", 13), ("stride", 1), ("dilation", 2), ("depthwise", 0), ("residual_cin", 64), ("cin", 129), ("cout", 0)):
        other = _lib.SepConvCfg(80, 128, 11, 2, 1, 1, 0, 1)
        setattr(other, field, bad)
        assert pro(cfg=C.byref(other)) == -1 and b"vadx_sepconv_block_ragged" in err() and b"prologue" in err(), (field, bad)
    assert pro(xs_t=79) == -1 and b"xs_t" in err()
    for kw in (dict(cin=80), dict(cin=0), dict(kernel=11), dict(kernel=29)):
        assert blk(**kw) == -1 and b"vadx_marblenet_block2_ragged" in err() and b"3x2x64" in err(), kw


def test_a_list_is_refused_on_another_layout_by_name():
    """As far as it goes without a device: the layout check passes a non-published stack, and the engine's list path names what it was
    built for (the engine itself needs a GPU to construct; both methods refuse before they touch anything but the `fused` flag)."""
    other = [(64, 1, 11, 1, 1, False, True), (64, 2, 13, 1, 1, True, True), (128, 1, 1, 1, 1, False, False)]
    marblenet.check_blocks(other)                                         # a layout the per-sub-block path takes
    assert tuple(tuple(b) for b in other) != tuple(tuple(b) for b in weights.MARBLENET_BLOCKS)

    class _Stub:                                                          # the refusal needs nothing but the flag
        fused = False
    with pytest.raises(ValueError, match="published MarbleNet 3x2x64"):
        marblenet.MarbleNetEngine.run_ragged(_Stub(), None)
    with pytest.raises(ValueError, match="published MarbleNet 3x2x64"):
        marblenet.MarbleNetEngine.detect(_Stub(), [np.zeros(8, np.int16)])
