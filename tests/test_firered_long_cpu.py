"""CPU: the FireRed long-window entry points (vadx_firered_long_workspace_bytes, vadx_firered_run_long, vadx_frontend_logmel_ragged_snip)
exist under the unchanged ABI number, are declared in the header with the reference seam they replace, and refuse bad arguments on the host,
by the argument's name, before any device call (there is no device here; the pointers below are host memory nothing may touch).  The table
builder is held to a numpy restatement, the workspace rule to 3 * P * frames floats, every Python refusal of the long engine happens before
an engine or a GPU is touched, and oracle.firered.run_clip(window=len(clip)) is ONE window -- the dynamic rule the GPU tests rely on."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, build, firered, ragged, weights
from vadx import frontend as vfe
from oracle import firered as ofr

NAMES = ("vadx_firered_long_workspace_bytes", "vadx_firered_run_long", "vadx_frontend_logmel_ragged_snip")
LONG_MAX, TILE = 360000, 64


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
    for name in NAMES + ("vadx_firered_long_tables",):                   # declared, and recorded in the ABI history comment
        assert len(re.findall(r"\b%s\b" % name, text)) >= 2, name
    assert int(re.search(r"^#define\s+VADX_FIRERED_LONG_MAX_FRAMES\s+(\d+)", text, flags=re.M).group(1)) == LONG_MAX == _lib.FIRERED_LONG_MAX_FRAMES
    assert int(re.search(r"^#define\s+VADX_FIRERED_LONG_TILE\s+(\d+)", text, flags=re.M).group(1)) == TILE == _lib.FIRERED_LONG_TILE == ragged.LONG_TILE
    assert LONG_MAX >= firered.valid_frame_count(3600 * 16000) == 359998        # the reference's 3600 s cap fits
    assert firered.valid_frame_count(firered.LONG_MAX_SAMPLES) == LONG_MAX and firered.valid_frame_count(firered.LONG_MAX_SAMPLES + 1) == LONG_MAX + 1
    # each new entry point cites the reference seam it replaces
    section = text[text.index("FireRed windows of ANY length"):text.index("int vadx_firered_run_long(")]
    for seam in ("Export_FireRedVAD.py:29,48,785-807", "Inference_FireRed_ONNX.py:541-547", ":644-650", "Inference_FireRed_ONNX.py:567-572",
                 "Export_FireRedVAD.py:229"):
        assert seam in section, seam
    decl = text.index("int vadx_frontend_logmel_ragged_snip(")
    assert "Inference_FireRed_ONNX.py:541-547" in text[text.rindex("/*", 0, decl):decl]
    # the struct binding has the header's fields, in its order
    body = text[text.index("typedef struct vadx_firered_long_tables {"):text.index("} vadx_firered_long_tables;")]
    fields = re.findall(r"\*(\w+);", body) + [f.strip() for f in re.search(r"int32_t ([\w, ]+);", body).group(1).split(",")]
    assert fields == [f for f, _ in _lib.FireRedLongTables._fields_]


def _cfg(frames=1, **kw):
    c = _lib.FireRedCfg()
    for k, v in dict(weights.FIRERED_CFG, **kw).items():
        setattr(c, k, int(v))
    c.frames, c.arithmetic = frames, _lib.ARITH["f32"]
    return c


def test_workspace_size_rule(lib):
    ws = lib.vadx_firered_long_workspace_bytes
    for P in (1, 24, 120, 128):
        for n in (1, 63, 64, 65, 998, 4096 * 998, 8500 * 998, 2 ** 31 - 1):
            assert ws(C.byref(_cfg(P=P)), n) == 3 * P * n * 4, (P, n)
    assert ws(C.byref(_cfg(frames=LONG_MAX)), 7) == ws(C.byref(_cfg(frames=113)), 7) == 3 * 128 * 7 * 4      # cfg->frames is not read
    assert ws(None, 5) == 0 and ws(C.byref(_cfg()), 0) == 0 and ws(C.byref(_cfg()), -3) == 0 and ws(C.byref(_cfg()), 2 ** 31) == 0
    assert ws(C.byref(_cfg(P=129)), 5) == 0 and ws(C.byref(_cfg(R=17)), 5) == 0 and ws(C.byref(_cfg(idim=64)), 5) == 0


def test_bad_arguments_are_refused_on_the_host(lib):
    buf = (C.c_char * 256)()
    ptr = (C.addressof(buf) + 15) & ~15
    err = lambda: lib.vadx_last_error()                                                                                 # noqa: E731
    who = b"vadx_firered_run_long"

    def tables(**kw):
        v = dict(frame_first=ptr, tile_first=ptr, tile_clip=ptr, clips=3, n_tiles=5, frames_total=300)
        v.update(kw)
        return _lib.FireRedLongTables(*[v[k] for k, _ in _lib.FireRedLongTables._fields_])
    cfg, need = _cfg(), 3 * 128 * 300 * 4
    run = lambda **kw: lib.vadx_firered_run_long(*[kw.get(k, v) for k, v in (                                          # noqa: E731
        ("cfg", C.byref(cfg)), ("packed", ptr), ("logmel", ptr), ("tables", C.byref(tables())), ("probs", ptr), ("workspace", ptr),
        ("workspace_bytes", need), ("stream", None))])
    for k in ("cfg", "packed", "logmel", "tables", "probs", "workspace"):
        assert run(**{k: None}) == -1 and who in err() and b"NULL" in err() and k.encode() in err(), k
    for k in ("frame_first", "tile_first", "tile_clip"):
        assert run(tables=C.byref(tables(**{k: None}))) == -1 and who in err() and b"NULL" in err() and k.encode() in err(), k
    for k in ("clips", "n_tiles", "frames_total"):
        for bad in (0, -1):
            assert run(tables=C.byref(tables(**{k: bad}))) == -1 and who in err() and k.encode() in err(), (k, bad)
    # counts that do not fit each other: every tile has 1 .. 64 frames
    for kw in (dict(n_tiles=301), dict(n_tiles=4), dict(frames_total=4, n_tiles=5), dict(frames_total=321)):
        assert run(tables=C.byref(tables(**kw))) == -1 and who in err() and b"n_tiles" in err() and b"frames_total" in err(), kw
    for bad in (0, -1, LONG_MAX + 1):                                    # frames above the cap
        assert run(cfg=C.byref(_cfg(frames=bad))) == -1 and who in err() and b"frames" in err(), bad
    for kw in (dict(P=129), dict(H=257), dict(odim=5), dict(N1=33), dict(R=0)):
        assert run(cfg=C.byref(_cfg(**kw))) == -1 and who in err() and b"cfg" in err(), kw
    split_on_other_widths = _cfg(H=64, P=32)
    split_on_other_widths.arithmetic = _lib.ARITH["h2"]
    assert run(cfg=C.byref(split_on_other_widths)) == -1 and who in err() and b"cfg" in err()
    for bad in (0, need - 1):                                            # a workspace that is too small: VADX_ENOSPACE, by name
        assert run(workspace_bytes=bad) == -2 and who in err() and b"workspace_bytes" in err() and str(need).encode() in err(), bad

    who = b"vadx_frontend_logmel_ragged_snip"
    _, fcfg, _, _, _ = vfe.host_tables("firered", 16000)
    fcfg.fold = vfe.KIND_SPLIT_H2
    snip = lambda **kw: lib.vadx_frontend_logmel_ragged_snip(*[kw.get(k, v) for k, v in (                              # noqa: E731
        ("cfg", C.byref(fcfg)), ("packed", ptr), ("mel_kb_host", ptr), ("pcm", ptr), ("pcm_len", 100000), ("clip_off", ptr), ("clip_len", ptr),
        ("mel_first", ptr), ("tile_first", ptr), ("tile_clip", ptr), ("clips", 7), ("n_tiles", 5), ("mel_total", 300), ("out", ptr),
        ("stream", None))])
    for k in ("cfg", "packed", "mel_kb_host", "pcm", "clip_off", "clip_len", "mel_first", "tile_first", "tile_clip", "out"):
        assert snip(**{k: None}) == -1 and who in err() and b"NULL" in err() and k.encode() in err(), k
    for k in ("clips", "n_tiles", "mel_total", "pcm_len"):
        assert snip(**{k: 0}) == -1 and who in err() and k.encode() in err(), k
    for kw in (dict(n_tiles=301), dict(mel_total=321)):
        assert snip(**kw) == -1 and who in err() and b"n_tiles" in err() and b"mel_total" in err(), kw
    centred = vfe.host_tables("marblenet", 16000)[1]
    centred.fold = vfe.KIND_SPLIT_H2
    assert snip(cfg=C.byref(centred)) == -1 and who in err() and b"centre pad" in err()
    dense = vfe.host_tables("firered", 16000)[1]
    dense.fold = vfe.KIND_DENSE
    assert snip(cfg=C.byref(dense)) == -1 and who in err() and b"kind" in err()
    resampled = vfe.host_tables("firered", 8000, in_sample_rate=8000)[1]
    resampled.fold = vfe.KIND_SPLIT_H2
    assert snip(cfg=C.byref(resampled)) == -1 and who in err() and b"prep" in err()


def restated_tables(frames):
    """frame_first, tile_first, tile_clip of vadx_firered_long_tables, written out clip by clip"""
    ff, tf, tc = [0], [0], []
    for b, f in enumerate(frames):
        tiles = -(-int(f) // TILE)
        ff.append(ff[-1] + int(f))
        tf.append(tf[-1] + tiles)
        tc += [b] * tiles
    return np.array(ff, np.int32), np.array(tf, np.int32), np.array(tc, np.int32)


def test_table_builder_against_a_numpy_restatement():
    rng = np.random.default_rng(8)
    for B in list(range(1, 66)) + [127, 128, 129, 511, 512, 1024, 1025]:
        frames = rng.choice([0, 1, 63, 64, 65, 127, 128, 129, 998], size=B) if B % 2 else rng.integers(0, 400, size=B)
        for got, want in zip(ragged.long_tables(frames), restated_tables(frames)):
            assert got.dtype == np.int32 and np.array_equal(got, want), B
        # the packed batch derives the frames from the lengths (snip edges; under 400 samples: none) and keeps the clips end to end
        lengths = np.where(frames > 0, 400 + 160 * (np.maximum(frames, 1) - 1) + rng.integers(0, 160, size=B), rng.integers(1, 400, size=B))
        clips = [np.full(int(n), b % 100, dtype=np.int16) for b, n in enumerate(lengths)]
        pc = ragged.PackedClips.from_clips(clips, device=None)
        assert np.array_equal(pc.frames, frames) and np.array_equal(pc.frames, [firered.valid_frame_count(int(n)) for n in lengths])
        assert np.array_equal(pc.frame_first, restated_tables(frames)[0]) and np.array_equal(pc.tile_clip, restated_tables(frames)[2])
        assert np.array_equal(pc.clip_off, np.concatenate([[0], np.cumsum(lengths)[:-1]])) and pc.clip_off.dtype == np.int64
        assert pc.pcm.shape == (int(lengths.sum()),) and all(pc.pcm[int(o)] == b % 100 for b, o in enumerate(pc.clip_off))
        assert (pc.n_frames, pc.n_tiles, len(pc)) == (int(frames.sum()), len(restated_tables(frames)[2]), B)
    rect = ragged.long_tables(np.full(5, 130))                           # a rectangular batch: the same tables with equal counts
    assert rect[0].tolist() == [0, 130, 260, 390, 520, 650] and rect[1].tolist() == [0, 3, 6, 9, 12, 15] and rect[2].tolist() == sorted(list(range(5)) * 3)
    with pytest.raises(ValueError, match="at least one"):
        ragged.long_tables([])
    with pytest.raises(ValueError, match="negative"):
        ragged.long_tables([3, -1])
    with pytest.raises(ValueError, match="int16"):
        ragged.PackedClips.from_clips([np.zeros(500, np.float32)], device=None)
    with pytest.raises(ValueError, match="empty"):
        ragged.PackedClips.from_clips([np.zeros(0, np.int16)], device=None)
    with pytest.raises(ValueError, match="clip 1 has 11 frames"):       # a listed clip above the cap is refused by name
        ragged.PackedClips.from_clips([np.zeros(500, np.int16), np.zeros(2000, np.int16)], device=None, max_frames=10)


def test_python_refusals_touch_no_engine_and_no_gpu(monkeypatch):
    def no_gpu():
        raise AssertionError("the GPU was touched before the refusal")
    w = weights.firered_synthetic(1234)
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(_lib, "lib", no_gpu)
    with pytest.raises(ValueError, match="input_audio_length=None.*long_windows=True"):
        firered.FireRedEngine(w, None)
    with pytest.raises(ValueError, match="in_sample_rate"):
        firered.FireRedEngine(w, 48000, in_sample_rate=48000, long_windows=True)
    with pytest.raises(ValueError, match="in_sample_rate"):
        firered.FireRedEngine(w, None, in_sample_rate=8000, long_windows=True)
    for bad in (399, 0, firered.LONG_MAX_SAMPLES + 1):
        with pytest.raises(ValueError, match="input_audio_length"):
            firered.FireRedEngine(w, bad, long_windows=True)
    with pytest.raises(ValueError, match="input_audio_length=None"):
        firered.FireRedSession(w, None)
    # the accepted range passes the argument check (and then asks for the GPU)
    for ok in (400, 16000, 18320, firered.LONG_MAX_SAMPLES, None):
        firered.check_long_arguments(ok, 16000, True)
        with pytest.raises(AssertionError, match="GPU was touched"):
            firered.FireRedEngine(w, ok, long_windows=True)
    # a clip over 3600 s in a dynamic list is refused by name from its length alone (no sample is read: a strided view of one zero)
    with pytest.raises(ValueError, match=r"clip 1 has 360001 frames.*3600 s"):
        ragged.PackedClips.from_lengths([16000, firered.LONG_MAX_SAMPLES + 1], max_frames=firered.LONG_MAX_FRAMES)
    pc = ragged.PackedClips.from_lengths([16000, firered.LONG_MAX_SAMPLES, 399], max_frames=firered.LONG_MAX_FRAMES)
    assert pc.frames.tolist() == [98, firered.LONG_MAX_FRAMES, 0] and pc.n_tiles == 2 + 5625 and pc.device is None and pc.pcm is None


def test_oracle_run_clip_at_the_clip_length_is_one_window():
    """The dynamic rule: window = len(clip) pads nothing, so the driver's loop runs the net once over the whole clip -- the probabilities
    are those of one forward call, and differ from the 1 s windows' at the window edges."""
    w = weights.firered_synthetic(1234)
    ow = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in w.items()}
    fe = ofr.Frontend()
    for n in (400, 5000, 30123):
        clip = weights.burst_clips(1, n, seed=n)[0]
        seg, probs, dec = ofr.run_clip(fe, ow, clip, None, window=n)
        one = ofr.forward(fe, ow, torch.from_numpy(clip.copy()).reshape(1, 1, -1))[0, 0].numpy()
        assert probs.shape == (firered.valid_frame_count(n),) == one.shape and np.array_equal(probs, one), n
    grid = ofr.run_clip(fe, ow, clip, np.zeros(16000), window=16000)[1]
    assert grid.shape[0] <= probs.shape[0] and not np.array_equal(grid, probs[:grid.shape[0]])
