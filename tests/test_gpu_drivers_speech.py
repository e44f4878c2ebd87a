"""GPU: the script-level drivers with save_speech_audio -- `detect_table`, the cut made from the device table, the timestamp files from
the table's read-back.  Each writes the wav that slicing the file by the rows it wrote gives (the nearest sample, the rule of
vadx.chunks.from_seconds), and the same timestamp files as the call without the argument."""
import os
import wave

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import audio_io, chunks, drivers, weights

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WAV = os.path.join(GOLD, "vad_sample.wav")
NEAR, FAR = os.path.join(GOLD, "dfsmn_nearend_mic.wav"), os.path.join(GOLD, "dfsmn_farend_speech.wav")
QUIET = lambda *_: None                                                           # noqa: E731


def sliced(path, rows):
    pcm = audio_io.load_wav(path, 16000)
    parts = [pcm[s:e] for s, e in chunks.from_seconds([rows], 16000)[0]]
    return np.concatenate(parts) if parts else np.zeros(0, np.int16)


def check(run, files, tmp_path, cut_from=None):
    """`run(files, second, indices, **extra)`: a single path, then a list"""
    read = lambda p: open(p).read()                                               # noqa: E731
    out = str(tmp_path / "speech.wav")
    seen = 0
    for arg in (files[0], list(files)):
        s0, i0, s1, i1 = (str(tmp_path / n) for n in ("s0.txt", "i0.txt", "s1.txt", "i1.txt"))
        base = run(arg, s0, i0)
        got = run(arg, s1, i1, save_speech_audio=out)
        assert got == base
        if isinstance(arg, list):
            assert len(got) == len(arg)
            for k in range(len(arg)):
                assert read(f"{s1}.{k}") == read(f"{s0}.{k}") and read(f"{i1}.{k}") == read(f"{i0}.{k}")
                want = sliced((cut_from or arg)[k], got[k])
                assert np.array_equal(audio_io.load_wav(f"{out}.{k}"), want)
                seen += len(got[k])
        else:
            assert read(s1) == read(s0) and read(i1) == read(i0)
            assert np.array_equal(audio_io.load_wav(out), sliced((cut_from or [arg])[0], got))
            seen += len(got)
    print(f"{seen} segments written")
    return seen


@pytest.fixture(scope="module")
def second_file(tmp_path_factory):
    pth = str(tmp_path_factory.mktemp("speech") / "burst.wav")
    with wave.open(pth, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(weights.burst_clips(1, 37000, seed=901)[0].tobytes())
    return pth


def test_fsmn_driver_saves_the_speech(tmp_path, second_file):
    from vadx import fsmn
    eng, nz = fsmn.FsmnEngine("synthetic:1234"), np.random.default_rng(1).standard_normal((2, 20000))
    run = lambda f, s, i, **kw: drivers.inference_fsmn(f, eng, s, i, pad_noise=nz if isinstance(f, list) else nz[:1], echo=QUIET, **kw)   # noqa: E731
    check(run, [WAV, second_file], tmp_path)


def test_firered_driver_saves_the_speech(tmp_path, second_file):
    from vadx import firered
    eng, nz = firered.FireRedEngine("synthetic:1234"), np.random.default_rng(2).standard_normal((2, 20000))
    run = lambda f, s, i, **kw: drivers.inference_firered(f, eng, s, i, pad_noise=nz if isinstance(f, list) else nz[:1], echo=QUIET, **kw)   # noqa: E731
    check(run, [WAV, second_file], tmp_path)


def test_marblenet_driver_saves_the_speech(tmp_path, second_file):
    from vadx import marblenet
    eng = marblenet.MarbleNetEngine("synthetic:1234")
    run = lambda f, s, i, **kw: drivers.inference_marblenet(f, eng, s, i, echo=QUIET, **kw)                                   # noqa: E731
    check(run, [WAV, second_file], tmp_path)


def test_dfsmn_drivers_save_the_speech(tmp_path, second_file):
    from vadx import dfsmn
    eng = dfsmn.DfsmnEngine("synthetic:1234")
    nz, nz2 = np.random.default_rng(3).standard_normal((2, 20000)), np.random.default_rng(4).standard_normal((2, 20000))
    fars = {NEAR: FAR, FAR: NEAR}

    def pair(f, s, i, **kw):
        many = isinstance(f, list)
        return drivers.inference_dfsmn(f, [fars[x] for x in f] if many else fars[f], eng, s, i, pad_noise_near=nz if many else nz[:1],
                                       pad_noise_far=nz2 if many else nz2[:1], echo=QUIET, **kw)
    check(pair, [NEAR, FAR], tmp_path)
    eng.set_near_only_constants(*weights.dfsmn_near_only_constants(1234))
    run = lambda f, s, i, **kw: drivers.inference_dfsmn_near_only(f, eng, s, i, pad_noise=nz if isinstance(f, list) else nz[:1], echo=QUIET, **kw)   # noqa: E731
    check(run, [WAV, second_file], tmp_path)
