"""CPU: vadx.prepare's host mirror, the arithmetic contract of csrc/prepare.hip, pinned to the functions it stands for -- np.mean,
timestamps.normalize_to_int16 / normalise_audio, clips.pad_to_window_grid, RaggedBatch.from_clips, audio_io._tomono / _ratecv -- on the
input set the GPU tests use (tests/_prepare_cases.py), and shown to tell the wrong summation orders apart on that set."""
import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, audio_io, build, clips, prepare, ragged, timestamps

import _prepare_cases as pc

F = np.float32
MS_LENGTHS = list(range(1, 301)) + [8191, 8192, 8193, 11039, 11040, 16000, 16383, 16384, 16385, 24577]


@pytest.mark.parametrize("sigma", [30, 3000, 20000])
def test_ms32_is_numpys_mean_of_squares(sigma):
    rng = np.random.default_rng(sigma)
    for n in MS_LENGTHS:
        x = np.clip(np.rint(rng.standard_normal(n) * sigma), -32768, 32767).astype(np.float32)
        got, want = prepare.ms32(x), np.mean(x * x)
        assert got.dtype == want.dtype == np.float32
        assert got.tobytes() == want.tobytes(), (n, got, want)


def test_an_unchunked_pairwise_sum_is_not_numpys():
    """the 8192-element reduction buffer is part of the contract: without it three of the lengths above already differ"""
    for n in (11039, 11040, 16000):
        differ = 0
        for seed in range(20):
            x = np.clip(np.rint(np.random.default_rng(seed).standard_normal(n) * 20000), -32768, 32767).astype(np.float32)
            differ += int(F(prepare._pairwise32(x * x) / F(n)) != np.mean(x * x))
        assert differ > 0, n


def test_peak_scale_is_normalize_to_int16s():
    """every peak 1 .. 32768: the scale, seen through the value the peak itself maps to; all 65536 inputs on a handful of peaks"""
    for p in range(1, 32769):
        x = np.asarray([0, -p if p == 32768 else p], dtype=np.int16)
        y, s = prepare.scale_host(x, "peak")
        assert s == F(32767.0) / F(p)
        assert np.array_equal(y, timestamps.normalize_to_int16(x.astype(np.float32)))
    every = np.arange(-32768, 32768).astype(np.int16)
    for p in (1, 2, 3, 255, 4681, 12345, 21845, 32766, 32767, 32768):
        x = every[np.abs(every.astype(np.int32)) <= p]
        y, _ = prepare.scale_host(x, "peak")
        want = timestamps.normalize_to_int16(x.astype(np.float32))
        assert y.dtype == want.dtype == np.int16 and np.array_equal(y, want), p
    y, s = prepare.scale_host(np.zeros(9, dtype=np.int16), "peak")
    assert s == 1 and not y.any()


@pytest.mark.parametrize("target", [8192.0, 3000.0, 60000.0])
def test_rms_mode_is_normalise_audio(target):
    rng = np.random.default_rng(int(target))
    for n in (1, 7, 8, 129, 8191, 8193, 16385, 24577):
        for kind in pc.KINDS:
            x = pc.signal(kind, n, rng)
            y, g = prepare.scale_host(x, "rms", target)
            want = timestamps.normalise_audio(x, target)
            assert y.dtype == want.dtype == np.int16 and np.array_equal(y, want), (n, kind)
            if kind == "silence":
                assert g == 1                                      # the guard `r > 0`: an all-zero clip is not scaled at all
    assert prepare.scale_host(np.zeros(5, dtype=np.int16), "rms")[0].tolist() == [0] * 5


def test_fill_wraps_like_numpys_cast():
    """fill = the low 16 bits of trunc(float64(rt) * z): what numpy's astype(int16) of the float64 product gives, for |z| up to 40"""
    z = np.concatenate([np.linspace(-40, 40, 4001), np.random.default_rng(5).standard_normal(4000)])
    for rt in (F(0), F(0.5), F(7.25), F(8191.97), F(18918.6), F(32768)):
        want = (rt * z).astype(np.int16)
        assert (rt * z).dtype == np.float64
        assert np.array_equal(prepare.fill_host(rt, z), want), rt
    assert np.any(np.abs(F(32768) * z) > 40000)                   # the wrap was exercised


def test_pad_count_is_pad_to_window_grids():
    z = np.zeros(40000)
    for window, stride in pc.GRIDS.values():
        for n in set(pc.lengths_of(window, stride)) | set(range(window - 3, window + 2 * stride + 3, 97)):
            got = len(clips.pad_to_window_grid(np.ones(n, dtype=np.int16), window, stride, z)) - n
            assert clips.pad_count(n, window, stride) == got, (window, stride, n)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("grid", list(pc.GRIDS))
def test_prepare_host_is_from_clips(grid, mode):
    window, stride = pc.GRIDS[grid]
    want = pc.reference(grid, mode)
    got = prepare.prepare_host(pc.clips_of(grid), window, stride, pc.noise_of(grid), mode)
    pc.same_tables(got, want)
    assert pc.first_difference(got.pcm_host, want.pcm_host) is None
    for b in (0, 5, len(got) - 1):
        assert np.array_equal(got.padded(b), want.padded(b))
    pads = want.padded_lengths - want.lengths
    assert pads.max() >= 8193 or grid == "small"                  # a tail that crosses an 8192 chunk is in the set


def test_prepare_host_draws_the_references_noise():
    """pad_noise=None: one np.random.normal(size=pad) per padded clip, in clip order -- from_clips' own draws"""
    cl = pc.clips_of("small")[:12]
    np.random.seed(1234)
    want = ragged.RaggedBatch.from_clips(cl, 512, 256, None, pc.PREP["peak"], device=None)
    np.random.seed(1234)
    got = prepare.prepare_host(cl, 512, 256, None, "peak")
    assert pc.first_difference(got.pcm_host, want.pcm_host) is None


def test_prepare_host_frames_is_ragged_frames():
    cl = pc.clips_of("small")
    for mode in (None, "rms"):
        want = ragged.RaggedFrames.from_clips([c if mode is None else timestamps.normalise_audio(c) for c in cl], device=None)
        got = prepare.prepare_host(cl, None, None, None, mode)
        for name in ragged.RaggedFrames.TABLES:
            assert np.array_equal(getattr(got, name), getattr(want, name)), name


# ---- non-vacuity: the input set tells the wrong arithmetics apart -----------------------------------------------------------------------

def _ms_sequential(x):
    sq = x * x
    return F(np.cumsum(sq, dtype=np.float32)[-1] / F(len(sq)))


def _ms_unchunked(x):
    return F(prepare._pairwise32(x * x) / F(len(x)))


def _ms_exact(x):
    return F(F(int(np.sum(x.astype(np.int64) ** 2))) / F(len(x)))


def _fused_sum(x):
    """numpy's pairwise tree with every `r + x * x` fused: the product is not rounded (exact in float64, like the sum before its rounding)"""
    n = len(x)
    d = x.astype(np.float64)
    acc = lambda r, v: F(np.float64(r) + v * v)            # noqa: E731
    if n < 8:
        r = F(0)
        for v in d:
            r = acc(r, v)
        return r
    if n <= 128:
        r = [F(F(v) * F(v)) for v in d[:8]]
        m = n - n % 8
        for i in range(8, m, 8):
            r = [acc(r[j], d[i + j]) for j in range(8)]
        res = F(F(F(r[0] + r[1]) + F(r[2] + r[3])) + F(F(r[4] + r[5]) + F(r[6] + r[7])))
        for v in d[m:]:
            res = acc(res, v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F(_fused_sum(x[:n2]) + _fused_sum(x[n2:]))


def _ms_fused(x):
    total = F(0)
    for c0 in range(0, len(x), prepare.CHUNK):
        total = F(total + _fused_sum(x[c0:c0 + prepare.CHUNK]))
    return F(total / F(len(x)))


@pytest.mark.parametrize("wrong", [_ms_sequential, _ms_unchunked, _ms_exact, _ms_fused], ids=["sequential", "unchunked", "exact", "fused"])
def test_the_input_set_tells_a_wrong_sum_apart(wrong):
    """each wrong mean of squares gives ANOTHER packed vector than the mirror on the FSMN grid's clips, in RMS mode (the scale and the
    tail) -- so a kernel that sums that way fails tests/test_gpu_prepare.py"""
    window, stride = pc.GRIDS["fsmn"]
    want = pc.reference("fsmn", "rms")
    got = prepare.prepare_host(pc.clips_of("fsmn"), window, stride, pc.noise_of("fsmn"), "rms", ms=wrong)
    assert pc.first_difference(got.pcm_host, want.pcm_host) is not None


# ---- ragged ingest -------------------------------------------------------------------------------------------------------------------

def _ingest_set():
    rng = np.random.default_rng(8)
    spec = [(48000, 2, 1), (48000, 2, 2), (48000, 2, 3), (48000, 2, 1000), (16000, 1, 1), (16000, 1, 1000), (8000, 1, 1), (8000, 1, 2), (8000, 1, 3),
            (8000, 1, 1000), (44100, 2, 4410), (22050, 1, 3001)]
    return [rng.integers(-32768, 32768, n * ch).astype(np.int16) for _, ch, n in spec], [s[1] for s in spec], [s[0] for s in spec]


def test_ragged_ingest_mirror_is_tomono_ratecv_and_audioop():
    raws, chans, rates = _ingest_set()
    pcm, offs, lens = audio_io.ingest_ragged_host(raws, chans, rates, 16000)
    assert np.all(offs % 8 == 0)
    covered = np.zeros(len(pcm), dtype=bool)
    for r, ch, rate, o, n in zip(raws, chans, rates, offs, lens):
        x = audio_io._tomono(r) if ch == 2 else r
        want = audio_io._ratecv(x, rate, 16000) if rate != 16000 else x
        assert n == len(want) and np.array_equal(pcm[o:o + n], want)
        if audio_io._audioop is not None:
            data = r.tobytes()
            if ch == 2:
                data = audio_io._audioop.tomono(data, 2, 0.5, 0.5)
            if rate != 16000:
                data, _ = audio_io._audioop.ratecv(data, 2, 1, rate, 16000, None)
            assert np.array_equal(pcm[o:o + n], np.frombuffer(data, dtype=np.int16))
        covered[o:o + n] = True
    assert not pcm[~covered].any()
    for bad in (dict(channels=[3] + chans[1:]), dict(rates=[0] + rates[1:]), dict(rates=[7] + rates[1:], sample_rate=65537)):
        kw = dict(channels=chans, rates=rates, sample_rate=16000)
        kw.update(bad)
        with pytest.raises(ValueError):
            audio_io.ingest_ragged_host(raws, **kw)


# ---- the C ABI refuses bad arguments before any HIP call (so this runs without a GPU) ------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_prepare_entry_points_validate_before_touching_the_device(lib):
    P = 0x10000                                                    # a well-aligned non-NULL address that is never dereferenced
    need = lib.vadx_prepare_workspace_bytes(3, 5)
    assert need >= 16 * 3 + 8 * 5 and need % 16 == 0
    assert lib.vadx_prepare_workspace_bytes(0, 5) == 0 and lib.vadx_prepare_workspace_bytes(3, 0) == 0
    good = dict(src=P, src_elems=100, src_off=P, lengths=P, dst_off=P, tile_first=P, tile_clip=P, batch=3, tiles=5, window=512, stride=256, mode=2,
                target=8192.0, ws=P, ws_bytes=need, noise=P, noise_elems=10, noise_off=P, dst=P, dst_elems=64)

    def stats(**kw):
        a = dict(good, **kw)
        return lib.vadx_prepare_stats(a["src"], a["src_elems"], a["src_off"], a["lengths"], a["tile_first"], a["tile_clip"], a["batch"], a["tiles"],
                                      a["mode"], a["ws"], a["ws_bytes"], None)

    def scale(**kw):
        a = dict(good, **kw)
        return lib.vadx_prepare_scale(a["src"], a["src_elems"], a["src_off"], a["lengths"], a["dst_off"], a["tile_first"], a["batch"], a["tiles"],
                                      a["window"], a["stride"], a["mode"], a["target"], a["ws"], a["ws_bytes"], None)

    def write(**kw):
        a = dict(good, **kw)
        return lib.vadx_prepare_write(a["src"], a["src_elems"], a["src_off"], a["lengths"], a["dst_off"], a["noise"], a["noise_elems"], a["noise_off"],
                                      a["batch"], a["tiles"], a["mode"], a["ws"], a["ws_bytes"], a["dst"], a["dst_elems"], None)

    shared = [dict(src=None), dict(src_off=None), dict(lengths=None), dict(ws=None), dict(src=P + 2), dict(ws=P + 8), dict(src_off=P + 4),
              dict(batch=0), dict(tiles=0), dict(mode=3), dict(mode=-1), dict(ws_bytes=need - 1), dict(src_elems=-1)]
    for fn, extra in ((stats, [dict(tile_first=None), dict(tile_clip=None), dict(tile_clip=P + 2)]),
                      (scale, [dict(dst_off=None), dict(window=0), dict(window=508), dict(stride=-8), dict(stride=12), dict(target=0.0),
                               dict(target=float("inf")), dict(dst_off=P + 4)]),
                      (write, [dict(dst=None), dict(dst=P + 8), dict(noise=None), dict(noise_off=None), dict(noise=P + 4), dict(dst_elems=0),
                               dict(noise_elems=-1)])):
        for kw in shared + extra:
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert fn.__name__[:4] in lib.vadx_last_error().decode() or "vadx_prepare" in lib.vadx_last_error().decode()
    r = lib.vadx_ingest_pcm16_ragged
    args = [P, 100, P, P, P, P, 16000, P, P, P, 3, 5, P, 64, P, None]
    for i, v in ((0, None), (2, None), (4, None), (12, None), (14, None), (10, 0), (11, 0), (6, 0), (1, -1), (13, -1), (2, P + 4), (4, P + 2), (0, P + 1)):
        a = list(args)
        a[i] = v
        assert r(*a) == -1, (i, v)
