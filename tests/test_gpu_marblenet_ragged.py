"""GPU: MarbleNet on ragged batches (clips of any lengths in one launch sequence, vadx.ragged.RaggedFrames): every clip's slice of
every output is bit for bit what the one-clip call gives -- at every edge of the front-end's 64-frame and the encoder's 32-frame
tiling, whatever the neighbours -- through `detect` and the driver, under the fp16 x 2 range protocol, and with tables that lie."""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import _lib, audio_io, drivers, marblenet, ragged, vadpost, weights

pytestmark = pytest.mark.gpu
WAV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vad_sample.wav")
SEED = 1234
POST = (3, 0.5, 10, 1000, 10, 3, 0)


@pytest.fixture(autouse=True, params=["f32", "h2"])
def gemm(request):
    """Every test of this file runs on both arithmetics of the fused blocks' 1x1 convs, like tests/test_gpu_marblenet.py."""
    prev = _lib.gemm_mode(request.param)
    yield request.param
    _lib.gemm_mode(prev)


# log-mel frames per clip: the 64-frame front-end tile with tails of 1, 2, 3 m-tiles and none; encoder frames T1 = 1, 1, 2, 8, 9, 24,
# 25, 32, 32, 33, 64, 64, 65, 65, 97, 129: the 32-frame tile full and partial, one to five tiles, the tail's 28-frame halo across a
# tile edge, both parities in front of the stride-2 prologue
FRAMES = (1, 2, 3, 16, 17, 48, 49, 63, 64, 65, 127, 128, 129, 130, 193, 257)
REM = (1, 159, 0)        # n = 160 (F - 1) + r, r cycling through 0, 1, 159 -- started at 1, so that the one-frame clip is not empty


def _edge_clips():
    """The clips of test 1 in shuffled order, seeded noise at different levels (neighbours differ)."""
    rng = np.random.default_rng(20)
    clips = []
    for i, f in enumerate(FRAMES):
        n = 160 * (f - 1) + REM[i % 3]
        level = (30.0, 300.0, 3000.0, 9000.0)[i % 4]
        clips.append(np.clip(np.rint(rng.standard_normal(n) * level), -32768, 32767).astype(np.int16))
    order = np.random.default_rng(21).permutation(len(clips))
    return [clips[k] for k in order]


_ENGINES, _ALONE = {}, {}


def _engine():
    if "eng" not in _ENGINES:
        _ENGINES["eng"] = marblenet.MarbleNetEngine(weights.marblenet_synthetic(SEED))
    return _ENGINES["eng"]


def _alone(gemm, key, clip):
    """The one-clip path on `clip`, computed once per arithmetic and shared: (logmel [F, 80], s0 [T1], s1 [T1]) on the host."""
    if (gemm, key) not in _ALONE:
        eng = _engine()
        lm = eng.frontend(len(clip)).logmel(clip[None])
        s0, s1, slen = eng.run(clip[None])
        assert slen == s1.shape[1] - 1
        _ALONE[(gemm, key)] = (lm[0].cpu().numpy(), s0[0].cpu().numpy(), s1[0].cpu().numpy())
    return _ALONE[(gemm, key)]


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_every_tile_edge_is_bitwise_the_one_clip_path(gemm):
    eng, clips = _engine(), _edge_clips()
    rf = eng.ragged(clips)
    assert sorted(rf.mel_frames.tolist()) == sorted(FRAMES)
    assert sorted(rf.enc_frames.tolist()) == [1, 1, 2, 8, 9, 24, 25, 32, 32, 33, 64, 64, 65, 65, 97, 129]
    fe = eng.frontend_ragged()
    lm = fe.logmel_ragged(rf).cpu().numpy()
    assert lm.shape == (sum(FRAMES), 80)
    before = eng.range_fallbacks
    s0, s1, enc_first = eng.run_ragged(rf)
    assert eng.range_fallbacks == before and eng.mode() == gemm
    s0, s1 = s0.cpu().numpy(), s1.cpu().numpy()
    assert np.array_equal(enc_first, rf.enc_first_host) and s0.shape == s1.shape == (enc_first[-1],)
    for b, c in enumerate(clips):
        want_lm, want0, want1 = _alone(gemm, ("edge", b), c)
        m0, m1, e0, e1 = rf.mel_first_host[b], rf.mel_first_host[b + 1], enc_first[b], enc_first[b + 1]
        assert _same_bytes(lm[m0:m1], want_lm), (b, len(c))
        assert _same_bytes(s0[e0:e1], want0) and _same_bytes(s1[e0:e1], want1), (b, len(c))
    assert eng._fe_ragged is fe and eng.frontend_ragged() is fe              # one Frontend object serves every length


def test_a_kind_without_a_ragged_form_is_refused_not_replaced(gemm, monkeypatch):
    """VADX_FRONTEND_FOLD=0 selects the dense product, which has no ragged form: the list path says so instead of running another."""
    monkeypatch.setenv("VADX_FRONTEND_FOLD", "0")
    eng = marblenet.MarbleNetEngine(weights.marblenet_synthetic(SEED))
    clips = _edge_clips()[:3]
    with pytest.raises(ValueError, match="split-product kinds"):
        eng.run_ragged(eng.ragged(clips))
    with pytest.raises(ValueError, match="split-product kinds"):
        eng.detect(clips)
    assert len(eng.detect(weights.burst_clips(2, 4000, seed=3))) == 2                # the rectangular path takes the dense kind as before


def test_neighbours_do_not_matter(gemm):
    eng = _engine()
    rng = np.random.default_rng(30)
    three = [np.rint(rng.standard_normal(n) * 2000).astype(np.int16) for n in (10401, 5281, 20799)]
    full_scale = np.where(rng.random(7777) < 0.5, -32768, 32767).astype(np.int16)
    quiet = np.rint(rng.standard_normal(3333) * 20).astype(np.int16)
    packs = ([three[0], full_scale, three[1], three[2]], [quiet, three[2], three[1], full_scale, three[0]])
    where = ((0, 2, 3), (4, 2, 1))
    got = []
    for pack, idx in zip(packs, where):
        rf = eng.ragged(pack)
        lm = eng.frontend_ragged().logmel_ragged(rf).cpu().numpy()
        s0, s1, ef = eng.run_ragged(rf)
        s0, s1 = s0.cpu().numpy(), s1.cpu().numpy()
        got.append([(lm[rf.mel_first_host[b]:rf.mel_first_host[b + 1]], s0[ef[b]:ef[b + 1]], s1[ef[b]:ef[b + 1]]) for b in idx])
    for k in range(3):
        for a, b in zip(got[0][k], got[1][k]):
            assert _same_bytes(a, b), k
        for a, b in zip(got[0][k], _alone(gemm, ("three", k), three[k])):
            assert _same_bytes(a, b), k


def test_detect_on_a_list(gemm):
    eng = _engine()
    wav = audio_io.load_wav(WAV)
    clips = _edge_clips() + [wav[:12345], wav[20000:70001], wav]
    out, track, dec, nf = eng.detect(clips, return_probs=True)
    assert len(out) == len(clips) and track.shape[0] == dec.shape[0] == len(clips) and track.shape[1] == max(nf)
    empty = 0
    for b, c in enumerate(clips):
        o1, t1, d1 = eng.detect(c[None], return_probs=True)
        assert nf[b] == t1.shape[1] == (len(c) // 160 + 1 - 1) // 2, b
        assert torch.equal(track[b, :nf[b]], t1[0]) and torch.equal(dec[b, :nf[b]], d1[0]), b
        assert not track[b, nf[b]:].any() and not dec[b, nf[b]:].any(), b
        assert out[b] == o1[0], b
        if nf[b] == 0:
            assert out[b] == []
            empty += 1
    assert empty == 2 and any(out) and out == eng.detect(clips)
    # the static export: every clip on its own 1 s window grid, explicit pad noise
    L = 16000
    wclips = [wav[1000:1000 + n] for n in (4800, 16000, 27200, 48000)]
    noise = np.random.default_rng(31).standard_normal((len(wclips), L))
    wout, wtrack, wdec, wnf = eng.detect(wclips, window_len=L, pad_noise=noise, return_probs=True)
    assert wnf.tolist() == [50, 50, 100, 150]
    for b, c in enumerate(wclips):
        o1, t1, d1 = eng.detect(c[None], window_len=L, pad_noise=noise[b:b + 1], return_probs=True)
        assert wnf[b] == t1.shape[1] and torch.equal(wtrack[b, :wnf[b]], t1[0]) and torch.equal(wdec[b, :wnf[b]], d1[0]), b
        assert wout[b] == o1[0], b
    assert any(wout)
    # a 2-D array keeps the path it had: run + vadpost by hand
    batch = weights.burst_clips(3, 24000, seed=9)
    got, tr, de = eng.detect(batch, return_probs=True)
    s0, s1, slen = eng.run(batch)
    hand = s1[:, :min(slen, s1.shape[1])].contiguous()
    pp = vadpost.VadPostprocessor(*POST, frame_shift_s=0.02, frame_length_s=None, device=eng.device)
    hdec, segs, counts = pp.process_batch(hand)
    segs, counts = segs.cpu().numpy(), counts.cpu().numpy()
    assert torch.equal(tr, hand) and torch.equal(de, hdec)
    assert got == [pp.segments_to_seconds(segs[b, :counts[b]].tolist(), hand.shape[1], 24000 / 16000) for b in range(3)]


def test_driver_hands_a_file_list_over_as_one_ragged_batch(gemm, tmp_path, monkeypatch):
    eng = _engine()
    wav = audio_io.load_wav(WAV)
    paths = []
    for k, (a, n) in enumerate(((0, 30001), (15000, 52000), (40000, 41234))):
        pth = str(tmp_path / f"c{k}.wav")
        with wave.open(pth, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(wav[a:a + n].tobytes())
        paths.append(pth)
    calls = []
    real = marblenet.MarbleNetEngine.run_ragged
    monkeypatch.setattr(marblenet.MarbleNetEngine, "run_ragged", lambda self, rf: (calls.append(len(rf)), real(self, rf))[1])
    quiet = lambda *_: None                                                 # noqa: E731
    sec, idx = str(tmp_path / "s.txt"), str(tmp_path / "i.txt")
    many = drivers.inference_marblenet(paths, eng, sec, idx, echo=quiet)
    assert calls == [3] and any(many)
    for k, pth in enumerate(paths):
        s1, i1 = str(tmp_path / "s1.txt"), str(tmp_path / "i1.txt")
        one = drivers.inference_marblenet(pth, eng, s1, i1, echo=quiet)
        assert many[k] == one
        assert open(f"{sec}.{k}").read() == open(s1).read() and open(f"{idx}.{k}").read() == open(i1).read()
    assert calls == [3]                                                     # a single file keeps the rectangular path


@pytest.mark.parametrize("scale,want_alone", [(3e4, (1, 1, 1)), (1600.0, (0, 1, 0))])
def test_range_protocol_covers_the_whole_ragged_batch(gemm, scale, want_alone):
    """The prologue's 1x1 weights scaled as tests/test_gpu_marblenet.py::test_fp16_range_protocol scales them (3e4), then by 1600.  The
    flag raised inside a three-clip list recomputes the WHOLE batch on float32 MFMAs, counted once, and every clip's scores are those
    of the float32 ragged call.
    Which clips leave the range alone: BatchNorm is folded, so block 1's output grows with the scale, and it is largest for SILENCE
    (log-mel = log 1e-7 = -16.1 in every band; loud noise sits near 0).  The float32 oracle's largest 1x1-conv operand at 3e4 is 2.8e6
    for the silent clip and 5.3e5 for the loud ones: every clip alone is 8 - 43 x past 65504, so that scale cannot show a batch in
    which one clip alone does it.  At 1600 the same figures are 1.5e5 and 2.8e4, a factor 2.3 on either side of 65504: only the
    silent clip flags, and it takes its two in-range neighbours along."""
    if gemm != "h2":
        pytest.skip("the range protocol belongs to the fp16 x 2 arithmetic")
    w = dict(weights.marblenet_synthetic(7))
    w["b0r0_pw"] = np.asarray(w["b0r0_pw"]) * scale
    rng = np.random.default_rng(40)
    clips = [np.rint(rng.standard_normal(9000) * 8000).astype(np.int16), np.zeros(5000, np.int16),
             np.rint(rng.standard_normal(12001) * 8000).astype(np.int16)]
    eng = marblenet.MarbleNetEngine(w)
    assert eng.mode() == "h2"
    alone = []
    for c in clips:
        before = eng.range_fallbacks
        eng.run(c[None])
        alone.append(eng.range_fallbacks - before)
    print("one-clip calls that left the fp16 range:", alone)
    assert tuple(alone) == want_alone
    before = eng.range_fallbacks
    s0, s1, ef = eng.run_ragged(eng.ragged(clips))
    assert eng.range_fallbacks == before + 1 and int(eng._flag[0].item()) == 0
    ref = marblenet.MarbleNetEngine(w)
    ref.arithmetic = "f32"
    r0, r1, _ = ref.run_ragged(ref.ragged(clips))
    assert torch.equal(s0, r0) and torch.equal(s1, r1) and ref.range_fallbacks == 0
    ok = marblenet.MarbleNetEngine(weights.marblenet_synthetic(7))
    ok.run_ragged(ok.ragged(clips))
    assert ok.mode() == "h2" and ok.range_fallbacks == 0                    # in-range audio and weights never flag


# ---- tables that lie: the C entry points, directly
SENTINEL = np.float32(-7.0e37)


class _Slack:
    """A device buffer with `margin` elements of slack on both sides of the `n` a launch may use, everything pre-filled with `fill`:
    even a kernel that ignored its guards and indexed with any value of the tables handed to it (offsets and clamped frame indices
    are bounded by the tables' largest entries times the channel count, which is what the caller sizes `margin` from) stays inside."""

    def __init__(self, n, margin, dtype, fill, device):
        self.n, self.margin = int(n), int(margin)
        self.t = torch.full((self.n + 2 * self.margin,), fill, dtype=dtype, device=device)

    def put(self, src):
        self.t[self.margin:self.margin + self.n] = src.reshape(-1)
        return self

    def ptr(self):
        return self.t.data_ptr() + self.margin * self.t.element_size()

    def host(self):
        return self.t[self.margin:self.margin + self.n].cpu().numpy()

    def margins_untouched(self, fill):
        m = self.margin
        return bool((self.t[:m] == fill).all()) and bool((self.t[m + self.n:] == fill).all())


def _table(host, extra, fill, device):
    """An int table on the device with `extra` more entries behind it (a guard-less kernel handed clip index B reads two past the end)."""
    return torch.from_numpy(np.concatenate([host, np.full(extra, fill, dtype=host.dtype)])).to(device)


def test_bad_tables_stay_inside(gemm):
    eng = _engine()
    dev, lib, st = eng.device, _lib.lib(), eng.stages
    rng = np.random.default_rng(50)
    lengths = (160 * 64 + 5, 160 * 129 + 80, 160 * 16, 160 * 63 + 159, 160 * 192 + 1)      # F = 65, 130, 17, 64, 193; T1 = 33, 65, 9, 32, 97
    clips = [np.rint(rng.standard_normal(n) * 1500).astype(np.int16) for n in lengths]
    rf = ragged.RaggedFrames.from_clips(clips, device=None)
    B, n_mel, n_enc = len(rf), rf.n_mel, rf.n_enc
    F, T1 = rf.mel_frames, rf.enc_frames
    mode = eng.mode()
    sfx = "_h" if mode == "h2" else ""
    mc = _lib.MarbleNetCfg(_lib.ARITH[mode], 0, eng._flag.data_ptr())
    p = lambda a: None if a is None else a.data_ptr()                       # noqa: E731
    fe = eng.frontend_ragged()
    EXTRA = 4
    # the largest frame / sample count any table below can make a kernel form, guards or not: every entry is <= these totals
    frames_bound = n_mel + 64 * (rf.n_fe_tiles + 1)
    pcm_margin = int(rf.pcm_host.shape[0]) + 160 * 64 + 512

    def tables(h):
        return {k: _table(v, EXTRA, v[-1] if k.endswith("first") else 0, dev) for k, v in h.items()}

    good = dict(mel_first=rf.mel_first_host, enc_first=rf.enc_first_host, fe_tile_first=rf.fe_tile_first_host, fe_tile_clip=rf.fe_tile_clip_host,
                enc_tile_first=rf.enc_tile_first_host, enc_tile_clip=rf.enc_tile_clip_host, clip_off=rf.clip_off_host, clip_len=rf.clip_len_host)
    pcm = _Slack(rf.pcm_host.shape[0], pcm_margin, torch.int16, 0, dev).put(torch.from_numpy(rf.pcm_host).to(dev))

    def frontend_launch(h, out):
        d = tables(h)
        with torch.cuda.device(dev):
            _lib.check(lib.vadx_frontend_logmel_ragged(C.byref(fe.cfg), fe.packed.data_ptr(), fe.mel_kb.ctypes.data, pcm.ptr(), pcm.n,
                                                       d["clip_off"].data_ptr(), d["clip_len"].data_ptr(), d["mel_first"].data_ptr(),
                                                       d["fe_tile_first"].data_ptr(), d["fe_tile_clip"].data_ptr(), B, rf.n_fe_tiles, n_mel,
                                                       out.ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        return d

    def rt_of(d):
        return _lib.MarbleNetRagged(d["enc_tile_first"].data_ptr(), d["enc_tile_clip"].data_ptr(), d["enc_first"].data_ptr(),
                                    d["mel_first"].data_ptr(), B, rf.n_enc_tiles, n_enc, n_mel)

    def stage_launch(k, h, x, outs):
        """Stage 0 = the prologue, 1 - 3 = the fused blocks, 4 = the tail; x / outs are _Slack buffers."""
        d = tables(h)
        rt = rt_of(d)
        with torch.cuda.device(dev):
            if k == 0:
                rc = lib.vadx_sepconv_block_ragged(C.byref(st[0]["cfg"]), p(st[0]["dw"]), p(st[0]["pw" + sfx]), p(st[0]["pb"]), x.ptr(), 80,
                                                   outs[0].ptr(), C.byref(rt), _lib.stream_ptr(), C.byref(mc))
            elif k < 4:
                a, b = st[2 * k - 1], st[2 * k]
                rc = lib.vadx_marblenet_block2_ragged(a["cfg"].cin, a["cfg"].kernel, p(a["dw"]), p(a["pw" + sfx]), p(a["pb"]), p(b["dw"]),
                                                      p(b["pw" + sfx]), p(b["pb"]), p(b["rw" + sfx]), p(b["rb"]), x.ptr(), outs[0].ptr(),
                                                      C.byref(rt), _lib.stream_ptr(), C.byref(mc))
            else:
                rc = lib.vadx_marblenet_tail_ragged(p(st[7]["dw"]), p(st[7]["pw" + sfx]), p(st[7]["pb"]), p(st[8]["pw" + sfx]), p(st[8]["pb"]),
                                                    eng.dec_w.data_ptr(), eng.dec_b.data_ptr(), x.ptr(), outs[0].ptr(), outs[1].ptr(),
                                                    C.byref(rt), _lib.stream_ptr(), C.byref(mc))
            _lib.check(rc)
        torch.cuda.synchronize()
        return d

    CH_IN, CH_OUT = (80, 128, 64, 64, 64), (128, 64, 64, 64, 1)

    def slack(total, ch):
        return _Slack(total * ch, ch * frames_bound, torch.float32, float(SENTINEL), dev)

    # ---- the good chain, every stage's output kept
    lm = slack(n_mel, 80)
    frontend_launch(good, lm)
    want_lm = eng.frontend_ragged().logmel_ragged(eng.ragged(clips)).cpu().numpy().reshape(-1)
    assert _same_bytes(lm.host(), want_lm) and lm.margins_untouched(float(SENTINEL))
    acts = [lm]
    for k in range(5):
        outs = [slack(n_enc, CH_OUT[k])] + ([slack(n_enc, 1)] if k == 4 else [])
        stage_launch(k, good, acts[k], outs)
        assert all(o.margins_untouched(float(SENTINEL)) for o in outs)
        acts.append(outs[0] if k < 4 else outs)
    w0, w1, _ = eng.run_ragged(eng.ragged(clips))
    assert _same_bytes(acts[5][0].host(), w0.cpu().numpy()) and _same_bytes(acts[5][1].host(), w1.cpu().numpy())
    assert int(eng._flag[0].item()) == 0

    def untouched(first, counts, ch, clip, lo, hi):
        """Mask over a packed [ch][T_b] buffer: frames [lo, hi) of clip `clip`."""
        m = np.zeros(int(first[-1]) * ch, dtype=bool)
        T, hi = int(counts[clip]), min(hi, int(counts[clip]))
        for c in range(ch):
            m[ch * int(first[clip]) + c * T + lo:ch * int(first[clip]) + c * T + hi] = True
        return m

    def check(got, want, mask, what):
        got, want = got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
        assert mask.any() and not mask.all(), what
        assert (got[mask] == SENTINEL.view(np.uint32)).all(), what            # the bad entry's own rows: never written
        assert np.array_equal(got[~mask], want[~mask]), what                  # everyone else: what the good tables give

    def lying(kind, first_key, clip_key, tile, counts):
        """(bad tables, clips whose frame range stays unwritten as {clip: (lo, hi)})"""
        h = {k: v.copy() for k, v in good.items()}
        if kind == "clip B":                        # the second tile of clip 1 names clip B
            g = int(h[first_key][1]) + 1
            h[clip_key][g] = B
            return h, {1: (tile, 2 * tile)}
        if kind == "tile beyond its clip":          # ... names clip 2, which has one tile
            g = int(h[first_key][1]) + 1
            h[clip_key][g] = 2
            return h, {1: (tile, 2 * tile)}
        if kind == "negative clip":
            h[clip_key][0] = -1
            return h, {0: (0, tile)}
        return None

    for kind in ("clip B", "tile beyond its clip", "negative clip"):
        h, hit = lying(kind, "fe_tile_first", "fe_tile_clip", 64, F)
        out = slack(n_mel, 80)
        frontend_launch(h, out)
        mask = np.zeros(n_mel * 80, dtype=bool)
        for b, (lo, hi) in hit.items():                                       # time-major rows
            mask[(int(rf.mel_first_host[b]) + lo) * 80:(int(rf.mel_first_host[b]) + min(hi, int(F[b]))) * 80] = True
        check(out.host(), lm.host(), mask, ("frontend", kind))
        assert out.margins_untouched(float(SENTINEL))
        for k in range(5):
            h, hit = lying(kind, "enc_tile_first", "enc_tile_clip", 32, T1)
            outs = [slack(n_enc, CH_OUT[k])] + ([slack(n_enc, 1)] if k == 4 else [])
            stage_launch(k, h, acts[k], outs)
            wants = [acts[k + 1]] if k < 4 else acts[5]
            for o, wv in zip(outs, wants):
                mask = np.zeros(n_enc * CH_OUT[k], dtype=bool)
                for b, (lo, hi) in hit.items():
                    mask |= untouched(rf.enc_first_host, T1, CH_OUT[k], b, lo, hi)
                check(o.host(), wv.host(), mask, (k, kind))
                assert o.margins_untouched(float(SENTINEL))

    # a decreasing prefix entry: entry 2 drops below entry 1, so clip 1 has a negative length and clip 2 a length its tiles deny
    h = {k: v.copy() for k, v in good.items()}
    h["mel_first"][2] = h["mel_first"][1] - 1
    out = slack(n_mel, 80)
    frontend_launch(h, out)
    mask = np.zeros(n_mel * 80, dtype=bool)
    mask[int(rf.mel_first_host[1]) * 80:int(rf.mel_first_host[3]) * 80] = True
    check(out.host(), lm.host(), mask, "frontend, decreasing prefix")
    assert out.margins_untouched(float(SENTINEL))
    for key in ("enc_first", "mel_first"):
        for k in range(5 if key == "enc_first" else 1):                       # (mel_first is the prologue's source table)
            h = {kk: v.copy() for kk, v in good.items()}
            h[key][2] = h[key][1] - 1
            outs = [slack(n_enc, CH_OUT[k])] + ([slack(n_enc, 1)] if k == 4 else [])
            stage_launch(k, h, acts[k], outs)
            wants = [acts[k + 1]] if k < 4 else acts[5]
            for o, wv in zip(outs, wants):
                mask = untouched(rf.enc_first_host, T1, CH_OUT[k], 1, 0, int(T1[1])) | untouched(rf.enc_first_host, T1, CH_OUT[k], 2, 0, int(T1[2]))
                check(o.host(), wv.host(), mask, (k, key, "decreasing prefix"))
                assert o.margins_untouched(float(SENTINEL))
    assert int(eng._flag[0].item()) == 0
