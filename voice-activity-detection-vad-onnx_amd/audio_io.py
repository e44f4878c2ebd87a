"""Audio ingest with the arithmetic of the reference drivers' pydub call chain
`AudioSegment.from_file(p).set_channels(1).set_frame_rate(16000).get_array_of_samples()`
(e.g. FSMN/Inference_FSMN_VAD_ONNX.py:68): pydub delegates to the stdlib `audioop`
(`tomono` with 0.5/0.5, then `ratecv`), which is what this does for PCM wav files.

`audioop` left the standard library in Python 3.13: when it cannot be imported the same integer arithmetic runs in numpy
(`_tomono`, `_ratecv`: the closed form of ratecv's phase walk that csrc/ingest.hip uses on the device; bit-identical to
audioop on 16-bit PCM, tests/test_cabi_cpu.py).  Only PCM wav is read -- the reference's pydub path hands anything
ffmpeg can decode to the same two calls; decode such files to wav first."""
from __future__ import annotations

import math
import wave

import numpy as np

try:
    import audioop as _audioop
except ImportError:              # Python >= 3.13
    _audioop = None


def _lin2lin16(data, width):
    """bytes of `width`-byte little-endian PCM -> int16 numpy (audioop.lin2lin(data, width, 2): keep the top 16 bits;
    8-bit wav is unsigned in the file but audioop treats the bytes as signed, like pydub's chain does after its own bias)."""
    if width == 2:
        return np.frombuffer(data, dtype="<i2").astype(np.int16)
    if width == 1:
        return (np.frombuffer(data, dtype=np.int8).astype(np.int16) << 8).astype(np.int16)
    if width == 4:
        return (np.frombuffer(data, dtype="<i4") >> 16).astype(np.int16)
    if width == 3:
        b = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3)
        return (b[:, 1].astype(np.int16) | (b[:, 2].astype(np.int8).astype(np.int16) << 8)).astype(np.int16)
    raise ValueError(f"unsupported sample width {width}")


def _tomono(x):
    """interleaved stereo int16 -> mono: floor(L * 0.5 + R * 0.5) (audioop.tomono(data, 2, 0.5, 0.5))"""
    v = x.astype(np.int64).reshape(-1, 2)
    return ((v[:, 0] + v[:, 1]) >> 1).astype(np.int16)


def _ratecv(x, in_rate, out_rate):
    """audioop.ratecv(data, 2, 1, in_rate, out_rate, None)[0] in closed form: output e uses m = ceil(e*I/O) + 1 consumed
    frames, phase d = (m-1)*O - e*I, out = floor((x[m-2]*d + x[m-1]*(O-d)) / O) with x[-1] = 0 (rates reduced by their gcd)."""
    g = math.gcd(int(in_rate), int(out_rate))
    I, O = int(in_rate) // g, int(out_rate) // g
    n = x.shape[0]
    if n == 0:
        return x.astype(np.int16)
    n_out = (n - 1) * O // I + 1
    e = np.arange(n_out, dtype=np.int64)
    m = (e * I + O - 1) // O + 1
    d = (m - 1) * O - e * I
    xp = np.concatenate(([0], x.astype(np.int64)))           # xp[k + 1] = x[k], xp[0] = the zero before the first frame
    prev, cur = xp[m - 1], xp[m]
    return np.floor_divide(prev * d + cur * (O - d), O).astype(np.int16)


def load_wav(path, sample_rate=16000, channels=1):
    """-> int16 numpy [n] (mono) at `sample_rate`."""
    with wave.open(path, "rb") as w:
        nch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        data = w.readframes(n)
    if _audioop is not None:
        if width != 2:
            data = _audioop.lin2lin(data, width, 2)
        if channels == 1 and nch == 2:
            data = _audioop.tomono(data, 2, 0.5, 0.5)
            nch = 1
        elif nch != channels:
            raise ValueError(f"unsupported channel conversion {nch} -> {channels}")
        if rate != sample_rate:
            data, _ = _audioop.ratecv(data, 2, nch, rate, sample_rate, None)
        return np.frombuffer(data, dtype=np.int16).copy()
    x = _lin2lin16(data, width)
    if channels == 1 and nch == 2:
        x = _tomono(x)
    elif nch != channels:
        raise ValueError(f"unsupported channel conversion {nch} -> {channels}")
    if rate != sample_rate:
        if channels != 1:
            raise ValueError("rate conversion of multi-channel audio needs the stdlib audioop")
        x = _ratecv(x, rate, sample_rate)
    return np.ascontiguousarray(x, dtype=np.int16)


def save_wav(path, samples, sample_rate=16000):
    """int16 mono samples [n] -> a 16-bit PCM wav file (what `load_wav` reads back bit for bit at the same rate)."""
    x = np.asarray(samples)
    if x.dtype != np.int16 or x.ndim != 1:
        raise ValueError(f"save_wav takes int16 [n] samples, got {x.dtype} {x.shape}")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sample_rate))
        w.writeframes(np.ascontiguousarray(x).astype("<i2").tobytes())


def read_wav_raw(path):
    """-> (int16 numpy [frames * channels] interleaved, channels, rate) without any conversion (16-bit PCM only)."""
    with wave.open(path, "rb") as w:
        nch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        data = w.readframes(n)
    return _lin2lin16(data, width).copy(), nch, rate


INGEST_TILE = 1024        # output samples per workgroup of vadx_ingest_pcm16_ragged
INGEST_ALIGN = 8          # every clip of ingest_ragged's output starts on a 16-byte boundary


def _ragged_plan(raws, channels, rates, sample_rate):
    """Checks and layout shared by `ingest_ragged` and its host mirror: -> (raws as int16 vectors, channels, rates, frames, out frames,
    where each clip starts in the packed output, its length).  Refuses what vadx_ingest_pcm16 refuses, per clip."""
    raws = [np.ascontiguousarray(r, dtype=np.int16).reshape(-1) for r in raws]
    B = len(raws)
    if B == 0:
        raise ValueError("a ragged batch needs at least one clip")
    channels = [int(channels)] * B if np.isscalar(channels) else [int(c) for c in channels]
    rates = [int(rates)] * B if np.isscalar(rates) else [int(r) for r in rates]
    if len(channels) != B or len(rates) != B:
        raise ValueError(f"{B} clips, {len(channels)} channel counts, {len(rates)} rates")
    frames, outs = [], []
    for b, (r, c, rate) in enumerate(zip(raws, channels, rates)):
        if c not in (1, 2):
            raise ValueError(f"clip {b}: 1 or 2 interleaved channels (got {c})")
        if rate <= 0 or sample_rate <= 0:
            raise ValueError(f"clip {b}: rates must be positive")
        if r.shape[0] == 0 or r.shape[0] % c:
            raise ValueError(f"clip {b}: {r.shape[0]} samples are not a positive whole number of {c}-channel frames")
        g = math.gcd(rate, int(sample_rate))
        if int(sample_rate) // g >= 65536 or r.shape[0] // c >= 2 ** 31:
            raise ValueError(f"clip {b}: reduced rates {rate // g} -> {int(sample_rate) // g} or {r.shape[0] // c} frames out of range")
        frames.append(r.shape[0] // c)
        outs.append((frames[-1] - 1) * (int(sample_rate) // g) // (rate // g) + 1)
    outs = np.asarray(outs, dtype=np.int64)
    room = (outs + INGEST_ALIGN - 1) // INGEST_ALIGN * INGEST_ALIGN
    return raws, channels, rates, np.asarray(frames, dtype=np.int64), np.concatenate([[0], np.cumsum(room)[:-1]]).astype(np.int64), outs


def ingest_ragged_host(raws, channels, rates, sample_rate=16000):
    """The host mirror of `ingest_ragged`: (pcm int16 numpy, clip_offsets, lengths) with the closed form csrc/prepare.hip evaluates per
    output sample (`_tomono`, `_ratecv`: audioop's arithmetic); the gaps that align the clips are zeros."""
    raws, channels, rates, _, offs, outs = _ragged_plan(raws, channels, rates, sample_rate)
    pcm = np.zeros(int(offs[-1] + (outs[-1] + INGEST_ALIGN - 1) // INGEST_ALIGN * INGEST_ALIGN), dtype=np.int16)
    for r, c, rate, o, n in zip(raws, channels, rates, offs, outs):
        x = _tomono(r) if c == 2 else r
        pcm[o:o + n] = _ratecv(x, rate, sample_rate)
    return pcm, offs, outs


def ingest_ragged(raws, channels, rates, sample_rate=16000, device="cuda:0", return_status=False):
    """Raw clips of ANY lengths, channel counts (1 or 2) and rates -> (pcm, clip_offsets, lengths): device int16 [total] mono at
    `sample_rate` with audioop's tomono + ratecv arithmetic (vadx_ingest_pcm16_ragged, one launch), clip b = lengths[b] samples from
    element clip_offsets[b] (host int64 arrays; every clip starts on a 16-byte boundary, the gaps are zeros) -- what
    `RaggedBatch.from_packed` takes.  raws: interleaved int16 vectors as `read_wav_raw` returns them; the upload is the file bytes, once.
    return_status: also the kernel's per-clip status words (device int32 [B], VADX_INGEST_ST_* bits; all zero for what this accepted)."""
    from . import _lib
    t = _lib.require_gpu()
    raws, channels, rates, frames, offs, outs = _ragged_plan(raws, channels, rates, sample_rate)
    B = len(raws)
    src_off = np.concatenate([[0], np.cumsum([r.shape[0] for r in raws])[:-1]]).astype(np.int64)
    per = np.maximum((outs + INGEST_TILE - 1) // INGEST_TILE, 1)
    tiles = int(per.sum())
    if tiles >= 2 ** 31:
        raise ValueError(f"{tiles} tiles of {INGEST_TILE} samples do not fit the int32 tile tables")
    total = int(offs[-1] + (outs[-1] + INGEST_ALIGN - 1) // INGEST_ALIGN * INGEST_ALIGN)
    src = t.from_numpy(np.concatenate(raws)).to(device)
    i64 = t.from_numpy(np.concatenate([src_off, frames, offs])).to(device)
    i32 = t.from_numpy(np.concatenate([np.asarray(channels), np.asarray(rates), np.concatenate([[0], np.cumsum(per)]),
                                       np.repeat(np.arange(B), per)]).astype(np.int32)).to(device)
    out = t.zeros(total, dtype=t.int16, device=src.device)
    status = t.zeros(B, dtype=t.int32, device=src.device)
    p64, p32 = i64.data_ptr(), i32.data_ptr()
    with t.cuda.device(src.device):
        _lib.check(_lib.lib().vadx_ingest_pcm16_ragged(src.data_ptr(), int(src.numel()), p64, p64 + 8 * B, p32, p32 + 4 * B, int(sample_rate),
                                                       p64 + 16 * B, p32 + 8 * B, p32 + 4 * (3 * B + 1), B, tiles, out.data_ptr(), total,
                                                       status.data_ptr(), _lib.stream_ptr()))
    return (out, offs, outs, status) if return_status else (out, offs, outs)


def ingest_device(raw_i16, channels, rate, sample_rate=16000, device="cuda:0"):
    """Batch of equal-length raw clips int16 [B, frames * channels] (interleaved) -> device int16 [B, n] mono at
    `sample_rate`, with audioop's tomono + ratecv arithmetic on the GPU (vadx_ingest_pcm16): the upload is the raw
    file bytes and the down-mix / resampling never touches the host."""
    from . import _lib
    t = _lib.require_gpu()
    x = raw_i16 if t.is_tensor(raw_i16) else t.from_numpy(np.ascontiguousarray(raw_i16, dtype=np.int16))
    if x.dim() == 1:
        x = x.unsqueeze(0)
    x = x.to(device).contiguous()
    B, n = x.shape
    if n % channels:
        raise ValueError("row length is not a whole number of frames")
    frames = n // channels
    L = _lib.lib()
    nout = L.vadx_ingest_out_frames(frames, int(rate), int(sample_rate))
    out = t.empty((B, nout), dtype=t.int16, device=x.device)
    with t.cuda.device(x.device):
        _lib.check(L.vadx_ingest_pcm16(x.data_ptr(), _lib.row_stride(x), int(channels), frames, int(rate), int(sample_rate),
                                       out.data_ptr(), _lib.row_stride(out), B, _lib.stream_ptr()))
    return out
