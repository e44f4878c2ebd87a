"""Times of vadx.prepare (a ragged batch normalised, padded and packed on the device) and of the ragged ingest before it, on the GPU.

    python tools/time_prepare.py [--out profiles/prepare.json] [--repeats 20] [--host-clips 256]

One process; the audio is resident before a clock starts.  Workloads: `ragged_1024x1_10s` = 1024 clips with lengths uniform in 1 - 10 s,
`rect_4096x10s` = 4096 clips of 10 s; FSMN's grid (16000 every 11040) and peak normalisation, pad noise as a resident device matrix.
Per workload, each the median (and range) of `--repeats` synchronised calls after two warm-up calls, on the same audio:
  from_packed   RaggedBatch.from_packed on the resident packed vector (host clock, ending in a synchronise);
  from_clips    RaggedBatch.from_clips of the same clips from host memory -- the per-clip host loop plus the upload (host clock), on the
                first `--host-clips` clips; `scaled_ms` is that time times B / host-clips, an estimate, not a measurement;
  stats / scale / write   each launch alone (device events); `write` with bytes read + written / time;
  memcpy        dst.copy_ of as many bytes as the write kernel writes, the ceiling (device events);
  ingest_ragged audio_io.ingest_ragged of `--host-clips` of the clips as 48 kHz stereo raw frames (host clock: the concatenation, the
                upload and one launch), and
  load_wav_loop the host's tomono + ratecv per clip on the same frames; both scaled the same way."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vadx  # noqa: F401,E402
from vadx import _lib, audio_io, prepare, ragged, timestamps  # noqa: E402
from vadx.clips import pad_count  # noqa: E402

DEV = torch.device("cuda:0")
WINDOW, STRIDE = 16000, 11040


def stats(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), calls=len(v))


def by_events(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return stats(ms)


def by_host(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def workload(name, lengths, repeats, host_clips):
    B = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum((lengths + 7) // 8 * 8)]).astype(np.int64)
    src = torch.randint(-20000, 20000, (int(starts[-1]),), dtype=torch.int16, device=DEV)
    starts = starts[:-1]
    pads = np.asarray([pad_count(int(n), WINDOW, STRIDE) for n in lengths], dtype=np.int64)
    noise = torch.randn((B, int(pads.max()) + 1), dtype=torch.float64, device=DEV)
    total = int((lengths + pads).sum())
    row = dict(clips=B, audio_seconds=float(lengths.sum() / 16000), src_bytes=2 * int(src.numel()), out_bytes=2 * total)
    out = torch.empty(total, dtype=torch.int16, device=DEV)
    row["from_packed"] = by_host(lambda: ragged.RaggedBatch.from_packed(src, starts, lengths, WINDOW, STRIDE, noise, "peak", out=out), repeats)
    # the three launches, each alone, on the tables from_packed builds
    L = _lib.lib()
    tile_first, tile_clip = prepare.chunk_tables(lengths)
    tiles = int(tile_first[-1])
    dst_off = np.concatenate([[0], np.cumsum(lengths + pads)]).astype(np.int64)
    noise_off = np.arange(B, dtype=np.int64) * noise.shape[1]
    i64 = torch.from_numpy(np.concatenate([starts, lengths, dst_off, noise_off])).to(DEV)
    i32 = torch.from_numpy(np.concatenate([tile_first, tile_clip])).to(DEV)
    p = [i64.data_ptr() + 8 * k for k in (0, B, 2 * B, 3 * B + 1)]
    ws = torch.empty(L.vadx_prepare_workspace_bytes(B, tiles), dtype=torch.uint8, device=DEV)
    a = (src.data_ptr(), int(src.numel()), p[0], p[1])
    s = _lib.stream_ptr
    row["stats"] = by_events(lambda: _lib.check(L.vadx_prepare_stats(*a, i32.data_ptr(), i32.data_ptr() + 4 * (B + 1), B, tiles, 1, ws.data_ptr(),
                                                                     ws.numel(), s())), repeats)
    row["scale"] = by_events(lambda: _lib.check(L.vadx_prepare_scale(*a, p[2], i32.data_ptr(), B, tiles, WINDOW, STRIDE, 1, 8192.0, ws.data_ptr(),
                                                                     ws.numel(), s())), repeats)
    row["write"] = by_events(lambda: _lib.check(L.vadx_prepare_write(*a, p[2], noise.data_ptr(), int(noise.numel()), p[3], B, tiles, 1, ws.data_ptr(),
                                                                     ws.numel(), out.data_ptr(), total, s())), repeats)
    moved = 2 * int(lengths.sum()) + 2 * total
    row["write"]["tb_per_s"] = moved / (row["write"]["median_ms"] * 1e-3) / 1e12
    big = torch.empty(total, dtype=torch.int16, device=DEV)
    row["memcpy"] = by_events(lambda: out.copy_(big), repeats)
    row["memcpy"]["tb_per_s"] = 4 * total / (row["memcpy"]["median_ms"] * 1e-3) / 1e12
    row["write_over_memcpy"] = row["write"]["median_ms"] / row["memcpy"]["median_ms"]
    # the host loop + upload, on the same audio
    sub = min(B, host_clips)
    host = src.cpu().numpy()
    clips = [host[starts[b]:starts[b] + lengths[b]] for b in range(sub)]
    zrows = noise[:sub].cpu().numpy()
    prep = lambda c: timestamps.normalize_to_int16(c.astype(np.float32))      # noqa: E731
    row["from_clips"] = by_host(lambda: ragged.RaggedBatch.from_clips(clips, WINDOW, STRIDE, zrows, prep, DEV), max(3, repeats // 4), warmup=1)
    row["from_clips"].update(clips_timed=sub, scaled_ms=row["from_clips"]["median_ms"] * B / sub)
    ref = ragged.RaggedBatch.from_clips(clips, WINDOW, STRIDE, zrows, prep, DEV)
    got = ragged.RaggedBatch.from_packed(src, starts[:sub], lengths[:sub], WINDOW, STRIDE, noise[:sub], "peak")
    row["equal_to_from_clips"] = bool(torch.equal(ref.pcm, got.pcm))
    # ingest: the same clips as 48 kHz stereo raw frames
    rng = np.random.default_rng(1)
    raws = [rng.integers(-20000, 20000, 2 * 3 * int(n)).astype(np.int16) for n in lengths[:sub]]
    row["ingest_ragged"] = by_host(lambda: audio_io.ingest_ragged(raws, 2, 48000, 16000, DEV), max(3, repeats // 4), warmup=1)
    row["ingest_ragged"].update(clips_timed=sub, scaled_ms=row["ingest_ragged"]["median_ms"] * B / sub)

    def load_loop():
        return [audio_io._ratecv(audio_io._tomono(r), 48000, 16000) for r in raws]
    row["load_wav_loop"] = by_host(load_loop, max(3, repeats // 4), warmup=1)
    row["load_wav_loop"].update(clips_timed=sub, scaled_ms=row["load_wav_loop"]["median_ms"] * B / sub)
    print(json.dumps({name: row}), flush=True)
    del src, out, big, noise
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/prepare.json")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-clips", type=int, default=256)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    rows = {"ragged_1024x1_10s": workload("ragged_1024x1_10s", rng.integers(16000, 160001, 1024), a.repeats, a.host_clips),
            "rect_4096x10s": workload("rect_4096x10s", np.full(4096, 160000), a.repeats, a.host_clips)}
    out = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, seed=a.seed, grid=[WINDOW, STRIDE], normalize="peak",
               note="int16, resident data; stats / scale / write / memcpy: device events around one launch; from_packed / from_clips / ingest_ragged / "
                    "load_wav_loop: host clock, ending in a synchronise; medians and ranges of `repeats` calls (a quarter of them for the host "
                    "loops) after warm-ups; from_clips, ingest_ragged and load_wav_loop run on `clips_timed` clips and scaled_ms multiplies by B / clips_timed "
                    "(an estimate); tb_per_s = (bytes read + bytes written) / median time",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
