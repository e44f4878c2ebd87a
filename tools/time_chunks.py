"""Times of vadx.chunks (the batched collect_chunks / drop_chunks: vadx_chunks_plan + vadx_chunks_copy) on the GPU.

    python tools/time_chunks.py [--out profiles/chunks.json] [--repeats 20] [--skip-silero]

One process, everything resident on the device before a clock starts (the int16 audio is drawn there; the segment table and the clip
lengths are uploaded once).  Workloads: `rect` = 4096 clips of 10 s as a [B, N] rectangle, `ragged` = 1024 clips with lengths uniform in
1 - 10 s as a packed vector (16-byte clip starts).  Every clip has 1 - 6 random segments that cover about half of it.  Per workload and mode
(collect, drop), each the median (and range) of `--repeats` calls after two warm-up calls:
  plan        vadx_chunks_plan alone (device events around the two launches);
  copy        vadx_chunks_copy alone into a preallocated destination (device events), with bytes read + written / time;
  call        the public call without `out`: plan, the 16-byte read-back, the allocation, the copy, then a synchronise (host clock);
  torch_cat   (a) what a caller can do without this module: per clip, torch.cat of device slices -- on the first 256 clips, synchronised
              once at the end (host clock); `scaled_ms` is that time times B / 256, an estimate, not a measurement;
  memcpy      (b) dst.copy_(src[:total]) of the same number of bytes, the ceiling (device events).
Unless --skip-silero: what get_speech_audio_batch adds to a config-2 step (4096 x 10 s float32 through SileroEngine.clips + segments,
synthetic weights): host clock around get_speech_timestamps_batch and around get_speech_audio_batch, alternating."""
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
from vadx import chunks, silero  # noqa: E402

DEV = torch.device("cuda:0")


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


def tables(rng, lengths):
    """1 - 6 segments per clip: 2k sorted cut points, every other interval is a segment (about half of the clip)"""
    out = []
    for n in lengths:
        k = int(rng.integers(1, 7))
        cuts = np.sort(rng.integers(0, int(n) + 1, 2 * k))
        out.append([(int(cuts[2 * j]), int(cuts[2 * j + 1])) for j in range(k)])
    return out


def workload(name, lengths, rect, rng, repeats):
    B = len(lengths)
    lengths = np.asarray(lengths, dtype=np.int64)
    if rect:
        N = int(lengths.max())
        starts = np.arange(B, dtype=np.int64) * N
        src_elems = B * N
    else:
        starts = np.concatenate([[0], np.cumsum((lengths + 7) // 8 * 8)]).astype(np.int64)
        src_elems, starts = int(starts[-1]), starts[:-1]
    src = torch.randint(-32768, 32768, (src_elems,), dtype=torch.int16, device=DEV)
    tss = tables(rng, lengths)
    segs, counts = (torch.from_numpy(a).to(DEV) for a in chunks.table_of(tss))
    lens_d, starts_d = torch.from_numpy(lengths).to(DEV), torch.from_numpy(starts).to(DEV)
    row = dict(clips=B, audio_seconds=float(lengths.sum() / 16000), src_bytes=2 * src_elems, segments=int(counts.sum().item()), cap=int(segs.shape[1]))
    for mode, fn in (("collect", chunks.collect_chunks_batch), ("drop", chunks.drop_chunks_batch)):
        plan = chunks.ChunkPlan(segs, counts, lens_d, mode, 8)
        total = plan.total
        dst = torch.empty(total, dtype=torch.int16, device=DEV)
        r = dict(total_elems=total, moved_bytes=4 * total)
        r["plan"] = by_events(lambda: chunks.ChunkPlan(segs, counts, lens_d, mode, 8), repeats)
        r["copy"] = by_events(lambda: plan.copy(src, starts_d, dst), repeats)
        r["copy"]["tb_per_s"] = r["moved_bytes"] / (r["copy"]["median_ms"] * 1e-3) / 1e12
        plan.check()
        r["call"] = by_host(lambda: fn((segs, counts), src, lengths=lens_d, clip_offsets=starts_d, align=8), repeats)
        r["memcpy"] = by_events(lambda: dst.copy_(src[:total]), repeats)
        r["memcpy"]["tb_per_s"] = r["moved_bytes"] / (r["memcpy"]["median_ms"] * 1e-3) / 1e12
        r["copy_over_memcpy"] = r["copy"]["median_ms"] / r["memcpy"]["median_ms"]
        sub = min(B, 256)
        host_starts = starts.tolist()

        def cat_loop():
            outs = []
            for b in range(sub):
                wav = src[host_starts[b]:host_starts[b] + int(lengths[b])]
                if mode == "collect":
                    parts = [wav[s:e] for s, e in tss[b]]
                else:
                    cur, parts = 0, []
                    for s, e in tss[b]:
                        parts.append(wav[cur:s])
                        cur = e
                    parts.append(wav[cur:])
                outs.append(torch.cat(parts))
            return outs
        r["torch_cat"] = by_host(cat_loop, max(3, repeats // 4))
        r["torch_cat"].update(clips_timed=sub, scaled_ms=r["torch_cat"]["median_ms"] * B / sub)
        # and the result is the same bytes as that loop's, clip by clip
        packed, off = fn((segs, counts), src, lengths=lens_d, clip_offsets=starts_d, align=8)
        off, n = off.cpu().numpy(), plan.lengths.cpu().numpy()
        r["equal_to_torch_cat"] = all(torch.equal(packed[off[b]:off[b] + n[b]], o) for b, o in enumerate(cat_loop()))
        row[mode] = r
        print(json.dumps({name: {mode: r}}), flush=True)
        del dst, plan, packed
    del src
    torch.cuda.empty_cache()
    return row


def silero_step(repeats):
    model = silero.load_silero_vad(onnx=True, use_cpu=True, path="synthetic:1234", device="cuda:0")
    B, N = 4096, 160000
    audio = torch.randn((B, N), dtype=torch.float32, device=DEV) * 0.05
    audio *= (torch.arange(N, device=DEV) // 12000 % 2).to(torch.float32) * 0.98 + 0.02      # loud / quiet every 0.75 s
    kw = dict(threshold=0.5, min_speech_duration_ms=250, min_silence_duration_ms=100)
    res = {}
    variants = {"timestamps": lambda: silero.get_speech_timestamps_batch(audio, model, **kw),
                "speech_audio": lambda: silero.get_speech_audio_batch(audio, model, **kw)}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: stats(v) for k, v in ms.items()}
    packed, _, ts = silero.get_speech_audio_batch(audio, model, **kw)
    res.update(clips=B, samples=N, segments=sum(len(t) for t in ts), packed_elems=int(packed.numel()),
               added_ms=res["speech_audio"]["median_ms"] - res["timestamps"]["median_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/chunks.json")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--skip-silero", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    rows = {"rect_4096x10s": workload("rect_4096x10s", np.full(4096, 160000), True, rng, a.repeats),
            "ragged_1024x1_10s": workload("ragged_1024x1_10s", rng.integers(16000, 160001, 1024), False, rng, a.repeats)}
    out = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, seed=a.seed,
               note="int16, resident data, align 8; plan / copy / memcpy: device events around the launches, median and range of `repeats` "
                    "synchronised calls after two warm-ups; call / torch_cat: host clock, ending in a synchronise; tb_per_s = (bytes read + "
                    "bytes written) / median time; torch_cat is timed on 256 clips and scaled_ms multiplies by B / 256 (an estimate)",
               rows=rows)
    if not a.skip_silero:
        out["silero_config2_step"] = silero_step(max(3, a.repeats // 4))
        print(json.dumps({"silero_config2_step": out["silero_config2_step"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
