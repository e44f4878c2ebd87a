"""Times of the long-window FireRed path (FireRedEngine(..., long_windows=True)) on the GPU, beside the default engine.

    python tools/time_firered_long.py [--out profiles/firered_long.json] [--clips 4096] [--repeats 20]

One process, fp16 x 2 ("h2"), every clip resident on the device before the clock starts:
  (a) `--clips` clips of 10 s at L = 16 000 on the default engine against the long engine: identical work (10 windows of 98 frames per clip)
      and bitwise-equal probabilities -- the price of keeping the activations in global memory and of R + 1 launches instead of one;
  (b) the same audio as ONE window of 998 frames per clip on the long engine, beside (a)'s default engine.  ANOTHER export (two window
      edges per clip instead of twenty): the times stand side by side, the probabilities are not compared;
  (c) 1024 clips of 1 - 10 s on a dynamic engine (`run_packed`: one snip-edge front-end launch, R + 1 net launches) against one rectangular
      long call per distinct length on the same clips;
  (d) one window of 3600 s (359 998 frames).
A call is the front-end, the net launches and the range-flag read, and ends in a device synchronise.  Per variant: warm-up, then `--repeats`
timed calls, the variants of one row alternating call by call (ABAB); reported are the median and the range of the host clock in ms.
Nothing is gated on these numbers."""
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
from vadx import _lib, firered, ragged, weights  # noqa: E402


def bursts(g, rows, n, dev):
    """int16 bursts generated on the device: N(0, 3000) with every third half second silent"""
    x = (torch.randn((rows, n), generator=g, device=dev) * 3000).clamp_(-32768, 32767).to(torch.int16)
    x *= (torch.arange(n, device=dev) // 8000 % 3 != 0).to(torch.int16)[None, :]
    return x


def time_variants(variants, repeats, warmup=2):
    """{name: fn} -> {name: dict(median_ms, min_ms, max_ms, calls)}; the variants alternate call by call"""
    for _ in range(warmup):
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
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), calls=len(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/firered_long.json")
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    prev = _lib.gemm_mode("h2")
    w = weights.firered_synthetic(1234)
    g = torch.Generator(device=dev).manual_seed(a.seed)
    B, N = a.clips, 160000
    rows = {}

    short = firered.FireRedEngine(w, 16000, device=dev)
    same = firered.FireRedEngine(w, 16000, device=dev, long_windows=True)
    x = bursts(g, B, N, dev)
    res = time_variants({"default": lambda: short.run(x, 10), "long": lambda: same.run(x, 10)}, a.repeats)
    rows["a_same_work"] = dict(clips=B, input_audio_length=16000, windows_per_clip=10, frames_per_window=short.T,
                               bitwise_equal=bool(torch.equal(short.run(x, 10), same.run(x, 10))), default=res["default"], long=res["long"],
                               long_over_default=res["long"]["median_ms"] / res["default"]["median_ms"],
                               workspace_bytes=same.workspace_bytes(B * 10 * short.T))
    print(json.dumps({"a_same_work": rows["a_same_work"]}), flush=True)
    same.release_workspace()
    one = firered.FireRedEngine(w, N, device=dev, long_windows=True)
    res = time_variants({"windows_of_1s": lambda: short.run(x, 10), "one_window": lambda: one.run(x, 1)}, a.repeats)
    rows["b_ten_seconds"] = dict(clips=B, audio_seconds=B * N / 16000.0, windows_of_1s=dict(res["windows_of_1s"], frames_per_clip=10 * short.T),
                                 one_window=dict(res["one_window"], frames_per_clip=one.T),
                                 one_window_over_windows_of_1s=res["one_window"]["median_ms"] / res["windows_of_1s"]["median_ms"],
                                 note="different exports: times side by side, probabilities not compared")
    print(json.dumps({"b_ten_seconds": rows["b_ten_seconds"]}), flush=True)
    fallbacks = short.blobs.range_fallbacks + same.blobs.range_fallbacks + one.blobs.range_fallbacks
    del x, one, same, short
    torch.cuda.empty_cache()

    # (c) 1024 clips of 1 - 10 s: ten distinct lengths, dynamic against one rectangular long call per length
    rng = np.random.default_rng(a.seed)
    lens = rng.choice(np.arange(1, 11) * 16000, size=1024)
    groups = {int(n): bursts(g, int((lens == n).sum()), int(n), dev) for n in sorted(set(lens.tolist()))}
    pcm = torch.cat([groups[int(n)].reshape(-1) for n in sorted(groups)])
    sorted_lens = np.concatenate([np.full(groups[n].shape[0], n, dtype=np.int64) for n in sorted(groups)])
    offs = np.concatenate([[0], np.cumsum(sorted_lens)[:-1]])
    dyn = firered.FireRedEngine(w, None, device=dev, long_windows=True)
    pc = ragged.PackedClips.from_packed(pcm, offs, sorted_lens)
    rect = {n: firered.FireRedEngine(w, n, device=dev, long_windows=True) for n in groups}
    res = time_variants({"dynamic": lambda: dyn.run_packed(pc), "per_length": lambda: [rect[n].run(groups[n], 1) for n in groups]}, a.repeats)
    rows["c_mixed_lengths"] = dict(clips=1024, distinct_lengths=len(groups), frames_total=pc.n_frames, dynamic=res["dynamic"],
                                   per_length=res["per_length"], dynamic_over_per_length=res["dynamic"]["median_ms"] / res["per_length"]["median_ms"])
    print(json.dumps({"c_mixed_lengths": rows["c_mixed_lengths"]}), flush=True)
    fallbacks += dyn.blobs.range_fallbacks + sum(e.blobs.range_fallbacks for e in rect.values())
    del rect, groups, pcm, pc
    torch.cuda.empty_cache()

    # (d) one window of 3600 s
    hour = bursts(g, 1, 3600 * 16000, dev).reshape(-1)
    pc = ragged.PackedClips.from_packed(hour, np.array([0]), np.array([hour.numel()]))
    res = time_variants({"run_packed": lambda: dyn.run_packed(pc)}, a.repeats)["run_packed"]
    rows["d_one_hour"] = dict(frames=pc.n_frames, audio_seconds=3600.0, run_packed=res, fraction_of_audio=res["median_ms"] / 1e3 / 3600.0)
    print(json.dumps({"d_one_hour": rows["d_one_hour"]}), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), mode=dyn.blobs.mode(), range_fallbacks=fallbacks + dyn.blobs.range_fallbacks,
               repeats=a.repeats, seed=a.seed,
               note="ms per call: median and range of `repeats` synchronised calls after warm-up (host clock), the variants of one row "
                    "alternating call by call; every clip is resident on the device before the clock starts; a call = front-end, net "
                    "launches, range-flag read",
               rows=rows)
    _lib.gemm_mode(prev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
