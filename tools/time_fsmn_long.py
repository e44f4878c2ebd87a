"""Times of the long-window FSMN path (FsmnEngine(..., long_windows=True)) on the GPU, beside the default engine.

    python tools/time_fsmn_long.py [--out profiles/fsmn_long.json] [--clips 4096] [--repeats 20]

Three questions, one process, fp16 x 2 ("h2"), every clip resident on the device before the clock starts:
  (a) `--clips` clips of 10 s: `flags` at L = 16 000 on the default engine (15 windows of 101 frames per clip) against `flags` at
      L = 160 000 on the long engine (ONE window of 1 001 frames per clip), on the same audio.  These are DIFFERENT exports (other DC mean,
      other inv_reference_air_factor, no noise-floor feedback inside a window): the times stand side by side with the frame counts,
      there is no pass / fail and the flags are not compared;
  (b) the same clips at L = 16 000 on the default engine against the long engine: identical work and identical flags -- the price of
      keeping a window's scores in global memory instead of LDS (an opt-in path: recorded, not gated);
  (c) one clip, one window of 9 600 000 samples (10 minutes): vadx_fsmn_window_stats_long against the two-kernel fallback
      (vadx_frontend_window_means + vadx_fsmn_energy) that vadx_fsmn_window_stats takes at that length, and the whole `flags` call as a
      fraction of the audio's duration.
A call is everything the method does (window statistics, log-mel front-end, the clips kernel, the range-flag read) and ends in a device
synchronise.  Per variant: warm-up, then `--repeats` timed calls, the variants of one question alternating call by call (ABAB);
reported are the median and the range (min, max) of the host clock in ms."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vadx  # noqa: F401,E402
from vadx import _lib, fsmn, weights  # noqa: E402


def bursts(rng, n):
    """int16 bursts: N(0, 3000) / N(0, 30) segments of 0.75 s"""
    loud = ((np.arange(n) // 12000 + int(rng.integers(0, 2))) % 2).astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * (30.0 + 2970.0 * loud)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


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
    ap.add_argument("--out", default="profiles/fsmn_long.json")
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    prev = _lib.gemm_mode("h2")
    w = weights.fsmn_synthetic(1234)
    short = fsmn.FsmnEngine(w, device=dev)
    same = fsmn.FsmnEngine(w, device=dev, long_windows=True)
    rng = np.random.default_rng(a.seed)
    B, N = a.clips, 160000
    rows = {}

    # (a) + (b): 10 s clips
    clips = np.stack([bursts(rng, N) for _ in range(B)])
    lb, stride = short.grid()
    padded, W = fsmn.pad_batch(clips, short.L, stride, rng.standard_normal((B, 16000)), None)
    x16 = torch.from_numpy(padded).to(dev)
    res = time_variants({"default": lambda: short.flags(x16, W), "long": lambda: same.flags(x16, W)}, a.repeats)
    rows["b_same_work"] = dict(clips=B, input_audio_length=short.L, windows_per_clip=W, frames_per_window=short.T, frames_per_clip=W * short.T,
                               bitwise_equal=bool(torch.equal(short.flags(x16, W), same.flags(x16, W))), default=res["default"], long=res["long"],
                               long_over_default=res["long"]["median_ms"] / res["default"]["median_ms"])
    print(json.dumps({"b_same_work": rows["b_same_work"]}), flush=True)
    del same
    one = fsmn.FsmnEngine(w, input_audio_length=N, device=dev, long_windows=True)
    x160 = torch.from_numpy(clips).to(dev)
    res = time_variants({"windows_of_1s": lambda: short.flags(x16, W), "one_window": lambda: one.flags(x160, 1)}, a.repeats)
    rows["a_ten_seconds"] = dict(clips=B, audio_seconds=B * N / 16000.0,
                                 windows_of_1s=dict(res["windows_of_1s"], input_audio_length=short.L, windows_per_clip=W, frames_per_clip=W * short.T),
                                 one_window=dict(res["one_window"], input_audio_length=N, windows_per_clip=1, frames_per_clip=one.T),
                                 one_window_over_windows_of_1s=res["one_window"]["median_ms"] / res["windows_of_1s"]["median_ms"],
                                 note="different exports: times side by side, flags not compared")
    print(json.dumps({"a_ten_seconds": rows["a_ten_seconds"]}), flush=True)
    fallbacks = short.blobs.range_fallbacks + one.blobs.range_fallbacks
    del x16, x160, one, short
    torch.cuda.empty_cache()

    # (c): ten minutes as one window
    Lc = fsmn.LONG_MAX_LENGTH
    big = fsmn.FsmnEngine(w, input_audio_length=Lc, device=dev, long_windows=True)
    xc = torch.from_numpy(bursts(rng, Lc)[None, :]).to(dev)
    means = torch.empty(1, dtype=torch.float32, device=dev)
    db = torch.empty((1, big.T), dtype=torch.float32, device=dev)
    sums = torch.empty(1, dtype=torch.int64, device=dev)
    Lb, st = _lib.lib(), _lib.stream_ptr()

    def stats_long():
        _lib.check(Lb.vadx_fsmn_window_stats_long(xc.data_ptr(), Lc, Lc, 1, 1, Lc, big.T, means.data_ptr(), db.data_ptr(), sums.data_ptr(), st))

    def stats_fallback():
        _lib.check(Lb.vadx_frontend_window_means(xc.data_ptr(), Lc, Lc, 1, 1, Lc, C.c_float(1.0), means.data_ptr(), st))
        _lib.check(Lb.vadx_fsmn_energy(xc.data_ptr(), Lc, Lc, 1, 1, Lc, big.T, means.data_ptr(), db.data_ptr(), st))

    res = time_variants({"long": stats_long, "fallback": stats_fallback}, a.repeats)
    whole = time_variants({"flags": lambda: big.flags(xc, 1)}, a.repeats)["flags"]
    rows["c_ten_minutes"] = dict(input_audio_length=Lc, frames=big.T, audio_seconds=Lc / 16000.0, stats_long=res["long"], stats_fallback=res["fallback"],
                                 fallback_over_long=res["fallback"]["median_ms"] / res["long"]["median_ms"], flags=whole,
                                 flags_fraction_of_audio=whole["median_ms"] / 1e3 / (Lc / 16000.0))
    print(json.dumps({"c_ten_minutes": rows["c_ten_minutes"]}), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), mode=big.blobs.mode(), range_fallbacks=fallbacks + big.blobs.range_fallbacks, look_backward=lb,
               repeats=a.repeats, seed=a.seed,
               note="ms per call: median and range of `repeats` synchronised calls after warm-up (host clock), the variants of one row "
                    "alternating call by call; every clip is resident on the device before the clock starts; a call = FsmnEngine.flags "
                    "(window statistics, front-end, clips kernel, range-flag read)",
               rows=rows)
    _lib.gemm_mode(prev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
