"""Times of the ragged Silero path (get_speech_timestamps_batch on a vadx.ragged.RaggedClips) on the GPU, beside the rectangle.

    python tools/time_silero_ragged.py [--out profiles/silero_ragged.json] [--clips 1024 4096] [--repeats 20]

fp16 x 2 kernels, one process, float32 clips on the +-1 scale, every input resident on the device before the clock starts (host packing, the
tables and the upload are outside every timed region).  Per clip count three settings:
  (a) lengths drawn uniformly from 1 - 10 s (seeded): ragged timestamps against get_speech_timestamps_batch(rectangle, lengths=) -- the
      only batched path before the ragged one -- and, scores alone, clips_ragged against clips() on the rectangle;
  (b) the same lengths rounded up to whole seconds: the same four calls;
  (c) every clip 10 s: clips_ragged against clips() on the same audio -- how far the ragged path is behind where it is not needed.
A call ends in a device synchronise.  Per row: warm-up, then `--repeats` timed calls, the variants of a row alternating call by call (ABAB);
reported are the median and the range (min, max) of the host clock in ms, the window counts both ways, and whether every clip's scores
and timestamps are the same both ways.  Nothing is gated on these numbers; they are recorded with the box they came from."""
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
from vadx import ragged, silero, weights  # noqa: E402


def bursts(rng, n):
    """float32 bursts on the +-1 scale: N(0, 3000) / N(0, 30) int16-level segments of 0.75 s"""
    loud = ((np.arange(n) // 12000 + int(rng.integers(0, 2))) % 2).astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * (30.0 + 2970.0 * loud)
    return np.clip(np.rint(x), -32768, 32767).astype(np.float32) * np.float32(0.000030517578)


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
    ap.add_argument("--out", default="profiles/silero_ragged.json")
    ap.add_argument("--clips", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = silero.SileroEngine(weights.silero_synthetic(1234), device=dev)
    eng.arithmetic = "h2"
    rng = np.random.default_rng(a.seed)
    kw = dict(threshold=0.5, min_speech_duration_ms=250, min_silence_duration_ms=100)

    def row(lengths, name, timestamps):
        clips = [bursts(rng, int(n)) for n in lengths]
        rb = ragged.RaggedClips.from_clips(clips, device=dev)
        rect = torch.zeros((len(clips), int(max(lengths))), dtype=torch.float32, device=dev)
        for b, c in enumerate(clips):
            rect[b, :len(c)] = torch.from_numpy(c)
        lens = [int(n) for n in lengths]
        del clips
        variants = {"scores_ragged": lambda: eng.clips_ragged(rb), "scores_rectangle": lambda: eng.clips(rect)}
        if timestamps:
            variants["timestamps_ragged"] = lambda: silero.get_speech_timestamps_batch(rb, eng, **kw)
            variants["timestamps_rectangle"] = lambda: silero.get_speech_timestamps_batch(rect, eng, lengths=lens, **kw)
        res = time_variants(variants, a.repeats)
        # same results both ways (the rectangle masked per clip, as the lengths= path masks it)
        got, rows_ = silero.get_speech_timestamps_batch(rb, eng, return_probs=True, **kw)
        want, rprobs = silero.get_speech_timestamps_batch(rect, eng, lengths=lens, return_probs=True, **kw)
        same = got == want and all(torch.equal(r, rprobs[b, :r.shape[0]]) for b, r in enumerate(rows_))
        T = int(rb.windows.max())
        out = dict(clips=len(rb), audio_seconds=float(rb.lengths.sum() / 16000), windows_ragged=rb.tiles * 16, windows_rectangle=rb.groups * 16 * T,
                   window_ratio=rb.tiles / (rb.groups * T), workspace_mb_ragged=rb.workspace_bytes / 2 ** 20,
                   workspace_mb_rectangle=rb.groups * T * 32768 / 2 ** 20, same_results=bool(same), **res)
        out["scores_rectangle_over_ragged"] = res["scores_rectangle"]["median_ms"] / res["scores_ragged"]["median_ms"]
        if timestamps:
            out["timestamps_rectangle_over_ragged"] = res["timestamps_rectangle"]["median_ms"] / res["timestamps_ragged"]["median_ms"]
        print(json.dumps({name: out}), flush=True)
        del rb, rect
        torch.cuda.empty_cache()
        return out

    rows = {}
    for B in a.clips:
        lengths = rng.integers(16000, 160001, B)
        rows[f"a_uniform_lengths_{B}"] = row(lengths, f"a_uniform_lengths_{B}", True)
        rows[f"b_whole_seconds_{B}"] = row((lengths + 15999) // 16000 * 16000, f"b_whole_seconds_{B}", True)
        rows[f"c_all_10s_{B}"] = row(np.full(B, 160000), f"c_all_10s_{B}", False)
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.mode(), range_fallbacks=eng.range_fallbacks, repeats=a.repeats, seed=a.seed,
               note="ms per call: median and range of `repeats` synchronised calls after warm-up (host clock), the variants of a row alternating "
                    "call by call; float32 clips resident on the device, tables built before the clock starts; scores_* = clips_ragged / "
                    "clips() (encoder + LSTM + range-flag read), timestamps_* = get_speech_timestamps_batch on the RaggedClips / on the "
                    "rectangle with lengths= (mask, encoder, LSTM, segmenter, host lists)",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
