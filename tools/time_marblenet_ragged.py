"""Times of the ragged MarbleNet path (MarbleNetEngine.run_ragged over a vadx.ragged.RaggedFrames) on the GPU, beside MarbleNetEngine.run.

    python tools/time_marblenet_ragged.py [--out profiles/marblenet_ragged.json] [--clips 1024] [--repeats 20]

Dynamic-axis mode (one window = one whole clip), one process, every clip resident on the device before the clock starts (host packing
and the upload are outside every timed region):
  (a) `--clips` clips with lengths drawn uniformly from 1 - 10 s (seeded): one run_ragged call against one run() call per distinct
      length, which is what drivers._grouped did with a list of files (every front-end blob built and cached before the clock starts);
  (b) the same lengths rounded up to whole seconds: run_ragged against ten rectangular run() calls, the grouped way's best case;
  (c) `--clips` clips of 10 s each: run_ragged against ONE run() call on the same audio -- the price of the tables where they are not needed.
A call is everything the method does (log-mel front-end, the five encoder launches, on "h2" the range-flag read) and ends in a device
synchronise.  Per row: warm-up, then `--repeats` timed calls, the two variants alternating call by call; reported are the median and the
range (min, max) of the host clock in ms, and whether every clip's scores are the same bytes both ways."""
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
from vadx import marblenet, weights  # noqa: E402


def bursts(rng, n):
    """int16 bursts: N(0, 3000) / N(0, 30) segments of 0.75 s"""
    loud = ((np.arange(n) // 12000 + int(rng.integers(0, 2))) % 2).astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * (30.0 + 2970.0 * loud)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def grouped(eng, clips):
    """One rectangular batch per distinct length: (device int16 [G, n], clip indices)"""
    by_len = {}
    for b, c in enumerate(clips):
        by_len.setdefault(len(c), []).append(b)
    return [(torch.from_numpy(np.stack([clips[b] for b in idx])).to(eng.device), idx) for idx in by_len.values()]


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


def same_scores(eng, rf, groups):
    s0, s1, first = eng.run_ragged(rf)
    for a, idx in groups:
        r0, r1, _ = eng.run(a)
        for j, b in enumerate(idx):
            if not (torch.equal(s0[first[b]:first[b + 1]], r0[j]) and torch.equal(s1[first[b]:first[b + 1]], r1[j])):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/marblenet_ragged.json")
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = marblenet.MarbleNetEngine(weights.marblenet_synthetic(1234), device=dev)
    rng = np.random.default_rng(a.seed)
    B = a.clips

    def row(lengths, name):
        clips = [bursts(rng, int(n)) for n in lengths]
        rf, groups = eng.ragged(clips), grouped(eng, clips)
        res = time_variants({"ragged": lambda: eng.run_ragged(rf), "rectangular": lambda: [eng.run(x) for x, _ in groups]}, a.repeats)
        out = dict(clips=len(rf), distinct_lengths=len(groups), rectangular_calls=len(groups), mel_frames=rf.n_mel, encoder_frames=rf.n_enc,
                   audio_seconds=float(rf.lengths.sum() / 16000), bitwise_equal=same_scores(eng, rf, groups), ragged=res["ragged"],
                   rectangular=res["rectangular"], rectangular_over_ragged=res["rectangular"]["median_ms"] / res["ragged"]["median_ms"])
        print(json.dumps({name: out}), flush=True)
        del rf, groups
        eng._fe.clear()                     # the per-length front-end blobs of this row
        torch.cuda.empty_cache()
        return out

    rows = {}
    lengths = rng.integers(16000, 160001, B)
    rows["a_uniform_lengths"] = row(lengths, "a_uniform_lengths")
    rows["b_ten_lengths"] = row((lengths + 15999) // 16000 * 16000, "b_ten_lengths")
    rows["c_equal_lengths"] = row(np.full(B, 160000), "c_equal_lengths")
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.mode(), range_fallbacks=eng.range_fallbacks, repeats=a.repeats, seed=a.seed,
               note="ms per call: median and range of `repeats` synchronised calls after warm-up (host clock), the two variants of a row "
                    "alternating call by call; every clip is resident on the device and every front-end blob built before the clock starts; "
                    "ragged = MarbleNetEngine.run_ragged (one front-end launch, five encoder launches, range-flag read), rectangular = one "
                    "MarbleNetEngine.run call per distinct clip length (what drivers._grouped did with a file list); dynamic-axis mode",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
