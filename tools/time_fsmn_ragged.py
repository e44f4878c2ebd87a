"""Times of the ragged FSMN path (FsmnEngine.flags_ragged over a vadx.ragged.RaggedBatch) on the GPU, beside FsmnEngine.flags().

    python tools/time_fsmn_ragged.py [--out profiles/fsmn_ragged.json] [--clips 1024] [--repeats 20]

Three questions, one process, every clip resident on the device before the clock starts (host packing and the upload are outside
every timed region; the bytes each way would upload are reported beside the times):
  (a) `--clips` clips with lengths drawn uniformly from 1 - 10 s (seeded): one flags_ragged call against one flags() call per distinct
      length, which is what drivers._grouped did with a list of files (beside it: one flags() call per distinct WINDOW COUNT, the
      grouping a caller could do by hand) -- and the same with the lengths rounded up to 10 distinct values, the grouped way's best case;
  (b) `--clips` clips of 10 s each: flags_ragged against ONE flags() call on the same audio -- the price of the gather pass and the
      table indirection;
  (c) the set of (a) with order = identity against the default longest-first order.
A call is everything the method does (gather, window statistics, log-mel front-end, the clips kernel, on "h2" the range-flag read) and
ends in a device synchronise.  Per variant: warm-up, then `--repeats` timed calls, the variants of one question alternating call by
call; reported are the median and the range (min, max) of the host clock in ms."""
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
from vadx import fsmn, ragged, weights  # noqa: E402


def bursts(rng, n):
    """int16 bursts: N(0, 3000) / N(0, 30) segments of 0.75 s"""
    loud = ((np.arange(n) // 12000 + int(rng.integers(0, 2))) % 2).astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * (30.0 + 2970.0 * loud)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def grouped(eng, rb, keys):
    """One flags() batch per distinct key (device int16 [G, n], W, clip indices): keys = rb.lengths is what drivers._grouped did with a
    list of files (one batch per distinct clip length), keys = rb.windows groups clips that merely share a window count"""
    by_len = {}
    for b, n in enumerate(keys.tolist()):
        by_len.setdefault(n, []).append(b)
    return [(torch.from_numpy(np.stack([rb.padded(b) for b in idx])).to(eng.device), int(rb.windows[idx[0]]), idx) for idx in by_len.values()]


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


def same_flags(eng, rb, groups):
    flags, nflags = eng.flags_ragged(rb)
    for a, W, idx in groups:
        ref = eng.flags(a, W)
        if not all(torch.equal(flags[b, :nflags[b]], ref[j]) for j, b in enumerate(idx)):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fsmn_ragged.json")
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = fsmn.FsmnEngine(weights.fsmn_synthetic(1234), device=dev)
    lb, stride = eng.grid()
    rng = np.random.default_rng(a.seed)
    B = a.clips
    noise = rng.standard_normal((B, 16000))

    def pack(lengths):
        rb = ragged.RaggedBatch.from_clips([bursts(rng, int(n)) for n in lengths], eng.L, stride, noise, None, dev)
        return rb, grouped(eng, rb, rb.lengths)

    def describe(rb, groups):
        return dict(clips=len(rb), windows=rb.n_windows, max_windows=rb.max_windows, distinct_lengths=len(groups),
                    packed_upload_bytes=int(rb.pcm_host.nbytes), rectangular_upload_bytes=int(len(rb) * rb.padded_lengths.max() * 2),
                    audio_seconds=float(rb.lengths.sum() / 16000))

    rows = {}
    # (a) + (c): any lengths
    lengths = rng.integers(16000, 160001, B)
    rb, groups = pack(lengths)
    by_windows = grouped(eng, rb, rb.windows)
    res = time_variants({"ragged": lambda: eng.flags_ragged(rb),
                         "ragged_identity_order": lambda: eng.flags_ragged(rb, order="identity"),
                         "grouped": lambda: [eng.flags(x, W) for x, W, _ in groups],
                         "grouped_by_windows": lambda: [eng.flags(x, W) for x, W, _ in by_windows]}, a.repeats)
    rows["a_uniform_lengths"] = dict(describe(rb, groups), bitwise_equal=same_flags(eng, rb, groups), ragged=res["ragged"], grouped=res["grouped"],
                                     grouped_over_ragged=res["grouped"]["median_ms"] / res["ragged"]["median_ms"],
                                     distinct_window_counts=len(by_windows), grouped_by_windows=res["grouped_by_windows"])
    del by_windows
    rows["c_order"] = dict(describe(rb, groups), longest_first=res["ragged"], identity=res["ragged_identity_order"],
                           identity_over_longest_first=res["ragged_identity_order"]["median_ms"] / res["ragged"]["median_ms"])
    print(json.dumps({k: rows[k] for k in ("a_uniform_lengths", "c_order")}), flush=True)
    del rb, groups
    torch.cuda.empty_cache()
    # (a'): the same draw rounded up to whole seconds: 10 distinct lengths
    rb, groups = pack((lengths + 15999) // 16000 * 16000)
    res = time_variants({"ragged": lambda: eng.flags_ragged(rb), "grouped": lambda: [eng.flags(x, W) for x, W, _ in groups]}, a.repeats)
    rows["a_ten_lengths"] = dict(describe(rb, groups), bitwise_equal=same_flags(eng, rb, groups), ragged=res["ragged"], grouped=res["grouped"],
                                 grouped_over_ragged=res["grouped"]["median_ms"] / res["ragged"]["median_ms"])
    print(json.dumps({"a_ten_lengths": rows["a_ten_lengths"]}), flush=True)
    del rb, groups
    torch.cuda.empty_cache()
    # (b): equal lengths, where flags() needs neither the gather nor the tables
    rb, groups = pack(np.full(B, 160000))
    (x, W, _), = groups
    res = time_variants({"ragged": lambda: eng.flags_ragged(rb), "flags": lambda: eng.flags(x, W)}, a.repeats)
    rows["b_equal_lengths"] = dict(describe(rb, groups), bitwise_equal=same_flags(eng, rb, groups), ragged=res["ragged"], flags=res["flags"],
                                   ragged_over_flags=res["ragged"]["median_ms"] / res["flags"]["median_ms"])
    print(json.dumps({"b_equal_lengths": rows["b_equal_lengths"]}), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.blobs.mode(), range_fallbacks=eng.blobs.range_fallbacks, look_backward=lb,
               stride=stride, repeats=a.repeats, seed=a.seed,
               note="ms per call: median and range of `repeats` synchronised calls after warm-up (host clock), the variants of one row "
                    "alternating call by call; every clip is resident on the device before the clock starts; ragged = FsmnEngine.flags_ragged "
                    "(gather, window statistics, front-end, clips kernel, range-flag read), grouped = one FsmnEngine.flags call per distinct "
                    "clip length (grouped_by_windows: per distinct window count), flags = one FsmnEngine.flags call; *_upload_bytes = what each layout would send over the host link",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
