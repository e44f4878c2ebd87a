"""Times of the ragged DFSMN path (DfsmnEngine.flags_ragged over a vadx.ragged.RaggedPairs) on the GPU, beside the rectangular path.

    python tools/time_dfsmn_ragged.py [--out profiles/dfsmn_ragged.json] [--pairs 1024] [--repeats 5] [--slow-repeats 2]

Two questions, one process, every pair resident on the device before the clock starts (host packing and the upload are outside every
timed region; the bytes each way would upload are reported beside the times):
  (a) `--pairs` near / far pairs with lengths drawn uniformly from 1 - 10 s (seeded): one flags_ragged call against one rectangular batch
      (`run` + vadx_dfsmn_vote) per distinct length, which is what drivers._grouped did with a list of file pairs -- and the same with the
      lengths rounded up to whole seconds, the grouped way's best case;
  (b) `--pairs` pairs of 10 s each: flags_ragged against ONE rectangular `run` + vadx_dfsmn_vote on the same audio -- the price of the two
      gather passes and the table indirection where the ragged path is not needed.
A call is everything the method does (gathers, front-ends, network, vote, on "h2" the range-flag read) and ends in a device synchronise.
Per variant: one warm-up call, then the timed calls, the variants of one row alternating call by call; reported are the median and the
range (min, max) of the host clock in ms and the number of calls n.  The per-length baseline of (a) is slow: it gets --slow-repeats calls."""
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
from vadx import _lib, dfsmn, ragged, weights  # noqa: E402


def bursts(rng, n):
    """int16 bursts: N(0, 3000) / N(0, 30) segments of 0.75 s"""
    loud = ((np.arange(n) // 12000 + int(rng.integers(0, 2))) % 2).astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * (30.0 + 2970.0 * loud)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def grouped(eng, rp):
    """One rectangular batch per distinct clip length: (near int16 [G, n], far, W, pair indices), on the device"""
    by_len = {}
    for b, n in enumerate(rp.lengths.tolist()):
        by_len.setdefault(n, []).append(b)
    up = lambda side, idx: torch.from_numpy(np.stack([rp.padded(b)[side] for b in idx])).to(eng.device)      # noqa: E731
    return [(up(0, idx), up(1, idx), int(rp.windows[idx[0]]), idx) for idx in by_len.values()]


def rectangular(eng, near, far, W):
    """`run` + vadx_dfsmn_vote: what DfsmnEngine.detect launches for an equal-length batch -> flags u8 [G, W * 36 + 15]"""
    lb, stride = eng.grid()
    vad = eng.run(near, far, W, stride)
    flags = torch.empty((near.shape[0], W * (eng.T_A - lb) + lb), dtype=torch.uint8, device=eng.device)
    _lib.check(_lib.lib().vadx_dfsmn_vote(vad.data_ptr(), near.shape[0], W, eng.T_A, lb, 0.5, 0.5, flags.data_ptr(), _lib.stream_ptr()))
    return flags


def time_variants(variants, repeats, warmup=1):
    """{name: fn} with repeats {name: n} -> {name: dict(median_ms, min_ms, max_ms, n)}; the variants alternate call by call"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for r in range(max(repeats.values())):
        for k, fn in variants.items():
            if r < repeats[k]:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), n=len(v)) for k, v in ms.items()}


def flag_mismatches(eng, rp, groups):
    """pairs whose ragged flags differ from their rectangular batch's (scores may differ in the last bits between the two sub-batch cuts)"""
    flags, nflags = eng.flags_ragged(rp)
    bad = 0
    for near, far, W, idx in groups:
        ref = rectangular(eng, near, far, W)
        bad += sum(not torch.equal(flags[b, :nflags[b]], ref[j]) for j, b in enumerate(idx))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/dfsmn_ragged.json")
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow-repeats", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = dfsmn.DfsmnEngine(weights.dfsmn_synthetic(1234), device=dev)
    lb, stride = eng.grid()
    rng = np.random.default_rng(a.seed)
    B = a.pairs
    noise = rng.standard_normal((B, eng.L))

    def pack(lengths):
        rp = ragged.RaggedPairs.from_clips([bursts(rng, int(n)) for n in lengths], [bursts(rng, int(n)) for n in lengths], eng.L, stride,
                                           noise, noise, None, dev)
        return rp, grouped(eng, rp)

    def describe(rp, groups):
        return dict(pairs=len(rp), windows=rp.n_windows, max_windows=rp.max_windows, distinct_lengths=len(groups),
                    packed_upload_bytes=int(2 * rp.near_host.nbytes), rectangular_upload_bytes=int(2 * len(rp) * rp.padded_lengths.max() * 2),
                    audio_seconds=float(rp.lengths.sum() / 16000))

    rows = {}
    lengths = rng.integers(16000, 160001, B)
    for key, lens, slow in (("a_uniform_lengths", lengths, a.slow_repeats), ("a_whole_seconds", (lengths + 15999) // 16000 * 16000, a.repeats)):
        rp, groups = pack(lens)
        res = time_variants({"ragged": lambda: eng.flags_ragged(rp), "grouped": lambda: [rectangular(eng, n, f, W) for n, f, W, _ in groups]},
                            {"ragged": a.repeats, "grouped": slow})
        rows[key] = dict(describe(rp, groups), pairs_with_other_flags=flag_mismatches(eng, rp, groups), **res,
                         grouped_over_ragged=res["grouped"]["median_ms"] / res["ragged"]["median_ms"])
        print(json.dumps({key: rows[key]}), flush=True)
        del rp, groups
        torch.cuda.empty_cache()
    # (b): equal lengths, where the rectangular path needs neither the gathers nor the tables
    rp, groups = pack(np.full(B, 160000))
    (near, far, W, _), = groups
    res = time_variants({"ragged": lambda: eng.flags_ragged(rp), "rectangular": lambda: rectangular(eng, near, far, W)},
                        {"ragged": a.repeats, "rectangular": a.repeats})
    rows["b_equal_lengths"] = dict(describe(rp, groups), pairs_with_other_flags=flag_mismatches(eng, rp, groups), **res,
                                   ragged_over_rectangular=res["ragged"]["median_ms"] / res["rectangular"]["median_ms"])
    print(json.dumps({"b_equal_lengths": rows["b_equal_lengths"]}), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.iccrn.arithmetic or _lib.gemm_mode(), range_fallbacks=eng.range_fallbacks,
               look_backward=lb, stride=stride, sub_batch=eng.sub_batch, seed=a.seed,
               note="ms per call: median and range of n synchronised calls after one warm-up call (host clock), the variants of one row "
                    "alternating call by call; every pair is resident on the device before the clock starts; ragged = DfsmnEngine.flags_ragged "
                    "(two gathers, network on sum W rows, ragged vote, range-flag read), grouped = one `run` + vadx_dfsmn_vote per distinct "
                    "clip length, rectangular = one `run` + vadx_dfsmn_vote; *_upload_bytes = what each layout would send over the host link; "
                    "pairs_with_other_flags = pairs whose flags differ between the two ways (their scores may differ in the last bits)",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
