"""Tick times of the MarbleNet stream path (vadx.marblenet.MarbleNetStreamBatch) on the GPU, beside what a caller had to do without it.

    python tools/time_marblenet_stream.py [--out profiles/marblenet_stream_tick.json] [--streams 64,1024,4096] [--frames 1,4,16] [--calls 20]

For every (S, k), on fp16 x 2, two things are timed, alternating call by call (ABAB) in one process so that drift of the clock or of the
host hits both alike, each call ending in a device synchronise, the median of --calls calls reported after three warm-up calls of each:
  tick      one step() of S streams by k frames (320 k samples each): the range-flag read (which synchronises) and the read-back of n_out
            included.  Every stream is primed with 96 frames first, so each tick emits k frames per stream.
  sliding   the same k new scores per stream without the stream path: `run_ragged` over a sliding buffer of k + 146 encoder frames per
            stream (each emitted frame reads 70 encoder frames on either side and the prologue three more: 73 + k + 73), as one ragged
            batch of S clips of (k + 146) * 320 samples whose tables are built once, outside the timed region (lengths never change).
One more tick runs under HIP events around the library call: `tick_device_ms`.  Weights: the synthetic checkpoint (seed 1234)."""
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
from vadx import _lib, marblenet, weights  # noqa: E402

HOP, CONTEXT = 320, 146


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/marblenet_stream_tick.json")
    ap.add_argument("--streams", default="64,1024,4096")
    ap.add_argument("--frames", default="1,4,16")
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.gemm_mode("h2")
    eng = marblenet.MarbleNetEngine(weights.marblenet_synthetic(1234), device=dev)
    rng = np.random.default_rng(7)
    ks = [int(v) for v in a.frames.split(",")]
    rows = []
    for S in [int(v) for v in a.streams.split(",")]:
        sb = marblenet.MarbleNetStreamBatch(eng, S)
        prime = torch.from_numpy(np.rint(rng.standard_normal((1, 96 * HOP)) * 3000).astype(np.int16)).to(dev).expand(S, -1).contiguous()
        sb.step(prime)
        for k in ks:
            x = torch.from_numpy(np.rint(rng.standard_normal((1, k * HOP)) * 3000).astype(np.int16)).to(dev).expand(S, -1).contiguous()
            clip = np.rint(rng.standard_normal((k + CONTEXT) * HOP) * 3000).astype(np.int16)
            rf = eng.ragged([clip] * S)

            def tick():
                _, _, n_out = sb.step(x)
                return n_out.cpu()

            def sliding():
                _, s1, _ = eng.run_ragged(rf)
                return s1

            for _ in range(3):
                tick(); sliding()
            assert int(tick().min()) == k
            ta, tb = [], []
            for _ in range(a.calls):
                ta.append(timed(tick)); tb.append(timed(sliding))
            with _lib.trace() as tr:
                tick()
            row = dict(streams=S, frames=k, arithmetic=eng.mode(), tick_ms=statistics.median(ta), sliding_ms=statistics.median(tb),
                       tick_min_ms=min(ta), sliding_min_ms=min(tb), tick_device_ms=tr.ms.get("vadx_marblenet_stream_tick"),
                       range_fallbacks=eng.range_fallbacks)
            row["sliding_over_tick"] = row["sliding_ms"] / row["tick_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del rf
        del sb
        torch.cuda.empty_cache()
    out = dict(tool="tools/time_marblenet_stream.py", calls=a.calls, device=torch.cuda.get_device_name(0), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
