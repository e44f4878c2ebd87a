"""The 8 kHz Silero network against the 16 kHz one on one MI355X: per arithmetic, one whole-clip step (encoder + recurrent kernel + the
range-flag read) over B = 4096 clips of 10 s -- 80 000 samples at 8 kHz, 160 000 at 16 kHz, 313 windows each -- alternating A B A B in
one process.  Prints one JSON line per arithmetic (median ms of each rate) and writes them to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import vadx  # noqa: E402,F401
from vadx import silero, weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--arith", default="h2,split,f32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    eng = silero.SileroEngine(weights.silero_synthetic(1234), weights_8k=weights.silero8k_synthetic(1234))
    B = a.batch
    x16 = torch.from_numpy(weights.burst_clips(B, 160000, seed=1).astype(np.float32) * np.float32(0.000030517578)).cuda()
    x8 = x16[:, ::2].contiguous()
    res = []
    for m in a.arith.split(","):
        eng.arithmetic = m
        t = {8000: [], 16000: []}
        for sr, x in ((8000, x8), (16000, x16)):           # warm-up (workspace growth, first launches)
            eng.clips(x, sampling_rate=sr)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for sr, x in ((8000, x8), (16000, x16)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.clips(x, sampling_rate=sr)             # (the guarded call reads the range flag on "h2": synchronises)
                torch.cuda.synchronize()
                t[sr].append((time.perf_counter() - t0) * 1e3)
        r = {"arith": m, "batch": B, "windows": 313, "ms_8k": float(np.median(t[8000])), "ms_16k": float(np.median(t[16000])),
             "ms_8k_all": [round(v, 3) for v in t[8000]], "ms_16k_all": [round(v, 3) for v in t[16000]],
             "fallbacks": eng.range_fallbacks}
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
