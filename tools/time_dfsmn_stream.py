"""Tick times of the DFSMN stream path (vadx.dfsmn.DfsmnStreamBatch) on the GPU, beside the network it wraps on the same windows.

    python tools/time_dfsmn_stream.py [--out profiles/dfsmn_stream_tick.json] [--streams 64,1024] [--windows 1,2] [--calls 5]

For every (S, k, active fraction) two things are timed, alternating call by call in one process, each call ending in a device synchronise,
the median of --calls calls reported (after one warm-up call of each at that shape):
  tick      one step() of S primed near + far streams by k windows: vadx_dfsmn_stream_windows, `run` on the active streams' rows,
            vadx_dfsmn_stream_vote, and the read-back of flags and tail to the host;
  run_vote  `DfsmnEngine.run` + vadx_dfsmn_vote + the flag read-back on the SAME window rows, already assembled: what a tick cannot do without.
active = 0.5 is the same tick with every other stream inactive (run_vote then sees only the active streams' rows): an inactive stream costs
no network time.  The weights are the synthetic checkpoint (seed 1234); the audio is seeded bursts."""
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
from vadx import _lib, dfsmn, weights  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/dfsmn_stream_tick.json")
    ap.add_argument("--streams", default="64,1024")
    ap.add_argument("--windows", default="1,2")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = dfsmn.DfsmnEngine(weights.dfsmn_synthetic(1234), device=dev)
    lb, stride = eng.grid()
    ks = [int(v) for v in a.windows.split(",")]
    rows = []
    for S in [int(v) for v in a.streams.split(",")]:
        n = eng.L + (max(ks) - 1) * stride
        near = torch.from_numpy(weights.burst_clips(S, n, seed=7)).to(dev)
        far = torch.from_numpy(weights.burst_clips(S, n, seed=8)).to(dev)
        sb = dfsmn.DfsmnStreamBatch(eng, S)
        sb.step(near[:, :eng.L].contiguous(), far[:, :eng.L].contiguous(), 1)        # every stream primed
        for k in ks:
            for frac in (1.0, 0.5):
                act = None if frac == 1.0 else (np.arange(S) % 2 == 0)
                n_act = S if act is None else int(act.sum())
                x, y = near[:, :k * stride].contiguous(), far[:, :k * stride].contiguous()
                wn, wf = near[:n_act, :eng.L].repeat_interleave(k, 0).contiguous(), far[:n_act, :eng.L].repeat_interleave(k, 0).contiguous()
                flags = torch.empty((n_act, k * (eng.T_A - lb) + lb), dtype=torch.uint8, device=dev)

                def tick():
                    f, t_ = sb.step(x, y, k, active=act)
                    return f.cpu(), t_.cpu()

                def run_vote():
                    vad = eng.run(wn, wf, 1)
                    _lib.check(_lib.lib().vadx_dfsmn_vote(vad.data_ptr(), n_act, k, eng.T_A, lb, 0.5, 0.5, flags.data_ptr(), _lib.stream_ptr()))
                    return flags.cpu()
                fns = dict(tick=tick, run_vote=run_vote)
                for fn in fns.values():
                    fn()
                ms = {name: [] for name in fns}
                for _ in range(a.calls):
                    for name, fn in fns.items():
                        ms[name].append(timed(fn))
                med = {name: statistics.median(v) for name, v in ms.items()}
                row = dict(S=S, k=k, active=frac, rows=n_act * k, n=a.calls, **{f"{name}_ms": med[name] for name in fns},
                           **{f"{name}_min_ms": min(ms[name]) for name in fns}, **{f"{name}_max_ms": max(ms[name]) for name in fns},
                           tick_over_run_vote=med["tick"] / med["run_vote"], realtime_fraction=med["tick"] / (k * stride / 16.0))
                rows.append(row)
                print(json.dumps(row), flush=True)
        del sb, near, far
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.iccrn.arithmetic or _lib.gemm_mode(), range_fallbacks=eng.range_fallbacks,
               look_backward=lb, stride=stride, sub_batch=eng.sub_batch,
               note="ms = median of n synchronised calls (host clock around the call and a device synchronise), the two variants alternating call "
                    "by call in one process after one warm-up call each; tick = DfsmnStreamBatch.step (stream_windows, run on the active rows, "
                    "stream_vote) + flags and tail read back to the host; run_vote = DfsmnEngine.run + vadx_dfsmn_vote + flag read-back on the "
                    "same number of assembled window rows; active = fraction of streams with audio in the tick; realtime_fraction = tick ms / "
                    "(k * 680 ms of new audio per stream)",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
