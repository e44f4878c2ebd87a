"""Tick times of the FireRed stream path (vadx.firered.FireRedStreamBatch) on the GPU, beside the route it replaces on the same audio.

    python tools/time_firered_stream.py [--out profiles/firered_stream_tick.json] [--streams 64,4096,65536] [--chunks 1,4,8] [--calls 20]

For every (arithmetic, S, k) four things are timed, alternating call by call in one process so that drift of the clock or of the host hits
all alike, each call ending in a device synchronise, the median of --calls calls reported (after three warm-up calls of each at that shape):
  tick      one step() of S streams by k chunks of 2 560 samples: front-end, ONE vadx_firered_stream_tick at the library's grouping (group = 0),
            the range-flag read ("h2" reads it every tick, which synchronises) and the read-back of the event counts (+ the events);
  group1    the same step at one stream per workgroup;
  groupmax  the same step at 112 // (14 k) streams per workgroup;
  parent    what had to be written without this path: per chunk `FireRedEngine.stream_run` (a fresh caches_out per call; float32 MFMAs
            whatever the arithmetic) + `StreamVadPostprocessorBatch.process_batch(flush=False)` on its probabilities, k times per tick.
One more tick runs under HIP events around each library call: `tick_frontend_device_ms` and `tick_net_device_ms` say where its device time goes.
The weights are the synthetic checkpoint (seed 1234, published widths, no look-ahead); the audio is seeded bursts generated on the device."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vadx  # noqa: F401,E402
from vadx import _lib, firered, vadpost, weights  # noqa: E402

CHUNK, POST = firered.STREAM_CHUNK_SAMPLES, (5, 0.4, 5, 8, 2000, 20)


def audio(S, n, dev, seed=7):
    """int16 bursts on the device: N(0, 3000) / N(0, 30) segments"""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.empty((S, n), dtype=torch.int16, device=dev)
    phase = (torch.arange(n, device=dev) // 6000) % 2
    for b in range(0, S, 1024):                  # row blocks: the float temporaries of one block stay small
        r = x[b:b + 1024]
        loud = (phase + torch.randint(0, 2, (r.shape[0], 1), device=dev, generator=g)) % 2
        f = torch.empty(r.shape, dtype=torch.float32, device=dev).normal_(generator=g)
        r.copy_(f.mul_(30.0 + 2970.0 * loud).clamp_(-32768, 32767).round_().to(torch.int16))
    return x


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/firered_stream_tick.json")
    ap.add_argument("--streams", default="64,4096,65536")
    ap.add_argument("--chunks", default="1,4,8")
    ap.add_argument("--modes", default="f32,split,h2")
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    w = weights.firered_synthetic(1234, dict(weights.FIRERED_CFG, N2=0, S2=0))
    ks = [int(v) for v in a.chunks.split(",")]
    rows = []
    for S in [int(v) for v in a.streams.split(",")]:
        x_all = audio(S, max(ks) * CHUNK, dev)
        for mode in a.modes.split(","):
            eng = firered.FireRedEngine(w, CHUNK, device=dev)
            eng.blobs.arithmetic = mode
            it = firered.FireRedStreamBatch(eng, S, POST)
            post = vadpost.StreamVadPostprocessorBatch(*POST, streams=S, device=dev)
            state = dict(caches=eng.new_caches(S))
            it.step(x_all[:, :CHUNK].contiguous())                # every stream primed: caches and decision state are live
            for k in ks:
                x = x_all[:, :k * CHUNK].contiguous()
                gmax = 112 // (14 * k)

                def parent():
                    for j in range(k):
                        pr, state["caches"] = eng.stream_run(x[:, j * CHUNK:(j + 1) * CHUNK].contiguous(), state["caches"])
                        post.process_batch(pr[:, 0, :], flush=False)
                fns = dict(tick=lambda: it.step(x, k), group1=lambda: it.step(x, k, group=1), groupmax=lambda: it.step(x, k, group=gmax),
                           parent=parent)
                for _ in range(3):
                    for fn in fns.values():
                        fn()
                ms = {name: [] for name in fns}
                for _ in range(a.calls):
                    for name, fn in fns.items():
                        ms[name].append(timed(fn))
                med = {name: statistics.median(v) for name, v in ms.items()}
                with _lib.trace() as tr:                          # one more tick under HIP events: where its device time goes
                    it.step(x, k)
                row = dict(S=S, k=k, mode=eng.blobs.mode(), group_max=gmax, range_fallbacks=eng.blobs.range_fallbacks,
                           **{f"{name}_ms": med[name] for name in fns}, **{f"{name}_min_ms": min(ms[name]) for name in fns},
                           tick_frontend_device_ms=tr.ms["vadx_frontend_logmel"], tick_net_device_ms=tr.ms["vadx_firered_stream_tick"],
                           parent_over_tick=med["parent"] / med["tick"], group1_over_groupmax=med["group1"] / med["groupmax"],
                           chunks_per_s=S * k / (med["tick"] / 1e3), realtime_fraction=med["tick"] / (k * CHUNK / 16.0))
                rows.append(row)
                print(json.dumps(row), flush=True)
            del it, post, state, eng
            torch.cuda.empty_cache()
        del x_all
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), calls=a.calls, chunk_samples=CHUNK, post=POST,
               note="ms = median of `calls` synchronised calls (host clock around the call and a device synchronise), the four variants "
                    "alternating call by call in one process after three warm-up calls each; tick = FireRedStreamBatch.step at group = 0 with "
                    "the range-flag read and the event read-back inside; group1 / groupmax = the same step at 1 and at 112 // (14 k) streams "
                    "per workgroup; parent = k x (stream_run + StreamVadPostprocessorBatch.process_batch(flush=False)); realtime_fraction = "
                    "tick ms / (k * 160 ms of audio); tick_frontend_device_ms / tick_net_device_ms = HIP events around vadx_frontend_logmel / "
                    "vadx_firered_stream_tick in one further tick",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
