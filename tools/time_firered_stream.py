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
The weights are the synthetic checkpoint (seed 1234, published widths, no look-ahead); the audio is seeded bursts generated on the device.

    python tools/time_firered_stream.py --ragged [--out profiles/firered_stream_tick_ragged.json] [--streams 64,4096,65536] [--chunks 4,8]

times `step_ragged` (fp16 x 2, resident int16 rectangle [S, k * 2560], every stream primed, the two sides alternating tick by tick, median of
--calls synchronised ticks) at max k chunks per stream against what a caller does with `step` today:
  uniform   every count = k                 against step(chunks=k);
  half      every other stream idle         against step(chunks=k, active=);
  jitter    counts uniform in 0 .. k        against the k masked one-chunk ticks step(active = counts > j), j = 0 .. k - 1.
`plan_ms` is the host's column_stream_plan alone (it is inside every step_ragged figure too).

    python tools/time_firered_stream.py --step [--streams 4096] [--chunks 4] [--modes split,h2]

prints the median `step` tick alone, one JSON line per shape: run it in turn on two builds (VADX_LIBRARY) to compare them."""
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


def ab(fns, calls):
    """{name: (median, min) ms} of the functions alternating call by call, after three warm-up calls each"""
    for _ in range(3):
        for fn in fns.values():
            fn()
    ms = {name: [] for name in fns}
    for _ in range(calls):
        for name, fn in fns.items():
            ms[name].append(timed(fn))
    return {name: (statistics.median(v), min(v)) for name, v in ms.items()}


def step_only(a, dev, w):
    for S in [int(v) for v in a.streams.split(",")]:
        for mode in a.modes.split(","):
            eng = firered.FireRedEngine(w, CHUNK, device=dev)
            eng.blobs.arithmetic = mode
            it = firered.FireRedStreamBatch(eng, S, POST)
            for k in [int(v) for v in a.chunks.split(",")]:
                x = audio(S, k * CHUNK, dev)
                it.step(x[:, :CHUNK].contiguous())
                med, lo = ab(dict(step=lambda: it.step(x, k)), a.calls)["step"]
                print(json.dumps(dict(S=S, k=k, mode=eng.blobs.mode(), step_ms=med, step_min_ms=lo, library=_lib.LIB_PATH)), flush=True)


def ragged(a, dev, w):
    import numpy as np
    from vadx import ragged as plan
    rows = []
    for S in [int(v) for v in a.streams.split(",")]:
        eng = firered.FireRedEngine(w, CHUNK, device=dev)
        eng.blobs.arithmetic = "h2"
        for k in [int(v) for v in a.chunks.split(",")]:
            x = audio(S, k * CHUNK, dev)
            chunks = [x[:, j * CHUNK:(j + 1) * CHUNK].contiguous() for j in range(k)]
            its = [firered.FireRedStreamBatch(eng, S, POST) for _ in range(2)]
            for it in its:
                it.step(chunks[0])
            rag, rect = its
            rng = np.random.default_rng(S + k)
            patterns = dict(uniform=np.full(S, k), half=np.where(np.arange(S) % 2 == 0, k, 0), jitter=rng.integers(0, k + 1, S))
            for name, counts in patterns.items():
                if name == "uniform":
                    today = lambda: rect.step(x, k)                                        # noqa: E731
                elif name == "half":
                    today = lambda: rect.step(x, k, active=counts > 0)                      # noqa: E731
                else:
                    def today():
                        for j in range(k):
                            if (counts > j).any():
                                rect.step(chunks[j], active=counts > j)
                t = ab(dict(ragged=lambda: rag.step_ragged(x, counts, chunk=CHUNK), today=today), a.calls)
                t0 = []
                for _ in range(a.calls):
                    c0 = time.perf_counter()
                    _, _, wg = plan.column_stream_plan(counts, 112 // 14)
                    t0.append((time.perf_counter() - c0) * 1e3)
                with _lib.trace() as tr:
                    rag.step_ragged(x, counts, chunk=CHUNK)
                row = dict(S=S, k=k, pattern=name, chunks=int(counts.sum()), workgroups=len(wg) - 1, ragged_ms=t["ragged"][0],
                           ragged_min_ms=t["ragged"][1], today_ms=t["today"][0], today_min_ms=t["today"][1],
                           today_over_ragged=t["today"][0] / t["ragged"][0], plan_ms=statistics.median(t0),
                           ragged_net_device_ms=tr.ms["vadx_firered_stream_tick_ragged"], ragged_frontend_device_ms=tr.ms["vadx_frontend_logmel"],
                           range_fallbacks=eng.blobs.range_fallbacks)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del its, rag, rect, x, chunks
            torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), calls=a.calls, chunk_samples=CHUNK, post=POST, mode="h2",
               note="ms = median of `calls` synchronised ticks, host clock, step_ragged and today's route alternating tick by tick after three "
                    "warm-up calls each; uniform = every count k against step(chunks=k); half = every other stream idle against "
                    "step(chunks=k, active=); jitter = counts uniform in 0..k against the k masked one-chunk ticks; plan_ms = "
                    "column_stream_plan alone on the host (inside ragged_ms too); *_device_ms = HIP events around the library call in one more tick",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", default=None)
    ap.add_argument("--chunks", default=None)
    ap.add_argument("--modes", default=None)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    a.out = a.out or ("profiles/firered_stream_tick_ragged.json" if a.ragged else "profiles/firered_stream_tick.json")
    a.streams = a.streams or ("4096" if a.step else "64,4096,65536")
    a.chunks = a.chunks or ("4" if a.step else "4,8" if a.ragged else "1,4,8")
    a.modes = a.modes or ("split,h2" if a.step else "f32,split,h2")
    dev = torch.device("cuda:0")
    w = weights.firered_synthetic(1234, dict(weights.FIRERED_CFG, N2=0, S2=0))
    if a.ragged:
        return ragged(a, dev, w)
    if a.step:
        return step_only(a, dev, w)
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
