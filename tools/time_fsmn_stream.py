"""Tick times of the FSMN stream path (vadx.fsmn.FsmnStreamBatch) on the GPU, beside FsmnEngine.flags() over the same windows.

    python tools/time_fsmn_stream.py [--out profiles/fsmn_stream_tick.json] [--streams 64,4096] [--windows 1,4]

For every (S, k): warm-up, then >= --seconds of timed calls, three repeats, the two paths alternating repeat by repeat in one process.  A
tick is one step() of S primed streams by k windows: window assembly, window statistics, log-mel front-end, the stream kernel, and the
range-flag read ("h2" reads it every tick, which synchronises) -- all inside the timed region, which ends in a device synchronise.
Beside it: flags() on B = S resident clips of W = k windows, i.e. the same front-end and the same dense-layer arithmetic on the same
number of windows without any carried state (it reads the range flag too).  Reported: ms per call (best of the repeats, host clock;
device events beside it), windows/s, and the real-time fraction: tick time over the k * stride / 16000 s of audio it covers.

    python tools/time_fsmn_stream.py --ragged [--out-ragged profiles/fsmn_stream_tick_ragged.json] [--ragged-streams 64,4096,65536] [--k 4]

writes the file above first, then times FsmnStreamBatch.step_ragged at max count k against what a caller does with `step`, in three
patterns: (a) every count = k against step(windows=k); (b) every other stream idle against step(windows=k, active=); (c) counts uniform
in 0 .. k against the k masked one-window ticks that serve them.  fp16 x 2, resident int16 samples, the median of 20 synchronised ticks,
the two sides alternating tick by tick (ABAB) in one process; beside the wall time of a tick its device time (events) and the host's
planning time (vadx.ragged.window_stream_plan) at that S."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vadx  # noqa: F401,E402
from vadx import fsmn, weights  # noqa: E402


def audio(S, n, dev, seed=7):
    """int16 bursts on the device: N(0, 3000) / N(0, 30) segments"""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.empty((S, n), dtype=torch.int16, device=dev)
    phase = (torch.arange(n, device=dev) // 12000) % 2
    for b in range(0, S, 1024):                  # row blocks: the float temporaries of one block stay small
        r = x[b:b + 1024]
        loud = (phase + torch.randint(0, 2, (r.shape[0], 1), device=dev, generator=g)) % 2
        f = torch.empty(r.shape, dtype=torch.float32, device=dev).normal_(generator=g)
        r.copy_(f.mul_(30.0 + 2970.0 * loud).clamp_(-32768, 32767).round_().to(torch.int16))
    return x


def one_repeat(fn, seconds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, t0 = 0, time.perf_counter()
    e0.record()
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        if time.perf_counter() - t0 >= seconds and n >= 3:
            break
    e1.record()
    torch.cuda.synchronize()
    return dict(calls=n, host_ms=(time.perf_counter() - t0) * 1e3 / n, device_ms=e0.elapsed_time(e1) / n)


def timed(fn):
    """one synchronised call -> (wall ms, device ms between two events)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def ragged_rows(eng, streams, k, ticks, dev):
    """The three patterns at every S that fits: rows of medians over `ticks` alternating ticks."""
    from vadx import ragged
    _, stride = eng.grid()
    rng = np.random.default_rng(11)
    rows = []
    for S in streams:
        # records, the window buffer, log-mel and the samples of S streams x k windows, twice (two batches): skip an S that cannot fit
        per_stream = 2 * 4 * 128 * 19 * 4 + k * (eng.L * 2 + eng.T * 81 * 4 + stride * 2)
        free = torch.cuda.mem_get_info(dev)[0]
        if 3 * S * per_stream > free:
            rows.append(dict(S=S, k=k, skipped=f"needs about {3 * S * per_stream / 2**30:.0f} GiB, {free / 2**30:.0f} GiB free"))
            print(json.dumps(rows[-1]), flush=True)
            continue
        x = audio(S, k * stride, dev)
        x1 = x[:, :stride]
        every_other = np.arange(S) % 2 == 0
        uniform = rng.integers(0, k + 1, S)
        patterns = [("a: every count = k", np.full(S, k), lambda it: it.step(x, k)),
                    ("b: every other stream idle", np.where(every_other, k, 0), lambda it: it.step(x, k, active=every_other)),
                    ("c: counts uniform in 0 .. k", uniform, lambda it: [it.step(x1, 1, active=uniform > j) for j in range(k)])]
        for name, counts, today in patterns:
            a, b = fsmn.FsmnStreamBatch(eng, S), fsmn.FsmnStreamBatch(eng, S)
            for it in (a, b):
                it.step(audio(S, eng.L, dev, seed=3))                 # prime: from here on a stream consumes n * stride samples
            new = lambda: a.step_ragged(x, counts, max_windows=k)     # noqa: E731
            old = lambda: today(b)                                    # noqa: E731
            for _ in range(3):
                new()
                old()
            tn, to = [], []
            for _ in range(ticks):                                    # ABAB
                tn.append(timed(new))
                to.append(timed(old))
            plan = []
            for _ in range(ticks):
                t0 = time.perf_counter()
                ragged.window_stream_plan(counts, k)
                plan.append((time.perf_counter() - t0) * 1e3)
            row = dict(S=S, k=k, pattern=name, windows=int(counts.sum()), mode=eng.blobs.mode(), range_fallbacks=eng.blobs.range_fallbacks,
                       ragged_ms=median([v[0] for v in tn]), ragged_device_ms=median([v[1] for v in tn]),
                       step_ms=median([v[0] for v in to]), step_device_ms=median([v[1] for v in to]), plan_ms=median(plan))
            row["ragged_over_step"] = row["ragged_ms"] / row["step_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del a, b
            torch.cuda.empty_cache()
        del x, x1
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/fsmn_stream_tick.json")
    ap.add_argument("--streams", default="64,4096")
    ap.add_argument("--windows", default="1,4")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ragged", action="store_true", help="then time step_ragged against step and write --out-ragged")
    ap.add_argument("--out-ragged", default="profiles/fsmn_stream_tick_ragged.json")
    ap.add_argument("--ragged-streams", default="64,4096,65536")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--ticks", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = fsmn.FsmnEngine(weights.fsmn_synthetic(1234), device=dev)
    lb, stride = eng.grid()
    rows = []
    for S in [int(v) for v in a.streams.split(",")]:
        for k in [int(v) for v in a.windows.split(",")]:
            it = fsmn.FsmnStreamBatch(eng, S)
            it.step(audio(S, eng.L, dev, seed=3))                     # prime: from here on every tick consumes k * stride samples
            x = audio(S, k * stride, dev)
            clips = audio(S, (k - 1) * stride + eng.L, dev)
            tick, whole = (lambda: it.step(x, k)), (lambda: eng.flags(clips, k))
            for _ in range(3):                                        # warm-up of both paths at this shape
                tick()
                whole()
            torch.cuda.synchronize()
            rt, rw = [], []
            for _ in range(a.repeats):                                # alternating: drift of the clock or the host hits both alike
                rt.append(one_repeat(tick, a.seconds))
                rw.append(one_repeat(whole, a.seconds))
            tms, wms = min(r["host_ms"] for r in rt), min(r["host_ms"] for r in rw)
            row = dict(S=S, k=k, mode=eng.blobs.mode(), range_fallbacks=eng.blobs.range_fallbacks,
                       tick_ms=tms, tick_device_ms=min(r["device_ms"] for r in rt), flags_ms=wms,
                       flags_device_ms=min(r["device_ms"] for r in rw), tick_over_flags=tms / wms,
                       windows_per_s=S * k / (tms / 1e3), realtime_fraction=tms / (k * stride / 16.0), tick=rt, flags=rw)
            rows.append(row)
            print(json.dumps({kk: v for kk, v in row.items() if kk not in ("tick", "flags")}), flush=True)
            del it, x, clips
            torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.blobs.mode(), look_backward=lb, stride=stride, seconds_per_repeat=a.seconds,
               repeats=a.repeats,
               note="ms per call = best of the repeats of >= seconds_per_repeat of synchronised calls (host clock; device events in *_device_ms), "
                    "tick and flags() alternating; tick = FsmnStreamBatch.step of S primed streams x k windows with the range-flag read inside; "
                    "flags = FsmnEngine.flags at B = S, W = k; realtime_fraction = tick ms / (k * stride / 16 ms of audio)",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)
    if a.ragged:
        rows = ragged_rows(eng, [int(v) for v in a.ragged_streams.split(",")], a.k, a.ticks, dev)
        out = dict(device=torch.cuda.get_device_name(0), mode=eng.blobs.mode(), look_backward=lb, stride=stride, ticks=a.ticks,
                   note="ms = median of `ticks` synchronised ticks, step_ragged and today's path alternating tick by tick in one process, "
                        "resident int16 samples, every stream primed; *_ms = wall time of a tick (host clock, the range-flag read inside), "
                        "*_device_ms = device events around the same tick, plan_ms = vadx.ragged.window_stream_plan on the host (inside "
                        "ragged_ms).  step_ms: (a) step(windows=k), (b) step(windows=k, active=), (c) k masked one-window ticks",
                   rows=rows)
        with open(a.out_ragged, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", a.out_ragged)


if __name__ == "__main__":
    main()
