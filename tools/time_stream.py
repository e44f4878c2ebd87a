"""Tick times of the Silero stream path (vadx.silero.VADIteratorBatch) on the GPU.

    python tools/time_stream.py [--out profiles/stream_tick.json] [--streams 1,64,...] [--windows 1,4,16]
    python tools/time_stream.py --profile S K TICKS         (a fixed run of step() ticks only, for rocprofv3 --kernel-trace --stats)
    python tools/time_stream.py --ragged [--out profiles/stream_tick_ragged.json] [--streams 64,4096,65536] [--windows 4,16]
                                                            (ragged ticks, step_ragged, against what a caller does today; see ragged_main)

For every (S, k): warm-up, then >= --seconds of timed ticks, three repeats.  A tick is timed by a host clock around work that ends in a
device synchronise (step() reads the range flag, which synchronises on "h2") and by HIP events around it.  Reported: ms per tick,
windows/s, and the real-time fraction: tick time over the k * 32 ms of audio it covers.  Inputs are float32 device tensors, which is what
VADIterator callers hand in.  Two reference rows: clips_pcm16 over the same S streams x (k * ticks) windows as one batch (ms per k
windows), and today's way at S = 64: 64 host VADIterators over vadx OnnxWrappers, one model call per window."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vadx  # noqa: F401,E402
from vadx import silero, weights  # noqa: E402

SCALE = np.float32(0.000030517578)


def audio(S, windows, dev, seed=7):
    """float32 bursts on the device: N(0, 3000) / N(0, 30) segments of int16 scale, times the reference's 1/32768"""
    g = torch.Generator(device=dev).manual_seed(seed)
    n = windows * 512
    x = torch.empty((S, n), dtype=torch.float32, device=dev)
    phase = (torch.arange(n, device=dev) // 12000) % 2
    for b in range(0, S, 4096):                 # row blocks: the temporaries of one block stay small at S = 65536
        r = x[b:b + 4096]
        loud = (phase + torch.randint(0, 2, (r.shape[0], 1), device=dev, generator=g)) % 2
        r.normal_(generator=g).mul_(30.0 + 2970.0 * loud).clamp_(-32768, 32767).round_().mul_(float(SCALE))
    return x


def timed(fn, seconds, repeats=3, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
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
        out.append(dict(ticks=n, host_ms=(time.perf_counter() - t0) * 1e3 / n, device_ms=e0.elapsed_time(e1) / n))
    return out


def best(reps, key):
    return min(r[key] for r in reps)


def median_ms(fn, ticks=20):
    """median host-clock ms of `ticks` calls, each ending in a device synchronise"""
    out = []
    for _ in range(ticks):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def ragged_main(a, eng, dev):
    """Ragged ticks against today's way, per (S, max k): median of 20 synchronised ticks, the two variants alternating A B A B on the same
    box (both medians of each are kept).  (a) every count = k against step; (b) every other stream idle against step(active=); (c)
    counts uniform in 0 .. k against the k masked one-window step ticks a caller issues today.  The host plan (stream_plan) and the device
    planner (HIP events around vadx_silero_stream_plan, _lib.trace) are reported on their own."""
    from vadx import _lib, ragged
    rows = []
    for S in [int(v) for v in a.streams.split(",")]:
        for k in [int(v) for v in a.windows.split(",")]:
            x = audio(S, k, dev)
            rng = np.random.default_rng(S + k)
            half = np.arange(S) % 2 == 0
            cases = dict(all_equal=np.full(S, k), half_idle=np.where(half, k, 0), uniform_0_k=rng.integers(0, k + 1, S))
            row = dict(S=S, k=k, mode=eng.mode())
            for name, counts in cases.items():
                its = [silero.VADIteratorBatch(eng, S) for _ in range(2)]
                masks = [counts > j for j in range(k)]

                def new():
                    its[0].step_ragged(x, counts)

                def old():
                    if name == "all_equal":
                        its[1].step(x)
                    elif name == "half_idle":
                        its[1].step(x, active=half)
                    else:
                        for j in range(k):
                            if masks[j].any():
                                its[1].step(x[:, j * 512:(j + 1) * 512], active=masks[j])
                for f in (new, old, new, old):          # warm-up, both
                    f()
                torch.cuda.synchronize()
                ms = [median_ms(f) for f in (new, old, new, old)]
                plan_ms = []
                for _ in range(20):
                    t0 = time.perf_counter()
                    ragged.stream_plan(counts, 512)
                    plan_ms.append((time.perf_counter() - t0) * 1e3)
                dev_plan, dev_tick = [], []
                for _ in range(20):
                    with _lib.trace() as tr:
                        its[0].step_ragged(x, counts)
                    dev_plan.append(tr.ms["vadx_silero_stream_plan"])
                    dev_tick.append(tr.ms["vadx_silero_stream_run_ragged"])
                row[name] = dict(ragged_ms=[ms[0], ms[2]], today_ms=[ms[1], ms[3]], windows=int(counts.sum()),
                                 tiles=ragged.stream_plan(counts, 512).tiles, host_plan_ms=float(np.median(plan_ms)),
                                 device_planner_ms=float(np.median(dev_plan)), device_tick_ms=float(np.median(dev_tick)),
                                 fallbacks=eng.range_fallbacks)
                print(json.dumps(dict(S=S, k=k, case=name, **row[name])), flush=True)
                del its
            rows.append(row)
            del x
            torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.mode(),
               note="median of 20 synchronised ticks (host clock, ms), variants alternating A B A B: [first, second] median of each; "
                    "ragged = step_ragged (host plan + one upload + device planner + tick + flag read), today = step / step(active=) / "
                    "k masked one-window step ticks; host_plan_ms = vadx.ragged.stream_plan alone; device_planner_ms / device_tick_ms = "
                    "HIP events around vadx_silero_stream_plan / vadx_silero_stream_run_ragged", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--streams", default=None)
    ap.add_argument("--windows", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--call-max-streams", type=int, default=65536)
    ap.add_argument("--profile", nargs=3, type=int, metavar=("S", "K", "TICKS"))
    a = ap.parse_args()
    a.out = a.out or ("profiles/stream_tick_ragged.json" if a.ragged else "profiles/stream_tick.json")
    a.streams = a.streams or ("64,4096,65536" if a.ragged else "1,64,1024,4096,16384,65536")
    a.windows = a.windows or ("4,16" if a.ragged else "1,4,16")
    dev = torch.device("cuda:0")
    eng = silero.SileroEngine(weights.silero_synthetic(1234), device=dev)
    if a.ragged:
        return ragged_main(a, eng, dev)
    if a.profile:
        S, k, n = a.profile
        it = silero.VADIteratorBatch(eng, S)
        x = audio(S, k, dev)
        for _ in range(n):
            it.step(x)
        torch.cuda.synchronize()
        print(f"profile run: S={S} k={k} ticks={n} mode={eng.mode()} fallbacks={eng.range_fallbacks}")
        return
    rows, ref_clips, ref_host = [], [], []
    for S in [int(v) for v in a.streams.split(",")]:
        for k in [int(v) for v in a.windows.split(",")]:
            it = silero.VADIteratorBatch(eng, S)
            x = audio(S, k, dev)
            step = timed(lambda: it.step(x), a.seconds)
            row = dict(S=S, k=k, mode=eng.mode(), step=step)
            if S <= a.call_max_streams:
                row["call"] = timed(lambda: it(x), a.seconds, warm=1)
            ms = best(step, "host_ms")
            row.update(step_ms=ms, step_device_ms=best(step, "device_ms"), windows_per_s=S * k / (ms / 1e3),
                       realtime_fraction=ms / (k * 32.0))
            if "call" in row:
                row["call_ms"] = best(row["call"], "host_ms")
            rows.append(row)
            print(json.dumps({kk: v for kk, v in row.items() if kk not in ("step", "call")}), flush=True)
            # reference: the same audio as one whole-clip batch (int16 PCM on the device), workspace capped at 4 M stream-windows
            W = max(k, min(16 * k, (4 << 20) // S) // k * k)
            pcm = (audio(S, W, dev) / float(SCALE)).round().to(torch.int16)
            rc = timed(lambda: eng.clips_pcm16(pcm), a.seconds)
            ref_clips.append(dict(S=S, k=k, windows=W, ms=best(rc, "host_ms"), ms_per_k_windows=best(rc, "host_ms") * k / W,
                                  windows_per_s=S * W / (best(rc, "host_ms") / 1e3)))
            print(json.dumps(ref_clips[-1]), flush=True)
            del it, x, pcm
            torch.cuda.empty_cache()
    # today's way: S host VADIterators, each over its own OnnxWrapper (one device call and one .item() per window)
    S = 64
    for k in [int(v) for v in a.windows.split(",")]:
        x = audio(S, k, dev).cpu()
        its = [silero.VADIterator(silero.OnnxWrapper(eng)) for _ in range(S)]

        def tick():
            for s in range(S):
                for t in range(k):
                    its[s](x[s, t * 512:(t + 1) * 512])
        r = timed(tick, a.seconds, warm=1)
        ref_host.append(dict(S=S, k=k, tick_ms=best(r, "host_ms"), windows_per_s=S * k / (best(r, "host_ms") / 1e3),
                             realtime_fraction=best(r, "host_ms") / (k * 32.0)))
        print(json.dumps(ref_host[-1]), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), mode=eng.mode(), seconds_per_repeat=a.seconds, repeats=3,
               note="ms per tick = best of three repeats of >= seconds_per_repeat of synchronised ticks (host clock; device events in "
                    "step_device_ms); realtime_fraction = tick ms / (k * 32 ms of audio)",
               rows=rows, ref_clips_pcm16=ref_clips, ref_host_iterators=ref_host)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
