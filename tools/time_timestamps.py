"""Times of vadx.tstable (flags / frame tables -> timestamps on the device) against the host paths `detect` runs, on the GPU.

    python tools/time_timestamps.py [--out profiles/timestamps.json] [--repeats 20]

One process; the inputs are resident on the device before a clock starts.  Workloads:
  flags    4096 clips x 1095 FSMN-shaped silence flags (10 s clips: config 3's shape), about six speech runs per clip,
           frame 0.01 s, fusion_threshold 0.3, min_duration 0.2;
  frames   4096 tracks x 1000 frames of FireRed-shaped scores (block-random), through VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0).
Per workload, each the median (and range) of `--repeats` synchronised calls after two warm-up calls, host clock unless said:
  host     what `detect` does today: flags.cpu() + the clips.flag_timestamps loop / clips.track_segments (vadx_vadpost, the
           counts.max() read, the table read-back, segments_to_seconds per clip);
  table    the new path up to a device table: tstable.from_flags / clips.track_table (vadx_vadpost + vadx_timestamps_frames), with the
           16-byte head read;
  lists    `table` + `.lists()`: the read-back of the used columns and the Python lists -- what a caller who wants host lists pays;
  kernel   vadx_timestamps_flags / vadx_timestamps_frames alone (device events);
and for `frames`, `vadpost`: vadx_vadpost alone (device events), the launch both paths share.  The results of both paths are compared
before anything is timed."""
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
from vadx import _lib, clips, tstable, vadpost  # noqa: E402

DEV = torch.device("cuda:0")


def stats(v):
    return dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), calls=len(v))


def by_events(fn, entry, repeats, warmup=2):
    """device time of the C entry point `entry` inside fn(): HIP events right around that call (vadx._lib.trace)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        with _lib.trace() as tr:
            fn()
        ms.append(tr.ms[entry] / tr.calls[entry])
    return stats(ms)


def by_host(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "timestamps.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
    args = ap.parse_args()
    rng = np.random.default_rng(7)
    B, R = args.batch, args.repeats
    res = dict(device=torch.cuda.get_device_name(0), batch=B, repeats=R)

    # ---- flags
    n, fd, fusion, minimum = 1095, 0.01, 0.3, 0.2
    blocks = rng.random((B, n // 90 + 1)) < 0.5
    flags_h = np.repeat(blocks, 90, axis=1)[:, :n].astype(np.uint8)
    flags = torch.from_numpy(flags_h).to(DEV)

    def host_flags():
        f = flags.cpu().numpy()
        return [clips.flag_timestamps(f[b], fd, fusion, minimum) for b in range(B)]
    table = lambda: tstable.from_flags(flags, None, fd, fusion, minimum)                  # noqa: E731
    want = host_flags()
    assert table().lists() == want
    keep = tstable.from_flags(flags, None, fd, fusion, minimum)
    res["flags"] = dict(frames=n, segments_per_clip=sum(len(w) for w in want) / B, cap=keep.cap,
                        host=by_host(host_flags, R), table=by_host(table, R), lists=by_host(lambda: table().lists(), R),
                        kernel=by_events(lambda: tstable.from_flags(flags, None, fd, fusion, minimum, retry=False, storage=keep.storage),
                                         "vadx_timestamps_flags", R))

    # ---- frames
    S = 1000
    track = torch.from_numpy(np.repeat(rng.random((B, S // 40 + 1)) < 0.5, 40, axis=1)[:, :S].astype(np.float32) * 0.9 + 0.05).to(DEV)
    pp = vadpost.VadPostprocessor(5, 0.4, 20, 2000, 20, 5, 0, device=DEV)
    nf, durs = np.full(B, S, dtype=np.int64), [S * 0.01 + 0.02] * B
    host_frames = lambda: clips.track_segments(pp, track, nf, durs)[0]                     # noqa: E731
    table = lambda: clips.track_table(pp, track, nf, durs, 16000)[0]                       # noqa: E731
    want = host_frames()
    assert table().lists() == want
    _, segs, counts = pp.process_batch(track, n_frames=nf)
    keep = tstable.from_frames(pp, segs, counts, nf, durs)
    res["frames"] = dict(frames=S, segments_per_clip=sum(len(w) for w in want) / B, cap=keep.cap,
                         host=by_host(host_frames, R), table=by_host(table, R), lists=by_host(lambda: table().lists(), R),
                         kernel=by_events(lambda: tstable.from_frames(pp, segs, counts, nf, durs, retry=False, storage=keep.storage),
                                          "vadx_timestamps_frames", R),
                         vadpost=by_events(lambda: pp.process_batch(track, n_frames=nf, check=False), "vadx_vadpost", R))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
