"""Host time of the whole-clip `detect` of FsmnEngine, FireRedEngine and MarbleNetEngine (dynamic axis), for comparing two trees.

    python tools/time_detect.py --out detect_branch_1.json                     one process: six rows, written as JSON
    python tools/time_detect.py --first PARENT.json... --second BRANCH.json...  the table kept in profiles/detect_host.txt

The kernels are the library's; what this times is everything `detect` does around them: padding / packing on the host, the upload, the
launch sequence, one read-back (which synchronises) and the seconds arithmetic per clip.  Per engine two rows: a LIST of 64 seeded
clips of 1 - 10 s (the ragged route) and a rectangular [32, 160 000] batch.  A row is warmed up twice, then timed `--repeats` (9) times
with the host clock around `detect`; the padding noise is given, so every call does the same work.  The script imports the `vadx` of
the tree it lies in, so a copy of it inside another checkout times that checkout.

--first / --second pools the runs of each side over its files (rounds) and accepts a row when the second side's median is no larger
than the first side's median plus the first side's own min - max spread: the only noise figure such a comparison has."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROWS = ("fsmn list", "fsmn [32, 160000]", "firered list", "firered [32, 160000]", "marblenet list", "marblenet [32, 160000]")


def measure(repeats, seed):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import vadx  # noqa: F401
    from vadx import firered, fsmn, marblenet, weights
    rng = np.random.default_rng(seed)
    lengths = rng.integers(16000, 160001, 64)
    clips = [weights.burst_clips(1, int(n), seed=seed + 1 + k)[0] for k, n in enumerate(lengths)]
    rect = weights.burst_clips(32, 160000, seed=seed + 100)
    noise = rng.standard_normal((64, 20000))
    engines = {"fsmn": fsmn.FsmnEngine(weights.fsmn_synthetic(1234)), "firered": firered.FireRedEngine(weights.firered_synthetic(1234)),
               "marblenet": marblenet.MarbleNetEngine(weights.marblenet_synthetic(1234))}
    rows = {}
    for name, eng in engines.items():
        for form, audio, nz in (("list", clips, noise), ("[32, 160000]", rect, noise[:32])):
            for _ in range(2):
                eng.detect(audio, pad_noise=nz)
            torch.cuda.synchronize()
            ms = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                eng.detect(audio, pad_noise=nz)
                ms.append((time.perf_counter() - t0) * 1e3)
            rows[f"{name} {form}"] = ms
            print(f"{name} {form}: median {statistics.median(ms):.3f} ms, {min(ms):.3f} - {max(ms):.3f}", flush=True)
    return dict(device=torch.cuda.get_device_name(0), repeats=repeats, seed=seed, audio_seconds_list=float(lengths.sum() / 16000), ms=rows)


def compare(first, second):
    def pooled(files, row):
        return [v for f in files for v in json.load(open(f))["ms"][row]]
    ok = True
    print(f"{'row':26s} {'first: median (min - max) ms':>34s} {'second: median (min - max) ms':>34s}   bound = first median + spread")
    for row in ROWS:
        a, b = pooled(first, row), pooled(second, row)
        bound = statistics.median(a) + (max(a) - min(a))
        good = statistics.median(b) <= bound
        ok = ok and good
        print(f"{row:26s} {statistics.median(a):12.3f} ({min(a):8.3f} - {max(a):8.3f}) {statistics.median(b):12.3f} ({min(b):8.3f} - {max(b):8.3f})"
              f"   {bound:9.3f}  {'ok' if good else 'SLOWER'}")
    print(f"{len(first)} + {len(second)} rounds; {'every row within the bound' if ok else 'a row exceeds its bound'}")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--first", nargs="+", metavar="JSON")
    ap.add_argument("--second", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.first or a.second:
        sys.exit(0 if compare(a.first, a.second) else 1)
    res = measure(a.repeats, a.seed)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
