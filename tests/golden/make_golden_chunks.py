#!/usr/bin/env python
"""Generate tests/golden/chunks.npz by RUNNING THE REFERENCE'S OWN collect_chunks / drop_chunks / _seconds_to_samples_tss
(Silero/modeling_modified/utils_vad.py:588-691) in the build container, as make_golden_iterator.py does for VADIterator.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chunks.py

Every case is one short integer-ramp clip (sample value = its own index, int16 and float32) and one table of rows: sorted and disjoint,
touching, overlapping, unsorted, reversed, negative indices, indices past the end, empty pieces, an empty table, and seconds=True rows at
x.5 values (0.5, 1.5, 2.5: the reference rounds to whole seconds, half to even).  Stored per case: the clip length, the rows, whether they
are seconds and at which rate, and for each function the output (which on a ramp IS the list of source indices) or the name of the
exception it raised.  Only numbers and names are stored.  The GPU box never runs this."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refload as R                      # noqa: E402

# (name, clip length, rows, seconds?, sampling rate)
CASES = [
    ("sorted_disjoint", 100, [(3, 10), (20, 37), (50, 99)], False, 0),
    ("touching", 64, [(0, 8), (8, 16), (16, 17), (17, 64)], False, 0),
    ("overlapping", 50, [(5, 20), (10, 30), (25, 26)], False, 0),
    ("unsorted", 80, [(40, 60), (1, 9), (70, 75), (20, 30)], False, 0),
    ("reversed", 40, [(30, 10), (5, 6), (39, 0)], False, 0),
    ("negative", 60, [(-50, -40), (-10, 58), (-100, 3), (5, -1)], False, 0),
    ("past_end", 33, [(30, 1000), (40, 50), (0, 33), (32, 34)], False, 0),
    ("empty_pieces", 20, [(4, 4), (0, 0), (20, 20), (7, 9), (9, 9)], False, 0),
    ("whole", 17, [(0, 17)], False, 0),
    ("one_sample", 1, [(0, 1)], False, 0),
    ("empty_clip", 0, [(0, 5), (-3, 2)], False, 0),
    ("empty_table", 25, [], False, 0),
    ("seconds_half", 40, [(0.5, 1.5), (2.5, 3.49), (3.5, 4.5)], True, 8),
    ("seconds_whole", 64, [(0.0, 1.0), (2.2, 2.9), (3.0, 7.6)], True, 10),
    ("seconds_no_rate", 30, [(0.0, 1.0)], True, 0),
]


def main():
    ns = {"torch": torch, "List": __import__("typing").List}
    R.select_nodes("Silero/modeling_modified/utils_vad.py", {"collect_chunks", "drop_chunks", "_seconds_to_samples_tss"}, ns)
    out = {"names": np.array([c[0] for c in CASES])}
    for name, n, rows, seconds, sr in CASES:
        tss = [{"start": s, "end": e} for s, e in rows]
        out[f"{name}_len"] = np.array(n, dtype=np.int64)
        out[f"{name}_rows"] = np.asarray(rows, dtype=np.float64 if seconds else np.int64).reshape(-1, 2)
        out[f"{name}_seconds"] = np.array([int(seconds), sr], dtype=np.int64)
        if seconds and sr:
            conv = ns["_seconds_to_samples_tss"](tss, sr)
            out[f"{name}_samples"] = np.asarray([(d["start"], d["end"]) for d in conv], dtype=np.int64).reshape(-1, 2)
        for fn in ("collect_chunks", "drop_chunks"):
            for dt, tag in ((torch.int16, "i16"), (torch.float32, "f32")):
                wav = torch.arange(n, dtype=dt)
                try:
                    got = ns[fn](tss, wav, seconds=seconds, sampling_rate=sr or None) if seconds else ns[fn](tss, wav)
                    assert got.dtype == dt and got.dim() == 1
                    out[f"{name}_{fn}_{tag}"] = got.numpy()
                    err = ""
                except Exception as e:          # noqa: BLE001  (the kind of error is the recorded result)
                    err = type(e).__name__
                out[f"{name}_{fn}_{tag}_error"] = np.array(err)
    path = os.path.join(HERE, "chunks.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote chunks.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(CASES)} cases)")


if __name__ == "__main__":
    main()
