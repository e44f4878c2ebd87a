"""Times of the ragged Silero path (get_speech_timestamps_batch on a vadx.ragged.RaggedClips) on the GPU, beside the rectangle.

    python tools/time_silero_ragged.py [--rate 16000 | 8000] [--out profiles/silero_ragged.json] [--clips 1024 4096] [--repeats 20]

--rate 8000 times the 8 kHz network (seeded 8 kHz weights, windows of 256 samples, the same durations in seconds) and writes
profiles/silero_ragged_8k.json unless --out says otherwise.

fp16 x 2 kernels, one process, float32 clips on the +-1 scale, every input resident on the device before the clock starts (host packing, the
tables and the upload are outside every timed region).  Per clip count three settings:
  (a) lengths drawn uniformly from 1 - 10 s (seeded): ragged timestamps against get_speech_timestamps_batch(rectangle, lengths=) -- the
      only batched path before the ragged one -- and, scores alone, clips_ragged against clips() on the rectangle;
  (b) the same lengths rounded up to whole seconds: the same four calls;
  (c) every clip 10 s: clips_ragged against clips() on the same audio -- how far the ragged path is behind where it is not needed;
  (d) call recordings: log-normal durations (median 30 s) cut to 1 - 120 s: the same four calls (above 8 GiB of workspace the rectangle runs
      span by span and the ragged batch in parts, as they would for a caller).
Then, for the largest clip count of (a), the price of part boundaries: clips_ragged on the batch in one part against the same batch under a
workspace cap lowered to an eighth of its workspace (`parts_*`).  A list that is above the cap as it stands is set (d) at 4096 clips
(its row says how many parts it ran in).
A call ends in a device synchronise.  Per row: warm-up, then `--repeats` timed calls, the variants of a row alternating call by call (ABAB);
reported are the median and the range (min, max) of the host clock in ms, the window counts both ways, and whether every clip's scores
and timestamps are the same both ways.  Nothing is gated on these numbers; they are recorded with the box they came from."""
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
from vadx import ragged, silero, weights  # noqa: E402


def bursts(rng, n):
    """float32 bursts on the +-1 scale: N(0, 3000) / N(0, 30) int16-level segments of 0.75 s"""
    loud = ((np.arange(n) // 12000 + int(rng.integers(0, 2))) % 2).astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * (30.0 + 2970.0 * loud)
    return np.clip(np.rint(x), -32768, 32767).astype(np.float32) * np.float32(0.000030517578)


def time_variants(variants, repeats, warmup=2):
    """{name: fn} -> {name: dict(median_ms, min_ms, max_ms, calls)}; the variants alternate call by call"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), calls=len(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=16000, choices=[16000, 8000])
    ap.add_argument("--out", default=None)
    ap.add_argument("--sets", default="abcd")
    ap.add_argument("--clips", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    rate = a.rate
    if a.out is None:
        a.out = "profiles/silero_ragged.json" if rate == 16000 else "profiles/silero_ragged_8k.json"
    dev = torch.device("cuda:0")
    eng = silero.SileroEngine(weights.silero_synthetic(1234), device=dev, weights_8k=weights.silero8k_synthetic(1234) if rate == 8000 else None)
    eng.arithmetic = "h2"
    rng = np.random.default_rng(a.seed)
    kw = dict(threshold=0.5, min_speech_duration_ms=250, min_silence_duration_ms=100, sampling_rate=rate)
    made = {}

    def row(lengths, name, timestamps):
        clips = [bursts(rng, int(n)) for n in lengths]
        rb = ragged.RaggedClips.from_clips(clips, device=dev, sampling_rate=rate)
        rect = torch.zeros((len(clips), int(max(lengths))), dtype=torch.float32, device=dev)
        for b, c in enumerate(clips):
            rect[b, :len(c)] = torch.from_numpy(c)
        lens = [int(n) for n in lengths]
        del clips
        variants = {"scores_ragged": lambda: eng.clips_ragged(rb), "scores_rectangle": lambda: eng.clips(rect, sampling_rate=rate)}
        if timestamps:
            variants["timestamps_ragged"] = lambda: silero.get_speech_timestamps_batch(rb, eng, **kw)
            variants["timestamps_rectangle"] = lambda: silero.get_speech_timestamps_batch(rect, eng, lengths=lens, **kw)
        res = time_variants(variants, a.repeats)
        # same results both ways (the rectangle masked per clip, as the lengths= path masks it)
        got, rows_ = silero.get_speech_timestamps_batch(rb, eng, return_probs=True, **kw)
        want, rprobs = silero.get_speech_timestamps_batch(rect, eng, lengths=lens, return_probs=True, **kw)
        same = got == want and all(torch.equal(r, rprobs[b, :r.shape[0]]) for b, r in enumerate(rows_))
        T = int(rb.windows.max())
        made[name] = rb
        out = dict(clips=len(rb), audio_seconds=float(rb.lengths.sum() / rate), parts=len(rb.parts(silero.WORKSPACE_CAP_BYTES)), windows_ragged=rb.tiles * 16, windows_rectangle=rb.groups * 16 * T,
                   window_ratio=rb.tiles / (rb.groups * T), workspace_mb_ragged=rb.workspace_bytes / 2 ** 20,
                   workspace_mb_rectangle=rb.groups * T * 32768 / 2 ** 20, same_results=bool(same), **res)
        out["scores_rectangle_over_ragged"] = res["scores_rectangle"]["median_ms"] / res["scores_ragged"]["median_ms"]
        if timestamps:
            out["timestamps_rectangle_over_ragged"] = res["timestamps_rectangle"]["median_ms"] / res["timestamps_ragged"]["median_ms"]
        print(json.dumps({name: out}), flush=True)
        del rect
        torch.cuda.empty_cache()
        return out

    def parts_row(rb, name):
        """the same batch in one part and under a cap of an eighth of its workspace (whole tiles, at least its longest group)"""
        cap0 = silero.WORKSPACE_CAP_BYTES
        low = max(int(rb.group_windows[0]), rb.tiles // 8) * 32768

        def capped():
            silero.WORKSPACE_CAP_BYTES = low
            try:
                return eng.clips_ragged(rb)
            finally:
                silero.WORKSPACE_CAP_BYTES = cap0
        whole = eng.clips_ragged(rb)[0].clone()
        same = torch.equal(capped()[0], whole)
        res = time_variants({"parts_one": lambda: eng.clips_ragged(rb), "parts_capped": capped}, a.repeats)
        out = dict(clips=len(rb), tiles=rb.tiles, n_parts_one=len(rb.parts(cap0)), n_parts_capped=len(rb.parts(low)), cap_mb=low / 2 ** 20,
                   workspace_mb=rb.workspace_bytes / 2 ** 20, same_results=bool(same), **res)
        out["capped_over_one"] = res["parts_capped"]["median_ms"] / res["parts_one"]["median_ms"]
        print(json.dumps({name: out}), flush=True)
        return out

    rows = {}
    for B in a.clips:
        lengths = rng.integers(rate, 10 * rate + 1, B)
        if "a" in a.sets:
            rows[f"a_uniform_lengths_{B}"] = row(lengths, f"a_uniform_lengths_{B}", True)
        if "b" in a.sets:
            rows[f"b_whole_seconds_{B}"] = row((lengths + rate - 1) // rate * rate, f"b_whole_seconds_{B}", True)
        if "c" in a.sets:
            rows[f"c_all_10s_{B}"] = row(np.full(B, 10 * rate), f"c_all_10s_{B}", False)
        if "d" in a.sets:
            calls = np.clip(np.exp(rng.normal(np.log(30.0), 0.8, B)), 1.0, 120.0)
            rows[f"d_call_recordings_{B}"] = row((calls * rate).astype(np.int64), f"d_call_recordings_{B}", True)
    big = f"a_uniform_lengths_{max(a.clips)}"
    if big in made:
        rows[f"parts_of_{big}"] = parts_row(made[big], f"parts_of_{big}")
    out = dict(device=torch.cuda.get_device_name(0), sampling_rate=rate, mode=eng.mode(rate), range_fallbacks=eng.range_fallbacks, repeats=a.repeats, seed=a.seed,
               note="ms per call: median and range of `repeats` synchronised calls after warm-up (host clock), the variants of a row alternating "
                    "call by call; float32 clips resident on the device, tables built before the clock starts; scores_* = clips_ragged / "
                    "clips() (encoder + LSTM + range-flag read), timestamps_* = get_speech_timestamps_batch on the RaggedClips / on the "
                    "rectangle with lengths= (mask, encoder, LSTM, segmenter, host lists)",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
