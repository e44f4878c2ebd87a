#!/usr/bin/env python
"""Generate tests/golden/silero_iterator.npz by RUNNING THE REFERENCE'S OWN VADIterator (Silero/modeling_modified/utils_vad.py:494-586)
in the build container, as make_golden.py does for the other fixtures.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_iterator.py

(a) replay tracks: the iterator over a stand-in model that replays scripted scores (the four kinds gen_silero_host uses, plus scores
    exactly at threshold and threshold - 0.15), four parameter sets, one reset_states() mid-track; every call's result in samples and in
    seconds (time_resolution 1 and 3).
(b) the iterator over the reference OnnxWrapper whose session is the oracle network on weights.silero_synthetic(1234), fed two
    burst_clips recordings window by window: per-call scores and events, the wrapper's final _state / _context.
Only numbers are stored.  The GPU box never runs this."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import _refload as R                      # noqa: E402
import vadx                               # noqa: E402,F401
from vadx import weights                  # noqa: E402
from oracle import mel as omel            # noqa: E402
from oracle import silero as osil         # noqa: E402

R.install_stubs(omel.melscale_fbanks)
torch.set_num_threads(4)

PARAMS = [dict(threshold=0.5, min_silence_duration_ms=100, speech_pad_ms=30),
          dict(threshold=0.6, min_silence_duration_ms=250, speech_pad_ms=30),
          dict(threshold=0.5, min_silence_duration_ms=100, speech_pad_ms=0),
          dict(threshold=0.5, min_silence_duration_ms=100, speech_pad_ms=30.03)]


class Replay:
    def __init__(self, probs):
        self.probs, self.i = probs, 0

    def reset_states(self):
        pass

    def __call__(self, chunk, sr):
        assert chunk.shape[-1] == 512 and sr == 16000
        v = self.probs[self.i]
        self.i += 1
        return torch.tensor([[v]], dtype=torch.float32)


def track(rng, kind, n, thr):
    if kind == 0:
        p = rng.uniform(0, 1, n)
    elif kind == 1:
        p = np.zeros(n)
        pos, hot = 0, True
        while pos < n:
            seg = int(rng.integers(3, 40))
            p[pos:pos + seg] = rng.uniform(thr, 1.0, min(seg, n - pos)) if hot else rng.uniform(0, thr - 0.15, min(seg, n - pos))
            pos += seg
            hot = not hot
    elif kind == 2:
        p = rng.uniform(thr + 0.05, 1.0, n)
        for _ in range(max(1, n // 30)):
            a = int(rng.integers(0, n))
            p[a:a + int(rng.integers(2, 12))] = rng.uniform(0.0, 0.3)
    else:
        p = np.clip(thr - 0.05 + 0.35 * np.sin(np.arange(n) / 7.0) + 0.1 * rng.standard_normal(n), 0, 1)
    p = p.astype(np.float32)
    # scores exactly at the two thresholds (as float32: thr - 0.15 rounds to either side of the double) and their neighbours
    edge = np.array([thr, thr - 0.15], dtype=np.float32)
    p[int(rng.integers(0, n - 6)):][:6] = edge[1]               # a run at thr - 0.15
    spots = rng.choice(n, 6, replace=False)
    for j, (e, d) in enumerate([(e, d) for e in edge for d in (0, 1, -1)]):
        p[spots[j]] = e if d == 0 else np.nextafter(e, np.float32(d))
    return p


def gen_replay(ns, out):
    rng = np.random.default_rng(77)
    it = 0
    for pi, prm in enumerate(PARAMS):
        for kind in range(4):
            n = int(rng.integers(150, 400))
            p = track(rng, kind, n, prm["threshold"])
            reset_at = n // 2 if (pi, kind) == (1, 2) else -1
            res = {}
            for tag, kw in (("samples", dict()), ("s1", dict(return_seconds=True, time_resolution=1)),
                            ("s3", dict(return_seconds=True, time_resolution=3))):
                vi = ns["VADIterator"](Replay([float(v) for v in p]), sampling_rate=16000, **prm)
                kinds, vals = np.zeros(n, np.int8), np.full(n, np.nan)
                for i in range(n):
                    if i == reset_at:
                        vi.reset_states()
                    r = vi(torch.zeros(512), **kw)
                    if r is not None:
                        kinds[i] = 1 if "start" in r else 2
                        vals[i] = r.get("start", r.get("end"))
                res[tag] = (kinds, vals)
            assert np.array_equal(res["samples"][0], res["s1"][0]) and np.array_equal(res["samples"][0], res["s3"][0])
            out[f"a{it}_probs"] = p
            out[f"a{it}_params"] = np.array([prm["threshold"], prm["min_silence_duration_ms"], prm["speech_pad_ms"]])
            out[f"a{it}_reset_at"] = np.array(reset_at)
            out[f"a{it}_kind"] = res["samples"][0]
            for tag in ("samples", "s1", "s3"):
                out[f"a{it}_{tag}"] = res[tag][1]
            it += 1
    out["a_tracks"] = np.array(it)


def gen_onnx(ns, out):
    w = {k: torch.from_numpy(v) for k, v in weights.silero_synthetic(1234).items()}

    class FakeSession:
        def __init__(self):
            self.outs = []

        def run(self, _names, feeds):
            assert int(feeds["sr"]) == 16000
            o, s = osil.net_forward(w, torch.from_numpy(feeds["input"]), torch.from_numpy(feeds["state"]))
            self.outs.append(float(o.reshape(-1)[0]))
            return [o.numpy(), s.numpy()]

    ns["np"] = np
    audio = weights.burst_clips(2, 150 * 512, seed=19).astype(np.float32) * np.float32(0.000030517578)
    out["b_audio"] = audio
    for c in range(2):
        wrapper = ns["OnnxWrapper"].__new__(ns["OnnxWrapper"])
        wrapper.session = FakeSession()
        wrapper.sample_rates = [16000]
        wrapper.reset_states()
        vi = ns["VADIterator"](wrapper)
        kinds, vals = np.zeros(150, np.int8), np.full(150, np.nan)
        for i in range(150):
            r = vi(torch.from_numpy(audio[c, i * 512:(i + 1) * 512].copy()))
            if r is not None:
                kinds[i] = 1 if "start" in r else 2
                vals[i] = r.get("start", r.get("end"))
        out[f"b{c}_probs"] = np.array(wrapper.session.outs, dtype=np.float32)
        out[f"b{c}_kind"] = kinds
        out[f"b{c}_samples"] = vals
        out[f"b{c}_state"] = wrapper._state.numpy()
        out[f"b{c}_context"] = wrapper._context.numpy()
        print(f"  clip {c}: {int((kinds == 1).sum())} starts, {int((kinds == 2).sum())} ends")


if __name__ == "__main__":
    ns = {"torch": torch, "warnings": __import__("warnings"), "Callable": __import__("typing").Callable,
          "List": __import__("typing").List}
    R.select_nodes("Silero/modeling_modified/utils_vad.py", {"VADIterator", "OnnxWrapper"}, ns)
    out = {}
    gen_replay(ns, out)
    gen_onnx(ns, out)
    path = os.path.join(HERE, "silero_iterator.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote silero_iterator.npz ({os.path.getsize(path) / 1024:.1f} KiB)")
