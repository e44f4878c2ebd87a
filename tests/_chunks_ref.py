"""A numpy restatement of the reference's collect_chunks / drop_chunks (Silero/modeling_modified/utils_vad.py:588-682), written from
their documented behaviour -- Python slices of one clip, concatenated -- and pinned to the reference's own output by
tests/test_chunks_cpu.py (tests/golden/chunks.npz).  Rows are (start, end) pairs in samples."""
import numpy as np


def collect(rows, wav):
    return np.concatenate([wav[int(s):int(e)] for s, e in rows] + [wav[:0]])


def drop(rows, wav):
    cur, out = 0, []
    for s, e in rows:
        out.append(wav[cur:int(s)])
        cur = int(e)
    return np.concatenate(out + [wav[cur:]])


def seconds_rows(rows, sampling_rate):
    """the reference's seconds -> samples: whole seconds (Python's round: half to even) times the rate"""
    return [(round(s) * sampling_rate, round(e) * sampling_rate) for s, e in rows]


def packed(mode, tables, clips, align=1):
    """What collect_chunks_batch / drop_chunks_batch must return for a batch: (packed, offsets [B+1], lengths [B]); every clip starts
    on a multiple of `align`, filler zeros."""
    parts = [(collect if mode == "collect" else drop)(rows, wav) for rows, wav in zip(tables, clips)]
    lengths = np.asarray([len(p) for p in parts], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum((lengths + align - 1) // align * align)]).astype(np.int64)
    out = np.zeros(int(offsets[-1]), dtype=clips[0].dtype)
    for b, p in enumerate(parts):
        out[offsets[b]:offsets[b] + len(p)] = p
    return out, offsets, lengths
