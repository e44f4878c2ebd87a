"""CPU: the host side of vadx.chunks (the batched collect_chunks / drop_chunks, Silero/modeling_modified/utils_vad.py:588-682).
tests/golden/chunks.npz holds what the reference's own functions return on integer-ramp clips (tests/golden/make_golden_chunks.py); the
numpy restatement the GPU tests compare with (tests/_chunks_ref.py) and the host mirror of the device plan (chunks.plan_host) are pinned to
it here, and every argument check of the three C entry points is shown to answer before any device call (there is no GPU here: a HIP
call would come back as another code)."""
import ctypes as C

import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import _lib, build, chunks

import _chunks_ref as ref


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


@pytest.fixture(scope="module")
def cases(golden):
    g = golden("chunks")
    out = []
    for name in g["names"].tolist():
        seconds, sr = g[f"{name}_seconds"].tolist()
        out.append(dict(name=name, n=int(g[f"{name}_len"]), rows=[tuple(r) for r in g[f"{name}_rows"].tolist()], seconds=bool(seconds), sr=int(sr),
                        samples=[tuple(r) for r in g[f"{name}_samples"].tolist()] if f"{name}_samples" in g else None,
                        want={(fn, tag): (g[f"{name}_{fn}_chunks_{tag}"] if f"{name}_{fn}_chunks_{tag}" in g else None,
                                          str(g[f"{name}_{fn}_chunks_{tag}_error"]))
                              for fn in ("collect", "drop") for tag in ("i16", "f32")}))
    return out


def _sample_rows(c):
    """the rows of a case in samples (the reference's own conversion for a seconds=True case), or None when the case is an error case"""
    if not c["seconds"]:
        return [(int(s), int(e)) for s, e in c["rows"]]
    return c["samples"]


def test_fixture_covers_what_it_should(cases):
    names = {c["name"] for c in cases}
    assert {"sorted_disjoint", "touching", "overlapping", "unsorted", "reversed", "negative", "past_end", "empty_pieces", "empty_table",
            "seconds_half", "seconds_no_rate"} <= names
    by = {c["name"]: c for c in cases}
    assert by["empty_table"]["want"][("collect", "i16")][1] == "ValueError" and by["empty_table"]["want"][("drop", "i16")][1] == ""
    assert all(err == "ValueError" for _, err in by["seconds_no_rate"]["want"].values())
    assert by["seconds_half"]["samples"] == [(0, 16), (16, 24), (32, 32)]          # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 4.5 -> 4


def test_numpy_restatement_equals_the_reference(cases):
    seen = 0
    for c in cases:
        rows = _sample_rows(c)
        if c["seconds"] and c["sr"]:
            assert ref.seconds_rows(c["rows"], c["sr"]) == rows, c["name"]
        for (fn, tag), (want, err) in c["want"].items():
            if err:
                continue
            wav = np.arange(c["n"], dtype=np.int16 if tag == "i16" else np.float32)
            got = (ref.collect if fn == "collect" else ref.drop)(rows, wav)
            assert got.dtype == want.dtype and np.array_equal(got, want), (c["name"], fn, tag)
            seen += 1
    assert seen >= 50


def test_plan_host_equals_the_reference(cases):
    """On a ramp the reference's output IS the list of source indices: the pieces of plan_host, laid end to end, must give it, and the
    plan's lengths and prefixes must agree with them -- for every case alone and for all of them as one batch, at every alignment."""
    ok = [c for c in cases if _sample_rows(c) is not None and c["name"] != "seconds_no_rate"]
    for mode in ("collect", "drop"):
        tables = [_sample_rows(c) for c in ok]
        segs, counts = chunks.table_of(tables)
        lens = np.asarray([c["n"] for c in ok])
        for align in (1, 8, 64):
            p = chunks.plan_host(segs, counts, lens, mode, align)
            assert p["status"] == 0 and p["clip_dst"][0] == 0 and p["total"] == p["clip_dst"][-1]
            assert np.array_equal(p["clip_dst"][1:] - p["clip_dst"][:-1], (p["lengths"] + align - 1) // align * align)
            for b, c in enumerate(ok):
                want, err = c["want"][(mode, "i16")]
                if err:                                   # collect of an empty table: the plan itself is simply empty
                    assert c["name"] == "empty_table" and p["n_pieces"][b] == 0 and p["lengths"][b] == 0
                    continue
                n = p["n_pieces"][b]
                assert n == len(tables[b]) + (mode == "drop")
                idx = np.concatenate([np.arange(lo, hi) for lo, hi in p["piece_src"][b, :n].tolist()] + [np.zeros(0, np.int64)])
                assert np.array_equal(idx, want.astype(np.int64)), (c["name"], mode)
                assert p["lengths"][b] == len(want)
                sizes = p["piece_src"][b, :n, 1] - p["piece_src"][b, :n, 0]
                assert np.array_equal(p["piece_dst"][b, :n], np.cumsum(sizes) - sizes) and np.all(p["piece_dst"][b, n:] == len(want))
                alone = chunks.plan_host(segs[b:b + 1], counts[b:b + 1], lens[b:b + 1], mode, align)
                assert np.array_equal(alone["piece_src"][0], p["piece_src"][b]) and alone["lengths"][0] == p["lengths"][b]
    bad = chunks.plan_host(np.zeros((3, 2, 2), np.int64), [3, -1, 1], [5, 5, -1], "collect")
    assert bad["status"] == chunks.ST_BAD_CLIP and bad["n_pieces"].tolist() == [-1, -1, -1] and bad["total"] == 0


def test_packed_reference_layout():
    clips = [np.arange(10, dtype=np.int16), np.arange(3, dtype=np.int16), np.arange(0, dtype=np.int16)]
    out, offsets, lengths = ref.packed("collect", [[(1, 4)], [(0, 3)], []], clips, align=8)
    assert offsets.tolist() == [0, 8, 16, 16] and lengths.tolist() == [3, 3, 0]
    assert out.tolist() == [1, 2, 3, 0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0]


def test_from_seconds_is_the_nearest_sample():
    assert chunks.from_seconds([[(0.25, 1.0), {"start": 0.00003, "end": 2.49997}], []], 16000) == [[(4000, 16000), (0, 40000)], []]


def test_layout_is_the_librarys(lib):
    for batch, cap in ((1, 1), (3, 64), (70000, 5), (2, 130)):
        assert lib.vadx_chunks_plan_bytes(batch, cap) == chunks.plan_layout(batch, cap)["bytes"]
    assert lib.vadx_chunks_plan_bytes(0, 4) == 0 and lib.vadx_chunks_plan_bytes(4, 0) == 0


def test_entry_points_validate_before_touching_the_device(lib):
    """Every VADX_EINVAL of vadx_chunks_plan / vadx_chunks_copy names its argument and comes back before any HIP call."""
    buf = (C.c_char * 8192)()
    base = C.addressof(buf)
    ptr = (base + 15) // 16 * 16                    # 16-byte aligned host memory: never dereferenced
    need = lib.vadx_chunks_plan_bytes(2, 3)
    assert 0 < need <= 4096

    def plan(segs=ptr, counts=ptr, lens=ptr, batch=2, cap=3, mode=chunks.COLLECT, align=8, rec=ptr, nbytes=need):
        return lib.vadx_chunks_plan(segs, counts, lens, batch, cap, mode, align, rec, nbytes, None)

    def copy(src=ptr, src_elems=100, clip_src=ptr, elem_bytes=2, rec=ptr, nbytes=need, batch=2, cap=3, dst=ptr, dst_elems=100):
        return lib.vadx_chunks_copy(src, src_elems, clip_src, elem_bytes, rec, nbytes, batch, cap, dst, dst_elems, None)

    refused = [(plan, dict(segs=None), b"segments"), (plan, dict(counts=None), b"counts"), (plan, dict(lens=None), b"clip_len"),
               (plan, dict(rec=None), b"plan"), (plan, dict(batch=0), b"batch=0"), (plan, dict(cap=0), b"cap=0"), (plan, dict(cap=-1), b"cap=-1"),
               (plan, dict(mode=2), b"mode=2"), (plan, dict(mode=-1), b"mode=-1"),
               (plan, dict(align=0), b"align=0"), (plan, dict(align=3), b"align=3"), (plan, dict(align=8192), b"align=8192"), (plan, dict(align=-8), b"align=-8"),
               (plan, dict(nbytes=need - 1), b"plan_bytes"), (plan, dict(rec=ptr + 8), b"16-byte"),
               (copy, dict(src=None), b"src"), (copy, dict(clip_src=None), b"clip_src"), (copy, dict(rec=None), b"plan"), (copy, dict(dst=None), b"dst"),
               (copy, dict(batch=0), b"batch=0"), (copy, dict(cap=0), b"cap=0"),
               (copy, dict(elem_bytes=1), b"elem_bytes=1"), (copy, dict(elem_bytes=8), b"elem_bytes=8"), (copy, dict(elem_bytes=3), b"elem_bytes=3"),
               (copy, dict(src=ptr + 2), b"src must be 16-byte aligned"), (copy, dict(dst=ptr + 8), b"dst must be 16-byte aligned"),
               (copy, dict(src_elems=-1), b"src_elems=-1"), (copy, dict(dst_elems=-1), b"dst_elems=-1"),
               (copy, dict(nbytes=need - 16), b"plan_bytes"),
               (copy, dict(dst_elems=(1 << 31) * 8192), b"2^31"), (copy, dict(elem_bytes=4, dst_elems=(1 << 31) * 4096), b"2^31")]
    for fn, kw, word in refused:
        assert fn(**kw) == -1, kw
        msg = lib.vadx_last_error()
        assert msg.startswith(b"vadx_chunks_plan: " if fn is plan else b"vadx_chunks_copy: ") and word in msg, (kw, msg)
    for align in (1, 2, 64, 4096):                  # and the python side refuses the same alignments
        assert chunks._check_align(align) == align
    for align in (0, 3, 8192):
        with pytest.raises(ValueError):
            chunks._check_align(align)


def test_python_argument_errors_need_no_device():
    with pytest.raises(ValueError, match="sampling_rate must be provided"):
        chunks.collect_chunks([{"start": 0, "end": 1}], None, seconds=True)
    with pytest.raises(ValueError, match="sampling_rate must be provided"):
        chunks.drop_chunks([{"start": 0, "end": 1}], None, seconds=True)
    with pytest.raises(ValueError, match="smaller than the longest list"):
        chunks.table_of([[(0, 1), (2, 3)]], cap=1)
    segs, counts = chunks.table_of([[], [{"start": 1, "end": 2}, (3, 4)]])
    assert segs.shape == (2, 2, 2) and counts.tolist() == [0, 2] and segs[1].tolist() == [[1, 2], [3, 4]]
    from vadx import silero
    assert silero.collect_chunks is chunks.collect_chunks and silero.drop_chunks is chunks.drop_chunks
