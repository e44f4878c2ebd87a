"""Silero's ragged batch on the host (vadx.ragged.RaggedClips._set_tables): every table is a function of the clips' lengths, written once
in numpy.  Checked here without a GPU: the workgroup table covers every (clip, window) exactly once, the groups are sorted, the prefixes
are prefixes, the workspace is sum(T_g) tiles, and the host refusals hold."""
import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import ragged

WIN, GROUP, RUN = 512, 16, 4

# the length set of tests/test_gpu_silero_ragged.py, test 1: one group that mixes T_b = 33 ... 1, one full group of T_b = 1, a partial one
MIXED = [512 * 33 - 100, 512 * 32, 512 * 30 + 1, 512 * 17 - 100, 512 * 16, 512 * 14 + 1, 512 * 9 - 100, 512 * 8, 512 * 4 + 1, 512 * 4 - 100,
         512 * 3, 513, 575, 576, 577, 511]
SHORT = [1, 3, 4, 63, 64, 65, 511, 412, 512]
LENGTHS_37 = MIXED + [SHORT[k % len(SHORT)] for k in range(21)]


def tables(lengths, align=8):
    lengths = np.asarray(lengths, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum((lengths + align - 1) // align * align)])[:-1]
    r = ragged.RaggedClips()
    r._set_tables(lengths, starts)
    return r, starts


def check(r, lengths, starts):
    lengths = np.asarray(lengths, dtype=np.int64)
    B = len(lengths)
    T = (lengths + WIN - 1) // WIN
    G = (B + GROUP - 1) // GROUP
    assert r.groups == G and len(r) == B
    # slots: a permutation of the clips, -1 behind the last clip of a partial group, sorted by window count (descending, stable)
    clip = r.slot_clip_host
    assert clip.shape == (G * GROUP,) and sorted(clip[:B].tolist()) == list(range(B)) and (clip[B:] == -1).all()
    ts = T[clip[:B]]
    assert (np.diff(ts) <= 0).all()
    for a, b in zip(clip[:B - 1], clip[1:B]):
        assert T[a] > T[b] or a < b                       # stable
    assert np.array_equal(r.slot_len_host[:B], lengths[clip[:B]]) and (r.slot_len_host[B:] == 0).all()
    assert np.array_equal(r.slot_off_host[:B], starts[clip[:B]]) and (r.slot_off_host[B:] == 0).all()
    # groups
    Tg = ts[::GROUP]
    assert np.array_equal(r.group_windows, Tg)
    assert r.gx_first_host.dtype == np.int32 and np.array_equal(r.gx_first_host, np.concatenate([[0], np.cumsum(Tg)]))
    assert r.tiles == int(Tg.sum()) and r.workspace_bytes == int(Tg.sum()) * 32768
    for g in range(G):
        sl = r.slot_len_host[g * GROUP:(g + 1) * GROUP]
        assert r.grp_min_len_host[g] == (sl.min() if (clip[g * GROUP:(g + 1) * GROUP] >= 0).all() else 0)
    # scores
    assert r.probs_first_host.dtype == np.int64 and np.array_equal(r.probs_first_host, np.concatenate([[0], np.cumsum(T)]))
    assert r.n_windows == int(T.sum())
    # the workgroup table: run-major, every (group, window) once -- and so every (clip, window) once, in its group's tile
    tab = r.wg_tab_host
    assert tab.dtype == np.int32 and tab.shape == (r.n_runs, 2)
    assert (np.diff(tab[:, 1]) >= 0).all()
    seen = np.zeros(r.tiles, dtype=np.int64)
    cover = np.zeros(r.n_windows, dtype=np.int64)
    for g, run in tab.tolist():
        assert 0 <= g < G and run * RUN < Tg[g]
        for t in range(run * RUN, min(run * RUN + RUN, Tg[g])):
            seen[r.gx_first_host[g] + t] += 1
            for s in range(g * GROUP, (g + 1) * GROUP):
                if clip[s] >= 0 and t < T[clip[s]]:
                    cover[r.probs_first_host[clip[s]] + t] += 1
    assert (seen == 1).all() and (cover == 1).all()
    for k in range(1, len(tab)):                          # within a run: groups in ascending order
        assert tab[k, 1] > tab[k - 1, 1] or tab[k, 0] == tab[k - 1, 0] + 1


def test_tables_of_the_gpu_test_set():
    assert len(LENGTHS_37) == 37
    r, starts = tables(LENGTHS_37)
    check(r, LENGTHS_37, starts)
    assert r.group_windows.tolist() == [33, 1, 1]
    assert sorted(set(((np.asarray(LENGTHS_37) + WIN - 1) // WIN).tolist())) == [1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33]
    assert r.grp_min_len_host.tolist()[0] == 511 and r.grp_min_len_host[2] == 0


@pytest.mark.parametrize("seed", range(6))
def test_tables_of_random_length_sets(seed):
    rng = np.random.default_rng(seed)
    B = int(rng.integers(1, 90))
    lengths = rng.integers(1, 512 * int(rng.integers(1, 40)) + 1, size=B)
    r, starts = tables(lengths, align=int(rng.integers(1, 9)))
    check(r, lengths, starts)


def test_window_ratio_of_the_timed_distribution():
    """4096 lengths uniform in 1 - 10 s: the ragged path encodes sum(T_g) of the rectangle's G * T_max windows (the value is in README)."""
    lengths = np.random.default_rng(2024).integers(16000, 160001, size=4096)
    r, _ = tables(lengths)
    ratio = r.tiles / (r.groups * int(r.windows.max()))
    print(f"sum T_g / (G T_max) = {ratio:.4f}")
    assert ratio < 1


def test_run_constant_matches_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vadx.h")).read()
    assert int(re.search(r"#define\s+VADX_SILERO_RAGGED_RUN\s+(\d+)", hdr).group(1)) == ragged.SILERO_RUN == RUN
    src = open(os.path.join(os.path.dirname(os.path.abspath(ragged.__file__)), "csrc", "silero_h2.hip")).read()
    assert int(re.search(r"constexpr int H2_NSUB = (\d+);", src).group(1)) == RUN


def test_host_refusals():
    with pytest.raises(ValueError, match="at least one clip"):
        ragged.RaggedClips.from_clips([], device=None)
    with pytest.raises(ValueError, match="clip 1 is empty"):
        ragged.RaggedClips.from_clips([np.zeros(5, np.float32), np.zeros(0, np.float32)], device=None)
    with pytest.raises(ValueError, match="dtype"):
        ragged.RaggedClips.from_clips([np.zeros(5, np.float64)], device=None)
    with pytest.raises(ValueError, match="dtype"):
        ragged.RaggedClips.from_clips([np.zeros(5, np.float32), np.zeros(5, np.int16)], device=None)
    r = ragged.RaggedClips()
    with pytest.raises(ValueError, match="is empty"):
        r._set_tables([5, 0], [0, 8])
    with pytest.raises(ValueError, match="2\\^31"):
        r._set_tables([2 ** 31], [0])
    with pytest.raises(ValueError, match="do not fit the int32"):          # 2^31 tiles: 2^20 groups of 2^11 windows
        r._set_tables(np.full(2 ** 24, 512 * 2 ** 11, dtype=np.int64), np.zeros(2 ** 24, dtype=np.int64))


def test_from_clips_packs_on_the_alignment():
    a, b, c = np.arange(5, dtype=np.int16), np.arange(9, dtype=np.int16) + 100, np.arange(3, dtype=np.int16) + 50
    r = ragged.RaggedClips.from_clips([a, b, c], device=None)
    assert r.clip_off.tolist() == [0, 8, 24] and r.pcm_host.shape == (32,)
    assert np.array_equal(r.pcm_host[8:17], b) and r.pcm_host[5:8].tolist() == [0, 0, 0]
    r = ragged.RaggedClips.from_clips([a, b, c], device=None, align=1)
    assert r.clip_off.tolist() == [0, 5, 14] and np.array_equal(r.pcm_host, np.concatenate([a, b, c]))
