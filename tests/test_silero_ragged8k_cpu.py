"""Silero's ragged batch on the host at either rate (vadx.ragged.RaggedClips._set_tables, .parts): the tables of the 8 kHz network count
windows of 256 samples and are otherwise the 16 kHz ones; a batch above a workspace cap is cut into runs of whole groups.  Checked here
without a GPU: at window 256 the workgroup table covers every (clip, window) exactly once, the sort is stable, the prefixes are prefixes
and the workspace is sum(T_g) tiles; at 16000 the keyword changes no byte of any table; `parts` covers every group once, in order, under
the cap, and refuses a group that does not fit by the cap's name."""
import numpy as np
import pytest

import vadx  # noqa: F401
from vadx import ragged
from test_silero_ragged_cpu import LENGTHS_37

GROUP, RUN, TILE = 16, 4, 32768

# the 8 kHz image of LENGTHS_37 (tests/test_gpu_silero_ragged8k.py runs it): one group that mixes T_b = 33 ... 1 with lengths
# 256 k - 50 / 256 k / 256 k + 1 in turn and 257, 287, 288, 289, 255 around the reflect pad and the window edge; one full group of
# one-window clips around the vector-load minimum and the 32-sample context; a partial group
MIXED8K = [256 * 33 - 50, 256 * 32, 256 * 30 + 1, 256 * 17 - 50, 256 * 16, 256 * 14 + 1, 256 * 9 - 50, 256 * 8, 256 * 4 + 1, 256 * 4 - 50,
           256 * 3, 257, 287, 288, 289, 255]
SHORT8K = [1, 3, 4, 31, 32, 33, 255, 206, 256]
LENGTHS8K_37 = MIXED8K + [SHORT8K[k % len(SHORT8K)] for k in range(21)]


def tables(lengths, align=8, **kw):
    lengths = np.asarray(lengths, dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum((lengths + align - 1) // align * align)])[:-1]
    r = ragged.RaggedClips()
    r._set_tables(lengths, starts, **kw)
    return r, starts


def check(r, lengths, starts, win):
    lengths = np.asarray(lengths, dtype=np.int64)
    B = len(lengths)
    T = (lengths + win - 1) // win
    G = (B + GROUP - 1) // GROUP
    assert r.groups == G and len(r) == B and r.window == win and r.sampling_rate == {512: 16000, 256: 8000}[win]
    clip = r.slot_clip_host
    assert clip.shape == (G * GROUP,) and sorted(clip[:B].tolist()) == list(range(B)) and (clip[B:] == -1).all()
    ts = T[clip[:B]]
    assert (np.diff(ts) <= 0).all()
    for a, b in zip(clip[:B - 1], clip[1:B]):
        assert T[a] > T[b] or a < b                       # stable
    assert np.array_equal(r.slot_len_host[:B], lengths[clip[:B]]) and (r.slot_len_host[B:] == 0).all()
    assert np.array_equal(r.slot_off_host[:B], starts[clip[:B]]) and (r.slot_off_host[B:] == 0).all()
    Tg = ts[::GROUP]
    assert np.array_equal(r.group_windows, Tg)
    assert r.gx_first_host.dtype == np.int32 and np.array_equal(r.gx_first_host, np.concatenate([[0], np.cumsum(Tg)]))
    assert r.tiles == int(Tg.sum()) and r.workspace_bytes == int(Tg.sum()) * TILE
    for g in range(G):
        sl = r.slot_len_host[g * GROUP:(g + 1) * GROUP]
        assert r.grp_min_len_host[g] == (sl.min() if (clip[g * GROUP:(g + 1) * GROUP] >= 0).all() else 0)
    assert r.probs_first_host.dtype == np.int64 and np.array_equal(r.probs_first_host, np.concatenate([[0], np.cumsum(T)]))
    assert r.n_windows == int(T.sum())
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


def test_the_37_lengths_at_8_khz():
    assert len(LENGTHS8K_37) == 37
    r, starts = tables(LENGTHS8K_37, sampling_rate=8000)
    check(r, LENGTHS8K_37, starts, 256)
    assert r.group_windows.tolist() == [33, 1, 1]
    assert r.windows[:16].tolist() == [33, 32, 31, 17, 16, 15, 9, 8, 5, 4, 3, 2, 2, 2, 2, 1]
    assert r.windows.tolist() == ((np.asarray(LENGTHS_37) + 511) // 512).tolist()          # the image: the 16 kHz set's window counts
    assert r.grp_min_len_host.tolist()[0] == 255 and r.grp_min_len_host[2] == 0
    assert {257, 287, 288, 289, 255} <= set(LENGTHS8K_37[:16]) and {1, 3, 4, 31, 32, 33, 255, 206, 256} <= set(LENGTHS8K_37[16:32])


@pytest.mark.parametrize("seed", range(6))
def test_random_length_sets_at_8_khz(seed):
    rng = np.random.default_rng(100 + seed)
    B = int(rng.integers(1, 90))
    lengths = rng.integers(1, 256 * int(rng.integers(1, 40)) + 1, size=B)
    r, starts = tables(lengths, align=int(rng.integers(1, 9)), sampling_rate=8000)
    check(r, lengths, starts, 256)


def test_the_keyword_changes_no_table_at_16000():
    a, starts = tables(LENGTHS_37)
    b, _ = tables(LENGTHS_37, sampling_rate=16000)
    check(b, LENGTHS_37, starts, 512)
    for name in ragged.RaggedClips.TABLES:
        x, y = getattr(a, name + "_host"), getattr(b, name + "_host")
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    assert (a.tiles, a.n_runs, a.n_windows, a.workspace_bytes, a.window) == (b.tiles, b.n_runs, b.n_windows, b.workspace_bytes, 512)
    clips = [np.zeros(n, np.int16) for n in LENGTHS_37[:20]]
    c = ragged.RaggedClips.from_clips(clips, None, 8)                                         # positional signature as before
    d = ragged.RaggedClips.from_clips(clips, device=None, sampling_rate=16000)
    assert c.sampling_rate == d.sampling_rate == 16000
    for name in ragged.RaggedClips.TABLES:
        assert getattr(c, name + "_host").tobytes() == getattr(d, name + "_host").tobytes(), name
    e = ragged.RaggedClips.from_clips(clips, device=None, sampling_rate=8000)
    assert e.window == 256 and e.n_windows > c.n_windows and np.array_equal(e.pcm_host, c.pcm_host)


@pytest.mark.parametrize("rate", [44100, 32000, 0, 16001])
def test_other_rates_are_refused(rate):
    with pytest.raises(ValueError, match=str(rate)):
        tables(LENGTHS_37, sampling_rate=rate)
    with pytest.raises(ValueError, match=str(rate)):
        ragged.RaggedClips.from_clips([np.zeros(5, np.float32)], device=None, sampling_rate=rate)


def check_parts(r, cap_tiles):
    parts = r.parts(cap_tiles * TILE)
    assert parts[0][0] == 0 and parts[-1][1] == r.groups
    for (a0, a1), (b0, b1) in zip(parts, parts[1:]):
        assert a1 == b0                                   # every group once, in order
    for g0, g1 in parts:
        assert g0 < g1
        assert int(r.group_windows[g0:g1].sum()) <= cap_tiles
        # greedy: the next group would not have fitted
        assert g1 == r.groups or int(r.group_windows[g0:g1 + 1].sum()) > cap_tiles
    return parts


@pytest.mark.parametrize("rate", [16000, 8000])
def test_parts_cover_every_group_once_under_the_cap(rate):
    rng = np.random.default_rng(7)
    win = ragged.SILERO_WINDOWS[rate]
    for _ in range(20):
        B = int(rng.integers(1, 200))
        lengths = rng.integers(1, win * int(rng.integers(1, 30)) + 1, size=B)
        r, _ = tables(lengths, sampling_rate=rate)
        t0 = int(r.group_windows[0])
        for cap in sorted({t0, t0 + 1, 2 * t0, max(t0, r.tiles - 1), r.tiles, r.tiles + 5}):
            parts = check_parts(r, cap)
            if cap >= r.tiles:
                assert parts == [(0, r.groups)]
            else:
                assert len(parts) >= 2
        assert r.parts(t0 * TILE + TILE - 1) == r.parts(t0 * TILE)          # a cap is used in whole tiles
        with pytest.raises(ValueError, match="WORKSPACE_CAP_BYTES"):
            r.parts((t0 - 1) * TILE)
        with pytest.raises(ValueError, match="WORKSPACE_CAP_BYTES"):
            r.parts(t0 * TILE - 1)


def test_parts_of_a_known_set():
    # T_g = 9, 5, 5, 2, 1 (the last group partial)
    lengths = [512 * 9] * 16 + [512 * 5] * 32 + [512 * 2] * 16 + [100] * 3
    r, _ = tables(lengths)
    assert r.group_windows.tolist() == [9, 5, 5, 2, 1] and r.tiles == 22
    assert r.parts(22 * TILE) == [(0, 5)] and r.parts(1 << 40) == [(0, 5)]
    assert r.parts(21 * TILE) == [(0, 4), (4, 5)]
    assert r.parts(14 * TILE) == [(0, 2), (2, 5)]
    assert r.parts(9 * TILE) == [(0, 1), (1, 2), (2, 5)]
    with pytest.raises(ValueError, match="WORKSPACE_CAP_BYTES"):
        r.parts(8 * TILE)
