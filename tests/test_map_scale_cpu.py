"""The scenes of tests/map_scale_scenes.py reach the paths they are for: shown here from the numpy specifications and plain
arithmetic alone, before tests/test_map_scale_gpu.py runs them on the device.  These are conditions of the scenes (their seeds are
chosen to meet them), not measurements.  The sizes named are map_store_kernels.hip's: a selection workgroup takes 1024 candidates
(MS_CHUNK) and sums the counts of the workgroups before it 256 at a time (MS_THREADS); the ranking holds 1024 weights at a time
(COV_TILE); the long-track ranking and the window's observer order take 256 entries a round."""
import numpy as np
import pytest

import ba_collect_spec as BSP
import covisibility_scenes as V
import covisibility_spec as CS
import map_fuse_scenes as F
import map_fuse_spec as FSP
import map_observations_scenes as OS
import map_observations_spec as OSP
import map_scale_scenes as Z
import map_store_spec as MSP


@pytest.fixture(scope="module")
def big():
    return Z.big_store()


# ---- the sorted restatement of the observation lists ----------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs,capacity", [(3, 4096), (11, 1000), (65, 4096)])
def test_sorted_observations_equal_the_looped_specification_on_the_small_worlds(n_kfs, capacity):
    tables, counts, live = V.world(40 + n_kfs + capacity, n_kfs, capacity=capacity)
    live, lonely = OS.with_unobserved(tables, live)
    ls = np.random.default_rng(n_kfs).permutation(np.flatnonzero(live)).astype(np.int32)
    for slots in (ls, ls[:1], ls[::3], np.array([lonely], np.int32), ls[:0]):
        want = OSP.observations(tables, live, slots)
        got = Z.observations_sorted(tables, live, slots)
        assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)), len(slots)
    assert want[0].tolist() == [0] and len(OSP.observations(tables, live, ls)[1]) > n_kfs


def test_sorted_observations_equal_the_looped_specification_on_a_rising_world():
    tables, counts, live = V.row_world("rising", 258)
    slots = np.random.default_rng(3).permutation(2500).astype(np.int32)
    want = OSP.observations(tables, live, slots)
    got = Z.observations_sorted(tables, live, slots)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and set(np.diff(want[0]).tolist()) == set(range(0, 259))


# ---- scene 1: the big store -------------------------------------------------------------------------------------------------------

def test_big_store_names_slots_past_2_to_the_20_and_lists_more_than_256_chunks(big):
    cap, slots, gone = big["capacity"], big["slots"], big["gone"]
    assert cap == (1 << 20) + 7 and cap % 64 != 0 and len(slots) == 300000 and len(set(slots.tolist())) == len(slots)
    have = set(slots.tolist())
    assert set(range(100)) <= have and set(range(65536 - 50, 65536 + 50)) <= have and set(range((1 << 20) - 50, cap)) <= have
    assert 140000 < len(gone) <= 150000 and set(gone.tolist()) < have
    assert Z.n_chunks(len(slots)) >= 258                                    # one frame: n_chunk alone passes the second stride of the base sum
    for live in (Z.live_bytes(cap, slots), Z.live_bytes(cap, slots, gone)):
        lst = MSP.select_slots(slots, live)
        assert (lst >= (1 << 20)).any() and (lst == cap - 1).any() and (lst >= 65536).sum() > 100000 and len(lst) == int(live.sum())
    assert len(MSP.select_slots(slots, Z.live_bytes(cap, slots, gone))) == len(slots) - len(gone)
    assert (gone >= (1 << 20)).any() and (gone < 100).any()                 # the erase reaches both ends too


# ---- scene 2: many frames, many chunks ----------------------------------------------------------------------------------------------

def test_frame_batches_pass_257_workgroups_both_ways():
    sc = Z.frames_scene()
    B = len(sc["small_frames"])
    cand = [sum(sc["small_n"][k] for k in f) for f in sc["small_frames"]]
    assert B == 300 and Z.n_chunks(max(cand)) == 1 and B * 1 >= 258            # n_chunk = 1: `me` runs to 299
    assert sum(1 for f in sc["small_frames"] if not f) >= 10 and sum(1 for f in sc["small_frames"] if len(f) == 2) >= 10
    used = [k for f in sc["small_frames"] for k in f]
    assert len(used) > 2 * len(set(used))                                   # keyframes are shared between frames
    lists = [MSP.select_keyframes([sc["small"][k] for k in f], sc["live"]) for f in sc["small_frames"]]
    assert sum(len(x) > 0 for x in lists) > 200 and any(len(x) == 0 and f for x, f in zip(lists, sc["small_frames"]))
    wide = [sum(sc["wide_n"][k] for k in f) for f in sc["wide_frames"]]
    assert wide == [90 * 1025, 0, 90 * 1025] and 3 * Z.n_chunks(max(wide)) >= 258
    wl = [MSP.select_keyframes([sc["wide"][k] for k in f], sc["live"]) for f in sc["wide_frames"]]
    assert len(wl[0]) > 1000 and len(wl[1]) == 0 and sorted(wl[0].tolist()) == sorted(wl[2].tolist()) and wl[0].tolist() != wl[2].tolist()
    assert any(t is None for t in sc["wide"]) and any(t is None for t in sc["small"])


# ---- scene 3: keyframes past the ranking tile -----------------------------------------------------------------------------------

def _cuts_inside_a_tie(row, n_best):
    order, n = CS.best(row, len(row))
    return n_best < n and row[order[n_best - 1]] == row[order[n_best]]


def test_rank_worlds_tie_across_the_tile_borders_and_n_best_cuts_inside_the_tie():
    tables, counts, live = Z.rank_world("equal", 2049)
    w = CS.weights(tables, live, Z.rank_queries(2049))
    assert Z.rank_queries(2049) == [0, 1023, 1024, 2048] and Z.rank_queries(1023) == [0, 1022] and Z.rank_queries(1024) == [0, 1023]
    assert Z.tie_across(w[0], Z.COV_TILE - 1) and Z.tie_across(w[0], 2 * Z.COV_TILE - 1)        # 1023 / 1024 and 2047 / 2048
    assert all(_cuts_inside_a_tie(w[0], n) for n in (10, 1023, 1024, 1025)) and not _cuts_inside_a_tie(w[0], 2049 + 3)
    assert (w[1] > 0).sum() == 5 and w[1][1022] == w[1][1024] == 2 and w[1][1021] == w[1][1025] == 1     # query 1023: ties either side of the border
    for n_kfs in (1024, 1025):
        tables, counts, live = Z.rank_world("equal", n_kfs)
        w = CS.weights(tables, live, [0])
        assert (w[0] > 0).sum() == n_kfs - 1 and (Z.tie_across(w[0], 1023) or n_kfs == 1024) and _cuts_inside_a_tie(w[0], 10) and _cuts_inside_a_tie(w[0], 1023) == (n_kfs == 1025)
    tables, counts, live = Z.rank_world("rising", 2049)
    w = CS.weights(tables, live, [0])
    assert w[0].tolist() == list(range(2049))                               # no ties: rank = n_kfs - 1 - index, counted over three tiles
    tables, counts, live = Z.rank_world("mixed", 2049)
    w = CS.weights(tables, live, Z.rank_queries(2049))
    assert ((w > 0).sum(1) > Z.COV_TILE).any() and any(_cuts_inside_a_tie(r, 10) for r in w)
    assert all(Z.tie_spans(r, 1023) for r in w) and any(Z.tie_spans(r, 2047) for r in w)       # index order decides across the borders


# ---- scene 4: a local map over every keyframe -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_kfs", Z.LOCAL_N_KFS)
def test_local_scene_has_more_segments_than_one_scan_round(n_kfs):
    sc = Z.local_scene(n_kfs)
    assert len(sc["tables"]) == n_kfs > 2 * Z.THREADS                       # ref = -1: S = n_kfs segments, three or more rounds of 256
    keys, row = CS.local_keyframes(sc["tables"], sc["store"].live, -1, 2)
    assert keys == list(range(n_kfs)) and row.tolist() == [-1, -1, -1]
    lst = MSP.select_keyframes(sc["tables"], sc["store"].live)
    assert set(sc["slots"].tolist()) <= set(lst.tolist()) and len(lst) > 1000
    n = [len(t) for t in sc["tables"]]
    assert 30 <= np.median(n) <= 50 and Z.n_chunks(sum(n)) >= 20


# ---- scene 5: long tracks and many points -----------------------------------------------------------------------------------------

def test_rising_world_has_tracks_past_two_rounds_of_512():
    tables, counts, live = V.row_world("rising", Z.RISING_N_KFS)
    slots = Z.rising_slots()
    assert len(set(slots.tolist())) == len(slots) and slots.max() < len(live)
    lengths = np.diff(Z.observations_sorted(tables, live, slots)[0])
    assert lengths.max() == 1026 >= 1025 and set(lengths.tolist()) == set(range(0, 1027))
    n = OSP.n_observers(tables, live)
    assert n.max() == 1026 and (n - 1 >= 1025).sum() == 1 and (n - 1 >= 3).sum() > 1000         # min_observations = 1025 keeps one point


def test_big_observation_list_has_more_than_256_chunks_of_points(big):
    assert len(big["slots"]) >= 263169 and Z.n_chunks(len(big["slots"])) >= 258
    tables = Z.big_tables(big)
    live = Z.live_bytes(big["capacity"], big["slots"])
    start, kf, feat = Z.observations_sorted(tables, live, big["slots"])
    assert len(tables) == 40 and 180000 < start[-1] < 240000 and np.diff(start).max() >= 3
    top = int(big["slots"].tolist().index(big["capacity"] - 1))
    assert start[top + 1] - start[top] == 40 and kf[start[top]:start[top + 1]].tolist() == list(range(40))     # every keyframe names slot capacity - 1


# ---- scene 6: many fixed observers ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_covisible", [3, 20])
def test_window_world_has_600_fixed_observers(max_covisible):
    tables, counts, live, xy = Z.window_world()
    c = BSP.collect(tables, xy, live, 0, max_covisible)
    K, Fx, Mp, N = (int(x) for x in c["counts"])
    assert K == max_covisible and Fx - 1 >= 600 and len(c["fixed_kf"]) == Fx - 1 and Mp > 100 and N > Fx
    assert len(tables) == 1025 and any(t is None for t in tables)


# ---- scene 7: many merges ---------------------------------------------------------------------------------------------------------

def test_merge_world_has_520_goners_in_classes_of_two(oracle):
    sc = Z.merge_world()
    r = FSP.fuse(sc["tables"], sc["live"], sc["positions"], sc["desc"], [Z.MERGE_CUR], Z.MERGE_TGT, F.oracle_search(oracle, sc))
    assert int(r["counts"][3]) >= 520 and len(r["goner"]) == int(r["counts"][3]) and int(r["counts"][2]) >= 20
    assert max(len(m) for m in r["stats"]["members"].values()) == 2
    L = set(r["list_slot"].tolist())
    assert all(int(k) in L and int(g) not in L for g, k in zip(r["goner"], r["keeper"]))       # the projected point keeps every time
    assert r["goner"].tolist() == sorted(r["goner"].tolist())
