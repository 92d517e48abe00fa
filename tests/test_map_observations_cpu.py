"""CPU checks of the observation calls on the resident map: the specification (tests/map_observations_spec.py) against hand-made
answers, against the observation lists a host snapshot keeps (api.MapSnapshot.collect_map_point_refresh) and against a literal
replay of the reference's cull_keyframes; the new ABI as a C compiler reads it and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import ba_collect_scenes as B
import covisibility_scenes as V
import map_observations_scenes as OS
import map_observations_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
NEW_SYMBOLS = ("orbx_map_observations_device", "orbx_map_observations", "orbx_map_refresh_points_device", "orbx_map_refresh_points",
               "orbx_map_keyframe_redundancy_device", "orbx_map_keyframe_redundancy")


def build_driver(tmp):
    exe = os.path.join(tmp, "map_observations_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_observations_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


# ---- the specification on hand-made answers --------------------------------------------------------------------------------

def test_a_slot_named_twice_in_one_keyframe_keeps_the_first_feature():
    live = np.ones(16, np.uint8)
    tables = [np.array([5, 7, 5, 7, 7], np.int32), np.array([-1, 7, 5], np.int32)]
    start, kf, feat = S.observations(tables, live, [7, 5])
    assert start.tolist() == [0, 2, 4] and kf.tolist() == [0, 1, 0, 1] and feat.tolist() == [1, 1, 0, 2]
    assert S.n_observers(tables, live)[[5, 7, 6]].tolist() == [2, 2, 0]
    # the redundancy counts features: the repeats are features too
    total, red, cull = S.redundancy(tables, live, [0, 1], 1, 0.5)
    assert total.tolist() == [5, 2] and red.tolist() == [5, 2] and cull.tolist() == [1, 1]
    assert S.redundancy(tables, live, [0], 2, 0.5)[1].tolist() == [0]


def test_a_dead_slot_is_observed_by_nobody():
    live = np.ones(16, np.uint8); live[3] = 0
    tables = [np.array([3, 4], np.int32), np.array([4, 3, 99, -1], np.int32)]                  # (99: past the capacity)
    start, kf, feat = S.observations(tables, live, [4])
    assert start.tolist() == [0, 2] and kf.tolist() == [0, 1] and feat.tolist() == [1, 0]
    assert S.n_observers(tables, live)[3] == 0
    assert S.redundancy(tables, live, [1, 0], 0, 0.9)[0].tolist() == [1, 1]


def test_a_keyframe_without_a_table_observes_nothing():
    live = np.ones(16, np.uint8)
    tables = [np.array([1, 2], np.int32), None, np.array([2], np.int32)]
    start, kf, feat = S.observations(tables, live, [2, 1, 9])
    assert start.tolist() == [0, 2, 3, 3] and kf.tolist() == [0, 2, 0] and feat.tolist() == [1, 0, 0]
    assert [x.tolist() for x in S.redundancy(tables, live, [1], 0, 0.5)] == [[0], [0], [0]]
    assert [x.tolist() for x in S.observations([], live, [2])] == [[0, 0], [], []]


# ---- against the lists a host snapshot keeps ---------------------------------------------------------------------------------

def _snapshot(pkg, tables, counts, live):
    """api.MapSnapshot of a world: keyframe k has id 100 + k, a live slot s is map point s, every feature that carries a live point
    is one observation, recorded keyframe by keyframe in feature order (one association per keyframe: no repeats in the tables)"""
    n_kf = len(tables)
    feat_mp, obs = [], {int(s): [] for s in np.flatnonzero(live)}
    for k, (t, n) in enumerate(zip(tables, counts)):
        ids = np.full(n, -1, np.int64) if t is None else np.asarray(t, np.int64)
        feat_mp.append(ids)
        for i, s in enumerate(ids.tolist()):
            if s in obs:
                obs[s].append((100 + k, i))
    mp_ids = sorted(obs)
    start, okf, ofeat = [0], [], []
    for m in mp_ids:
        okf.extend(k for k, _ in obs[m]); ofeat.extend(f for _, f in obs[m]); start.append(len(okf))
    off = np.zeros(n_kf + 1, np.int32); off[1:] = np.cumsum(counts)
    return pkg.MapSnapshot(kf_ids=[100 + k for k in range(n_kf)], kf_bad=np.zeros(n_kf, np.uint8), kf_pose_wc=np.tile([1.0, 0, 0, 0, 0, 0, 0], (n_kf, 1)),
                           kf_n_keypoints=counts, kf_feat_start=off, feat_mp_id=np.concatenate(feat_mp + [np.zeros(0, np.int64)]),
                           feat_uv=np.zeros((int(off[-1]), 2), np.float32), cov_start=np.zeros(n_kf + 1, np.int32), cov_kf_id=np.zeros(0, np.uint64), mp_ids=mp_ids,
                           mp_bad=np.zeros(len(mp_ids), np.uint8), mp_pos=np.zeros((len(mp_ids), 3)), mp_obs_start=start, mp_obs_kf_id=okf, mp_obs_feat_idx=ofeat)


@pytest.mark.parametrize("seed,n_kfs", [(1, 3), (2, 11), (3, 64)])
def test_spec_equals_the_lists_a_snapshot_keeps(pkg, seed, n_kfs):
    tables, counts, live = V.world(seed, n_kfs)
    tables = B.once(tables)
    slots = np.random.default_rng(seed).permutation(np.flatnonzero(live)).astype(np.int32)
    d = _snapshot(pkg, tables, counts, live).collect_map_point_refresh(slots.tolist())
    start, kf, feat = S.observations(tables, live, slots)
    assert d.mp_ids == slots.tolist() and d.obs_start.tobytes() == start.tobytes() and start[-1] > 0
    for p in range(len(slots)):                                              # (the snapshot numbers keyframes in first-seen order: compare as sets)
        mine = {(100 + int(k), int(f)) for k, f in zip(kf[start[p]:start[p + 1]], feat[start[p]:start[p + 1]])}
        theirs = {(d.kf_ids[k], int(f)) for k, f in zip(d.obs_kf[start[p]:start[p + 1]], d.obs_feat[start[p]:start[p + 1]])}
        assert mine == theirs and len(mine) == start[p + 1] - start[p]
        assert kf[start[p]:start[p + 1]].tolist() == sorted(kf[start[p]:start[p + 1]].tolist())
    assert S.n_observers(tables, live)[slots].tolist() == np.diff(start).tolist()


# ---- against the reference's cull_keyframes ----------------------------------------------------------------------------------

def _host_map(tables, live):
    kf_points = {k: ([] if t is None else [int(s) if 0 <= s < len(live) else None for s in t.tolist()]) for k, t in enumerate(tables)}
    observers = {int(s): set() for s in np.flatnonzero(live)}
    for k, pts in kf_points.items():
        for s in pts:
            if s in observers:
                observers[s].add(k)
    return kf_points, observers


@pytest.mark.parametrize("threshold", [0.5, 0.9])
def test_redundancy_spec_restates_cull_keyframes(threshold):
    tables, counts, live, want = OS.ratio_world()
    cand = [3, 4, 5, 6, 0]
    kf_points, observers = _host_map(tables, live)
    ref = S.cull_keyframes_replay(kf_points, observers, cand, 3, threshold)
    total, red, cull = S.redundancy(tables, live, cand, 3, threshold)
    assert [(int(t), int(r), bool(c)) for t, r, c in zip(total, red, cull)] == [ref[k] for k in cand]
    assert [(int(t), int(r)) for t, r in zip(total[:4], red[:4])] == [want[k] for k in (3, 4, 5, 6)] == [(10, 5), (11, 6), (10, 9), (20, 19)]
    # the inequality is strict: a ratio exactly at the threshold is not culled, one feature above it is
    assert cull.tolist() == ([0, 1, 1, 1, 0] if threshold == 0.5 else [0, 0, 0, 1, 0])
    assert 5 / 10 == 0.5 and 9 / 10 == 0.9 and 6 / 11 > 0.5 and 19 / 20 > 0.9


@pytest.mark.parametrize("seed,n_kfs", [(4, 11), (5, 64)])
def test_redundancy_spec_restates_cull_keyframes_on_random_worlds(seed, n_kfs):
    tables, counts, live = V.world(seed, n_kfs)
    kf_points, observers = _host_map(tables, live)
    cand = list(range(n_kfs))
    for min_obs in (0, 3):
        ref = S.cull_keyframes_replay(kf_points, observers, cand, min_obs, 0.5)
        total, red, cull = S.redundancy(tables, live, cand, min_obs, 0.5)
        assert [(int(t), int(r), bool(c)) for t, r, c in zip(total, red, cull)] == [ref[k] for k in cand]
    assert total.max() > 500 and 0 < red.sum() < total.sum()


# ---- the ABI and the C++ mirror ------------------------------------------------------------------------------------------------

def test_new_symbols_and_header_as_c(pkg, tmp_path):
    L = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("map_observations_device", "map_observations", "map_refresh_points_device", "map_refresh_points", "map_keyframe_redundancy_device",
              "map_keyframe_redundancy"):
        assert hasattr(pkg.Handle, m), m
    assert L.orbx_abi_version() == 2
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "orbx.h"\nint main(void) {\n  void* p[] = {%s};\n  printf("%%zu\\n", sizeof(p) / sizeof(p[0]));\n  return 0;\n}\n'
                   % ", ".join("(void*)%s" % s for s in NEW_SYMBOLS))
    obj = tmp_path / "decl.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert obj.exists()


def test_map_observations_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_driver(str(tmp_path)))
