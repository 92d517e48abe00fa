"""CPU checks of the local-BA window collected from the resident map: the specification (tests/ba_collect_spec.py) against the
restatement of the reference's collect_visual_ba_data (oracle/local_mapper_ref.py) and against hand-made edge cases, the scene the
GPU tests solve (tests/ba_collect_scenes.py), the new ABI as a C compiler reads it and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import ba_collect_scenes as B
import ba_collect_spec as S
import covisibility_scenes as V
import covisibility_spec as CS
from oracle import local_mapper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
NEW_SYMBOLS = ("orbx_map_collect_ba_window_device", "orbx_map_collect_ba_window", "orbx_ba_solve_visual_obs32_device", "orbx_map_local_ba")


def build_driver(tmp):
    exe = os.path.join(tmp, "ba_collect_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "ba_collect_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


def reference_map(tables, xy, live, cur):
    """oracle/local_mapper_ref.Map of a world whose tables name every slot once per keyframe: keyframe k has id 100 + k (ids ascend
    with position), a live slot s is map point s, every observation is associated in both directions in keyframe order, and cur's
    covisibility list is given in the library's order (weight descending, then position)."""
    m = R.Map()
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    for s in np.flatnonzero(live).tolist():
        m.map_points[s] = R.MapPoint(np.zeros(3))
    for k, t in enumerate(tables):
        ids = [None] * len(xy[k]) if t is None else [None if s < 0 else int(s) for s in t.tolist()]
        m.keyframes[100 + k] = R.KeyFrame(ident, [(float(x), float(y)) for x, y in xy[k]], ids)
        for i, s in enumerate(ids):
            if s is not None and s in m.map_points:
                assert 100 + k not in m.map_points[s].observations
                m.map_points[s].observations[100 + k] = i
    row = CS.weights(tables, live, [cur])[0]
    best, n = CS.best(row, len(tables))
    m.keyframes[100 + cur].covisibility_weights = {100 + int(b): int(row[b]) for b in best[:n]}
    return m


def _against_reference(tables, xy, live, cur, max_covisible):
    got = S.collect(tables, xy, live, cur, max_covisible)
    want = R.collect_visual_ba_data(reference_map(tables, xy, live, cur), 100 + cur, max_covisible)
    if want is None:
        assert got["empty"]
        return got, want
    K, F, M, N = got["counts"]
    assert not got["empty"] and M > 0 and N > 0
    local = got["local_kf"][:1 + K]
    assert [want["anchor_kf_id"]] + want["optimized_kf_ids"] == [100 + int(k) for k in local]                 # equal in order
    assert want["mp_ids"] == got["list_slot"].tolist()                                                         # equal in order
    assert set(want["fixed_kf_poses"]) - {want["anchor_kf_id"]} == {100 + int(k) for k in got["fixed_kf"]} and F == 1 + len(got["fixed_kf"])
    assert got["fixed_kf"].tolist() == sorted(got["fixed_kf"].tolist())
    observers = [int(k) for k in local] + got["fixed_kf"].tolist()

    def key(o):
        i = o["kf_idx"]
        kf = observers[i + 1] if i >= -1 else observers[len(local) + (-2 - i)]
        return (100 + kf, int(got["list_slot"][o["mp_idx"]]), float(o["u"]), float(o["v"]), bool(i >= 0))

    mine = sorted(key(o) for o in got["obs32"])
    theirs = sorted((o["kf_id"], o["mp_id"], o["uv"][0], o["uv"][1], o["is_kf_optimized"]) for o in want["observations"])
    assert mine == theirs and len(mine) == N
    return got, want


@pytest.mark.parametrize("seed,n_kfs", [(1, 3), (2, 11), (3, 64)])
def test_spec_equals_the_reference_restatement(seed, n_kfs):
    """world(seed, n) with its repeats removed: every observation associated once, in both directions"""
    tables, counts, live = V.world(seed, n_kfs)
    tables = B.once(tables)
    xy = B.keypoints(seed, counts)
    seen = 0
    for cur in sorted({0, n_kfs - 1, n_kfs // 2}):
        got, want = _against_reference(tables, xy, live, cur, 20)
        seen += want is not None
    assert seen > 0
    if n_kfs == 64:
        assert got["counts"][0] == 20 and got["counts"][1] > 1                                                # more covisibles than the cap; other observers


@pytest.mark.parametrize("max_covisible", [0, 1, 3])
def test_spec_equals_the_reference_where_covisibles_exceed_the_cap(max_covisible):
    tables, counts, live = V.world(2, 11)
    tables = B.once(tables)
    xy = B.keypoints(2, counts)
    cur = 3
    assert (CS.weights(tables, live, [cur])[0] > 0).sum() > 3
    got, want = _against_reference(tables, xy, live, cur, max_covisible)
    assert want is not None and got["counts"][0] == max_covisible and len(got["local_kf"]) == 1 + max_covisible
    assert got["counts"][1] - 1 == (CS.weights(tables, live, [cur])[0] > 0).sum() - max_covisible             # every other covisible is a fixed observer


def _xy(tables):
    return [np.arange(2 * (0 if t is None else len(t)), dtype=np.float32).reshape(-1, 2) + 100 * k for k, t in enumerate(tables)]


def test_repeats_inside_a_keyframe_give_one_observation_each():
    live = np.ones(16, np.uint8)
    tables = [np.array([5, 5, 7], np.int32), np.array([7, 7, 7, 9], np.int32)]
    r = S.collect(tables, _xy(tables), live, 0, 4)
    assert r["counts"].tolist() == [1, 1, 3, 7] and r["list_slot"].tolist() == [5, 7, 9]
    assert r["obs32"]["kf_idx"].tolist() == [-1, -1, -1, 0, 0, 0, 0] and r["obs32"]["mp_idx"].tolist() == [0, 0, 1, 1, 1, 1, 2]
    assert r["obs32"]["u"].tolist() == [0.0, 2.0, 4.0, 100.0, 102.0, 104.0, 106.0]                             # each observer's features in index order
    assert S.collect(tables, _xy(tables), live, 1, 4)["list_slot"].tolist() == [7, 9, 5]                      # first seen walking local = [1, 0]


def test_dead_and_minus_one_entries_are_skipped():
    live = np.ones(16, np.uint8); live[3] = 0
    tables = [np.array([-1, 3, 4, -1, 6], np.int32), np.array([3, 4, -1], np.int32), np.array([3, -1], np.int32)]
    r = S.collect(tables, _xy(tables), live, 0, 0)
    assert r["counts"].tolist() == [0, 2, 2, 3] and r["list_slot"].tolist() == [4, 6] and r["fixed_kf"].tolist() == [1]
    assert r["obs32"]["kf_idx"].tolist() == [-1, -1, -2] and r["obs32"]["mp_idx"].tolist() == [0, 1, 0]
    assert r["obs32"]["v"].tolist() == [5.0, 9.0, 103.0]                                                       # keyframe 2 names only the dead slot: no observer


def test_a_keyframe_without_a_table_is_never_fixed_and_cur_without_one_is_empty():
    live = np.ones(16, np.uint8)
    tables = [np.array([1, 2], np.int32), None, np.array([2], np.int32)]
    xy = _xy(tables); xy[1] = np.zeros((5, 2), np.float32)
    r = S.collect(tables, xy, live, 0, 0)
    assert r["fixed_kf"].tolist() == [2] and r["counts"].tolist() == [0, 2, 2, 3]
    e = S.collect(tables, xy, live, 1, 3)
    assert e["empty"] and e["counts"].tolist() == [0, 1, 0, 0] and e["local_kf"].tolist() == [1, -1, -1, -1]
    assert R.collect_visual_ba_data(reference_map(tables, xy, live, 1), 101, 3) is None


def test_cur_as_the_only_keyframe():
    live = np.ones(16, np.uint8)
    tables = [np.array([8, 1, 8], np.int32)]
    r = S.collect(tables, _xy(tables), live, 0, 20)
    assert r["counts"].tolist() == [0, 1, 2, 3] and not r["empty"] and len(r["fixed_kf"]) == 0 and r["local_kf"].tolist() == [0] + [-1] * 20
    assert r["obs32"]["kf_idx"].tolist() == [-1, -1, -1] and r["obs32"]["mp_idx"].tolist() == [0, 1, 0]


def test_ba_scene_is_what_it_claims():
    sc = B.ba_scene()
    xy = [np.stack([k["x"], k["y"]], 1) for k in sc["kps"]]
    r = S.collect(sc["tables"], xy, sc["store"].live, sc["cur"], sc["max_covisible"])
    K, F, M, N = r["counts"]
    assert K == 3 and F == 3 and M >= 140 and N > 3 * M                                                       # two fixed observers besides the anchor
    assert len(sc["tables"]) == 6 and all(len(t) == len(k) for t, k in zip(sc["tables"], sc["kps"]))
    t1 = sc["tables"][1]
    assert len(np.unique(t1[t1 >= 0])) < (t1 >= 0).sum()                                                       # a point observed twice by one keyframe
    assert all((sc["store"].live[t[t >= 0]] == 0).sum() == 2 for t in sc["tables"])                            # slots that are not live
    assert np.linalg.norm(sc["poses_wc"][:, 4:], axis=1).min() > 1.0                                           # (the relative bar on translations)


def test_new_symbols_and_header_as_c(pkg, tmp_path):
    L = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("map_collect_ba_window_device", "map_collect_ba_window", "ba_solve_visual_obs32_device", "map_local_ba"):
        assert hasattr(pkg.Handle, m), m
    assert issubclass(pkg.MapLocalBAResult, pkg.VisualBAResultData)
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "orbx.h"\nint main(void) {\n  void* p[] = {%s};\n  printf("%%zu %%zu\\n", sizeof(p) / sizeof(p[0]), sizeof(orbx_ba_obs32));\n'
                   '  return 0;\n}\n' % ", ".join("(void*)%s" % s for s in NEW_SYMBOLS))
    obj = tmp_path / "decl.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert obj.exists()
    assert S.BA_OBS32 == pkg.BA_OBS32


def test_ba_collect_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_driver(str(tmp_path)))
