"""CPU checks of point creation and removal on the resident map: the specification (tests/map_create_spec.py) against hand-made
answers, one per rule; against a literal sequential replay of the reference on every scene; what every scene is required to show;
the new ABI as a C compiler reads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_create_scenes as W
import map_create_spec as S
import triangulation_scenes as G
import triangulation_spec as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
NEW_SYMBOLS = ("orbx_keyframe_set_map_point_slots_device", "orbx_map_create_points_device", "orbx_map_create_points", "orbx_map_remove_points",
               "orbx_map_cull_points")
MARGIN = 1e-9


def build_driver(tmp):
    exe = os.path.join(tmp, "map_create_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_create_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


# ---- the specification on hand-made answers --------------------------------------------------------------------------------

class _Search:
    """stands in for the oracle: every search answers the next prepared pair list and records the flags it was given"""

    def __init__(self, answers):
        self.answers, self.seen = list(answers), []

    def Camera(self, **kw):
        return None

    def search_for_triangulation(self, cam, kp1, desc1, mp1, has1, kp2, desc2, mp2, *rest):
        self.seen.append((np.array(mp1, np.uint8), np.array(mp2, np.uint8)))
        return self.answers.pop(0)


def _stereo_keyframe(has):
    n = len(has)
    kf = dict(kp=np.zeros(n, G.KEYPOINT), desc=np.arange(32 * n, dtype=np.uint32).astype(np.uint8).reshape(n, 32), mp=np.zeros(n, np.uint8),
              pts=np.arange(3 * n, dtype=np.float64).reshape(n, 3) + 1.0, has=np.array(has, np.uint8), node=None,
              pose=np.array([np.cos(0.1), 0.0, np.sin(0.1), 0.0, 1.0, 2.0, 3.0]))
    return kf


def _stereo(table, live, free, has=(1, 1, 1, 0, 1)):
    cur = _stereo_keyframe(has)
    return cur, S.create_points(None, G.CAMERA, TS.default_config(), 0, cur, [], [table], live, free, S.STEREO)


def test_a_dead_or_out_of_range_entry_counts_as_free():
    live = np.zeros(16, np.uint8); live[3] = 1
    cur, r = _stereo(np.array([3, 5, -1, 5, 99], np.int32), live, [9, 8, 7, 6])
    assert r["counts"].tolist() == [3, 0, 3, 0]                            # features 1 (dead slot 5), 2 (-1) and 4 (99 is no slot); 0 is flagged, 3 has no stereo point
    assert r["new_idx1"].tolist() == [1, 2, 4] and r["new_slot"].tolist() == [9, 8, 7] and r["new_neighbour"].tolist() == [-1] * 3 == r["new_idx2"].tolist()
    assert r["tables"][0].tolist() == [3, 9, 8, 5, 7]                      # the dead entry of feature 3 stays: nothing was created there
    assert np.allclose(r["new_points"][0], TS.transform_point(cur["pose"], cur["pts"][1])) and r["new_desc"].tobytes() == cur["desc"][[1, 2, 4]].tobytes()


def test_truncation_drops_the_later_stereo_candidates():
    live = np.zeros(16, np.uint8)
    _, r = _stereo(np.full(5, -1, np.int32), live, [4, 2])
    assert r["counts"].tolist() == [4, 0, 2, 2] and r["new_idx1"].tolist() == [0, 1] and r["tables"][0].tolist() == [4, 2, -1, -1, -1]
    _, r = _stereo(np.full(5, -1, np.int32), live, [])
    assert r["counts"].tolist() == [4, 0, 0, 4] and r["tables"][0].tolist() == [-1] * 5 and len(r["new_slot"]) == 0


def test_a_keyframe_without_a_table_is_given_one():
    _, r = _stereo(None, np.ones(16, np.uint8), [11, 12, 13, 14, 15])
    assert r["counts"].tolist() == [4, 0, 4, 0] and r["tables"][0].tolist() == [11, 12, 13, -1, 14]


def _pair_world():
    """the pair scene's current keyframe with neighbours 0 and 3, and validated pairs: A, B, C with neighbour 0 and D, E with
    neighbour 3, where E is on the same current feature as A"""
    sc = G.pair_scene()
    cur, nbs = sc["current"], [sc["neighbours"][0], sc["neighbours"][3]]
    ok = []
    for nb, gt in zip(nbs, (sc["gt"][0], sc["gt"][3])):
        ok.append([(int(a), int(b)) for a, b in gt
                   if TS.triangulate_pair(sc["camera"], TS.default_config(), 0, cur["kp"], cur["pts"], cur["has"], cur["pose"], nb["kp"], nb["pts"], nb["has"],
                                          nb["pose"], int(a), int(b))[0] == TS.CREATED])
    both = sorted(set(a for a, _ in ok[0]) & set(a for a, _ in ok[1]))
    A = next(p for p in ok[0] if p[0] == both[0]); E = next(p for p in ok[1] if p[0] == both[0])
    B, Cc = [p for p in ok[0] if p[0] not in both][:2]
    D = next(p for p in ok[1] if p[0] not in both)
    return sc, cur, nbs, [[A, B, Cc], [D, E]]


def test_creation_order_is_free_slot_order_and_the_last_pair_of_a_feature_wins():
    sc, cur, nbs, answers = _pair_world()
    (A, B, Cc), (D, E) = answers
    live = np.zeros(64, np.uint8)
    tables = [np.full(len(cur["kp"]), -1, np.int32), None, np.full(len(nbs[1]["kp"]), -1, np.int32)]
    r = S.create_points(_Search(answers), sc["camera"], TS.default_config(), 0, cur, nbs, tables, live, [40, 41, 42, 43, 44, 45], S.NEIGHBOURS)
    assert r["counts"].tolist() == [0, 5, 5, 0] and r["new_slot"].tolist() == [40, 41, 42, 43, 44]
    assert r["new_neighbour"].tolist() == [0, 0, 0, 1, 1] and list(zip(r["new_idx1"].tolist(), r["new_idx2"].tolist())) == [A, B, Cc, D, E]
    assert r["tables"][0][A[0]] == 44 and r["tables"][1][A[1]] == 40 and r["tables"][2][E[1]] == 44       # A's point is observed by its neighbour only
    assert r["tables"][0][B[0]] == 41 and r["tables"][0][D[0]] == 43 and (r["tables"][0] >= 0).sum() == 4
    assert r["new_desc"].tobytes() == cur["desc"][[A[0], B[0], Cc[0], D[0], E[0]]].tobytes() and r["stats"][:, 3].tolist() == [3, 2]
    # truncated behind A, B, C, D: E never happens, so A keeps the current feature
    r = S.create_points(_Search(answers), sc["camera"], TS.default_config(), 0, cur, nbs, tables, live, [40, 41, 42, 43], S.NEIGHBOURS)
    assert r["counts"].tolist() == [0, 5, 4, 1] and r["tables"][0][A[0]] == 40 and r["tables"][2][E[1]] == -1


def test_a_dropped_stereo_candidate_stays_unflagged_for_the_neighbour_phase():
    sc, cur, nbs, answers = _pair_world()
    live = np.zeros(64, np.uint8)
    tables = [None, None, None]
    cand = np.flatnonzero(cur["has"])
    look = _Search(answers)
    r = S.create_points(look, sc["camera"], TS.default_config(), 0, cur, nbs, tables, live, [50, 51], S.STEREO | S.NEIGHBOURS)
    assert r["counts"][0] == len(cand) and r["counts"][2] == 2 and r["new_idx1"].tolist() == cand[:2].tolist()
    assert np.flatnonzero(look.seen[0][0]).tolist() == cand[:2].tolist()   # only the two that were given a slot are flagged; no pair is created: the slots ran out
    assert r["counts"][1] == 5 and r["counts"][3] == len(cand) + 5 - 2


def test_remove_clears_repeats_and_purges_stale_entries():
    live = np.zeros(16, np.uint8); live[[2, 3]] = 1
    tables = [np.array([2, 3, 2, 7, -1], np.int32), None, np.array([7, 7, 3], np.int32)]
    out, lv, n = S.remove_points(tables, live, [2, 7, 2])                  # 2 is live and named twice in keyframe 0; 7 is dead: its stale entries go too
    assert out[0].tolist() == [-1, 3, -1, -1, -1] and out[1] is None and out[2].tolist() == [-1, -1, 3] and n == 5
    assert lv.tolist() == [0, 0, 0, 1] + [0] * 12
    kp = S.remove_replay(S.tables_as_points(tables, live), [2])
    assert kp == S.tables_as_points(S.remove_points(tables, live, [2])[0], live)


def test_cull_keeps_the_candidates_order_and_compares_strictly():
    live = np.ones(8, np.uint8)
    tables = [np.array([0, 1, 2, 3], np.int32), np.array([1, 2, 3, 3], np.int32), np.array([2, 3], np.int32), None]
    # observers: slot 0: 1, slot 1: 2, slot 2: 3, slot 3: 3 (twice in keyframe 1 counts once), slot 5: 0
    culled, out, lv, n = S.cull_points(tables, live, [3, 5, 1, 0, 2], 3)
    assert culled.tolist() == [5, 1, 0]                                    # 2 and 3 have exactly three observers: not fewer
    assert out[0].tolist() == [-1, -1, 2, 3] and out[1].tolist() == [-1, 2, 3, 3] and n == 3 and lv.tolist() == [0, 0, 1, 1, 1, 0, 1, 1]


# ---- every scene: against the sequential reference, and what it must show ---------------------------------------------------

FOUND = {"t1_grid": (175, 65, 0), "t3_nodes": (185, 130, 29), "t10_grid": (222, 360, 121), "t10_nodes_current_only": (179, 275, 88),
         "t10_nodes": (186, 286, 97), "large": (406, 336, 72)}            # S, N, current features created more than once


@pytest.mark.parametrize("name", list(W.CASES))
def test_spec_equals_the_reference_replay_and_scene_shows_every_case(oracle, name):
    w = W.world(name)
    sc = w["scene"]
    r = W.expected(oracle, name)
    kp = S.create_replay(sc["current"], sc["neighbours"], w["tables"], w["live"], w["free_slots"], r["created_pairs"])
    assert kp == S.tables_as_points(r["tables"], S.live_after(w["live"], r))
    i1 = r["new_idx1"][r["new_neighbour"] >= 0]
    per = np.bincount(i1, minlength=1)
    assert (int(r["counts"][0]), int(r["counts"][1]), int((per > 1).sum())) == FOUND[name] and r["counts"][3] == 0
    overwritten = sum(int((a[a != b] >= 0).sum()) for a, b in zip(w["tables"], r["tables"]) if a is not None)
    T = len(sc["neighbours"])
    if T >= 3:
        assert (per > 1).any() and overwritten >= 1
    if T == 10:
        assert per.max() == 5
    for t in range(T):                                                     # no feature of a neighbour is matched twice
        i2 = r["new_idx2"][r["new_neighbour"] == t]
        assert len(set(i2.tolist())) == len(i2)
    near = sum(1 for e in r["evaluated"] if e[6] <= MARGIN)
    assert near <= 1 and near <= 0.01 * len(r["evaluated"])
    assert any(t is None for t in w["tables"][1:]) and (name != "t10_grid" or w["tables"][0] is None)
    assert not set(w["free_slots"].tolist()) & {int(s) for t in w["tables"] if t is not None for s in t.tolist()} and not w["live"][w["free_slots"]].any()
    assert len(set(w["free_slots"].tolist())) == len(w["free_slots"]) and (np.diff(w["free_slots"]) < 0).any()
    if name == "large":
        assert len(sc["current"]["kp"]) > W.CHUNK and (r["new_idx1"][r["new_neighbour"] < 0] >= W.CHUNK).any()


def test_remove_and_cull_equal_the_replay_after_creation(oracle):
    w = W.world("t3_nodes")
    r = W.expected(oracle, "t3_nodes")
    live = S.live_after(w["live"], r)
    cand = r["new_slot"][::-1].copy()
    culled, out, lv, n = S.cull_points(r["tables"], live, cand, 2)
    assert 0 < len(culled) < len(cand) and n == len(culled)                # a point observed by its neighbour only has one observer, each named once
    assert S.remove_replay(S.tables_as_points(r["tables"], live), culled) == S.tables_as_points(out, lv)
    assert lv.sum() == live.sum() - len(culled)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_and_header_as_c(pkg, tmp_path):
    L = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("map_create_points_device", "map_create_points", "map_remove_points", "map_cull_points"):
        assert hasattr(pkg.Handle, m), m
    assert L.orbx_abi_version() == 2 and (pkg.MAP_CREATE_STEREO, pkg.MAP_CREATE_NEIGHBOURS) == (1, 2)
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "orbx.h"\n'
                   'int (*f1)(orbx_keyframe*, const orbx_map_points*, const int*) = orbx_keyframe_set_map_point_slots_device;\n'
                   'int (*f2)(orbx_handle*, const orbx_camera*, const orbx_triangulation_config*, int, orbx_map_points*, orbx_keyframe*, orbx_keyframe* const*, int, int, '
                   'const int*, int, int*, int*, int*, int*, int*, double*, uint8_t*, int*) = orbx_map_create_points_device;\n'
                   'int (*f3)(orbx_handle*, const orbx_camera*, const orbx_triangulation_config*, int, orbx_map_points*, orbx_keyframe*, orbx_keyframe* const*, int, int, '
                   'const int*, int, int*, int*, int*, int*, int*, double*, int*) = orbx_map_create_points;\n'
                   'int (*f4)(orbx_handle*, orbx_map_points*, int, const orbx_keyframe* const*, int, const int*, int*) = orbx_map_remove_points;\n'
                   'int (*f5)(orbx_handle*, orbx_map_points*, int, const orbx_keyframe* const*, int, const int*, int, int*, int*) = orbx_map_cull_points;\n'
                   'int phases = ORBX_MAP_CREATE_STEREO | ORBX_MAP_CREATE_NEIGHBOURS;\n'
                   'int main(void) {\n  void* p[] = {%s};\n  printf("%%zu %%d\\n", sizeof(p) / sizeof(p[0]), phases);\n  return 0;\n}\n'
                   % ", ".join("(void*)%s" % s for s in NEW_SYMBOLS))
    obj = tmp_path / "decl.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert obj.exists()


def test_null_handles_are_refused_without_a_device(pkg):
    L = pkg.load_library()
    one = np.zeros(4, np.int32)
    v = one.ctypes.data_as(C.c_void_p)
    assert L.orbx_keyframe_set_map_point_slots_device(None, None, v) == -1
    assert L.orbx_map_create_points_device(None, None, None, 0, None, None, None, 0, 3, v, 0, v, v, v, v, v, v, v, v) == -1
    assert L.orbx_map_create_points(None, None, None, 0, None, None, None, 0, 3, v, 0, v, v, v, v, v, v, v) == -1
    assert L.orbx_map_remove_points(None, None, 0, None, 0, v, v) == -1
    assert L.orbx_map_cull_points(None, None, 0, None, 0, v, 3, v, v) == -1
    assert one.tolist() == [0, 0, 0, 0]


def test_map_create_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_driver(str(tmp_path)))
