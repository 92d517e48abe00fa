"""CPU checks of fuse and merge on the resident map: the specification (tests/map_fuse_spec.py) against hand-made answers, one per
rule; against a literal sequential replay of the reference on worlds that meet the four agreement conditions; what every scene is
required to show; the new ABI as a C compiler reads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_fuse_scenes as F
import map_fuse_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
NEW_SYMBOLS = ("orbx_keyframe_get_map_point_slots", "orbx_map_fuse_device", "orbx_map_fuse", "orbx_map_search_in_neighbors")


def _fuse(tables, live, src, tgt, hits):
    """hits: {(slot, keyframe): feature} — what the search finds"""
    tables = S.Tables(tables, [len(t) for t in tables])
    cap = len(live)
    pos = np.arange(cap, dtype=np.float64).reshape(-1, 1).repeat(3, 1)      # (a point's position names its slot)

    def search(p, d, tg):
        return np.array([[hits.get((int(x[0]), t), -1) for t in tg] for x in p], np.int32).reshape(len(p), len(tg))
    return S.fuse(tables, live, pos, np.zeros((cap, 32), np.uint8), src, tgt, search)


def _t(*rows):
    return [np.array(r, np.int32) for r in rows]


def build_driver(tmp):
    exe = os.path.join(tmp, "map_fuse_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_fuse_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


# ---- the specification on hand-made answers --------------------------------------------------------------------------------

def test_association_and_the_observed_skip():
    live = np.ones(8, np.uint8)
    r = _fuse(_t([3, 4], [-1, 4, -1]), live, [0], [1], {(3, 1): 2, (4, 1): 0})
    assert r["list_slot"].tolist() == [3, 4] and r["match"].tolist() == [[2], [-1]] and r["skipped"] == 1        # 4 is observed by the target
    assert r["tables"][1].tolist() == [-1, 4, 3] and r["counts"].tolist() == [2, 1, 1, 0] and len(r["goner"]) == 0


def test_more_observers_keep_and_a_tie_goes_to_the_earlier_in_the_list():
    live = np.ones(8, np.uint8)
    # 3 (one observer) meets 5 (two): 5 keeps, and keyframe 0's feature is re-pointed
    r = _fuse(_t([3], [5], [5]), live, [0], [1], {(3, 1): 0})
    assert r["goner"].tolist() == [3] and r["keeper"].tolist() == [5] and [t.tolist() for t in r["tables"]] == [[5], [5], [5]]
    # one observer each: the projected point keeps
    r = _fuse(_t([3], [5]), live, [0], [1], {(3, 1): 0})
    assert r["goner"].tolist() == [5] and r["keeper"].tolist() == [3] and [t.tolist() for t in r["tables"]] == [[3], [3]]
    # two points of the list, tied, claim one feature: the earlier one keeps; the later is a goner although the list holds both
    r = _fuse(_t([6, 2], [-1]), live, [0], [1], {(6, 1): 0, (2, 1): 0})
    assert r["goner"].tolist() == [2] and r["keeper"].tolist() == [6] and [t.tolist() for t in r["tables"]] == [[6, -1], [6]]
    assert r["counts"].tolist() == [2, 2, 1, 1]
    # tied members outside the list come after those in it, by ascending slot: 7 and 1 are named, 4 projects
    r = _fuse(_t([4], [7], [1]), live, [0], [1, 2], {(4, 1): 0, (4, 2): 0})
    assert r["keeper"].tolist() == [4, 4] and r["goner"].tolist() == [1, 7]
    r = _fuse(_t([4], [7], [1], [7, 1]), live, [0], [1, 2], {(4, 1): 0, (4, 2): 0})                   # 7 and 1: two observers each
    assert r["keeper"].tolist() == [1, 1] and r["goner"].tolist() == [4, 7] and r["tables"][3].tolist() == [-1, 1]       # (the keeper's own feature stays)


def test_the_keepers_own_feature_is_preferred_and_else_the_lowest():
    live = np.ones(8, np.uint8)
    # keyframe 2 names both 3 (the keeper, at feature 2) and 5 (the goner, at feature 0): the keeper's feature stays, the other is erased
    r = _fuse(_t([3], [5], [5, -1, 3], [3]), live, [0], [1], {(3, 1): 0})
    assert r["keeper"].tolist() == [3] and r["tables"][2].tolist() == [-1, -1, 3] and r["tables"][1].tolist() == [3]
    # keyframe 2 names the goner twice and not the keeper: the lowest of the two gets the keeper
    r = _fuse(_t([3], [5], [-1, 5, 5], [3], [3]), live, [0], [1], {(3, 1): 0})
    assert r["tables"][2].tolist() == [-1, 3, -1]
    # a class that names and claims in one keyframe: 3 claims feature 0 of keyframe 2, which names 5 at feature 1; 5 keeps
    r = _fuse(_t([3], [5], [-1, 5], [5]), live, [0], [1, 2], {(3, 1): 0, (3, 2): 0})
    assert r["keeper"].tolist() == [5] and r["tables"][2].tolist() == [-1, 5] and r["tables"][0].tolist() == [5] and r["counts"][2] == 0
    assert r["stats"]["names_and_claims"] == 1
    # ... and where 3 keeps, the lowest feature of the two gets it: the claimed one
    r = _fuse(_t([3], [5], [-1, 5], [3], [3]), live, [0], [1, 2], {(3, 1): 0, (3, 2): 0})
    assert r["keeper"].tolist() == [3] and r["tables"][2].tolist() == [3, -1] and r["counts"][2] == 1


def test_a_dead_entry_is_overwritten_and_a_keyframe_outside_is_untouched():
    live = np.ones(8, np.uint8); live[6] = 0
    r = _fuse(_t([3], [6, 6]), live, [0], [1], {(3, 1): 1})
    assert r["tables"][1].tolist() == [6, 3] and r["counts"].tolist() == [1, 1, 1, 0]
    # the caller leaves keyframe 2, which names the goner, out of kfs[]: its table is not the call's to change
    live = np.ones(8, np.uint8)
    outside = np.array([5], np.int32)
    r = _fuse(_t([3], [5]), live, [0], [1], {(3, 1): 0})
    assert r["goner"].tolist() == [5] and len(r["tables"]) == 2 and outside.tolist() == [5]
    # a target without a table gets one; another keyframe without one stays so
    tabs = S.Tables([np.array([3], np.int32), None, None], [1, 2, 2])
    r = S.fuse(tabs, live, np.zeros((8, 3)), np.zeros((8, 32), np.uint8), [0], [1], lambda p, d, tg: np.array([[1]], np.int32))
    assert r["tables"][1].tolist() == [-1, 3] and r["tables"][2] is None
    # nothing to do
    assert _fuse(_t([3], [5]), live, [], [1], {})["counts"].tolist() == [0, 0, 0, 0]
    assert _fuse(_t([3], [5]), live, [0], [], {})["counts"].tolist() == [1, 0, 0, 0]


# ---- against the sequential reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_spec_equals_the_reference_replay_under_the_agreement_conditions(oracle, seed):
    sc = F.agree_world(seed)
    search = F.oracle_search(oracle, sc)
    tgt = [1, 2, 3]
    r = S.fuse(sc["tables"], sc["live"], sc["positions"], sc["desc"], [0], tgt, search)
    tables, removed, fused, obs_added = S.reference_replay(sc["tables"], sc["live"], sc["positions"], sc["desc"], [0], tgt, search)
    # the conditions themselves: classes of at most two, no feature matched twice, the projected point keeps, counts more than n_tgt apart
    st = r["stats"]
    assert max(len(m) for m in st["members"].values()) == 2 and all(len(j) == 1 for j in st["claims"].values())
    flat = [(t, int(f)) for row in r["match"] for t, f in enumerate(row) if f >= 0]
    assert len(flat) == len(set(flat)) and all(int(k) in st["place"] and int(g) not in st["place"] for g, k in zip(r["goner"], r["keeper"]))
    assert all(abs(int(st["nobs"][g]) - int(st["nobs"][k])) > len(tgt) for g, k in zip(r["goner"], r["keeper"]))
    assert all((a is None and b is None) or a.tobytes() == b.tobytes() for a, b in zip(r["tables"], tables))
    assert sorted(removed) == r["goner"].tolist() and fused == r["counts"][3] >= 30 and obs_added == r["counts"][2] >= 60


# ---- what every scene shows ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2])
def test_scenes_show_every_case(oracle, seed):
    sc = F.world(seed)
    r = S.fuse(sc["tables"], sc["live"], sc["positions"], sc["desc"], [F.CUR], F.TGT, F.oracle_search(oracle, sc))
    got = F.scene_counts(sc, r, F.TGT)
    assert all(got[k] >= v for k, v in F.REQUIRED.items()), got
    counts = sc["tables"].counts
    assert counts[6] == 2100 and counts[8] == 0 and sc["tables"][7] is None and r["counts"][0] % 128 != 0 and 350 < sc["live"].sum() < 450
    assert (r["match"][:, F.TGT.index(6)] >= 2048).any()                   # a match past the first chunk of the large keyframe
    assert (r["match"][:, F.TGT.index(7)] >= 0).any()                      # an association in the keyframe without a table
    x = S.search_in_neighbors(sc["tables"], sc["live"], sc["positions"], sc["desc"], F.CUR, F.ALL_NB, F.oracle_search(oracle, sc))
    assert x["b"]["counts"][1] >= 20 and x["b"]["counts"][3] >= 3 and not set(x["affected"].tolist()) & set(x["a"]["goner"].tolist() + x["b"]["goner"].tolist())


# ---- the ABI ---------------------------------------------------------------------------------------------------------------

def test_new_symbols_and_header_as_c(pkg, tmp_path):
    L = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("map_fuse_device", "map_fuse", "map_search_in_neighbors"):
        assert hasattr(pkg.Handle, m), m
    assert hasattr(pkg.KeyFrame, "get_map_point_slots") and L.orbx_abi_version() == 2
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "orbx.h"\n'
                   'int (*f1)(const orbx_keyframe*, int*) = orbx_keyframe_get_map_point_slots;\n'
                   'int (*f2)(orbx_handle*, const orbx_camera*, orbx_map_points*, int, orbx_keyframe* const*, int, const int*, int, const int*, double, unsigned, int, int*, '
                   'int*, int*, int*, int*) = orbx_map_fuse_device;\n'
                   'int (*f3)(orbx_handle*, const orbx_camera*, orbx_map_points*, int, orbx_keyframe* const*, int, const int*, int, const int*, double, unsigned, int, int*, '
                   'int*, int*, int*, int*) = orbx_map_fuse;\n'
                   'int main(void) {\n  void* p[] = {%s};\n  printf("%%zu\\n", sizeof(p) / sizeof(p[0]));\n  return 0;\n}\n' % ", ".join("(void*)%s" % s for s in NEW_SYMBOLS))
    obj = tmp_path / "decl.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert obj.exists()


def test_null_handles_are_refused_without_a_device(pkg):
    L = pkg.load_library()
    one = np.zeros(4, np.int32)
    v = one.ctypes.data_as(C.c_void_p)
    assert L.orbx_keyframe_get_map_point_slots(None, v) == -1
    assert L.orbx_map_fuse_device(None, None, None, C.c_int(0), None, C.c_int(0), None, C.c_int(0), None, C.c_double(1.0), C.c_uint(50), C.c_int(0), v, v, v, v, v) == -1
    assert L.orbx_map_fuse(None, None, None, C.c_int(0), None, C.c_int(0), None, C.c_int(0), None, C.c_double(1.0), C.c_uint(50), C.c_int(0), v, v, v, v, v) == -1
    assert one.tolist() == [0, 0, 0, 0]


def test_map_fuse_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_driver(str(tmp_path)))
