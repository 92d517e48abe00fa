"""CPU checks of the inertial local-BA window collected from the resident map: the specification (tests/inertial_collect_spec.py) against
the restatement of the reference's collect_inertial_ba_data (oracle/local_mapper_ref.py) and against hand-made edge cases, that the stereo
flag matters to the solve, the scenes the GPU tests solve (tests/inertial_collect_scenes.py), the new ABI as a C compiler reads it and
the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import ba_collect_scenes as B
import covisibility_scenes as V
import inertial_collect_scenes as I
import inertial_collect_spec as S
import inertial_edge_windows as W
import orientation_cases as OC
from oracle import local_mapper_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
NEW_SYMBOLS = ("orbx_ba_solve_inertial_obs32", "orbx_ba_solve_inertial_obs32_device", "orbx_map_collect_inertial_window_device",
               "orbx_map_collect_inertial_window", "orbx_map_local_inertial_ba")


def build_driver(tmp):
    exe = os.path.join(tmp, "inertial_collect_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "inertial_collect_driver.cpp"),
                    "-o", exe, "-L", LIBDIR, "-lorbx_hip", "-L", ROCM_LIB, "-lamdhip64", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ROCM_LIB], check=True)
    return exe


def _against_reference(tables, xy, has, live, chain):
    got = S.collect(tables, xy, has, live, chain)
    m, cur = I.reference_map(tables, xy, has, live, chain)
    want = R.collect_inertial_ba_data(m, cur, window_size=len(chain))
    if want is None:
        assert got is None or got["empty"]
        return got, want
    K, F, M, N = got["counts"]
    assert not got["empty"] and K == len(chain) and M > 0
    assert want["opt_kf_ids"] == [100 + k for k in chain]
    assert set(want["mp_ids"]) == set(got["list_slot"].tolist()) and len(want["mp_ids"]) == M                    # P as a set (here also in order)
    assert want["mp_ids"] == got["list_slot"].tolist()
    assert set(want["fixed_kf_poses"]) - {100 + chain[0]} == {100 + int(k) for k in got["fixed_kf"]} and F == 1 + len(got["fixed_kf"])
    assert got["fixed_kf"].tolist() == sorted(got["fixed_kf"].tolist())

    def key(o):
        i = int(o["kf_idx"])
        kf = chain[i] if i >= 1 else chain[0] if i == -1 else int(got["fixed_kf"][-2 - i])
        return (100 + kf, int(got["list_slot"][o["mp_idx"] & ~S.STEREO]), float(o["u"]), float(o["v"]), bool(o["mp_idx"] & S.STEREO), i >= 1)

    assert 0 not in got["obs32"]["kf_idx"]                                                                        # the anchor's observations are fixed
    mine = sorted(key(o) for o in got["obs32"])
    theirs = sorted((o["kf_id"], o["mp_id"], o["uv"][0], o["uv"][1], o["is_stereo"], o["is_kf_in_window"]) for o in want["visual_observations"])
    assert mine == theirs and len(mine) == N
    pos = {100 + k: i for i, k in enumerate(chain)}                                                                # the edges' window indices: (i, i + 1)
    assert [(pos[e["kf_i_id"]], pos[e["kf_j_id"]]) for e in want["imu_edges"]] == [(i, i + 1) for i in range(K - 1)]
    return got, want


@pytest.mark.parametrize("seed,n_kfs", [(1, 3), (2, 11), (3, 64)])
def test_spec_equals_the_reference_restatement(seed, n_kfs):
    """world(seed, n) with its repeats removed: every observation associated once, in both directions; has_point random at 0.5; chains
    are tails of the keyframe list"""
    tables, counts, live = V.world(seed, n_kfs)
    tables = B.once(tables)
    xy = B.keypoints(seed, counts)
    has = I.has_points(seed, counts)
    seen = stereo = fixed = 0
    for chain in I.tails(n_kfs):
        got, want = _against_reference(tables, xy, has, live, chain)
        if want is not None:
            seen += 1; fixed += int(got["counts"][1]) > 1
            st = (got["obs32"]["mp_idx"] & S.STEREO) != 0
            stereo += bool(st.any() and not st.all())
    assert seen > 0 and stereo > 0
    if n_kfs >= 11:
        assert fixed > 0 and len(I.tails(n_kfs)) == 3


def _xy(tables):
    return [np.arange(2 * (0 if t is None else len(t)), dtype=np.float32).reshape(-1, 2) + 100 * k for k, t in enumerate(tables)]


def _none(tables):
    return [None] * len(tables)


def test_repeats_inside_a_keyframe_give_one_observation_each():
    live = np.ones(16, np.uint8)
    tables = [np.array([5, 5, 7], np.int32), np.array([7, 7, 7, 9], np.int32)]
    has = [np.array([1, 0, 1], np.uint8), np.array([0, 1, 0, 1], np.uint8)]
    r = S.collect(tables, _xy(tables), has, live, [0, 1])
    assert r["counts"].tolist() == [2, 1, 3, 7] and r["list_slot"].tolist() == [5, 7, 9]
    assert r["obs32"]["kf_idx"].tolist() == [-1, -1, -1, 1, 1, 1, 1]
    assert r["obs32"]["mp_idx"].tolist() == [0 | S.STEREO, 0, 1 | S.STEREO, 1, 1 | S.STEREO, 1, 2 | S.STEREO]
    assert r["obs32"]["u"].tolist() == [0.0, 2.0, 4.0, 100.0, 102.0, 104.0, 106.0]                             # each observer's features in index order
    assert S.collect(tables, _xy(tables), has, live, [1, 0])["list_slot"].tolist() == [7, 9, 5]               # first seen walking the chain [1, 0]


def test_dead_and_minus_one_entries_are_skipped():
    live = np.ones(16, np.uint8); live[3] = 0
    tables = [np.array([-1, 3, 4, -1, 6], np.int32), np.array([3, 4, -1], np.int32), np.array([3, -1], np.int32), np.array([6, 3], np.int32)]
    r = S.collect(tables, _xy(tables), _none(tables), live, [0, 1])
    assert r["counts"].tolist() == [2, 2, 2, 4] and r["list_slot"].tolist() == [4, 6] and r["fixed_kf"].tolist() == [3]
    assert r["obs32"]["kf_idx"].tolist() == [-1, -1, 1, -2] and r["obs32"]["mp_idx"].tolist() == [0, 1, 0, 1]
    assert r["obs32"]["v"].tolist() == [5.0, 9.0, 103.0, 301.0]                                                # keyframe 2 names only the dead slot: no observer


def test_an_anchor_without_a_table_still_anchors():
    live = np.ones(16, np.uint8)
    tables = [None, np.array([1, 2], np.int32), np.array([2], np.int32)]
    xy = _xy(tables); xy[0] = np.zeros((5, 2), np.float32)
    r = S.collect(tables, xy, _none(tables), live, [0, 1])
    assert r["counts"].tolist() == [2, 2, 2, 3] and r["fixed_kf"].tolist() == [2] and r["obs32"]["kf_idx"].tolist() == [1, 1, -2]
    m, cur = I.reference_map(tables, xy, _none(tables), live, [0, 1])
    assert len(R.collect_inertial_ba_data(m, cur, 2)["visual_observations"]) == 3


def test_a_chain_of_every_keyframe_has_no_other_observer():
    live = np.ones(16, np.uint8)
    tables = [np.array([1, 2], np.int32), np.array([2, 3], np.int32), np.array([3, 1], np.int32)]
    r = S.collect(tables, _xy(tables), _none(tables), live, [0, 1, 2])
    assert r["counts"].tolist() == [3, 1, 3, 6] and len(r["fixed_kf"]) == 0 and r["obs32"]["kf_idx"].tolist() == [-1, -1, 1, 1, 2, 2]


def test_a_point_seen_only_by_the_anchor_and_a_fixed_keyframe():
    live = np.ones(16, np.uint8)
    tables = [np.array([9, 1], np.int32), np.array([1], np.int32), np.array([9], np.int32)]
    has = [np.array([1, 0], np.uint8), None, np.array([1], np.uint8)]
    r = S.collect(tables, _xy(tables), has, live, [0, 1])
    assert r["counts"].tolist() == [2, 2, 2, 4] and r["list_slot"].tolist() == [9, 1] and r["fixed_kf"].tolist() == [2]
    assert r["obs32"]["kf_idx"].tolist() == [-1, -1, 1, -2] and r["obs32"]["mp_idx"].tolist() == [0 | S.STEREO, 1, 1, 0 | S.STEREO]
    w = S.widen(r["obs32"], 2)                                                                                  # point 0: no observation by a window keyframe
    assert w["kf_idx"].tolist() == [-1, -1, 1, -1] and w["fixed_idx"].tolist() == [0, 0, -1, 1] and w["_pad"].tolist() == [1, 0, 0, 1]
    assert w["mp_idx"].tolist() == [0, 1, 1, 0]


def test_a_chain_listed_in_descending_position():
    live = np.ones(16, np.uint8)
    tables = [np.array([4], np.int32), np.array([1, 2], np.int32), np.array([2, 3], np.int32), np.array([3, 4], np.int32)]
    r = S.collect(tables, _xy(tables), _none(tables), live, [3, 2, 1])
    assert r["counts"].tolist() == [3, 2, 4, 7] and r["list_slot"].tolist() == [3, 4, 2, 1] and r["fixed_kf"].tolist() == [0]
    assert r["obs32"]["kf_idx"].tolist() == [-1, -1, 1, 1, 2, 2, -2] and r["obs32"]["mp_idx"].tolist() == [0, 1, 2, 0, 3, 2, 1]
    _against_reference(tables, _xy(tables), _none(tables), live, [3, 2, 1])


def test_a_chain_of_one_and_a_chain_without_points_are_empty():
    live = np.ones(16, np.uint8)
    tables = [np.array([1, 2], np.int32), np.array([-1], np.int32), None, np.array([1], np.int32)]
    xy = _xy(tables); xy[2] = np.zeros((3, 2), np.float32)
    assert S.collect(tables, xy, _none(tables), live, [0]) is None
    m, cur = I.reference_map(tables, xy, _none(tables), live, [0])
    assert R.collect_inertial_ba_data(m, cur, 1) is None                                                        # :940-942
    e = S.collect(tables, xy, _none(tables), live, [1, 2])
    assert e["empty"] and e["counts"].tolist() == [2, 1, 0, 0] and len(e["fixed_kf"]) == 0
    m, cur = I.reference_map(tables, xy, _none(tables), live, [1, 2])
    assert R.collect_inertial_ba_data(m, cur, 2) is None                                                        # :946-948


def test_the_stereo_flag_matters_to_the_solve(pkg):
    """the oracle with every stereo flag cleared against the flagged solve: a solver that ignored the bit cannot pass the 1e-6 parity bar"""
    w = pkg.synth.inertial_window(W.SEEDS[0], 5, 60, pkg.BA_OBS)
    assert 0 < (w["obs"]["_pad"] & 1).sum() < len(w["obs"])
    flagged = W.oracle(w)
    clear = dict(w); clear["obs"] = w["obs"].copy(); clear["obs"]["_pad"] = 0
    plain = W.oracle(clear)
    diff = max(W.rel(plain[k], flagged[k]) for k in W.OUTPUTS)
    print("flag cleared vs flagged: %.3e = %.1f x the 1e-6 bar; final error %.6f vs %.6f" % (diff, diff / 1e-6, plain["final_error"], flagged["final_error"]))
    assert diff > 100 * 1e-6


def test_widen_equals_the_mirror_and_its_inverse(pkg):
    w = pkg.synth.keypoint_precision(pkg.synth.inertial_window(3, 4, 40, pkg.BA_OBS, n_fixed=2))
    o32 = pkg.ba_obs_to_obs32(w["obs"], 2, inertial=True)
    assert o32.dtype == pkg.BA_OBS32 == S.BA_OBS32 and pkg.BA_OBS32_STEREO == S.STEREO
    assert ((o32["mp_idx"] & S.STEREO) != 0).tolist() == ((w["obs"]["_pad"] & 1) != 0).tolist() and (o32["mp_idx"] & S.STEREO).any()
    assert S.widen(o32, 2).tobytes() == np.ascontiguousarray(w["obs"], S.BA_OBS).tobytes()
    assert (pkg.ba_obs_to_obs32(w["obs"], 2)["mp_idx"] == w["obs"]["mp_idx"]).all()                            # the visual form carries no flag


@pytest.mark.parametrize("K", [5, 11])
def test_inertial_scene_is_what_it_claims_and_its_seed_is_the_first(K):
    seed = I.SCENE_SEEDS[K]
    assert I.first_seed(K) == seed
    sc, win, c, o = I.solved_scene(seed, K)
    Kc, F, M, N = (int(x) for x in c["counts"])
    assert Kc == K and F == 3 and c["fixed_kf"].tolist() == [0, 1] and sc["chain"] == list(range(2, K + 2)) and M >= W.POINTS[K] * 0.85 and N > 3 * M
    st = (c["obs32"]["mp_idx"] & S.STEREO) != 0
    assert 0.3 < st.mean() < 0.7
    assert all((t == -1).sum() == 3 and (sc["store"].live[t[t >= 0]] == 0).sum() == 2 for t in sc["tables"])     # distractors in every keyframe
    assert OC.lm_margin(o["trace"]) >= W.MARGIN and o["iterations"] > 0 and o["final_error"] < o["initial_error"]
    assert 0 not in win["obs"]["kf_idx"] and (win["obs"]["kf_idx"] >= 1).any()


def test_new_symbols_and_header_as_c(pkg, tmp_path):
    L = pkg.load_library()
    assert L.orbx_abi_version() == 2
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("ba_solve_inertial_obs32", "ba_solve_inertial_obs32_device", "map_collect_inertial_window_device", "map_collect_inertial_window",
              "map_local_inertial_ba"):
        assert hasattr(pkg.Handle, m), m
    src = tmp_path / "decl.c"
    src.write_text('#include <stdio.h>\n#include "orbx.h"\n#if ORBX_ABI_VERSION != 2 || ORBX_BA_OBS32_STEREO != 0x40000000\n#error "ABI"\n#endif\n'
                   'int main(void) {\n  void* p[] = {%s};\n  printf("%%zu %%zu\\n", sizeof(p) / sizeof(p[0]), sizeof(orbx_ba_obs32));\n'
                   '  return 0;\n}\n' % ", ".join("(void*)%s" % s for s in NEW_SYMBOLS))
    obj = tmp_path / "decl.o"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert obj.exists()


def test_inertial_collect_driver_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_driver(str(tmp_path)))
