"""The maps of tests/global_map_cases.py on the CPU: conditions on the REFERENCE alone (the oracle's global_ba_solve_schur), checked without
the code under test.  They are what lets tests/test_global_map_gpu.py demand equal iteration counts with the project's tolerances,
unchanged: every case runs its 10 iterations, every accept / reject decision is at least 1e-3 (relative) away from a tie, so that no
rounding difference can flip it, and the points behind the cameras come back as they went in.

Measured (N observations, seconds = one oracle solve on one thread, decisions A = accepted, r = rejected, margin = smallest
|trial - current| / current over the decisions):

case         K    n     M     behind  N      seconds  decisions   margin
k129         129  774   2612  20      6343   0.9      rrrArArrAr  0.061
k160         160  960   3212  24      7989   1.4      rrrArArrAr  0.025
k171         171  1026  3412  24      8303   1.7      rrrArrArAr  0.025
k257         257  1542  3912  30      10498  6.0      rrrArrAArr  0.035
k200_banded  200  1200  4000  24      7536   2.3      rrrArrArrr  0.052
(M counts the 12 far points of the coupled cases.)

Also here: the library exports the new entry points and api.py binds them.
"""
import os
import subprocess

import numpy as np
import pytest

import global_map_cases as G
from orientation_cases import lm_margin

MARGIN = 1e-3
NEW_SYMBOLS = ("orbx_ba_solve_global_map", "orbx_ba_solve_global_map_obs32", "orbx_ba_solve_global_map_obs32_device", "orbx_ba_global_map_max_keyframes",
               "orbx_map_collect_global_device", "orbx_map_collect_global", "orbx_map_global_ba")


@pytest.mark.parametrize("name", list(G.CASES))
def test_reference_pins_the_answer(oracle, name):
    w = G.case(name)
    banded, kw, n_behind = G.CASES[name]
    K = kw["K"]
    assert len(w["poses_cw"]) == K > 128 and len(w["fixed_cw"]) == 1 and len(w["behind"]) == n_behind
    assert len(w["points"]) == kw["M"] + (0 if banded else G.L.COMMON_POINTS)
    o = G.oracle_answer(oracle, name)
    steps = "".join("A" if t[3] < t[0] else "r" for t in o["trace"])
    margin = lm_margin(o["trace"])
    print("%s: K %d, n %d, M %d, N %d, iterations %d, decisions %s, margin %.3f, error %.3f -> %.3f" % (
        name, K, 6 * K, len(w["points"]), len(w["obs"]), o["iterations"], steps, margin, o["initial_error"], o["final_error"]))
    assert o["iterations"] == 10 and len(o["trace"]) == 10 and np.all(o["trace"][:, 3] > 0)      # ten decisions, none skipped by a stop rule
    assert margin >= MARGIN
    assert "A" in steps and o["final_error"] < o["initial_error"]
    assert np.array_equal(o["points"][w["behind"]], w["points"][w["behind"]])
    seen = np.bincount(w["obs"]["mp_idx"], minlength=len(w["points"]))
    assert (seen[w["behind"]] > 0).sum() >= 10                                                 # (observed: the solver meets them)
    deg = G.L.kf_obs(w)
    assert deg.min() >= 1
    d = G.behind_depths(w)
    assert len(d) >= 20 and np.all(d < -1.0)                                                   # behind every camera that observes them
    pairs = np.zeros((K, K), bool)                                                             # keyframe pairs that share a point
    o_ = w["obs"][w["obs"]["kf_idx"] >= 0]
    order = np.argsort(o_["mp_idx"], kind="stable")
    mp, kf = o_["mp_idx"][order], o_["kf_idx"][order]
    for s, e in zip(np.flatnonzero(np.r_[True, mp[1:] != mp[:-1]]), np.flatnonzero(np.r_[mp[1:] != mp[:-1], True]) + 1):
        k = kf[s:e]
        pairs[np.ix_(k, k)] = True
    assert pairs.all() != banded                                                               # coupled: every pair; banded: true zero blocks


def test_big_map_shape():
    w = G.case("big")
    assert len(w["poses_cw"]) == 1025 and len(w["points"]) == G.BIG["M"] and len(w["behind"]) == G.BIG_BEHIND
    assert G.L.kf_obs(w).min() >= 1
    d = G.behind_depths(w)
    assert len(d) >= 40 and np.all(d < -1.0)                                    # behind every camera that observes them


def test_library_exports_the_whole_map_solver(pkg):
    L = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in pkg.ABI_SYMBOLS, s
    for m in ("ba_solve_global_map", "ba_solve_global_map_obs32", "ba_solve_global_map_obs32_device", "ba_global_map_max_keyframes",
              "map_collect_global_device", "map_collect_global", "map_global_ba"):
        assert callable(getattr(pkg.Handle, m))
    assert L.orbx_ba_global_map_max_keyframes() >= 1024


def test_cpp_mirrors_compile_link_and_run(pkg, tmp_path):
    """orbx::solve_global_ba_map, map_collect_global[_device], map_global_ba and run_global_ba(..., whole_map) built with g++ against the
    library (tests/cpp/global_ba_map_driver.cpp)"""
    pkg.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "orb-slam3-rust_amd")
    exe = os.path.join(str(tmp_path), "global_ba_map_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "global_ba_map_driver.cpp"), "-o", exe,
                    "-L", libdir, "-lorbx_hip", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "GLOBAL_BA_MAP_DRIVER_OK %d" % pkg.load_library().orbx_ba_global_map_max_keyframes() in r.stdout, (r.stdout, r.stderr)
