"""The windows of tests/large_ba_windows.py on the CPU: 57 to 128 optimised keyframes (visual, global), 23 to 51 (inertial) — the sizes at
which the per-panel reduced solve takes its strided and second-pass paths.  Conditions on the inputs and on the REFERENCE alone, checked
without the code under test, as tests/test_ba_covis_cpu.py does for the smaller windows; tests/test_ba_large_gpu.py then compares with
the tolerances of tests/test_ba_gpu.py, test_global_ba.py and test_inertial_ba.py, unchanged.

Per visual and global case: the oracle's Schur form (global_ba_solve_schur for the global ones) on the shuffled array and on the reversed
one.  Required: the same iteration count, 50 x spread <= 1e-6 on poses and points (covis_windows.rel), 50 x the spread of final_error
<= 1e-8 and of initial_error <= 1e-12, lm_margin >= 1e-9, an accepted step, final_error < initial_error, 20 observations or more on every
optimised keyframe.  Per inertial case: the conditions of covis_windows.inertial_scene (an answer, lm_margin >= 1e-7) and observations
on every keyframe.

Measured (what the tests assert on; F fixed cameras, M points — the last 12 of them seen by every camera —, N observations; seconds =
one oracle solve):

visual   K    n    last   F   M     N      obs per kf    iterations  spread    final_error  initial_error  margin   steps       seconds  seed
                   panel                   min/med/max               spread    spread       spread                  (A / r)
         57   342  6      12  2862  5689   67/82/98      10 10       2.6e-12   2.9e-11      1.6e-15        8.3e-03  AAAArrrrAA  0.12     2
         61   366  14     17  3062  6273   62/83/99      10 10       9.9e-12   1.7e-11      1.7e-15        2.2e-03  AArrAAAArr  0.11     1
         65   390  6      10  3262  6609   69/87/108     10 10       1.7e-13   1.6e-11      2.2e-15        1.8e-02  AArrrrAAAA  0.12     2
         67   402  2      14  3362  6880   71/85/103     10 10       1.2e-12   4.4e-11      6.2e-16        1.7e-02  AArrrAAAAA  0.14     1
         87   522  10     19  4362  9118   68/85/105     10 10       3.0e-12   1.9e-10      3.1e-15        3.1e-03  AAAArrrrAA  0.27     1
         88   528  0      11  4412  9311   74/93/117     10 10       2.8e-10   9.3e-11      2.2e-15        4.2e-02  AAAArrrrrr  0.31     1
         89   534  6      16  4462  9482   59/90/113     10 10       2.2e-16   1.7e-16      5.3e-15        8.8e-02  rrrArArArA  0.30     3
         109  654  14     13  5462  11696  74/96/116     10 10       2.3e-16   2.3e-15      1.6e-15        1.9e-03  rrrArArrAr  0.53     1
         110  660  4      20  5512  11840  70/91/114     10 10       2.7e-10   1.8e-10      1.1e-15        1.4e-02  AArrAArrrr  0.91     1
         128  768  0      15  6412  13735  67/95/128     10 10       3.9e-15   3.5e-15      3.7e-15        1.2e-02  rrrArArArA  1.42     1
global   88   528  0      1   4412  9109   83/101/135    10 10       2.6e-16   1.1e-15      1.9e-15        3.5e-02  rrrArArArA  0.44     1
         128  768  0      1   6412  13597  80/106/129    10 10       3.1e-16   3.8e-15      1.8e-15        1.6e-02  rrrArArArA  1.35     1
(errors: K = 57 4.45 -> 0.70 px, K = 89 5.17 -> 2.61, K = 128 6.72 -> 4.55, global K = 128 5.43 -> 3.82: the accepted steps are large ones.)

inertial K    n    last   M    15 K + 3 M  N     obs per kf     iterations  margin   steps       seconds  seed
                   panel                         min/med/max
         23   345  9      300  1245        6015  247/250/254    10          9.4e-07  AAAAArrrrr  2.3      3
         27   405  5      290  1275        6823  240/244/247    10          3.0e-07  AAAAArrrrr  2.3      1
         28   420  4      290  1290        7065  242/244/247    10          2.2e-07  AAAAAAArAr  2.3      3
         35   525  13     250  1275        7781  200/217/226    10          7.8e-07  AAAArrrrrr  2.1      1
         36   540  12     250  1290        7979  198/217/226    10          1.1e-06  AAAArrrrrr  2.1      1
         44   660  4      210  1290        7688  160/172/177    10          7.4e-07  AAAAAAArAr  1.8      6
         45   675  3      205  1290        7787  150/172/177    10          3.5e-07  AAAArrrArr  1.8      1
         51   765  13     175  1290        7419  119/145/154    10          2.1e-06  AAAArrrrrr  1.5      3
(keyframes dt = 0.08 s apart: at synth.inertial_window's default 0.25 s the last keyframes of a 51-keyframe window see nothing.)

How the seeds were chosen: counting up from 1 until every condition above held — conditions on the reference alone.  Passed over:
visual K = 57 seed 1 and K = 65 seed 1 (the reference's own final_error differs by 1.0e-9 and 1.1e-9 between the array and the
reversed array), K = 89 seeds 1 and 2 (2.5e-7 and 1.2e-7; ten accepted steps out of ten: the loop ends far from the minimum, still
descending fast, as tests/test_ba_covis_cpu.py describes — such a window cannot carry the 1e-8 bound whatever is compared with the
reference); inertial K = 23 seeds 1-2, K = 28 seeds 1-2, K = 44 seeds 1-5, K = 51 seeds 1-2: an accept / reject decision within
7.7e-10 .. 7.2e-8 (relative) of a tie.  Every other case took its first seed.

Why the far points and the inertial sizes 28 and 45.  The corridor alone gives a BANDED reduced system, and the factor of a band is a band:
every tile far from the diagonal holds exact zeros, so the paths this file is about — tile slots 3 to 5 of the panel block, the outer
column-block pairs of the Schur product, the second-pass rows — would multiply zeros, and a kernel that skipped them would pass.  Tried
on an MI355X with variants of the library that only SKIP in-bounds work: with the panel block's slots 3.. left out, the K = 67 window
WITHOUT the far points still passed test_large_visual_parity; with them it fails (final_error off by 1.5e-3), K = 65 passes.  Likewise
slot 4 left out: K = 88 passes, 89 fails (final_error 2.5e-7, points 1.4e-6); slot 5: 109 passes, 110 fails; the second pass over the
rows below a panel: 87 passes, 88 fails; rows 512.. of the backward substitution: 88 passes, 89 fails, inertial 35 passes, 36 fails; the
second pass of the assembly: 57 passes, 61 fails (after one iteration).  The inertial sizes of the table's edges, 27 and 44, reach slots
3 and 5 with the last five of the last keyframe's fifteen states only (n - 400 = 5, n - 656 = 4 rows), which nothing couples to the
first keyframes: both pass with the slot left out.  At 28 and 45 the slot holds a whole keyframe, and both fail with it left out (as do
36 with slot 4 and 51 with slot 5), so those two sizes are cases as well.
"""
import time

import numpy as np
import pytest

import covis_windows as W
import large_ba_windows as L
from orientation_cases import lm_margin

SPREAD_FLOOR = 1e-6
INITIAL_ERROR_TOL, FINAL_ERROR_TOL = 1e-12, 1e-8       # tests/test_ba_gpu.py
MARGIN = 1e-9
MIN_KF_OBS = 20


def measure_visual(oracle, K, global_mode=False, seed=None):
    """The reference's Schur form on the case's shuffled array and on the reversed one -> (measured values, the conditions that fail)"""
    make, solve = (L.global_map, L.oracle_global) if global_mode else (L.visual_window, L.oracle_visual)
    w, r = make(K, "shuffled", seed), make(K, "reversed", seed)
    assert np.array_equal(r["obs"], w["obs"][::-1]) and np.array_equal(r["points"], w["points"])
    t0 = time.perf_counter()
    runs = [solve(oracle, K, "shuffled", seed), solve(oracle, K, "reversed", seed)]
    secs = (time.perf_counter() - t0) / 2
    deg = L.kf_obs(w)
    m = dict(K=K, F=len(w["fixed_cw"]), M=len(w["points"]), N=len(w["obs"]), deg=(int(deg.min()), int(np.median(deg)), int(deg.max())), seconds=secs)
    if any(x is None for x in runs):
        return m, ["the reference answers None"]
    a, b = runs
    fe = [x["final_error"] for x in runs]; e0 = [x["initial_error"] for x in runs]
    steps = "".join("A" if t[3] < t[0] else "r" for t in a["trace"])
    m.update(iterations=[x["iterations"] for x in runs], spread=max(W.rel(a["poses_wc"], b["poses_wc"]), W.rel(a["points"], b["points"])),
             fe_spread=(max(fe) - min(fe)) / min(fe), e0_spread=(max(e0) - min(e0)) / min(e0), margin=min(lm_margin(x["trace"]) for x in runs),
             steps=steps, initial_error=a["initial_error"], final_error=a["final_error"])
    bad = []
    if len(set(m["iterations"])) != 1:
        bad.append("iteration counts %s" % m["iterations"])
    if not 50.0 * m["spread"] <= SPREAD_FLOOR:
        bad.append("spread %.3e" % m["spread"])
    if not 50.0 * m["fe_spread"] <= FINAL_ERROR_TOL:
        bad.append("final_error spread %.3e" % m["fe_spread"])
    if not 50.0 * m["e0_spread"] <= INITIAL_ERROR_TOL:
        bad.append("initial_error spread %.3e" % m["e0_spread"])
    if not m["margin"] >= MARGIN:
        bad.append("margin %.3e" % m["margin"])
    if "A" not in steps:
        bad.append("no accepted step")
    if not a["final_error"] < a["initial_error"]:
        bad.append("final_error %.6f >= initial_error %.6f" % (a["final_error"], a["initial_error"]))
    if deg.min() < MIN_KF_OBS:
        bad.append("a keyframe with %d observations" % deg.min())
    return m, bad


def measure_inertial(oracle, K, seed=None):
    w = L.inertial_window(K, seed)
    t0 = time.perf_counter()
    o = L.oracle_inertial(oracle, K, seed)
    secs = time.perf_counter() - t0
    deg = L.kf_obs(w)
    m = dict(K=K, M=len(w["points"]), N=len(w["obs"]), unknowns=15 * K + 3 * len(w["points"]), deg=(int(deg.min()), int(np.median(deg)), int(deg.max())), seconds=secs)
    if o is None:
        return m, ["the reference answers None"]
    m.update(iterations=o["iterations"], margin=lm_margin(o["trace"]), steps="".join("A" if t[3] < t[0] else "r" for t in o["trace"]),
             initial_error=o["initial_error"], final_error=o["final_error"])
    bad = []
    if not m["margin"] >= W.INERTIAL_MARGIN:
        bad.append("margin %.3e" % m["margin"])
    if deg.min() < 1:
        bad.append("a keyframe without observations")
    return m, bad


def _assert_common_points_couple_every_pair(w):
    """every optimised keyframe observes every one of the far points: no pair of keyframes without a shared point, no tile of the reduced
    system that is zero by structure"""
    o = w["obs"]; K = len(w["poses_cw"])
    c = o[np.isin(o["mp_idx"], w["common"]) & (o["kf_idx"] >= 0)]
    assert len(w["common"]) == L.COMMON_POINTS and np.array_equal(w["common"], np.arange(len(w["points"]) - L.COMMON_POINTS, len(w["points"])))
    assert len(c) == K * L.COMMON_POINTS and len(np.unique(c["mp_idx"].astype(np.int64) * K + c["kf_idx"])) == len(c)


def _line(tag, m):
    return "%s: %s" % (tag, ", ".join("%s %s" % (k, ("%.3e" % v) if isinstance(v, float) else v) for k, v in m.items()))


@pytest.mark.parametrize("K", list(L.VISUAL))
def test_reference_determines_the_visual_answer(oracle, K):
    m, bad = measure_visual(oracle, K)
    print(_line("visual K = %d" % K, m))
    assert not bad, bad
    _assert_common_points_couple_every_pair(L.visual_window(K))
    assert m["K"] == K and 10 <= m["F"] <= 20 and m["M"] == 50 * K + L.COMMON_POINTS and L.last_panel_width(6 * K) == {57: 6, 61: 14, 65: 6, 67: 2, 87: 10, 88: 0, 89: 6, 109: 14, 110: 4, 128: 0}[K]


def test_largest_visual_case_fills_the_k_splits():
    assert len(L.visual_window(128)["points"]) >= 32 * L.KSPLIT_MAX          # ~32 points per k-split: 128 of them from M = 4096


@pytest.mark.parametrize("K", list(L.GLOBAL))
def test_reference_determines_the_global_answer(oracle, K):
    m, bad = measure_visual(oracle, K, global_mode=True)
    print(_line("global K = %d" % K, m))
    assert not bad, bad
    w = L.global_map(K)
    _assert_common_points_couple_every_pair(w)
    assert m["F"] == 1 and 10 <= len(w["behind"]) <= 40 and not np.isin(w["behind"], w["common"]).any()
    seen = np.bincount(w["obs"]["mp_idx"], minlength=len(w["points"]))
    assert (seen[w["behind"]] > 0).sum() >= 10                               # (observed: the solver meets them and must leave them alone)
    o = L.oracle_global(oracle, K)
    assert np.array_equal(o["points"][w["behind"]], w["points"][w["behind"]])
    ob = w["obs"][np.isin(w["obs"]["mp_idx"], w["behind"])]                  # behind every camera that observes them, at the initial poses
    pose = np.where((ob["kf_idx"] >= 0)[:, None], w["poses_cw"][np.maximum(ob["kf_idx"], 0)], w["fixed_cw"][np.maximum(ob["fixed_idx"], 0)])
    depth = np.array([(L.synth._quat_rot(p[:4], x) + p[4:])[2] for p, x in zip(pose, w["points"][ob["mp_idx"]])])
    assert len(ob) >= 20 and np.all(depth < -1.0)


@pytest.mark.parametrize("K", list(L.INERTIAL))
def test_reference_determines_the_inertial_answer(oracle, K):
    m, bad = measure_inertial(oracle, K)
    print(_line("inertial K = %d" % K, m))
    assert not bad, bad
    assert m["unknowns"] <= 1300 and m["iterations"] >= 2


def test_cases_reach_every_path():
    """paths() over the cases covers every row of the table of large_ba_windows; the 87 / 88 and 35 / 36 pairs lie on opposite sides of
    the second-pass edge.  Whoever trims the case lists reads here which edge went with it."""
    vis = {K: L.paths(6 * K, True) for K in list(L.VISUAL) + list(L.GLOBAL)}
    ine = {K: L.paths(15 * K, False) for K in L.INERTIAL}
    missing = [r for r in L.VISUAL_ROWS if not any(r in p for p in vis.values())]
    assert not missing, "no visual case reaches %s" % missing
    missing = [r for r in L.INERTIAL_ROWS if not any(r in p for p in ine.values())]
    assert not missing, "no inertial case reaches %s" % missing
    second = {"rows_below_second_pass", "rhs_update_second_pass", "back_rows_q2"}
    assert not (vis[87] & second) and "rows_below_second_pass" in vis[88] and "rows_below_second_pass_is_rhs" in vis[88]
    assert not (vis[88] & {"rhs_update_second_pass", "back_rows_q2"}) and second <= vis[89]
    assert not (ine[35] & second) and second <= ine[36]
    # each threshold sits where its smallest case says: the size before it does not reach it
    first = {"gather_grid_capped": 61, "assemble_second_pass": 61, "schur_4_column_blocks": 65, "schur_5_column_blocks": 86, "schur_6_column_blocks": 107,
             "column_tile_slot_3": 67, "column_tile_slot_4": 89, "column_tile_slot_5": 110, "rows_below_second_pass": 88, "rhs_update_second_pass": 89,
             "back_rows_q2": 89, "full_768": 128}
    for row, K in first.items():
        assert row in L.paths(6 * K, True) and row not in L.paths(6 * (K - 1), True), row
    first = {"column_tile_slot_3": 27, "column_tile_slot_4": 36, "column_tile_slot_5": 44, "rows_below_second_pass": 36, "rhs_update_second_pass": 36,
             "back_rows_q2": 36, "odd_stride_765": 51}
    for row, K in first.items():
        assert row in L.paths(15 * K, False) and row not in L.paths(15 * (K - 1), False), row
    # the thresholds in unknowns, as derived from the constants
    for row, n in (("gather_grid_capped", 362), ("assemble_second_pass", 363), ("column_tile_slot_3", 401), ("column_tile_slot_4", 529),
                   ("column_tile_slot_5", 657), ("rows_below_second_pass", 528), ("rhs_update_second_pass", 529), ("back_rows_q2", 529)):
        assert row in L.paths(n, True) and row not in L.paths(n - 1, True), row
    assert all(p == set() for p in (L.paths(320, True), L.paths(315, False))) and L.paths(324, True) == {"per_panel"}
    # ... and the slot holds a whole keyframe's fifteen states at the size after each inertial edge (at 27 and 44: the last five and four)
    assert [L.slot_rows(15 * K, t) for K, t in ((27, 3), (28, 3), (44, 5), (45, 5), (36, 4))] == [5, 20, 4, 19, 12]
    assert all(15 * K > L.BF_MAX_N and 6 * K <= 306 for K in L.INERTIAL) and all(6 * K > L.BF_MAX_N for K in vis)
