"""The covisibility windows of tests/covis_windows.py, on the CPU: the inputs have the structure claimed, and the REFERENCE determines the
answer tightly enough for the GPU comparison of tests/test_ba_covis_gpu.py.  Conditions on the inputs, checked without the code under test.

Per case: the oracle's Schur form on the window, on the window "reversed" (the shuffled array back to front) and, where 6 K + 3 M <= 2500,
its dense form.  spread = the largest difference (covis_windows.rel = test_ba_gpu.py's _rel: per keyframe rotation angle and relative
translation, per point relative position) between any two of them; required: the same iteration count in all, 50 x spread <= 1e-6 (the
max(1e-6, 50 x spread) rule of test_fuzz_gpu.py / test_global_ba.py lands on its floor), 50 x the spread of final_error <= 1e-8 and of initial_error <= 1e-12 (the bounds they are compared within on the
GPU) and lm_margin >= 1e-9 (no accept / reject decision on a rounding tie).

Measured (this table is what the tests assert on; fill = share of pairs of different optimised keyframes sharing a point):

case                 K   F    M     N     track        0 / 1 obs   fixed-only  obs per kf      fill   iterations   spread    final_error  margin   steps (Accepted / rejected)
                                           min/med/max  points      points      min/med/max                          spread
k12_f4               12  4    700   575   1 / 1 / 5    344 / 186   69          29 / 34 / 43    0.348  10 10 10     3.8e-10   4.4e-12      3.3e-07  AAAAAAAAAA
k20_f12              20  12   2000  2599  1 / 2 / 6    691 / 516   290         64 / 79 / 100   0.295  10 10        1.5e-09   9.5e-11      9.7e-03  AAAArrrrrr
k20_f100             20  100  3000  6435  1 / 3 / 9    635 / 547   1456        51 / 57 / 65    0.158  10 10        6.0e-13   1.7e-11      6.8e-02  AArrrAAAAA
k26_f30              26  30   2500  2344  1 / 2 / 4    1072 / 701  576         27 / 40 / 57    0.111  10 10        4.9e-13   7.9e-13      1.4e-03  ArArrrrArr
k49_f60              49  60   6000  7726  1 / 2 / 7    2114 / 1502 1381        46 / 71 / 90    0.114  10 10        1.1e-12   9.6e-12      5.1e-02  AArrrrArAA
k55_f20              55  20   3000  5312  1 / 2 / 7    884 / 526   182         54 / 70 / 94    0.197  10 10        8.7e-13   4.6e-11      2.9e-02  rrAAAArrAA
long_tracks          10  110  600   28972 1 / 50 / 120 7 / 3       103         231 / 247 / 262 1.0    10 10 10     5.9e-15   3.9e-15      8.2e-07  AAAArrrrrr
empty_kf             10  5    600   970   1 / 2 / 8    219 / 107   48          0 / 71 / 79     0.556  10 10 10     1.1e-11   4.7e-13      9.9e-07  AAAAAAAAAA
thin_kf              10  5    600   972   1 / 2 / 8    219 / 106   47          2 / 71 / 79     0.6    10 10 10     1.4e-11   6.9e-13      9.9e-07  AAAAAAAAAA
tiles_identity_dups  10  5    605   1124  1 / 3 / 9    224 / 88    71          58 / 73 / 84    0.8    10 10 10     1.3e-11   1.2e-14      2.4e-06  AAAAAArrrr

(three iteration counts: Schur, Schur on the reversed array, dense.)  long_tracks: 6 / 8 / 9 / 14 / 2 points with exactly 32 / 33 / 64 / 65 /
120 observations (two of each made by the option, the others the window's own).  tiles_identity_dups: points 32..71 without an optimised
observer (18 of them seen by fixed cameras), 40 identity observations, 35 pairs observed twice and 5 three times.
Thinned inertial scene: seed 31 (the first tried), 1534 observations, 10 iterations, margin 2.3e-05.
Global cases (one fixed keyframe): global_k20 spread 1.1e-12, final_error spread 1.8e-10, margin 8.5e-03; global_k40 5.9e-13, 2.9e-11, 1.9e-01.

How the seeds were chosen: counting up from the prototype's until every condition asserted below held — conditions on the reference
alone (for most rows an accepted first step was asked for as well, which only the prefix cases need; the K = 26 row keeps 45 % of the
visible points instead of 35 %: at 35 % most steps of the first seeds are rejected).  What the seeds passed over failed on: on sparse windows whose
ten steps are nearly all accepted the loop ends far from the minimum and still descending fast, and the reference's own final_error
then differs by 1e-7 .. 2e-5 between the array and the reversed array (38 seeds of the K = 55 row: 27 of them above 1e-8) while poses
and points agree to 1e-9 .. 4e-7.  Such a window cannot carry the 1e-8 final_error bound, whatever is compared with the reference.
"""
import numpy as np
import pytest

import covis_windows as W
from orientation_cases import lm_margin

SPREAD_FLOOR = 1e-6
INITIAL_ERROR_TOL, FINAL_ERROR_TOL = 1e-12, 1e-8       # tests/test_ba_gpu.py
MARGIN = 1e-9


def _oracle_runs(oracle, name):
    w = W.case(name); r = W.case(name, "reversed")
    assert np.array_equal(r["obs"], w["obs"][::-1]) and np.array_equal(r["points"], w["points"])
    cam = oracle.Camera(**w["camera"])
    runs = [oracle.ba_solve_schur(cam, oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"]),
            oracle.ba_solve_schur(cam, oracle.ba_config(), r["poses_cw"], r["fixed_cw"], r["points"], r["obs"])]
    if W.dense_fits(w):
        runs.append(oracle.ba_solve_dense(cam, oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"]))
    return w, runs


@pytest.mark.parametrize("name", W.SPARSE)
def test_sparse_cases_have_the_structure_of_a_map(name):
    w = W.case(name); st = W.stats(w)
    print(name, {k: v for k, v in st.items() if k not in ("kf_obs", "track_opt", "track_lengths")})
    assert len(w["fixed_cw"]) >= 2
    assert st["cov_fill"] < 0.5 and st["one_obs"] >= 100 and st["fixed_only"] >= 50
    assert st["track"][1] <= 8                                              # median track of a real window: 2-8 observations
    assert not np.array_equal(np.sort(w["obs"], order=["mp_idx"]), w["obs"])        # (shuffled: neither keyframe- nor point-major)
    assert (np.diff(w["obs"]["mp_idx"]) < 0).sum() > len(w["obs"]) // 4
    fx, op = w["fixed_path_idx"], w["opt_path_idx"]
    assert fx.min() < op.max() and op.min() < fx.max()                      # fixed and optimised cameras interleave along the path


def test_long_track_case_has_the_exact_lengths():
    w = W.case("long_tracks"); st = W.stats(w)
    T = len(w["poses_cw"]) + len(w["fixed_cw"])
    tl = np.bincount(w["obs"]["mp_idx"], minlength=len(w["points"]))
    for L in (32, 33, 64, 65, T):
        assert (tl == L).sum() >= 2, L
    assert T > 96 and len(w["poses_cw"]) == 10
    # the 32-lane rounds see the lengths on both sides of their boundaries among the points that have an optimised observer
    assert all(((tl == L) & (st["track_opt"] > 0)).any() for L in (32, 33, 64, 65, T))


def test_empty_and_thin_keyframe_cases():
    e = W.stats(W.case("empty_kf")); t = W.stats(W.case("thin_kf"))
    assert e["kf_obs"][3] == 0 and np.all(np.delete(e["kf_obs"], 3) > 20)
    assert t["kf_obs"][3] == 2 and np.all(np.delete(t["kf_obs"], 3) > 20)
    assert np.array_equal(np.delete(e["kf_obs"], 3), np.delete(t["kf_obs"], 3))


def test_tiles_identity_duplicates_case():
    w = W.case("tiles_identity_dups"); st = W.stats(w); o = w["obs"]
    assert len(w["points"]) % 16 != 0
    j0, j1 = W.CASES["tiles_identity_dups"]["fixed_only_block"]
    assert j0 % 16 == 0 and (j1 - j0) == 2 * 16 + 8
    assert st["track_opt"][j0:j1].sum() == 0 and (st["track_opt"][j0 - 16:j0] > 0).any() and (st["track_opt"][j1:j1 + 8] > 0).any()
    blk = (o["mp_idx"] >= j0) & (o["mp_idx"] < j1)
    assert (blk & (o["fixed_idx"] >= 0)).sum() >= 8                         # (the tiles are not simply unobserved)
    assert st["identity_obs"] == 40 and st["duplicate_pairs"] == 40
    pair = o["mp_idx"][o["kf_idx"] >= 0].astype(np.int64) * 64 + o["kf_idx"][o["kf_idx"] >= 0]
    cnt = np.unique(pair, return_counts=True)[1]
    assert (cnt == 2).sum() == 35 and (cnt == 3).sum() == 5
    # the duplicates are not adjacent in the shuffled array
    pos = {}
    for i, (m, k) in enumerate(zip(o["mp_idx"], o["kf_idx"])):
        if k >= 0:
            pos.setdefault((m, k), []).append(i)
    gaps = [max(v) - min(v) for v in pos.values() if len(v) > 1]
    assert len(gaps) == 40 and min(gaps) > 1


@pytest.mark.parametrize("name", list(W.CASES))
def test_reference_determines_the_answer(oracle, name):
    w, runs = _oracle_runs(oracle, name)
    assert all(r is not None for r in runs)
    its = [r["iterations"] for r in runs]
    spread = max(max(W.rel(a["poses_wc"], b["poses_wc"]), W.rel(a["points"], b["points"])) for i, a in enumerate(runs) for b in runs[i + 1:])
    margin = min(lm_margin(r["trace"]) for r in runs)
    fe = [r["final_error"] for r in runs]; e0 = [r["initial_error"] for r in runs]
    fe_spread = (max(fe) - min(fe)) / min(fe); e0_spread = (max(e0) - min(e0)) / min(e0)
    print("%s: iterations %s spread %.3e final_error spread %.3e initial_error spread %.3e margin %.3e errors %.6f -> %.6f, steps %s" %
          (name, its, spread, fe_spread, e0_spread, margin, runs[0]["initial_error"], fe[0], "".join("A" if t[3] < t[0] else "r" for t in runs[0]["trace"])))
    assert len(set(its)) == 1, its
    assert 50.0 * spread <= SPREAD_FLOOR, spread
    # the errors are compared within 1e-12 (initial) and 1e-8 (final) relative: the reference's own runs must leave the same factor of 50
    # below them.  (A sparse window whose ten steps are nearly all accepted ends far from the minimum, descending fast: there the reference's
    # final_error differs by 1e-7 .. 2e-5 between the array and the reversed array while poses and points agree to 1e-9 .. 4e-7 — measured on 38 seeds
    # of the K = 55 row.  Such a seed cannot carry the 1e-8 bound, so the table holds the first seed of each row that meets every condition.)
    assert 50.0 * fe_spread <= FINAL_ERROR_TOL and 50.0 * e0_spread <= INITIAL_ERROR_TOL, (fe_spread, e0_spread)
    assert margin >= MARGIN, margin
    assert runs[0]["final_error"] < runs[0]["initial_error"]
    if name in W.PREFIX_CASES:                                              # the first step is accepted: there is a step to compare after one iteration
        assert all(r["trace"][0, 3] < r["trace"][0, 0] for r in runs)


def test_empty_keyframe_does_not_move_in_the_reference(oracle):
    """no residual and no coupling: the reference hands the pose back (through the scaled axis and back: rounding only)"""
    w = W.case("empty_kf")
    o = oracle.ba_solve_schur(oracle.Camera(**w["camera"]), oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert W.rel(o["poses_wc"][3:4], np.asarray(oracle.se3_inverse(w["poses_cw"][3])).reshape(1, 7)) < 1e-12


def test_orders_are_permutations_of_one_observation_set():
    for name in ("k12_f4", "tiles_identity_dups"):
        ref = np.sort(W.case(name, "kf_major")["obs"], order=["mp_idx", "kf_idx", "fixed_idx", "u", "v"])
        for order in W.ORDERS:
            w = W.case(name, order)
            assert np.array_equal(np.sort(w["obs"], order=["mp_idx", "kf_idx", "fixed_idx", "u", "v"]), ref), (name, order)
        assert np.all(np.diff(W.case(name, "point_major")["obs"]["mp_idx"]) >= 0)


def test_thinned_inertial_scene_is_found(oracle):
    w, o, seed = W.inertial_scene(oracle)
    print("inertial scene: seed %d, N %d, iterations %d, margin %.3e" % (seed, len(w["obs"]), o["iterations"], lm_margin(o["trace"])))
    assert lm_margin(o["trace"]) >= W.INERTIAL_MARGIN and o["iterations"] >= 2
    assert (np.diff(w["obs"]["mp_idx"]) < 0).sum() > len(w["obs"]) // 4


@pytest.mark.parametrize("name", list(W.GLOBAL_CASES))
def test_global_cases_are_solvable(oracle, name):
    """one fixed keyframe (the global solver's form): the monocular scale is a free gauge, so the bound of the GPU comparison is
    max(1e-6, 50 x spread) and the spread is only recorded here"""
    from test_global_ba import _gcfg, _rel
    w = W.covis_window(**W.GLOBAL_CASES[name]); r = W.covis_window(order="reversed", **W.GLOBAL_CASES[name])
    cam = oracle.Camera(**w["camera"])
    a = oracle.global_ba_solve_schur(cam, _gcfg(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    b = oracle.global_ba_solve_schur(cam, _gcfg(), r["poses_cw"], r["fixed_cw"], r["points"], r["obs"])
    spread = max(_rel(a["poses_wc"], b["poses_wc"]), _rel(a["points"], b["points"]))
    fe_spread = abs(a["final_error"] - b["final_error"]) / a["final_error"]
    print("%s: iterations %d / %d spread %.3e final_error spread %.3e margin %.3e" % (name, a["iterations"], b["iterations"], spread, fe_spread, lm_margin(a["trace"])))
    assert a["iterations"] == b["iterations"] and a["final_error"] < a["initial_error"]
    assert 50.0 * fe_spread <= FINAL_ERROR_TOL                             # (as in test_reference_determines_the_answer)
    assert lm_margin(a["trace"]) >= MARGIN and W.stats(w)["cov_fill"] < 0.5
