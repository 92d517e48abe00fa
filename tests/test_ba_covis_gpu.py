"""GPU parity of local BA on the covisibility windows of tests/covis_windows.py: sparse covisibility, shuffled observation arrays, many
fixed observers interleaved with the optimised keyframes, the identity observer, empty and two-observation keyframes, 16-point tiles
without an optimised observer, duplicated (point, keyframe) pairs at random positions, tracks of exactly 32 / 33 / 64 / 65 / all cameras.
tests/test_ba_covis_cpu.py proves on the reference alone that every case pins its answer (50 x oracle spread <= 1e-6, LM margins >= 1e-9),
so the tolerances are test_ba_gpu.py's, unchanged: iterations equal, initial_error 1e-12, final_error 1e-8, poses and points 1e-6.

Measured on an MI355X (largest over the cases; the bound beside it):

- parity, ten cases: initial_error <= 3.3e-15 (1e-12), final_error <= 4.0e-10 (1e-8), poses <= 1.2e-9 and points <= 2.5e-10 (1e-6);
  iteration counts equal everywhere; second run the same bits.
- prefixes after 1 / 3 / 7 iterations (k12_f4, k26_f30, k49_f60): final_error <= 2.5e-9, poses <= 1.2e-8, points <= 1.6e-9.  First step
  against the oracle's, relative to the oracle's step norm: 1.2e-12, 5.3e-12, 1.2e-12; the oracle against itself on the reversed array
  1.2e-13, 3.9e-13, 3.6e-13, so the bound max(1e-9, 50 x that) is 1e-9 in all three.
- input orders (k12_f4, k20_f100, long_tracks, tiles_identity_dups): every order within 2.0e-10 of the oracle on that order; across
  orders <= 1.1e-10.  A stable regrouping by point (and by relabelled point) gives the SAME BITS as the shuffled array in all four cases:
  the comment above ba_prep_count_kernel holds as written.  kf_major and point_major are such regroupings of each other and agree
  bitwise; so do shuffled and reversed in the cases with tracks of at most 9 observations (the lanes' shuffle tree adds a short track
  in an order that its reversal does not change); long_tracks differs by 1.9e-16 and the duplicate chains by 2.4e-12.
- duplicates at shuffled positions against the dense oracle, four orders: poses <= 1.5e-13, points <= 5.3e-12.
- empty keyframe's pose against the oracle's: 0 (bitwise); tracks of exactly 32 / 33 / 64 / 65 / 120 observations: points <= 2.0e-16.
- thinned inertial window: poses 1.7e-11, velocities 1.1e-11, biases 3.6e-17, points 4.0e-11 (1e-6).
- global BA: 7.0e-13 and 4.7e-13 against a bound that stays at its 1e-6 floor (oracle spreads 1.1e-12, 5.9e-13).
No test of this file failed on the kernels as they were: no kernel or ABI change came out of it.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import covis_windows as W
from conftest import assert_ba_close
from orientation_cases import lm_margin

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6           # tests/test_ba_gpu.py
ORDER_CASES = ("k12_f4", "k20_f100", "long_tracks", "tiles_identity_dups")
PREFIX_CASES = W.PREFIX_CASES
WIRE_CASES = ("k20_f12", "long_tracks", "tiles_identity_dups")


def _gpu(gpu_handle, pkg, w, obs=None, **cfg):
    return gpu_handle.ba_solve_visual(pkg.CameraModel(**w["camera"]), pkg.LocalBAConfigLM(**cfg), w["poses_cw"], w["fixed_cw"], w["points"],
                                      w["obs"] if obs is None else obs)


def _oracle(oracle, w, dense=False, **kw):
    solve = oracle.ba_solve_dense if dense else oracle.ba_solve_schur
    return solve(oracle.Camera(**w["camera"]), oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], **kw)


def _assert_parity(g, o, tag):
    e0 = abs(g["initial_error"] - o["initial_error"]) / o["initial_error"]; e1 = abs(g["final_error"] - o["final_error"]) / o["final_error"]
    rp, rx = W.rel(g["poses_wc"], o["poses_wc"]), W.rel(g["points"], o["points"])
    print("%s: iterations %d / %d, initial_error %.2e, final_error %.2e, poses %.2e, points %.2e" % (tag, g["iterations"], o["iterations"], e0, e1, rp, rx))
    assert g["iterations"] == o["iterations"], tag
    assert e0 < 1e-12 and e1 < 1e-8, (tag, e0, e1)
    assert rp < POSE_TOL and rx < POSE_TOL, (tag, rp, rx)
    assert_ba_close(g, o, POSE_TOL)


def _same_bits(a, b):
    return a["iterations"] == b["iterations"] and a["initial_error"] == b["initial_error"] and a["final_error"] == b["final_error"] and \
        np.asarray(a["poses_wc"]).tobytes() == np.asarray(b["poses_wc"]).tobytes() and np.asarray(a["points"]).tobytes() == np.asarray(b["points"]).tobytes()


def _keep(r):
    """a result whose arrays may be views of a prepared batch: a copy that survives the next solve"""
    return None if r is None else dict(r, poses_wc=np.array(r["poses_wc"], copy=True), points=np.array(r["points"], copy=True))


# ---- a. parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(W.CASES))
def test_covis_parity(gpu_handle, oracle, pkg, name):
    w = W.case(name)
    g = _gpu(gpu_handle, pkg, w); o = _oracle(oracle, w)
    _assert_parity(g, o, name)
    assert _same_bits(_gpu(gpu_handle, pkg, w), g)                         # fixed-order reductions: run to run the same bits


# ---- b. prefixes -----------------------------------------------------------------------------------------------------------------------
def _align(q_like, ref):
    """poses [K,7] with every quaternion in the sign of `ref`'s (q and -q are one rotation; a difference of poses needs one sign)"""
    a = np.array(q_like, np.float64, copy=True)
    flip = (a[:, :4] * np.asarray(ref)[:, :4]).sum(1) < 0
    a[flip, :4] *= -1.0
    return a


def _step_error(got, want, start):
    """|step_got - step_want| / |step_want| over all poses, and over all points (2-norms; step = state after one iteration - input)"""
    gp, wp, sp = _align(got["poses_wc"], want["poses_wc"]), np.asarray(want["poses_wc"]), _align(start["poses_wc"], want["poses_wc"])
    return max(np.linalg.norm(gp - wp) / np.linalg.norm(wp - sp),
               np.linalg.norm(got["points"] - want["points"]) / np.linalg.norm(want["points"] - start["points"]))


@pytest.mark.parametrize("name", PREFIX_CASES)
def test_covis_prefixes_and_first_step(gpu_handle, oracle, pkg, name):
    w = W.case(name); r = W.case(name, "reversed")
    for it in (1, 3, 7):
        g = _gpu(gpu_handle, pkg, w, max_iterations=it); o = _oracle(oracle, w, stop_after=it)
        assert g["iterations"] == it
        _assert_parity(g, o, "%s after %d" % (name, it))
        if it == 1:
            ocfg = oracle.ba_config(); ocfg.max_iterations = 0
            start = oracle.ba_solve_schur(oracle.Camera(**w["camera"]), ocfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
            assert start["iterations"] == 0 and np.array_equal(start["points"], w["points"])
            assert np.linalg.norm(o["points"] - start["points"]) > 1e-3   # (the first step is accepted: there is a step to compare)
            own = _step_error(_oracle(oracle, r, stop_after=1), o, start)    # the reference against itself on the reversed array
            bound = max(1e-9, 50.0 * own)
            err = _step_error(g, o, start)
            print("%s first step: %.3e (oracle on the reversed array %.3e, bound %.3e)" % (name, err, own, bound))
            assert err <= bound, (err, bound)


# ---- c. input order --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORDER_CASES)
def test_covis_every_input_order(gpu_handle, oracle, pkg, name):
    res = {}
    for order in W.ORDERS:
        w = W.case(name, order)
        g = _gpu(gpu_handle, pkg, w)
        _assert_parity(g, _oracle(oracle, w), "%s %s" % (name, order))
        res[order] = g
    first = res[W.ORDERS[0]]
    for order, g in res.items():
        assert g["iterations"] == first["iterations"], order
        d = max(W.rel(g["poses_wc"], first["poses_wc"]), W.rel(g["points"], first["points"]))
        print("%s %s against %s: %.3e" % (name, order, W.ORDERS[0], d))
        assert d < POSE_TOL, (order, d)


@pytest.mark.parametrize("name", ORDER_CASES)
def test_covis_regrouping_that_keeps_each_points_order_keeps_the_bits(gpu_handle, pkg, name):
    """ba_kernels.hip above ba_prep_count_kernel: the observations of a point keep their INPUT order, "so every sum downstream keeps its
    order and its bits".  Then any permutation of the array that leaves each point's observations in their relative order — a stable sort
    by point index, a stable sort by a random relabelling of the points — must give the same bits as the shuffled array itself.  (The
    oracle sums in array order and does not have this property.)"""
    w = W.case(name); o = w["obs"]
    ref = _gpu(gpu_handle, pkg, w)
    by_point = o[np.argsort(o["mp_idx"], kind="stable")]
    label = np.random.default_rng(5).permutation(len(w["points"]))
    by_label = o[np.argsort(label[o["mp_idx"]], kind="stable")]
    assert not np.array_equal(by_point, o) and not np.array_equal(by_label, by_point)
    for tag, arr in (("stable sort by point", by_point), ("stable sort by relabelled point", by_label)):
        assert _same_bits(_gpu(gpu_handle, pkg, w, obs=arr), ref), (name, tag)
    # ... whereas an order that does change a point's own order changes rounding only
    g = _gpu(gpu_handle, pkg, W.case(name, "reversed"))
    assert g["iterations"] == ref["iterations"] and W.rel(g["points"], ref["points"]) < POSE_TOL


def test_covis_duplicates_at_shuffled_positions(gpu_handle, oracle, pkg):
    """second and third observations of a (point, keyframe) pair anywhere in the array: the chain of the tile slot follows the input order,
    W_jk is the sum of the pair's blocks — against the oracle's literal dense formulation, in every order"""
    for order in W.ORDERS:
        w = W.case("tiles_identity_dups", order)
        assert W.stats(w)["duplicate_pairs"] == 40
        _assert_parity(_gpu(gpu_handle, pkg, w), _oracle(oracle, w, dense=True), "duplicates %s (dense)" % order)


# ---- d. wire formats and upload paths -----------------------------------------------------------------------------------------------------
def test_covis_wire_formats_pinned_memory_and_compiled_caller(gpu_handle, pkg, tmp_path):
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    wins = [pkg.synth.keypoint_precision(W.case(n)) for n in WIRE_CASES]
    assert W.stats(wins[2])["identity_obs"] == 40
    want = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    for i, w in enumerate(wins):                                            # (and the batch is the single-window solve)
        assert _same_bits(_gpu(gpu_handle, pkg, w), want[i]), i
    # the 16-byte form == the 32-byte form; the identity observer travels as -1 - F
    c = pkg.ba_obs_to_obs32(wins[2]["obs"], len(wins[2]["fixed_cw"]))
    ident = (wins[2]["obs"]["kf_idx"] < 0) & (wins[2]["obs"]["fixed_idx"] < 0)
    assert ident.sum() == 40 and np.all(c["kf_idx"][ident] == -1 - len(wins[2]["fixed_cw"]))
    got32 = [_keep(r) for r in gpu_handle.prepare_ba_batch(wins, obs32=True).solve(cam, cfg)]
    prepared = [_keep(r) for r in gpu_handle.prepare_ba_batch(wins).solve(cam, cfg)]
    # observations in page-locked memory (read where they lie) == staged, batch and single, the single-window entry point in both forms
    packed = pkg.Handle.pack_ba_windows(wins); packed32 = pkg.Handle.pack_ba_windows(wins, obs32=True)
    assert packed32[0]["obs"].dtype == pkg.BA_OBS32
    pinned = gpu_handle.ba_solve_visual_batch(cam, cfg, packed)
    for i in range(len(wins)):
        for tag, got in (("obs32", got32), ("prepared", prepared), ("pinned", pinned)):
            assert _same_bits(got[i], want[i]), (tag, i)
        for tag, o in (("single pinned", packed[i]["obs"]), ("single pinned32", packed32[i]["obs"]),
                       ("single obs32", pkg.ba_obs_to_obs32(wins[i]["obs"], len(wins[i]["fixed_cw"])))):
            assert _same_bits(_gpu(gpu_handle, pkg, wins[i], obs=o), want[i]), (tag, i)
    # the compiled caller through the C ABI
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(root, "orb-slam3-rust_amd")
    exe = str(tmp_path / "ba_batch_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "ba_batch_driver.cpp"),
                    "-o", exe, "-L", libdir, "-lorbx_hip", "-Wl,-rpath," + libdir], check=True)
    pkg.synth.write_ba_batch_file(str(tmp_path / "batch.bin"), wins, pkg.BA_OBS)
    for mode in ("pinned", "pageable", "pinned32"):
        r = subprocess.run([exe, str(tmp_path / "batch.bin"), str(tmp_path / "out.bin"), "2", mode], check=True, capture_output=True, text=True, timeout=300)
        assert json.loads(r.stdout.strip().splitlines()[-1])["windows"] == len(wins)
        got = pkg.synth.read_ba_batch_results(str(tmp_path / "out.bin"), wins)
        for i, g in enumerate(got):
            assert g["status"] == 0 and _same_bits(g, want[i]), (mode, i)


# ---- e. batch --------------------------------------------------------------------------------------------------------------------------
def test_covis_batch_equals_single_in_either_window_order(gpu_handle, pkg):
    """13 windows (8 or more: 16 lanes per point in the per-observation kernels): every case, two dense windows, one the reference answers
    None for"""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    wins = [W.case(n) for n in W.CASES] + [pkg.synth.ba_window(3100, 20, 900, pkg.BA_OBS), pkg.synth.ba_window(3101, 7, 200, pkg.BA_OBS, n_fixed_extra=2)]
    empty = dict(wins[0]); empty["obs"] = wins[0]["obs"][:0]
    wins.insert(5, empty)
    assert len(wins) == 13
    single = [_gpu(gpu_handle, pkg, w) for w in wins]
    assert single[5] is None
    for tag, idx in (("as listed", list(range(13))), ("reversed", list(range(13))[::-1])):
        batch = gpu_handle.ba_solve_visual_batch(cam, cfg, [wins[i] for i in idx])
        for k, i in enumerate(idx):
            if single[i] is None:
                assert batch[k] is None
            else:
                assert _same_bits(batch[k], single[i]), (tag, i)


# ---- f. edges --------------------------------------------------------------------------------------------------------------------------
def test_covis_empty_and_two_observation_keyframe(gpu_handle, oracle, pkg):
    for name in ("empty_kf", "thin_kf"):
        w = W.case(name)
        assert W.stats(w)["kf_obs"][3] == (0 if name == "empty_kf" else 2)
        g = _gpu(gpu_handle, pkg, w); o = _oracle(oracle, w)
        _assert_parity(g, o, name)
        if name == "empty_kf":
            # no residual, no coupling: the pose comes back as the reference returns it (its input, through the scaled axis and back)
            d = W.rel(g["poses_wc"][3:4], o["poses_wc"][3:4])
            print("empty keyframe against the oracle's: %.3e" % d)
            assert d < 1e-12


def test_covis_identity_observer_in_both_wire_formats(gpu_handle, oracle, pkg):
    w = pkg.synth.keypoint_precision(W.case("tiles_identity_dups"))
    F = len(w["fixed_cw"])
    o = _oracle(oracle, w)
    g64 = _gpu(gpu_handle, pkg, w)
    g32 = _gpu(gpu_handle, pkg, w, obs=pkg.ba_obs_to_obs32(w["obs"], F))
    _assert_parity(g64, o, "identity observer, 32-byte form"); _assert_parity(g32, o, "identity observer, 16-byte form")
    assert _same_bits(g64, g32)
    # it is the identity pose that observes: the same observations through one more fixed keyframe that IS the identity
    w2 = dict(w); w2["fixed_cw"] = np.concatenate([w["fixed_cw"], [[1.0, 0, 0, 0, 0, 0, 0]]])
    o2 = w["obs"].copy(); ident = (o2["kf_idx"] < 0) & (o2["fixed_idx"] < 0); o2["fixed_idx"][ident] = F
    w2["obs"] = o2
    assert ident.sum() == 40 and _same_bits(_gpu(gpu_handle, pkg, w2), g64)
    # and they matter: without them the answer is another one
    w3 = dict(w); w3["obs"] = w["obs"][~ident]
    assert W.rel(_gpu(gpu_handle, pkg, w3)["points"], g64["points"]) > 1e-6


def test_covis_fixed_only_tiles_and_exact_track_lengths(gpu_handle, oracle, pkg):
    w = W.case("tiles_identity_dups"); j0, j1 = W.CASES["tiles_identity_dups"]["fixed_only_block"]
    g = _gpu(gpu_handle, pkg, w); o = _oracle(oracle, w)
    seen = np.bincount(w["obs"]["mp_idx"], minlength=len(w["points"]))[j0:j1] > 0
    assert seen.sum() >= 4 and W.rel(g["points"][j0:j1][seen], o["points"][j0:j1][seen]) < POSE_TOL
    assert np.array_equal(g["points"][j0:j1][~seen], w["points"][j0:j1][~seen])            # an unobserved point stays where it was
    assert np.abs(g["points"][j0:j1][seen] - w["points"][j0:j1][seen]).max() > 1e-4         # the points of the fixed-only tiles did move
    w = W.case("long_tracks")
    g = _gpu(gpu_handle, pkg, w); o = _oracle(oracle, w)
    tl = np.bincount(w["obs"]["mp_idx"], minlength=len(w["points"]))
    T = len(w["poses_cw"]) + len(w["fixed_cw"])
    for L in (32, 33, 64, 65, T):
        sel = tl == L
        d = W.rel(g["points"][sel], o["points"][sel])
        print("tracks of %d observations (%d points): %.3e" % (L, sel.sum(), d))
        assert sel.sum() >= 2 and d < POSE_TOL, L
        assert np.abs(g["points"][sel] - w["points"][sel]).max() > 1e-4


# ---- g. the same structure through the other two solvers ----------------------------------------------------------------------------------
def test_covis_thinned_shuffled_inertial_window(gpu_handle, oracle, pkg):
    """tests/test_inertial_ba.py's tolerances on synth.inertial_window(K = 10, M = 400) with 40 % of its observations, shuffled"""
    from test_inertial_ba import TOL, _gpu as inertial_gpu, _rel
    w, o, seed = W.inertial_scene(oracle)
    g = inertial_gpu(gpu_handle, w)
    assert g["iterations"] == o["iterations"]
    assert abs(g["initial_error"] - o["initial_error"]) < 1e-10 * o["initial_error"]
    assert abs(g["final_error"] - o["final_error"]) < 1e-7 * o["final_error"]
    for key in ("poses_wc", "velocities", "biases", "points"):
        print("inertial (seed %d) %s: %.3e" % (seed, key, _rel(g[key], o[key])))
        assert _rel(g[key], o[key]) < TOL, key
    g2 = inertial_gpu(gpu_handle, w)
    assert all(np.array_equal(g[k], g2[k]) for k in ("poses_wc", "velocities", "biases", "points"))


@pytest.mark.parametrize("name", list(W.GLOBAL_CASES))
def test_covis_global_ba(gpu_handle, oracle, pkg, name):
    """tests/test_global_ba.py's rule: one fixed keyframe leaves the monocular scale a free gauge, so the bound is max(1e-6, 50 x the spread
    of the reference's own runs) — its Schur form on the window and on the reversed array, and its dense form where that fits"""
    from test_global_ba import TOL, _gcfg, _rel
    w = W.covis_window(**W.GLOBAL_CASES[name]); r = W.covis_window(order="reversed", **W.GLOBAL_CASES[name])
    cam = oracle.Camera(**w["camera"])
    o = oracle.global_ba_solve_schur(cam, _gcfg(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    runs = [o, oracle.global_ba_solve_schur(cam, _gcfg(), r["poses_cw"], r["fixed_cw"], r["points"], r["obs"])]
    if W.dense_fits(w):
        runs.append(oracle.global_ba_solve_dense(cam, _gcfg(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"]))
    spread = max(max(_rel(a["poses_wc"], b["poses_wc"]), _rel(a["points"], b["points"])) for i, a in enumerate(runs) for b in runs[i + 1:])
    tol = max(TOL, 50.0 * spread)
    g = gpu_handle.ba_solve_global(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"])
    d = max(_rel(g["poses_wc"], o["poses_wc"]), _rel(g["points"], o["points"]))
    print("%s: %.3e (spread %.3e, bound %.3e), margin %.3e" % (name, d, spread, tol, lm_margin(o["trace"])))
    assert len(set(x["iterations"] for x in runs)) == 1 and g["iterations"] == o["iterations"]
    assert abs(g["initial_error"] - o["initial_error"]) < 1e-12 * o["initial_error"]
    assert abs(g["final_error"] - o["final_error"]) < 1e-8 * o["final_error"]
    assert d < tol
