"""GPU tests of the whole-map global BA (orbx_ba_solve_global_map[_obs32[_device]], csrc/global_ba_kernels.hip): maps of 129 to 257
optimised keyframes against the CPU oracle's global_ba_solve_schur, small maps on the same path, the three observation forms, failure
handling, and a map of 1025 optimised keyframes (a reduced system of 6150 unknowns) without an oracle.
tests/test_global_map_cpu.py proves on the reference alone that every case pins its answer, so the tolerances are the project's own,
unchanged (tests/test_global_ba.py, tests/test_ba_large_gpu.py): iterations equal, initial_error 1e-12, final_error 1e-8, poses and points
1e-6, the points behind the cameras bit-identical to the input.

Measured on an MI355X (largest over the cases; the bound beside it):

- the five maps past 128 keyframes (n = 774, 960, 1026, 1542, 1200 banded): iteration counts equal everywhere (10 / 10); initial_error
  <= 3.4e-15 (1e-12), final_error <= 1.8e-13 (1e-8), poses <= 2.7e-14 and points <= 9.1e-15 (1e-6); the points behind the cameras
  untouched, others moved.
- the small maps on the same path: global_k20 initial_error 3.8e-16, final_error 5.7e-11, poses 3.0e-11, points 6.3e-12; global_map(128)
  initial_error 1.1e-15, final_error 2.2e-14, poses 2.4e-15, points 2.0e-14; iteration counts equal to ba_solve_global's.
- the 16-byte form from the host and from device memory, a second run, the 20-keyframe map after the 257-keyframe one on one handle:
  the same bits.  A NaN pixel at K = 160: one iteration, the zero-iteration result.  An index out of range, 2049 optimised keyframes, an
  all-reduce hook: refused, output arrays as they were; ba_solve_global still refuses 129 keyframes with its own message.
- K = 1025 (n = 6150, M = 20 000, N = 39 116): 10 iterations, error 24.449 -> 24.028 px, twice the same bits, 1.2 s.
The slowest test is the K = 257 parity case, 2.9 s, of which the oracle's solve is 2.7 s.
"""
import ctypes as C

import numpy as np
import pytest

import covis_windows as W
import global_map_cases as G
import large_ba_windows as L
from conftest import assert_ba_close

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6           # tests/test_ba_gpu.py
PATTERN = -7.25e11        # what the output arrays of a refused call are filled with beforehand
OLD_REFUSAL = "at most 128 optimised keyframes per window"


def _gpu(h, pkg, w, obs=None, **cfg):
    return h.ba_solve_global_map(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(**cfg), w["poses_cw"], w["fixed_cw"][0], w["points"],
                                 w["obs"] if obs is None else obs)


def _assert_parity(g, o, tag):
    from test_global_ba import TOL, _rel
    e0 = abs(g["initial_error"] - o["initial_error"]) / o["initial_error"]; e1 = abs(g["final_error"] - o["final_error"]) / o["final_error"]
    rp, rx = W.rel(g["poses_wc"], o["poses_wc"]), W.rel(g["points"], o["points"])
    print("%s: iterations %d / %d, initial_error %.2e, final_error %.2e, poses %.2e, points %.2e" % (tag, g["iterations"], o["iterations"], e0, e1, rp, rx))
    assert g["iterations"] == o["iterations"], tag
    assert e0 < 1e-12 and e1 < 1e-8, (tag, e0, e1)
    assert rp < POSE_TOL and rx < POSE_TOL, (tag, rp, rx)
    assert _rel(g["poses_wc"], o["poses_wc"]) < TOL and _rel(g["points"], o["points"]) < TOL
    assert_ba_close(g, o, POSE_TOL)


def _assert_behind_untouched_and_others_moved(g, w):
    assert np.array_equal(g["points"][w["behind"]], w["points"][w["behind"]])
    moved = np.setdiff1d(np.unique(w["obs"]["mp_idx"]), w["behind"])
    assert np.abs(g["points"][moved] - w["points"][moved]).max() > 1e-4


def _same_bits(a, b):
    return a["iterations"] == b["iterations"] and a["initial_error"] == b["initial_error"] and a["final_error"] == b["final_error"] and \
        np.asarray(a["poses_wc"]).tobytes() == np.asarray(b["poses_wc"]).tobytes() and np.asarray(a["points"]).tobytes() == np.asarray(b["points"]).tobytes()


def _raw(h, pkg, fn_name, w, poses, pts, obs, n_obs=None):
    """the C entry point itself on caller-owned output arrays filled with PATTERN -> (rc, message, poses_wc_out, points, iterations, e0, e1)"""
    from orb_slam3_rust_amd.api import SHOULD_STOP_FN, _vp
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7); fixed = np.ascontiguousarray(w["fixed_cw"][0])
    pts = np.array(pts, np.float64, copy=True).reshape(-1, 3)
    out = np.full((max(len(poses), 1), 7), PATTERN)
    it = C.c_int(-5); e0 = C.c_double(PATTERN); e1 = C.c_double(PATTERN)
    cam = pkg.CameraModel(**w["camera"])._c(); cfg = pkg.GlobalBAConfig()._c()
    rc = getattr(h._L, fn_name)(h._h, C.byref(cam), C.byref(cfg), C.c_int(len(poses)), _vp(poses), _vp(fixed), C.c_int(len(pts)), _vp(pts),
                                C.c_int(len(obs) if n_obs is None else n_obs), _vp(obs), C.cast(None, SHOULD_STOP_FN), None, _vp(out), C.byref(it), C.byref(e0), C.byref(e1))
    return rc, h._L.orbx_last_error(h._h).decode(), out, pts, it.value, e0.value, e1.value


def _old_path_still_refuses_and_small_solve_succeeds(h, pkg):
    w = L.global_map(128)
    poses = np.ascontiguousarray(np.concatenate([w["poses_cw"], w["poses_cw"][:1]]))      # 129 optimised keyframes
    with pytest.raises(pkg.OrbxError) as e:
        h.ba_solve_global(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), poses, w["fixed_cw"][0], w["points"], w["obs"])
    assert e.value.code == -1 and OLD_REFUSAL in str(e.value)
    small = W.covis_window(**W.GLOBAL_CASES["global_k20"])
    a = _gpu(h, pkg, small)
    assert a["iterations"] > 0 and a["final_error"] < a["initial_error"]


# ---- 1. parity with the oracle past 128 keyframes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
def test_global_map_parity(gpu_handle, oracle, pkg, name):
    w = G.case(name)
    assert len(w["poses_cw"]) > 128
    g = _gpu(gpu_handle, pkg, w)
    _assert_parity(g, G.oracle_answer(oracle, name), "global map %s (n = %d)" % (name, 6 * len(w["poses_cw"])))
    _assert_behind_untouched_and_others_moved(g, w)


# ---- 2. small shapes on the new path -------------------------------------------------------------------------------------------------------
def test_small_maps_take_the_new_path_and_match(gpu_handle, oracle, pkg):
    small = W.covis_window(**W.GLOBAL_CASES["global_k20"])
    for tag, w, o in (("global_k20", small, oracle.global_ba_solve_schur(oracle.Camera(**small["camera"]), L._gcfg(oracle), small["poses_cw"], small["fixed_cw"],
                                                                           small["points"], small["obs"])),
                      ("global_map(128)", L.global_map(128), L.oracle_global(oracle, 128))):
        g = _gpu(gpu_handle, pkg, w)
        _assert_parity(g, o, tag)
        old = gpu_handle.ba_solve_global(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"])
        assert g["iterations"] == old["iterations"]
        if "behind" in w:
            _assert_behind_untouched_and_others_moved(g, w)


def test_two_keyframes_solve_and_empty_problems_are_empty(gpu_handle, oracle, pkg):
    w = pkg.synth.ba_window(6, 2, 80, pkg.BA_OBS, n_fixed_extra=0)             # the fixed keyframe and K = 1 optimised one
    assert len(w["poses_cw"]) == 1 and len(w["fixed_cw"]) == 1
    g = _gpu(gpu_handle, pkg, w)
    o = oracle.global_ba_solve_schur(oracle.Camera(**w["camera"]), L._gcfg(oracle), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    assert g["iterations"] == o["iterations"] > 0 and g["final_error"] < g["initial_error"]
    assert abs(g["final_error"] - o["final_error"]) < 1e-8 * o["final_error"]
    obs = np.ascontiguousarray(w["obs"], pkg.BA_OBS)
    for poses, pts, ob in ((np.zeros((0, 7)), w["points"], obs[:0]), (w["poses_cw"], np.zeros((0, 3)), obs[:0]), (w["poses_cw"], w["points"], obs[:0])):
        rc, msg, out, p, it, e0, e1 = _raw(gpu_handle, pkg, "orbx_ba_solve_global_map", w, poses, pts, ob if len(ob) else np.zeros(1, pkg.BA_OBS), n_obs=0)
        assert rc == -6 and (it, e0, e1) == (0, 0.0, 0.0) and np.all(out == PATTERN)       # ORBX_ERR_EMPTY
    assert gpu_handle.ba_solve_global_map(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), np.zeros((0, 7)), w["fixed_cw"][0], w["points"], obs[:0]) is None


# ---- 3. the observation forms, run to run, workspace reuse -----------------------------------------------------------------------------------
def test_obs32_forms_and_second_run_give_the_same_bits(gpu_handle, pkg):
    import torch
    w = pkg.synth.keypoint_precision(G.case("k171"))
    ref = _gpu(gpu_handle, pkg, w)
    assert ref["iterations"] == 10 and ref["final_error"] < ref["initial_error"]
    assert _same_bits(_gpu(gpu_handle, pkg, w), ref)                           # fixed-order sums: run to run the same bits
    o32 = pkg.ba_obs_to_obs32(w["obs"], 1)
    assert o32 is not None and o32.dtype == pkg.BA_OBS32 and len(o32) == len(w["obs"])
    cam, cfg = pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig()
    assert _same_bits(gpu_handle.ba_solve_global_map_obs32(cam, cfg, w["poses_cw"], w["fixed_cw"][0], w["points"], o32), ref)
    assert _same_bits(_gpu(gpu_handle, pkg, w, obs=o32), ref)
    dev = torch.from_numpy(np.ascontiguousarray(o32).view(np.uint8).copy()).cuda()
    assert _same_bits(gpu_handle.ba_solve_global_map_obs32_device(cam, cfg, w["poses_cw"], w["fixed_cw"][0], w["points"], dev, len(o32)), ref)


def test_small_map_after_the_largest_on_one_handle(gpu_handle, pkg):
    """the workspaces of a K = 257 solve stay allocated when a 20-keyframe map follows: the same bits as on a handle that has solved
    nothing else"""
    small = W.covis_window(**W.GLOBAL_CASES["global_k20"])
    assert _gpu(gpu_handle, pkg, G.case("k257"))["iterations"] == 10
    after = _gpu(gpu_handle, pkg, small)
    fresh = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 600, device=0, max_w=752, max_h=480, max_batch=1)
    try:
        want = _gpu(fresh, pkg, small)
    finally:
        fresh.close()
    assert want["iterations"] > 0 and want["final_error"] < want["initial_error"]
    assert _same_bits(after, want)


# ---- 4. failure handling ---------------------------------------------------------------------------------------------------------------------
def test_failed_factorisation_ends_the_solve(gpu_handle, pkg):
    """one NaN pixel fails the first pivot it reaches: the solve ends after that iteration with exactly the zero-iteration result"""
    w = dict(G.case("k160"))
    w["obs"] = w["obs"].copy(); w["obs"]["u"][7] = np.nan
    r = _gpu(gpu_handle, pkg, w)
    z = _gpu(gpu_handle, pkg, w, max_iterations=0)
    assert z["iterations"] == 0 and np.array_equal(z["points"], w["points"])
    assert r["iterations"] == 1
    assert np.array_equal(np.asarray(r["poses_wc"]), np.asarray(z["poses_wc"])) and np.array_equal(r["points"], z["points"])


def test_refusals_write_nothing_and_leave_the_handle_usable(gpu_handle, pkg):
    w = G.case("k129")
    obs = np.ascontiguousarray(w["obs"], pkg.BA_OBS)
    # an observation index out of range
    for field, value in (("mp_idx", len(w["points"])), ("kf_idx", len(w["poses_cw"])), ("mp_idx", -1)):
        bad = obs.copy(); bad[field][1234] = value
        rc, msg, out, pts, it, e0, e1 = _raw(gpu_handle, pkg, "orbx_ba_solve_global_map", w, w["poses_cw"], w["points"], bad)
        assert rc == -1 and "observation 1234" in msg and "out of range" in msg, msg
        assert np.all(out == PATTERN) and np.array_equal(pts, w["points"]) and it == 0
        _old_path_still_refuses_and_small_solve_succeeds(gpu_handle, pkg)
    # one keyframe more than the cap
    cap = gpu_handle.ba_global_map_max_keyframes()
    assert cap >= 1024
    poses = np.ascontiguousarray(np.tile(w["poses_cw"][:1], (cap + 1, 1)))
    rc, msg, out, pts, it, e0, e1 = _raw(gpu_handle, pkg, "orbx_ba_solve_global_map", w, poses, w["points"], obs)
    assert rc == -1 and "at most %d optimised keyframes" % cap in msg, msg
    assert np.all(out == PATTERN) and np.array_equal(pts, w["points"]) and it == 0
    _old_path_still_refuses_and_small_solve_succeeds(gpu_handle, pkg)
    # an all-reduce hook installed
    gpu_handle.set_allreduce(lambda ptr, n, stream: None)
    try:
        o32 = pkg.ba_obs_to_obs32(pkg.synth.keypoint_precision(w)["obs"], 1)
        for fn, ob in (("orbx_ba_solve_global_map", obs), ("orbx_ba_solve_global_map_obs32", o32)):
            rc, msg, out, pts, it, e0, e1 = _raw(gpu_handle, pkg, fn, w, w["poses_cw"], w["points"], ob)
            assert rc == -1 and "all-reduce" in msg, msg
            assert np.all(out == PATTERN) and np.array_equal(pts, w["points"])
    finally:
        gpu_handle.set_allreduce(None)
    _old_path_still_refuses_and_small_solve_succeeds(gpu_handle, pkg)


def test_should_stop_is_polled_once_per_iteration(gpu_handle, oracle, pkg):
    from test_global_ba import TOL, _rel
    w = G.case("k129")
    calls = []
    r = gpu_handle.ba_solve_global_map(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"],
                                       should_stop=lambda: (calls.append(1) or len(calls) > 3))
    assert r["iterations"] == 3
    o = oracle.global_ba_solve_schur(oracle.Camera(**w["camera"]), L._gcfg(oracle), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"], stop_after=3)
    assert _rel(r["poses_wc"], o["poses_wc"]) < TOL and _rel(r["points"], o["points"]) < TOL


# ---- 5. map size, no oracle ------------------------------------------------------------------------------------------------------------------
def test_map_of_1025_keyframes(gpu_handle, pkg):
    w = G.case("big")
    assert 6 * len(w["poses_cw"]) == 6150
    g = _gpu(gpu_handle, pkg, w)
    print("K = 1025 (n = 6150, M = %d, N = %d): %d iterations, error %.3f -> %.3f px" % (len(w["points"]), len(w["obs"]), g["iterations"], g["initial_error"], g["final_error"]))
    assert g["iterations"] > 0 and g["final_error"] < g["initial_error"]
    assert np.array_equal(g["points"][w["behind"]], w["points"][w["behind"]])
    assert _same_bits(_gpu(gpu_handle, pkg, w), g)
