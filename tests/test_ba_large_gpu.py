"""GPU parity of BA on windows of 57 to 128 optimised keyframes (visual, global) and 23 to 51 (inertial): reduced systems of 342 to 768
unknowns, where the per-panel solve (ba_big_step_kernel per 16-column panel, ba_big_back_kernel) and the kernels that feed it first take
their capped grids, their fourth to sixth column blocks and tile slots, their second passes and their full LDS arrays
(large_ba_windows.paths names what each size reaches; every parity test prints it; a dozen far points seen by every camera keep the
tiles far from the diagonal from being exact zeros: tests/test_ba_large_cpu.py says what was tried to see that this matters).  tests/test_ba_large_cpu.py proves on the reference
alone that every case pins its answer, so the tolerances are the project's own, unchanged: visual and global — iterations equal,
initial_error 1e-12, final_error 1e-8, poses and points 1e-6 (tests/test_ba_gpu.py, tests/test_global_ba.py); inertial — initial_error
1e-10, final_error 1e-7, states and points 1e-6 (tests/test_inertial_ba.py).

Measured on an MI355X (largest over the cases; the bound beside it):

- visual, ten sizes: initial_error <= 3.5e-14 (1e-12), final_error <= 5.5e-10 (1e-8), poses <= 1.5e-10 and points <= 1.9e-11 (1e-6);
  iteration counts equal everywhere; K = 128 a second time the same bits.
- global K = 88, 128: initial_error 2.1e-15, final_error 2.2e-14, poses 2.5e-15, points 2.1e-14; points behind the cameras untouched.
- inertial, eight sizes: initial_error <= 1.1e-15 (1e-10), final_error <= 5.1e-15 (1e-7), poses <= 8.8e-12, velocities <= 8.2e-12, biases
  <= 1.2e-16, points <= 8.5e-12 (1e-6).
- the 16-byte observation form from the host and from device memory, the batch of (57, 128, 88, 20, 110) keyframes, the small window
  after the largest on one handle: the bits of the single 32-byte-form solve.  A NaN pixel at n = 528 and 768: one iteration, the
  zero-iteration result.  129 optimised keyframes and 52 inertial ones: refused, output arrays as they were.
The slowest tests are the inertial parity cases, 0.9 to 1.3 s each (test_large_inertial_parity[36] 1.24 s), nearly all of it the dense
inertial oracle; the visual K = 128 parity takes 0.45 s.
No test of this file failed on the kernels as they were: no kernel change came out of it.
"""
import ctypes as C

import numpy as np
import pytest

import covis_windows as W
import large_ba_windows as L
from conftest import assert_ba_close

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-6           # tests/test_ba_gpu.py
BATCH = (57, 128, 88, "k20_f12", 110)
PATTERN = -7.25e11        # what the output arrays of a refused call are filled with beforehand


def _gpu(gpu_handle, pkg, w, obs=None, **cfg):
    return gpu_handle.ba_solve_visual(pkg.CameraModel(**w["camera"]), pkg.LocalBAConfigLM(**cfg), w["poses_cw"], w["fixed_cw"], w["points"],
                                      w["obs"] if obs is None else obs)


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


def _batch_window(name):
    return W.case(name) if isinstance(name, str) else L.visual_window(name)


# ---- 1. visual parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", list(L.VISUAL))
def test_large_visual_parity(gpu_handle, oracle, pkg, K):
    w = L.visual_window(K)
    assert len(w["poses_cw"]) == K and 6 * K > L.BF_MAX_N
    g = _gpu(gpu_handle, pkg, w)
    _assert_parity(g, L.oracle_visual(oracle, K), "visual K = %d (n = %d: %s)" % (K, 6 * K, ", ".join(sorted(L.paths(6 * K, True)))))
    if K == 128:
        assert _same_bits(_gpu(gpu_handle, pkg, w), g)                     # fixed-order reductions: run to run the same bits


# ---- 2. the 16-byte observation form, from the host and from device memory -------------------------------------------------------------------
@pytest.mark.parametrize("K", (89, 128))
def test_large_visual_obs32_and_device_observations(gpu_handle, pkg, K):
    import torch
    w = pkg.synth.keypoint_precision(L.visual_window(K))
    ref = _gpu(gpu_handle, pkg, w)
    assert ref["iterations"] == 10 and ref["final_error"] < ref["initial_error"]
    o32 = pkg.ba_obs_to_obs32(w["obs"], len(w["fixed_cw"]))
    assert o32 is not None and o32.dtype == pkg.BA_OBS32 and len(o32) == len(w["obs"])
    assert _same_bits(_gpu(gpu_handle, pkg, w, obs=o32), ref)
    dev = torch.from_numpy(np.ascontiguousarray(o32).view(np.uint8).copy()).cuda()
    g = gpu_handle.ba_solve_visual_obs32_device(pkg.CameraModel(**w["camera"]), pkg.LocalBAConfigLM(), w["poses_cw"], w["fixed_cw"], w["points"], dev, len(o32))
    assert _same_bits(g, ref)


# ---- 3. batch -----------------------------------------------------------------------------------------------------------------------------
def test_large_visual_batch_equals_single(gpu_handle, pkg):
    """n = 342, 768, 528, 120 and 660 in one call: the per-panel launches are sized by n = 768, and the small window (LDS solve) and the
    342-unknown one return early from most of them"""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA); cfg = pkg.LocalBAConfigLM()
    wins = [_batch_window(n) for n in BATCH]
    assert [len(w["poses_cw"]) for w in wins] == [57, 128, 88, 20, 110]
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    for name, w, b in zip(BATCH, wins, batch):
        assert _same_bits(b, _gpu(gpu_handle, pkg, w)), name


# ---- 4. failed factorisation ----------------------------------------------------------------------------------------------------------------
def test_large_visual_failed_factorisation_ends_the_solve(gpu_handle, pkg):
    """tests/test_ba_gpu.py's test_ba_failed_factorisation_ends_the_solve_on_every_reduced_system_path at n = 528 and 768: one NaN pixel
    fails every pivot; the solve ends after that iteration with exactly the zero-iteration result, alone and in a batch"""
    cam = pkg.CameraModel(**pkg.synth.EUROC_CAMERA)
    wins = []
    for K in (88, 128):
        w = dict(L.visual_window(K))
        w["obs"] = w["obs"].copy(); w["obs"]["u"][7] = np.nan
        wins.append(w)
    cfg, cfg0 = pkg.LocalBAConfigLM(), pkg.LocalBAConfigLM(max_iterations=0)
    batch = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    for w, b in zip(wins, batch):
        r = gpu_handle.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        z = gpu_handle.ba_solve_visual(cam, cfg0, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        assert z["iterations"] == 0 and np.array_equal(z["points"], w["points"])
        for got in (r, b):
            assert got["iterations"] == 1, len(w["poses_cw"])
            assert np.array_equal(np.asarray(got["poses_wc"]), np.asarray(z["poses_wc"])) and np.array_equal(got["points"], z["points"])


# ---- 5. global BA at the bound ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", list(L.GLOBAL))
def test_large_global_ba_matches_oracle(gpu_handle, oracle, pkg, K):
    from test_global_ba import TOL, _rel
    w = L.global_map(K)
    o = L.oracle_global(oracle, K)
    g = gpu_handle.ba_solve_global(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"])
    _assert_parity(g, o, "global K = %d" % K)
    assert _rel(g["poses_wc"], o["poses_wc"]) < TOL and _rel(g["points"], o["points"]) < TOL
    assert np.array_equal(g["points"][w["behind"]], w["points"][w["behind"]])
    moved = np.setdiff1d(np.unique(w["obs"]["mp_idx"]), w["behind"])
    assert np.abs(g["points"][moved] - w["points"][moved]).max() > 1e-4


def test_global_ba_of_130_keyframes_is_refused_and_writes_nothing(gpu_handle, pkg):
    from orb_slam3_rust_amd.api import SHOULD_STOP_FN, _vp
    w = L.global_map(128)
    poses = np.ascontiguousarray(np.concatenate([w["poses_cw"], w["poses_cw"][:1]]))   # 129 optimised keyframes + the fixed one
    fixed = np.ascontiguousarray(w["fixed_cw"][0]); pts = np.array(w["points"], copy=True); obs = np.ascontiguousarray(w["obs"], pkg.BA_OBS)
    out = np.full((len(poses), 7), PATTERN)
    it = C.c_int(-5); e0 = C.c_double(PATTERN); e1 = C.c_double(PATTERN)
    cam = pkg.CameraModel(**w["camera"])._c(); cfg = pkg.GlobalBAConfig()._c()
    rc = gpu_handle._L.orbx_ba_solve_global(gpu_handle._h, C.byref(cam), C.byref(cfg), C.c_int(len(poses)), _vp(poses), _vp(fixed), C.c_int(len(pts)), _vp(pts),
                                            C.c_int(len(obs)), _vp(obs), C.cast(None, SHOULD_STOP_FN), None, _vp(out), C.byref(it), C.byref(e0), C.byref(e1))
    assert rc == -1                                                         # ORBX_ERR_INVALID
    assert "at most 128 optimised keyframes per window" in gpu_handle._L.orbx_last_error(gpu_handle._h).decode()
    assert np.all(out == PATTERN) and np.array_equal(pts, w["points"]) and it.value == 0
    with pytest.raises(pkg.OrbxError) as e:
        gpu_handle.ba_solve_global(pkg.CameraModel(**w["camera"]), pkg.GlobalBAConfig(), poses, fixed, pts, obs)
    assert e.value.code == -1
    # ... and the handle solves the next map as if nothing had been asked
    small = W.covis_window(**W.GLOBAL_CASES["global_k20"])
    a = gpu_handle.ba_solve_global(pkg.CameraModel(**small["camera"]), pkg.GlobalBAConfig(), small["poses_cw"], small["fixed_cw"][0], small["points"], small["obs"])
    assert a["iterations"] > 0 and a["final_error"] < a["initial_error"]


# ---- 6. inertial parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", list(L.INERTIAL))
def test_large_inertial_parity(gpu_handle, oracle, K):
    from test_inertial_ba import TOL, _gpu as inertial_gpu, _rel
    w = L.inertial_window(K)
    assert len(w["poses_wc"]) == K and 15 * K > L.BF_MAX_N
    o = L.oracle_inertial(oracle, K)
    g = inertial_gpu(gpu_handle, w)
    e0 = abs(g["initial_error"] - o["initial_error"]) / o["initial_error"]; e1 = abs(g["final_error"] - o["final_error"]) / o["final_error"]
    print("inertial K = %d (n = %d: %s): iterations %d / %d, initial_error %.2e, final_error %.2e, %s" % (
        K, 15 * K, ", ".join(sorted(L.paths(15 * K, False))), g["iterations"], o["iterations"], e0, e1,
        ", ".join("%s %.2e" % (k, _rel(g[k], o[k])) for k in ("poses_wc", "velocities", "biases", "points"))))
    assert g["iterations"] == o["iterations"]
    assert e0 < 1e-10 and e1 < 1e-7, (e0, e1)
    for key in ("poses_wc", "velocities", "biases", "points"):
        assert _rel(g[key], o[key]) < TOL, key


def test_inertial_ba_of_52_keyframes_is_refused_and_writes_nothing(gpu_handle, pkg):
    from orb_slam3_rust_amd.api import SHOULD_STOP_FN, _vp
    K = 52
    w = pkg.synth.inertial_window(1, K, 60, pkg.BA_OBS, n_fixed=1, dt=0.08)
    poses = np.ascontiguousarray(w["poses_wc"]); vel = np.ascontiguousarray(w["velocities"]); bias = np.ascontiguousarray(w["biases"])
    fixed = np.ascontiguousarray(w["fixed_cw"]); pts = np.array(w["points"], copy=True); obs = np.ascontiguousarray(w["obs"], pkg.BA_OBS)
    ek = np.ascontiguousarray(w["edge_kf"], np.int32); pre = np.ascontiguousarray(w["preint"], np.float64)
    out_p = np.full((K, 7), PATTERN); out_v = np.full((K, 3), PATTERN); out_b = np.full((K, 6), PATTERN)
    it = C.c_int(-5); e0 = C.c_double(PATTERN); e1 = C.c_double(PATTERN)
    cam = pkg.CameraModel(**w["camera"])._c(); cfg = pkg.LocalInertialBAConfig()._c()
    rc = gpu_handle._L.orbx_ba_solve_inertial(gpu_handle._h, C.byref(cam), C.byref(cfg), C.c_int(K), _vp(poses), _vp(vel), _vp(bias), C.c_int(len(fixed)), _vp(fixed),
                                              C.c_int(len(pts)), _vp(pts), C.c_int(len(obs)), _vp(obs), C.c_int(len(ek)), _vp(ek), _vp(pre),
                                              C.cast(None, SHOULD_STOP_FN), None, _vp(out_p), _vp(out_v), _vp(out_b), C.byref(it), C.byref(e0), C.byref(e1))
    assert rc == -1
    assert "at most 51 keyframes per inertial window" in gpu_handle._L.orbx_last_error(gpu_handle._h).decode()
    assert np.all(out_p == PATTERN) and np.all(out_v == PATTERN) and np.all(out_b == PATTERN) and np.array_equal(pts, w["points"]) and it.value == 0
    with pytest.raises(pkg.OrbxError) as e:
        gpu_handle.ba_solve_inertial(pkg.CameraModel(**w["camera"]), pkg.LocalInertialBAConfig(), poses, vel, bias, fixed, pts, obs, ek, pre)
    assert e.value.code == -1 and "at most 51 keyframes per inertial window" in str(e.value)


# ---- 7. handle reuse --------------------------------------------------------------------------------------------------------------------------
def test_small_window_after_the_largest_on_one_handle(gpu_handle, pkg):
    """the arena of a K = 128 solve stays allocated when a five-keyframe window follows: nothing of the large solve's partial sums, factor
    or state may reach the small one — the same bits as on a handle that has solved nothing else"""
    big = L.visual_window(128)
    small = pkg.synth.ba_window(77, 6, 150, pkg.BA_OBS)
    assert len(small["poses_cw"]) == 5
    assert _gpu(gpu_handle, pkg, big)["iterations"] == 10
    after = _gpu(gpu_handle, pkg, small)
    fresh = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 600, device=0, max_w=752, max_h=480, max_batch=1)
    try:
        want = _gpu(fresh, pkg, small)
    finally:
        fresh.close()
    assert want["iterations"] > 0 and want["final_error"] < want["initial_error"]
    assert _same_bits(after, want)
