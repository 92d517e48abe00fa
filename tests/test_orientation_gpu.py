"""The pose solvers at real-world orientations and at the quaternion edges (tests/orientation_cases.py): visual local BA (single, batch,
obs32), global BA, local inertial BA, PnP-RANSAC and pose-inertial optimization against their CPU oracle / numpy restatement with the
tolerances of their own test files; the double cover q / -q on the GPU; world-rotation invariance of the visual cost without the
oracle; the IMU residual's device function near a zero and near a half turn of its error rotation.

Tolerances (each comparison names its own):
- poses: every quaternion COMPONENT within 1e-6 of the oracle's — the same sign, not only the same rotation — and translations /
  points within 1e-6 relative: the solvers' parity tolerance (BASELINE north star).
- initial_error: 1e-12 relative for the visual solvers (as tests/test_ba_gpu.py, tests/test_global_ba.py), 1e-10 for the inertial
  one (as tests/test_inertial_ba.py: its IMU rows are forward differences).  At the 1e-10 cut of se3_from_params a rotation of 1e-9
  rad moves the pose by less than the 1e-6 pose tolerance but the cost by ~1e-8 relative: the 1e-12 comparison is what sees the cut.
- final_error: 1e-8 relative (visual), 1e-7 (inertial), as their own files.
- invariance: the visual initial_error at G equals the one at the identity within 1e-10 relative: turning the world leaves every
  camera-frame point the same up to the rounding of one more rotation of ~10 m coordinates (~1e-15 m, ~1e-13 of the cost).
"""
import numpy as np
import pytest

import orb_slam3_rust_amd as P
from oracle import oracle as O
from conftest import pose_errors, point_errors
import orientation_cases as C
import pnp_spec as NS
import pose_inertial_spec as PS
from test_pnp_gpu import assert_matches_spec as pnp_matches_spec
from test_pose_inertial_gpu import assert_matches_spec as pi_matches_spec

pytestmark = pytest.mark.gpu
synth = P.synth
TOL = 1e-6
MARGIN = 1e-7          # LM accept / reject decisions of a selected inertial scene: |trial - current| / current of the oracle's >= this


def assert_poses(got, want, tol=TOL, where=""):
    """component by component on the quaternion (the sign included), per keyframe rotation angle and relative translation"""
    got = np.asarray(got, np.float64).reshape(-1, 7); want = np.asarray(want, np.float64).reshape(-1, 7)
    dq = np.abs(got[:, :4] - want[:, :4]).max()
    ang, dt = pose_errors(got, want)
    assert dq < tol and ang < tol and dt < tol, (where, dq, ang, dt)


def _rel_err(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module")
def cam():
    return P.CameraModel(**synth.EUROC_CAMERA)


# ---- visual local BA -----------------------------------------------------------------------------------------------------------------
def _visual(case):
    # two fixed observers besides the anchor: with one, the monocular scale is a free gauge and the oracle's own dense and Schur forms
    # differ by up to 2e-4 at these orientations (tests/test_global_ba.py takes that spread as its tolerance; here the gauge is fixed)
    return C.scene("ba_window", case, 2, 6, 200, P.BA_OBS, n_fixed_extra=2)


def _vis_gpu(h, w):
    return h.ba_solve_visual(P.CameraModel(**w["camera"]), P.LocalBAConfigLM(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])


def _vis_oracle(w):
    return O.ba_solve_dense(O.Camera(**w["camera"]), O.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])


@pytest.fixture(scope="module")
def visual_identity(gpu_handle):
    return _vis_gpu(gpu_handle, _visual("identity"))


@pytest.mark.parametrize("case", C.IDS)
def test_visual_ba_parity_and_invariance(gpu_handle, visual_identity, case):
    w = _visual(case)
    o, g = _vis_oracle(w), _vis_gpu(gpu_handle, w)
    assert g["iterations"] == o["iterations"]
    assert _rel_err(g["initial_error"], o["initial_error"]) < 1e-12
    assert _rel_err(g["final_error"], o["final_error"]) < 1e-8
    assert_poses(g["poses_wc"], o["poses_wc"])
    assert point_errors(g["points"], o["points"]) < TOL
    assert _rel_err(g["initial_error"], visual_identity["initial_error"]) < 1e-10          # (c): no oracle involved
    n = C.negate(C.negate(w, ["poses_cw"], alternate=True), ["fixed_cw"])
    gn = _vis_gpu(gpu_handle, n)                                                           # (b): scaled axis / rotation matrix of q == of -q
    assert gn["iterations"] == g["iterations"] and gn["initial_error"] == g["initial_error"] and gn["final_error"] == g["final_error"]
    assert gn["poses_wc"].tobytes() == g["poses_wc"].tobytes() and gn["points"].tobytes() == g["points"].tobytes()


def test_visual_ba_batch_and_obs32_at_every_orientation(gpu_handle, cam):
    """one batch holding a window at every case (each window's result must not depend on its neighbours' orientations), against the
    oracle; the 16-byte observation form of the f32-rounded windows equals the 32-byte form bit for bit and the oracle within TOL; a batch
    of the same windows with every quaternion negated gives the same bits"""
    cfg = P.LocalBAConfigLM()
    wins = [synth.keypoint_precision(C.scene("ba_window", c, 3, 5, 120, P.BA_OBS, n_fixed_extra=1)) for c in C.IDS]
    res = gpu_handle.ba_solve_visual_batch(cam, cfg, wins)
    r32 = gpu_handle.prepare_ba_batch(wins, obs32=True).solve(cam, cfg)
    neg = gpu_handle.ba_solve_visual_batch(cam, cfg, [C.negate(w, ["poses_cw", "fixed_cw"]) for w in wins])
    for c, w, g, g32, gn in zip(C.IDS, wins, res, r32, neg):
        o = _vis_oracle(w)
        assert g["iterations"] == o["iterations"], c
        assert _rel_err(g["initial_error"], o["initial_error"]) < 1e-12, c
        assert _rel_err(g["final_error"], o["final_error"]) < 1e-8, c
        assert_poses(g["poses_wc"], o["poses_wc"], where=c)
        assert point_errors(g["points"], o["points"]) < TOL, c
        for x in (g32, gn):
            assert (x["iterations"], x["initial_error"], x["final_error"]) == (g["iterations"], g["initial_error"], g["final_error"]), c
            assert x["poses_wc"].tobytes() == g["poses_wc"].tobytes() and x["points"].tobytes() == g["points"].tobytes(), c


# ---- global BA -----------------------------------------------------------------------------------------------------------------------
def _gcfg():
    return O.BaConfig(10, 1e-6, 1e-6, float(np.sqrt(5.991)), 0)      # GlobalBAConfig::default, as tests/test_global_ba.py


def _global_scene(case):
    """the first seed whose oracle solve is well determined: the oracle's dense and Schur forms agree on the final error within 1e-10
    relative and on every point within 1e-7.  With one fixed keyframe the monocular scale is free, and away from the identity the
    additive scaled-axis update of T_cw parameters adds shallow directions: on some scenes the two exact-arithmetic-equivalent forms
    then end 7e-6 apart in the final error after ten iterations, which no implementation can be held to 1e-8 against."""
    for k in range(40):
        seed = 5 + 7919 * k
        w = C.scene("ba_window", case, seed, 6, 150, P.BA_OBS)
        ocam = O.Camera(**w["camera"])
        o = O.global_ba_solve_dense(ocam, _gcfg(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        o2 = O.global_ba_solve_schur(ocam, _gcfg(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        if _rel_err(o2["final_error"], o["final_error"]) < 1e-10 and point_errors(o2["points"], o["points"]) < 1e-7:
            return seed, w, o, o2
    raise AssertionError("no well-determined global BA scene")


@pytest.mark.parametrize("case", C.IDS)
def test_global_ba_parity_and_invariance(gpu_handle, case):
    seed, w, o, o2 = _global_scene(case)
    solve = lambda x: gpu_handle.ba_solve_global(P.CameraModel(**x["camera"]), P.GlobalBAConfig(), x["poses_cw"], x["fixed_cw"][0],
                                                 x["points"], x["obs"])
    g = solve(w)
    global_identity = solve(C.scene("ba_window", "identity", seed, 6, 150, P.BA_OBS))
    assert g["iterations"] == o["iterations"]
    assert _rel_err(g["initial_error"], o["initial_error"]) < 1e-12
    assert _rel_err(g["final_error"], o["final_error"]) < 1e-8
    # one fixed keyframe: the monocular scale is a free gauge, the answer is defined up to the spread between the oracle's own two
    # formulations (the rule of tests/test_global_ba.py and tests/test_fuzz_gpu.py)
    tol = max(TOL, 50.0 * max(np.abs(o2["poses_wc"] - o["poses_wc"]).max(), point_errors(o2["points"], o["points"])))
    assert_poses(g["poses_wc"], o["poses_wc"], tol)
    assert point_errors(g["points"], o["points"]) < tol
    assert _rel_err(g["initial_error"], global_identity["initial_error"]) < 1e-10          # (c)
    gn = solve(C.negate(w, ["poses_cw", "fixed_cw"]))                                       # (b)
    assert gn["iterations"] == g["iterations"] and gn["final_error"] == g["final_error"]
    assert gn["poses_wc"].tobytes() == g["poses_wc"].tobytes() and gn["points"].tobytes() == g["points"].tobytes()


# ---- local inertial BA ---------------------------------------------------------------------------------------------------------------
def _inertial_oracle(w):
    return O.inertial_ba_solve(O.Camera(**w["camera"]), O.inertial_ba_config(), w["poses_wc"], w["velocities"], w["biases"], w["fixed_cw"],
                               w["points"], w["obs"], w["edge_kf"], w["preint"])


def _inertial_gpu(h, w):
    return h.ba_solve_inertial(P.CameraModel(**w["camera"]), P.LocalInertialBAConfig(), w["poses_wc"], w["velocities"], w["biases"],
                               w["fixed_cw"], w["points"], w["obs"], w["edge_kf"], w["preint"])


def _inertial_scene(case, **kw):
    """the first seed whose oracle solve has every accept / reject decision more than MARGIN (relative) from a tie.  Away from R_wc = I
    the reference's mixed Jacobian (T_wc parameters, the T_cw form of the pose block) makes most steps uphill: lambda grows by 10 per
    rejection and the trial cost closes in on the current one — to 4e-7 relative after eight rejections in a row — so a decision can
    come within the two implementations' rounding of a tie."""
    for k in range(40):
        w = C.scene("inertial_window", case, 31 + 7919 * k, 5, 150, P.BA_OBS, n_fixed=2, **kw)
        o = _inertial_oracle(w)
        if C.lm_margin(o["trace"]) >= MARGIN:
            return w, o
    raise AssertionError("no inertial scene with margins")


@pytest.mark.parametrize("case", C.IDS + ["euroc_window_yaw0.4", "euroc_window_yaw-2.9"])
def test_inertial_ba_parity(gpu_handle, case):
    kw = dict(euroc_yaw=float(case.split("yaw")[1])) if case.startswith("euroc_window") else {}
    w, o = _inertial_scene("identity" if kw else case, **kw)
    g = _inertial_gpu(gpu_handle, w)
    assert g["iterations"] == o["iterations"]
    assert _rel_err(g["initial_error"], o["initial_error"]) < 1e-10
    assert _rel_err(g["final_error"], o["final_error"]) < 1e-7
    assert_poses(g["poses_wc"], o["poses_wc"])
    for key in ("velocities", "biases", "points"):
        assert np.max(np.abs(g[key] - o[key])) / max(1.0, np.max(np.abs(o[key]))) < TOL, key       # tests/test_inertial_ba.py's _rel
    # (b): poses through scaled_axis, fixed observers through their rotation matrix, delta_rot through the scaled axis of the error
    # rotation (-dR negates the error quaternion; the `!(w >= 0)` flip undoes it): the same bits
    n = C.negate(C.negate(C.negate(w, ["poses_wc"], alternate=True), ["fixed_cw"]), ["preint"], alternate=True)
    gn = _inertial_gpu(gpu_handle, n)
    assert gn["iterations"] == g["iterations"] and gn["final_error"] == g["final_error"]
    assert all(gn[k].tobytes() == g[k].tobytes() for k in ("poses_wc", "velocities", "biases", "points"))


# ---- PnP-RANSAC ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.IDS)
def test_pnp_parity_truth_and_double_cover(gpu_handle, cam, case):
    for seed, n, outl in ((1, 300, 0.3), (2, 1000, 0.0), (3, 12, 0.0)):
        s = C.scene("pnp_problem", case, 700 + seed, n, outl, 15.0, 0.5)
        g = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"])
        want = NS.solve(s["camera"], s["points3d"], s["points2d"], s["prior_wc"])
        pnp_matches_spec(g, want, (case, seed))
        assert np.abs(g.pose[:4] - want["pose"][:4]).max() < 1e-6, (case, seed)              # the spec's sign, component by component
        if n >= 100:                                                                         # ground truth, anywhere in SO(3)
            assert g.stats["status"] == P.PNP_OK and NS.rotation_angle(g.pose, s["pose_wc"]) < 1e-3
            assert np.linalg.norm(g.pose[4:] - s["pose_wc"][4:]) < 1e-2 and np.array_equal(g.inlier_mask, s["inliers"])
        # (b) the prior's quaternion is carried through every LM step: -prior negates every quaternion of the solve and nothing else.
        # The spec predicts: the pose quaternion negated (by value: IEEE negation, a signed zero may differ), all else byte-identical.
        gn = gpu_handle.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], synth.with_quaternion_signs(s)["prior_wc"])
        assert np.array_equal(-gn.pose[:4], g.pose[:4]) and gn.pose[4:].tobytes() == g.pose[4:].tobytes(), (case, seed)
        assert gn.inlier_mask.tobytes() == g.inlier_mask.tobytes() and gn.reproj_errors.tobytes() == g.reproj_errors.tobytes()
        assert gn.stats == g.stats


# ---- pose-inertial optimization ------------------------------------------------------------------------------------------------------
PI_MARGIN = 1e-4       # as tests/test_pose_inertial_gpu.py: every chi2 the reclassification evaluates this far from its threshold


def _pi_scene(case, seed, n, outliers, stereo, near):
    for k in range(50):
        s = C.scene("pose_inertial_problem", case, seed + 100003 * k, n, outliers, stereo, 2.0, 0.05, near_identity=near)
        want = PS.solve_scene(s)
        if want["margin"] >= PI_MARGIN:
            return s, want
    raise AssertionError("no scene with margins")


def _pi_args(s):
    return (s["pose_wc"], s["velocity"], s["bias"], s["prev_kf_pose_wc"], s["prev_kf_velocity"], s["preint"], s["points3d"], s["points2d"],
            s["is_stereo"])


def _pi_bytes(r):
    return (r.pose.tobytes(), r.velocity.tobytes(), r.bias.tobytes(), r.inlier_mask.tobytes(), r.num_inliers, r.iterations, r.status)


@pytest.mark.parametrize("case", C.IDS)
def test_pose_inertial_parity_and_double_cover(gpu_handle, cam, case):
    for seed, n, outl, stereo, near in ((1, 300, 0.2, 0.5, True), (2, 300, 0.0, 1.0, False), (3, 1000, 0.4, 0.0, True)):
        s, want = _pi_scene(case, 900 + seed, n, outl, stereo, near)
        g = gpu_handle.pose_inertial_optimization(cam, *_pi_args(s))
        pi_matches_spec(g, want, s, (case, seed))
        assert np.abs(g.pose[:4] - want["pose"][:4]).max() < 1e-6, (case, seed)
        # (b) pose_wc through scaled_axis; prev_kf's quaternion through imu_residual_qi, where -q_i negates the error quaternion (undone
        # by the scaled axis' flip) and rotates by the same bits; delta_rot likewise.  The spec predicts every output byte-identical —
        # except for a pose_wc with w = +-0 (atpi), whose two signs give the scaled axes +pi a and -pi a.
        fields = ["prev_kf_pose_wc", "preint"] + ([] if s["pose_wc"][0] == 0.0 else ["pose_wc"])
        gn = gpu_handle.pose_inertial_optimization(cam, *_pi_args(synth.with_quaternion_signs(s, -1.0, fields)))
        assert _pi_bytes(gn) == _pi_bytes(g), (case, seed)


@pytest.mark.parametrize("case", [n for n, _ in C.PLAIN])
def test_pose_inertial_recovers_truth_with_gravity_anywhere(gpu_handle, cam, case):
    """The reference's visual block is the true derivative only at R_wc = I (elsewhere most problems end TOO_FEW), so
    truth recovery is a property of the specification only there.  Here the world is turned by G and then, by a second rotation, the
    current frame's true orientation is put back within 0.05 rad of the identity: gravity, the velocities, the previous keyframe and
    the preintegrated deltas all point anywhere in SO(3) while the visual block stays valid.  2 deg / 5 cm -> 1e-3 rad / 1 cm in four
    iterations, as test_recovers_truth_near_identity."""
    G0 = dict(C.PLAIN)[case]
    for seed in range(3):
        s0 = synth.pose_inertial_problem(seed, 300, 0.0, 0.5, 2.0, 0.05, near_identity=True, G=G0)
        delta = synth.world_rotation(np.random.default_rng(seed).normal(size=3), 0.05)
        G = C.qmul(C.qmul(delta, C.conj(s0["true_pose_wc"][:4])), G0)
        s = synth.pose_inertial_problem(seed, 300, 0.0, 0.5, 2.0, 0.05, near_identity=True, G=G / np.linalg.norm(G))
        assert PS.rotation_angle(s["true_pose_wc"], [1.0, 0, 0, 0]) < 0.051
        g = gpu_handle.pose_inertial_optimization(cam, *_pi_args(s))
        assert g.status == P.POSE_INERTIAL_OK and g.num_inliers == 300, (case, seed)
        assert PS.rotation_angle(g.pose, s["true_pose_wc"]) < 1e-3 and np.linalg.norm(g.pose[4:] - s["true_pose_wc"][4:]) < 1e-2, (case, seed)


# ---- (d) the IMU residual's device function ------------------------------------------------------------------------------------------
def _imu_states(pose_i, pose_j, v_i, v_j):
    return [np.concatenate([O.se3_to_params(p), v]) for p, v in ((pose_i, v_i), (pose_j, v_j))]


def test_imu_residual_device_function_at_euroc_orientations_and_error_rotations_to_pi(gpu_handle):
    """orbx_debug_imu_residual (the device function the inertial BA calls) against the oracle's O.inertial_imu_residual within
    1e-12 * max(1, |block|) per 3-block (tests/test_inertial_ba.py's bound, taken block by block).  The two round the products that form
    the error quaternion in their own ways (fma or not): ~1e-16 absolute, which is why the bound is not relative to a tiny rotation.  At
    error rotations of 1e-8 .. 1e-5 rad it still separates nalgebra's atan2(|v|, |w|) from acos(|w|), which loses ~eps / sin(theta / 2)
    absolute there (the whole angle at 1e-8 rad, where |w| rounds to 1).  States at EuRoC orientations (every yaw), error rotations from
    1e-8 rad up to pi - 1e-9 from below, delta_rot given with both signs."""
    rng = np.random.default_rng(17)
    ladder = [1e-8, 1e-7, 1e-5, 1e-3, 0.1, 1.0, 2.0, 3.0, np.pi - 1e-3, np.pi - 1e-5, np.pi - 1e-7, np.pi - 1e-9, np.pi - 1e-11]
    poses, vel, edges, pre, want = [], [], [], [], []
    for yaw in np.linspace(-np.pi, np.pi, 7):
        qi = C.qmul(synth.euroc_orientation(yaw), synth.world_rotation(rng.normal(size=3), 0.1))
        qj = C.qmul(qi, synth.world_rotation(rng.normal(size=3), 0.02))
        pi, pj, vi, vj = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3), rng.normal(0, 0.5, 3), rng.normal(0, 0.5, 3)
        for ang in ladder:
            if np.pi - ang < 1e-9:
                # within 1e-9 of the half turn, w of the error quaternion is ~1e-10 or less: one rounding of the three products that
                # form it (host vs device, fma or not) can flip its sign, and the residual jumps from +pi a to -pi a — both right
                continue
            E = synth.world_rotation(rng.normal(size=3), ang)                 # the error rotation dR^-1 R_i^-1 R_j to be produced
            dR = C.qmul(C.qmul(C.conj(qi), qj), C.conj(E))
            dv, dp = rng.normal(0, 0.3, 3), rng.normal(0, 0.1, 3)
            for sgn in (1.0, -1.0):
                k = len(poses)
                poses += [np.concatenate([qi, pi]), np.concatenate([qj, pj])]
                vel += [vi, vj]
                edges.append((k, k + 1))
                pre.append(np.concatenate([sgn * dR, dv, dp, [0.05]]))
                si, sj = _imu_states(poses[k], poses[k + 1], vi, vj)
                want.append(O.inertial_imu_residual(si, sj, pre[-1]))
    got = gpu_handle.debug_imu_residual(np.array(poses), np.array(vel), np.array(edges), np.array(pre))
    want = np.array(want)
    for e in range(len(want)):
        for b in range(3):
            w_, g_ = want[e, 3 * b:3 * b + 3], got[e, 3 * b:3 * b + 3]
            assert np.abs(g_ - w_).max() <= 1e-12 * max(1.0, np.abs(w_).max()), (e, b, g_, w_)
    # the oracle itself: the error rotation comes back, its angle within 1e-9 rad (the products that form it round at ~1e-16 each)
    kept = [a for a in ladder if np.pi - a >= 1e-9]
    angs = np.linalg.norm(want[0::2, :3], axis=1).reshape(-1, len(kept))
    assert np.abs(angs - np.array(kept)).max() < 1e-9
