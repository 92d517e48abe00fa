"""The world-rotation option of the scene generators (synth: G, euroc_yaw, with_quaternion_signs) and the double cover q / -q on the
CPU oracle and the numpy restatements.  The GPU side is tests/test_orientation_gpu.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import orb_slam3_rust_amd as P
from oracle import oracle as O
import orientation_cases as C
import pnp_spec as NS
import pose_inertial_spec as PS

synth = P.synth
HERE = os.path.dirname(os.path.abspath(__file__))


def digest(scene):
    """sha256 over a scene's fields in name order: name, dtype, shape and bytes of every array; the camera dict by repr"""
    h = hashlib.sha256()
    for k in sorted(scene):
        v = scene[k]
        h.update(k.encode())
        if isinstance(v, dict):
            h.update(repr(sorted(v.items())).encode())
        else:
            a = np.ascontiguousarray(v)
            h.update(str(a.dtype).encode() + repr(a.shape).encode() + a.tobytes())
    return h.hexdigest()


DEFAULT_SCENES = {
    "ba_window(1,6,150)": lambda: synth.ba_window(1, 6, 150, P.BA_OBS),
    "ba_window(3,8,300,n_fixed_extra=2)": lambda: synth.ba_window(3, 8, 300, P.BA_OBS, n_fixed_extra=2),
    "inertial_window(2,5,150)": lambda: synth.inertial_window(2, 5, 150, P.BA_OBS),
    "inertial_window(6,4,90,n_fixed=0)": lambda: synth.inertial_window(6, 4, 90, P.BA_OBS, n_fixed=0),
    "pnp_problem(11,300,0.3,10,0.3)": lambda: synth.pnp_problem(11, 300, 0.3, 10.0, 0.3),
    "pnp_problem(4,5,0,10,0.3)": lambda: synth.pnp_problem(4, 5, 0.0, 10.0, 0.3),
    "pose_inertial_problem(3,300,0.2,0.5,2,0.05)": lambda: synth.pose_inertial_problem(3, 300, 0.2, 0.5, 2.0, 0.05),
    "pose_inertial_problem(8,200,0,0.5,1,0.02,near,imu_noise)":
        lambda: synth.pose_inertial_problem(8, 200, 0.0, 0.5, 1.0, 0.02, near_identity=True, imu_noise=1e-3),
}


def test_default_scenes_are_unchanged():
    """G=None (the default) gives every generator's scenes bit for bit as before the option existed: the digests in
    tests/golden/synth_default_digests.json were taken from the generators without it."""
    with open(os.path.join(HERE, "golden", "synth_default_digests.json")) as f:
        want = json.load(f)
    assert set(want) == set(DEFAULT_SCENES)
    for name, fn in DEFAULT_SCENES.items():
        assert digest(fn()) == want[name], name
    # G = the identity quaternion turns nothing (compared by value: a product with 1 and 0s may change the sign of a zero)
    s0 = synth.ba_window(1, 6, 150, P.BA_OBS)
    s1 = synth.ba_window(1, 6, 150, P.BA_OBS, G=[1.0, 0.0, 0.0, 0.0])
    for k in ("poses_cw", "fixed_cw", "points", "gt_points"):
        assert np.array_equal(s0[k], s1[k]), k


def test_cases_cover_the_double_cover_and_the_edges():
    """half of the random rotations have w < 0; pi + 1e-9 has w < 0; pi has w == 0 exactly; the anchored cases put the anchor pose on
    its edge"""
    plain = dict(C.PLAIN)
    assert sum(plain["random%d" % i][0] < 0 for i in range(4)) == 2
    assert plain["pi+1e-9"][0] < 0 < plain["pi-1e-9"][0] and plain["pi"][0] == 0.0
    for case in ("at1e-9", "atpi"):
        s = C.scene("ba_window", case, 1, 6, 150, P.BA_OBS, n_fixed_extra=2)
        assert s["poses_cw"][0, :4].tobytes() == dict(C.ANCHORED)[case].tobytes()
    p = O.se3_to_params(np.concatenate([dict(C.ANCHORED)["at1e-12"], [0.0, 0.0, 0.0]]))
    assert 0 < np.linalg.norm(p[:3]) < 1e-10 < np.linalg.norm(O.se3_to_params(np.concatenate([dict(C.ANCHORED)["at1e-9"], [0, 0, 0.0]]))[:3])


def _reproject(cam, pose_cw, X):
    pc = synth._quat_rot(pose_cw[:4], X) + pose_cw[4:]
    return np.stack([cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"], cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]], 1)


@pytest.mark.parametrize("case", [n for n, _ in C.PLAIN])
def test_turned_scenes_are_consistent(case):
    """A turned scene is the same scene: every ground-truth camera sees every ground-truth point where it did (1e-9 px: rounding of
    10 m coordinates through one more rotation), and the inertial window's exact deltas — recomputed against the fixed world gravity —
    still give a ground-truth IMU residual of the noise only (the same bound as tests/test_inertial_ba.py), with the same noise."""
    G = dict(C.PLAIN)[case]
    a, b = synth.ba_window(4, 5, 120, P.BA_OBS), synth.ba_window(4, 5, 120, P.BA_OBS, G=G)
    assert a["obs"].tobytes() == b["obs"].tobytes()
    for k in range(len(a["gt_poses_cw"])):
        assert np.abs(_reproject(a["camera"], a["gt_poses_cw"][k], a["gt_points"]) -
                      _reproject(b["camera"], b["gt_poses_cw"][k], b["gt_points"])).max() < 1e-9
    for kw in (dict(G=G), dict(euroc_yaw=0.7), dict(G=G, euroc_yaw=-2.0)):
        w0, w = synth.inertial_window(3, 5, 60, P.BA_OBS), synth.inertial_window(3, 5, 60, P.BA_OBS, **kw)
        assert w0["obs"].tobytes() == w["obs"].tobytes() and np.array_equal(w0["preint"][:, :4], w["preint"][:, :4])
        for e, (i, j) in enumerate(w["edge_kf"]):
            st = [np.concatenate([O.se3_to_params(w["gt_poses_wc"][k]), w["gt_velocities"][k]]) for k in (i, j)]
            st0 = [np.concatenate([O.se3_to_params(w0["gt_poses_wc"][k]), w0["gt_velocities"][k]]) for k in (i, j)]
            r, r0 = O.inertial_imu_residual(st[0], st[1], w["preint"][e]), O.inertial_imu_residual(st0[0], st0[1], w0["preint"][e])
            assert np.abs(r - r0).max() < 1e-9, (kw, e)
    # the EuRoC orientation: the optical axis horizontal, gravity in the image plane pointing down the image
    w = synth.inertial_window(3, 5, 60, P.BA_OBS, euroc_yaw=0.7)
    R = PS.qrot(w["gt_poses_wc"][0, :4], np.eye(3))                     # rows: the camera's x, y, z axes in the world
    assert abs(R[2, 2]) < 0.1 and R[1, 2] < -0.99
    p, q = synth.pnp_problem(6, 50, 0.2, 10.0, 0.3), synth.pnp_problem(6, 50, 0.2, 10.0, 0.3, G=G)
    assert p["points2d"].tobytes() == q["points2d"].tobytes()
    assert NS.detailed(p["camera"], q["pose_wc"], q["points3d"], p["points2d"].astype(np.float64), 8.0)[1].tolist() == p["inliers"].tolist()
    s0, s = (synth.pose_inertial_problem(7, 50, 0.0, 0.5, 2.0, 0.05, imu_noise=0.0, G=g) for g in (None, G))
    assert np.abs(PS.imu_residual(s["prev_kf_pose_wc"], s["prev_kf_velocity"], s["true_pose_wc"], s["true_velocity"], s["preint"])).max() < 1e-12


def test_with_quaternion_signs():
    s = synth.inertial_window(2, 4, 40, P.BA_OBS)
    n = synth.with_quaternion_signs(s)
    for k in ("poses_wc", "fixed_cw", "preint"):
        assert np.array_equal(n[k][:, :4], -s[k][:, :4]) and n[k][:, 4:].tobytes() == s[k][:, 4:].tobytes(), k
    assert n["gt_poses_wc"] is s["gt_poses_wc"]                              # ground truth is not a solver input
    m = synth.with_quaternion_signs(s, {"poses_wc": [1, -1, 1, -1]}, fields=["poses_wc"])
    assert np.array_equal(m["poses_wc"][:, 0], s["poses_wc"][:, 0] * np.array([1, -1, 1, -1])) and m["preint"] is s["preint"]
    s = synth.pose_inertial_problem(1, 10, 0.0, 0.5, 2.0, 0.05)
    p = synth.with_quaternion_signs(s)
    for k in ("pose_wc", "prev_kf_pose_wc", "preint"):
        assert p[k].shape == s[k].shape and np.array_equal(p[k][:4], -s[k][:4]) and p[k][4:].tobytes() == s[k][4:].tobytes(), k


# ---- the double cover on the oracle and the specs ------------------------------------------------------------------------------------
def _flip_some(scene, fields, rng):
    signs = {}
    for f in fields:
        n = len(np.asarray(scene[f]).reshape(-1, np.asarray(scene[f]).shape[-1]))
        signs[f] = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        signs[f][0] = -1.0
    return synth.with_quaternion_signs(scene, signs, fields)


def test_oracle_se3_to_params_double_cover():
    """nalgebra's scaled_axis is the same for q and -q (the `!(w >= 0)` flip) except at w = +-0, where both signs count as
    non-negative: q = (+0, v) and -q = (-0, -v) give +pi v and -pi v, the same rotation"""
    rng = np.random.default_rng(3)
    for q in list(rng.normal(size=(50, 4))) + [dict(C.PLAIN)["pi+1e-9"], dict(C.PLAIN)["pi-1e-9"]]:
        q = q / np.linalg.norm(q)
        p = np.concatenate([q, [1.0, 2.0, 3.0]])
        assert O.se3_to_params(p).tobytes() == O.se3_to_params(np.concatenate([-q, p[4:]])).tobytes()
        assert PS.scaled_axis(q).tobytes() == PS.scaled_axis(-q).tobytes()
    q = dict(C.PLAIN)["pi"]
    a, b = O.se3_to_params(np.concatenate([q, [0, 0, 0.0]])), O.se3_to_params(np.concatenate([-q, [0, 0, 0.0]]))
    assert np.array_equal(a[:3], -b[:3]) and abs(np.linalg.norm(a[:3]) - np.pi) < 1e-15


@pytest.mark.parametrize("case", ["identity", "euroc_yaw2.3", "random1", "pi+1e-9", "at1e-9", "atpi-1e-9"])
def test_oracle_double_cover_bit_for_bit(case):
    """Every quaternion the visual and inertial solvers take is turned into a scaled axis (poses, the IMU error rotation) or a rotation
    matrix (fixed observers) before it is used; both are the same for q and -q.  So the oracle's results are byte-identical."""
    rng = np.random.default_rng(11)
    w = C.scene("ba_window", case, 2, 6, 150, P.BA_OBS, n_fixed_extra=2)
    n = _flip_some(w, ["poses_cw", "fixed_cw"], rng)
    for fn in (O.ba_solve_dense, O.ba_solve_schur):
        a = fn(O.Camera(**w["camera"]), O.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
        b = fn(O.Camera(**w["camera"]), O.ba_config(), n["poses_cw"], n["fixed_cw"], n["points"], n["obs"])
        assert all(a[k].tobytes() == b[k].tobytes() for k in ("poses_wc", "points", "trace")) and a["iterations"] == b["iterations"]
    wi = C.scene("inertial_window", case, 3, 4, 100, P.BA_OBS, n_fixed=1)
    ni = _flip_some(wi, ["poses_wc", "fixed_cw", "preint"], rng)
    a, b = (O.inertial_ba_solve(O.Camera(**x["camera"]), O.inertial_ba_config(), x["poses_wc"], x["velocities"], x["biases"], x["fixed_cw"],
                                x["points"], x["obs"], x["edge_kf"], x["preint"]) for x in (wi, ni))
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("poses_wc", "velocities", "biases", "points", "trace"))


@pytest.mark.parametrize("case", ["identity", "euroc_yaw2.3", "random0", "random3", "pi+1e-9", "atpi"])
def test_spec_double_cover(case):
    """PnP carries the prior's quaternion through every LM step (a product with exp(delta) on the left) and returns its inverse: with
    -prior, every quaternion of the solve is the exact negation of the one with +prior and every rotation matrix, residual, cost and
    decision is the same.  Prediction: the pose quaternion negated (IEEE negation, so compared by value: a signed zero may differ),
    the translation, inlier mask, errors and statistics byte-identical.  Pose-inertial: pose_wc enters through scaled_axis; prev_kf
    enters the IMU residual as a quaternion (imu_residual_qi), where -q_i negates the error quaternion, whose scaled_axis is then the
    same, and the rotations by -q_i are bit-identical; delta_rot likewise.  Prediction: every output byte-identical."""
    s = C.scene("pnp_problem", case, 17, 200, 0.3, 10.0, 0.3)
    a = NS.solve(s["camera"], s["points3d"], s["points2d"], s["prior_wc"])
    b = NS.solve(s["camera"], s["points3d"], s["points2d"], synth.with_quaternion_signs(s)["prior_wc"])
    assert np.array_equal(-a["pose"][:4], b["pose"][:4]) and a["pose"][4:].tobytes() == b["pose"][4:].tobytes()
    for k in ("inlier_mask", "reproj_errors", "counts"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(a[k] == b[k] for k in ("status", "ransac_inliers", "best_hypothesis", "hypotheses_evaluated", "refine_iterations"))
    p = C.scene("pose_inertial_problem", case, 5, 200, 0.2, 0.5, 2.0, 0.05, near_identity=True)
    want = PS.solve_scene(p)
    for fields in (["pose_wc"], ["prev_kf_pose_wc"], ["preint"], ["pose_wc", "prev_kf_pose_wc", "preint"]):
        if "pose_wc" in fields and p["pose_wc"][0] == 0.0:
            continue        # w = +-0 (atpi): scaled_axis gives +pi a and -pi a (test_oracle_se3_to_params_double_cover), no longer the same bits
        got = PS.solve_scene(synth.with_quaternion_signs(p, -1.0, fields))
        for k in ("pose", "velocity", "bias", "inlier_mask"):
            assert got[k].tobytes() == want[k].tobytes(), (fields, k)
        assert (got["iterations"], got["status"], got["num_inliers"]) == (want["iterations"], want["status"], want["num_inliers"])


@pytest.mark.parametrize("case", [n for n, _ in C.PLAIN])
def test_pnp_spec_recovers_truth_over_so3(case):
    """the restatement itself recovers the ground truth at every world rotation (the GPU is held to the same in the GPU file)"""
    s = synth.pnp_problem(23, 300, 0.3, 15.0, 0.5, G=dict(C.PLAIN)[case])
    r = NS.solve(s["camera"], s["points3d"], s["points2d"], s["prior_wc"])
    assert r["status"] == NS.OK and NS.rotation_angle(r["pose"], s["pose_wc"]) < 1e-3
    assert np.linalg.norm(r["pose"][4:] - s["pose_wc"][4:]) < 1e-2 and np.array_equal(r["inlier_mask"], s["inliers"])
