"""Pose-inertial optimization on the GPU (orbx_pose_inertial_*, pose_inertial_kernels.hip) against the numpy restatement of the
reference (tests/pose_inertial_spec.py); single, batch and device forms against each other byte for byte; PnP chained into it on the
device; the C++ and module-level mirrors."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_inertial_spec as S
from test_pose_inertial_cpu import build_pose_inertial_driver

pytestmark = pytest.mark.gpu

MARGIN = 1e-4


@pytest.fixture(scope="module")
def cam(pkg):
    return pkg.CameraModel(**pkg.synth.EUROC_CAMERA)


def scene(pkg, seed, n, outliers, stereo, near, cfg=None):
    """A scene whose every chi2 the specification evaluates lies more than MARGIN (relative) from its threshold: a mask flip can then
    not be blamed on rounding.  Returns (scene, the specification's result)."""
    for k in range(50):
        s = pkg.synth.pose_inertial_problem(seed + 100003 * k, n, outliers, stereo, 2.0, 0.05, near_identity=near)
        want = S.solve_scene(s, cfg)
        if want["margin"] >= MARGIN:
            return s, want
    raise AssertionError("no scene with margins")


def args(s):
    return (s["pose_wc"], s["velocity"], s["bias"], s["prev_kf_pose_wc"], s["prev_kf_velocity"], s["preint"], s["points3d"], s["points2d"],
            s["is_stereo"])


def assert_matches_spec(g, want, s, where=""):
    assert (g.iterations, g.status, g.num_inliers, g.num_observations) == \
        (want["iterations"], want["status"], want["num_inliers"], want["num_observations"]), where
    assert np.array_equal(g.inlier_mask, want["inlier_mask"]), where
    assert g.bias.tobytes() == np.asarray(s["bias"], np.float64).tobytes(), where
    ang = S.rotation_angle(g.pose, want["pose"])
    dt = np.linalg.norm(g.pose[4:] - want["pose"][4:]) / max(np.linalg.norm(want["pose"][4:]), 1e-12)
    dv = np.linalg.norm(g.velocity - want["velocity"]) / max(np.linalg.norm(want["velocity"]), 1e-12)
    assert ang < 1e-6 and dt < 1e-6 and dv < 1e-6, (where, ang, dt, dv)


def _bytes(r):
    return (r.pose.tobytes(), r.velocity.tobytes(), r.bias.tobytes(), r.inlier_mask.tobytes(), r.num_inliers, r.num_observations,
            r.iterations, r.status)


@pytest.mark.parametrize("near", [True, False])
@pytest.mark.parametrize("n", [0, 3, 5, 10, 300, 2000])
def test_parity_with_spec(gpu_handle, cam, pkg, n, near):
    statuses = set()
    for oi, outliers in enumerate((0.0, 0.2, 0.4)):
        for si, stereo in enumerate((0.0, 0.5, 1.0)):
            for wi, w in enumerate((0.0, 1.0, 10.0)):
                cfg = dict(imu_weight=w)
                s, want = scene(pkg, 7919 * n + 97 * oi + 13 * si + wi + (5 if near else 0), n, outliers, stereo, near, cfg)
                g = gpu_handle.pose_inertial_optimization(cam, *args(s), cfg=pkg.PoseInertialConfig(imu_weight=w))
                assert_matches_spec(g, want, s, (n, near, outliers, stereo, w))
                statuses.add(g.status)
    if n < 5:
        assert statuses == {pkg.POSE_INERTIAL_TOO_FEW}


def test_recovers_truth_near_identity(gpu_handle, cam, pkg):
    for seed in range(4):
        s = pkg.synth.pose_inertial_problem(seed, 300, 0.0, 0.5, 2.0, 0.05, near_identity=True)
        g = gpu_handle.pose_inertial_optimization(cam, *args(s))
        assert g.status == pkg.POSE_INERTIAL_OK and g.iterations == 4 and g.num_inliers == 300
        assert S.rotation_angle(g.pose, s["true_pose_wc"]) < 1e-3 and np.linalg.norm(g.pose[4:] - s["true_pose_wc"][4:]) < 1e-2


def test_zero_and_one_iteration(gpu_handle, cam, pkg):
    s, _ = scene(pkg, 3, 300, 0.2, 0.5, False)
    g = gpu_handle.pose_inertial_optimization(cam, *args(s), cfg=pkg.PoseInertialConfig(max_iterations=0))
    assert (g.iterations, g.status, g.num_inliers) == (0, pkg.POSE_INERTIAL_OK, 300) and g.inlier_mask.all()
    # the state round-trips through the parameters: translation, velocity and bias by value, the rotation through scaled_axis
    assert g.pose[4:].tobytes() == s["pose_wc"][4:].tobytes() and g.velocity.tobytes() == s["velocity"].tobytes()
    assert g.bias.tobytes() == s["bias"].tobytes()
    assert np.abs(g.pose[:4] - S.extract_pose(S.params_from_state(s["pose_wc"], s["velocity"], s["bias"]))[:4]).max() < 1e-15
    for near in (True, False):
        s, want = scene(pkg, 4, 500, 0.3, 0.5, near, dict(max_iterations=1))
        g = gpu_handle.pose_inertial_optimization(cam, *args(s), cfg=pkg.PoseInertialConfig(max_iterations=1))
        assert g.iterations == 1
        assert_matches_spec(g, want, s, near)        # progress 0: the *_init thresholds


def test_every_point_behind_the_camera(gpu_handle, cam, pkg):
    s = pkg.synth.pose_inertial_problem(8, 200, 0.0, 0.5, 1.0, 0.02, near_identity=True)
    t = s["true_pose_wc"][4:]
    s["points3d"] = 2.0 * t - s["points3d"]                 # z_c -> -z_c
    g = gpu_handle.pose_inertial_optimization(cam, *args(s))
    want = S.solve_scene(s)
    # iteration 1: every observation active with e = (100, 100) and a zero block, then masked out; iteration 2: too few
    assert (g.iterations, g.status, g.num_inliers) == (2, pkg.POSE_INERTIAL_TOO_FEW, 0) and not g.inlier_mask.any()
    assert_matches_spec(g, want, s)


def test_invalid_configs(gpu_handle, cam, pkg):
    s = pkg.synth.pose_inertial_problem(9, 20, 0.0, 0.5, 1.0, 0.02)
    bad = [dict(max_iterations=-1), dict(max_iterations=65), dict(chi2_mono_init=0.0), dict(chi2_stereo_init=-1.0),
           dict(chi2_mono_final=float("nan")), dict(chi2_stereo_final=0.0), dict(imu_weight=-1.0), dict(imu_weight=float("inf")),
           dict(imu_weight=float("nan"))]
    for b in bad:
        with pytest.raises(pkg.OrbxError) as e:
            gpu_handle.pose_inertial_optimization(cam, *args(s), cfg=pkg.PoseInertialConfig(**b))
        assert e.value.code == -1, b
    g = gpu_handle.pose_inertial_optimization(cam, *args(s), cfg=pkg.PoseInertialConfig(max_iterations=64, imu_weight=0.0))
    assert g.iterations >= 1


def _mixed(pkg, count):
    sizes = [0, 3, 5, 10, 50, 300, 1000, 2000]
    out = []
    for i in range(count):
        s = pkg.synth.pose_inertial_problem(5000 + i, sizes[i % len(sizes)], (0.0, 0.2, 0.4)[i % 3], (0.0, 0.5, 1.0)[i % 5 % 3],
                                            2.0, 0.05, near_identity=bool(i % 2))
        out.append(s)
    return out


def _stack(pkg, scenes, dev):
    import torch
    n = np.array([len(s["points3d"]) for s in scenes])
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([s[k] for s in scenes]), dt)
    stk = lambda k: np.ascontiguousarray(np.stack([s[k] for s in scenes]), np.float64)
    host = [off, cat("points3d", np.float64), cat("points2d", np.float32), cat("is_stereo", np.uint8)] + \
           [stk(k) for k in ("pose_wc", "velocity", "bias", "prev_kf_pose_wc", "prev_kf_velocity", "preint")]
    return off, [torch.from_numpy(a).to(dev) for a in host]


def test_batch_equals_singles_equals_device(gpu_handle, cam, pkg):
    import torch
    scenes = _mixed(pkg, 512)
    batch = gpu_handle.pose_inertial_optimization_batch(cam, [args(s) for s in scenes])
    statuses = set()
    for i, (s, b) in enumerate(zip(scenes, batch)):
        one = gpu_handle.pose_inertial_optimization(cam, *args(s))
        assert _bytes(one) == _bytes(b), i
        statuses.add(b.status)
    assert {pkg.POSE_INERTIAL_OK, pkg.POSE_INERTIAL_TOO_FEW} <= statuses
    off, t = _stack(pkg, scenes, torch.device("cuda", 0))
    poses, vel, bias, inl, res = gpu_handle.pose_inertial_optimization_batch_device(cam, *t)
    torch.cuda.synchronize()
    poses, vel, bias, inl = poses.cpu().numpy(), vel.cpu().numpy(), bias.cpu().numpy(), inl.cpu().numpy()
    res = res.cpu().numpy().view(pkg.POSE_INERTIAL_RESULT).reshape(-1)
    for p, b in enumerate(batch):
        got = (poses[p].tobytes(), vel[p].tobytes(), bias[p].tobytes(), inl[off[p]:off[p + 1]].tobytes(), int(res[p]["num_inliers"]),
               int(res[p]["num_observations"]), int(res[p]["iterations"]), int(res[p]["status"]))
        assert got == _bytes(b), p


def test_pnp_chained_into_pose_inertial_on_device(gpu_handle, cam, pkg):
    """The tracker's PnP -> refine_with_imu sequence with no host round trip: the PnP device batch's offsets / points and output poses
    go straight into the pose-inertial device batch; the result equals PnP's host batch followed by the pose-inertial host batch."""
    import torch
    scenes = _mixed(pkg, 96)
    dev = torch.device("cuda", 0)
    off, t = _stack(pkg, scenes, dev)
    max_n = int(np.diff(off).max())
    pnp_poses, _, _, _ = gpu_handle.solve_pnp_ransac_batch_device(cam, t[0], t[1], t[2], t[4], max_n)
    poses, vel, bias, inl, res = gpu_handle.pose_inertial_optimization_batch_device(cam, t[0], t[1], t[2], t[3], pnp_poses, *t[5:])
    torch.cuda.synchronize()
    pnp_host = gpu_handle.solve_pnp_ransac_batch(cam, [(s["points3d"], s["points2d"], s["pose_wc"]) for s in scenes])
    host = gpu_handle.pose_inertial_optimization_batch(
        cam, [(r.pose,) + args(s)[1:] for r, s in zip(pnp_host, scenes)])
    poses, vel, bias, inl = poses.cpu().numpy(), vel.cpu().numpy(), bias.cpu().numpy(), inl.cpu().numpy()
    res = res.cpu().numpy().view(pkg.POSE_INERTIAL_RESULT).reshape(-1)
    for p, h in enumerate(host):
        got = (poses[p].tobytes(), vel[p].tobytes(), bias[p].tobytes(), inl[off[p]:off[p + 1]].tobytes(), int(res[p]["num_inliers"]),
               int(res[p]["num_observations"]), int(res[p]["iterations"]), int(res[p]["status"]))
        assert got == _bytes(h), p


def test_deterministic(gpu_handle, cam, pkg):
    s = pkg.synth.pose_inertial_problem(21, 2000, 0.3, 0.5, 2.0, 0.05)
    a = gpu_handle.pose_inertial_optimization(cam, *args(s))
    b = gpu_handle.pose_inertial_optimization(cam, *args(s))
    assert _bytes(a) == _bytes(b)


def test_module_level_function_equals_handle(gpu_handle, cam, pkg):
    s = pkg.synth.pose_inertial_problem(22, 400, 0.2, 0.5, 2.0, 0.05, near_identity=True)
    r = pkg.pose_inertial_optimization(s["pose_wc"], s["velocity"], s["bias"], s["prev_kf_pose_wc"], s["prev_kf_velocity"],
                                       np.full(6, 7.0), s["preint"], (s["points3d"], s["points2d"], s["is_stereo"]), cam)
    g = gpu_handle.pose_inertial_optimization(cam, *args(s))
    assert _bytes(r) == _bytes(g)


def test_cpp_mirror_equals_python(gpu_handle, cam, pkg, tmp_path):
    exe = build_pose_inertial_driver(str(tmp_path))
    for seed, n, near in ((3, 500, True), (4, 2, False), (5, 200, False)):
        s = pkg.synth.pose_inertial_problem(seed, n, 0.2, 0.5, 2.0, 0.05, near_identity=near)
        fin, fout = os.path.join(tmp_path, "in.bin"), os.path.join(tmp_path, "out.bin")
        with open(fin, "wb") as f:
            f.write(struct.pack("<i", n))
            for k in ("pose_wc", "velocity", "bias", "prev_kf_pose_wc", "prev_kf_velocity", "preint"):
                f.write(np.ascontiguousarray(s[k], np.float64).tobytes())
            f.write(np.ascontiguousarray(s["points3d"]).tobytes()); f.write(np.ascontiguousarray(s["points2d"]).tobytes())
            f.write(np.ascontiguousarray(s["is_stereo"], np.uint8).tobytes())
        subprocess.run([exe, fin, fout], check=True, timeout=120)
        out = open(fout, "rb").read()
        g = gpu_handle.pose_inertial_optimization(cam, *args(s))
        assert out == g.pose.tobytes() + g.velocity.tobytes() + g.bias.tobytes() + struct.pack("<3Q", g.num_inliers, g.num_observations,
                                                                                                  g.iterations)
