"""Pose-inertial optimization (pose_inertial_optimization, src/optimizer/pose_inertial_optim.rs:94-216) without a GPU: the ABI's
defaults and layouts, the numpy restatement (tests/pose_inertial_spec.py) against the oracle's IMU residual, the reference's own unit
tests, the properties the specification implies, ground-truth recovery where the reference's Jacobian holds, and the C++ mirror's
build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_inertial_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb-slam3-rust_amd")
CAM = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, baseline=0.11007)


def build_pose_inertial_driver(tmp):
    exe = os.path.join(tmp, "pose_inertial_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "pose_inertial_driver.cpp"), "-o", exe, "-L", LIBDIR, "-lorbx_hip",
                    "-Wl,-rpath," + LIBDIR], check=True)
    return exe


def test_default_config_mirrors_reference(pkg):
    from orb_slam3_rust_amd.api import _PoseInertialConfig
    L = pkg.load_library()                       # loads without a device
    c = _PoseInertialConfig()
    L.orbx_default_pose_inertial_config(C.byref(c))
    got = {k: getattr(c, k) for k, _ in _PoseInertialConfig._fields_}
    # pose_inertial_optim.rs:34-45
    assert got == S.DEFAULTS == dict(max_iterations=4, chi2_mono_init=12.0, chi2_stereo_init=15.6, chi2_mono_final=5.991,
                                     chi2_stereo_final=7.815, imu_weight=1.0)
    assert got == {k: getattr(pkg.PoseInertialConfig(), k) for k in got}


def test_config_and_result_layouts_match_header(pkg, tmp_path):
    from orb_slam3_rust_amd.api import _PoseInertialConfig, _PoseInertialResult
    src = tmp_path / "lay.c"
    fields_c = [f for f, _ in _PoseInertialConfig._fields_]
    fields_r = [f for f, _ in _PoseInertialResult._fields_]
    args = ["sizeof(orbx_pose_inertial_config)"] + ["offsetof(orbx_pose_inertial_config, %s)" % f for f in fields_c]
    args += ["sizeof(orbx_pose_inertial_result)"] + ["offsetof(orbx_pose_inertial_result, %s)" % f for f in fields_r]
    args += ["ORBX_POSE_INERTIAL_OK", "ORBX_POSE_INERTIAL_TOO_FEW", "ORBX_POSE_INERTIAL_SINGULAR", "ORBX_ABI_VERSION"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "orbx.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n'
                   % (" ".join(["%zu"] * (len(args) - 4) + ["%d"] * 4), ", ".join(args)))
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [C.sizeof(_PoseInertialConfig)] + [getattr(_PoseInertialConfig, f).offset for f in fields_c]
    want += [C.sizeof(_PoseInertialResult)] + [getattr(_PoseInertialResult, f).offset for f in fields_r]
    want += [pkg.POSE_INERTIAL_OK, pkg.POSE_INERTIAL_TOO_FEW, pkg.POSE_INERTIAL_SINGULAR, 2]
    assert got == want
    assert pkg.POSE_INERTIAL_RESULT.itemsize == C.sizeof(_PoseInertialResult) == 16
    assert [pkg.POSE_INERTIAL_RESULT.fields[f][1] for f in fields_r] == [getattr(_PoseInertialResult, f).offset for f in fields_r]


def test_spec_imu_residual_equals_oracle(pkg, oracle):
    """The spec's compute_imu_residual against the oracle's (state = scaled axis | t | v per keyframe)."""
    for seed in range(20):
        s = pkg.synth.pose_inertial_problem(seed, 0, 0.0, 0.0, 3.0, 0.1, near_identity=bool(seed % 2), imu_noise=0.01 * (seed % 3))
        si = np.concatenate([S.scaled_axis(s["prev_kf_pose_wc"][:4]), s["prev_kf_pose_wc"][4:], s["prev_kf_velocity"]])
        sj = np.concatenate([S.scaled_axis(s["pose_wc"][:4]), s["pose_wc"][4:], s["velocity"]])
        want = oracle.inertial_imu_residual(si, sj, s["preint"])
        got = S.imu_residual(S.extract_pose(si), si[6:9], S.extract_pose(sj), sj[6:9], s["preint"])
        assert np.allclose(got, want, rtol=1e-12, atol=1e-13), (seed, got - want)
        # the exact preintegration of the true motion: zero residual at the truth
        r0 = S.imu_residual(s["prev_kf_pose_wc"], s["prev_kf_velocity"], s["true_pose_wc"], s["true_velocity"], s["preint"])
        assert seed % 3 or np.abs(r0).max() < 1e-12


def test_reference_unit_tests():
    # test_pose_extraction (:436-452)
    p = np.zeros(15)
    p[:6] = [0.1, 0.2, 0.3, 1.0, 2.0, 3.0]
    pose = S.extract_pose(p)
    assert np.abs(pose[4:] - [1.0, 2.0, 3.0]).max() < 1e-10
    # test_pose_inertial_optimization_no_observations (:454-477): identity state, identity preintegration, default config
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    pre = np.array([1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0])
    r = S.solve(CAM, ident, np.zeros(3), np.zeros(6), ident, np.zeros(3), pre, np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0))
    assert r["num_observations"] == 0 and r["iterations"] == 1 and r["status"] == S.TOO_FEW and r["num_inliers"] == 0
    assert r["pose"].tobytes() == ident.tobytes()


def test_scaled_axis_round_trip_and_lu():
    rng = np.random.default_rng(0)
    for _ in range(50):
        r = rng.normal(size=3)
        r *= rng.uniform(0, 3) / np.linalg.norm(r)            # an angle below pi: the round trip is the identity
        assert np.allclose(S.scaled_axis(S.from_scaled_axis(r)), r, atol=1e-12)
    q = np.array([-0.5, 0.5, 0.5, 0.5])                       # w < 0: the axis flips, the angle stays below pi
    assert np.allclose(S.scaled_axis(q), -np.array([1, 1, 1]) / np.sqrt(3) * (2 * np.pi / 3))
    assert not S.scaled_axis(np.array([1.0, 0, 0, 0])).any()
    for n in (3, 7, 15):
        A = rng.normal(size=(n, n)); b = rng.normal(size=n)
        assert np.allclose(S.lu_solve(A, b), np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)
    assert S.lu_solve(np.array([[1.0, 2.0], [2.0, 4.0]]), np.ones(2)) is None      # an exactly zero pivot
    assert S.lu_solve(np.zeros((3, 3)), np.ones(3)) is None


@pytest.mark.parametrize("near", [True, False])
def test_bias_comes_back_unchanged(pkg, near):
    """The residual does not read the bias: its columns of J are exactly zero, the damped H has 1e-9 on their diagonal and zeros
    beside it, the gradient is zero there, and delta is +-0."""
    for seed in range(6):
        s = pkg.synth.pose_inertial_problem(seed, 300, 0.3, 0.5, 2.0, 0.05, near_identity=near)
        for w in (0.0, 1.0, 10.0):
            r = S.solve_scene(s, dict(imu_weight=w))
            assert r["bias"].tobytes() == s["bias"].tobytes()
            assert r["status"] == S.OK or r["iterations"] > 1


def test_recovers_truth_near_identity(pkg):
    """Where the reference's visual block is the true derivative (R_wc near I) and without outliers, four iterations bring the pose
    from 2 deg / 5 cm off to within 1e-3 rad / 1 cm of the truth, with the IMU residual near zero."""
    for seed in range(8):
        s = pkg.synth.pose_inertial_problem(seed, 300, 0.0, 0.5, 2.0, 0.05, near_identity=True)
        r = S.solve_scene(s)
        assert r["status"] == S.OK and r["iterations"] == 4 and r["num_inliers"] == 300
        assert S.rotation_angle(r["pose"], s["true_pose_wc"]) < 1e-3
        assert np.linalg.norm(r["pose"][4:] - s["true_pose_wc"][4:]) < 1e-2
        res = S.imu_residual(s["prev_kf_pose_wc"], s["prev_kf_velocity"], r["pose"], r["velocity"], s["preint"])
        assert np.abs(res).max() < 1e-2


def test_synthetic_scene_margins(pkg):
    s = pkg.synth.pose_inertial_problem(5, 2000, 0.4, 0.5, 2.0, 0.05)
    e0, e1 = S.reprojection_errors(s["camera"], s["true_pose_wc"], s["points3d"], s["points2d"].astype(np.float64))
    err = np.hypot(e0, e1)
    assert err[s["inliers"]].max() <= 2.01 and err[~s["inliers"]].min() >= 29.9
    assert s["is_stereo"].sum() == 1000 and (s["bias"] != 0).all()
    assert S.rotation_angle(s["pose_wc"], s["true_pose_wc"]) == pytest.approx(np.deg2rad(2.0), rel=1e-9)


def test_cpp_pose_inertial_mirror_compiles_and_links(pkg, tmp_path):
    pkg.load_library()
    assert os.path.exists(build_pose_inertial_driver(str(tmp_path)))
