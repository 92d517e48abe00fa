#!/usr/bin/env python3
"""Pose-inertial optimization rates (orbx_pose_inertial_batch_device / orbx_pose_inertial_optimize): problems/s and per-kernel device
time after warm-up, for
  - 512 problems x n in {300, 1000, 2000} (20 % outliers, half stereo, R_wc near the identity, where a problem runs all its
    iterations: with EuRoC-like orientations most end early, the reference's Jacobian being right only near R_wc = I),
    device-resident: call time from HIP events around the calls on the library's stream, kernel time from the library's own
    per-launch HIP events, and
  - one problem with n = 1000 through the host entry point, host copies included (the tracker's call shape): wall time per call and
    the kernel's HIP-event time.
With the algorithmic f64 operation count per problem from the shapes and the fraction of the 78.6 TFLOP/s f64 vector peak.
usage: python scripts/pose_inertial_rate.py [--steps K] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import orb_slam3_rust_amd as P  # noqa: E402

PEAK_F64 = 78.6e12
# f64 operations per unit of work, counted from the kernel's expressions (pose_inertial_kernels.hip)
OPS_XFORM = 30                              # nalgebra quaternion * vector + translation
OPS_VISUAL = OPS_XFORM + 38 + 21 * 4 + 6 * 4 + 1   # residual and 2x6 block, H upper triangle, rhs, count
OPS_RECLASS = OPS_XFORM + 12
OPS_IMU = 16 * 150                          # 16 residual evaluations (two quaternion products, scaled axis, two rotations)
OPS_SYSTEM = 15 * 15 * 9 * 2 + 15 * 9 * 2 + 15 * 15 * 15 * 2 // 3 + 15 * 15 * 2   # IMU J^T J and J^T r, LU, solves


def flops_per_problem(n, active_sum, iterations):
    return active_sum * OPS_VISUAL + iterations * (n * OPS_RECLASS + OPS_IMU + OPS_SYSTEM)


def active_per_iteration(s, cfg):
    """the specification's masked-in counts, summed over the iterations run (the visual rows the kernel accumulated)"""
    tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    sys.path.insert(0, tests)
    import pose_inertial_spec as S
    calls = []
    orig = S.visual_rows

    def counting(cam, pose, X, uv):
        calls.append(len(X))
        return orig(cam, pose, X, uv)
    S.visual_rows = counting
    try:
        S.solve_scene(s, cfg.__dict__)
    finally:
        S.visual_rows = orig
    return sum(calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cam = P.CameraModel(**P.synth.EUROC_CAMERA)
    h = P.Handle(cam, 100)
    cfg = P.PoseInertialConfig()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(h.stream, device=dev)
    out = dict(gpu=torch.cuda.get_device_name(0), config=cfg.__dict__, batch=[], single=None, peak_f64_tflops=PEAK_F64 / 1e12)
    for n in (300, 1000, 2000):
        NP = 512
        scenes = [P.synth.pose_inertial_problem(60_000 + 10 * i + n, n, 0.2, 0.5, 2.0, 0.05, near_identity=True) for i in range(NP)]
        off = torch.tensor(np.arange(NP + 1) * n, dtype=torch.int32, device=dev)
        t = [off] + [torch.from_numpy(np.ascontiguousarray(np.concatenate([s[k] for s in scenes]), dt)).to(dev)
                     for k, dt in (("points3d", np.float64), ("points2d", np.float32), ("is_stereo", np.uint8))]
        t += [torch.from_numpy(np.ascontiguousarray(np.stack([s[k] for s in scenes]), np.float64)).to(dev)
              for k in ("pose_wc", "velocity", "bias", "prev_kf_pose_wc", "prev_kf_velocity", "preint")]
        for _ in range(a.warmup):
            r = h.pose_inertial_optimization_batch_device(cam, *t, cfg=cfg)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.steps):
            r = h.pose_inertial_optimization_batch_device(cam, *t, cfg=cfg)
        e1.record(stream)
        torch.cuda.synchronize()
        call_ms = e0.elapsed_time(e1) / a.steps
        h.set_profiling(True); h.kernel_times()
        for _ in range(a.steps):
            h.pose_inertial_optimization_batch_device(cam, *t, cfg=cfg)
        kt = h.kernel_times(); h.set_profiling(False)
        res = r[4].cpu().numpy().view(P.POSE_INERTIAL_RESULT).reshape(-1)
        sample = range(0, NP, 64)
        fl = [flops_per_problem(n, active_per_iteration(scenes[i], cfg), int(res[i]["iterations"])) for i in sample]
        kern = {k: v[0] / a.steps * 1e3 for k, v in kt.items()}      # us per call
        dev_us = sum(kern.values())
        tot = float(np.mean(fl)) * NP
        row = dict(problems=NP, n=n, outliers=0.2, stereo=0.5, call_ms_hip_events=call_ms, problems_per_s=NP / (call_ms * 1e-3),
                   kernel_us_per_call=kern, device_us_per_call=dev_us, mean_iterations=float(res["iterations"].mean()),
                   statuses={str(k): int((res["status"] == k).sum()) for k in np.unique(res["status"])},
                   flops_per_problem_sampled=float(np.mean(fl)), tflops_device=tot / (dev_us * 1e-6) / 1e12,
                   fraction_of_f64_peak=tot / (dev_us * 1e-6) / PEAK_F64)
        out["batch"].append(row)
        print(json.dumps(row), flush=True)
    # one problem, n = 1000, through the host entry point (upload, one launch, download, synchronise)
    s = P.synth.pose_inertial_problem(77, 1000, 0.2, 0.5, 2.0, 0.05, near_identity=True)
    pa = (s["pose_wc"], s["velocity"], s["bias"], s["prev_kf_pose_wc"], s["prev_kf_velocity"], s["preint"], s["points3d"], s["points2d"],
          s["is_stereo"])
    for _ in range(a.warmup):
        g = h.pose_inertial_optimization(cam, *pa, cfg=cfg)
    reps = a.steps * 10
    t0 = time.perf_counter()
    for _ in range(reps):
        g = h.pose_inertial_optimization(cam, *pa, cfg=cfg)
    wall = (time.perf_counter() - t0) / reps
    h.set_profiling(True); h.kernel_times()
    for _ in range(reps):
        h.pose_inertial_optimization(cam, *pa, cfg=cfg)
    kt = h.kernel_times(); h.set_profiling(False)
    kern = {k: v[0] / reps * 1e3 for k, v in kt.items()}
    f = flops_per_problem(1000, active_per_iteration(s, cfg), g.iterations)
    out["single"] = dict(n=1000, outliers=0.2, stereo=0.5, wall_us_per_call=wall * 1e6, calls_per_s=1.0 / wall, kernel_us_per_call=kern,
                         device_us_per_call=sum(kern.values()), iterations=g.iterations, status=g.status, num_inliers=g.num_inliers,
                         flops=f, fraction_of_f64_peak=f / (sum(kern.values()) * 1e-6) / PEAK_F64)
    print(json.dumps(out["single"]), flush=True)
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
