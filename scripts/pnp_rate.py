#!/usr/bin/env python3
"""PnP-RANSAC rates (orbx_pnp_ransac_batch_device / orbx_pnp_ransac): problems/s and per-kernel device time after warm-up, for
  - 512 problems x n in {300, 1000, 2000} at 30 % outliers, device-resident (the throughput form), and
  - one problem with n = 1000 through the host entry point, host copies included (the reference's call shape).
With the algorithmic f64 operation count per problem from the shapes and the fraction of the 78.6 TFLOP/s f64 vector peak.
usage: python scripts/pnp_rate.py [--steps K] [--warmup W] [--out FILE.json]"""
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
# f64 operations per unit of work, counted from the kernels' expressions (pnp_kernels.hip)
OPS_XFORM = 18        # R X + t: 9 multiplies, 9 adds
OPS_TEST = 10         # 1/z, x/z, y/z, two multiply-adds and subtractions, the squared norm
OPS_ACCUM = OPS_XFORM + 8 + 28 + 21 * 4 + 6 * 4 + 3    # residual, pose block, H upper triangle, rhs, cost
OPS_COST = OPS_XFORM + 8 + 3
OPS_SOLVE = 6 * 6 * 6 // 3 + 2 * 36 + 60                # 6x6 Cholesky, two triangular solves, Exp + pose update
OPS_DETAIL = 30 + 12                                    # nalgebra rotation + translation, projection, error


def flops_per_problem(n, inliers, H, m, hyp_it, ref_it, ref_done):
    hyp = H * hyp_it * (m * (OPS_ACCUM + OPS_COST) + OPS_SOLVE)
    score = H * n * (OPS_XFORM + OPS_TEST)
    refine = n * (OPS_XFORM + OPS_TEST) + ref_done * (inliers * (OPS_ACCUM + OPS_COST) + OPS_SOLVE)
    return dict(hypotheses=hyp, scoring=score, refine=refine, detailed=n * OPS_DETAIL, total=hyp + score + refine + n * OPS_DETAIL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cam = P.CameraModel(**P.synth.EUROC_CAMERA)
    h = P.Handle(cam, 100)
    cfg = P.PnPConfig()
    dev = torch.device("cuda", 0)
    out = dict(gpu=torch.cuda.get_device_name(0), config=cfg.__dict__, batch=[], single=None, peak_f64_tflops=PEAK_F64 / 1e12)
    for n in (300, 1000, 2000):
        P_ = 512
        probs = [P.synth.pnp_problem(50_000 + 10 * i + n, n, 0.3, 10.0, 0.3) for i in range(P_)]
        off = torch.tensor(np.arange(P_ + 1) * n, dtype=torch.int32, device=dev)
        p3 = torch.from_numpy(np.concatenate([s["points3d"] for s in probs])).to(dev)
        p2 = torch.from_numpy(np.concatenate([s["points2d"] for s in probs])).to(dev)
        pr = torch.from_numpy(np.stack([s["prior_wc"] for s in probs])).to(dev)
        for _ in range(a.warmup):
            r = h.solve_pnp_ransac_batch_device(cam, off, p3, p2, pr, n, cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r = h.solve_pnp_ransac_batch_device(cam, off, p3, p2, pr, n, cfg)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.steps
        h.set_profiling(True); h.kernel_times()
        for _ in range(a.steps):
            h.solve_pnp_ransac_batch_device(cam, off, p3, p2, pr, n, cfg)
        kt = h.kernel_times(); h.set_profiling(False)
        res = r[3].cpu().numpy().view(P.PNP_RESULT).reshape(-1)
        assert (res["status"] == P.PNP_OK).all()
        fl = [flops_per_problem(n, int(x["n_inliers"]), cfg.max_iterations, cfg.model_points, cfg.hypothesis_iterations,
                                cfg.refine_iterations, int(x["refine_iterations"])) for x in res]
        tot = sum(f["total"] for f in fl)
        kern = {k: v[0] / a.steps * 1e3 for k, v in kt.items()}      # us per call
        dev_us = sum(kern.values())
        row = dict(problems=P_, n=n, outliers=0.3, wall_ms_per_call=wall * 1e3, problems_per_s=P_ / wall, kernel_us_per_call=kern,
                   device_us_per_call=dev_us, mean_hypotheses_evaluated=float(res["hypotheses_evaluated"].mean()),
                   mean_refine_iterations=float(res["refine_iterations"].mean()),
                   flops_per_problem={k: float(np.mean([f[k] for f in fl])) for k in fl[0]},
                   tflops_device=tot / (dev_us * 1e-6) / 1e12, fraction_of_f64_peak=tot / (dev_us * 1e-6) / PEAK_F64)
        out["batch"].append(row)
        print(json.dumps(row), flush=True)
    # one problem, n = 1000, through the host entry point (upload, three launches, download, synchronise)
    s = P.synth.pnp_problem(77, 1000, 0.3, 10.0, 0.3)
    for _ in range(a.warmup):
        g = h.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"], cfg)
    reps = a.steps * 10
    t0 = time.perf_counter()
    for _ in range(reps):
        g = h.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"], cfg)
    wall = (time.perf_counter() - t0) / reps
    h.set_profiling(True); h.kernel_times()
    for _ in range(reps):
        h.solve_pnp_ransac_detailed(cam, s["points3d"], s["points2d"], s["prior_wc"], cfg)
    kt = h.kernel_times(); h.set_profiling(False)
    kern = {k: v[0] / reps * 1e3 for k, v in kt.items()}
    f = flops_per_problem(1000, g.stats["n_inliers"], cfg.max_iterations, cfg.model_points, cfg.hypothesis_iterations,
                          cfg.refine_iterations, g.stats["refine_iterations"])
    out["single"] = dict(n=1000, outliers=0.3, wall_us_per_call=wall * 1e6, calls_per_s=1.0 / wall, kernel_us_per_call=kern,
                         device_us_per_call=sum(kern.values()), stats=g.stats, flops=f["total"],
                         fraction_of_f64_peak=f["total"] / (sum(kern.values()) * 1e-6) / PEAK_F64)
    print(json.dumps(out["single"]), flush=True)
    h.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(out, fo, indent=1)


if __name__ == "__main__":
    main()
