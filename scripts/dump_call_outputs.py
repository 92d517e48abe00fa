#!/usr/bin/env python3
"""Run every entry point whose kernels use the shared workgroup primitives (csrc/block_dev.hpp, ransac_dev.hpp, the SE3 helpers of
pose_dev.hpp) once, on scenes of the tests' own scene modules, and write every output array as .npy into a directory.  Two builds
compute the same bytes iff scripts/compare_dumps.py reports their directories all equal.   usage: dump_call_outputs.py <out dir>
The scenes and helpers are those of the tree the script lives in, so a copy of this file inside another checkout dumps that build."""
import dataclasses
import os
import sys

os.environ["ORBX_SM_LDS"] = "0"          # stereo matching in its three-launch form (stereo_bucket / stereo_match / stereo_compact_kernel)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = sys.argv[1]
os.makedirs(OUT, exist_ok=True)
n_files = 0


def dump(name, o):
    """arrays, tensors and scalars as .npy; dicts, lists, tuples and dataclasses field by field"""
    global n_files
    import torch
    if isinstance(o, torch.Tensor):
        torch.cuda.synchronize()
        o = o.cpu().numpy()
    if dataclasses.is_dataclass(o):
        o = {f.name: getattr(o, f.name) for f in dataclasses.fields(o)}
    if isinstance(o, dict):
        for k in sorted(o, key=str):
            dump("%s.%s" % (name, k), o[k])
    elif isinstance(o, (list, tuple)) and not all(isinstance(x, (int, float)) for x in o):
        for i, x in enumerate(o):
            dump("%s.%d" % (name, i), x)
    elif o is None:
        return
    else:
        a = np.ascontiguousarray(np.atleast_1d(np.asarray(o)))
        assert a.dtype != object, name
        if a.dtype.names:                                                  # records as bytes: compare_dumps.py compares with array_equal
            a = a.view(np.uint8)
        elif a.dtype.kind == "f":                                          # likewise floats, so that a NaN equals itself
            a = a.view("u%d" % a.dtype.itemsize)
        np.save(os.path.join(OUT, name + ".npy"), a)
        n_files += 1


def main():
    import orb_slam3_rust_amd as pkg
    import loop_verify_scenes as Z
    import map_store_scenes as M
    import track_reference_scenes as R
    import tracking_scenes as G
    import triangulation_scenes as TS
    import test_map_store_gpu as tm
    import test_pose_inertial_gpu as tpi
    import test_track_reference_gpu as tr
    import test_tracking_gpu as tt
    import test_triangulation_gpu as ttri
    cam = pkg.CameraModel(**G.CAMERA)
    h = pkg.Handle(pkg.CameraModel(**pkg.synth.EUROC_CAMERA), 2000, device=0, max_w=1920, max_h=1080, max_batch=8)
    try:
        # tracking against the local map: both modes, round edges among the sizes (b3: 90, 257, 33 map points)
        for name in ("b1", "b3", "middle_without_map_points", "no_model_next_to_good"):
            for mode in (0, 1):
                dump("track.%s.m%d" % (name, mode), tt._run_device(h, pkg, cam, G.batches()[name], mode))
        # tracking against the reference keyframe
        for name in ("block_edges_keyframe", "realistic", "ties", "b3_shared_keyframe", "valid_all_zero"):
            dump("tref.%s" % name, tr._run_device(h, pkg, cam, R.batches()[name]))
        # tracking on the resident map-point store
        store, scs, frames_kf = M.shared_batch()
        w = tm._World(h, pkg, store.positions, store.desc, store.live)
        try:
            kf = [[w.keyframe(t) for t in sc["tables"]] for sc in scs]
            frames = [scs[0]["frame"], scs[1]["frame"], scs[0]["frame"]]
            kfs = [[kf[s][k] for s, k in fk] for fk in frames_kf]
            for mode in (0, 1):
                dump("map_track.m%d" % mode, tm._np(pkg, h.map_track_frames_device(cam, w.mp, keyframes=kfs, cfg=pkg.TrackConfig.for_mode(mode),
                                                                                  **tm._frame_tensors(frames))))
        finally:
            w.close()
        # loop verification (every scene under its own configuration) and Sim3 on its own
        for name in sorted(Z.PAIRS):
            cfg = pkg.LoopVerifyConfig(**dict(Z.PAIRS[name][1] or {}, sim3=pkg.Sim3SolverConfig(**(Z.PAIRS[name][2] or {}))))
            r = h.verify_loop_candidates(cam, [Z.pair(name)], cfg)[0]
            dump("loop.%s" % name, {k: r[k] for k in ("status", "matches", "feature_matches", "pts_current", "pts_loop", "inlier", "sim3", "record")})
        for name in sorted(Z.SIM3_SETS):
            dump("sim3.%s" % name, h.compute_sim3_ransac_batch([Z.sim3_set(name)[:2]], pkg.Sim3SolverConfig(**Z.SIM3_SETS[name][1])))
        # PnP and pose-inertial batches
        probs = []
        for i, n in enumerate([0, 3, 4, 5, 6, 12, 50, 255, 256, 257, 300, 1000] * 4):
            s = pkg.synth.pnp_problem(1000 + i, n, (0.0, 0.3, 0.6, 1.0)[i % 4], prior_rot_deg=10.0, prior_trans_m=0.3)
            probs.append((s["points3d"], s["points2d"], s["prior_wc"]))
        for i, r in enumerate(h.solve_pnp_ransac_batch(cam, probs)):
            dump("pnp.%02d" % i, dict(pose=r.pose, inlier=r.inlier_mask, err=r.reproj_errors, stats=[r.stats[k] for k in pkg.PNP_RESULT.names]))
        for i, r in enumerate(h.pose_inertial_optimization_batch(cam, [tpi.args(s) for s in tpi._mixed(pkg, 48)])):
            dump("pose_inertial.%02d" % i, dict(pose=r.pose, velocity=r.velocity, bias=r.bias, inlier=r.inlier_mask,
                                                counts=[r.num_inliers, r.num_observations, r.iterations, r.status]))
        # triangulation from neighbour keyframes
        for name in ("t3_nodes", "t10_grid"):
            sc = TS.fused_scene(name)
            cur = ttri._keyframe(pkg, h, sc["current"], 1)
            nbs = [ttri._keyframe(pkg, h, k, 10 + t) for t, k in enumerate(sc["neighbours"])]
            for inertial in (0, 1):
                nb, i1, i2, pts, res = cur.triangulate_from_neighbors(pkg.CameraModel(**sc["camera"]), nbs, is_inertial=inertial)
                dump("tri.%s.i%d" % (name, inertial), dict(nb=nb, i1=i1, i2=i2, pts=pts, per_neighbour=res.per_neighbour))
            h.synchronize()
            cur.close()
            for k in nbs:
                k.close()
        # the cross-check matcher and a one-pair stereo match (the three-launch path)
        rng = np.random.default_rng(5)
        for nq, nt in ((257, 2049), (2049, 257), (1000, 1000)):
            t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
            q = np.concatenate([t[rng.integers(0, nt, nq // 2)] ^ rng.integers(0, 2, (nq // 2, 32), dtype=np.uint8), rng.integers(0, 256, (nq - nq // 2, 32), dtype=np.uint8)])
            dump("crosscheck.%dx%d" % (nq, nt), h.hamming_match_crosscheck(q, t))
        for k in range(2):
            left, right = pkg.synth.stereo_pair(5, k)
            dump("stereo.%d" % k, h.process_stereo(left, right))
    finally:
        h.close()
    print("%d arrays written to %s" % (n_files, OUT))


if __name__ == "__main__":
    main()
