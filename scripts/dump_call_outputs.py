#!/usr/bin/env python3
"""Run every entry point whose kernels use the shared workgroup primitives (csrc/block_dev.hpp, ransac_dev.hpp, the SE3 helpers of
pose_dev.hpp) once, on scenes of the tests' own scene modules, and write every output array as .npy into a directory.  Two builds
compute the same bytes iff scripts/compare_dumps.py reports their directories all equal.   usage: dump_call_outputs.py <out dir>
The scenes and helpers are those of the tree the script lives in, so a copy of this file inside another checkout dumps that build
(or ORBX_LIBRARY names the other build's library).  Stereo matching runs in its three-launch form unless ORBX_SM_LDS is set: a
second run with ORBX_SM_LDS=1 into another directory dumps the one-launch form.  Only specified outputs are written: rows behind a
count, and the order inside a counting sort's bucket, are nobody's."""
import dataclasses
import os
import sys

os.environ.setdefault("ORBX_SM_LDS", "0")    # stereo matching in its three-launch form (stereo_bucket / stereo_match / stereo_compact_kernel)

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


def scans(pkg, h, cam, M, tm):
    """the entry points whose kernels scan counts or counters (BlockScan, block_counter_scan)"""
    import torch
    import ba_collect_spec  # noqa: F401  (test_ba_collect_gpu's)
    import block_primitive_scenes as B
    import camera_cases as CC
    import camera_scenes as CS
    import covisibility_scenes as V
    import test_ba_collect_gpu as tbc
    import test_covisibility_gpu as tcv

    def local(w, refs, n_best, frames):
        r = tm._np(pkg, h.map_track_local_device(cam, w.mp, w.kfs, refs, n_best, cfg=pkg.TrackConfig.for_mode(1), **tm._frame_tensors(frames)))
        n, N = int(r["list_offsets"][-1]), int(r["offsets"][-1])
        out = {k: r[k] for k in ("list_offsets", "local_kf", "offsets", "poses", "results", "pnp_results")}
        out.update({k: r[k][:n] for k in ("list_slot", "positions", "mp_desc")})
        out.update({k: r[k][:N] for k in ("mp_idx", "feat_idx", "points3d", "points2d", "inlier", "err")})
        out.update({"%s.%d" % (k, b): r[k][b, :len(f[0])] for k in ("matched", "matched_slot") for b, f in enumerate(frames)})
        return out

    # selection, covisibility and the BA window on covisibility_scenes' worlds; local-map tracking on its tracking world
    rows = M.random_rows(6)
    for n_kfs in (11, 65, 257):
        tables, counts, live = V.world(20 + n_kfs, n_kfs)
        w, xy = tbc._world(h, pkg, rows, tables, counts, live, 20 + n_kfs)
        try:
            dump("select.%d" % n_kfs, tm._select(h, w.mp, keyframes=[[k for k, t in zip(w.kfs, tables) if t is not None], w.kfs[:3], w.kfs]))
            dump("covis.%d" % n_kfs, tcv._cov(h, w.mp, w.kfs, tcv._queries(n_kfs), 20))
            for cur in (0, n_kfs // 2):
                r = tbc._collect(h, pkg, w.mp, w.kfs, cur, 20); r.pop("raw")
                dump("ba_window.%d.%d" % (n_kfs, cur), r)
        finally:
            w.close()
    w, store, tables, cases = tcv._tracking(h, pkg)
    try:
        dump("map_local", local(w, [r for _, r in cases], 2, [f for f, _ in cases]))
    finally:
        w.close()
    # ... and past one round of the scans: segments, observers
    rng = np.random.default_rng(3)
    pos, desc = rng.uniform(-5.0, 5.0, (B.TINY_CAPACITY, 3)), rng.integers(0, 256, (B.TINY_CAPACITY, 32), dtype=np.uint8)
    for n_kfs, n_best, refs in B.COV_SEG_CASES:
        tables, counts, live = B.tiny_world(n_kfs)
        w = tm._World(h, pkg, pos, desc, live, capacity=B.TINY_CAPACITY)
        try:
            for t, n in zip(tables, counts):
                w.keyframe(t, n=n)
            dump("map_local.tiny.%d.%d" % (n_kfs, n_best), local(w, refs, n_best, [B.tiny_frame()] * len(refs)))
        finally:
            w.close()
    for n_obs, max_cov in B.BA_ORDER_CASES:
        tables, xy, live = B.ba_order_world(n_obs)
        w = tbc._BaWorld(h, pkg, pos, desc, live, capacity=B.TINY_CAPACITY)
        try:
            for t, p in zip(tables, xy):
                w.keyframe(t, p)
            r = tbc._collect(h, pkg, w.mp, w.kfs, 0, max_cov); r.pop("raw")
            dump("ba_window.tiny.%d" % n_obs, r)
        finally:
            w.close()
    # batch extraction and stereo matching (ORBX_SM_LDS chooses the form), and the matcher alone on the edge buckets
    pairs = np.stack([np.stack(pkg.synth.stereo_pair(5, f)) for f in range(4)])
    o = h.alloc_batch_outputs(4, 2000 + 64)
    h.process_stereo_batch_device(torch.from_numpy(pairs).cuda(), o)
    h.synchronize()
    for b in range(4):
        dump("stereo_batch.%d" % b, h.unpack_batch_outputs(o, b))
    for name, rows_ in (("edges", B.STEREO_ROWS), ("one", B.STEREO_ONE)):
        dump("stereo_rows.%s" % name, h.stereo_match(*B.stereo_rows(rows_)))
    # guided_match and search_for_triangulation[_bow]
    kp, d, kq, dq = pkg.synth.matcher_features(200, 2000, 1500, pkg.KEYPOINT)
    uv = np.stack([kq["x"].astype(np.float64) + 3.0, kq["y"].astype(np.float64) - 2.0], 1)
    for mode in (0, 1):
        dump("guided.m%d" % mode, h.guided_match(kp, d, 752.0, 480.0, uv, dq, 15.0, mode))
        for name, cells in (("edges", B.GUIDED_CELLS), ("one", B.GUIDED_ONE)):
            g = B.guided_cells(cells)
            dump("guided.%s.m%d" % (name, mode), h.guided_match(g[0], g[1], 752.0, 480.0, g[2], g[3], 15.0, mode))
    args = lambda s: (s["kp1"], s["desc1"], s["mp1"], s["stereo1"], s["kp2"], s["desc2"], s["mp2"], s["pose1_wc"], s["pose2_wc"])
    for name in ("euroc", "grid63", "grid64", "big"):
        s = CS.two_view(CC.BY_NAME[name])
        dump("tri_search.%s" % name, h.search_for_triangulation(pkg.CameraModel(**s["camera"]), *args(s), 50))
        n = CS.with_nodes(s)
        dump("tri_search_bow.%s" % name, h.search_for_triangulation_bow(pkg.CameraModel(**s["camera"]), n["kp1"], n["desc1"], n["mp1"], n["stereo1"], n["node1"], n["kp2"],
                                                                         n["desc2"], n["mp2"], n["node2"], n["pose1_wc"], n["pose2_wc"], 50))
    for name, cells in (("edges", B.TRI_CELLS), ("one", B.TRI_ONE)):
        s = B.tri_cells(cells)
        dump("tri_search.cells_%s" % name, h.search_for_triangulation(pkg.CameraModel(**s["camera"]), *args(s), 50))
    # local BA: point counts around one and two rounds of the prep scans, and the project's 20 / 2000 window
    for seed, K, Mp in ((810, 4, 1023), (810, 4, 1024), (810, 4, 1025), (810, 4, 2049), (42, 20, 2000)):
        bw = pkg.synth.ba_window(seed, K, Mp, pkg.BA_OBS)
        bc = pkg.CameraModel(**bw["camera"])
        r = h.ba_solve_visual(bc, pkg.LocalBAConfigLM(), bw["poses_cw"], bw["fixed_cw"], bw["points"], bw["obs"])
        dump("ba.%d.%d" % (K, Mp), {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in r.items()})
        dump("ba_blocks.%d.%d" % (K, Mp), h.debug_ba_blocks(bc, pkg.LocalBAConfigLM(), bw["poses_cw"], bw["fixed_cw"], bw["points"], bw["obs"]))


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
        scans(pkg, h, cam, M, tm)
    finally:
        h.close()
    print("%d arrays written to %s" % (n_files, OUT))


if __name__ == "__main__":
    main()
