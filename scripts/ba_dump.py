#!/usr/bin/env python3
"""Solve a fixed list of bundle-adjustment cases — one per path of ba_solve_batch — and write every result (poses, points, velocities and
biases, iterations and errors) as .npy files, so that two builds of the library can be compared bit for bit:
    ORBX_LIBRARY=<build A> python scripts/ba_dump.py dumps/a  &&  ORBX_LIBRARY=<build B> python scripts/ba_dump.py dumps/b
    python scripts/compare_dumps.py dumps/a dumps/b
The 18-window batch runs as two halves on two streams, or on one with ORBX_BA_NO_SPLIT=1 (read once per process): its files are named
after the mode, so a second run with the switch set, into the same folder, adds the other set."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import orb_slam3_rust_amd as P

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
cam = P.CameraModel(**P.synth.EUROC_CAMERA)
h = P.Handle(cam, 100)
cfg = P.LocalBAConfigLM()


def save(name, results):
    for i, r in enumerate(results if isinstance(results, list) else [results]):
        if r is None:
            np.save(os.path.join(out, "%s_%02d_none.npy" % (name, i)), np.zeros(0))
            continue
        for key in ("poses_wc", "points", "velocities", "biases"):
            if key in r:
                np.save(os.path.join(out, "%s_%02d_%s.npy" % (name, i, key)), np.asarray(r[key]))
        np.save(os.path.join(out, "%s_%02d_stats.npy" % (name, i)), np.array([r["iterations"], r["initial_error"], r["final_error"]]))


def windows(seed, shapes, n, fixed=None):
    return [P.synth.ba_window(seed + i, *shapes[i % len(shapes)], P.BA_OBS, n_fixed_extra=fixed[i % len(fixed)] if fixed else 0) for i in range(n)]


# single window (BASELINE configs[2]), in the 32-byte and in the 16-byte form of the observations
w = P.synth.keypoint_precision(P.synth.ba_window(42, 20, 2000, P.BA_OBS))
save("single", h.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], w["obs"]))
save("single32", h.ba_solve_visual(cam, cfg, w["poses_cw"], w["fixed_cw"], w["points"], P.ba_obs_to_obs32(w["obs"], len(w["fixed_cw"]))))
# 7 windows: the fused step; 9: the two kernels, 16 lanes per point; reduced systems of every solve path among them
save("batch7", h.ba_solve_visual_batch(cam, cfg, windows(800, [(5, 80), (20, 600), (26, 350), (33, 400), (56, 500), (12, 300), (3, 40)], 7)))
save("batch9", h.ba_solve_visual_batch(cam, cfg, windows(900, [(40, 300), (70, 200), (50, 400), (12, 500), (24, 350), (33, 260), (18, 640), (66, 120), (5, 80)], 9)))
# 18 windows of mixed shapes, one the reference answers None for: two streams, or one
wins = windows(700, [(5, 90), (12, 400), (20, 900), (3, 40), (8, 250), (25, 600)], 18, fixed=[0, 1, 0, 0, 2, 0])
wins[13] = dict(wins[13], obs=wins[13]["obs"][:0])
save("batch18_nosplit" if os.environ.get("ORBX_BA_NO_SPLIT") is not None else "batch18_split", h.ba_solve_visual_batch(cam, cfg, wins))
# global BA: one fixed keyframe
g = P.synth.ba_window(2177, 7, 300, P.BA_OBS)
save("global", h.ba_solve_global(cam, cfg, g["poses_cw"], g["fixed_cw"][0], g["points"], g["obs"]))
# inertial: the 15-d system in LDS tiles (K = 5), factored in one launch (13), one launch per panel (22)
for seed, K, M in ((2, 5, 150), (11, 13, 300), (12, 22, 400)):
    w = P.synth.inertial_window(seed, K, M, P.BA_OBS, n_fixed=1)
    save("inertial%02d" % K, h.ba_solve_inertial(P.CameraModel(**w["camera"]), P.LocalInertialBAConfig(), w["poses_wc"], w["velocities"], w["biases"],
                                                  w["fixed_cw"], w["points"], w["obs"], w["edge_kf"], w["preint"]))
print("%d files in %s" % (len(os.listdir(out)), out))
