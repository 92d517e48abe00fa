#!/usr/bin/env python3
"""Host time per call of the single-problem host forms (the matchers, the triangulation and fuse searches, the pair loop, the BoW
calls, the orbx_keyframe_* searches) and of orbx_fuse_search_device, each with its synchronisation, as api.py calls them.

Two sizes: typical (2000 features a keyframe, 10 neighbours, 500 map points or queries) and small (100 features, 10 neighbours, 100
points).  The forms alternate, --rounds rounds of --steps calls each; per form the median over the rounds and the spread (min, max)
of the per-call time.  The row "control_numpy" is a numpy-only workload (a sort and a copy) timed the same way: it moves with the
box, not with the library.

Two builds are compared by running the script in alternating processes, ORBX_LIBRARY naming the other build's library, and merging
the outputs: --combine parent=a1.json,a2.json,... head=b1.json,b2.json,... takes every process's median and prints, per row and
build, the median [min, max] over the processes.
usage: python scripts/host_forms_rate.py [--rounds R] [--steps S] [--out FILE.json]
       python scripts/host_forms_rate.py --combine LABEL=FILE,FILE,... [LABEL=...] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RADIUS_SCALE = 3.0 * (1.2 * (1.2 * 1.2) * ((1.2 * 1.2) * (1.2 * 1.2)))
SIZES = dict(typical=dict(features=2000, neighbours=10, points=500), small=dict(features=100, neighbours=10, points=100))


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def combine(groups, out):
    rows = {}
    for g in groups:
        label, files = g.split("=", 1)
        for f in files.split(","):
            with open(f) as fh:
                for name, r in json.load(fh)["rows"].items():
                    rows.setdefault(name, {}).setdefault(label, []).append(r["ms"]["median"])
    res = dict(what="host ms per call: median [min, max] over the processes of each build, every process's value its own median",
               processes={k: len(v) for k, v in next(iter(rows.values())).items()},
               rows={name: {label: stat(v) for label, v in by.items()} for name, by in rows.items()})
    for name, by in res["rows"].items():
        print("%-52s %s" % (name, "   ".join("%s %.4f [%.4f, %.4f]" % (k, v["median"], v["min"], v["max"]) for k, v in by.items())))
    if out:
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)


def forms(P, h, cam, size):
    """name -> a callable that makes one call and returns when its results are on the host"""
    import numpy as np
    import torch
    import triangulation_scenes as TS
    n, T, Pn = size["features"], size["neighbours"], size["points"]
    KP = P.KEYPOINT
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kpt = lambda kp: torch.from_numpy(np.ascontiguousarray(kp).view(np.float32).reshape(-1, 7).copy()).cuda()
    rng = np.random.default_rng(5)
    keep = []
    kpL, dL, kpR, dR = P.synth.matcher_features(1, n, n, KP)
    sel = rng.integers(0, n, Pn)
    uv = np.ascontiguousarray(np.stack([kpL["x"][sel], kpL["y"][sel]], 1).astype(np.float64) + rng.normal(0, 3, (Pn, 2)))
    qd = dL[sel].copy()
    voc = P.OrbVocabulary.from_nodes(*P.synth.vocabulary(21, k=10, depth=3), k=10, l=3, handle=h)
    s = P.synth.two_view_features(2, n, KP, dup=0.3)
    node1 = voc.transform_arrays(s["desc1"], 1)[2]; node2 = voc.transform_arrays(s["desc2"], 1)[2]
    sv = (s["kp1"], s["desc1"], s["mp1"], s["stereo1"], s["kp2"], s["desc2"], s["mp2"], s["pose1_wc"], s["pose2_wc"])
    sb = (s["kp1"], s["desc1"], s["mp1"], s["stereo1"], node1, s["kp2"], s["desc2"], s["mp2"], node2, s["pose1_wc"], s["pose2_wc"])
    f = P.synth.fuse_scene(3, Pn, T, n, KP)
    fd = (d(f["positions"]), d(f["mp_desc"]), np.ascontiguousarray(f["kf_poses_wc"], np.float64), d(f["kf_feat_offset"]), kpt(f["kps"]), d(f["descs"]))
    # the scene's generator keeps about 85 % of its points per keyframe: n features are n / 1.15 points and 15 % distractors
    sc = TS.make_scene(4, n_points=int(n / 1.15), T=T, n_distract=int(0.15 * n), nodes="all")

    def keyframe(kf):
        t = (kpt(kf["kp"]), d(kf["desc"]), d(kf["pts"]), d(kf["has"]))
        keep.append(t)
        k = P.KeyFrame(h, t[0], t[1], len(kf["kp"]), t[2], t[3], pose_wc=kf["pose"])
        k.set_map_points([7 if m else None for m in kf["mp"]])
        k.set_feature_nodes(kf["node"])
        return k

    cur = keyframe(sc["current"]); nbs = [keyframe(k) for k in sc["neighbours"]]
    off = f["kf_feat_offset"]
    fkfs = []
    for t in range(T):
        tt = (kpt(f["kps"][off[t]:off[t + 1]]), d(f["descs"][off[t]:off[t + 1]]))
        keep.append(tt)
        fkfs.append(P.KeyFrame(h, tt[0], tt[1], int(off[t + 1] - off[t]), pose_wc=f["kf_poses_wc"][t]))
    k1, k2 = sc["current"], sc["neighbours"][0]
    pairs = np.ascontiguousarray(sc["gt"][0], np.int32)
    tcam = P.CameraModel(**TS.CAMERA)
    h.synchronize()

    def fuse_device():
        h.fuse_search_device(cam, *fd, RADIUS_SCALE)
        h.synchronize()

    calls = {
        "stereo_match": lambda: h.stereo_match(kpL, dL, kpR, dR),
        "hamming_match_crosscheck": lambda: h.hamming_match_crosscheck(dL, dR),
        "hamming_batch": lambda: h.hamming_batch(dL, dR),
        "guided_match": lambda: h.guided_match(kpL, dL, 752.0, 480.0, uv, qd, 40.0, 1),
        "search_for_triangulation": lambda: h.search_for_triangulation(cam, *sv),
        "search_for_triangulation_bow": lambda: h.search_for_triangulation_bow(cam, *sb),
        "fuse_search": lambda: h.fuse_search(cam, f["positions"], f["mp_desc"], f["kf_poses_wc"], off, f["kps"], f["descs"], RADIUS_SCALE),
        "fuse_search_device": fuse_device,
        "triangulate_pairs": lambda: h.triangulate_pairs(tcam, k1["kp"], k1["pts"], k1["has"], k1["pose"], k2["kp"], k2["pts"], k2["has"], k2["pose"], pairs),
        "bow_transform": lambda: voc.transform_arrays(dL, 1),
        "bow_vectors": lambda: voc.vectors_arrays(dL, 1),
        "keyframe_guided_match": lambda: cur.guided_match(752.0, 480.0, uv, qd, 40.0, 1),
        "keyframe_search_for_triangulation": lambda: cur.search_for_triangulation(tcam, nbs[0]),
        "keyframe_fuse_search": lambda: P.KeyFrame.fuse_search(h, cam, f["positions"], f["mp_desc"], fkfs, RADIUS_SCALE),
        "keyframe_triangulate_from_neighbors": lambda: cur.triangulate_from_neighbors(tcam, nbs, cap=4 * n),
    }
    return calls, (keep, voc, cur, nbs, fkfs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs="+", default=None)
    a = ap.parse_args()
    if a.combine:
        combine(a.combine, a.out)
        return
    import numpy as np
    import torch
    import orb_slam3_rust_amd as P
    cam = P.CameraModel(**P.synth.EUROC_CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    calls, alive = {}, []
    for label, size in SIZES.items():
        c, keep = forms(P, h, cam, size)
        calls.update({"%s/%s" % (k, label): v for k, v in c.items()})
        alive.append(keep)
    ctl = np.random.default_rng(9).random(60000)

    def control():
        np.sort(ctl).copy()

    calls["control_numpy"] = control
    for fn in calls.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            times[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    res = dict(gpu=torch.cuda.get_device_name(0), library=os.environ.get("ORBX_LIBRARY", "liborbx_hip.so"), rounds=a.rounds, steps_per_round=a.steps, sizes=SIZES,
               rows={k: dict(ms=stat(t)) for k, t in times.items()})
    print(json.dumps({k: round(r["ms"]["median"], 4) for k, r in res["rows"].items()}))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    h.synchronize()


if __name__ == "__main__":
    main()
