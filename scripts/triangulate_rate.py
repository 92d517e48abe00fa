#!/usr/bin/env python3
"""Host time of KeyFrame.triangulate_from_neighbors (one call: T batched searches + the pair loop + the ordered compaction, one
download) against the search part alone done the way a caller had to before: T sequential KeyFrame.search_for_triangulation calls
(each its own launches, synchronisation and download of pairs; the triangulation would still have to follow on the host).
Both forms search the same neighbours: those the baseline test keeps.
T = 10 neighbours, about 2000 features per keyframe, device-resident keyframes (tests/triangulation_scenes.py).  Both forms are
timed in the same process in alternating rounds; per form the median over the rounds and the spread (min, max) are reported, plus
the device time per kernel of the fused call.
usage: python scripts/triangulate_rate.py [--rounds R] [--steps K] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import orb_slam3_rust_amd as P  # noqa: E402
import triangulation_scenes as G  # noqa: E402


def keyframe(h, kf, kid):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    k = P.KeyFrame(h, d(np.ascontiguousarray(kf["kp"]).view(np.float32).reshape(-1, 7).copy()), d(kf["desc"]), len(kf["kp"]), d(kf["pts"]), d(kf["has"]),
                   keyframe_id=kid, pose_wc=kf["pose"])
    k.set_map_points([7 if m else None for m in kf["mp"]])
    if kf.get("node") is not None:
        k.set_feature_nodes(kf["node"])
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("triangulate_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**G.CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    out = dict(gpu=torch.cuda.get_device_name(0), neighbours=a.neighbours, rounds=a.rounds, steps_per_round=a.steps, rows=[])
    for nodes in ("none", "all"):
        sc = G.make_scene(21, n_points=1700, T=a.neighbours, n_distract=300, nodes=nodes)
        cur = keyframe(h, sc["current"], 1)
        nbs = [keyframe(h, nb, 10 + t) for t, nb in enumerate(sc["neighbours"])]
        fused = lambda: cur.triangulate_from_neighbors(cam, nbs, cap=8192)
        # the same work for both forms: the sequential caller makes the baseline test (:137-141) itself and searches only the
        # neighbours the fused call searches
        far = [k for k, nb in zip(nbs, sc["neighbours"]) if np.linalg.norm(nb["pose"][4:] - sc["current"]["pose"][4:]) >= cam.baseline]
        seq = lambda: [cur.search_for_triangulation(cam, k, 50) for k in far]
        for _ in range(a.warmup):
            r = fused(); s = seq()
        t_f, t_s = [], []
        for _ in range(a.rounds):                                    # alternating rounds: drift hits both forms alike
            for f, acc in ((fused, t_f), (seq, t_s)):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    f()
                acc.append((time.perf_counter() - t0) / a.steps * 1e3)
        h.set_profiling(True)
        h.kernel_times()                                             # start a fresh accumulation window
        for _ in range(a.steps):
            fused()
        kt = {k: v[0] / a.steps * 1e3 for k, v in h.kernel_times().items()}
        h.set_profiling(False)
        row = dict(feature_vector_search=(nodes == "all"), features_current=len(sc["current"]["kp"]),
                   features_per_neighbour=[len(nb["kp"]) for nb in sc["neighbours"]], neighbours_searched=len(far), matches_found=r[4].num_matches_found,
                   new_points=r[4].num_new_points, pairs_of_sequential_searches=int(sum(len(p) for p in s)),
                   fused_call_ms=dict(median=statistics.median(t_f), min=min(t_f), max=max(t_f)),
                   sequential_searches_ms=dict(median=statistics.median(t_s), min=min(t_s), max=max(t_s)),
                   note=("the sequential form here is the grid search: the parent has no FeatureVector search on device-resident keyframes"
                         if nodes == "all" else "both forms run the grid search"))
        row["fused_over_sequential"] = row["fused_call_ms"]["median"] / row["sequential_searches_ms"]["median"]
        if kt:
            row["fused_kernel_us_per_call"] = kt
        out["rows"].append(row)
        print(json.dumps(row))
        cur.close()
        for k in nbs:
            k.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "triangulate_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
