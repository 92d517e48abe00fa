#!/usr/bin/env python3
"""Host time of Handle.track_frames_device (one call: grid build, project-and-search, gather, PnP-RANSAC, finish; every array
device-resident, one synchronisation at the end) against the same run's sequence of the calls a tracker had to make before it:
the map points projected on the host (numpy), Handle.guided_match once per frame (upload, two launches, download), the matches
compacted on the host into PnP's layout, Handle.solve_pnp_ransac_batch on all frames.  Both forms do track_local_map's work
(mode 1) on the same frames and arrive at the same poses.
The fused call is timed twice: with the map points, their descriptors and the poses already on the device (what a tracker that keeps
its local map there pays), and with their upload from host arrays inside the timed window (the sequential form's starting point; the
frame's features are on the device in both, where the extractor leaves them).
B = 1 and B = 64 frames, about 2000 features and 1500 map points per frame (tests/tracking_scenes.py).  The forms are timed in
the same process in alternating rounds, each round at least --round-seconds long; per form the median over the rounds and the spread
(min, max) are reported, plus the device time per kernel of the fused call.
usage: python scripts/track_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
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
import tracking_scenes as G  # noqa: E402
import tracking_spec as S  # noqa: E402


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--map-points", type=int, default=1500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**G.CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    cfg = P.TrackConfig.for_mode(P.TRACK_LOCAL_MAP)
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, mode="track_local_map", rows=[])
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for B in (1, 64):
        frames = [G.frame(100 + b, a.map_points, a.features) for b in range(B)]
        fc = np.array([len(f[0]) for f in frames], np.int32)
        mo = np.zeros(B + 1, np.int32); mo[1:] = np.cumsum([len(f[2]) for f in frames])
        dev = dict(kp=d(np.concatenate([f[0] for f in frames]).view(np.float32).reshape(-1, 7).copy()), desc=d(np.concatenate([f[1] for f in frames])),
                   feat_start=d((np.cumsum(fc) - fc).astype(np.int32)), feat_count=d(fc), max_feat=int(fc.max()),
                   positions=d(np.concatenate([f[2] for f in frames])), mp_desc=d(np.concatenate([f[3] for f in frames])), mp_offsets=mo,
                   search_poses_wc=d(np.stack([f[4] for f in frames])), priors_wc=d(np.stack([f[5] for f in frames])))

        def fused():
            o = h.track_frames_device(cam, cfg=cfg, **dev)
            h.synchronize()
            return o

        host = dict(positions=np.concatenate([f[2] for f in frames]), mp_desc=np.concatenate([f[3] for f in frames]),
                    search_poses_wc=np.stack([f[4] for f in frames]), priors_wc=np.stack([f[5] for f in frames]))

        def fused_upload():
            o = h.track_frames_device(cam, cfg=cfg, **dict(dev, **{k: torch.from_numpy(v).cuda() for k, v in host.items()}))
            h.synchronize()
            return o

        def sequential():
            probs = []
            for kp, desc, X, md, sp, pr in frames:
                z, u, v = S.project(G.CAMERA, sp, X)
                ids = np.flatnonzero(~(z <= 0.0))
                idx, _ = h.guided_match(kp, desc, cfg.img_w, cfg.img_h, np.stack([u[ids], v[ids]], 1), md[ids], cfg.radius, cfg.mode)
                hit = idx >= 0
                probs.append((X[ids[hit]], np.stack([kp["x"][idx[hit]], kp["y"][idx[hit]]], 1), pr))
            return h.solve_pnp_ransac_batch(cam, probs)

        forms = (("fused", fused), ("fused_upload", fused_upload), ("sequential", sequential))
        for _ in range(a.warmup):
            o = fused(); fused_upload(); s = sequential()
        poses = o["poses"].cpu().numpy()
        same = all(poses[b].tobytes() == s[b].pose.tobytes() for b in range(B))
        steps, times = {}, {k: [] for k, _ in forms}
        for k, f in forms:                                           # calls per round: enough to fill round_seconds
            t0 = time.perf_counter(); f(); f(); one = (time.perf_counter() - t0) / 2
            steps[k] = max(10, int(np.ceil(a.round_seconds / one)))
        for _ in range(a.rounds):                                    # alternating rounds: drift hits every form alike
            for k, f in forms:
                t0 = time.perf_counter()
                for _ in range(steps[k]):
                    f()
                times[k].append((time.perf_counter() - t0) / steps[k] * 1e3)
        ksteps = steps["fused"]
        h.set_profiling(True)
        h.kernel_times()                                             # start a fresh accumulation window
        for _ in range(ksteps):
            fused()
        kt = {k: v[0] / ksteps * 1e3 for k, v in h.kernel_times().items()}
        h.set_profiling(False)
        res = o["results"].cpu().numpy().view(P.TRACK_RESULT).reshape(-1)
        row = dict(frames=B, features_per_frame=int(fc[0]), map_points_per_frame=int(mo[1]), correspondences=int(res["n_correspondences"].sum()),
                   inliers=int(res["n_inliers"].sum()), poses_equal_sequential_form=bool(same),
                   calls_per_round=steps, fused_call_ms=stat(times["fused"]), fused_call_with_map_point_upload_ms=stat(times["fused_upload"]),
                   sequential_calls_ms=stat(times["sequential"]))
        row["fused_over_sequential"] = row["fused_call_ms"]["median"] / row["sequential_calls_ms"]["median"]
        row["fused_with_upload_over_sequential"] = row["fused_call_with_map_point_upload_ms"]["median"] / row["sequential_calls_ms"]["median"]
        row["fused_ms_per_frame"] = row["fused_call_ms"]["median"] / B
        if kt:
            row["fused_kernel_us_per_call"] = kt
        out["rows"].append(row)
        print(json.dumps(row))
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "track_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
