#!/usr/bin/env python3
"""Host time of Handle.track_reference_device (one call: batched mutual nearest neighbour, resolve, gather, PnP-RANSAC, finish;
every array device-resident, one synchronisation at the end) against the same run's sequence of the calls a tracker had to make
before it: per frame orbx_hamming_match_crosscheck_device on the same device-resident descriptors, a download of the matches, the
gather of the matches with a live map point on the host (numpy), then one Handle.solve_pnp_ransac_batch on all frames.  Both forms
do track_with_reference_kf's work (tracker.rs:992-1064) on the same frames; the poses must agree byte for byte.
B = 1 and B = 64 frames, 2000 features per frame, 2000 per keyframe, about 1200 of them with a live map point
(tests/track_reference_scenes.py).  The forms are timed in the same process in alternating rounds, each round at least
--round-seconds long; per form the median over the rounds and the spread (min, max) are reported, plus the device time per kernel
of both forms (orbx_set_profiling).
usage: python scripts/track_reference_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
import argparse
import ctypes as C
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
import track_reference_scenes as R  # noqa: E402


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--keyframe-features", type=int, default=2000)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7 or a.round_seconds < 0.3:
        raise SystemExit("at least 7 rounds of at least 0.3 s")
    if not torch.cuda.is_available():
        raise SystemExit("track_reference_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**R.CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    L = h._L
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, path="track_with_reference_kf", rows=[])
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for B in a.frames:
        # 3/5 of the keyframe's rows are map points seen in the frame, none of them lost: 1200 of 2000
        frames = [R.ref_frame(300 + b, a.keyframe_features, a.features, holes=0.0) for b in range(B)]
        fc = np.array([len(f[0]) for f in frames], np.int32)
        fs = (np.cumsum(fc) - fc).astype(np.int64)
        ko = np.zeros(B + 1, np.int32); ko[1:] = np.cumsum([len(f[2]) for f in frames])
        dev = dict(kp=d(np.concatenate([f[0] for f in frames]).view(np.float32).reshape(-1, 7).copy()), desc=d(np.concatenate([f[1] for f in frames])),
                   feat_start=d(fs.astype(np.int32)), feat_count=d(fc), max_feat=int(fc.max()), kf_desc=d(np.concatenate([f[2] for f in frames])),
                   kf_positions=d(np.concatenate([f[3] for f in frames])), kf_valid=d(np.concatenate([f[4] for f in frames])), kf_offsets=ko,
                   priors_wc=d(np.stack([f[5] for f in frames])))
        torch.cuda.synchronize()

        def fused():
            o = h.track_reference_device(cam, **dev)
            h.synchronize()
            return o

        # the parent's sequence on the same device-resident descriptors
        d_m = torch.empty((int(np.diff(ko).max()), P.DMATCH.itemsize), dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        q_ptr, t_ptr = dev["kf_desc"].data_ptr(), dev["desc"].data_ptr()

        def sequential():
            probs = []
            for b, (kp, _, _, pos, valid, pr) in enumerate(frames):
                nq, nt = int(ko[b + 1] - ko[b]), int(fc[b])
                h._check(L.orbx_hamming_match_crosscheck_device(h._h, C.c_void_p(q_ptr + 32 * int(ko[b])), C.c_int(nq), C.c_void_p(t_ptr + 32 * int(fs[b])),
                                                                C.c_int(nt), C.c_void_p(d_m.data_ptr()), C.c_void_p(d_n.data_ptr())))
                h.synchronize()
                n = int(d_n.item())
                m = d_m[:n].cpu().numpy().view(P.DMATCH).reshape(-1)
                keep = valid[m["query_idx"]] != 0
                qi, ti = m["query_idx"][keep], m["train_idx"][keep]
                probs.append((pos[qi], np.stack([kp["x"][ti], kp["y"][ti]], 1), pr))
            return h.solve_pnp_ransac_batch(cam, probs)

        forms = (("fused", fused), ("sequential", sequential))
        for _ in range(a.warmup):
            o = fused(); s = sequential()
        poses = o["poses"].cpu().numpy()
        res = o["results"].cpu().numpy().view(P.TRACK_REF_RESULT).reshape(-1)
        assert (res["status"] != P.TRACK_TOO_FEW_CORRESPONDENCES).all(), res["status"]
        assert all(poses[b].tobytes() == s[b].pose.tobytes() for b in range(B)), "the fused call and the sequence of calls disagree"
        steps, times = {}, {k: [] for k, _ in forms}
        for k, f in forms:                                           # calls per round: enough to fill round_seconds
            t0 = time.perf_counter(); f(); f(); one = (time.perf_counter() - t0) / 2
            steps[k] = max(3, int(np.ceil(a.round_seconds / one)))
        for _ in range(a.rounds):                                    # alternating rounds: drift hits every form alike
            for k, f in forms:
                t0 = time.perf_counter()
                for _ in range(steps[k]):
                    f()
                times[k].append((time.perf_counter() - t0) / steps[k] * 1e3)
        kt = {}
        h.set_profiling(True)
        for k, f in forms:
            h.kernel_times()                                         # start a fresh accumulation window
            for _ in range(steps[k]):
                f()
            kt[k] = {name: v[0] / steps[k] * 1e3 for name, v in h.kernel_times().items()}
        h.set_profiling(False)
        row = dict(frames=B, features_per_frame=int(fc[0]), keyframe_features=int(ko[1]), matches=int(res["n_matches"].sum()),
                   correspondences=int(res["n_correspondences"].sum()), inliers=int(res["n_inliers"].sum()), poses_equal_sequential_form=True,
                   calls_per_round=steps, fused_call_ms=stat(times["fused"]), sequential_calls_ms=stat(times["sequential"]))
        row["fused_over_sequential"] = row["fused_call_ms"]["median"] / row["sequential_calls_ms"]["median"]
        row["fused_range_wholly_below_sequential_range"] = row["fused_call_ms"]["max"] < row["sequential_calls_ms"]["min"]
        row["fused_ms_per_frame"] = row["fused_call_ms"]["median"] / B
        row["fused_kernel_us_per_call"] = kt["fused"]
        row["sequential_kernel_us_per_call"] = kt["sequential"]
        out["rows"].append(row)
        print(json.dumps(row))
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "track_reference_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
