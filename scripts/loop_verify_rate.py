#!/usr/bin/env python3
"""Host time of Handle.verify_loop_candidates_device (one call: ratio matcher, resolve, Sim3-RANSAC, reprojection count; every
feature array device-resident, one synchronisation at the end) for B = 1 and B = 8 pairs of 2000-feature keyframes, with the
brute-force and the FeatureVector matcher, and the device time per kernel (orbx_set_profiling).  No earlier call sequence does
this work, so nothing is compared with it.  The yardstick for the brute-force matcher is tref_nn_kernel (track_ref_kernels.hip),
timed in the same process on the same 2000 x 2000 descriptors: lv_match_kernel computes the same 4 M distances per pair without
the column atomics.  Per figure the median over the rounds and the spread (min, max) are reported; each round is at least
--round-seconds long.
usage: python scripts/loop_verify_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
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

import loop_verify_scenes as Z  # noqa: E402
import orb_slam3_rust_amd as P  # noqa: E402


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7 or a.round_seconds < 0.3:
        raise SystemExit("at least 7 rounds of at least 0.3 s")
    if not torch.cuda.is_available():
        raise SystemExit("loop_verify_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**Z.CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, path="verify_loop_candidate", rows=[])
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    scenes = [Z.keyframe_pair(500 + b, a.features, (3 * a.features) // 4, outlier_frac=0.2, stereo_common=0.9, with_nodes=True) for b in range(max(a.pairs))]

    def timed(f):
        t0 = time.perf_counter(); f(); f(); one = (time.perf_counter() - t0) / 2
        steps = max(3, int(np.ceil(a.round_seconds / one)))
        times = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            times.append((time.perf_counter() - t0) / steps * 1e3)
        h.set_profiling(True)
        h.kernel_times()                                             # start a fresh accumulation window
        for _ in range(steps):
            f()
        kt = {name: v[0] / steps * 1e3 for name, v in h.kernel_times().items()}
        h.set_profiling(False)
        return steps, stat(times), kt

    for B in a.pairs:
        pairs = scenes[:B]
        for form in ("brute_force", "feature_vector"):
            use = pairs if form == "feature_vector" else [tuple({k: v for k, v in s.items() if k != "node"} for s in p) for p in pairs]
            arr, cn, ln, co, lo, cp, lp = h._loop_verify_pack(use)
            dev = [d(arr["cur_desc"]), d(arr["cur_pts"]), d(arr["cur_has"]), co, cp, d(arr["loop_kp"].view(np.uint8).reshape(-1, 28)), d(arr["loop_desc"]),
                   d(arr["loop_pts"]), d(arr["loop_has"]), lo, lp, cn, ln]
            torch.cuda.synchronize()

            def call():
                o = h.verify_loop_candidates_device(cam, *dev)
                h.synchronize()
                return o
            for _ in range(a.warmup):
                o = call()
            res = o["results"].cpu().numpy().view(P.LOOP_VERIFY_RESULT).reshape(-1)
            assert (res["status"] == P.LOOP_OK).all(), res["status"]
            steps, t, kt = timed(call)
            row = dict(pairs=B, matcher=form, features_per_keyframe=a.features, matches=int(res["n_matches"].sum()), point_pairs=int(res["n_pairs"].sum()),
                       inliers=int(res["n_inliers"].sum()), verified=int(res["n_verified"].sum()), calls_per_round=steps, call_ms=t,
                       ms_per_pair=t["median"] / B, kernel_us_per_call=kt)
            if form == "brute_force":
                # the yardstick: tref_nn_kernel on the same descriptors (current keyframe as the reference keyframe, loop keyframe as the frame)
                n = a.features
                fo = (np.arange(B) * n).astype(np.int32)
                tr = dict(kp=d(np.zeros((B * n, 7), np.float32)), desc=dev[6], feat_start=d(fo), feat_count=d(np.full(B, n, np.int32)), max_feat=n,
                          kf_desc=dev[0], kf_positions=d(np.zeros((B * n, 3))), kf_valid=d(np.zeros(B * n, np.uint8)), kf_offsets=co,
                          priors_wc=d(np.tile([1.0, 0, 0, 0, 0, 0, 0], (B, 1))))
                torch.cuda.synchronize()

                def yard():
                    h.track_reference_device(cam, **tr)
                    h.synchronize()
                for _ in range(a.warmup):
                    yard()
                _, _, ykt = timed(yard)
                row["yardstick_tref_nn_kernel_us"] = ykt["tref_nn_kernel"]
                row["lv_match_over_tref_nn"] = kt["lv_match_kernel"] / ykt["tref_nn_kernel"]
                row["lv_match_within_110_percent_of_tref_nn"] = bool(kt["lv_match_kernel"] <= 1.1 * ykt["tref_nn_kernel"])
            out["rows"].append(row)
            print(json.dumps(row))
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "loop_verify_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
