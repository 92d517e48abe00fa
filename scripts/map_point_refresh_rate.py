#!/usr/bin/env python3
"""Host time of the map-point refresh (phase 4 of search_in_neighbors) at local-mapping size: T = 40 resident keyframes of 2000
features, M = 12 000 map points with track lengths drawn from 2..40 and a few at 65..300.  Two figures: the whole host call of the
keyframe form (KeyFrame.refresh_map_points: points and lists up, results down, synchronous) and the device form with everything
resident (Handle.refresh_map_points_device, one synchronisation per call); the device time per kernel (orbx_set_profiling).
Nothing in the library did this work before, so the yardstick is a compiled host loop of the specification over the same arrays
(scripts/map_point_refresh_host_loop.cpp) at 1 and 16 threads, in the same run; its outputs are compared with the call's first.
Per figure the median over the rounds and the spread (min, max); each round is at least --round-seconds long.
usage: python scripts/map_point_refresh_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import orb_slam3_rust_amd as P  # noqa: E402


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def workload(T, n_feat, M, n_long, seed=1):
    rng = np.random.default_rng(seed)
    q = rng.normal(0, 1, (T, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    poses = np.concatenate([q, rng.uniform(-0.5, 0.5, (T, 3))], 1)
    lengths = rng.integers(2, 41, M)
    lengths[rng.permutation(M)[:n_long]] = rng.integers(65, 301, n_long)
    start = np.zeros(M + 1, np.int32); start[1:] = np.cumsum(lengths)
    N = int(start[-1])
    return dict(positions=np.stack([rng.uniform(-2, 2, M), rng.uniform(-2, 2, M), rng.uniform(4, 10, M)], 1), obs_start=start,
                obs_kf=rng.integers(0, T, N).astype(np.int32), obs_feat=rng.integers(0, n_feat, N).astype(np.int32), kf_poses_wc=poses,
                kf_feat_offset=(np.arange(T + 1) * n_feat).astype(np.int32), descs=rng.integers(0, 256, (T * n_feat, 32), dtype=np.uint8),
                scale_range=1.2 ** 7, mp_desc=rng.integers(0, 256, (M, 32), dtype=np.uint8), normals=np.tile([0.0, 0.0, 1.0], (M, 1)))


def build_host_loop(tmp):
    so = os.path.join(tmp, "libmp_refresh_host_loop.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mpopcnt", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "scripts", "map_point_refresh_host_loop.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.mp_refresh_host_loop.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 5 + [C.c_int]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keyframes", type=int, default=40)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--points", type=int, default=12000)
    ap.add_argument("--long-points", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7 or a.round_seconds < 0.3:
        raise SystemExit("at least 7 rounds of at least 0.3 s")
    if not torch.cuda.is_available():
        raise SystemExit("map_point_refresh_rate.py measures on the GPU; none is visible")
    h = P.Handle(P.CameraModel(**P.synth.EUROC_CAMERA), 2000, device=0, max_w=752, max_h=480, max_batch=1)
    w = workload(a.keyframes, a.features, a.points, a.long_points)
    T, M, N = a.keyframes, a.points, int(w["obs_start"][-1])
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    kfs = [P.KeyFrame(h, torch.zeros((a.features, P.KEYPOINT.itemsize), dtype=torch.uint8, device="cuda"),
                      d(w["descs"][t * a.features:(t + 1) * a.features]), a.features, keyframe_id=t, pose_wc=w["kf_poses_wc"][t]) for t in range(T)]
    dev = dict(positions=d(w["positions"]), obs_start=d(w["obs_start"]), obs_kf=d(w["obs_kf"]), obs_feat=d(w["obs_feat"]), descs=d(w["descs"]),
               mp_desc=d(w["mp_desc"]), normals=d(w["normals"]))
    torch.cuda.synchronize()

    def timed(f, profile):
        t0 = time.perf_counter(); f(); f(); one = (time.perf_counter() - t0) / 2
        steps = max(3, int(np.ceil(a.round_seconds / one)))
        times = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(steps):
                f()
            times.append((time.perf_counter() - t0) / steps * 1e3)
        kt = None
        if profile:
            h.set_profiling(True)
            h.kernel_times()
            for _ in range(steps):
                f()
            kt = {name: v[0] / steps * 1e3 for name, v in h.kernel_times().items()}
            h.set_profiling(False)
        return steps, stat(times), kt

    def kf_call():
        return P.KeyFrame.refresh_map_points(h, kfs, w["positions"], w["obs_start"], w["obs_kf"], w["obs_feat"], w["scale_range"], w["mp_desc"], w["normals"])

    def dev_call():
        o = h.refresh_map_points_device(dev["positions"], dev["obs_start"], dev["obs_kf"], dev["obs_feat"], N, w["kf_poses_wc"], w["kf_feat_offset"],
                                        dev["descs"], w["scale_range"], dev["mp_desc"], dev["normals"])
        h.synchronize()
        return o
    for _ in range(a.warmup):
        got = kf_call(); dev_call()
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, path="search_in_neighbors phase 4",
               keyframes=T, features_per_keyframe=a.features, points=M, observations=N, long_points=a.long_points,
               hamming_distances=int((np.diff(w["obs_start"]).astype(np.int64) ** 2).sum()),
               descriptor_bytes_not_crossing_pcie_per_refresh=32 * T * a.features)
    with tempfile.TemporaryDirectory() as tmp:
        HL = build_host_loop(tmp)
        ho = dict(mp_desc=w["mp_desc"].copy(), normals=w["normals"].copy(), mn=np.zeros(M), mx=np.zeros(M), rec=np.zeros(M, P.MP_REFRESH_RECORD))

        def host(threads):
            return HL.mp_refresh_host_loop(M, w["positions"].ctypes.data, w["obs_start"].ctypes.data, w["obs_kf"].ctypes.data, w["obs_feat"].ctypes.data, T,
                                           w["kf_poses_wc"].ctypes.data, w["kf_feat_offset"].ctypes.data, w["descs"].ctypes.data, w["scale_range"],
                                           ho["mp_desc"].ctypes.data, ho["normals"].ctypes.data, ho["mn"].ctypes.data, ho["mx"].ctypes.data,
                                           ho["rec"].ctypes.data, threads)
        host(16)
        assert ho["rec"].tobytes() == got.records.tobytes() and np.array_equal(ho["mp_desc"], got.mp_desc), "the host loop and the call disagree"
        out["largest_differences_call_vs_host_loop"] = dict(normal=float(np.abs(ho["normals"] - got.normals).max()),
                                                            min_distance=float(np.abs(ho["mn"] - got.min_distance).max()),
                                                            max_distance=float(np.abs(ho["mx"] - got.max_distance).max()))
        steps, t, kt = timed(kf_call, True)
        out["keyframe_form_host_call_ms"] = t; out["keyframe_form_calls_per_round"] = steps; out["kernel_us_per_call"] = kt
        steps, t, _ = timed(dev_call, False)
        out["device_form_ms"] = t; out["device_form_calls_per_round"] = steps
        for threads in (1, 16):
            steps, t, _ = timed(lambda: host(threads), False)
            out["host_loop_ms_%d_threads" % threads] = t
        # what the host loop needs first: every keyframe's descriptors on the host
        steps, t, _ = timed(lambda: [k.download() for k in kfs], False)
        out["download_of_the_keyframes_ms"] = t
    out["keyframe_form_faster_than_16_thread_loop"] = bool(out["keyframe_form_host_call_ms"]["median"] < out["host_loop_ms_16_threads"]["median"])
    out["device_form_faster_than_16_thread_loop"] = bool(out["device_form_ms"]["median"] < out["host_loop_ms_16_threads"]["median"])
    for k in kfs:
        k.close()
    h.close()
    print(json.dumps(out))
    path = a.out or os.path.join(ROOT, "profiles", "map_point_refresh_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
