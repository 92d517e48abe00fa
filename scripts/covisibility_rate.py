#!/usr/bin/env python3
"""Host time of the covisibility calls on the resident map against the same run's sequence a caller makes today.

  covisibility alone    Handle.map_covisibility_device (weights and the 10 best neighbours of Q query keyframes; one synchronisation
                        at the end) against the weights and top-10 computed from the slot tables on the host with numpy: a mark
                        array over the store, one gather over every keyframe's de-duplicated table, a row sum and a stable sort.
                        A compiled, incrementally maintained graph (what the reference keeps) is cheaper than this recomputation,
                        so the host figure bounds the host cost from above.
  local-map tracking    Handle.map_track_local_device (reference-keyframe index in, pose out) against that host computation
                        followed by Handle.map_track_frames_device with the chosen keyframe lists.

100 and 1000 keyframes of 2000 features over a store of 50 000 live points (capacity 65 536); 1 and 64 queries / frames.  Frame b's
reference keyframe is the first of a group of 11 keyframes that observe the frame's points, so its 10 best covisibles are the
rest of the group; the other keyframes observe a sliding window of the remaining points.  The forms are timed in the same process
in alternating rounds, each round at least --round-seconds long; per form the median over the rounds and the spread (min, max) are
reported, plus the device time per kernel of the resident tracking call.
usage: python scripts/covisibility_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
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

CAPACITY, LIVE, GROUP, KF_FEAT, SCENES, N_BEST = 65536, 50000, 11, 2000, 8, 10
COV_KERNELS = ("cov_mark_kernel", "cov_count_kernel", "cov_rank_kernel", "cov_seg_kernel")
SEL_KERNELS = ("map_mark_kernel", "map_flag_kernel", "map_emit_kernel")


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def overlap(a, b):
    return not (a["max"] < b["min"] or b["max"] < a["min"])


def measure(forms, rounds, round_seconds):
    steps, times = {}, {k: [] for k, _ in forms}
    for k, f in forms:
        t0 = time.perf_counter(); f(); one = time.perf_counter() - t0
        steps[k] = max(3, int(np.ceil(round_seconds / one)))
    for _ in range(rounds):
        for k, f in forms:
            t0 = time.perf_counter()
            for _ in range(steps[k]):
                f()
            times[k].append((time.perf_counter() - t0) / steps[k] * 1e3)
    return steps, {k: stat(v) for k, v in times.items()}


def dedup(t):
    """a slot table with every repeat set to -1 (what a host-side graph would keep per keyframe as well)"""
    u = t.copy()
    order = np.argsort(t, kind="stable")
    rep = np.zeros(len(t), bool)
    rep[order[1:]] = t[order[1:]] == t[order[:-1]]
    u[rep] = -1
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("covisibility_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**G.CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    cfg = P.TrackConfig.for_mode(P.TRACK_LOCAL_MAP)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rng = np.random.default_rng(1)
    pos = rng.uniform(-5.0, 5.0, (CAPACITY, 3)); desc = rng.integers(0, 256, (CAPACITY, 32), dtype=np.uint8); live = np.zeros(CAPACITY, np.uint8)
    order = rng.permutation(CAPACITY).astype(np.int32)
    scenes, used = [], 0
    for s in range(SCENES):
        n_mp = int(np.linspace(1500, 4000, SCENES)[s])
        f = G.frame(200 + s, n_mp, KF_FEAT)
        slots = order[used:used + n_mp]; used += n_mp
        pos[slots] = f[2]; desc[slots] = f[3]
        scenes.append((f, slots))
    live[order[:LIVE]] = 1
    rest = order[used:LIVE]
    mp = P.MapPointStore(h, CAPACITY)
    ls = np.flatnonzero(live).astype(np.int32)
    mp.set(ls, pos[ls], desc[ls])
    zk, zd = torch.zeros((KF_FEAT, 7), dtype=torch.float32, device="cuda"), torch.zeros((KF_FEAT, 32), dtype=torch.uint8, device="cuda")
    # the keyframes: SCENES groups of GROUP keyframes over their frame's points, then keyframes over a sliding window of the rest
    tables = []
    for f, slots in scenes:
        c = np.concatenate([slots, slots[rng.integers(0, len(slots), GROUP * KF_FEAT - len(slots))]]).astype(np.int32)
        c = c[rng.permutation(len(c))]
        c[rng.uniform(size=len(c)) < 0.25] = -1
        tables.extend(np.ascontiguousarray(t) for t in c.reshape(GROUP, KF_FEAT))
    while len(tables) < 1000:
        lo = (len(tables) * 37) % max(len(rest) - 6000, 1)
        t = rest[lo + rng.integers(0, 6000, KF_FEAT)].astype(np.int32)
        t[rng.uniform(size=KF_FEAT) < 0.25] = -1
        tables.append(t)
    all_kfs = []
    for t in tables:
        k = P.KeyFrame(h, zk, zd, KF_FEAT)
        k.set_map_point_slots(mp, t)
        all_kfs.append(k)
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, capacity=CAPACITY, live_points=int(live.sum()),
               keyframe_features=KF_FEAT, n_best=N_BEST,
               note="the host figures are numpy's recomputation from the slot tables; a compiled, incrementally maintained graph is cheaper, so they bound the host cost from above",
               rows=[])
    for n_kfs in (100, 1000):
        kfs = all_kfs[:n_kfs]
        uniq = np.stack([dedup(t) for t in tables[:n_kfs]])                        # [n_kfs, KF_FEAT]
        for B in (1, 64):
            ref = [(b % SCENES) * GROUP for b in range(B)]
            frames = [scenes[b % SCENES][0] for b in range(B)]
            fc = np.array([len(f[0]) for f in frames], np.int32)
            dev = dict(kp=d(np.concatenate([f[0] for f in frames]).view(np.float32).reshape(-1, 7).copy()), desc=d(np.concatenate([f[1] for f in frames])),
                       feat_start=d((np.cumsum(fc) - fc).astype(np.int32)), feat_count=d(fc), max_feat=int(fc.max()),
                       search_poses_wc=d(np.stack([f[4] for f in frames])), priors_wc=d(np.stack([f[5] for f in frames])))

            def cov_resident():
                o = h.map_covisibility_device(mp, kfs, ref, N_BEST)
                h.synchronize()
                return o

            def cov_host():
                safe = np.maximum(uniq, 0)
                seen = (uniq >= 0) & (live[safe] != 0)
                best = []
                for q in ref:
                    mark = np.zeros(CAPACITY, bool)
                    mark[uniq[q][seen[q]]] = True
                    w = (mark[safe] & seen).sum(axis=1)
                    w[q] = 0
                    top = np.argsort(-w, kind="stable")[:N_BEST]
                    best.append(top[w[top] > 0])
                return best

            def local_resident():
                o = h.map_track_local_device(cam, mp, kfs, ref, N_BEST, cfg=cfg, **dev)
                h.synchronize()
                return o

            def parent_sequence():
                lists = [[kfs[q]] + [kfs[int(i)] for i in b] for q, b in zip(ref, cov_host())]
                o = h.map_track_frames_device(cam, mp, keyframes=lists, cfg=cfg, **dev)
                h.synchronize()
                return o

            for _ in range(a.warmup):
                c = cov_resident(); o = local_resident(); s = parent_sequence()
            hb = cov_host()
            cb, cn = c["best"].cpu().numpy(), c["n_best"].cpu().numpy()
            same_best = all(cb[i, :cn[i]].tolist() == hb[i].tolist() for i in range(B))
            same_pose = o["poses"].cpu().numpy().tobytes() == s["poses"].cpu().numpy().tobytes() and \
                o["list_offsets"].cpu().numpy().tolist() == s["list_offsets"].cpu().numpy().tolist()
            forms = (("covisibility_resident", cov_resident), ("covisibility_host", cov_host), ("track_local_resident", local_resident),
                     ("track_parent_sequence", parent_sequence))
            steps, t = measure(forms, a.rounds, a.round_seconds)
            h.set_profiling(True)
            h.kernel_times()
            for _ in range(steps["track_local_resident"]):
                local_resident()
            kt = {k: v[0] / steps["track_local_resident"] * 1e3 for k, v in h.kernel_times().items()}
            h.set_profiling(False)
            res = o["results"].cpu().numpy().view(P.TRACK_RESULT).reshape(-1)
            row = dict(keyframes=n_kfs, queries=B, frames=B, list_points=int(o["list_offsets"][-1].item()), inliers=int(res["n_inliers"].sum()),
                       best_equal_to_host=bool(same_best), track_equal_to_parent_sequence=bool(same_pose), calls_per_round=steps,
                       covisibility_resident_ms=t["covisibility_resident"], covisibility_host_ms=t["covisibility_host"],
                       covisibility_ranges_overlap=overlap(t["covisibility_resident"], t["covisibility_host"]),
                       track_local_resident_ms=t["track_local_resident"], track_parent_sequence_ms=t["track_parent_sequence"],
                       track_ranges_overlap=overlap(t["track_local_resident"], t["track_parent_sequence"]), track_local_kernel_us_per_call=kt,
                       covisibility_kernels_us_per_call=sum(v for k, v in kt.items() if k in COV_KERNELS),
                       selection_kernels_us_per_call=sum(v for k, v in kt.items() if k in SEL_KERNELS))
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
    h.synchronize()
    for k in all_kfs:
        k.close()
    mp.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "covisibility_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
