#!/usr/bin/env python3
"""Host time of Handle.map_track_frames_device (the local-map selection from the resident store, then the tracker's launches; one
synchronisation at the end) against the same run's sequence a caller has to make without the store: the first-seen distinct union
of the keyframes' slot tables and the gather of positions and descriptors on the host (numpy), their upload, then
Handle.track_frames_device.  The host part and the upload are also timed alone.  numpy is slower at the union than a compiled shim
would be (a hash set over about 22 k entries): the host figure is an upper bound on what such a shim pays.
Likewise the reference-keyframe form: Handle.map_track_reference_device against Handle.keyframe_track_reference with kf_positions /
kf_valid gathered on the host and sent with the call.
B = 1 and B = 64 frames; per frame 11 keyframes of 2000 features (22 000 candidates, a quarter of them None) over 1500 - 4000
distinct points; a store of 50 000 live points.  The forms are timed in the same process in alternating rounds, each round at
least --round-seconds long; per form the median over the rounds and the spread (min, max) are reported, plus the device time per
kernel of the resident call.
usage: python scripts/map_store_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
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
import track_reference_scenes as R  # noqa: E402
import tracking_scenes as G  # noqa: E402

CAPACITY, LIVE, N_KF, KF_FEAT, SCENES = 65536, 50000, 11, 2000, 8


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def overlap(a, b):
    return not (a["max"] < b["min"] or b["max"] < a["min"])


def first_seen_union(tables, live):
    """what the caller does on the host: distinct live slots in first-seen order"""
    c = np.concatenate(tables)
    c = c[c >= 0]
    c = c[live[c] != 0]
    _, idx = np.unique(c, return_index=True)
    return c[np.sort(idx)]


def measure(forms, rounds, round_seconds):
    steps, times = {}, {k: [] for k, _ in forms}
    for k, f in forms:
        t0 = time.perf_counter(); f(); f(); one = (time.perf_counter() - t0) / 2
        steps[k] = max(10, int(np.ceil(round_seconds / one)))
    for _ in range(rounds):
        for k, f in forms:
            t0 = time.perf_counter()
            for _ in range(steps[k]):
                f()
            times[k].append((time.perf_counter() - t0) / steps[k] * 1e3)
    return steps, {k: stat(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_store_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**G.CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    cfg = P.TrackConfig.for_mode(P.TRACK_LOCAL_MAP)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    rng = np.random.default_rng(1)
    # the store: SCENES frames' points at their own slots, random live points up to LIVE
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
    mp = P.MapPointStore(h, CAPACITY)
    ls = np.flatnonzero(live).astype(np.int32)
    mp.set(ls, pos[ls], desc[ls])
    zk, zd = torch.zeros((KF_FEAT, 7), dtype=torch.float32, device="cuda"), torch.zeros((KF_FEAT, 32), dtype=torch.uint8, device="cuda")
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, capacity=CAPACITY, live_points=int(live.sum()),
               note="the host figures are numpy's: a compiled shim is faster at the union", rows=[], reference_rows=[])
    keep = []
    for B in (1, 64):
        frames, tables, kfs = [], [], []
        for b in range(B):
            f, slots = scenes[b % SCENES]
            c = np.concatenate([slots, slots[rng.integers(0, len(slots), N_KF * KF_FEAT - len(slots))]]).astype(np.int32)
            c = c[rng.permutation(len(c))]
            c[rng.uniform(size=len(c)) < 0.25] = -1
            tb = [np.ascontiguousarray(t) for t in c.reshape(N_KF, KF_FEAT)]
            ks = []
            for t in tb:
                k = P.KeyFrame(h, zk, zd, KF_FEAT)
                k.set_map_point_slots(mp, t)
                ks.append(k)
            frames.append(f); tables.append(tb); kfs.append(ks); keep.extend(ks)
        fc = np.array([len(f[0]) for f in frames], np.int32)
        dev = dict(kp=d(np.concatenate([f[0] for f in frames]).view(np.float32).reshape(-1, 7).copy()), desc=d(np.concatenate([f[1] for f in frames])),
                   feat_start=d((np.cumsum(fc) - fc).astype(np.int32)), feat_count=d(fc), max_feat=int(fc.max()),
                   search_poses_wc=d(np.stack([f[4] for f in frames])), priors_wc=d(np.stack([f[5] for f in frames])))

        def resident():
            o = h.map_track_frames_device(cam, mp, keyframes=kfs, cfg=cfg, **dev)
            h.synchronize()
            return o

        def host_part():
            lists = [first_seen_union(tb, live) for tb in tables]
            cat = np.concatenate(lists)
            mo = np.zeros(B + 1, np.int32); mo[1:] = np.cumsum([len(x) for x in lists])
            return pos[cat], desc[cat], mo

        staged = host_part()

        def upload():
            t = torch.from_numpy(staged[0]).cuda(), torch.from_numpy(staged[1]).cuda()
            torch.cuda.synchronize()
            return t

        def parent_sequence():
            p, de, mo = host_part()
            o = h.track_frames_device(cam, positions=torch.from_numpy(p).cuda(), mp_desc=torch.from_numpy(de).cuda(), mp_offsets=mo, cfg=cfg, **dev)
            h.synchronize()
            return o

        forms = (("resident", resident), ("parent_sequence", parent_sequence), ("host_union_and_gather", host_part), ("upload", upload))
        for _ in range(a.warmup):
            o = resident(); s = parent_sequence(); upload()
        same = o["poses"].cpu().numpy().tobytes() == s["poses"].cpu().numpy().tobytes() and \
            o["list_offsets"].cpu().numpy().tolist() == staged[2].tolist()
        steps, t = measure(forms, a.rounds, a.round_seconds)
        h.set_profiling(True)
        h.kernel_times()
        for _ in range(steps["resident"]):
            resident()
        kt = {k: v[0] / steps["resident"] * 1e3 for k, v in h.kernel_times().items()}
        h.set_profiling(False)
        res = o["results"].cpu().numpy().view(P.TRACK_RESULT).reshape(-1)
        row = dict(frames=B, keyframes_per_frame=N_KF, candidates_per_frame=N_KF * KF_FEAT, list_points=int(staged[2][-1]), inliers=int(res["n_inliers"].sum()),
                   equal_to_parent_sequence=bool(same), calls_per_round=steps, resident_call_ms=t["resident"], parent_sequence_ms=t["parent_sequence"],
                   host_union_and_gather_ms=t["host_union_and_gather"], upload_ms=t["upload"],
                   ranges_overlap=overlap(t["resident"], t["parent_sequence"]), resident_kernel_us_per_call=kt,
                   selection_kernels_us_per_call=sum(v for k, v in kt.items() if k in ("map_mark_kernel", "map_flag_kernel", "map_emit_kernel")))
        out["rows"].append(row)
        print(json.dumps(row))
        # the reference-keyframe form: frame b against one 2000-feature keyframe
        rf = [R.ref_frame(300 + s, KF_FEAT, KF_FEAT) for s in range(min(B, SCENES))]
        rkf, rtab = [], []
        for s, f in enumerate(rf):
            n_ok = int(np.sum(np.asarray(f[4]) != 0))
            t = np.full(len(f[2]), -1, np.int32)
            sl = order[used:used + n_ok]; used += n_ok
            t[np.asarray(f[4]) != 0] = sl
            pos[sl] = np.asarray(f[3])[np.asarray(f[4]) != 0]; live[sl] = 1
            mp.set(sl, pos[sl], desc[sl])
            k = P.KeyFrame(h, torch.zeros((len(t), 7), dtype=torch.float32, device="cuda"), d(f[2]), len(t))
            k.set_map_point_slots(mp, t)
            rkf.append(k); rtab.append(t); keep.append(k)
        fr = [rf[b % len(rf)] for b in range(B)]
        ks = [rkf[b % len(rf)] for b in range(B)]
        tb = [rtab[b % len(rf)] for b in range(B)]
        fc = np.array([len(f[0]) for f in fr], np.int32)
        rdev = dict(kp=d(np.concatenate([f[0] for f in fr]).view(np.float32).reshape(-1, 7).copy()), desc=d(np.concatenate([f[1] for f in fr])),
                    feat_start=d((np.cumsum(fc) - fc).astype(np.int32)), feat_count=d(fc), max_feat=int(fc.max()), priors_wc=d(np.stack([f[5] for f in fr])))

        def ref_resident():
            o = h.map_track_reference_device(R_CAM, mp, ks, **rdev)
            h.synchronize()
            return o

        def ref_host_rows():
            rows = []
            for t in tb:
                ok = (t >= 0) & (live[np.maximum(t, 0)] != 0)
                p = np.zeros((len(t), 3)); p[ok] = pos[t[ok]]
                rows.append((p, ok.astype(np.uint8)))
            return rows

        def ref_parent():
            rows = ref_host_rows()
            o = h.keyframe_track_reference(R_CAM, ks, rdev["kp"], rdev["desc"], rdev["feat_start"], rdev["feat_count"], rdev["max_feat"], [r[0] for r in rows],
                                           [r[1] for r in rows], rdev["priors_wc"])
            h.synchronize()
            return o

        R_CAM = P.CameraModel(**R.CAMERA)
        for _ in range(a.warmup):
            o = ref_resident(); s = ref_parent()
        same = o["poses"].cpu().numpy().tobytes() == s["poses"].cpu().numpy().tobytes()
        steps, t = measure((("resident", ref_resident), ("parent_sequence", ref_parent), ("host_rows", ref_host_rows)), a.rounds, a.round_seconds)
        row = dict(frames=B, keyframe_features=KF_FEAT, equal_to_parent_sequence=bool(same), calls_per_round=steps, resident_call_ms=t["resident"],
                   parent_sequence_ms=t["parent_sequence"], host_rows_ms=t["host_rows"], ranges_overlap=overlap(t["resident"], t["parent_sequence"]))
        out["reference_rows"].append(row)
        print(json.dumps(row))
    h.synchronize()
    for k in keep:
        k.close()
    mp.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "map_store_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
