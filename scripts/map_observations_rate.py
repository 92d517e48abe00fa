#!/usr/bin/env python3
"""Host time of the observation calls on the resident map against the same run's sequence a caller makes today.

  (a) refresh      Handle.map_refresh_points (lists derived on the device, the refresh kernels, the descriptors written back into the
                   store; host form, synchronous) and Handle.map_refresh_points_device with one synchronisation, against today's
                   sequence: the observation lists built on the host from the slot tables (numpy: one gather over the de-duplicated
                   tables, a stable sort by point), KeyFrame.refresh_map_points with them, MapPointStore.set of the descriptors.  The
                   list building is numpy: a compiled shim that maintains mp.observations per association pays less for it, so that
                   part bounds the host cost from above; it is reported apart for that reason.
                   40 resident keyframes of 2000 features (1800 of them on a point, none twice), 12 000 points.
  (b) lists alone  Handle.map_observations_device and one synchronisation, against the numpy list building.
  (c) redundancy   Handle.map_keyframe_redundancy (host form) for 20 candidates among N = 100 and 1000 resident keyframes of 2000
                   features, store of 50 000 live points, against a numpy recomputation (bincount over the de-duplicated tables, one
                   gather per candidate).  Again an upper bound on what a compiled shim with maintained observation counts pays.

The forms are timed in the same process in alternating rounds, each at least --round-seconds long; per form the median over the
rounds and the spread (min, max), plus the device time per kernel (orbx_get_kernel_times).
usage: python scripts/map_observations_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import orb_slam3_rust_amd as P  # noqa: E402

SCALE_RANGE = 1.2 ** 7
KF_FEAT = 2000


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


def kernel_us(h, f, steps):
    h.set_profiling(True)
    h.kernel_times()
    for _ in range(steps):
        f()
    kt = {k: v[0] / steps * 1e3 for k, v in h.kernel_times().items()}
    h.set_profiling(False)
    return kt


def uniq_table(t):
    """a slot table with every repeat of a slot set to -1 (what orbx_keyframe_set_map_point_slots keeps beside the table)"""
    u = t.copy()
    order = np.argsort(t, kind="stable")
    rep = np.zeros(len(t), bool)
    rep[order[1:]] = t[order[1:]] == t[order[:-1]]
    u[rep] = -1
    return u


def host_lists(cat_slot, cat_kf, cat_feat, live, index, slots):
    """the specification's lists in numpy from the concatenated de-duplicated tables (entries in keyframe order)"""
    index[slots] = np.arange(len(slots), dtype=np.int32)
    ok = cat_slot >= 0
    ok[ok] = live[cat_slot[ok]] == 1
    p = np.full(len(cat_slot), -1, np.int32)
    p[ok] = index[cat_slot[ok]]
    keep = p >= 0
    order = np.argsort(p[keep], kind="stable")                               # by point; the keyframes stay ascending inside a point
    start = np.zeros(len(slots) + 1, np.int32)
    start[1:] = np.cumsum(np.bincount(p[keep], minlength=len(slots)))
    index[slots] = -1
    return start, cat_kf[keep][order], cat_feat[keep][order]


def world(h, rng, capacity, n_live, n_kfs, per_kf, pool=None):
    """a store of n_live points and n_kfs keyframes of KF_FEAT features, per_kf of them on a point of the keyframe's pool, none twice"""
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    live_slots = np.sort(rng.permutation(capacity)[:n_live]).astype(np.int32)
    pos = rng.uniform(-5.0, 5.0, (capacity, 3)); desc = rng.integers(0, 256, (capacity, 32), dtype=np.uint8)
    live = np.zeros(capacity, np.uint8); live[live_slots] = 1
    mp = P.MapPointStore(h, capacity)
    mp.set(live_slots, pos[live_slots], desc[live_slots])
    tables, kfs = [], []
    for k in range(n_kfs):
        src = live_slots if pool is None else live_slots[(k * 37) % max(n_live - pool, 1):][:pool]
        t = np.full(KF_FEAT, -1, np.int32)
        t[rng.permutation(KF_FEAT)[:per_kf]] = rng.permutation(src)[:per_kf]
        pose = np.concatenate([[1.0, 0, 0, 0], rng.uniform(-30.0, -20.0, 3)])
        kf = P.KeyFrame(h, torch.zeros((KF_FEAT, 7), dtype=torch.float32, device="cuda"), d(rng.integers(0, 256, (KF_FEAT, 32), dtype=np.uint8)), KF_FEAT, pose_wc=pose)
        kf.set_map_point_slots(mp, t)
        tables.append(t); kfs.append(kf)
    return mp, kfs, tables, live, live_slots, pos, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_observations_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**P.synth.EUROC_CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds,
               note="host_lists and redundancy_numpy are numpy recomputations from the slot tables: an upper bound on what a compiled shim that "
                    "maintains mp.observations per association pays; parent_sequence = host_lists + KeyFrame.refresh_map_points + MapPointStore.set",
               refresh=[], redundancy=[])
    # ---- (a), (b): the README's refresh shape
    rng = np.random.default_rng(11)
    mp, kfs, tables, live, slots, pos, desc = world(h, rng, 16384, 12000, 40, 1800)
    uq = [uniq_table(t) for t in tables]
    cat_slot = np.concatenate(uq); cat_kf = np.repeat(np.arange(40, dtype=np.int32), KF_FEAT); cat_feat = np.tile(np.arange(KF_FEAT, dtype=np.int32), 40)
    index = np.full(16384, -1, np.int32)
    normals = np.tile([0.0, 0.0, 1.0], (len(slots), 1))
    d_normals = torch.from_numpy(normals).cuda()
    desc_now = desc.copy()

    def lists_host():
        return host_lists(cat_slot, cat_kf, cat_feat, live, index, slots)

    def lists_device():
        o = h.map_observations_device(mp, kfs, slots)
        h.synchronize()
        return o

    def refresh_resident():
        return h.map_refresh_points(mp, kfs, slots, SCALE_RANGE, normals)

    def refresh_resident_device():
        o = h.map_refresh_points_device(mp, kfs, slots, SCALE_RANGE, d_normals)
        h.synchronize()
        return o

    def parent_refresh(l):
        r = P.KeyFrame.refresh_map_points(h, kfs, pos[slots], l[0], l[1], l[2], SCALE_RANGE, desc_now[slots], normals)
        mp.set(slots, descriptors=r.mp_desc)
        return r

    def parent_sequence():
        return parent_refresh(lists_host())

    for _ in range(a.warmup):
        lists_device(); refresh_resident(); refresh_resident_device(); parent_sequence()
    l0 = lists_host()
    ld = lists_device()
    N = int(l0[0][-1])
    same_lists = all(x.cpu().numpy()[:len(y)].tobytes() == y.tobytes() for x, y in zip((ld["obs_start"], ld["obs_kf"], ld["obs_feat"]), l0))
    mp.set(slots, descriptors=desc[slots])
    par = parent_refresh(l0)
    mp.set(slots, descriptors=desc[slots])
    res = refresh_resident()
    same_refresh = all(getattr(res, k).tobytes() == getattr(par, k).tobytes() for k in ("mp_desc", "normals", "min_distance", "max_distance", "records"))
    desc_now[slots] = res.mp_desc
    forms = (("lists_device", lists_device), ("host_lists", lists_host), ("refresh_resident", refresh_resident), ("refresh_resident_device", refresh_resident_device),
             ("parent_refresh_and_set", lambda: parent_refresh(l0)), ("parent_sequence", parent_sequence))
    steps, t = measure(forms, a.rounds, a.round_seconds)
    row = dict(keyframes=40, keyframe_features=KF_FEAT, points=len(slots), observations=N, lists_equal_to_host=bool(same_lists),
               refresh_equal_to_parent_sequence=bool(same_refresh), calls_per_round=steps, **{k + "_ms": v for k, v in t.items()},
               refresh_ranges_overlap=overlap(t["refresh_resident"], t["parent_sequence"]),
               refresh_vs_parent_without_lists_ranges_overlap=overlap(t["refresh_resident"], t["parent_refresh_and_set"]),
               lists_ranges_overlap=overlap(t["lists_device"], t["host_lists"]),
               lists_kernel_us_per_call=kernel_us(h, lists_device, steps["lists_device"]),
               refresh_kernel_us_per_call=kernel_us(h, refresh_resident_device, steps["refresh_resident_device"]))
    out["refresh"].append(row)
    print(json.dumps(row), flush=True)
    h.synchronize()
    for k in kfs:
        k.close()
    mp.close()
    # ---- (c): redundancy of 20 candidates among N keyframes
    rng = np.random.default_rng(12)
    mp, all_kfs, tables, live, slots, pos, desc = world(h, rng, 65536, 50000, 1000, 1500, pool=6000)
    uq = [uniq_table(t) for t in tables]
    for n_kfs in (100, 1000):
        kfs = all_kfs[:n_kfs]
        cand = (np.arange(20, dtype=np.int32) * (n_kfs // 20)).astype(np.int32)
        cat_u = np.concatenate(uq[:n_kfs])

        def redundancy_numpy():
            s = cat_u[cat_u >= 0]
            n = np.bincount(s[live[s] == 1], minlength=len(live))
            tot, red = [], []
            for c in cand:
                tc = tables[c][tables[c] >= 0]
                tc = tc[live[tc] == 1]
                tot.append(len(tc)); red.append(int((n[tc] - 1 >= 3).sum()))
            tot = np.array(tot, np.int32); red = np.array(red, np.int32)
            return tot, red, ((tot > 0) & (red.astype(np.float64) / np.maximum(tot, 1) > 0.9)).astype(np.uint8)

        def redundancy_resident():
            return h.map_keyframe_redundancy(mp, kfs, cand, 3, 0.9)

        def redundancy_device():
            o = h.map_keyframe_redundancy_device(mp, kfs, cand, 3, 0.9)
            h.synchronize()
            return o

        for _ in range(a.warmup):
            redundancy_resident(); redundancy_device(); redundancy_numpy()
        same = all(x.tobytes() == y.tobytes() for x, y in zip(redundancy_resident(), redundancy_numpy()))
        forms = (("redundancy_resident", redundancy_resident), ("redundancy_device", redundancy_device), ("redundancy_numpy", redundancy_numpy))
        steps, t = measure(forms, a.rounds, a.round_seconds)
        tot, red, cull = redundancy_resident()
        row = dict(resident_keyframes=n_kfs, candidates=len(cand), keyframe_features=KF_FEAT, live_points=50000, equal_to_numpy=bool(same),
                   total=tot.tolist(), redundant=red.tolist(), culled=int(cull.sum()), calls_per_round=steps, **{k + "_ms": v for k, v in t.items()},
                   ranges_overlap=overlap(t["redundancy_resident"], t["redundancy_numpy"]),
                   kernel_us_per_call=kernel_us(h, redundancy_device, steps["redundancy_device"]))
        out["redundancy"].append(row)
        print(json.dumps(row), flush=True)
    h.synchronize()
    for k in all_kfs:
        k.close()
    mp.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "map_observations_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
