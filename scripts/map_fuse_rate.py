#!/usr/bin/env python3
"""Host time of Handle.map_search_in_neighbors (fuse and merge on the resident map: both passes, one download, the erase, the
refresh) against the same run's sequence a caller makes today.

  resident   Handle.map_search_in_neighbors: whole host call with its synchronisation.
  today      per pass: the selection downloaded (Handle.map_select_points_device and a copy to the host), KeyFrame.fuse_search on the
             list, the resolve of the specification on host copies of every table (tests/map_fuse_spec.py: numpy and plain Python),
             KeyFrame.set_map_point_slots per changed keyframe, MapPointStore.erase; then Handle.map_refresh_points on the affected
             list.  The resolve is interpreted Python: it bounds from above what a compiled shim pays for it; it is reported apart
             (today_without_resolve subtracts it call by call).

The world: N = 100 resident keyframes of 2000 features with nearly the same pose, a store of 50 000 live points in front of them;
the current keyframe shares 600 landmarks with each of its 20 neighbours — a third under the same slot (skipped as observed), a
third unassociated in the neighbour (associations), a third under another slot (merges).  Every call starts from the same world:
the tables and the erased slots are put back outside the timed region.  The forms alternate, --rounds rounds of at least
--round-seconds each; per form the median and the spread (min, max), plus the device time per kernel (orbx_get_kernel_times).
usage: python scripts/map_fuse_rate.py [--rounds R] [--round-seconds S] [--out FILE.json]"""
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

import map_fuse_spec as S  # noqa: E402
import orb_slam3_rust_amd as P  # noqa: E402

RADIUS_SCALE = 3.0 * (1.2 * (1.2 * 1.2) * ((1.2 * 1.2) * (1.2 * 1.2)))
SCALE_RANGE = 1.2 ** 7
CAPACITY, N_LIVE, N_KFS, KF_FEAT, N_NB, SHARED = 65536, 50000, 100, 2000, 20, 600


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def project(cam, pose, X):
    a = 2.0 * np.arctan2(pose[2], pose[0])
    c, s = np.cos(a), np.sin(a)
    d = X - pose[4:]
    x, z = c * d[:, 0] - s * d[:, 2], s * d[:, 0] + c * d[:, 2]             # R(y, a)^T d
    return np.stack([cam["fx"] * x / z + cam["cx"], cam["fy"] * d[:, 1] / z + cam["cy"]], 1)


def flip(rng, d, k):
    out = d.copy()
    rows = np.arange(len(d))
    for _ in range(k):
        b = rng.integers(0, 256, len(d))
        out[rows, b >> 3] ^= (1 << (b & 7)).astype(np.uint8)
    return out


def build(h, rng, cam):
    """-> (store, keyframes, tables, live slots, slot normals)"""
    n_lm = N_LIVE
    X = np.stack([rng.uniform(-1.8, 1.8, n_lm), rng.uniform(-1.0, 1.0, n_lm), rng.uniform(5.0, 9.0, n_lm)], 1)
    D = rng.integers(0, 256, (n_lm, 32), dtype=np.uint8)
    slots = np.sort(rng.permutation(CAPACITY)[:N_LIVE]).astype(np.int32)    # landmark i's first slot is slots[i]
    pos = np.zeros((CAPACITY, 3)); desc = np.zeros((CAPACITY, 32), np.uint8)
    pos[slots] = X; desc[slots] = flip(rng, D, 3)
    # duplicates: landmarks [0, 2000) are the current keyframe's; a neighbour's merge candidates name a second slot of the landmark
    spare = np.setdiff1d(np.arange(CAPACITY), slots)[:2000].astype(np.int32)
    pos[spare] = X[:2000]; desc[spare] = flip(rng, D[:2000], 3)
    live_slots = np.concatenate([slots, spare])
    mp = P.MapPointStore(h, CAPACITY)
    mp.set(live_slots, pos[live_slots], desc[live_slots])
    kfs, tables = [], []
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for k in range(N_KFS):
        a = rng.uniform(-0.02, 0.02)
        pose = np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0] + list(rng.uniform(-0.3, 0.3, 3)))
        if k == 0:
            lm = np.arange(KF_FEAT); t = slots[lm].copy(); t[1500:] = -1
        else:
            own = 2000 + rng.permutation(n_lm - 2000)[:KF_FEAT - SHARED]
            sh = rng.permutation(2000)[:SHARED]                            # (the last 500 are unassociated in the current keyframe: the pass back)
            lm = np.concatenate([sh, own])
            t = slots[lm].copy()
            if 1 <= k <= N_NB:
                t[SHARED // 3:2 * SHARED // 3] = -1
                t[2 * SHARED // 3:SHARED] = spare[sh[2 * SHARED // 3:]]
        order = rng.permutation(KF_FEAT)
        lm, t = lm[order], t[order]
        kp = np.zeros(KF_FEAT, P.KEYPOINT)
        uv = project(cam, pose, X[lm]) + rng.uniform(-0.4, 0.4, (KF_FEAT, 2))
        kp["x"] = uv[:, 0]; kp["y"] = uv[:, 1]; kp["size"] = 31.0
        kf = P.KeyFrame(h, d(kp.view(np.uint8).reshape(-1, kp.dtype.itemsize)), d(flip(rng, D[lm], 3)), KF_FEAT, pose_wc=pose)
        kf.set_map_point_slots(mp, t)
        kfs.append(kf); tables.append(t.astype(np.int32))
    return mp, kfs, tables, live_slots, pos, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_fuse_rate.py measures on the GPU; none is visible")
    camd = P.synth.EUROC_CAMERA
    cam = P.CameraModel(**camd)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    rng = np.random.default_rng(21)
    mp, kfs, tables, live_slots, pos, desc = build(h, rng, camd)
    live = np.zeros(CAPACITY, np.uint8); live[live_slots] = 1
    nb = list(range(1, 1 + N_NB))
    normals = np.tile([0.0, 0.0, 1.0], (CAPACITY, 1))
    touched = [0] + nb

    def restore(goners):
        if len(goners):
            mp.set(goners, pos[goners], desc[goners])
        mp.set(live_slots, descriptors=desc[live_slots])
        for k in range(N_KFS):
            kfs[k].set_map_point_slots(mp, tables[k])
        h.synchronize()

    def resident():
        return h.map_search_in_neighbors(cam, mp, kfs, 0, nb, RADIUS_SCALE, SCALE_RANGE, slot_normals=normals)

    resolve_s = [0.0]

    def today():
        resolve_s[0] = 0.0
        tabs = S.Tables([t.copy() for t in tables], [KF_FEAT] * N_KFS)
        lv = live
        gone = []
        for src, tgt in (([0], nb), (nb, [0])):
            o = h.map_select_points_device(mp, keyframes=[[kfs[i] for i in src]])
            n = int(o["list_offsets"][-1].item())
            L = o["list_slot"][:n].cpu().numpy(); lp = o["positions"][:n].cpu().numpy(); ld = o["mp_desc"][:n].cpu().numpy()
            idx, _ = P.KeyFrame.fuse_search(h, cam, lp, ld, [kfs[t] for t in tgt], RADIUS_SCALE, 50)
            t0 = time.perf_counter()
            r = S.fuse(tabs, lv, pos, desc, src, tgt, lambda p_, d_, tg: idx)
            resolve_s[0] += time.perf_counter() - t0
            assert r["list_slot"].tobytes() == L.tobytes()
            for k in range(N_KFS):
                if r["tables"][k].tobytes() != tabs[k].tobytes():
                    kfs[k].set_map_point_slots(mp, r["tables"][k])
            tabs = S.Tables(r["tables"], [KF_FEAT] * N_KFS)
            gone.append(r["goner"])
        g = np.concatenate(gone)
        if len(g):
            mp.erase(g)
        o = h.map_select_points_device(mp, keyframes=[[kfs[i] for i in touched]])
        aff = o["list_slot"][:int(o["list_offsets"][-1].item())].cpu().numpy()
        return g, aff, h.map_refresh_points(mp, kfs, aff, SCALE_RANGE, normals[aff]), tabs

    # once each: the same result
    r = resident()
    res_tables = [k.get_map_point_slots() for k in kfs]
    g_res = np.concatenate([r["goner_a"], r["goner_b"]])
    restore(g_res)
    g, aff, ref, tabs = today()
    same = (np.array_equal(np.sort(g), np.sort(g_res)) and aff.tobytes() == r["affected"].tobytes() and ref.mp_desc.tobytes() == r["refresh"].mp_desc.tobytes() and
            all(a_.tobytes() == b_.tobytes() for a_, b_ in zip(res_tables, tabs)))
    restore(g)
    times = dict(resident=[], today=[], today_without_resolve=[])
    calls = {}
    for rnd in range(a.rounds):
        for name in ("resident", "today"):
            tot, tot_nr, n = 0.0, 0.0, 0
            while tot < a.round_seconds or n < 3:
                t0 = time.perf_counter()
                out = resident() if name == "resident" else today()
                dt = time.perf_counter() - t0
                tot += dt; n += 1
                if name == "today":
                    tot_nr += dt - resolve_s[0]
                restore(np.concatenate([out["goner_a"], out["goner_b"]]) if name == "resident" else out[0])
            times[name].append(tot / n * 1e3)
            if name == "today":
                times["today_without_resolve"].append(tot_nr / n * 1e3)
            calls[name] = n
    t = {k: stat(v) for k, v in times.items()}
    h.set_profiling(True)
    h.kernel_times()
    out = resident()
    kt = {k: v[0] * 1e3 for k, v in h.kernel_times().items()}
    h.set_profiling(False)
    apart = lambda x, y: x["max"] < y["min"] or y["max"] < x["min"]
    row = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, resident_keyframes=N_KFS, neighbours=N_NB,
               keyframe_features=KF_FEAT, live_points=len(live_slots), counts=r["counts"].tolist(), affected=len(r["affected"]),
               equal_to_todays_sequence=bool(same), calls_per_round=calls, **{k + "_ms": v for k, v in t.items()},
               ranges_apart=bool(apart(t["resident"], t["today"])), ranges_apart_without_resolve=bool(apart(t["resident"], t["today_without_resolve"])),
               kernel_us_per_call=kt,
               note="today's resolve is tests/map_fuse_spec.py, interpreted Python over host copies of the tables: an upper bound on what a compiled shim pays; "
                    "today_without_resolve leaves it out and so bounds the shim's sequence from below")
    print(json.dumps(row), flush=True)
    h.synchronize()
    for k in kfs:
        k.close()
    mp.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "map_fuse_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(row, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
