#!/usr/bin/env python3
"""Host time of Handle.map_correct_loop (the rigid loop correction and the loop closer's fuse on the resident map) against the same
run's sequence a caller makes today, at N = 100 and N = 1000 resident keyframes.

  resident   Handle.map_correct_loop: whole host call with its synchronisation.
  today      Handle.map_covisibility for all keyframes (the N x N weights come down); the walk over them in numpy; every table
             read back (KeyFrame.get_map_point_slots); the affected list in numpy; MapPointStore.download of it (which brings the
             whole store down: the only download there is); the correction in numpy; MapPointStore.set of the positions; the fuse
             in numpy over the host tables; KeyFrame.set_map_point_slots per changed keyframe; KeyFrame.set_pose; MapPointStore.erase.
             The numpy parts (walk, list, correction, fuse) are timed apart: they bound from above what a compiled shim pays for
             them, and today_without_numpy leaves them out, which bounds the shim's sequence from below.

The world: N keyframes of 2000 features whose tables walk along a band of a store of 50 000 live points, so that neighbours in the
trajectory share most of their points; a spanning chain; the last keyframe closes a loop on the first with 300 matched features.
Every call starts from the same world: positions, tables, poses and erased slots are put back outside the timed region.  The forms
alternate, --rounds rounds of at least --round-seconds each; per form the median and the spread (min, max), plus the device time per
kernel (orbx_get_kernel_times).
usage: python scripts/loop_correct_rate.py [--rounds R] [--round-seconds S] [--sizes 100,1000] [--out FILE.json]"""
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

import loop_correct_spec as S  # noqa: E402
import orb_slam3_rust_amd as P  # noqa: E402

CAPACITY, N_LIVE, KF_FEAT, WINDOW, N_MATCH = 65536, 50000, 2000, 3000, 300
SIM3 = np.array([np.cos(0.02), 0.0, np.sin(0.02), 0.0, 0.4, -0.05, 0.3, 1.0])


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def build(h, rng, N):
    slots = np.sort(rng.permutation(CAPACITY)[:N_LIVE]).astype(np.int32)
    pos = np.zeros((CAPACITY, 3)); desc = np.zeros((CAPACITY, 32), np.uint8)
    pos[slots] = rng.uniform(-30, 30, (N_LIVE, 3)); desc[slots] = rng.integers(0, 256, (N_LIVE, 32), dtype=np.uint8)
    mp = P.MapPointStore(h, CAPACITY)
    mp.set(slots, pos[slots], desc[slots])
    kfs, tables, poses = [], [], []
    z_kp = torch.zeros((KF_FEAT, 7), dtype=torch.float32, device="cuda"); z_d = torch.zeros((KF_FEAT, 32), dtype=torch.uint8, device="cuda")
    for k in range(N):
        start = int(k * (N_LIVE - WINDOW) / max(N - 1, 1))
        t = slots[start + rng.permutation(WINDOW)[:KF_FEAT]].copy()
        t[rng.random(KF_FEAT) < 0.05] = -1
        a = rng.uniform(-3, 3)
        pose = np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0] + list(rng.uniform(-30, 30, 3)))
        kf = P.KeyFrame(h, z_kp, z_d, KF_FEAT, pose_wc=pose)
        kf.set_map_point_slots(mp, t)
        kfs.append(kf); tables.append(t.astype(np.int32)); poses.append(pose)
    fc = np.flatnonzero(tables[N - 1] >= 0)[:N_MATCH]; fl = np.flatnonzero(tables[0] >= 0)[:N_MATCH]
    return mp, kfs, tables, np.array(poses), slots, pos, desc, np.stack([fc, fl], 1).astype(np.int32)


def walk(w, parent, cur, min_weight, max_depth):
    """the reach over a downloaded weight table, level by level"""
    N = len(w)
    level = np.full(N, -1); level[cur] = 0
    front = np.array([cur])
    for d in range(max_depth):
        if not len(front):
            break
        hit = (w[front] >= min_weight).any(0) | ((parent >= 0) & (level[np.maximum(parent, 0)] == d))
        front = np.flatnonzero(hit & (level < 0))
        level[front] = d + 1
    return level >= 0


def first_seen(tables, aff, live):
    cat = np.concatenate([tables[k] for k in np.flatnonzero(aff)])
    cat = cat[(cat >= 0) & (cat < len(live))]
    cat = cat[live[cat] == 1]
    _, idx = np.unique(cat, return_index=True)
    return cat[np.sort(idx)].astype(np.int32)


def host_fuse(tables, live, cur, loop, matches):
    """-> (changed keyframes {k: new table}, goner, keeper): loop_correct_spec.fuse with the counting and the rewrite in numpy"""
    pr = S.pairs(tables, live, cur, loop, matches)
    nobs = np.zeros(len(live), np.int64)
    for t in tables:
        u = np.unique(t[t >= 0])
        nobs[u[live[u] == 1]] += 1
    goner, keeper = _classes(pr, nobs)
    lut = np.arange(len(live), dtype=np.int32); lut[goner] = keeper
    changed = {}
    for k, t in enumerate(tables):
        n = np.where(t >= 0, lut[np.maximum(t, 0)], t)
        if n.tobytes() != t.tobytes():
            changed[k] = n
    return changed, goner, keeper


def _classes(pr, nobs):
    flat = [int(s) for s in pr.reshape(-1).tolist() if s >= 0]
    first = {}
    for i, s in enumerate(flat):
        first.setdefault(s, i)
    root = {s: s for s in first}

    def find(s):
        while root[s] != s:
            root[s] = root[root[s]]; s = root[s]
        return s
    for a, b in pr.tolist():
        if a >= 0:
            root[find(a)] = find(b)
    classes = {}
    for s in first:
        classes.setdefault(find(s), []).append(s)
    to = {}
    for members in classes.values():
        keep = min(members, key=lambda s: (-int(nobs[s]), first[s]))
        to.update({s: keep for s in members if s != keep})
    goner = np.array(sorted(to), np.int32)
    return goner, np.array([to[int(g)] for g in goner], np.int32)


def measure(h, N, a):
    rng = np.random.default_rng(5)
    mp, kfs, tables, poses, live_slots, pos, desc, matches = build(h, rng, N)
    live = np.zeros(CAPACITY, np.uint8); live[live_slots] = 1
    parent = np.arange(-1, N - 1, dtype=np.int32)
    cur, loop = N - 1, 0
    cfg = P.LoopCorrectConfig()
    numpy_s = [0.0]

    def restore(lst, goners, changed):
        if len(goners):
            mp.set(goners, pos[goners], desc[goners])
        if len(lst):
            mp.set(lst, pos[lst])
        for k in changed:
            kfs[k].set_map_point_slots(mp, tables[k])
        for k in range(N):
            kfs[k].set_pose(poses[k])
        h.synchronize()

    def resident():
        return h.map_correct_loop(mp, kfs, parent, cur, loop, SIM3, matches, cfg)

    def today():
        numpy_s[0] = 0.0
        w = h.map_covisibility(mp, kfs, range(N))[0]
        t0 = time.perf_counter()
        aff = walk(w, parent, cur, cfg.min_covisibility_weight, cfg.max_propagation_depth)
        numpy_s[0] += time.perf_counter() - t0
        tabs = [k.get_map_point_slots() for k in kfs]
        t0 = time.perf_counter()
        lst = first_seen(tabs, aff, live)
        numpy_s[0] += time.perf_counter() - t0
        p = mp.download(lst)[0]
        t0 = time.perf_counter()
        p = S.correct_points(SIM3, p)
        new_poses = [S.correct_pose(SIM3, poses[k]) for k in np.flatnonzero(aff)]
        changed, goner, keeper = host_fuse(tabs, live, cur, loop, matches)
        numpy_s[0] += time.perf_counter() - t0
        mp.set(lst, p)
        for k, t in changed.items():
            kfs[k].set_map_point_slots(mp, t)
        for k, q in zip(np.flatnonzero(aff), new_poses):
            kfs[k].set_pose(q)
        if len(goner):
            mp.erase(goner)
        h.synchronize()
        return dict(affected=aff.astype(np.uint8), list_slot=lst, goner=goner, keeper=keeper, changed=changed)

    # once each: the same result
    r = resident()
    res_tables = [k.get_map_point_slots() for k in kfs]
    res_pos = mp.download(r["list_slot"])[0]
    changed_res = [k for k in range(N) if res_tables[k].tobytes() != tables[k].tobytes()]
    restore(r["list_slot"], r["goner"], changed_res)
    t = today()
    td_tables = [k.get_map_point_slots() for k in kfs]
    td_pos = mp.download(t["list_slot"])[0]
    same = (all(r[k].tobytes() == t[k].tobytes() for k in ("affected", "list_slot", "goner", "keeper")) and
            all(x.tobytes() == y.tobytes() for x, y in zip(res_tables, td_tables)) and
            bool(np.all(np.abs(res_pos - td_pos) <= S.tolerance(SIM3, pos[r["list_slot"]])[:, None])))
    restore(t["list_slot"], t["goner"], t["changed"])
    times = dict(resident=[], today=[], today_without_numpy=[], numpy=[])
    calls = {}
    for rnd in range(a.rounds):
        for name in ("resident", "today"):
            tot, tot_np, n = 0.0, 0.0, 0
            while tot < a.round_seconds or n < 3:
                t0 = time.perf_counter()
                out = resident() if name == "resident" else today()
                dt = time.perf_counter() - t0
                tot += dt; n += 1
                if name == "today":
                    tot_np += numpy_s[0]
                restore(out["list_slot"], out["goner"], changed_res)
            times[name].append(tot / n * 1e3)
            if name == "today":
                times["today_without_numpy"].append((tot - tot_np) / n * 1e3); times["numpy"].append(tot_np / n * 1e3)
            calls[name] = n
    tm = {k: stat(v) for k, v in times.items()}
    h.set_profiling(True)
    h.kernel_times()
    out = resident()
    kt = {k: v[0] * 1e3 for k, v in h.kernel_times().items()}
    h.set_profiling(False)
    apart = lambda x, y: x["max"] < y["min"] or y["max"] < x["min"]
    row = dict(resident_keyframes=N, keyframe_features=KF_FEAT, live_points=len(live_slots), matches=len(matches), counts=r["counts"].tolist(),
               changed_keyframes=len(changed_res), equal_to_todays_sequence=bool(same), calls_per_round=calls, **{k + "_ms": v for k, v in tm.items()},
               ranges_apart=bool(apart(tm["resident"], tm["today"])), ranges_apart_without_numpy=bool(apart(tm["resident"], tm["today_without_numpy"])),
               kernel_us_per_call=kt)
    h.synchronize()
    for k in kfs:
        k.close()
    mp.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--sizes", default="100,1000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loop_correct_rate.py measures on the GPU; none is visible")
    h = P.Handle(P.CameraModel(**P.synth.EUROC_CAMERA), 2000, device=0, max_w=752, max_h=480, max_batch=1)
    rows = []
    for N in (int(x) for x in a.sizes.split(",")):
        rows.append(measure(h, N, a))
        print(json.dumps(rows[-1]), flush=True)
    h.close()
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, sizes=rows,
               note="today's numpy parts (the walk, the affected list, the correction, the fuse) are interpreted Python and numpy over host copies: an upper bound on "
                    "what a compiled shim pays; today_without_numpy leaves them out and so bounds the shim's sequence from below.  MapPointStore.download brings "
                    "the whole store down whatever the list: the only download of positions there is")
    path = a.out or os.path.join(ROOT, "profiles", "loop_correct_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
