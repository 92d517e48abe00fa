#!/usr/bin/env python3
"""Host time of Handle.map_create_points and Handle.map_cull_points (steps 3, 3b and 5 of process_keyframe on the resident map)
against the same run's sequence a caller makes today.

  create, resident   Handle.map_create_points: whole host call with its synchronisation (both phases, one download, set_device).
  create, today      KeyFrame.triangulate_from_neighbors; the stereo points in numpy; MapPointStore.set; orbx_keyframe_get / set_map_point_slots
                     per changed keyframe; orbx_keyframe_set_map_points for the flags.  The per-keyframe table and flag calls go through the
                     C ABI with ready int32 / int64 arrays, as a compiled shim would make them: no per-element Python.  The numpy parts
                     (stereo points, the table edits, the ids from the tables) are reported apart: today_without_numpy subtracts them and
                     is what the sequence's library calls cost, with ctypes' call overhead.
  cull, resident     Handle.map_cull_points on 12 000 candidates over all resident keyframes.
  cull, today        Handle.map_observations + the comparison on the host + MapPointStore.erase + orbx_keyframe_get_map_point_slots of
                     every keyframe (the tables live on the device) and orbx_keyframe_set_map_point_slots of the changed ones, the same way.

The world: tests/triangulation_scenes.py's current keyframe of about 2000 features with 10 neighbours, among 100 resident keyframes,
and a store of 50 000 live points.  Every call starts from the same world: tables, flags and store are put back outside the timed
region.  The forms alternate, --rounds rounds of at least --round-seconds each; per form the median and the spread (min, max), plus
the device time per kernel (orbx_get_kernel_times).
usage: python scripts/map_create_rate.py [--rounds R] [--round-seconds S] [--out FILE.json]"""
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
import triangulation_scenes as G  # noqa: E402
import triangulation_spec as TS  # noqa: E402

CAPACITY, N_LIVE, N_KFS, KF_FEAT, N_NB, N_CAND, MIN_OBS, N_FREE = 65536, 50000, 100, 2000, 10, 12000, 3, 4000


def stat(t):
    return dict(median=statistics.median(t), min=min(t), max=max(t))


def build(h, rng):
    """-> (store, keyframes [N_KFS] (0: current, 1..N_NB: its neighbours), host tables, host keyframe dicts, live slots, rows)"""
    sc = G.make_scene(seed=31, n_points=1700, T=N_NB, n_distract=297)
    live_slots = np.sort(rng.permutation(CAPACITY)[:N_LIVE]).astype(np.int32)
    pos = np.zeros((CAPACITY, 3)); desc = np.zeros((CAPACITY, 32), np.uint8)
    pos[live_slots] = rng.uniform(-5.0, 5.0, (N_LIVE, 3)); desc[live_slots] = rng.integers(0, 256, (N_LIVE, 32), dtype=np.uint8)
    mp = P.MapPointStore(h, CAPACITY)
    mp.set(live_slots, pos[live_slots], desc[live_slots])
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    kp_t = lambda kp: d(np.ascontiguousarray(kp).view(np.float32).reshape(-1, 7).copy())
    kfs, tables, dicts = [], [], []
    for k, kf in enumerate([sc["current"]] + list(sc["neighbours"])):
        n = len(kf["kp"])
        t = np.full(n, -1, np.int32)
        on = np.flatnonzero(kf["mp"])
        t[on] = rng.choice(live_slots, len(on), replace=False)
        x = P.KeyFrame(h, kp_t(kf["kp"]), d(kf["desc"]), n, d(kf["pts"]), d(kf["has"]), keyframe_id=k, pose_wc=kf["pose"])
        x.set_map_point_slots(mp, t)
        x.set_map_points([7 if m else None for m in kf["mp"]])
        kfs.append(x); tables.append(t); dicts.append(kf)
    for k in range(1 + N_NB, N_KFS):                                        # the other resident keyframes: tables only matter
        t = rng.choice(live_slots, KF_FEAT).astype(np.int32)
        t[rng.random(KF_FEAT) < 0.3] = -1
        x = P.KeyFrame(h, torch.zeros((KF_FEAT, 7), dtype=torch.float32, device="cuda"), torch.zeros((KF_FEAT, 32), dtype=torch.uint8, device="cuda"), KF_FEAT,
                       keyframe_id=k)
        x.set_map_point_slots(mp, t)
        kfs.append(x); tables.append(t); dicts.append(None)
    return sc, mp, kfs, tables, dicts, live_slots, pos, desc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_create_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**G.CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    rng = np.random.default_rng(33)
    sc, mp, kfs, tables, dicts, live_slots, pos, desc = build(h, rng)
    live = np.zeros(CAPACITY, np.uint8); live[live_slots] = 1
    free = rng.permutation(np.flatnonzero(live == 0))[:N_FREE].astype(np.int32)
    cur, nbs = kfs[0], kfs[1:1 + N_NB]
    cd = dicts[0]
    near = list(range(1 + N_NB))
    R = TS.rotation_matrix(cd["pose"][:4])
    numpy_s = [0.0]
    # the per-keyframe calls of today's sequence as a compiled shim makes them: the C ABI on ready arrays
    L = h._L
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ids_of = lambda tab: np.where(tab >= 0, 7, -1).astype(np.int64)
    ids0 = [ids_of(t) for t in tables]
    bufs = [np.empty(max(k.n, 1), np.int32) for k in kfs]

    def set_slots(k, tab):
        h._check(L.orbx_keyframe_set_map_point_slots(kfs[k]._p, mp._p, vp(tab)))

    def get_slots(k):
        h._check(L.orbx_keyframe_get_map_point_slots(kfs[k]._p, vp(bufs[k])))
        return bufs[k][:kfs[k].n]

    def set_ids(k, ids):
        h._check(L.orbx_keyframe_set_map_points(kfs[k]._p, vp(ids)))

    def restore_create(new_slots):
        if len(new_slots):
            mp.erase(new_slots)
        for k in near:
            set_slots(k, tables[k])
            set_ids(k, ids0[k])
        h.synchronize()

    def create_resident():
        return h.map_create_points(cam, mp, cur, nbs, free)

    def create_today():
        numpy_s[0] = 0.0
        t0 = time.perf_counter()
        tabs = {0: tables[0].copy()}
        cand = np.flatnonzero((cd["has"] != 0) & (tabs[0] < 0))
        S = len(cand)
        sp = cd["pts"][cand] @ R.T + cd["pose"][4:]
        tabs[0][cand] = free[:S]
        flags0 = ids_of(tabs[0])
        numpy_s[0] += time.perf_counter() - t0
        set_ids(0, flags0)                                                  # the neighbour phase sees the stereo points
        nb, i1, i2, pts, _ = cur.triangulate_from_neighbors(cam, nbs)
        t0 = time.perf_counter()
        N = len(nb)
        slots = free[:S + N]
        for e in range(N):
            t = 1 + int(nb[e])
            if t not in tabs:
                tabs[t] = None
        numpy_s[0] += time.perf_counter() - t0
        for t in tabs:                                                      # the tables live on the device: read, edit, write
            if tabs[t] is None:
                tabs[t] = get_slots(t)
        t0 = time.perf_counter()
        for e in range(N):
            tabs[1 + int(nb[e])][i2[e]] = slots[S + e]
            tabs[0][i1[e]] = slots[S + e]
        new_pos = np.concatenate([sp, pts]); new_desc = np.concatenate([cd["desc"][cand], cd["desc"][i1]])
        ids = {t: ids_of(tab) for t, tab in tabs.items()}
        keep = {t: tab.copy() for t, tab in tabs.items()}                   # (the read buffers are reused by the next call)
        numpy_s[0] += time.perf_counter() - t0
        mp.set(slots, new_pos, new_desc)
        for t, tab in tabs.items():
            set_slots(t, tab)
            set_ids(t, ids[t])
        return slots, new_pos, keep

    # once each: the same result
    r = create_resident()
    res_tables = [kfs[k].get_map_point_slots() for k in near]
    res_rows = mp.download(r["new_slot"])
    restore_create(r["new_slot"])
    slots, new_pos, tabs = create_today()
    same_create = (slots.tobytes() == r["new_slot"].tobytes() and all(res_tables[k].tobytes() == (tabs[k] if k in tabs else tables[k]).tobytes() for k in near) and
                   res_rows[1].tobytes() == mp.download(slots)[1].tobytes() and bool(np.allclose(res_rows[0], mp.download(slots)[0], rtol=1e-12, atol=0.0)))
    restore_create(slots)

    # ---- cull: candidates among the live points; observers over all resident keyframes
    cand = rng.permutation(live_slots)[:N_CAND].astype(np.int32)

    def restore_cull(culled):
        if len(culled):
            mp.set(culled, pos[culled], desc[culled])
        for k in range(N_KFS):
            set_slots(k, tables[k])
        h.synchronize()

    def cull_resident():
        return h.map_cull_points(mp, kfs, cand, MIN_OBS)

    def cull_today():
        numpy_s[0] = 0.0
        start, _, _ = h.map_observations(mp, kfs, cand)
        t0 = time.perf_counter()
        culled = cand[np.diff(start) < MIN_OBS]
        numpy_s[0] += time.perf_counter() - t0
        mp.erase(culled)
        out = []
        for k in range(N_KFS):
            t = get_slots(k)
            t0 = time.perf_counter()
            hit = np.isin(t, culled)
            changed = bool(hit.any())
            if changed:
                t[hit] = -1
            numpy_s[0] += time.perf_counter() - t0
            if changed:
                set_slots(k, t)
            out.append(t)
        return culled, out

    c_res = cull_resident()
    c_tables = [k.get_map_point_slots() for k in kfs]
    restore_cull(c_res)
    c_today, t_today = cull_today()
    same_cull = c_res.tobytes() == c_today.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(c_tables, t_today))
    restore_cull(c_today)

    forms = dict(create_resident=(create_resident, lambda o: restore_create(o["new_slot"])), create_today=(create_today, lambda o: restore_create(o[0])),
                 cull_resident=(cull_resident, restore_cull), cull_today=(cull_today, lambda o: restore_cull(o[0])))
    times = {k: [] for k in list(forms) + ["create_today_without_numpy", "cull_today_without_numpy"]}
    calls = {}
    for rnd in range(a.rounds):
        for name, (run, restore) in forms.items():
            tot, tot_nn, n = 0.0, 0.0, 0
            while tot < a.round_seconds or n < 3:
                t0 = time.perf_counter()
                out = run()
                dt = time.perf_counter() - t0
                tot += dt; n += 1
                if name.endswith("today"):
                    tot_nn += dt - numpy_s[0]
                restore(out)
            times[name].append(tot / n * 1e3)
            if name.endswith("today"):
                times[name + "_without_numpy"].append(tot_nn / n * 1e3)
            calls[name] = n
    t = {k: stat(v) for k, v in times.items()}
    h.set_profiling(True)
    h.kernel_times()
    o = create_resident()
    kt_create = {k: v[0] * 1e3 for k, v in h.kernel_times().items()}
    restore_create(o["new_slot"])
    h.kernel_times()
    o = cull_resident()
    kt_cull = {k: v[0] * 1e3 for k, v in h.kernel_times().items()}
    restore_cull(o)
    h.set_profiling(False)
    new_us = lambda kt: sum(v for k, v in kt.items() if k.startswith(("mc_", "mr_")))
    apart = lambda x, y: x["max"] < y["min"] or y["max"] < x["min"]
    row = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, resident_keyframes=N_KFS, neighbours=N_NB,
               current_features=int(cur.n), live_points=int(N_LIVE), create_counts=r["counts"].tolist(), cull_candidates=N_CAND, culled=int(len(c_res)),
               min_observations=MIN_OBS, create_equal_to_todays_sequence=bool(same_create), cull_equal_to_todays_sequence=bool(same_cull), calls_per_round=calls,
               **{k + "_ms": v for k, v in t.items()},
               create_ranges_apart=bool(apart(t["create_resident"], t["create_today"])),
               create_ranges_apart_without_numpy=bool(apart(t["create_resident"], t["create_today_without_numpy"])),
               cull_ranges_apart=bool(apart(t["cull_resident"], t["cull_today"])),
               cull_ranges_apart_without_numpy=bool(apart(t["cull_resident"], t["cull_today_without_numpy"])),
               create_kernel_us_per_call=kt_create, cull_kernel_us_per_call=kt_cull,
               create_new_kernels_us=new_us(kt_create), create_triangulation_launches_us=sum(v for k, v in kt_create.items() if k.startswith("tri_")),
               cull_new_kernels_us=new_us(kt_cull),
               note="today's per-keyframe table and flag calls go through the C ABI on ready int32 / int64 arrays (no per-element Python); its numpy "
                    "parts (the stereo points, the table edits, the ids from the tables, the comparison) are interpreted and bound a compiled shim from "
                    "above; *_without_numpy leaves them out: the sequence's library calls and copies, with ctypes' call overhead.  Stereo positions of "
                    "the two create forms are compared to 1e-12 relative (numpy's matrix product against the kernel's), everything else byte for byte")
    print(json.dumps(row), flush=True)
    h.synchronize()
    for k in kfs:
        k.close()
    mp.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "map_create_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(row, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
