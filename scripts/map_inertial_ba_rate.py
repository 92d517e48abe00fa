#!/usr/bin/env python3
"""Host time of local INERTIAL BA from the resident map against the same run's sequence a caller makes today.

  (a) collection alone   Handle.map_collect_inertial_window_device and one synchronisation.
  (b) local inertial BA  Handle.map_local_inertial_ba (collection on the device, one small download, the solve on the observations
                         where they lie, the scatter of the optimised positions) against today's sequence:
                         MapSnapshot.collect_inertial_ba_data and flatten_inertial_ba_problem (the sequence's collect part), then
                         Handle.ba_solve_inertial and MapPointStore.set (its solve part).  The snapshot walk is Python: a compiled
                         shim pays less for it, so the collect part bounds the host cost from above; it is reported apart from the
                         solve part for that reason, and the resident call is compared against the solve part alone as well.

One window — synth.inertial_window(42, 10, 2000) (the README's inertial row: 10 keyframes, about 2000 points, about 20 k observations,
9 IMU edges, two older keyframes that only observe) — inside a map of 100 and of 1000 resident keyframes.  The window's keyframes carry
one feature per observation (at least 2000 features); the other resident keyframes have 2000 features over other points of the store.
The store's positions are put back before every local BA of either form (the same MapPointStore.set in both, also timed alone).  The
forms are timed in the same process in alternating rounds, each at least --round-seconds long; per form the median over the rounds and
the spread (min, max), plus the device time per kernel.
usage: python scripts/map_inertial_ba_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
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

CAPACITY, LIVE, KF_FEAT = 65536, 50000, 2000
SEED, K, M, N_FIXED = 42, 10, 2000, 2
BAC_KERNELS = ("bac_index_kernel", "bac_count_kernel", "bac_order_kernel", "bac_emit_kernel", "bac_restore_kernel")
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


def kernel_us(h, f, steps):
    h.set_profiling(True)
    h.kernel_times()
    for _ in range(steps):
        f()
    kt = {k: v[0] / steps * 1e3 for k, v in h.kernel_times().items()}
    h.set_profiling(False)
    return kt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_inertial_ba_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**P.synth.EUROC_CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, capacity=CAPACITY, live_points=LIVE,
               resident_keyframe_features=KF_FEAT,
               note="parent_collect is MapSnapshot's Python walk and flatten: an upper bound on what a compiled shim pays; every local BA of either form is "
                    "preceded by the same MapPointStore.set that puts the window's positions back (reset_ms)",
               rows=[])
    rng = np.random.default_rng(SEED)
    win = P.synth.keypoint_precision(P.synth.inertial_window(SEED, K, M, P.BA_OBS, n_fixed=N_FIXED))
    obs = win["obs"]
    order = rng.permutation(CAPACITY).astype(np.int32)
    win_slots, rest = order[:M], order[M:LIVE]
    pos = rng.uniform(-5.0, 5.0, (CAPACITY, 3)); desc = rng.integers(0, 256, (CAPACITY, 32), dtype=np.uint8)
    pos[win_slots] = win["points"]
    live_slots = np.sort(order[:LIVE]).astype(np.int32)
    mp = P.MapPointStore(h, CAPACITY)
    mp.set(live_slots, pos[live_slots], desc[live_slots])
    # keyframes 0, 1: the older observers; 2 .. K + 1: the chain, oldest first
    tables, uvs, stereo, poses = [], [], [], []
    for k in range(K + N_FIXED):
        o = obs[(obs["kf_idx"] < 0) & (obs["fixed_idx"] == k)] if k < N_FIXED else obs[obs["kf_idx"] == k - N_FIXED]
        pad = max(KF_FEAT - len(o), 0)
        tables.append(np.concatenate([win_slots[o["mp_idx"]], np.full(pad, -1, np.int32)]).astype(np.int32))
        uvs.append(np.concatenate([np.stack([o["u"], o["v"]], 1), rng.uniform(1.0, 470.0, (pad, 2))]).astype(np.float32))
        stereo.append(np.concatenate([o["_pad"] & 1, np.zeros(pad, np.int32)]).astype(np.uint8))
        poses.append(P.se3_inverse(win["fixed_cw"][k]) if k < N_FIXED else win["poses_wc"][k - N_FIXED])
    while len(tables) < 1000:
        lo = (len(tables) * 37) % max(len(rest) - 6000, 1)
        t = rest[lo + rng.integers(0, 6000, KF_FEAT)].astype(np.int32)
        t[rng.uniform(size=KF_FEAT) < 0.25] = -1
        tables.append(t); uvs.append(rng.uniform(1.0, 470.0, (KF_FEAT, 2)).astype(np.float32)); stereo.append((rng.uniform(size=KF_FEAT) < 0.5).astype(np.uint8))
        poses.append(np.array([1.0, 0, 0, 0, 0, 0, 0]))
    all_kfs = []
    for t, uv, st, pose in zip(tables, uvs, stereo, poses):
        zd = torch.zeros((len(t), 32), dtype=torch.uint8, device="cuda")
        kf = P.KeyFrame(h, d(G.keypoints(uv).view(np.uint8).reshape(-1, G.KEYPOINT.itemsize)), zd, len(t),
                        d_points_cam=torch.zeros((len(t), 3), dtype=torch.float64, device="cuda"), d_has_point=d(st), pose_wc=pose)
        kf.set_map_point_slots(mp, t)
        all_kfs.append(kf)
    cfg = P.LocalInertialBAConfig(window_size=K)
    chain = list(range(N_FIXED, N_FIXED + K))
    init = np.ascontiguousarray(win["points"])
    vel, bias, ek, pre = win["velocities"], win["biases"], win["edge_kf"], win["preint"]
    for n_kfs in (100, 1000):
        kfs = all_kfs[:n_kfs]
        # today's host-side map of the same keyframes (ids: 1000 + position; a point's id is its slot)
        ids = 1000 + np.arange(n_kfs, dtype=np.uint64)
        cnt = np.array([len(t) for t in tables[:n_kfs]], np.int32)
        fs = np.zeros(n_kfs + 1, np.int32); fs[1:] = np.cumsum(cnt)
        feat_mp = np.concatenate(tables[:n_kfs]).astype(np.int64)
        feat_kf = np.repeat(ids, cnt)
        feat_ix = (np.arange(len(feat_mp)) - np.repeat(fs[:-1], cnt)).astype(np.int32)
        seen = feat_mp >= 0
        by_mp = np.argsort(feat_mp[seen], kind="stable")
        obs_mp, obs_kf, obs_ix = feat_mp[seen][by_mp], feat_kf[seen][by_mp], feat_ix[seen][by_mp]
        mp_obs_start = np.searchsorted(obs_mp, live_slots.astype(np.int64)).astype(np.int32)
        mp_obs_start = np.concatenate([mp_obs_start, [np.searchsorted(obs_mp, live_slots[-1], side="right")]]).astype(np.int32)
        prev = np.full(n_kfs, -1, np.int64); kvel = np.zeros((n_kfs, 3)); kbias = np.zeros((n_kfs, 6)); has_pre = np.zeros(n_kfs, np.uint8); kpre = np.zeros((n_kfs, 11))
        for i, k in enumerate(chain):
            kvel[k] = vel[i]; kbias[k] = bias[i]
            if i:
                prev[k] = 1000 + chain[i - 1]; has_pre[k] = 1; kpre[k] = pre[i - 1]
        snap = P.MapSnapshot(imu_initialized=True, kf_ids=ids, kf_bad=np.zeros(n_kfs, np.uint8), kf_pose_wc=np.stack(poses[:n_kfs]), kf_n_keypoints=cnt,
                             kf_feat_start=fs, feat_mp_id=feat_mp, feat_uv=np.concatenate(uvs[:n_kfs]), cov_start=np.zeros(n_kfs + 1, np.int32),
                             cov_kf_id=np.zeros(0, np.uint64), mp_ids=live_slots.astype(np.uint64), mp_bad=np.zeros(len(live_slots), np.uint8), mp_pos=pos[live_slots],
                             mp_obs_start=mp_obs_start, mp_obs_kf_id=obs_kf, kf_prev_id=prev, kf_velocity=kvel, kf_bias=kbias, kf_has_preint=has_pre, kf_preint=kpre,
                             feat_stereo=np.concatenate(stereo[:n_kfs]), mp_obs_feat_idx=obs_ix)
        cur_id = 1000 + chain[-1]

        def reset():
            mp.set(win_slots, positions=init)

        def collect_device():
            o = h.map_collect_inertial_window_device(mp, kfs, chain)
            h.synchronize()
            return o

        def local_ba_resident():
            reset()
            return h.map_local_inertial_ba(cam, mp, kfs, chain, vel, bias, ek, pre, cfg)

        def parent_collect():
            prob = snap.collect_inertial_ba_data(cur_id, cfg)
            return (prob,) + tuple(P.flatten_inertial_ba_problem(prob))

        def parent_solve(c):
            reset()
            prob, p_wc, p_vel, p_bias, p_fixed, p_pts, p_obs, p_ek, p_pre = c
            r = h.ba_solve_inertial(cam, cfg, p_wc, p_vel, p_bias, p_fixed, p_pts, p_obs, p_ek, p_pre)
            mp.set(np.array(prob.mp_ids, np.int32), positions=r["points"])
            return r

        def parent_sequence():
            return parent_solve(parent_collect())

        reset()
        for _ in range(a.warmup):
            dev = collect_device(); lb = local_ba_resident(); par = parent_sequence()
        reset()
        dev = collect_device()
        Kc, Fc, Mc, Nc = (int(x) for x in dev["counts"].cpu().numpy())
        c0 = parent_collect()
        o32 = dev["obs32"][:Nc].cpu().numpy().view(P.BA_OBS32).reshape(-1)
        # the parent lists its observations point by point and the anchor's pose last: the same multiset, another order
        slot_of = dev["list_slot"][:Mc].cpu().numpy()
        fx = dev["fixed_kf"].cpu().numpy()
        mine = sorted((int(chain[i]) if i >= 1 else int(chain[0]) if i == -1 else int(fx[-2 - i]), int(slot_of[m & ~P.BA_OBS32_STEREO]), float(u), float(v),
                       bool(m & P.BA_OBS32_STEREO), i >= 1) for i, m, u, v in o32.tolist())
        theirs = sorted((int(o.kf_id) - 1000, int(o.mp_id), float(np.float32(o.observed_uv[0])), float(np.float32(o.observed_uv[1])), bool(o.is_stereo),
                         bool(o.is_kf_in_window)) for o in c0[0].visual_observations)
        same_window = mine == theirs and slot_of.tolist() == [int(m) for m in c0[0].mp_ids] and len(c0[7]) == len(ek)
        same_ba = lb["iterations"] == par["iterations"] and abs(lb["final_error"] - par["final_error"]) <= 1e-9 * par["final_error"]
        forms = (("reset", reset), ("collect_device", collect_device), ("local_ba_resident", local_ba_resident), ("parent_collect", parent_collect),
                 ("parent_solve", lambda: parent_solve(c0)), ("parent_sequence", parent_sequence))
        steps, t = measure(forms, a.rounds, a.round_seconds)
        kt_collect = kernel_us(h, collect_device, steps["collect_device"])
        kt_ba = kernel_us(h, local_ba_resident, steps["local_ba_resident"])
        row = dict(window_keyframes=K, window_points=Mc, window_observations=Nc, imu_edges=int(len(ek)), resident_keyframes=n_kfs, counts=[Kc, Fc, Mc, Nc],
                   iterations=int(lb["iterations"]), window_equal_to_parent_as_multiset=bool(same_window),
                   local_ba_agrees_with_parent_sequence=bool(same_ba), final_error=[lb["final_error"], par["final_error"]], calls_per_round=steps,
                   **{k + "_ms": v for k, v in t.items()},
                   local_ba_ranges_overlap=overlap(t["local_ba_resident"], t["parent_sequence"]),
                   local_ba_vs_parent_solve_ranges_overlap=overlap(t["local_ba_resident"], t["parent_solve"]),
                   collect_kernel_us_per_call=kt_collect, local_ba_kernel_us_per_call=kt_ba,
                   collect_new_kernels_us_per_call=sum(v for k, v in kt_collect.items() if k in BAC_KERNELS),
                   collect_selection_kernels_us_per_call=sum(v for k, v in kt_collect.items() if k in SEL_KERNELS),
                   local_ba_kernels_us_per_call=sum(kt_ba.values()))
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    h.synchronize()
    for k in all_kfs:
        k.close()
    mp.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "map_inertial_ba_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
