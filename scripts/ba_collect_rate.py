#!/usr/bin/env python3
"""Host time of local BA from the resident map against the same run's sequence a caller makes today.

  (a) collection alone   Handle.map_collect_ba_window_device and one synchronisation.
  (b) local BA           Handle.map_local_ba (collection on the device, one small download, the solve on the observations where
                         they lie, the scatter of the optimised positions) against today's sequence:
                         MapSnapshot.collect_visual_ba_data, flatten_ba_problem and the 16-byte form into pinned memory (the
                         sequence's collect part), then Handle.ba_solve_visual from that pinned memory and MapPointStore.set (its
                         solve part).  The snapshot walk is Python: a compiled shim pays less for it, so the collect part bounds
                         the host cost from above; it is reported apart from the solve part for that reason.
  (c) the solve alone    Handle.ba_solve_visual_obs32_device on the collected observations against Handle.ba_solve_visual on the
                         same observations in pinned host memory: same window, same process.

Two windows — synth.ba_window(42, 20, 2000) (the README's local-BA row) and synth.ba_window(43, 50, 8000) (configs[4]) — each inside
a map of 100 and of 1000 resident keyframes.  A window's keyframes carry one feature per observation (at least 2000 features); the
other resident keyframes have 2000 features over other points of the store, so they share nothing with the window.  The store's
positions are put back before every local BA of either form (the same MapPointStore.set in both, also timed alone), so that every
solve starts from the same perturbed window.  The forms are timed in the same process in alternating rounds, each at least
--round-seconds long; per form the median over the rounds and the spread (min, max), plus the device time per kernel.
usage: python scripts/ba_collect_rate.py [--rounds R] [--round-seconds S] [--warmup W] [--out FILE.json]"""
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
WINDOWS = ((42, 20, 2000), (43, 50, 8000))
BAC_KERNELS = ("bac_index_kernel", "bac_count_kernel", "bac_order_kernel", "bac_emit_kernel", "bac_restore_kernel")
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
        raise SystemExit("ba_collect_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**P.synth.EUROC_CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, capacity=CAPACITY, live_points=LIVE,
               resident_keyframe_features=KF_FEAT,
               note="parent_collect is MapSnapshot's Python walk, flatten and the copy into pinned memory: an upper bound on what a compiled shim pays; "
                    "every local BA of either form is preceded by the same MapPointStore.set that puts the window's positions back (reset_ms)",
               rows=[])
    for seed, K, M in WINDOWS:
        rng = np.random.default_rng(seed)
        win = P.synth.keypoint_precision(P.synth.ba_window(seed, K, M, P.BA_OBS))
        obs = win["obs"]
        order = rng.permutation(CAPACITY).astype(np.int32)
        win_slots, rest = order[:M], order[M:LIVE]
        pos = rng.uniform(-5.0, 5.0, (CAPACITY, 3)); desc = rng.integers(0, 256, (CAPACITY, 32), dtype=np.uint8)
        pos[win_slots] = win["points"]
        live_slots = np.sort(order[:LIVE]).astype(np.int32)
        mp = P.MapPointStore(h, CAPACITY)
        mp.set(live_slots, pos[live_slots], desc[live_slots])
        # the window's keyframes: keyframe 0 is the anchor (fixed_idx 0), keyframe 1 + i the i-th optimised one
        tables, uvs, poses = [], [], []
        for k in range(K):
            o = obs[(obs["kf_idx"] == k - 1) & (obs["fixed_idx"] == -1)] if k else obs[obs["kf_idx"] < 0]
            pad = max(KF_FEAT - len(o), 0)
            tables.append(np.concatenate([win_slots[o["mp_idx"]], np.full(pad, -1, np.int32)]).astype(np.int32))
            uvs.append(np.concatenate([np.stack([o["u"], o["v"]], 1), rng.uniform(1.0, 470.0, (pad, 2))]).astype(np.float32))
            poses.append(P.se3_inverse(win["poses_cw"][k - 1] if k else win["fixed_cw"][0]))
        while len(tables) < 1000:
            lo = (len(tables) * 37) % max(len(rest) - 6000, 1)
            t = rest[lo + rng.integers(0, 6000, KF_FEAT)].astype(np.int32)
            t[rng.uniform(size=KF_FEAT) < 0.25] = -1
            tables.append(t); uvs.append(rng.uniform(1.0, 470.0, (KF_FEAT, 2)).astype(np.float32)); poses.append(np.array([1.0, 0, 0, 0, 0, 0, 0]))
        all_kfs = []
        for t, uv, pose in zip(tables, uvs, poses):
            zd = torch.zeros((len(t), 32), dtype=torch.uint8, device="cuda")
            kf = P.KeyFrame(h, d(G.keypoints(uv).view(np.uint8).reshape(-1, G.KEYPOINT.itemsize)), zd, len(t), pose_wc=pose)
            kf.set_map_point_slots(mp, t)
            all_kfs.append(kf)
        cfg = P.LocalBAConfigLM(max_covisible_keyframes=K - 1)
        init = np.ascontiguousarray(win["points"])
        for n_kfs in (100, 1000):
            kfs = all_kfs[:n_kfs]
            # today's host-side map of the same keyframes (ids: 1000 + position; a point's id is its slot)
            ids = 1000 + np.arange(n_kfs, dtype=np.uint64)
            cnt = np.array([len(t) for t in tables[:n_kfs]], np.int32)
            fs = np.zeros(n_kfs + 1, np.int32); fs[1:] = np.cumsum(cnt)
            feat_mp = np.concatenate(tables[:n_kfs]).astype(np.int64)
            feat_kf = np.repeat(ids, cnt)
            seen = feat_mp >= 0
            by_mp = np.argsort(feat_mp[seen], kind="stable")
            obs_mp, obs_kf = feat_mp[seen][by_mp], feat_kf[seen][by_mp]
            mp_obs_start = np.searchsorted(obs_mp, live_slots.astype(np.int64)).astype(np.int32)
            mp_obs_start = np.concatenate([mp_obs_start, [np.searchsorted(obs_mp, live_slots[-1], side="right")]]).astype(np.int32)
            _, best, nb = h.map_covisibility(mp, kfs, [0], K - 1)
            cov_start = np.zeros(n_kfs + 1, np.int32); cov_start[1:] = int(nb[0])
            snap = P.MapSnapshot(kf_ids=ids, kf_bad=np.zeros(n_kfs, np.uint8), kf_pose_wc=np.stack(poses[:n_kfs]), kf_n_keypoints=cnt, kf_feat_start=fs,
                                 feat_mp_id=feat_mp, feat_uv=np.concatenate(uvs[:n_kfs]), cov_start=cov_start, cov_kf_id=ids[best[0, :nb[0]]],
                                 mp_ids=live_slots.astype(np.uint64), mp_bad=np.zeros(len(live_slots), np.uint8), mp_pos=pos[live_slots],
                                 mp_obs_start=mp_obs_start, mp_obs_kf_id=obs_kf)
            pinned = torch.empty(len(obs) * P.BA_OBS32.itemsize, dtype=torch.uint8).pin_memory()
            pin32 = pinned.numpy().view(P.BA_OBS32)

            def reset():
                mp.set(win_slots, positions=init)

            def collect_device():
                o = h.map_collect_ba_window_device(mp, kfs, 0, K - 1)
                h.synchronize()
                return o

            def local_ba_resident():
                reset()
                return h.map_local_ba(cam, mp, kfs, 0, cfg, read_points=False)

            def parent_collect():
                prob = snap.collect_visual_ba_data(1000, cfg)
                poses_cw, fixed_cw, pts, ob = P.flatten_ba_problem(prob)
                o32 = P.ba_obs_to_obs32(ob, len(fixed_cw))
                pin32[:len(o32)] = o32
                return prob, poses_cw, fixed_cw, pts, len(o32)

            def parent_solve(c):
                reset()
                prob, poses_cw, fixed_cw, pts, n = c
                r = h.ba_solve_visual(cam, cfg, poses_cw, fixed_cw, pts, pin32[:n])
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
            same_window = Nc == c0[4] and dev["obs32"][:Nc].cpu().numpy().tobytes() == pin32[:Nc].tobytes() and \
                dev["list_slot"][:Mc].cpu().numpy().tolist() == c0[0].mp_ids
            lk = dev["local_kf"].cpu().numpy()
            poses_cw = np.array([P.se3_inverse(poses[k]) for k in lk[1:1 + Kc]]).reshape(-1, 7)
            fixed_cw = np.array([P.se3_inverse(poses[lk[0]])]).reshape(-1, 7)
            pts0 = dev["positions"][:Mc].cpu().numpy()

            def solve_device_obs():
                return h.ba_solve_visual_obs32_device(cam, cfg, poses_cw, fixed_cw, pts0, dev["obs32"], Nc)

            def solve_pinned_obs():
                return h.ba_solve_visual(cam, cfg, poses_cw, fixed_cw, pts0, pin32[:Nc])

            sd, sp = solve_device_obs(), solve_pinned_obs()
            same_solve = sd["poses_wc"].tobytes() == sp["poses_wc"].tobytes() and sd["points"].tobytes() == sp["points"].tobytes()
            same_ba = lb.iterations == par["iterations"] and lb.final_error == par["final_error"] and \
                np.array([lb.optimized_poses[k] for k in lb.optimized_poses]).tobytes() == par["poses_wc"].tobytes()
            forms = (("reset", reset), ("collect_device", collect_device), ("local_ba_resident", local_ba_resident), ("parent_collect", parent_collect),
                     ("parent_solve", lambda: parent_solve(c0)), ("parent_sequence", parent_sequence), ("solve_device_obs", solve_device_obs),
                     ("solve_pinned_obs", solve_pinned_obs))
            steps, t = measure(forms, a.rounds, a.round_seconds)
            kt_collect = kernel_us(h, collect_device, steps["collect_device"])
            kt_ba = kernel_us(h, local_ba_resident, steps["local_ba_resident"])
            row = dict(window_keyframes=K, window_points=Mc, window_observations=Nc, resident_keyframes=n_kfs, counts=[Kc, Fc, Mc, Nc],
                       iterations=int(lb.iterations), window_equal_to_parent=bool(same_window), solve_equal_device_vs_pinned=bool(same_solve),
                       local_ba_equal_to_parent_sequence=bool(same_ba), calls_per_round=steps, **{k + "_ms": v for k, v in t.items()},
                       local_ba_ranges_overlap=overlap(t["local_ba_resident"], t["parent_sequence"]),
                       local_ba_vs_parent_solve_ranges_overlap=overlap(t["local_ba_resident"], t["parent_solve"]),
                       solve_ranges_overlap=overlap(t["solve_device_obs"], t["solve_pinned_obs"]),
                       collect_kernel_us_per_call=kt_collect, local_ba_kernel_us_per_call=kt_ba,
                       collect_new_kernels_us_per_call=sum(v for k, v in kt_collect.items() if k in BAC_KERNELS),
                       collect_covisibility_kernels_us_per_call=sum(v for k, v in kt_collect.items() if k in COV_KERNELS),
                       collect_selection_kernels_us_per_call=sum(v for k, v in kt_collect.items() if k in SEL_KERNELS),
                       local_ba_kernels_us_per_call=sum(kt_ba.values()))
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        h.synchronize()
        for k in all_kfs:
            k.close()
        mp.close()
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "ba_collect_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
