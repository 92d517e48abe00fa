#!/usr/bin/env python3
"""Host time of global BA from the resident map, and of the whole-map solver against what existed before it.

  (a) map scale     Handle.map_global_ba (collection on the device, one download of counts, slots and positions, the whole-map solve on
                    the observations where they lie, the scatter of the optimised positions) on 300 and 1000 resident keyframes of 2000
                    features over a store of 50 000 live points: ms per call of 10 LM iterations, ms per iteration, device time per
                    kernel grouped into collection / lists / build / Schur / factorisation / back-substitution / decision, the rest of
                    the host call (uploads, the downloads, the host's pose conversions, launch gaps: wall time of the profiled calls minus
                    their kernels), the downloads' bytes as one pinned copy timed alone, and the factorisation's achieved
                    f64 rate (n^3 / 3 flop per factorisation) against the f64 matrix peak AMD publishes for the MI355X.
                    The map is covis_windows.covis_window's corridor, 100 m long: a camera sees about 6 % of the points, a point is seen
                    by as many of the keyframes.  A keyframe keeps its first 2000 observations.  The store's positions are put back
                    before every call (also timed alone), so that every solve starts from the same map.
  (b) K = 128       Handle.ba_solve_global_map against Handle.ba_solve_global on large_ba_windows.global_map(128), alternated.
  (c) the CPU       the oracle's global_ba_solve_schur on global_map_cases' K = 257 map: a one-thread structured restatement of the
                    reference's solver, not the Rust crate.

Forms are timed in the same process in alternating rounds, each at least --round-seconds long; per form the median over the rounds and
the spread (min, max).  The uploads and the download cross the box's host link: those parts depend on it.
usage: python scripts/global_ba_rate.py [--rounds R] [--round-seconds S] [--sizes 300,1000] [--out FILE.json]"""
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
import covis_windows as W  # noqa: E402
import global_map_cases as GM  # noqa: E402
import large_ba_windows as L  # noqa: E402
import tracking_scenes as G  # noqa: E402

CAPACITY, LIVE, KF_FEAT, SPAN = 65536, 50000, 2000, 100.0
F64_MATRIX_PEAK_TFLOPS = 78.6            # AMD's published peak f64 matrix rate of the MI355X
GROUPS = (("collection", ("map_mark_kernel", "map_flag_kernel", "map_emit_kernel", "bac_index_kernel", "bac_count_kernel", "bac_order_kernel", "bac_emit_kernel",
                          "bac_restore_kernel", "map_scatter_kernel")),
          ("lists", ("gba_ingest_kernel", "gba_scan_kernel", "gba_place_kernel", "gba_order_kernel", "gba_kfplace_kernel", "gba_kforder_kernel")),
          ("build", ("gba_pose_kernel", "gba_build_kernel")),
          ("schur", ("gba_kf_schur_kernel",)),
          ("factorisation", ("gba_panel_kernel", "gba_syrk_kernel")),
          ("back_substitution", ("gba_back_kernel", "gba_pose_trial_kernel", "gba_backsub_kernel")),
          ("decision", ("gba_decide_kernel", "gba_finish_kernel")))


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


def kernel_ms(h, f, steps):
    """-> (per-kernel (ms, launches) per call, wall ms per call of the same profiled calls)"""
    h.set_profiling(True)
    h.kernel_times()
    t0 = time.perf_counter()
    for _ in range(steps):
        f()
    wall = (time.perf_counter() - t0) / steps * 1e3
    kt = {k: (v[0] / steps, v[1] / steps) for k, v in h.kernel_times().items()}
    h.set_profiling(False)
    return kt, wall


def map_scale(h, cam, n_kfs, a):
    K = n_kfs - 1
    win = P.synth.keypoint_precision(W.covis_window(seed=7, K=K, F=1, M=LIVE, step=SPAN / n_kfs, keep=1.0, depth=(2, 6), order="kf_major"))
    obs = win["obs"]
    rng = np.random.default_rng(n_kfs)
    slots = np.sort(rng.permutation(CAPACITY)[:LIVE]).astype(np.int32)      # point j lives in slots[j]
    mp = P.MapPointStore(h, CAPACITY)
    init = np.ascontiguousarray(win["points"])
    mp.set(slots, init, rng.integers(0, 256, (LIVE, 32), dtype=np.uint8))
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    kfs, n_obs = [], 0
    for k in range(n_kfs):
        o = obs[(obs["kf_idx"] == k - 1) & (obs["fixed_idx"] == -1)] if k else obs[obs["kf_idx"] < 0]
        o = o[:KF_FEAT]
        n_obs += len(o)
        pad = KF_FEAT - len(o)
        t = np.concatenate([slots[o["mp_idx"]], np.full(pad, -1, np.int32)]).astype(np.int32)
        uv = np.concatenate([np.stack([o["u"], o["v"]], 1), rng.uniform(1.0, 470.0, (pad, 2))]).astype(np.float32)
        pose = P.se3_inverse(win["poses_cw"][k - 1] if k else win["fixed_cw"][0])
        kf = P.KeyFrame(h, d(G.keypoints(uv).view(np.uint8).reshape(-1, G.KEYPOINT.itemsize)), torch.zeros((KF_FEAT, 32), dtype=torch.uint8, device="cuda"), KF_FEAT,
                        pose_wc=pose)
        kf.set_map_point_slots(mp, t)
        kfs.append(kf)

    def reset():
        mp.set(slots, positions=init)

    def collect_device():
        o = h.map_collect_global_device(mp, kfs)
        h.synchronize()
        return o

    def global_ba():
        reset()
        return h.map_global_ba(cam, mp, kfs)

    r = global_ba()
    r2 = global_ba()
    same = r["iterations"] == r2["iterations"] and r["final_error"] == r2["final_error"] and r["poses_wc"].tobytes() == r2["poses_wc"].tobytes()
    steps, t = measure((("reset", reset), ("collect_device", collect_device), ("map_global_ba", global_ba)), a.rounds, a.round_seconds)
    kt, profiled_wall = kernel_ms(h, global_ba, steps["map_global_ba"])
    # the call's one download (counts, P's slots and positions) and the solver's result record, as one pinned copy of the same size
    Mc = int(r["counts"][2])
    down_bytes = 16 + 28 * Mc + 8 * (8 + 6 * K + 3 * Mc)
    src = torch.empty(down_bytes, dtype=torch.uint8, device="cuda"); dst = torch.empty(down_bytes, dtype=torch.uint8).pin_memory()

    def download():
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()

    _, t_down = measure((("download", download),), a.rounds, a.round_seconds)
    groups = {g: sum(kt[k][0] for k in names if k in kt) for g, names in GROUPS}
    launches = {g: sum(kt[k][1] for k in names if k in kt) for g, names in GROUPS}
    kernels = sum(groups.values())
    n = 6 * K
    it = int(r["iterations"])
    fact_ms = groups["factorisation"]
    tflops = (n ** 3 / 3.0) * it / (fact_ms * 1e-3) / 1e12 if fact_ms > 0 else 0.0
    call = t["map_global_ba"]["median"] - t["reset"]["median"]
    row = dict(resident_keyframes=n_kfs, optimised_keyframes=K, n=n, counts=[int(x) for x in r["counts"]], features_per_keyframe=KF_FEAT, observations=n_obs,
               iterations=it, initial_error=r["initial_error"], final_error=r["final_error"], two_runs_same_bits=bool(same), calls_per_round=steps,
               **{k + "_ms": v for k, v in t.items()},
               map_global_ba_without_reset_ms=call, ms_per_lm_iteration=call / max(it, 1),
               kernel_ms_per_call=groups, launches_per_call=launches, kernels_ms_per_call=kernels,
               profiled_call_without_reset_ms=profiled_wall - t["reset"]["median"],
               host_uploads_download_and_gaps_ms=profiled_wall - t["reset"]["median"] - kernels,
               download_bytes=down_bytes, download_alone_ms=t_down["download"],
               factorisation_launches_per_iteration=launches["factorisation"] / max(it, 1) + kt.get("gba_back_kernel", (0, 0))[1] / max(it, 1),
               factorisation_tflops=tflops, trailing_update_tflops=(n ** 3 / 3.0) * it / (kt["gba_syrk_kernel"][0] * 1e-3) / 1e12,
               panel_launch_us=kt["gba_panel_kernel"][0] * 1e3 / max(kt["gba_panel_kernel"][1], 1), f64_matrix_peak_tflops=F64_MATRIX_PEAK_TFLOPS, factorisation_fraction_of_peak=tflops / F64_MATRIX_PEAK_TFLOPS,
               kernel_detail_ms_per_call={k: v[0] for k, v in kt.items()})
    h.synchronize()
    for k in kfs:
        k.close()
    mp.close()
    return row


def k128(h, cam, a):
    w = L.global_map(128)
    c, cfg = P.CameraModel(**w["camera"]), P.GlobalBAConfig()
    new = lambda: h.ba_solve_global_map(c, cfg, w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"])
    old = lambda: h.ba_solve_global(c, cfg, w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"])
    rn, ro = new(), old()
    steps, t = measure((("ba_solve_global_map", new), ("ba_solve_global", old)), a.rounds, a.round_seconds)
    apart = not overlap(t["ba_solve_global_map"], t["ba_solve_global"])
    faster = "ba_solve_global_map" if t["ba_solve_global_map"]["median"] < t["ba_solve_global"]["median"] else "ba_solve_global"
    return dict(K=128, n=768, M=len(w["points"]), N=len(w["obs"]), iterations=[rn["iterations"], ro["iterations"]], calls_per_round=steps,
                **{k + "_ms": v for k, v in t.items()}, ranges_lie_apart=bool(apart), faster=faster if apart else "neither (the ranges overlap)")


def cpu_oracle():
    from oracle import oracle as O
    w = GM.case("k257")
    t0 = time.perf_counter()
    o = O.global_ba_solve_schur(O.Camera(**w["camera"]), L._gcfg(O), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    return w, o, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-seconds", type=float, default=0.3)
    ap.add_argument("--sizes", default="300,1000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("global_ba_rate.py measures on the GPU; none is visible")
    cam = P.CameraModel(**P.synth.EUROC_CAMERA)
    h = P.Handle(cam, 2000, device=0, max_w=752, max_h=480, max_batch=1)
    out = dict(gpu=torch.cuda.get_device_name(0), rounds=a.rounds, round_seconds=a.round_seconds, capacity=CAPACITY, live_points=LIVE,
               note="map_global_ba is timed with the MapPointStore.set that puts the map's positions back before it (reset_ms, also timed alone); "
                    "host_uploads_download_and_gaps_ms is the wall time of the PROFILED calls (the run the kernel times come from) without the reset and without the kernels: "
                    "uploads of poses and tables, the two downloads, the host's pose conversions and launch gaps; it and download_alone_ms (a pinned copy of the "
                    "downloads' bytes with its synchronisation) cross the box's host link and move with it",
               map_scale=[])
    for n_kfs in (int(x) for x in a.sizes.split(",")):
        row = map_scale(h, cam, n_kfs, a)
        out["map_scale"].append(row)
        print(json.dumps(row), flush=True)
    out["k128"] = k128(h, cam, a)
    print(json.dumps(out["k128"]), flush=True)
    w, o, secs = cpu_oracle()
    g = h.ba_solve_global_map(P.CameraModel(**w["camera"]), P.GlobalBAConfig(), w["poses_cw"], w["fixed_cw"][0], w["points"], w["obs"])
    steps, t = measure((("ba_solve_global_map", lambda: h.ba_solve_global_map(P.CameraModel(**w["camera"]), P.GlobalBAConfig(), w["poses_cw"], w["fixed_cw"][0],
                                                                              w["points"], w["obs"])),), a.rounds, a.round_seconds)
    out["k257_against_cpu"] = dict(K=257, n=1542, N=len(w["obs"]), cpu="the oracle's global_ba_solve_schur: a one-thread structured restatement, not the Rust crate",
                                   cpu_seconds=secs, iterations=[g["iterations"], o["iterations"]], ba_solve_global_map_ms=t["ba_solve_global_map"])
    print(json.dumps(out["k257_against_cpu"]), flush=True)
    h.close()
    path = a.out or os.path.join(ROOT, "profiles", "global_ba_rate.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
