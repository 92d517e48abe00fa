"""Seeded scenes for the inertial local-BA window collected from the resident map.

has_points()     per keyframe of a covisibility_scenes world, stereo bytes drawn at 0.5
chains()         the chains a world is collected with: tails of the keyframe list of three lengths, each as a tail (ascending position),
                 reversed in position and scattered over the list; a chain whose anchor has no table; the chain of every keyframe
reference_map()  oracle/local_mapper_ref.Map of a world and a chain: prev_kf links follow the chain, every observation is associated
                 in both directions, points_cam says has_point
inertial_scene() synth.inertial_window(seed, K, M, n_fixed=2) as a resident map: K + 2 keyframes (the two older observers first, then the
                 chain) whose tables, keypoints and stereo bytes are the window's observations, with -1 and dead-slot distractors and
                 the features permuted; the store holds the window's perturbed points
SCENE_SEEDS      per K the first seed of inertial_edge_windows.SEEDS at which the oracle, on the window the specification collects from
                 that scene, keeps every LM decision inertial_edge_windows.MARGIN from a tie (tests/test_inertial_collect_cpu.py
                 checks that these are the ones)
"""
import numpy as np

import orb_slam3_rust_amd as P
from oracle import local_mapper_ref as R
import inertial_collect_spec as S
import inertial_edge_windows as W
import map_store_scenes as M
import orientation_cases as C

SCENE_SEEDS = {5: 31, 11: 23788}


def has_points(seed, counts):
    rng = np.random.default_rng(seed + 9000)
    return [(rng.uniform(size=n) < 0.5).astype(np.uint8) for n in counts]


def tails(n_kfs):
    """the tail chains of a world of n_kfs keyframes: lengths 2, 3 and min(10, n_kfs)"""
    return [list(range(n_kfs - L, n_kfs)) for L in sorted({L for L in (2, 3, min(10, n_kfs)) if 2 <= L <= n_kfs})]


def chains(n_kfs, tables, seed=0):
    """-> list of (name, chain)"""
    out = []
    rng = np.random.default_rng(seed + 9100)
    for t in tails(n_kfs):
        out.append(("tail%d" % len(t), t))
        out.append(("reversed%d" % len(t), t[::-1]))
        out.append(("scattered%d" % len(t), rng.permutation(n_kfs)[:len(t)].tolist()))
    none = [k for k, t in enumerate(tables) if t is None]
    if none and n_kfs >= 2:
        out.append(("anchor_without_table", [none[0]] + [k for k in range(n_kfs) if k != none[0]][:2]))
    if 2 <= n_kfs <= 65:
        out.append(("all", list(range(n_kfs))))
    return out


def reference_map(tables, xy, has, live, chain):
    """keyframe k has id 100 + k, a live slot s is map point s, every observation is associated in both directions in keyframe order;
    chain[i]'s prev_kf is chain[i - 1] and it carries a preintegration with dt > 0.  -> (map, id of the current keyframe)"""
    m = R.Map()
    ident = np.array([1.0, 0, 0, 0, 0, 0, 0])
    for s in np.flatnonzero(live).tolist():
        m.map_points[s] = R.MapPoint(np.zeros(3))
    for k, t in enumerate(tables):
        ids = [None] * len(xy[k]) if t is None else [None if s < 0 else int(s) for s in t.tolist()]
        m.keyframes[100 + k] = R.KeyFrame(ident, [(float(x), float(y)) for x, y in xy[k]], ids,
                                          points_cam=[] if has[k] is None else [bool(b) for b in has[k]])
        for i, s in enumerate(ids):
            if s is not None and s in m.map_points:
                assert 100 + k not in m.map_points[s].observations
                m.map_points[s].observations[100 + k] = i
    pre = np.array([1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.25])
    for i in range(1, len(chain)):
        m.keyframes[100 + chain[i]].prev_kf = 100 + chain[i - 1]
        m.keyframes[100 + chain[i]].imu_preintegrated = pre
    m.imu_initialized = True
    return m, 100 + chain[-1]


def inertial_scene(seed, K, n_mp=None):
    """-> dict(window (synth's, pixel coordinates rounded to f32), store (host image), slots [n_mp], tables, xy, has, poses_wc [K + 2, 7],
    chain = [2 .. K + 1], camera)"""
    n_mp = W.POINTS[K] if n_mp is None else n_mp
    w = P.synth.keypoint_precision(P.synth.inertial_window(seed, K, n_mp, P.BA_OBS, n_fixed=2))
    rng = np.random.default_rng([0x1C5, seed, K])
    store = M.Store()
    pick = rng.permutation(store.capacity)[:n_mp + 2]
    slots, dead = pick[:n_mp].astype(np.int32), pick[n_mp:].astype(np.int32)
    store.set(slots, w["points"], rng.integers(0, 256, (n_mp, 32), dtype=np.uint8))
    poses = np.concatenate([np.array([P.se3_inverse(p) for p in w["fixed_cw"]]).reshape(-1, 7), w["poses_wc"]])
    o = w["obs"]
    tables, xy, has = [], [], []
    for k in range(K + 2):
        mine = o[(o["kf_idx"] < 0) & (o["fixed_idx"] == k)] if k < 2 else o[o["kf_idx"] == k - 2]
        n_extra = 5
        t = np.concatenate([slots[mine["mp_idx"]], [-1] * (n_extra - 2), dead]).astype(np.int32)      # distractors: no point; slots that are not live
        p = np.concatenate([np.stack([mine["u"], mine["v"]], 1), np.stack([rng.uniform(1.0, 750.0, n_extra), rng.uniform(1.0, 478.0, n_extra)], 1)]).astype(np.float32)
        h = np.concatenate([mine["_pad"] & 1, rng.integers(0, 2, n_extra)]).astype(np.uint8)
        perm = rng.permutation(len(t))
        tables.append(t[perm]); xy.append(p[perm]); has.append(h[perm])
    return dict(window=w, store=store, slots=slots, tables=tables, xy=xy, has=has, poses_wc=poses, chain=list(range(2, K + 2)), camera=w["camera"])


def spec_window(sc):
    """the window the specification collects from an inertial_scene, as ba_solve_inertial's arguments (observations widened)"""
    c = S.collect(sc["tables"], sc["xy"], sc["has"], sc["store"].live, sc["chain"])
    w = sc["window"]
    F = int(c["counts"][1])
    fixed_cw = np.array([P.se3_inverse(sc["poses_wc"][k]) for k in [sc["chain"][0]] + c["fixed_kf"].tolist()]).reshape(-1, 7)
    return dict(poses_wc=sc["poses_wc"][sc["chain"]], velocities=w["velocities"], biases=w["biases"], fixed_cw=fixed_cw,
                points=sc["store"].positions[c["list_slot"]], obs=S.widen(c["obs32"], F), edge_kf=w["edge_kf"], preint=w["preint"], camera=sc["camera"]), c


_solved = {}


def solved_scene(seed, K):
    """(scene, its spec window, the collection, the oracle's result), cached per process: do not write to them"""
    if (seed, K) not in _solved:
        sc = inertial_scene(seed, K)
        win, c = spec_window(sc)
        _solved[(seed, K)] = (sc, win, c, W.oracle(win))
    return _solved[(seed, K)]


def first_seed(K):
    for seed in W.SEEDS:
        if C.lm_margin(solved_scene(seed, K)[3]["trace"]) >= W.MARGIN:
            return seed
    raise AssertionError("no seed at K = %d keeps every LM decision %.0e from a tie" % (K, W.MARGIN))
