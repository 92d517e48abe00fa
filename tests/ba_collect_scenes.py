"""Seeded scenes for the local-BA window collected from the resident map, on tests/covisibility_scenes.py's worlds.

keypoints()   per keyframe of a world, f32 pixel coordinates that no two features share (an observation is told by its u, v)
once()        a world with the repeats inside every table removed: every observation associated once, as the reference's map is
ba_scene()    a small geometric scene: keyframes around one place whose keypoints are noisy projections of the store's points;
              the stored positions and the keyframes' poses are perturbed, so that LM has work to do.  Keyframe 0 is the current
              one; with max_covisible = 3 the two keyframes that share the least with it are fixed observers.
"""
import numpy as np

import map_store_scenes as M
import tracking_scenes as G


def keypoints(seed, counts):
    rng = np.random.default_rng(seed + 7000)
    return [np.stack([rng.uniform(1.0, G.W - 1.0, n), rng.uniform(1.0, G.H - 1.0, n)], 1).astype(np.float32).reshape(-1, 2) for n in counts]


def once(tables):
    out = []
    for t in tables:
        if t is None:
            out.append(None)
            continue
        keep = np.ones(len(t), bool)
        seen = set()
        for i, s in enumerate(t.tolist()):
            if s >= 0 and s in seen:
                keep[i] = False
            seen.add(s)
        out.append(np.where(keep, t, -1).astype(np.int32))
    return out


def _project(pose_wc, X, cam=G.CAMERA):
    q = pose_wc[:4] * np.array([1.0, -1.0, -1.0, -1.0])
    Xc = np.stack([G._rot(q, x - pose_wc[4:]) for x in X])
    return np.stack([cam["fx"] * Xc[:, 0] / Xc[:, 2] + cam["cx"], cam["fy"] * Xc[:, 1] / Xc[:, 2] + cam["cy"]], 1), Xc[:, 2]


def ba_scene(seed=300, n_kf=6, n_mp=150, noise_px=0.4):
    """-> dict(store (host image, positions perturbed), tables [n_kf], kps [n_kf] KEYPOINT, poses_wc [n_kf,7] (perturbed),
    slots [n_mp], cur = 0, max_covisible = 3)"""
    rng = np.random.default_rng(seed)
    centre = np.array([2.0, 1.0, 0.5])                                       # (translations well away from zero: the 1e-6 bar is relative)
    true_poses = [np.concatenate([G._quat(rng.normal(size=3), rng.uniform(0.0, 0.08)), centre + rng.uniform(-0.4, 0.4, 3)]) for _ in range(n_kf)]
    base = np.concatenate([[1.0, 0.0, 0.0, 0.0], centre])
    X = G.backproject(base, np.stack([rng.uniform(120.0, 630.0, n_mp), rng.uniform(90.0, 390.0, n_mp)], 1), rng.uniform(4.0, 10.0, n_mp))
    store = M.Store()
    pick = rng.permutation(store.capacity)[:n_mp + 2]
    slots, dead = pick[:n_mp].astype(np.int32), pick[n_mp:].astype(np.int32)
    store.set(slots, X + rng.normal(0.0, 0.04, X.shape), rng.integers(0, 256, (n_mp, 32), dtype=np.uint8))
    share = [1.0, 0.9, 0.8, 0.7, 0.35, 0.2][:n_kf] + [0.5] * max(n_kf - 6, 0)        # the fraction of the points each keyframe observes
    tables, kps = [], []
    for k, T in enumerate(true_poses):
        uv, z = _project(T, X)
        vis = np.flatnonzero((z > 0.5) & (uv[:, 0] > 2) & (uv[:, 0] < G.W - 2) & (uv[:, 1] > 2) & (uv[:, 1] < G.H - 2) & (rng.uniform(size=n_mp) < share[k]))
        n_extra = 6
        xy = np.concatenate([uv[vis] + np.clip(rng.normal(0.0, noise_px, (len(vis), 2)), -1.5, 1.5),
                             np.stack([rng.uniform(1.0, G.W - 1.0, n_extra), rng.uniform(1.0, G.H - 1.0, n_extra)], 1)])
        t = np.concatenate([slots[vis], [-1] * (n_extra - 2), dead]).astype(np.int32)   # distractors without a point, two on slots that are not live
        if k == 1:                                                          # a point observed twice by one keyframe: two observations
            t = np.concatenate([t, t[:1]]); xy = np.concatenate([xy, xy[:1] + 0.25])
        perm = rng.permutation(len(t))
        tables.append(t[perm]); kps.append(G.keypoints(xy[perm]))
    poses = np.stack([G.perturb(rng, T, rot_deg=0.4, trans=0.02) for T in true_poses])
    return dict(store=store, tables=tables, kps=kps, poses_wc=poses, slots=slots, cur=0, max_covisible=3)
