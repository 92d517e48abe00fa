"""Seeded scenes for the resident map-point store: a store of CAPACITY slots, keyframe slot tables and frames to track.

scene(): one frame of tests/tracking_scenes.py whose map points are given random slots and split, with overlap, over n_kf keyframe
slot tables; the tables also carry -1 entries, repeats and slots that are not live.  Positions and descriptors are that module's,
untouched, so its >= 1e-9 margins from the decision points carry over.
tables_with_total(): slot tables alone, with an exact number of candidates, for the selection kernels' chunk edges.
"""
import numpy as np

import tracking_scenes as G

CAPACITY = 4096
CHUNK = 1024                  # candidates per workgroup of the selection kernels (map_store_kernels.hip: MS_CHUNK)


class Store:
    """host image of a store: positions [CAPACITY,3], desc [CAPACITY,32], live [CAPACITY]"""

    def __init__(self, capacity=CAPACITY):
        self.capacity = capacity
        self.positions = np.zeros((capacity, 3)); self.desc = np.zeros((capacity, 32), np.uint8); self.live = np.zeros(capacity, np.uint8)

    def set(self, slots, positions, desc):
        self.positions[slots] = positions; self.desc[slots] = desc; self.live[slots] = 1

    def live_slots(self):
        return np.flatnonzero(self.live).astype(np.int32)


def scene(seed, n_mp, n_feat, n_kf, store=None, taken=None, **kw):
    """-> dict(frame=(kp, desc, search_pose, prior), slots [n_mp] (the slot of each of the frame's map points), tables [n_kf],
    dead [..] slots the tables name that are not live).  Fills `store` (a fresh one by default); `taken`: slots already in use."""
    rng = np.random.default_rng(seed + 1000)
    f = G.frame(seed, n_mp, n_feat, **kw)
    store = store or Store()
    free = np.setdiff1d(np.arange(store.capacity), np.concatenate([store.live_slots(), np.asarray(taken if taken is not None else [], np.int64)]))
    pick = rng.permutation(free)[:n_mp + 8]
    slots, dead = pick[:n_mp].astype(np.int32), pick[n_mp:].astype(np.int32)
    store.set(slots, f[2], f[3])
    parts = [[] for _ in range(n_kf)]
    for s in slots:                                             # every point in one keyframe, some in a second one too
        k = int(rng.integers(n_kf))
        parts[k].append(int(s))
        if n_kf > 1 and rng.uniform() < 0.35:
            parts[int((k + 1 + rng.integers(n_kf - 1)) % n_kf)].append(int(s))
    tables = []
    for k, p in enumerate(parts):
        p = p + [-1] * int(rng.integers(1, 6)) + [int(d) for d in dead[rng.integers(0, 2, len(dead)) == 1]]
        if len(p) > 2:
            p.append(p[0])                                      # a repeat inside the keyframe
        tables.append(np.array(p, np.int32)[rng.permutation(len(p))])
    return dict(frame=(f[0], f[1], f[4], f[5]), slots=slots, tables=tables, dead=dead, store=store, track_frame=f)


def tables_with_total(seed, total, n_kf=3, capacity=CAPACITY):
    """(tables, live): n_kf slot tables with exactly `total` candidates; about half as many distinct slots as candidates, some -1,
    some not live.  Slot A is the first candidate and again the one before the last; slot Z appears only as the very last."""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(capacity)[:max(total // 2, 1) + 2]
    A, Z, pool = int(pool[0]), int(pool[1]), pool[2:]
    c = pool[rng.integers(0, len(pool), total)].astype(np.int32) if len(pool) else np.full(total, -1, np.int32)
    c[rng.uniform(size=total) < 0.1] = -1
    if total >= 1:
        c[0] = A
    if total >= 3:
        c[-2] = A; c[-1] = Z
    live = np.zeros(capacity, np.uint8)
    live[pool[rng.uniform(size=len(pool)) < 0.85]] = 1
    live[A] = live[Z] = 1
    cuts = np.sort(rng.integers(0, total + 1, n_kf - 1)) if n_kf > 1 else np.array([], np.int64)
    return [t.copy() for t in np.split(c, cuts)], live


def random_rows(seed, capacity=CAPACITY):
    rng = np.random.default_rng(seed)
    return rng.uniform(-5.0, 5.0, (capacity, 3)), rng.integers(0, 256, (capacity, 32), dtype=np.uint8)


def shared_batch(seed=90):
    """Three scenes in one store and three frames over them that share keyframes and slots: frame 0 = scene A's keyframes and
    scene B's first, frame 1 = scene B's and scene A's first, frame 2 = scene A's alone (in reverse order).
    -> (store, scenes [3], frames_kf: per frame a list of (scene, keyframe index))"""
    store = Store()
    scs = [scene(seed, 150, 260, 3, store=store), scene(seed + 1, 90, 140, 2, store=store), scene(seed + 2, 40, 80, 1, store=store)]
    frames_kf = [[(0, 0), (0, 1), (0, 2), (1, 0)], [(1, 0), (1, 1), (0, 0)], [(0, 2), (0, 1), (0, 0)]]
    return store, scs, frames_kf
