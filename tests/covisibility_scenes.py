"""Seeded scenes for covisibility on the resident map, built on tests/map_store_scenes.py.

world()          keyframe slot tables over one store: feature counts from SIZES (the count kernel's block edges), slots drawn from a
                 shared pool so that keyframes overlap, with -1 entries, repeats inside a table, slots that are not live and
                 keyframes without a table
row_world()      tables whose weight row of keyframe 0 is all equal / all zero / rising with the index (best = reverse index order)
tracking_world() three map_store_scenes scenes in one store: scene A's keyframes share many points (a reference with more covisibles
                 than n_best), scene C is one keyframe that shares nothing (a reference without covisibles)
"""
import numpy as np

import map_store_scenes as M

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
N_KFS = [1, 2, 3, 11, 64, 65, 257]


def world(seed, n_kfs, capacity=M.CAPACITY, sizes=SIZES):
    """-> (tables [n_kfs] (int32 arrays, None = no table), n_features [n_kfs], live u8 [capacity])"""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(capacity)[:max(capacity * 3 // 8, 8)]
    live = np.zeros(capacity, np.uint8)
    live[pool[rng.uniform(size=len(pool)) < 0.85]] = 1
    order = rng.permutation(len(sizes))
    tables, counts = [], []
    for k in range(n_kfs):
        n = int(sizes[order[k % len(sizes)]])
        t = pool[rng.integers(0, len(pool), n)].astype(np.int32)
        t[rng.uniform(size=n) < 0.1] = -1
        if n >= 2:
            t[-1] = t[0]                                        # a repeat inside the keyframe, whatever the draw gave
        counts.append(n)
        tables.append(None if k % 7 == 5 else t)
    return tables, counts, live


def row_world(kind, n_kfs, capacity=M.CAPACITY):
    """keyframe 0 observes slots [0, 2 * n_kfs); keyframe k > 0 shares `equal`: 3 of them, `zero`: none, `rising`: k of them."""
    live = np.ones(capacity, np.uint8)
    base = np.arange(2 * n_kfs, dtype=np.int32)
    tables = [base]
    for k in range(1, n_kfs):
        own = np.array([2 * n_kfs + k], np.int32)
        share = {"equal": base[k:k + 3], "zero": base[:0], "rising": base[:k]}[kind]
        tables.append(np.concatenate([own, share]).astype(np.int32))
    return tables, [len(t) for t in tables], live


def tracking_world(seed=130):
    """-> (store, scenes [3], tables (all scenes' keyframes in order), first (index of each scene's first keyframe))"""
    store = M.Store()
    scs = []
    for i, (n_mp, n_feat, n_kf) in enumerate([(160, 260, 6), (90, 140, 2), (40, 80, 1)]):      # (no scene takes a slot an earlier one names as dead)
        scs.append(M.scene(seed + i, n_mp, n_feat, n_kf, store=store, taken=np.concatenate([s["dead"] for s in scs] + [np.zeros(0, np.int32)])))
    tables = [t for sc in scs for t in sc["tables"]]
    first = np.cumsum([0] + [len(sc["tables"]) for sc in scs])[:3]
    return store, scs, tables, [int(x) for x in first]
