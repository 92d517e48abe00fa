"""Seeded worlds for point creation on the resident map: tests/triangulation_scenes.py's keyframes with their map-point flags turned
into slot tables over a store of CAPACITY slots.

A flagged feature names a live slot (keyframes share slots: the pool is smaller than the flags drawn from it).  About a fifth of the
unflagged features name a DEAD slot, which must read as unflagged and be overwritten like -1.  A few slots are named twice in one
keyframe.  One neighbour — and in t10_grid the current keyframe too — has no table: all its flags are 0, whatever the scene drew.
free_slots is a shuffled list of slots that are dead and that no table names (the caller's precondition).
"""
import numpy as np

import triangulation_scenes as G

CAPACITY = 4096
LIVE_POOL, DEAD_POOL = 1500, 1000               # slots [0, 1500) are live, [1500, 2500) dead and nameable, [2500, 4096) free
N_FREE = 1200
CHUNK = 1024                                    # mc_stereo_kernel's round (map_store_kernels.hip: MS_CHUNK)
CASES = dict(G.FUSED_CASES, large=dict(seed=21, n_points=1000, T=3, n_distract=200))
NO_TABLE = {"t1_grid": [1], "t3_nodes": [3], "t10_grid": [0, 4], "t10_nodes_current_only": [4], "t10_nodes": [4], "large": [3]}   # places in [cur] + neighbours
_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = G.fused_scene(name) if name in G.FUSED_CASES else G.make_scene(**CASES[name])
    return _cache[name]


def _table(rng, mp):
    n = len(mp)
    t = np.full(n, -1, np.int32)
    on = np.flatnonzero(mp)
    t[on] = rng.choice(LIVE_POOL, len(on), replace=False)
    off = np.flatnonzero(mp == 0)
    dead = off[rng.random(len(off)) < 0.2]
    t[dead] = LIVE_POOL + rng.integers(0, DEAD_POOL, len(dead))
    for _ in range(min(3, len(on) // 2)):                                  # a slot named twice: both features are flagged
        a, b = rng.choice(on, 2, replace=False)
        t[b] = t[a]
    return t


def world(name):
    """-> dict(scene, tables [1 + T] (None: no table), live [CAPACITY], positions, desc (the store's rows), free_slots int32 [N_FREE])"""
    key = ("world", name)
    if key not in _cache:
        sc = scene(name)
        rng = np.random.default_rng([0xC4EA, CASES[name]["seed"]])
        kfs = [sc["current"]] + list(sc["neighbours"])
        tables = [_table(rng, np.asarray(kf["mp"])) for kf in kfs]
        for k in NO_TABLE[name]:
            tables[k] = None
        live = np.zeros(CAPACITY, np.uint8); live[:LIVE_POOL] = 1
        positions = rng.uniform(-5.0, 5.0, (CAPACITY, 3)); desc = rng.integers(0, 256, (CAPACITY, 32), dtype=np.uint8)
        free = (LIVE_POOL + DEAD_POOL + rng.permutation(CAPACITY - LIVE_POOL - DEAD_POOL)[:N_FREE]).astype(np.int32)
        _cache[key] = dict(scene=sc, tables=tables, live=live, positions=positions, desc=desc, free_slots=free)
    return _cache[key]


def expected(oracle, name, phases=3, n_free=N_FREE, is_inertial=0):
    """the specification's answer for world(name); computed once"""
    import map_create_spec as S
    import triangulation_spec as TS
    key = ("spec", name, phases, n_free, is_inertial)
    if key not in _cache:
        w = world(name)
        sc = w["scene"]
        _cache[key] = S.create_points(oracle, sc["camera"], TS.default_config(), is_inertial, sc["current"], sc["neighbours"], w["tables"], w["live"],
                                      w["free_slots"][:n_free], phases)
    return _cache[key]
