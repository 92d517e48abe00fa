"""Seeded scenes for the observation calls on the resident map, on tests/covisibility_scenes.py's worlds and
tests/map_store_scenes.py's stores.

keyframe_rows()    what a world's keyframes carry besides their tables: descriptors [n,32] and a pose whose camera centre is well
                   away from the store's positions (every viewing distance is far above the 1e-10 guard)
with_unobserved()  a world's live bytes with one more live slot that no table names
ratio_world()      keyframes whose redundancy ratio is exactly 0.5 / one feature above 0.5 / exactly 0.9 / one feature above 0.9
SCALE_RANGE        scale_factor ** (num_levels - 1) of the default extractor
"""
import numpy as np

import map_store_scenes as M

SCALE_RANGE = 1.2 ** 7


def keyframe_rows(seed, counts):
    """-> (descs: per keyframe u8 [n,32], poses_wc f64 [K,7])"""
    rng = np.random.default_rng(seed + 9000)
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in counts]
    poses = np.zeros((len(counts), 7)); poses[:, 0] = 1.0
    poses[:, 4:] = rng.uniform(-30.0, -20.0, (len(counts), 3))              # (M.random_rows draws positions from [-5, 5]^3)
    return descs, poses


def with_unobserved(tables, live):
    """-> (live with one more slot set, that slot): live, named by no table"""
    named = set()
    for t in tables:
        if t is not None:
            named.update(int(s) for s in t.tolist())
    s = next(s for s in range(len(live)) if s not in named)
    out = np.array(live, np.uint8, copy=True)
    out[s] = 1
    return out, s


def ratio_world(capacity=M.CAPACITY):
    """Keyframes 0..2 observe the slots [0, 100): with a candidate that names one of them the point has three other observers.
    Keyframes 3..6 are the candidates: `shared` of their features name such a slot, the others a slot of their own.
    -> (tables, counts, live, {candidate: (total, redundant at min_observations = 3)})"""
    live = np.ones(capacity, np.uint8)
    common = np.arange(100, dtype=np.int32)
    tables = [common.copy() for _ in range(3)]
    want = {}
    own = 200
    for k, (total, shared) in enumerate([(10, 5), (11, 6), (10, 9), (20, 19)], start=3):
        t = np.concatenate([common[10 * k:10 * k + shared], np.arange(own, own + total - shared)]).astype(np.int32)
        own += total
        tables.append(t[::-1].copy())
        want[k] = (total, shared)
    return tables, [len(t) for t in tables], live, want
