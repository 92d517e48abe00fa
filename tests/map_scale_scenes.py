"""Seeded scenes for the resident map at the size of a real map, on the builders of tests/map_store_scenes.py,
tests/covisibility_scenes.py and tests/map_fuse_scenes.py.  Every scene is there for one path of map_store_kernels.hip that starts
only beyond the sizes of the other map tests; tests/test_map_scale_cpu.py proves from the specifications that it gets there.

big_store()        a store of 2^20 + 7 slots, about 300000 of them live: slot numbers past 2^16 and 2^20, one call naming them all
big_tables()       40 keyframes of 6000 features over it: observation lists of more than 256 chunks of points
frames_scene()     300 frames of one small keyframe and 3 frames of 90 keyframes x 1025 features over one 4096-slot store
rank_world()       covisibility worlds of 1023 ... 2049 keyframes: the ranking tile's border
local_scene()      600 / 1025 keyframes of about 40 features around one trackable frame: a local map over every keyframe
rising_slots()     the slots asked of row_world("rising", 1026): every track length from 0 to 1026
window_world()     1025 keyframes, more than 600 of them fixed observers of keyframe 0's window
merge_world()      one fuse pass with 560 classes of two
observations_sorted()  tests/map_observations_spec.observations restated on sorted arrays, for the big store
"""
import numpy as np

import ba_collect_scenes as B
import covisibility_scenes as V
import map_fuse_scenes as F
import map_store_scenes as M

CHUNK = M.CHUNK
THREADS = 256                                    # map_store_kernels.hip: MS_THREADS, the stride of the chunk-count sums
COV_TILE = 1024                                  # weights the ranking workgroup holds at a time

# ---- scene 1: the big store ---------------------------------------------------------------------------------------------------

BIG_CAPACITY = (1 << 20) + 7
BIG_LIVE = 300000


def big_store(seed=1):
    """-> dict(capacity, positions [capacity,3], desc [capacity,32] (random rows for every slot), slots int32 [BIG_LIVE] (the live
    slots in the shuffled order of the one set call), gone int32 (the half that is erased; slot capacity - 1 and one slot above
    2^20 stay))"""
    rng = np.random.default_rng(seed)
    cap = BIG_CAPACITY
    blocks = np.concatenate([np.arange(0, 100), np.arange(65536 - 50, 65536 + 50), np.arange((1 << 20) - 50, cap)])
    rest = rng.permutation(cap)
    rest = rest[~np.isin(rest, blocks)][:BIG_LIVE - len(blocks)]            # drawn uniformly from the other slots
    slots = rng.permutation(np.concatenate([blocks, rest])).astype(np.int32)
    assert len(slots) == BIG_LIVE == len(np.unique(slots))
    keep = {cap - 1, (1 << 20) + 1, 0, 65536}
    gone = np.array([s for s in slots[::2].tolist() if s not in keep], np.int32)
    positions = rng.uniform(-5.0, 5.0, (cap, 3))
    desc = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    return dict(capacity=cap, positions=positions, desc=desc, slots=slots, gone=gone)


def live_bytes(capacity, slots, gone=()):
    live = np.zeros(capacity, np.uint8)
    live[np.asarray(slots, np.int64)] = 1
    live[np.asarray(gone, np.int64)] = 0
    return live


BIG_KFS, BIG_FEAT = 40, 6000


def big_tables(big, seed=2):
    """40 slot tables of 6000 features over the big store: mostly live slots (the three blocks among them), some -1, some slots
    that are not live, repeats inside a table by the draw"""
    rng = np.random.default_rng(seed)
    slots, cap = big["slots"], big["capacity"]
    tables = []
    for k in range(BIG_KFS):
        t = slots[rng.integers(0, len(slots), BIG_FEAT)].astype(np.int32)
        t[rng.uniform(size=BIG_FEAT) < 0.05] = -1
        dead = rng.uniform(size=BIG_FEAT) < 0.05
        t[dead] = rng.integers(0, cap, int(dead.sum()))                     # (a few of these are live by chance)
        t[:3] = [cap - 1, 65536, 0]
        tables.append(t)
    return tables


def observations_sorted(tables, live, slots):
    """map_observations_spec.observations on arrays: every (keyframe, live slot) pair with the first feature that names it, sorted
    by (place of the slot in `slots`, keyframe) -> (obs_start int32 [M+1], obs_kf int32 [N], obs_feat int32 [N])"""
    live = np.asarray(live)
    slots = np.asarray(slots, np.int64).reshape(-1)
    place = np.full(len(live), -1, np.int64)
    place[slots] = np.arange(len(slots))
    ks, fs, ps = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for k, t in enumerate(tables):
        if t is None:
            continue
        t = np.asarray(t, np.int64).reshape(-1)
        f = np.flatnonzero((t >= 0) & (t < len(live)))
        f = f[live[t[f]] != 0]
        s, first = np.unique(t[f], return_index=True)                       # (the index of the first occurrence)
        asked = place[s] >= 0
        ks.append(np.full(int(asked.sum()), k, np.int64)); fs.append(f[first][asked]); ps.append(place[s][asked])
    k, f, p = np.concatenate(ks), np.concatenate(fs), np.concatenate(ps)
    order = np.lexsort((k, p))
    start = np.zeros(len(slots) + 1, np.int64)
    start[1:] = np.cumsum(np.bincount(p, minlength=len(slots)))
    return start.astype(np.int32), k[order].astype(np.int32), f[order].astype(np.int32)


# ---- scene 2: many frames, many chunks ------------------------------------------------------------------------------------------

N_SMALL_FRAMES, N_SMALL_KFS, N_WIDE_KFS, WIDE_FEAT = 300, 120, 90, 1025


def frames_scene(seed=3):
    """-> dict(live, small [120] / wide [90] slot tables (None: a keyframe without a table), small_n / wide_n their feature counts,
    small_frames [300]: per frame the indices into small (none, one, or two), wide_frames [3]: indices into wide (the middle one
    empty, the third the first reversed))"""
    wide, wide_n, live = V.world(seed, N_WIDE_KFS, sizes=[WIDE_FEAT])
    rng = np.random.default_rng(seed + 1)
    pool = rng.permutation(M.CAPACITY)[:600]
    small, small_n = [], []
    for k in range(N_SMALL_KFS):
        n = int(rng.integers(0, 41))
        t = pool[rng.integers(0, len(pool), n)].astype(np.int32)
        t[rng.uniform(size=n) < 0.1] = -1
        small.append(None if k % 11 == 7 else t); small_n.append(n)
    live = live.copy()
    live[pool[rng.uniform(size=len(pool)) < 0.8]] = 1
    small_frames = []
    for b in range(N_SMALL_FRAMES):
        if b % 13 == 5:
            small_frames.append([])                                         # a frame without keyframes
        elif b % 17 == 3:
            small_frames.append([b % N_SMALL_KFS, (7 * b) % N_SMALL_KFS])
        else:
            small_frames.append([(5 * b) % N_SMALL_KFS])                    # (300 frames over 120 keyframes: most are shared)
    wide_frames = [list(range(N_WIDE_KFS)), [], list(range(N_WIDE_KFS))[::-1]]
    return dict(live=live, small=small, small_n=small_n, wide=wide, wide_n=wide_n, small_frames=small_frames, wide_frames=wide_frames)


def n_chunks(n_cand):
    """workgroups per frame of a selection whose largest frame has n_cand candidates"""
    return max(1, (int(n_cand) + CHUNK - 1) // CHUNK)


# ---- scene 3: keyframes past the ranking tile -----------------------------------------------------------------------------------

RANK_N_KFS = [1023, 1024, 1025, 2049]
RANK_KINDS = ["mixed", "equal", "rising"]
RANK_CAPACITY = 8192                             # (row_world names slots up to 3 * n_kfs)
RANK_SIZES = [63, 64, 65, 255, 257]            # few features: small weights, so most rank decisions are ties


def rank_world(kind, n_kfs):
    """-> (tables, feature counts, live) over a store of RANK_CAPACITY slots"""
    if kind == "mixed":
        return V.world(300 + n_kfs, n_kfs, capacity=RANK_CAPACITY, sizes=RANK_SIZES)
    return V.row_world(kind, n_kfs, capacity=RANK_CAPACITY)


def rank_queries(n_kfs):
    return sorted({q for q in (0, 1023, 1024, n_kfs - 1) if q < n_kfs})


def rank_n_best(n_kfs):
    return [10, 1023, 1024, 1025, n_kfs + 3]


def tie_across(row, i):
    """equal positive weights at indices i and i + 1"""
    return i + 1 < len(row) and row[i] > 0 and row[i] == row[i + 1]


def tie_spans(row, i):
    """some positive weight occurs both at or before index i and behind it"""
    row = np.asarray(row)
    return bool(set(row[:i + 1][row[:i + 1] > 0].tolist()) & set(row[i + 1:][row[i + 1:] > 0].tolist()))


# ---- scene 4: a local map over every keyframe -----------------------------------------------------------------------------------

LOCAL_N_KFS = [600, 1025]


def local_scene(n_kfs, seed=70):
    """map_store_scenes.scene (one trackable frame, its 300 points over eight keyframes) and n_kfs - 8 more keyframes of 30 ... 50
    features over the same store: the frame's slots, other live slots with random rows, -1 and slots that are not live.
    -> dict(store, frame, slots (the frame's points), tables [n_kfs])"""
    sc = M.scene(seed, 300, 420, 8)
    st = sc["store"]
    rng = np.random.default_rng(seed + n_kfs)
    free = np.setdiff1d(np.arange(st.capacity), np.concatenate([st.live_slots(), sc["dead"]]))
    more = rng.permutation(free)[:1500].astype(np.int32)
    pos, desc = M.random_rows(seed + 1)
    st.set(more, pos[more], desc[more])
    pool = np.concatenate([sc["slots"], more, sc["dead"], rng.permutation(np.setdiff1d(free, more))[:200].astype(np.int32)])
    tables = list(sc["tables"])
    for k in range(8, n_kfs):
        n = int(rng.integers(30, 51))
        t = pool[rng.integers(0, len(pool), n)].astype(np.int32)
        t[rng.uniform(size=n) < 0.1] = -1
        tables.append(t)
    order = rng.permutation(n_kfs)                                          # the eight keyframes of the frame lie anywhere among them
    return dict(store=st, frame=sc["frame"], slots=sc["slots"], tables=[tables[i] for i in order])


# ---- scene 5: long tracks -------------------------------------------------------------------------------------------------------

RISING_N_KFS = 1026


def rising_slots(seed=5):
    """slots asked of row_world("rising", 1026): the 1025 slots of every track length from 2 to 1026, slots only keyframe 0 or
    only every eighth other keyframe observes (length 1) and 200 slots nobody observes, shuffled"""
    rng = np.random.default_rng(seed)
    n = RISING_N_KFS
    own = 2 * n + np.arange(1, n)[::8]
    nobody = 3 * n + rng.permutation(M.CAPACITY - 3 * n)[:200]
    return rng.permutation(np.concatenate([np.arange(n + 20), own, nobody])).astype(np.int32)


# ---- scene 6: many fixed observers ------------------------------------------------------------------------------------------------

WINDOW_N_KFS = 1025
WINDOW_SIZES = [1, 63, 64, 65, 257]


def window_world(seed=61):
    """-> (tables, feature counts, live, keypoints_xy): keyframe 0 is the current one and has a table"""
    tables, counts, live = V.world(seed, WINDOW_N_KFS, sizes=WINDOW_SIZES)
    return tables, counts, live, B.keypoints(seed, counts)


# ---- scene 7: many merges -------------------------------------------------------------------------------------------------------

MERGE_CAPACITY, MERGE_PAIRS = 2048, 560
MERGE_CUR, MERGE_TGT = 0, [1, 2, 3]


def merge_world(seed=7):
    """map_fuse_scenes.agree_world's classes of two, 560 of them: the current keyframe 0 and five observers name slot s of a
    landmark, one of the targets 1..3 and keyframe 9 name its duplicate s2; the pass keeps s and s2 goes."""
    b = F._Builder(seed + 900, 10, MERGE_CAPACITY)
    rng = b.rng
    for _ in range(MERGE_PAIRS):
        lm = b.landmark(); s, s2 = b.slot(lm), b.slot(lm)
        b.see(0, lm, s)
        for k in (4, 5, 6, 7, 8):
            b.see(k, lm, s)
        x, y = (int(v) for v in rng.permutation([1, 2, 3])[:2])
        b.see(x, lm, s2); b.see(9, lm, s2)
        if rng.uniform() < 0.5:
            b.see(y, lm, -1)
    for _ in range(60):                                                     # associations beside the merges
        lm = b.landmark(); s = b.slot(lm)
        b.see(0, lm, s)
        b.see(int(rng.integers(1, 4)), lm, -1)
    others = [b.slot(b.landmark()) for _ in range(40)]
    for k in range(10):
        b.clutter(k, 20, [int(v) for v in rng.permutation(others)[:10]])
    return b.finish()


# ---- scene 8: the frame count as a grid row ---------------------------------------------------------------------------------------

MAX_GRID_ROWS = 65535
