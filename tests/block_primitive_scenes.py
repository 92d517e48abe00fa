"""Scenes for the workgroup primitives of csrc/block_dev.hpp (ordered append, block sum, scan of counts, counter scan) at the sizes
where they can go wrong: one below, at and one above a 256-thread round, two rounds and one, a block index past the thread count,
a tri_compact_kernel chunk (1024 pairs) that is exceeded; for the scans, segment and observer counts around one and two rounds,
and keypoints that fall only into the counters at a thread edge, a wave edge and the end sentinel of each counting sort.  Each
scene is built from the existing scene modules; tests/test_block_primitives_cpu.py checks on the specifications that the scenes are
what they are for, tests/test_block_primitives_gpu.py runs them.
"""
import numpy as np

import loop_verify_scenes as Z
import track_reference_scenes as R
import tracking_scenes as G
import triangulation_scenes as T

ROUND = 256                                  # threads of the converted kernels: entries per round of the ordered append
SIZES = (255, 256, 257, 513)
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def round_edges(n):
    """the last entry of each 256-round and the first of the next, below n"""
    return [i for i in range(ROUND - 1, n) if i % ROUND in (ROUND - 1, 0)]


# ---- track_frames_device, mode 1 ------------------------------------------------------------------------------------------
def _track_frame(seed, n_mp, n_feat):
    """tracking_scenes.frame with its map points in a seeded random order: frame() lists the points that have a feature first,
    which would put one run of flagged points in front of one run of unflagged ones"""
    f = G.frame(seed, n_mp, n_feat)
    perm = np.random.default_rng(seed + 5000).permutation(n_mp)
    return (f[0], f[1], np.ascontiguousarray(f[2][perm]), np.ascontiguousarray(f[3][perm]), f[4], f[5])


def track_rounds():
    """B = 5 frames of 0, 255, 256, 257 and 513 map points on 200 features: some points match, some have no feature"""
    return _once("track_rounds", lambda: [_track_frame(400 + k, n, 200) for k, n in enumerate((0,) + SIZES)])


def track_many():
    """B = 257 frames of 8 map points and 16 features: block 256 sums the 256 earlier counts in two passes of its strided loop and
    writes offsets[B]"""
    return _once("track_many", lambda: [_track_frame(1000 + b, 8, 16) for b in range(ROUND + 1)])


# ---- track_reference_device -----------------------------------------------------------------------------------------------
def _ref_keyframe(seed, n_kf):
    """a keyframe whose every row is a map point with its feature in the frame (so nearly every row is a mutual match), rows shuffled"""
    return R.from_track_frame(G.frame(seed, n_kf, n_kf + 60), seed + 1000, 0, holes=0.0)


def reference_rounds(live):
    """keyframes of 255, 256, 257 and 513 rows; live: "edges" (only round_edges carry a map point), "all" or "none" """
    def make():
        out = []
        for k, n in enumerate(SIZES):
            s = _once(("ref_kf", n), lambda: _ref_keyframe(500 + k, n))
            v = np.zeros(n, np.uint8)
            if live == "all":
                v[:] = 1
            elif live == "edges":
                v[round_edges(n)] = 1
            out.append(R.with_valid(s, v))
        return out
    return _once(("reference_rounds", live), make)


# ---- verify_loop_candidates, brute-force matcher ----------------------------------------------------------------------------
LOOP_CFG = dict(Z.MATCH_ONLY, match_ratio=2.0, match_max_dist=256)       # nearly every current feature is a match; stops after the gather
LOOP_CFG_SOME = dict(Z.MATCH_ONLY)                                        # the default ratio test: some features match, most do not
LOOP_N2 = 300


def _loop_keyframe(rng, desc, has):
    n = len(desc)
    d = Z.as_keyframe(desc)
    d["points_cam"] = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(1.0, 9.0, n)], 1)
    d["has_point"] = np.ascontiguousarray(has, np.uint8)
    d["pose_wc"] = G.pose(rng)
    return d


def loop_rounds(live):
    """(current, loop) pairs with 255, 256, 257 and 513 current features; live: "all" (every feature has a stereo point) or "edges"
    (of the current features only round_edges have one)"""
    def make():
        out = []
        for k, n in enumerate(SIZES):
            rng = np.random.default_rng(600 + k)
            d1, d2 = Z.descriptor_table(610 + k, n, LOOP_N2)
            has = np.ones(n, np.uint8)
            if live == "edges":
                has[:] = 0; has[round_edges(n)] = 1
            out.append((_loop_keyframe(rng, d1, has), _loop_keyframe(rng, d2, np.ones(LOOP_N2, np.uint8))))
        return out
    return _once(("loop_rounds", live), make)


# ---- triangulate_from_neighbors -------------------------------------------------------------------------------------------
TRI_CHUNK = 1024                             # pairs per round of tri_compact_kernel


def tri_scene():
    """T = 3 neighbours (kinds 0, 1, 2 of triangulation_scenes); the feature count is raised so that neighbour 0's search leaves
    more than TRI_CHUNK pairs: its list takes two rounds and neighbour 2's continues it"""
    return _once("tri", lambda: T.make_scene(21, n_points=3200, T=3, n_distract=200))


def tri_expected(oracle, is_inertial=0):
    import triangulation_spec as S
    sc = tri_scene()
    return _once(("tri_expected", is_inertial),
                 lambda: S.triangulate_from_neighbors(oracle, sc["camera"], S.default_config(), is_inertial, sc["current"], sc["neighbours"]))


# ---- the ordered scan of counts over rounds (cov_seg_kernel, bac_order_kernel) ----------------------------------------------
TINY_CAPACITY = 96
TINY_KFS = 513


def tiny_world(n_kfs=TINY_KFS):
    """-> (tables, n_features, live): keyframe 0 observes slots 0, 1, 2; every other keyframe k has 0-3 features, each on one of
    those three or on [-1, 4 + k // 6) (slots 3 and 40 are not live), every eleventh has no table.  The first n_kfs keyframes of
    one world of TINY_KFS: a frame over all of them has n_kfs selection segments of 0-3 candidates, slots are seen for the first
    time all along them, and about half the keyframes share a point with keyframe 0."""
    def make():
        rng = np.random.default_rng(700)
        tables, counts = [np.array([0, 1, 2], np.int32)], [3]
        for k in range(1, TINY_KFS):
            n = 3 if k == TINY_KFS - 1 else int(rng.integers(0, 4))            # (the one segment of the third round has candidates)
            t = np.where(rng.random(n) < 0.55, rng.integers(0, 3, n), rng.integers(-1, 4 + k // 6, n)).astype(np.int32)
            tables.append(None if k % 11 == 5 else t); counts.append(n)
        live = np.ones(TINY_CAPACITY, np.uint8); live[[3, 40]] = 0
        return tables, counts, live
    tables, counts, live = _once("tiny_world", make)
    return tables[:n_kfs], counts[:n_kfs], live


# (n_kfs, n_best, ref_kf of the call's frames): -1 = every keyframe, S = n_kfs segments; else S = 1 + n_best segments
COV_SEG_CASES = [(64, 62, [-1, 0]), (65, 64, [0, -1]), (255, 2, [-1, 0]), (256, 2, [-1, 0]), (257, 2, [0, -1]), (513, 255, [0, -1]), (513, 256, [0]), (513, 300, [0, 1])]


def cov_seg_expected(n_kfs, n_best, refs):
    """(list_offsets, list_slot, local_kf, keys per frame) of a local-map selection by covisibility_spec and map_store_spec"""
    import covisibility_spec as CV
    import map_store_spec as MS
    tables, _, live = tiny_world(n_kfs)
    keys, rows, lists = [], [], []
    for r in refs:
        k, row = CV.local_keyframes(tables, live, r, n_best)
        keys.append(k); rows.append(row); lists.append(MS.select_keyframes([tables[i] for i in k], live))
    off = np.zeros(len(refs) + 1, np.int32); off[1:] = np.cumsum([len(x) for x in lists])
    return off, np.concatenate(lists).astype(np.int32), np.stack(rows).astype(np.int32), keys


def tiny_frame():
    """a small frame to track: the selection is what the cases are for"""
    f = _once("tiny_frame", lambda: G.frame(707, 8, 16))
    return (f[0], f[1], f[4], f[5])


# (observers n_loc + n_fixed, max_covisible): one round of bac_order_kernel's scan is ROUND observers
BA_ORDER_CASES = [(256, 3), (257, 3), (520, 300)]


def ba_order_world(n_obs):
    """-> (tables, keypoints_xy, live): keyframe 0 (cur) observes slots 0, 1, 2; n_obs - 1 further keyframes have 1-3 features, the
    first on one of those slots (every one observes the window: a local keyframe or a fixed observer), the others on [-1, 5) (slot 3
    is not live); after every eighth stands a keyframe that observes nothing of it: no table, no feature, or -1 and dead slots."""
    import ba_collect_scenes as BC

    def make():
        rng = np.random.default_rng(720 + n_obs)
        tables = [np.array([0, 1, 2], np.int32)]
        for k in range(1, n_obs):
            n = int(rng.integers(1, 4))
            t = rng.integers(-1, 5, n).astype(np.int32)
            t[0] = rng.integers(0, 3)
            tables.append(t[rng.permutation(n)])
            if k % 8 == 0:
                tables.append([None, np.zeros(0, np.int32), np.array([-1, 3], np.int32)][(k // 8) % 3])
        counts = [2 if t is None else len(t) for t in tables]
        live = np.zeros(TINY_CAPACITY, np.uint8); live[:3] = 1; live[4:8] = 1
        return tables, BC.keypoints(720 + n_obs, counts), live
    return _once(("ba_order_world", n_obs), make)


# ---- the counter scan of the four counting sorts ------------------------------------------------------------------------------
# Counters {0, 64 PER - 1, 64 PER, the last}: the first counter of the block, the last of wave 0's last thread, the first of wave
# 1's first thread, and the one whose end is the sentinel (the total).  ONE: every keypoint in a single counter.
SB_ROWS = 4096                               # stereo matcher: row buckets, 4 per thread
STEREO_ROWS = (0, 64 * 4 - 1, 64 * 4, SB_ROWS - 1)
STEREO_ONE = (100,)
GG_COLS, GG_ROWS = 64, 48                    # guided grid: 3072 cells, 3 per thread
GUIDED_CELLS = (0, 64 * 3 - 1, 64 * 3, GG_COLS * GG_ROWS - 1)
GUIDED_ONE = (1000,)
TRI_CELLS = (0, 64 * 4 - 1, 64 * 4, 64 * 64 - 1)   # triangulation grid at 64 x 64 cells of 32 px, 4 per thread
TRI_ONE = (2080,)


def _noisy(rng, desc, p):
    flips = rng.random((len(desc), 256)) < p
    return np.packbits(np.unpackbits(desc, axis=1, bitorder="little") ^ flips.astype(np.uint8), axis=1, bitorder="little")


def stereo_rows(rows, n=240):
    """(kpL, descL, kpR, descR): the right keypoints lie in the image rows `rows` only (row bucket = floor(y); the last bucket also
    takes what lies beyond it); left keypoint i is the partner of right keypoint perm[i]: its row +- 0.4, 1.3 to 120 px to the right,
    its descriptor with a few bits flipped"""
    def make():
        rng = np.random.default_rng([0xB10C, len(rows), int(rows[0])])
        kpL = np.zeros(n, G.KEYPOINT); kpR = np.zeros(n, G.KEYPOINT)
        kpR["y"] = np.asarray(rows, np.float32)[rng.integers(0, len(rows), n)] + rng.uniform(0.05, 0.95, n).astype(np.float32)
        if rows[-1] == SB_ROWS - 1:
            kpR["y"][np.flatnonzero(kpR["y"] >= SB_ROWS - 1)[::3]] += np.float32(700.0)      # rows beyond the last bucket are counted in it
        kpR["x"] = rng.uniform(31.0, 600.0, n).astype(np.float32)
        dR = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        perm = rng.permutation(n)
        kpL["y"] = kpR["y"][perm] + rng.uniform(-0.4, 0.4, n).astype(np.float32)
        kpL["x"] = kpR["x"][perm] + rng.uniform(1.3, 120.0, n).astype(np.float32)
        dL = _noisy(rng, dR[perm], 0.04)
        for kp in (kpL, kpR):
            kp["size"] = 31.0; kp["class_id"] = -1
        return kpL, dL, kpR, dR
    return _once(("stereo_rows", tuple(rows)), make)


def row_bucket(y):
    """match_kernels.hip: row_bucket"""
    y = np.asarray(y, np.float32)
    return np.where(y >= 0, np.minimum(y, SB_ROWS - 1).astype(np.int64), 0)


def _in_cells(rng, cells, n, cw, ch, lo=0.3, hi=0.7):
    c = np.asarray(cells)[rng.integers(0, len(cells), n)]
    return np.stack([(c % 64 + rng.uniform(lo, hi, n)) * cw, (c // 64 + rng.uniform(lo, hi, n)) * ch], 1)


def guided_cells(cells, n=300, nq=200):
    """(kp, desc, q_uv, q_desc) for guided_match at 752 x 480: the keypoints lie in the grid cells `cells` only; the queries are noisy
    copies of keypoints, up to 6 px away"""
    def make():
        rng = np.random.default_rng([0x6C11, len(cells), int(cells[0])])
        kp = G.keypoints(_in_cells(rng, cells, n, G.W / GG_COLS, G.H / GG_ROWS, 0.1, 0.9))
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        src = rng.integers(0, n, nq)
        uv = np.stack([kp["x"][src].astype(np.float64), kp["y"][src].astype(np.float64)], 1) + rng.uniform(-6.0, 6.0, (nq, 2))
        return kp, desc, uv, _noisy(rng, desc[src], 0.05)
    return _once(("guided_cells", tuple(cells)), make)


def guided_cell_of(kp, w=G.W, h=G.H):
    """guided_search_dev.hpp: grid_build_body's cell of a keypoint"""
    sat = lambda v, last: np.clip(np.where(v > 0, np.minimum(v, last + 1.0), 0.0).astype(np.int64), 0, last)
    return sat(kp["y"].astype(np.float64) * (GG_ROWS / h), GG_ROWS - 1) * GG_COLS + sat(kp["x"].astype(np.float64) * (GG_COLS / w), GG_COLS - 1)


def track_cells(cells, n_mp=80, n_extra=40):
    """one frame for track_frames_device whose features (one under every map point, n_extra more) lie in the grid cells `cells` only"""
    def make():
        rng = np.random.default_rng([0x7C11, len(cells), int(cells[0])])
        T = G.pose(rng)
        cw, ch = G.W / GG_COLS, G.H / GG_ROWS
        uv = _in_cells(rng, cells, n_mp, cw, ch)
        xy = np.concatenate([uv + rng.uniform(-2.0, 2.0, (n_mp, 2)), _in_cells(rng, cells, n_extra, cw, ch, 0.1, 0.9)])
        perm = rng.permutation(len(xy))
        desc = rng.integers(0, 256, (len(xy), 32), dtype=np.uint8)
        md = np.stack([G.flip(rng, desc[np.flatnonzero(perm == i)[0]], rng.integers(0, 21)) for i in range(n_mp)])
        return [(G.keypoints(xy[perm]), desc, G.backproject(T, uv, rng.uniform(2.0, 12.0, n_mp)), md, T, G.perturb(rng, T))]
    return _once(("track_cells", tuple(cells)), make)


def track_four_cells():
    return track_cells(GUIDED_CELLS)


def track_one_cell():
    return track_cells(GUIDED_ONE)


def tri_cells(cells, n_per=70, n_distract=60):
    """camera_scenes.two_view's dict at the `grid64` camera (64 x 64 cells of 32 px) with keyframe 2's features in the grid cells
    `cells` only: view-2 pixels are drawn inside the cells, back-projected, and seen from view 1; distractors of keyframe 2 lie in
    the same cells"""
    import camera_cases as CC
    import camera_scenes as CS

    def make():
        case = CC.BY_NAME["grid64"]
        cam, w, h = dict(case["camera"]), float(case["w"]), float(case["h"])
        rng = np.random.default_rng([0x7C31, len(cells), int(cells[0])])
        s = CS.EUROC_FX / cam["fx"]
        pose1 = np.concatenate([CS._quat([0.0, 1.0, 0.0], 0.0005), [0.0, 0.0, 0.0]])
        pose2 = np.concatenate([CS._quat([0.1, 1.0, 0.05], -0.03 * s), np.array([0.45, 0.03, 0.05]) * s])
        n = n_per * len(cells)
        uv2 = _in_cells(rng, cells, n, 32.0, 32.0, 0.1, 0.9)
        X = G.backproject(pose2, uv2, rng.uniform(5.0, 14.0, n), cam)
        uv1, pc1 = CS.project(cam, pose1, X)
        ok = (pc1[:, 2] > 0.5) & (uv1[:, 0] > 0) & (uv1[:, 0] < w) & (uv1[:, 1] > 0) & (uv1[:, 1] < h)
        uv1, uv2 = uv1[ok], uv2[ok]
        m = len(uv1)
        d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        out = dict(camera=cam, pose1_wc=pose1, pose2_wc=pose2)
        xy1 = np.concatenate([uv1 + rng.normal(0, 0.4, (m, 2)), np.stack([rng.uniform(0, w, n_distract), rng.uniform(0, h, n_distract)], 1)])
        xy2 = np.concatenate([uv2 + rng.uniform(-0.4, 0.4, (m, 2)), _in_cells(rng, cells, n_distract, 32.0, 32.0, 0.1, 0.9)])
        for name, xy, dd in (("1", xy1, d), ("2", xy2, _noisy(rng, d, 0.03))):
            kp = np.zeros(len(xy), G.KEYPOINT)
            kp["x"] = np.clip(xy[:, 0], 0.0, np.nextafter(np.float32(w), np.float32(0))).astype(np.float32)
            kp["y"] = np.clip(xy[:, 1], 0.0, np.nextafter(np.float32(h), np.float32(0))).astype(np.float32)
            kp["size"] = 31.0
            kp["octave"] = rng.integers(0, 3, len(xy))
            desc = np.concatenate([dd, rng.integers(0, 256, (n_distract, 32), dtype=np.uint8)])
            perm = rng.permutation(len(xy))
            out["kp" + name] = kp[perm]; out["desc" + name] = desc[perm]
            out["mp" + name] = (rng.random(len(xy)) < 0.3).astype(np.uint8)
        out["stereo1"] = (rng.random(len(xy1)) < 0.5).astype(np.uint8)
        return out
    return _once(("tri_cells", tuple(cells)), make)


def tri_cell_of(kp, cols=64, rows=64):
    """match_kernels.hip: tri_grid_build_body's cell of a keypoint (f32 divide, `as usize`, min)"""
    f = lambda v, last: np.clip(np.where(v > 0, np.minimum(v, last + 1.0), 0.0).astype(np.int64), 0, last)
    return f(kp["y"] / np.float32(32.0), rows - 1) * cols + f(kp["x"] / np.float32(32.0), cols - 1)
