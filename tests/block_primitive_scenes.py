"""Scenes for the workgroup primitives of csrc/block_dev.hpp (ordered append, block sum) at the sizes where they can go wrong: one
below, at and one above a 256-thread round, two rounds and one, a block index past the thread count, and a tri_compact_kernel
chunk (1024 pairs) that is exceeded.  Each scene is built from the existing scene modules; tests/test_block_primitives_cpu.py
checks on the specifications that the scenes are what they are for, tests/test_block_primitives_gpu.py runs them.
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
