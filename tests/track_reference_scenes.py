"""Seeded scenes for tracking against the reference keyframe (orbx_track_reference): a frame = (kp, desc, kf_desc, kf_positions,
kf_valid, prior_wc).

Built on tracking_scenes: frame() gives 3-D points in front of a pose, keypoints at their noisy projections plus distractor
features, and per map point the matched feature's descriptor with a few flipped bits.  Here those map-point descriptors are the
keyframe's rows that carry a map point; distractor rows (random descriptors, no map point) are added, some map-point rows lose
their point (holes in `valid`), and the keyframe's rows are shuffled so that keyframe and frame indices differ.
"""
import numpy as np

import tracking_scenes as G

KEYPOINT = G.KEYPOINT
CAMERA = G.CAMERA
TILE = 16                      # keyframe rows per block of tref_nn_kernel (track_ref_kernels.hip: TREF_TILE)
BLOCK = 256                    # threads per block: frame features per pass of tref_nn_kernel, keyframe rows per pass of tref_resolve_kernel


def from_track_frame(f, seed, n_distract, holes=0.2):
    """a tracking_scenes frame (kp, desc, positions, mp_desc, search_pose, prior) as a reference-keyframe scene"""
    kp, desc, X, md, _, prior = f
    rng = np.random.default_rng(seed)
    n = len(md)
    kd = np.concatenate([md, rng.integers(0, 256, (n_distract, 32), dtype=np.uint8)])
    pos = np.concatenate([X, rng.uniform(-5.0, 5.0, (n_distract, 3))])
    valid = np.concatenate([rng.uniform(size=n) >= holes, np.zeros(n_distract, bool)]).astype(np.uint8)
    perm = rng.permutation(n + n_distract)
    return (kp, desc, np.ascontiguousarray(kd[perm]), np.ascontiguousarray(pos[perm]), np.ascontiguousarray(valid[perm]), prior)


def ref_frame(seed, n_kf, n_feat, holes=0.2):
    """a keyframe of n_kf rows, about 60 % of them map points seen in a frame of n_feat features"""
    n_mp = max(1, min(n_kf, (3 * n_kf + 4) // 5))
    f = G.frame(seed, n_mp, max(n_feat, 1))
    s = from_track_frame(f, seed + 1000, max(n_kf - n_mp, 0), holes)
    return (s[0][:n_feat], s[1][:n_feat], s[2][:n_kf], s[3][:n_kf], s[4][:n_kf], s[5])


def with_valid(s, valid):
    return s[:4] + (np.ascontiguousarray(valid, np.uint8),) + s[5:]


def _random_geometry(rng, n_kf, n_feat):
    kp = G.keypoints(np.stack([rng.uniform(1.0, G.W - 1.0, n_feat), rng.uniform(1.0, G.H - 1.0, n_feat)], 1))
    T = G.pose(rng)
    pos = G.backproject(T, np.stack([rng.uniform(20.0, 700.0, n_kf), rng.uniform(20.0, 460.0, n_kf)], 1), rng.uniform(2.0, 10.0, n_kf))
    return kp, pos, G.perturb(rng, T)


def ties(seed, n_kf=500, n_feat=700, n_base=8):
    """every descriptor is one of n_base rows: whole groups of equal distances in both directions, across blocks and tiles"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_base, 32), dtype=np.uint8)
    kp, pos, prior = _random_geometry(rng, n_kf, n_feat)
    return (kp, base[rng.integers(0, n_base, n_feat)], base[rng.integers(0, n_base, n_kf)], pos, (rng.uniform(size=n_kf) < 0.7).astype(np.uint8), prior)


def identical(seed, n_kf=70, n_feat=300):
    """all descriptors equal: every distance is 0 and the only mutual pair is (0, 0)"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    kp, pos, prior = _random_geometry(rng, n_kf, n_feat)
    return (kp, np.tile(d, (n_feat, 1)), np.tile(d, (n_kf, 1)), pos, np.ones(n_kf, np.uint8), prior)


def n_correspondences(seed, k, extra=3):
    """exactly k mutual matches, all with a map point: tracking_scenes.n_correspondences has k features, each 4 bits from its own
    map point, and `extra` map points with a random descriptor (nobody's nearest neighbour)"""
    f = G.n_correspondences(seed, k, extra)
    return (f[0], f[1], f[3], f[2], np.ones(len(f[2]), np.uint8), f[5])


def no_model(seed, n_kf=40, n_feat=60):
    """every keyframe row carries the position of the row seven places on: the matches are as good as ever, but no pose explains
    five of the correspondences, so no PnP hypothesis passes and PnP reports NO_MODEL with the prior's bytes"""
    s = ref_frame(seed, n_kf, n_feat, holes=0.0)
    return s[:3] + (np.ascontiguousarray(np.roll(s[3], 7, axis=0)),) + s[4:]


def shared_keyframe(seed):
    """three frames with different counts; frames 0 and 2 name the same keyframe (frame 2: a shuffled subset of frame 0's features
    with a few more flipped bits)"""
    a = ref_frame(seed, 130, 200)
    rng = np.random.default_rng(seed + 2000)
    pick = rng.permutation(len(a[0]))[:150]
    desc2 = np.stack([G.flip(rng, a[1][i], rng.integers(0, 6)) for i in pick])
    c = (a[0][pick].copy(), desc2, a[2], a[3], a[4], G.perturb(rng, a[5]))
    return [a, ref_frame(seed + 1, BLOCK + 1, 90), c]


# The batches the GPU test runs: name -> list of frames.  (n_kf, n_feat) are the smallest sizes at which the kernels can go wrong:
# one row / one feature, below and at a tile, one either side of TILE and BLOCK keyframe rows and of BLOCK frame features, a thin
# table either way, an empty side, and one table of the size a tracker sees.
def batches():
    return {
        "small": [ref_frame(61, 1, 1), ref_frame(62, 15, 17), ref_frame(63, 16, 256)],
        "tile_edges": [ref_frame(64, TILE - 1, 70), ref_frame(65, TILE, 70), ref_frame(66, TILE + 1, 70)],
        "block_edges_keyframe": [ref_frame(67, BLOCK - 1, 100), ref_frame(68, BLOCK, 100), ref_frame(69, BLOCK + 1, 100)],
        "block_edges_frame": [ref_frame(70, 100, BLOCK - 1), ref_frame(71, 100, BLOCK + 1)],
        "thin": [ref_frame(72, 300, 2), ref_frame(73, 2, 300)],
        "empty_sides": [ref_frame(74, 0, 40), ref_frame(75, 40, 0), ref_frame(76, 50, 60)],
        "realistic": [ref_frame(77, 2000, 2000)],
        "ties": [ties(78)],
        "identical": [identical(79)],
        "corr_3_4": [n_correspondences(80, 3), n_correspondences(81, 4)],
        "no_model_next_to_good": [no_model(82), ref_frame(83, 100, 160)],
        "valid_all_zero": [with_valid(ref_frame(84, 60, 90), np.zeros(60, np.uint8))],
        "b3_shared_keyframe": shared_keyframe(85),
    }
