"""Seeded scenes for the frame tracker (orbx_track_frames): a frame = (kp, desc, positions, mp_desc, search_pose_wc, prior_wc).

frame(): 3-D points in front of a pose, keypoints at their noisy projections plus distractors (shuffled, so that feature and
map-point indices differ), random frame descriptors, map-point descriptors = the matched feature's with a few flipped bits.
The edge_* builders place keypoints and points by hand for the smallest shapes at which the call can go wrong.
"""
import numpy as np

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CAMERA = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, baseline=0.11007)      # EuRoC cam0
W, H = 752.0, 480.0


def _quat(axis, ang):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(ang / 2.0)], a * np.sin(ang / 2.0)])


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _rot(q, v):
    qv = q[1:]
    t = 2.0 * np.cross(qv, v)
    return v + q[0] * t + np.cross(qv, t)


def pose(rng, rot=0.4, trans=2.0):
    return np.concatenate([_quat(rng.normal(size=3), rng.uniform(0.0, rot)), rng.uniform(-trans, trans, 3)])


def perturb(rng, pose_wc, rot_deg=1.0, trans=0.03):
    q = _qmul(_quat(rng.normal(size=3), np.deg2rad(rot_deg)), pose_wc[:4])
    d = rng.normal(size=3)
    return np.concatenate([q / np.linalg.norm(q), pose_wc[4:] + d * trans / np.linalg.norm(d)])


def backproject(pose_wc, uv, depth, cam=CAMERA):
    """world points that project to uv [n,2] at the given depths in the camera of pose_wc"""
    uv = np.asarray(uv, np.float64).reshape(-1, 2); depth = np.broadcast_to(np.asarray(depth, np.float64), (len(uv),))
    Xc = np.stack([(uv[:, 0] - cam["cx"]) / cam["fx"] * depth, (uv[:, 1] - cam["cy"]) / cam["fy"] * depth, depth], 1)
    return _rot(pose_wc[:4], Xc) + pose_wc[4:]


def keypoints(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    kp = np.zeros(len(xy), KEYPOINT)
    kp["x"] = xy[:, 0]; kp["y"] = xy[:, 1]; kp["size"] = 31.0; kp["angle"] = 0.0; kp["response"] = 1.0
    return kp


def flip(rng, d, nbits):
    """a copy of the 32-byte descriptor with exactly nbits bits flipped"""
    bits = np.unpackbits(np.asarray(d, np.uint8).reshape(32))
    bits[rng.choice(256, int(nbits), replace=False)] ^= 1
    return np.packbits(bits)


def frame(seed, n_mp, n_feat, noise_px=0.5, max_flip=20, behind=0, x_range=(20.0, 710.0), y_range=(20.0, 460.0), camera=None, w=None, h=None):
    """min(n_mp - behind, n_feat) map points with a feature at their noisy projection, `behind` points behind the camera (placed
    first in the list), the other features distractors anywhere in the image.  camera / w / h: another camera and image size (the
    defaults are EuRoC cam0 and 752 x 480; x_range / y_range then have to be given to suit)."""
    rng = np.random.default_rng(seed)
    cam = CAMERA if camera is None else camera
    w = W if w is None else float(w); h = H if h is None else float(h)
    T = pose(rng)
    n_vis = max(n_mp - behind, 0)
    uv = np.stack([rng.uniform(*x_range, n_vis), rng.uniform(*y_range, n_vis)], 1)
    X = np.concatenate([backproject(T, np.stack([rng.uniform(100.0, 600.0, behind), rng.uniform(100.0, 400.0, behind)], 1), -rng.uniform(1.0, 5.0, behind), cam),
                        backproject(T, uv, rng.uniform(2.0, 12.0, n_vis), cam)])
    n_hit = min(n_vis, n_feat)
    xy = np.concatenate([uv[:n_hit] + np.clip(rng.normal(0.0, noise_px, (n_hit, 2)), -2.0, 2.0),
                         np.stack([rng.uniform(1.0, w - 1.0, n_feat - n_hit), rng.uniform(1.0, h - 1.0, n_feat - n_hit)], 1)])
    perm = rng.permutation(n_feat)                      # feature f holds row perm[f]
    inv = np.argsort(perm)
    kp = keypoints(xy[perm])
    desc = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    md = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    for i in range(n_hit):
        md[behind + i] = flip(rng, desc[inv[i]], rng.integers(0, max_flip + 1))
    return (kp, desc, X, md, T, perturb(rng, T))


def with_poses(f, search=None, prior=None):
    return f[:4] + (f[4] if search is None else search, f[5] if prior is None else prior)


def _one(T, uv_mp, xy_feat, desc, md, depth=5.0, prior=None):
    return (keypoints(xy_feat), np.asarray(desc, np.uint8).reshape(-1, 32), backproject(T, uv_mp, depth), np.asarray(md, np.uint8).reshape(-1, 32), T,
            T.copy() if prior is None else prior)


def edge_candidates(seed, n_cand):
    """one map point whose cell range holds exactly n_cand features (all of the frame's), one of them its match"""
    rng = np.random.default_rng(seed)
    T = pose(rng)
    c = np.array([300.3, 200.7])
    xy = c + rng.uniform(-4.0, 4.0, (n_cand, 2))
    desc = rng.integers(0, 256, (n_cand, 32), dtype=np.uint8)
    k = n_cand - 1                                       # the last one visited in its cell
    return _one(T, [c], xy, desc, [flip(rng, desc[k], 7)])


def edge_outside(seed):
    """every point in front but outside [0, 2cx) x [0, 2cy): mode 0 skips them all; mode 1 searches the clamped cells — u = -5
    reaches the first columns, u = -100 (negative max cell) wraps to whole rows, u = 2000 has an empty range"""
    rng = np.random.default_rng(seed)
    T = pose(rng)
    uv = np.array([[-5.0, 100.2], [-5.0, 300.4], [-100.0, 200.6], [2000.0, 240.3], [400.1, -6.0], [740.0, 100.7], [300.2, 497.0]])
    xy = np.array([[3.0, 101.0], [4.0, 299.0], [500.0, 201.0], [740.0, 241.0], [401.0, 2.0], [741.0, 100.0], [301.0, 478.0], [100.0, 50.0]])
    desc = rng.integers(0, 256, (len(xy), 32), dtype=np.uint8)
    md = [flip(rng, desc[i], 5) for i in range(len(uv))]
    return _one(T, uv, xy, desc, md)


def edge_ties(seed):
    """equal best distances in two cells; the lower feature index sits in the LATER cell.  Point 0: both at distance 3 (mode 0
    takes the first cell's, mode 1's ratio test rejects); point 1: both at distance 0 (0 > 0.75 * 0 is false: both modes accept)."""
    rng = np.random.default_rng(seed)
    T = pose(rng)
    uv = np.array([[200.5, 150.5], [500.5, 300.5]])
    xy = np.array([[206.0, 155.0], [195.0, 146.0], [506.0, 305.0], [495.0, 296.0]])       # features 0, 2 in later cells than 1, 3
    d0 = rng.integers(0, 256, 32, dtype=np.uint8); d1 = rng.integers(0, 256, 32, dtype=np.uint8)
    m0 = flip(rng, d0, 3)
    return _one(T, uv, xy, [d0, d0, d1, d1], [m0, d1])


def edge_single(seed):
    """exactly one candidate per point (no ratio test), at distances 90, 100 and 101: TH_HIGH is `<` in mode 0, `<=` in mode 1"""
    rng = np.random.default_rng(seed)
    T = pose(rng)
    uv = np.array([[100.5, 100.5], [300.5, 200.5], [500.5, 300.5], [650.5, 400.5]])
    xy = uv[:3] + 1.0
    desc = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    md = [flip(rng, desc[0], 90), flip(rng, desc[1], 100), flip(rng, desc[2], 101), rng.integers(0, 256, 32, dtype=np.uint8)]
    return _one(T, uv, xy, desc, md)


def edge_ratio(seed):
    """two candidates: best 30 against second 40 (30 > 0.75 * 40 is false: accepted in both modes) and best 31 against second
    40 (rejected by mode 1 only)"""
    rng = np.random.default_rng(seed)
    T = pose(rng)
    uv = np.array([[150.5, 120.5], [550.5, 350.5]])
    xy = np.array([[151.0, 121.0], [153.0, 119.0], [551.0, 351.0], [553.0, 349.0]])
    m0 = rng.integers(0, 256, 32, dtype=np.uint8); m1 = rng.integers(0, 256, 32, dtype=np.uint8)
    bits = rng.permutation(256)

    def far(d, k):                                         # k fixed leading bits of one permutation: distances are exact
        b = np.unpackbits(d); b[bits[:k]] ^= 1
        return np.packbits(b)
    return _one(T, uv, xy, [far(m0, 30), far(m0, 40), far(m1, 31), far(m1, 40)], [m0, m1])


def n_correspondences(seed, k, extra=3):
    """exactly k map points with a feature under them, `extra` more with nothing within the radius"""
    rng = np.random.default_rng(seed)
    T = pose(rng)
    gx, gy = np.meshgrid(np.arange(6) * 100.0 + 80.3, np.arange(4) * 100.0 + 60.7)
    cells = np.stack([gx.ravel(), gy.ravel()], 1)[rng.permutation(24)]
    uv = cells[:k + extra]
    xy = uv[:k] + rng.uniform(-0.7, 0.7, (k, 2))
    desc = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    md = [flip(rng, desc[i], 4) for i in range(k)] + [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(extra)]
    order = rng.permutation(k + extra)
    f = _one(T, uv[order], xy, desc, np.asarray(md)[order], depth=rng.uniform(2.0, 9.0, k + extra), prior=perturb(rng, T))
    return f


def duplicate_inliers(seed, n=40):
    """a clean frame in which map points 5 and 30 are the same point: two inlier correspondences on one feature"""
    f = frame(seed, n, n + 20, noise_px=0.3)
    X, md = f[2].copy(), f[3].copy()
    X[30] = X[5]; md[30] = md[5]
    return (f[0], f[1], X, md, f[4], f[5])


def no_model(seed, n_mp=20, n_feat=40):
    """a clean frame whose PnP prior looks the other way (the search pose turned by 180 degrees): every point is behind the
    prior's camera, no hypothesis started there collects 5 inliers, and PnP reports NO_MODEL with the prior's bytes"""
    f = frame(seed, n_mp, n_feat)
    q = _qmul(_quat([0.0, 1.0, 0.0], np.pi), f[4][:4])
    return with_poses(f, prior=np.concatenate([q / np.linalg.norm(q), f[4][4:]]))


def empty_features(seed, n_mp=6):
    f = frame(seed, n_mp, 8)
    return (f[0][:0], f[1][:0]) + f[2:]


def empty_map(seed, n_feat=30):
    f = frame(seed, 4, n_feat)
    return f[:2] + (f[2][:0], f[3][:0]) + f[4:]


# The batches the GPU test runs (both modes each): name -> list of frames.  Sizes differ per frame; B = 1, 2, 3.
def batches():
    return {
        "b1": [frame(11, 300, 420)],
        "b2": [frame(12, 150, 260, behind=7), frame(13, 70, 50)],
        "b3": [frame(14, 90, 200), frame(15, 257, 300, behind=20), frame(16, 33, 90)],
        "no_features": [empty_features(17)],
        "middle_without_map_points": [frame(18, 40, 80), empty_map(19), frame(20, 25, 60)],
        "mp_1_4_5": [frame(21, 1, 30), frame(22, 4, 30), frame(23, 5, 30)],
        "cand_63_64_65": [edge_candidates(24, 63), edge_candidates(25, 64), edge_candidates(26, 65)],
        "all_behind": [frame(27, 12, 40, behind=12), frame(28, 30, 60)],
        "all_outside": [edge_outside(29)],
        "ties": [edge_ties(30)],
        "single_candidate_th_high": [edge_single(31)],
        "ratio": [edge_ratio(32)],
        "duplicate_inliers": [duplicate_inliers(33)],
        "corr_3_4": [n_correspondences(34, 3), n_correspondences(35, 4)],
        "corr_9_10": [n_correspondences(36, 9), n_correspondences(37, 10)],
        "no_model_next_to_good": [no_model(38), frame(39, 60, 100)],
    }
