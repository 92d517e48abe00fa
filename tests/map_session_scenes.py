"""A geometrically coherent world that can be stepped: the fixed inputs of a local-mapping session on the resident map, for
tests/map_session_spec.py's model and the device (tests/test_map_session_cpu.py, tests/test_map_session_gpu.py).

session(seed) -> nine keyframes, N_LANDMARKS landmarks 4 to 10 m in front of them, each with a 256-bit descriptor, and the tracker's
prior per keyframe.  It returns no map state: the store starts empty and the keyframes without tables.

Keyframes.  The camera centres lie on a line through the origin, 0.2 to 0.3 m apart (keyframe BIG only 0.06 m behind its
predecessor: closer than the stereo baseline, so the baseline gate fails for that pair; at 0.2 m the far landmarks are below the
parallax gate and the near ones above it), and the rotations stay below MAX_ROT.  An arc with a few degrees of rotation gives the
neighbour phase nothing to do: the reference's search forms R12 as R2^-1 R1^-1 and t12 as -R2^-1 (t1 + t2) (tests/
triangulation_scenes.py, make_scene), which is the relative pose only where the current keyframe does not rotate and the two
centres are parallel vectors, and every keyframe of a session is the current one once.
Features.  250 to 400 per keyframe: a landmark's projection moved by less than 0.4 px with a descriptor 0 to 5 bits off, or
clutter with a random descriptor; about 40 % of the landmark features carry a stereo point, the landmark in the camera frame moved
by less than a millimetre.  Keyframe BIG has 1100 features (MS_CHUNK is 1024, the uniq pass works in blocks of 256), its landmark
features shuffled among the clutter; keyframe EMPTY has none, so the tracker is lost at the step after it and the map is joined
again by fuse.
Margins are tests/map_fuse_scenes.py's: random descriptors are about 128 bits apart, the rows of one landmark at most 10, and every
feature lies within a pixel of its projection where the search radii are 10 px and more.
Duplicates on purpose.  Landmark N_TWINS + i lies within 15 mm of landmark i and its descriptor is TWIN_BITS bits off: at most 10
bits to a point's own feature, 14 to 34 to its look-alike's, 50 is the threshold.  Every keyframe drops about 15 % of the visible
landmarks, so a point meets its look-alike's feature where its own is missing, in the current keyframe (pass B merges) as in a
neighbour (pass A).  Beside them: a current feature that pairs with two neighbours is created twice, and after keyframe EMPTY the
stereo phase creates again what the older keyframes hold.

CAPACITY and the mapper's constants below were chosen from the model's own counts, which tests/test_map_session_cpu.py prints and
asserts.  The model alone (BA by the oracle) gives per step created / dropped / culled / fuse goners / slots handed out again /
near-gate pairs / BA iterations:

  seed 1   0: 80/0/0/0/0/0/0     1: 139/0/0/5/0/0/8    2: 128/0/5/26/10/0/7   3: 83/0/2/39/39/0/7    4: 56/0/1/35/50/0/7
           5: 35/0/1/29/35/0/8   6: 0/0/0/0/0/0/0      7: 82/19/0/46/49/0/7   8: 56/17/0/39/56/0/6
  seed 2   0: 142/0/0/0/0/0/0    1: 166/0/0/8/0/0/7    2: 41/0/16/25/13/0/7   3: 108/0/1/54/47/0/7   4: 60/0/2/47/60/0/9
           5: 59/0/0/46/59/0/7   6: 0/0/0/0/0/0/0      7: 79/27/2/61/56/0/7   8: 64/0/0/49/64/0/7

CAPACITY = 420 (no multiple of 64): the live points peak at 438 (seed 1) and 446 (seed 2) slots wanted at step 7, so the free list
runs short there, and from step 3 on about every slot creation hands out has held a point before.  Keyframe 1 (seed 1, at step 4)
and keyframe 2 (seed 2, at step 3) are flagged redundant and left out from the next step on.  map_fuse_spec.reference_replay's
agreement conditions are met by 3 of 16 passes (seed 1) and 2 of 16 (seed 2): the others have a class of three, a feature matched
twice or a keeper outside the list, which is what the specification exists for.  No pair is within 1e-9 of a triangulation gate.
"""
import numpy as np

import ba_collect_scenes as B
import tracking_scenes as G
from map_fuse_scenes import RADIUS_SCALE, SCALE_RANGE           # the fuse radius and the refresh's scale range, as that scene has them

CAMERA = G.CAMERA
N_KF, BIG, EMPTY = 9, 4, 6
N_LANDMARKS = 420
N_TWINS, TWIN_BITS = 60, 24
CAPACITY = 420
SEEDS = (1, 2)
MAX_ROT = 0.0005                # rad: tests/triangulation_scenes.py's cur_rot
PRIOR_ROT_DEG = 1.2             # the tracker searches from a motion-model guess this far from the keyframe's pose: some features lie outside its radius
# the mapper's constants
TRACK_NBEST = 2                 # the tracker's local map: the previous keyframe and its two best covisibles
N_NEIGHBOURS = 3                # the best covisibles that creation and fuse look at
MAX_FREE = 500                  # the most slots a creation call is handed
GRACE, CULL_MIN_OBS = 2, 2      # a point is a culling candidate once, two steps after its creation
BA_COVISIBLE = 3                # LocalBAConfigLM::max_covisible_keyframes: older keyframes are fixed observers
N_OUTLIERS = 10                 # the worst-reprojecting observations whose points go after BA
KF_MIN_OBS, KF_THRESHOLD = 3, 0.6
MAX_UNLISTED = 1                # keyframes the session leaves out once flagged: the list still reaches eight

_cache = {}


def _poses(rng):
    out = []
    d = np.array([1.0, 0.02, 0.03]); d /= np.linalg.norm(d)
    a = 0.5
    for k in range(N_KF):
        a += 0.0 if k == 0 else (0.06 if k == BIG else rng.uniform(0.2, 0.3))
        out.append(np.concatenate([G._quat(rng.normal(size=3), rng.uniform(0.0, MAX_ROT)), a * d]))
    return np.stack(out)


def session(seed):
    """-> dict(camera, keyframes [9] of dict(kp, desc, pts, has, mp (zeros), node (None), pose, landmark int32 [n]: the landmark
    behind each feature or -1), poses [9,7], landmarks [N,3], landmark_desc [N,32]).  Cached: never modify it."""
    if seed in _cache:
        return _cache[seed]
    rng = np.random.default_rng([0x5E55, seed])
    poses = _poses(rng)
    X = np.stack([rng.uniform(-3.0, 6.0, N_LANDMARKS), rng.uniform(-2.0, 2.0, N_LANDMARKS), rng.uniform(4.0, 10.0, N_LANDMARKS)], 1)
    ldesc = rng.integers(0, 256, (N_LANDMARKS, 32), dtype=np.uint8)
    for i in range(N_TWINS):                                                  # look-alikes: landmark N_TWINS + i beside landmark i
        X[N_TWINS + i] = X[i] + rng.uniform(-0.015, 0.015, 3)
        ldesc[N_TWINS + i] = G.flip(rng, ldesc[i], TWIN_BITS)
    kfs = []
    for k in range(N_KF):
        if k == EMPTY:
            n = 0
            kf = dict(kp=G.keypoints(np.zeros((0, 2))), desc=np.zeros((0, 32), np.uint8), pts=np.zeros((0, 3)), has=np.zeros(0, np.uint8),
                      landmark=np.zeros(0, np.int32))
        else:
            uv, z = B._project(poses[k], X, CAMERA)
            vis = np.flatnonzero((z > 0.5) & (uv[:, 0] > 20.0) & (uv[:, 0] < G.W - 20.0) & (uv[:, 1] > 20.0) & (uv[:, 1] < G.H - 20.0))
            vis = vis[rng.uniform(size=len(vis)) < 0.85]
            n = 1100 if k == BIG else int(rng.integers(250, 401))
            vis = rng.permutation(vis)[:min(len(vis), n - 40)]
            m = len(vis)
            xy = np.concatenate([uv[vis] + rng.uniform(-0.4, 0.4, (m, 2)), np.stack([rng.uniform(1.0, G.W - 1.0, n - m), rng.uniform(1.0, G.H - 1.0, n - m)], 1)])
            desc = np.concatenate([np.stack([G.flip(rng, ldesc[i], rng.integers(0, 6)) for i in vis]), rng.integers(0, 256, (n - m, 32), dtype=np.uint8)])
            q = poses[k][:4] * np.array([1.0, -1.0, -1.0, -1.0])
            pts = np.zeros((n, 3)); has = np.zeros(n, np.uint8)
            pts[:m] = np.stack([G._rot(q, x - poses[k][4:]) for x in X[vis]]) + rng.uniform(-1e-3, 1e-3, (m, 3))
            has[:m] = rng.uniform(size=m) < 0.4
            pts[has == 0] = 0.0
            lm = np.concatenate([vis, np.full(n - m, -1)]).astype(np.int32)
            perm = rng.permutation(n)                                         # landmark features among the clutter, on both sides of 256 and 1024
            kf = dict(kp=G.keypoints(xy[perm]), desc=np.ascontiguousarray(desc[perm]), pts=np.ascontiguousarray(pts[perm]), has=np.ascontiguousarray(has[perm]),
                      landmark=lm[perm])
        kf.update(mp=np.zeros(n, np.uint8), node=None, pose=poses[k].copy())
        kfs.append(kf)
    priors = np.stack([G.perturb(rng, T, rot_deg=PRIOR_ROT_DEG, trans=0.03) for T in poses])
    _cache[seed] = dict(camera=CAMERA, keyframes=kfs, poses=poses, priors=priors, landmarks=X, landmark_desc=ldesc, seed=seed)
    return _cache[seed]
