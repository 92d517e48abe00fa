"""Local-BA windows with the structure of a SLAM map (tests/test_ba_covis_cpu.py, tests/test_ba_covis_gpu.py).

Test infrastructure only.  synth.ba_window and synth.inertial_window are DENSE windows: keyframes 0.15 m apart looking at one cloud, so
nearly every keyframe sees nearly every point, the observations arrive keyframe-major with ascending point index, and there are one to
four fixed observers.  covis_window makes the other kind:

- K + F cameras on a sideways path `step` metres apart (small yaw and height wobble) past a corridor of points `depth` metres away: a
  camera sees a short stretch of the corridor, so the covisibility graph is a band and most keyframe pairs share no point;
- WHICH cameras are fixed is a random subset of the path: fixed and optimised keyframes interleave, and fixed_cw[0] is any of them;
- a camera observes a visible point with probability `keep` (detector misses): short tracks, many points seen once or by fixed
  cameras only, observation counts per keyframe that differ several-fold;
- the observation array is shuffled (a caller walking a hash map of map points) unless `order` says otherwise;
- options put the rarely reached edges in: tracks of exactly 32 / 33 / 64 / 65 / all cameras, observations from the identity pose
  (kf_idx = fixed_idx = -1), optimised keyframes with no or very few observations, whole 16-point tiles without an optimised observer,
  (point, keyframe) pairs observed two and three times.

The returned dict is synth.ba_window's, so every entry point and helper takes it unchanged.
"""
import numpy as np

import orb_slam3_rust_amd as P
from conftest import pose_errors, point_errors

synth = P.synth
ORDERS = ("shuffled", "kf_major", "point_major", "reversed")
LONG_TRACK_LENGTHS = (32, 33, 64, 65, None)             # None: every camera of the window


def rel(a, b):
    """tests/test_ba_gpu.py's _rel: poses [K,7] -> max(rotation angle, relative translation error) over the keyframes; points [M,3] ->
    max relative error"""
    a = np.asarray(a); b = np.asarray(b)
    if a.shape[-1] == 7:
        return max(pose_errors(a, b))
    return point_errors(a, b)


def reorder(obs, order, seed):
    """`obs` (in keyframe-major order: fixed observers by index, then optimised keyframes by index, the identity observer last; ascending
    point index within one) in the order named: "kf_major" as it is, "point_major" regrouped by point (stable), "shuffled" by the seeded
    permutation, "reversed" the shuffled array back to front."""
    assert order in ORDERS
    if order == "kf_major":
        return obs.copy()
    if order == "point_major":
        return obs[np.argsort(obs["mp_idx"], kind="stable")]
    sh = obs[np.random.default_rng([0xC1, seed]).permutation(len(obs))]
    return sh if order == "shuffled" else sh[::-1].copy()


def covis_window(seed, K, F, M, step, keep, depth, order="shuffled", long_tracks=0, identity_observer=0, empty_kf=(), thin_kf=None,
                 fixed_only_block=None, duplicates=0, yaw_rate=0.03, noise_px=1.0, w=752, h=480, camera=None):
    """See the module docstring.  K optimised and F fixed cameras, M points; `depth` = (near, far) in metres.
    long_tracks=n: 5 n points are moved behind the middle of the corridor where every camera sees them, observed by every camera, and
      then cut to tracks of exactly 32, 33, 64, 65 and K + F observations (n of each; all optimised observers kept, fixed ones at random).
    identity_observer=n: n more observations with kf_idx = fixed_idx = -1, of points the identity pose sees, projected through it.
    empty_kf=[k, ...]: optimised keyframe k loses every observation.  thin_kf={k: n}: it keeps n of them (chosen at random).
    fixed_only_block=(j0, j1): points j0 <= j < j1 lose their optimised observers.
    duplicates=n: n (point, optimised keyframe) pairs get a second observation 0.7 px away, every eighth of them a third; with the
      shuffled orders they land at random positions of the array.
    Returns dict(poses_cw [K,7], fixed_cw [F,7], points [M,3], obs, gt_poses_cw, gt_points, camera, fixed_path_idx, opt_path_idx)."""
    cam = dict(synth.EUROC_CAMERA if camera is None else camera)
    rng = np.random.default_rng([0xC0, seed])
    rngo = np.random.default_rng([0xC2, seed])            # the options draw from their own stream: the plain window does not depend on them
    T = K + F
    span = step * T
    pts = np.stack([rng.uniform(-4, span + 4, M), rng.uniform(-2.5, 2.5, M), rng.uniform(depth[0], depth[1], M)], 1)
    long_ids = np.zeros(0, np.int64)
    if long_tracks:
        # |x - camera x| <= span / 2 + 1 must stay inside the image at the cameras' yaw: z >= 2 (span / 2 + 1) fx / cx is ample
        long_ids = np.sort(rngo.choice(M, 5 * long_tracks, replace=False))
        z0 = 2.0 * (span / 2 + 1.0) * cam["fx"] / cam["cx"]
        n = len(long_ids)
        pts[long_ids] = np.stack([span / 2 + rngo.uniform(-1, 1, n), rngo.uniform(-1.5, 1.5, n), rngo.uniform(z0, z0 + 4.0, n)], 1)
    is_long = np.zeros(M, bool); is_long[long_ids] = True
    poses_cw = []
    for k in range(T):
        q_wc = synth._quat_from_axis_angle([0, 1, 0], yaw_rate * np.sin(0.7 * k))
        t_wc = np.array([step * k, 0.05 * np.sin(k), 0.1 * np.cos(0.5 * k)])
        qi = q_wc * np.array([1, -1, -1, -1.0])
        poses_cw.append(np.concatenate([qi, -synth._quat_rot(qi, t_wc)]))
    poses_cw = np.array(poses_cw)
    path = rng.permutation(T)
    fixed_ids = [int(k) for k in path[:F]]; opt_ids = sorted(int(k) for k in path[F:])

    def project(pose):
        pc = synth._quat_rot(pose[:4], pts) + pose[4:]
        u = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]; v = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
        return u, v, (pc[:, 2] > 0.1) & (u >= 0) & (u < w) & (v >= 0) & (v < h)

    parts = []
    for role, ids in (("f", fixed_ids), ("o", opt_ids)):
        for slot, k in enumerate(ids):
            u, v, inside = project(poses_cw[k])
            vis = inside & ((rng.random(M) < keep) | is_long)
            nz = rng.normal(0, noise_px, (M, 2))
            j = np.nonzero(vis)[0]
            o = np.zeros(len(j), P.BA_OBS)
            o["kf_idx"] = slot if role == "o" else -1; o["fixed_idx"] = slot if role == "f" else -1
            o["mp_idx"] = j; o["u"] = u[j] + nz[j, 0]; o["v"] = v[j] + nz[j, 1]
            parts.append(o)
    obs = np.concatenate(parts)
    drop = np.zeros(len(obs), bool)
    for i, j in enumerate(long_ids):
        L = LONG_TRACK_LENGTHS[i % len(LONG_TRACK_LENGTHS)]
        mine = np.nonzero(obs["mp_idx"] == j)[0]
        assert len(mine) == T, "long-track point %d is seen by %d of %d cameras" % (j, len(mine), T)
        if L is not None:
            fx = mine[obs["kf_idx"][mine] < 0]
            drop[rngo.choice(fx, T - L, replace=False)] = True
    if fixed_only_block is not None:
        j0, j1 = fixed_only_block
        drop |= (obs["kf_idx"] >= 0) & (obs["mp_idx"] >= j0) & (obs["mp_idx"] < j1)
    for k in empty_kf:
        drop |= obs["kf_idx"] == k
    for k, n in (thin_kf or {}).items():
        mine = np.nonzero((obs["kf_idx"] == k) & ~drop)[0]
        drop[rngo.choice(mine, len(mine) - n, replace=False)] = True
    obs = obs[~drop]
    extra = []
    if duplicates:
        opt = np.nonzero(obs["kf_idx"] >= 0)[0]
        dup = obs[np.sort(rngo.choice(opt, duplicates, replace=False))].copy()
        dup["u"] += rngo.normal(0, 0.7, len(dup)); dup["v"] += rngo.normal(0, 0.7, len(dup))
        third = dup[::8].copy()
        third["u"] += rngo.normal(0, 0.7, len(third)); third["v"] += rngo.normal(0, 0.7, len(third))
        extra += [dup, third]
    if identity_observer:
        u, v, inside = project(np.array([1.0, 0, 0, 0, 0, 0, 0]))
        j = np.nonzero(inside)[0]
        assert len(j) >= identity_observer, "the identity pose sees %d points" % len(j)
        j = np.sort(rngo.choice(j, identity_observer, replace=False))
        o = np.zeros(len(j), P.BA_OBS)
        o["kf_idx"] = -1; o["fixed_idx"] = -1; o["mp_idx"] = j
        o["u"] = u[j] + rngo.normal(0, noise_px, len(j)); o["v"] = v[j] + rngo.normal(0, noise_px, len(j))
        extra.append(o)
    if extra:
        obs = np.concatenate([obs] + extra)
        # back to keyframe-major: fixed observers, optimised keyframes, the identity observer; ascending point index, duplicates adjacent
        ident = (obs["kf_idx"] < 0) & (obs["fixed_idx"] < 0)
        key = np.where(ident, F + K, np.where(obs["kf_idx"] >= 0, F + obs["kf_idx"], obs["fixed_idx"]))
        obs = obs[np.lexsort((obs["mp_idx"], key))]
    obs = reorder(obs, order, seed)
    init = poses_cw[opt_ids].copy()
    for i in range(len(init)):
        dq = synth._quat_from_axis_angle(rng.normal(0, 1, 3), np.deg2rad(rng.normal(0, 0.5)))
        init[i, :4] = synth._quat_mul(dq, init[i, :4]); init[i, 4:] += rng.normal(0, 0.02, 3)
    init_pts = pts + rng.normal(0, 0.03, pts.shape)
    return dict(poses_cw=init, fixed_cw=poses_cw[fixed_ids].copy(), points=init_pts, obs=obs, gt_poses_cw=poses_cw[opt_ids].copy(),
                gt_points=pts, camera=cam, fixed_path_idx=np.array(fixed_ids), opt_path_idx=np.array(opt_ids))


def thin_and_shuffle(window, keep, seed):
    """`window` (of any generator) with each observation kept with probability `keep` and the rest permuted"""
    rng = np.random.default_rng([0xC3, seed])
    o = window["obs"][rng.random(len(window["obs"])) < keep]
    w = dict(window)
    w["obs"] = o[rng.permutation(len(o))]
    return w


def stats(window):
    """The structure of a window: N, track lengths (observations per point: min, median, max over the observed points, and the set of
    lengths), points with no / one observation, points seen by fixed cameras only, observations per optimised keyframe (array and min,
    median, max), covisibility fill (share of the pairs of different optimised keyframes that share a point), identity observations,
    (point, optimised keyframe) pairs observed more than once."""
    o = window["obs"]; K = len(window["poses_cw"]); M = len(window["points"])
    isopt = o["kf_idx"] >= 0
    tl = np.bincount(o["mp_idx"], minlength=M)
    tl_opt = np.bincount(o["mp_idx"][isopt], minlength=M)
    deg = np.bincount(o["kf_idx"][isopt], minlength=K)
    A = np.zeros((M, K), np.int64); A[o["mp_idx"][isopt], o["kf_idx"][isopt]] = 1
    cov = (A.T @ A) > 0
    off = ~np.eye(K, dtype=bool)
    pair = o["mp_idx"][isopt].astype(np.int64) * K + o["kf_idx"][isopt]
    seen = tl[tl > 0]
    return dict(N=len(o), track=(int(seen.min()), int(np.median(seen)), int(seen.max())), track_lengths=set(int(x) for x in seen),
                zero_obs=int((tl == 0).sum()), one_obs=int((tl == 1).sum()), fixed_only=int(((tl > 0) & (tl_opt == 0)).sum()),
                kf_obs=deg, deg=(int(deg.min()), int(np.median(deg)), int(deg.max())),
                cov_fill=float(cov[off].mean()) if K > 1 else 1.0,
                identity_obs=int(((o["kf_idx"] < 0) & (o["fixed_idx"] < 0)).sum()),
                duplicate_pairs=int((np.unique(pair, return_counts=True)[1] > 1).sum()),
                track_opt=tl_opt)


# ---- the cases (tests/test_ba_covis_cpu.py proves the conditions on them; its docstring holds the measured numbers) -----------------------
# name -> keyword arguments of covis_window.  The first six are the sparse ones.
CASES = {
    "k12_f4": dict(seed=16, K=12, F=4, M=700, step=2.0, keep=0.5, depth=(2, 5)),
    "k20_f12": dict(seed=11, K=20, F=12, M=2000, step=1.5, keep=0.4, depth=(2, 6)),
    "k20_f100": dict(seed=18, K=20, F=100, M=3000, step=1.0, keep=0.3, depth=(2, 8)),
    "k26_f30": dict(seed=38, K=26, F=30, M=2500, step=2.0, keep=0.45, depth=(2, 5)),
    "k49_f60": dict(seed=16, K=49, F=60, M=6000, step=1.2, keep=0.3, depth=(2, 6)),
    "k55_f20": dict(seed=43, K=55, F=20, M=3000, step=1.0, keep=0.35, depth=(2, 6)),
    "long_tracks": dict(seed=34, K=10, F=110, M=600, step=0.15, keep=0.95, depth=(4, 10), long_tracks=2),
    "empty_kf": dict(seed=21, K=10, F=5, M=600, step=1.0, keep=0.5, depth=(2, 6), empty_kf=[3]),
    "thin_kf": dict(seed=21, K=10, F=5, M=600, step=1.0, keep=0.5, depth=(2, 6), thin_kf={3: 2}),
    "tiles_identity_dups": dict(seed=23, K=10, F=5, M=605, step=1.0, keep=0.5, depth=(2, 6), fixed_only_block=(32, 72),
                                identity_observer=40, duplicates=40),
}
SPARSE = ("k12_f4", "k20_f12", "k20_f100", "k26_f30", "k49_f60", "k55_f20")
EDGES = ("long_tracks", "empty_kf", "thin_kf", "tiles_identity_dups")
PREFIX_CASES = ("k12_f4", "k26_f30", "k49_f60")         # compared after 1, 3 and 7 iterations too; their first step must be an accepted one
_cache = {}


def case(name, order="shuffled"):
    """the window of CASES[name] (made once per order and process; treat it as read-only)"""
    if (name, order) not in _cache:
        _cache[(name, order)] = covis_window(order=order, **CASES[name])
    return _cache[(name, order)]


def dense_fits(window):
    """the oracle's dense formulation is used where its matrix stays small: 6 K + 3 M <= 2500"""
    return 6 * len(window["poses_cw"]) + 3 * len(window["points"]) <= 2500


# ---- the thinned inertial scene (3g) --------------------------------------------------------------------------------------------------
INERTIAL_MARGIN = 1e-7


def inertial_scene(oracle):
    """synth.inertial_window(K = 10, M = 400) thinned to 40 % of its observations and shuffled: the first of at most 40 seeds whose oracle
    solve has every accept / reject decision at least INERTIAL_MARGIN (relative) from a tie — the selection of _inertial_scene in
    tests/test_orientation_gpu.py.  Returns (window, oracle result, seed)."""
    from orientation_cases import lm_margin
    for k in range(40):
        seed = 31 + 7919 * k
        w = thin_and_shuffle(synth.inertial_window(seed, 10, 400, P.BA_OBS, n_fixed=2), 0.4, seed)
        o = oracle.inertial_ba_solve(oracle.Camera(**w["camera"]), oracle.inertial_ba_config(), w["poses_wc"], w["velocities"], w["biases"],
                                     w["fixed_cw"], w["points"], w["obs"], w["edge_kf"], w["preint"])
        if o is not None and lm_margin(o["trace"]) >= INERTIAL_MARGIN:
            return w, o, seed
    raise AssertionError("no thinned inertial scene with margins among 40 seeds")


# ---- global BA on covisibility windows (3g): one fixed keyframe ---------------------------------------------------------------------------
GLOBAL_CASES = {
    "global_k20": dict(seed=42, K=20, F=1, M=2000, step=1.5, keep=0.4, depth=(2, 6)),
    "global_k40": dict(seed=47, K=40, F=1, M=4000, step=1.2, keep=0.35, depth=(2, 6)),
}
