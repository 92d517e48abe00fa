"""Fixed-seed scenes that take loop verification where a map merge takes it (tests/test_loop_verify_world_cpu.py,
tests/test_loop_verify_world_gpu.py): keyframe pairs under any camera, any world rotation, hundreds of metres from the origin,
between maps related by any rotation and scale; Sim3 point sets with an explicit rotation, a point offset and a scale.  The scenes
of tests/loop_verify_scenes.py stay as they are; these are the same construction with the fixed numbers turned into arguments.

A scene, its specification result (tests/loop_verify_spec.py) and the two spreads that set its tolerance are computed once per
process.  The spreads (`spread`): how far a second formulation of Horn's closed form (the 4 x 4 quaternion matrix through
numpy.linalg.eigh) lies from the specification's SVD form on the very points the returned model was fitted to, and how far the
specification's mse lies from the same sum in np.longdouble.  A test bounds the GPU by max(its usual figure, 50 x spread)."""
import functools

import numpy as np

import camera_cases
import loop_verify_scenes as Z
import loop_verify_spec as S
import orientation_cases
import pnp_spec
from pnp_spec import quat_mul

_quat, _R = Z._quat, Z._R
PI = float(np.pi)
AXES = dict(x=(1.0, 0.0, 0.0), y=(0.0, 1.0, 0.0), z=(0.0, 0.0, 1.0), diag=(1.0, 1.0, 1.0), oblique=tuple(orientation_cases.AXIS))
ANGLES = dict(pi=PI, pi_1e9=PI - 1e-9, pi_1e3=PI - 1e-3, a22=2.2)


# ---- keyframe pairs ---------------------------------------------------------------------------------------------------
def world_pair(seed, camera, w, h, G=None, offset=(0.0, 0.0, 0.0), map_rotation=0.08, map_shift=0.5, map_scale=1.0, max_octave=8, behind=0, behind_centre=0,
               n_feat=300, n_common=220, outlier_frac=0.2, noise=0.01, px_noise=0.3, with_nodes=False):
    """loop_verify_scenes.keyframe_pair with its fixed numbers as arguments.  Landmarks are back-projected pixels of the w x h image
    of `camera` at 2-8 m, so the loop keyframe sees all of them whatever the camera.  The true world is turned by the unit
    quaternion G about the origin and shifted by `offset`.  The current keyframe's map is a similarity of the loop keyframe's: turned
    by map_rotation rad about a random axis, shifted by up to map_shift m per axis, and scaled by map_scale (pose translation and
    points_cam).  outlier_frac of the common features carry a wrong stereo point in the current keyframe.  The first `behind`
    common points of the current keyframe are mirrored through its camera plane (z alone), the next `behind_centre` through its
    centre (the whole point, so the pixel stays).  No random draw depends on G, offset, map_scale, behind or
    behind_centre, so two scenes of one seed that differ in those only have the same descriptors and noise."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = camera["fx"], camera["fy"], camera["cx"], camera["cy"]

    def landmarks(n):
        u, v, z = rng.uniform(0, w, n), rng.uniform(0, h, n), rng.uniform(2, 8, n)
        return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    pose_l = np.concatenate([_quat(rng.normal(size=3), 0.4), rng.uniform(-2, 2, 3)])
    Xl = landmarks(n_common)                                                                                # loop camera frame
    X = Xl @ _R(pose_l[:4]).T + pose_l[4:]
    q_c = _quat(rng.normal(size=3), 0.1)
    pose_c_true = np.concatenate([quat_mul(pose_l[:4], q_c), pose_l[4:] + rng.uniform(-0.3, 0.3, 3)])
    Xc = (X - pose_c_true[4:]) @ _R(pose_c_true[:4])
    dq, dt = _quat(rng.normal(size=3), map_rotation), rng.uniform(-1.0, 1.0, 3) * map_shift
    if G is not None:                                                                                       # the world turns: both true poses
        G = np.asarray(G, np.float64)
        pose_l = np.concatenate([quat_mul(G, pose_l[:4]), _R(G) @ pose_l[4:]])
        pose_c_true = np.concatenate([quat_mul(G, pose_c_true[:4]), _R(G) @ pose_c_true[4:]])
    off = np.asarray(offset, np.float64)
    pose_l = np.concatenate([pose_l[:4], pose_l[4:] + off])
    pose_c_true = np.concatenate([pose_c_true[:4], pose_c_true[4:] + off])
    pose_c = np.concatenate([quat_mul(dq, pose_c_true[:4]), map_scale * (_R(dq) @ pose_c_true[4:] + dt)])   # the other map's belief
    base = rng.integers(0, 256, (n_common, 32), dtype=np.uint8)
    n_other = n_feat - n_common

    def side(Xcam, pose, is_cur):
        desc = np.concatenate([Z._flip(rng, base, 8), rng.integers(0, 256, (n_other, 32), dtype=np.uint8)])
        pts = np.concatenate([Xcam + rng.normal(0, noise, Xcam.shape), landmarks(n_other)])
        if is_cur:
            bad = rng.random(n_common) < outlier_frac
            pts[:n_common][bad] += rng.uniform(0.5, 2.0, (int(bad.sum()), 3)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 3))
            pts[:behind, 2] -= 2.2 * pts[:behind, 2]
            pts[behind:behind + behind_centre] *= -1.2
            pts = pts * map_scale
        has = np.ones(n_feat, np.uint8)
        kp = np.zeros(n_feat, Z.KEYPOINT)
        uv = np.stack([fx * Xcam[:, 0] / Xcam[:, 2] + cx, fy * Xcam[:, 1] / Xcam[:, 2] + cy], 1)
        uv = np.concatenate([uv + rng.normal(0, px_noise, uv.shape), np.stack([rng.uniform(0, w, n_other), rng.uniform(0, h, n_other)], 1)])
        kp["x"], kp["y"] = uv[:, 0], uv[:, 1]
        kp["octave"] = rng.integers(0, max_octave, n_feat)
        node = np.concatenate([np.arange(n_common) // 3 + 10, rng.integers(10, 10 + max(n_common // 3, 1) + 40, n_other)]).astype(np.uint32)
        node[n_common:][rng.random(n_other) < 0.2] = S.NODE_NONE
        perm = rng.permutation(n_feat)
        d = dict(desc=desc[perm], points_cam=pts[perm], has_point=has[perm], kp=kp[perm], pose_wc=pose)
        if with_nodes:
            d["node"] = node[perm]
        return d
    return side(Xc, pose_c, True), side(Xl, pose_l, False)


def _case(name):
    c = camera_cases.BY_NAME[name]
    return dict(camera=c["camera"], w=c["w"], h=c["h"])


EUROC = _case("euroc")
WORLD_SEED = 31                                   # the one seed of the world-pose runs; "world_none" is their G = None, zero-offset run
NEAR, FAR = (350.0, -1200.0, 40.0), (1e4, -2e4, 300.0)
FREE = dict(fix_scale=False)

# name -> (world_pair arguments, verify configuration, Sim3 configuration, expected status)
PAIRS = {}
for _cam, _seed in (("euroc", 41), ("kitti", 42), ("square512", 43), ("anisotropic", 44), ("tiny", 45), ("big", 46)):
    PAIRS["cam_" + _cam] = (dict(seed=_seed, **_case(_cam)), {}, {}, S.OK)
PAIRS["world_none"] = (dict(seed=WORLD_SEED, **EUROC), {}, {}, S.OK)
for _n, _G in orientation_cases.PLAIN:
    PAIRS["world_" + _n] = (dict(seed=WORLD_SEED, G=_G, offset=NEAR, **EUROC), {}, {}, S.OK)
PAIRS["world_far"] = (dict(seed=WORLD_SEED, G=orientation_cases.PLAIN[2][1], offset=FAR, **EUROC), {}, {}, S.OK)
PAIRS["merge_pi"] = (dict(seed=51, map_rotation=PI - 0.01, map_shift=300.0, **EUROC), {}, {}, S.OK)
PAIRS["merge_2.4"] = (dict(seed=52, map_rotation=2.4, map_shift=300.0, with_nodes=True, **EUROC), {}, {}, S.OK)
PAIRS["merge_s0.8"] = (dict(seed=53, map_scale=0.8, **EUROC), {}, FREE, S.OK)
PAIRS["merge_s3"] = (dict(seed=54, map_scale=3.0, **EUROC), {}, FREE, S.OK)
PAIRS["merge_s0.8_fixed"] = (dict(seed=53, map_scale=0.8, **EUROC), {}, {}, S.NO_MODEL)
PAIRS["behind"] = (dict(seed=55, behind=12, **EUROC), {}, {}, S.OK)
PAIRS["behind_centre"] = (dict(seed=56, behind_centre=40, **EUROC), {}, {}, S.OK)
WORLD_NAMES = [n for n in PAIRS if n.startswith("world_") and n != "world_none"]
SHIFTED = [n for n in PAIRS if n.startswith("world_") and n != "world_none" or n.startswith("merge_")]      # offset or scale away from 1
CLAMP_OCTAVES = (-3, 40)


@functools.lru_cache(maxsize=None)
def pair(name):
    return world_pair(**PAIRS[name][0])


@functools.lru_cache(maxsize=None)
def pair_spec(name):
    cur, loop = pair(name)
    return S.verify_pair(PAIRS[name][0]["camera"], cur, loop, PAIRS[name][1], PAIRS[name][2])


@functools.lru_cache(maxsize=None)
def clamp_pair(octave):
    """the behind-free control pair of the EuRoC camera with every loop octave set to `octave`"""
    cur, loop = pair("cam_euroc")
    kp = loop["kp"].copy()
    kp["octave"] = octave
    return cur, dict(loop, kp=kp)


@functools.lru_cache(maxsize=None)
def clamp_spec(octave):
    return S.verify_pair(PAIRS["cam_euroc"][0]["camera"], *clamp_pair(octave))


# ---- Sim3 point sets --------------------------------------------------------------------------------------------------
def sim3_world_set(seed, n, outlier_frac, axis=None, angle=0.0, offset=0.0, scale=1.0, noise=0.01):
    """loop_verify_scenes.sim3_points with an explicit rotation (axis, angle; no axis: the identity), the first set offset by
    `offset` m along every axis, and a scale.  The error lives in the second set's metric, so noise and outlier range grow with a
    scale above 1; the matching threshold is threshold_for(scale)."""
    rng = np.random.default_rng(seed)
    p1 = rng.uniform(-5, 5, (n, 3)) + offset
    R = np.eye(3) if axis is None else _R(_quat(axis, angle))
    t = rng.uniform(-3, 3, 3)
    m = max(scale, 1.0)
    p2 = scale * p1 @ R.T + t + rng.normal(0, noise * m, (n, 3))
    bad = rng.random(n) < outlier_frac
    p2[bad] = p2[bad] + rng.uniform(1.0, 8.0, (int(bad.sum()), 3)) * rng.choice([-1.0, 1.0], (int(bad.sum()), 3)) * m
    return p1, p2, dict(R=R, t=t, scale=scale)


def threshold_for(scale):
    return S.SIM3_DEFAULTS["inlier_threshold"] * max(scale, 1.0)


def exact_set(seed, n, R):
    """points on the 1/8 grid, an exactly representable rotation and translation, no noise: every operation of a fit is exact or
    nearly so, and every non-degenerate hypothesis holds all n points"""
    rng = np.random.default_rng(seed)
    p1 = rng.integers(-40, 41, (n, 3)) / 8.0
    t = np.array([1.5, -2.25, 0.625])
    return p1, p1 @ np.asarray(R, np.float64).T + t, dict(R=np.asarray(R, np.float64), t=t, scale=1.0)


EXACT = dict(rz90=[[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], flip_x=[[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]],
             identity=[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])

# name -> (generator, its arguments, Sim3 configuration)
SIM3_SETS = {}
ROTATION_SEEDS = {}                                # (axis, angle) -> seed, where the first seed tried does not meet the rule
for _i, _ax in enumerate(AXES):
    for _j, _an in enumerate(ANGLES):
        _name = "rot_%s_%s" % (_ax, _an)
        SIM3_SETS[_name] = ("world", dict(seed=ROTATION_SEEDS.get(_name, 400 + 10 * _i + _j), n=80, outlier_frac=0.3, axis=AXES[_ax], angle=ANGLES[_an]), {})
SIM3_SETS["rot_identity"] = ("world", dict(seed=399, n=80, outlier_frac=0.3), {})
ROTATIONS = [n for n in SIM3_SETS if n.startswith("rot_")]
for _k, _R_exact in EXACT.items():
    SIM3_SETS["exact_" + _k] = ("exact", dict(seed=500, n=40, R=_R_exact), dict(max_iterations=1024))
EXACT_SETS = ["exact_" + k for k in EXACT]
H_EDGE_SEED = 778
SIM3_SETS["h_edges"] = ("points", dict(seed=H_EDGE_SEED, n=120, outlier_frac=0.5, noise=0.03), dict(max_iterations=1024))
H_EDGES = (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024)
SIM3_SETS["n3"] = ("points", dict(seed=703, n=3, outlier_frac=0.0), dict(min_inliers=3))
SIM3_SETS["n4"] = ("points", dict(seed=704, n=4, outlier_frac=0.0), dict(min_inliers=3))
for _n in (255, 256, 257, 1000, 2049):
    SIM3_SETS["n%d" % _n] = ("points", dict(seed=700 + _n, n=_n, outlier_frac=0.4), {})
SIM3_SETS["n15"] = ("points", dict(seed=715, n=15, outlier_frac=0.0), {})
SIM3_SETS["n2"] = ("points", dict(seed=702, n=2, outlier_frac=0.0), {})
POINT_COUNTS = ["n3", "n4", "n255", "n256", "n257", "n1000", "n2049"]
for _s in (2009, 2019, 2025):
    SIM3_SETS["unrefined_%d" % _s] = ("points", dict(seed=_s, n=40, outlier_frac=0.55, noise=0.03), {})
for _s in (3068, 3090):
    SIM3_SETS["unrefined_free_%d" % _s] = ("points", dict(seed=_s, n=40, outlier_frac=0.55, noise=0.03, scale=1.4), FREE)
UNREFINED = [n for n in SIM3_SETS if n.startswith("unrefined_")]
for _o, _s in ((1e3, 601), (1e4, 602), (1e5, 603)):
    SIM3_SETS["offset_%g" % _o] = ("world", dict(seed=_s, n=80, outlier_frac=0.3, axis=AXES["oblique"], angle=1.1, offset=_o), {})
OFFSETS = [n for n in SIM3_SETS if n.startswith("offset_")]
for _sc, _s in ((0.05, 611), (0.5, 612), (20.0, 613)):
    SIM3_SETS["scale_%g" % _sc] = ("world", dict(seed=_s, n=80, outlier_frac=0.3, axis=AXES["oblique"], angle=1.1, scale=_sc),
                                   dict(fix_scale=False, inlier_threshold=threshold_for(_sc)))
SCALES = [n for n in SIM3_SETS if n.startswith("scale_")]
for _sc, _s in ((1.02, 621), (0.8, 622)):
    SIM3_SETS["rescaled_%g" % _sc] = ("world", dict(seed=_s, n=80, outlier_frac=0.3, axis=AXES["oblique"], angle=1.1, scale=_sc), {})
RESCALED = [n for n in SIM3_SETS if n.startswith("rescaled_")]
SIM3_STATUS = {"n2": 1, "rescaled_0.8": 1}          # every other set: 0 (OK)
SPREAD_SETS = OFFSETS + SCALES + [n for n in UNREFINED if "free" in n]          # the sets whose tolerance follows max(figure, 50 x spread)


@functools.lru_cache(maxsize=None)
def sim3_set(name):
    gen, kw, _ = SIM3_SETS[name]
    return dict(world=sim3_world_set, exact=exact_set, points=Z.sim3_points)[gen](**kw)


@functools.lru_cache(maxsize=None)
def sim3_spec(name, max_iterations=None):
    p1, p2, _ = sim3_set(name)
    cfg = dict(SIM3_SETS[name][2])
    if max_iterations is not None:
        cfg["max_iterations"] = max_iterations
    return S.sim3_ransac(p1, p2, cfg)


# ---- the two spreads --------------------------------------------------------------------------------------------------
def horn_quaternion(p1, p2, fix_scale):
    """Horn's closed form in its other formulation (Horn 1987, section 4): the unit quaternion of the rotation is the eigenvector of
    the largest eigenvalue of the symmetric 4 x 4 matrix N built from H = sum a b^T.  Returns (q [w, x, y, z], scale, t)."""
    c1, c2 = p1.mean(0), p2.mean(0)
    a, b = p1 - c1, p2 - c2
    H = a.T @ b
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = H
    N = np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                  [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                  [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
                  [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz]])
    q = np.linalg.eigh(N)[1][:, 3]
    scale = 1.0 if fix_scale else float(np.sqrt((b * b).sum() / (a * a).sum()))
    return q, scale, c2 - scale * pnp_spec.quat_R(q) @ c1


def fitted_points(p1, p2, cfg, spec):
    """the indices the specification's returned model was fitted to: the winner's inliers if the refit was kept, else its sample"""
    c = dict(S.SIM3_DEFAULTS); c.update(cfg or {})
    idx = pnp_spec.sample(c["seed"], spec["best_hypothesis"], len(p1), 3)
    if not spec["refined"]:
        return np.array(idx)
    m = S.horn(p1[idx], p2[idx], c["fix_scale"])
    return np.flatnonzero(S.err2(m[2], m[3], p1, p2) < c["inlier_threshold"] ** 2)


def spread(p1, p2, cfg, spec):
    """(model, mse): the largest of rotation angle, relative translation and relative scale between the specification's model and
    horn_quaternion's on the points it was fitted to; the relative difference of its mse to the same sum in np.longdouble"""
    c = dict(S.SIM3_DEFAULTS); c.update(cfg or {})
    p1 = np.asarray(p1, np.float64); p2 = np.asarray(p2, np.float64)
    fit = fitted_points(p1, p2, c, spec)
    q, scale, t = horn_quaternion(p1[fit], p2[fit], c["fix_scale"])
    s = spec["sim3"]
    model = max(pnp_spec.rotation_angle(np.concatenate([q, t]), s[:7]), float(np.linalg.norm(t - s[4:7]) / max(np.linalg.norm(s[4:7]), 1e-12)),
                abs(scale - s[7]) / s[7])
    L = np.longdouble
    inl = spec["inlier"].astype(bool)
    d = p1[inl].astype(L) @ spec["M"].astype(L).T + spec["t"].astype(L) - p2[inl].astype(L)
    mse = (d * d).sum() / L(int(inl.sum()))
    return model, float(abs(L(spec["mse"]) - mse) / mse)


@functools.lru_cache(maxsize=None)
def sim3_spread(name):
    p1, p2, _ = sim3_set(name)
    return spread(p1, p2, SIM3_SETS[name][2], sim3_spec(name))


@functools.lru_cache(maxsize=None)
def pair_spread(name):
    s = pair_spec(name)
    return spread(s["pts_current"], s["pts_loop"], PAIRS[name][2], S.sim3_ransac(s["pts_current"], s["pts_loop"], PAIRS[name][2]))


def tolerances(n_inliers, spreads=None):
    """(bound on rotation, translation and scale; bound on mse): tests/test_loop_verify_gpu.py's figures, or with `spreads` the
    larger of those and 50 x each spread"""
    tol = 1e-9 if n_inliers >= 50 else 1e-8
    if spreads is None:
        return tol, 1e-9
    return max(tol, 50.0 * spreads[0]), max(1e-9, 50.0 * spreads[1])
