"""Synthetic local-mapping scenes for triangulate_from_neighbors: a current keyframe plus T neighbours that share 3-D points.

Neighbour t is of kind t % 4:
  0  0.45 m sideways.  Neighbour 0 has exactly the current keyframe's rotation, so that a feature at the same pixel in both
     gives bit-identical rays — the only way the DLT's |w| < 1e-10 exit is reached (rays parallel to 1e-10 rad);
  1  0.05 m sideways: below the stereo baseline, skipped by the baseline test (:137-141);
  2  0.15 m backwards along the viewing direction: low parallax, so pairs fall to the stereo branches or to SKIPPED, and the
     current camera's centre projects inside the neighbour's image (the crafted REJ_DIST features sit on that epipole);
  3  1.0 m sideways, the other way.
Rotations are small yaw / pitch offsets.  Depths are log-uniform in 1..80 m.  About half the features carry points_cam (the
true camera-frame point scaled by 1 + N(0, 0.01); 5 % of them by 3 or 1/3: gross depth errors).  Octaves agree with the
distance ratio for most pairs and are off by 3 or more levels for 8 %.  3 % of the points are seen by the neighbours at the
image of the mirrored point behind the current camera (same pixel in the current keyframe, positive-depth test fails).
Distractors, map-point flags on both sides and optional node ids (features of one point share a node) complete a keyframe.
"""
import math

import numpy as np

from triangulation_spec import rotation_matrix

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CAMERA = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, baseline=0.11007)
BASELINES = (0.45, 0.05, 0.15, 1.0)
NO_NODE = 0xFFFFFFFF


def _quat(axis, ang):
    axis = np.asarray(axis, np.float64); axis = axis / np.linalg.norm(axis)
    return np.concatenate([[math.cos(ang / 2)], axis * math.sin(ang / 2)])


def _qmul(a, b):
    w1, x1, y1, z1 = a; w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _project(cam, pose, X):
    pc = (X - pose[4:]) @ rotation_matrix(pose[:4])            # R^T (X - t), row-wise
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"], cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]], 1)
    return uv, pc


def _flip(rng, d, p=0.02):
    f = rng.random((len(d), 256)) < p
    return np.packbits(np.unpackbits(d, axis=1, bitorder="little") ^ f.astype(np.uint8), axis=1, bitorder="little")


def _keyframe(n):
    return dict(kp=np.zeros(n, KEYPOINT), desc=np.zeros((n, 32), np.uint8), mp=np.zeros(n, np.uint8), pts=np.zeros((n, 3)),
                has=np.zeros(n, np.uint8), node=np.full(n, NO_NODE, np.uint32))


def make_scene(seed, n_points=350, T=4, n_distract=120, nodes="none", empty=None, full_mp=None, cur_rot=0.0005):
    """Returns dict(camera, current, neighbours [T], gt [T] = int32 [m,2] true (idx1, idx2) pairs incl. the crafted ones).
    cur_rot: the current keyframe's rotation angle.  The reference's search forms R12 as R2^-1 R1^-1 (:428), which is the relative
    rotation only for R1 = I, so scenes that go through the search keep it small; pair-level scenes may turn the camera freely."""
    rng = np.random.default_rng([0x7121, seed])
    cam = dict(CAMERA)
    W, H = 2 * cam["cx"], 2 * cam["cy"]
    q_cur = _quat([0.1, 1.0, 0.05], cur_rot)
    pose_cur = np.concatenate([q_cur, [0.0, 0.0, 0.0]])
    R_cur = rotation_matrix(q_cur)
    poses = []
    for t in range(T):
        kind, b = t % 4, BASELINES[t % 4]
        d = {0: [1.0, 0.02, 0.03], 1: [1.0, -0.05, 0.0], 2: [0.03, 0.02, -1.0], 3: [-1.0, 0.04, 0.08]}[kind]
        d = np.asarray(d) + (rng.normal(0, 0.03, 3) if t >= 4 else 0.0)
        c = R_cur @ (d / np.linalg.norm(d)) * b
        q = q_cur if t == 0 else _qmul(q_cur, _qmul(_quat([0, 1, 0], rng.uniform(-0.03, 0.03)), _quat([1, 0, 0], rng.uniform(-0.02, 0.02))))
        poses.append(np.concatenate([q, c]))
    # shared points, in the current camera's frame
    z = np.exp(rng.uniform(0.0, math.log(80.0), n_points))
    u = rng.uniform(20, W - 20, n_points); v = rng.uniform(20, H - 20, n_points)
    pc_cur = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], 1)
    X = pc_cur @ R_cur.T + pose_cur[4:]
    behind = (rng.random(n_points) < 0.03) & (z < 10)
    pdesc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    pnode = rng.integers(1, 13, n_points).astype(np.uint32)
    o1 = rng.integers(0, 8, n_points)

    def stereo(pc, n):
        has = (rng.random(n) < 0.5).astype(np.uint8)
        s = 1.0 + rng.normal(0, 0.01, n)
        gross = rng.random(n) < 0.05
        s[gross] = np.where(rng.random(gross.sum()) < 0.5, 3.0, 1.0 / 3.0)
        return has, pc * s[:, None] * has[:, None]

    # crafted features (see the module text); appended to the point features before the shuffle
    crafted_cur, crafted_nb = [], {t: [] for t in range(T)}
    if T >= 1 and empty != 0:
        tries = 0
        while len(crafted_nb[0]) < 1 and tries < 200:                     # identical pixel + identical rotation: parallel rays
            tries += 1
            uu, vv = np.float32(rng.uniform(40, W - 40)), np.float32(rng.uniform(40, H - 40))
            xn = np.array([(float(uu) - cam["cx"]) / cam["fx"], (float(vv) - cam["cy"]) / cam["fy"], 1.0])
            r = R_cur @ xn
            if float(r @ r) / (math.sqrt(float(r @ r)) * math.sqrt(float(r @ r))) < 1.0:
                dd = rng.integers(0, 256, (1, 32), dtype=np.uint8)
                crafted_cur.append(dict(x=uu, y=vv, desc=dd, has=1, pts=xn * 1e12, t=0, node=100 + len(crafted_cur)))
                crafted_nb[0].append(dict(x=uu, y=vv, desc=_flip(rng, dd), node=crafted_cur[-1]["node"]))
    t_back = 2 if T > 2 and empty != 2 else None
    if t_back is not None:
        ep, _ = _project(cam, poses[t_back], pose_cur[None, 4:])
        for _ in range(2):                                                # a "stereo point" 1e-7 m in front of the current camera
            uu, vv = np.float32(rng.uniform(40, W - 40)), np.float32(rng.uniform(40, H - 40))
            xn = np.array([(float(uu) - cam["cx"]) / cam["fx"], (float(vv) - cam["cy"]) / cam["fy"], 1.0])
            dd = rng.integers(0, 256, (1, 32), dtype=np.uint8)
            crafted_cur.append(dict(x=uu, y=vv, desc=dd, has=1, pts=xn * 1e-7, t=t_back, node=100 + len(crafted_cur)))
            crafted_nb[t_back].append(dict(x=np.float32(ep[0, 0] + rng.normal(0, 0.3)), y=np.float32(ep[0, 1] + rng.normal(0, 0.3)), desc=_flip(rng, dd),
                                           node=crafted_cur[-1]["node"]))

    def assemble(uv, pc, sel, octv, crafted, all_mp):
        """features = selected points | crafted | distractors, shuffled; returns (keyframe, position of point i or -1, positions of crafted)"""
        m, k = len(sel), len(crafted)
        n = m + k + n_distract
        kf = _keyframe(n)
        has, pts = stereo(pc[sel], m)
        kf["kp"]["x"][:m] = (uv[sel, 0] + rng.normal(0, 0.3, m)).astype(np.float32)
        kf["kp"]["y"][:m] = (uv[sel, 1] + rng.normal(0, 0.3, m)).astype(np.float32)
        kf["kp"]["octave"][:m] = octv[sel]
        kf["desc"][:m] = _flip(rng, pdesc[sel]); kf["has"][:m] = has; kf["pts"][:m] = pts; kf["node"][:m] = pnode[sel]
        kf["has"][:m][behind[sel]] = 0; kf["pts"][:m][behind[sel]] = 0.0
        for j, cf in enumerate(crafted):
            kf["kp"]["x"][m + j] = cf["x"]; kf["kp"]["y"][m + j] = cf["y"]; kf["desc"][m + j] = cf["desc"]
            kf["has"][m + j] = cf.get("has", 0); kf["pts"][m + j] = cf.get("pts", 0.0); kf["node"][m + j] = cf["node"]
        kf["kp"]["x"][m + k:] = rng.uniform(0, W, n_distract).astype(np.float32); kf["kp"]["y"][m + k:] = rng.uniform(0, H, n_distract).astype(np.float32)
        kf["kp"]["octave"][m + k:] = rng.integers(0, 8, n_distract)
        kf["desc"][m + k:] = rng.integers(0, 256, (n_distract, 32), dtype=np.uint8)
        dh, dp = stereo(np.stack([np.zeros(n_distract), np.zeros(n_distract), np.exp(rng.uniform(0, math.log(80.0), n_distract))], 1), n_distract)
        kf["has"][m + k:] = dh; kf["pts"][m + k:] = dp
        kf["node"][m + k:] = np.where(rng.random(n_distract) < 0.3, NO_NODE, rng.integers(1, 13, n_distract)).astype(np.uint32)
        kf["kp"]["size"] = 31.0
        kf["mp"][:] = 1 if all_mp else (rng.random(n) < 0.25)
        kf["mp"][m:m + k] = 1 if all_mp else 0
        perm = rng.permutation(n)
        inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
        for key in ("kp", "desc", "mp", "pts", "has", "node"):
            kf[key] = np.ascontiguousarray(kf[key][perm])
        where = np.full(len(uv), -1, np.int64); where[sel] = inv[:m]
        return kf, where, inv[m:m + k]

    uv_cur, _ = _project(cam, pose_cur, X)
    cur, where_cur, crafted_pos_cur = assemble(uv_cur, pc_cur, np.arange(n_points), o1, crafted_cur, False)
    cur["pose"] = pose_cur
    neighbours, gt = [], []
    for t in range(T):
        if empty == t:
            nb = _keyframe(0); nb["pose"] = poses[t]
            neighbours.append(nb); gt.append(np.zeros((0, 2), np.int32))
            continue
        Xt = np.where(behind[:, None], pose_cur[4:] - 0.5 * (X - pose_cur[4:]), X)         # mirrored through the current centre
        uv, pc = _project(cam, poses[t], Xt)
        ok = np.isfinite(uv).all(1) & (uv[:, 0] > 2) & (uv[:, 0] < W - 2) & (uv[:, 1] > 2) & (uv[:, 1] < H - 2) & ((pc[:, 2] > 0.5) | behind)
        sel = np.nonzero(ok & (rng.random(n_points) < 0.85))[0]
        ratio = np.linalg.norm(X - poses[t][4:], axis=1) / np.linalg.norm(X - pose_cur[4:], axis=1)
        o2 = np.clip(o1 - np.round(np.log(ratio) / math.log(1.2)).astype(np.int64), 0, 7)
        off = rng.random(n_points) < 0.08
        o2 = np.where(off, np.where(o1 >= 4, o1 - 3 - rng.integers(0, 2, n_points), o1 + 3 + rng.integers(0, 2, n_points)), o2)
        nb, where, crafted_pos = assemble(uv, pc, sel, np.clip(o2, 0, 7), crafted_nb[t], full_mp == t)
        nb["pose"] = poses[t]
        pairs = [(where_cur[i], where[i]) for i in sel]
        mine = [j for j, cf in enumerate(crafted_cur) if cf["t"] == t]
        pairs += [(crafted_pos_cur[j], crafted_pos[k]) for k, j in enumerate(mine)]
        neighbours.append(nb); gt.append(np.array(sorted(pairs), np.int32).reshape(-1, 2))
    for kf, keep in [(cur, nodes in ("all", "current"))] + [(nb, nodes == "all") for nb in neighbours]:
        if not keep:
            kf["node"] = None
    return dict(camera=cam, current=cur, neighbours=neighbours, gt=gt)


def pair_set(scene, t, n_pairs, seed=0):
    """n_pairs (idx1, idx2) for the pair-level entry points: the true pairs of neighbour t, repeated as needed, with every fourth
    slot a random pair (wrong correspondences: reprojection, depth and scale rejections)."""
    rng = np.random.default_rng([0x9A1, seed, n_pairs])
    gt = scene["gt"][t]
    n1, n2 = len(scene["current"]["kp"]), len(scene["neighbours"][t]["kp"])
    out = np.zeros((n_pairs, 2), np.int32)
    for i in range(n_pairs):
        out[i] = (rng.integers(0, n1), rng.integers(0, n2)) if i % 4 == 3 else gt[(i - i // 4) % len(gt)]
    return out


# ---- the scenes the GPU tests run (the CPU tests check the spec's branch coverage and near-threshold share on the same ones) ----
PAIR_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)       # around the wave (64) and the 256-thread block of tri_triangulate_kernel
FUSED_CASES = {                                              # T in {1, 3, 10}; kind 1 neighbours (t % 4 == 1) are below the baseline
    "t1_grid": dict(seed=1, T=1),
    "t3_nodes": dict(seed=2, T=3, nodes="all"),
    "t10_grid": dict(seed=3, T=10, empty=4, full_mp=7),
    "t10_nodes_current_only": dict(seed=4, T=10, nodes="current", empty=4, full_mp=7),
    "t10_nodes": dict(seed=5, T=10, nodes="all", empty=4, full_mp=7),
}
_cache = {}


def pair_scene():
    """About 600 features per keyframe, the current camera turned 0.3 rad (no search involved: the pairs are given)."""
    if "pair" not in _cache:
        _cache["pair"] = make_scene(11, n_points=460, T=4, n_distract=140, cur_rot=0.3)
    return _cache["pair"]


def pair_case(n_pairs):
    """(scene, neighbour index, pairs [n_pairs,2]) of the pair-level tests."""
    sc = pair_scene()
    t = (0, 2, 3, 1)[PAIR_COUNTS.index(n_pairs) % 4]
    return sc, t, pair_set(sc, t, n_pairs, seed=7)


def pair_expected(n_pairs, is_inertial=0):
    """[(status, method, p, margin)] of the spec for pair_case(n_pairs); computed once."""
    import triangulation_spec as S
    key = ("pair", n_pairs, is_inertial)
    if key not in _cache:
        sc, t, pairs = pair_case(n_pairs)
        c, nb = sc["current"], sc["neighbours"][t]
        _cache[key] = [S.triangulate_pair(sc["camera"], S.default_config(), is_inertial, c["kp"], c["pts"], c["has"], c["pose"], nb["kp"], nb["pts"],
                                          nb["has"], nb["pose"], int(a), int(b)) for a, b in pairs]
    return _cache[key]


def fused_scene(name):
    if ("scene", name) not in _cache:
        _cache[("scene", name)] = make_scene(**FUSED_CASES[name])
    return _cache[("scene", name)]


def fused_expected(oracle, name, is_inertial):
    """(created, stats, result, evaluated) of the spec for a fused case; computed once."""
    import triangulation_spec as S
    key = ("fused", name, is_inertial)
    if key not in _cache:
        sc = fused_scene(name)
        _cache[key] = S.triangulate_from_neighbors(oracle, sc["camera"], S.default_config(), is_inertial, sc["current"], sc["neighbours"])
    return _cache[key]
