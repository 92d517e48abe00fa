"""Seeded synthetic inputs of the shapes BASELINE.json names.

There is no EuRoC data in the build or on the GPU box, so every test and bench input is
generated here: EuRoC-shaped stereo pairs (752x480 u8, rectified, cam0 intrinsics), matcher
descriptor sets, and local-BA windows.  Pure numpy; identical bytes feed the HIP path and the
CPU oracle.
"""
import numpy as np

# Public EuRoC cam0 values; the reference reads them from
# mav0/cam0/sensor.yaml (src/io/euroc.rs:329-359).
EUROC_CAMERA = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, baseline=0.11007)


def stereo_pair(seed, frame, w=752, h=480, n_rect=None, n_disc=None):
    """One rectified stereo pair (left, right) of u8 [h, w] images.

    A mid-grey canvas with random axis-aligned rectangles and discs, each at its own disparity
    (2..60 px at 752 wide, scaled with width), painted far-to-near so that nearer objects occlude;
    rows are identical in both views (rectified), per-pixel noise U[-4,4] is independent.
    """
    rng = np.random.default_rng([0x5EED, seed, frame])
    area = (w * h) / (752.0 * 480.0)
    n_rect = int(600 * area) if n_rect is None else n_rect
    n_disc = int(300 * area) if n_disc is None else n_disc
    n = n_rect + n_disc
    sx = w / 752.0
    disp = rng.uniform(2.0, 60.0, n) * sx
    order = np.argsort(disp, kind="stable")          # far first
    cx = rng.uniform(0, w, n)
    cy = rng.uniform(0, h, n)
    sz_w = rng.integers(6, 61, n)
    sz_h = rng.integers(6, 61, n)
    gray = rng.integers(0, 256, n)
    left = np.full((h, w), 128, np.int16)
    right = np.full((h, w), 128, np.int16)
    yy, xx = np.mgrid[0:64, 0:64]
    for i in order:
        x0 = int(cx[i]) - int(sz_w[i]) // 2
        y0 = int(cy[i]) - int(sz_h[i]) // 2
        d = int(round(disp[i]))
        if i < n_rect:
            ww, hh = int(sz_w[i]), int(sz_h[i])
            for img, xs in ((left, x0), (right, x0 - d)):
                xa, xb = max(xs, 0), min(xs + ww, w)
                ya, yb = max(y0, 0), min(y0 + hh, h)
                if xa < xb and ya < yb:
                    img[ya:yb, xa:xb] = gray[i]
        else:
            r = int(sz_w[i]) // 2
            m = (yy[:2 * r + 1, :2 * r + 1] - r) ** 2 + (xx[:2 * r + 1, :2 * r + 1] - r) ** 2 <= r * r
            for img, xs in ((left, x0), (right, x0 - d)):
                xa, xb = max(xs, 0), min(xs + 2 * r + 1, w)
                ya, yb = max(y0, 0), min(y0 + 2 * r + 1, h)
                if xa < xb and ya < yb:
                    sub = m[ya - y0:yb - y0, xa - xs:xb - xs]
                    img[ya:yb, xa:xb][sub] = gray[i]
    left += rng.integers(-4, 5, (h, w), dtype=np.int16)
    right += rng.integers(-4, 5, (h, w), dtype=np.int16)
    return (np.clip(left, 0, 255).astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8))


def stereo_batch(seed, first_frame, batch, w=752, h=480):
    """[batch, 2, h, w] u8: the layout orbx_process_stereo_batch_device takes."""
    out = np.empty((batch, 2, h, w), np.uint8)
    for b in range(batch):
        out[b, 0], out[b, 1] = stereo_pair(seed, first_frame + b, w, h)
    return out


def matcher_features(seed, n_left, n_right, keypoint_dtype, w=752, h=480):
    """Feature sets for the matcher microbench (SURVEY.md §8d 'Value distributions'):
    256 iid Bernoulli(1/2) bits; 70 % of right descriptors are a left one with Binomial(256,0.06)
    bits flipped, yR = yL + U{-1,0,1}, xR = xL - U[1.3,120]; the rest independent."""
    rng = np.random.default_rng([0xFEA7, seed])
    kpL = np.zeros(n_left, keypoint_dtype)
    kpR = np.zeros(n_right, keypoint_dtype)
    kpL["x"] = rng.uniform(31, w - 31, n_left).astype(np.float32)
    kpL["y"] = rng.uniform(31, h - 31, n_left).astype(np.float32)
    descL = rng.integers(0, 256, (n_left, 32), dtype=np.uint8)
    descR = rng.integers(0, 256, (n_right, 32), dtype=np.uint8)
    kpR["x"] = rng.uniform(31, w - 31, n_right).astype(np.float32)
    kpR["y"] = rng.uniform(31, h - 31, n_right).astype(np.float32)
    n_corr = min(int(0.7 * n_right), n_left)
    src = rng.permutation(n_left)[:n_corr]
    dst = rng.permutation(n_right)[:n_corr]
    flips = rng.random((n_corr, 256)) < 0.06
    bits = np.unpackbits(descL[src], axis=1, bitorder="little") ^ flips.astype(np.uint8)
    descR[dst] = np.packbits(bits, axis=1, bitorder="little")
    kpR["y"][dst] = kpL["y"][src] + rng.integers(-1, 2, n_corr).astype(np.float32)
    kpR["x"][dst] = kpL["x"][src] - rng.uniform(1.3, 120.0, n_corr).astype(np.float32)
    for kp in (kpL, kpR):
        kp["size"] = 31.0
        kp["angle"] = rng.uniform(0, 360, len(kp)).astype(np.float32)
        kp["response"] = rng.uniform(0, 1e-3, len(kp)).astype(np.float32)
        kp["octave"] = 0
        kp["class_id"] = -1
    return kpL, descL, kpR, descR


def _quat_from_axis_angle(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(ang / 2)], axis * np.sin(ang / 2)])


def _quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _quat_rot(q, v):
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return v @ R.T


def _unit_G(G):
    """the world rotation G (w,x,y,z) of a generator, as given; only its norm is checked — its sign is the caller's choice"""
    G = np.asarray(G, np.float64).reshape(4)
    assert abs(np.linalg.norm(G) - 1.0) < 1e-12, "G must be a unit quaternion"
    return G


def _rotate_cw(G, pose_cw):
    """T_cw [..., 7] of a scene turned by G: q_cw G^-1; t_cw is unchanged (R_cw G^T (G X) + t_cw = R_cw X + t_cw)"""
    out = np.array(pose_cw, np.float64, copy=True).reshape(-1, 7)
    Gc = G * np.array([1, -1, -1, -1.0])
    for k in range(len(out)):
        out[k, :4] = _quat_mul(out[k, :4], Gc)
    return out.reshape(np.shape(pose_cw))


def _rotate_wc(G, pose_wc):
    """T_wc [..., 7] of a scene turned by G: (G q_wc, G t_wc)"""
    out = np.array(pose_wc, np.float64, copy=True).reshape(-1, 7)
    for k in range(len(out)):
        out[k, :4] = _quat_mul(G, out[k, :4])
    out[:, 4:] = _quat_rot(G, out[:, 4:])
    return out.reshape(np.shape(pose_wc))


def world_rotation(axis, angle):
    """G for the generators' `G` argument: the rotation by `angle` rad about `axis`, (cos(angle / 2), axis sin(angle / 2)) with no
    sign canonicalisation — angles in (pi, 2 pi) give w < 0 — and w exactly 0 at angle == pi."""
    G = _quat_from_axis_angle(axis, angle)
    if angle == np.pi:
        G[0] = 0.0
    return G


def euroc_orientation(yaw):
    """G that turns a generator's camera (looking along world +z) into EuRoC cam0's (_EUROC_R_WC: optical axis horizontal, image down
    = world down), then turns it by `yaw` rad about world z"""
    return _quat_mul(_quat_from_axis_angle([0.0, 0.0, 1.0], yaw), _quat_from_R(_EUROC_R_WC))


# the quaternion-carrying inputs of each generator: field -> slice of the quaternion in the last axis
_QUAT_FIELDS = dict(poses_cw=slice(0, 4), fixed_cw=slice(0, 4), poses_wc=slice(0, 4), preint=slice(0, 4), prior_wc=slice(0, 4),
                    pose_wc=slice(0, 4), prev_kf_pose_wc=slice(0, 4))


def with_quaternion_signs(scene, signs=-1.0, fields=None):
    """A copy of a generator's scene with the quaternions of its solver inputs multiplied by `signs` — +1 or -1, one number for every
    quaternion or, per field, an array with one sign per row — so that a test can hand a solver either of the two quaternions of each
    rotation (nalgebra does not canonicalise).  `fields` defaults to every input field of _QUAT_FIELDS the scene has (for
    pose_inertial_problem the `preint` field is one row; for inertial_window one row per edge).  Negation is exact: no other bit
    changes."""
    out = dict(scene)
    for f in (fields if fields is not None else [f for f in _QUAT_FIELDS if f in scene]):
        a = np.array(scene[f], np.float64, copy=True)
        rows = a.reshape(-1, a.shape[-1])
        sg = signs[f] if isinstance(signs, dict) else signs
        sg = np.broadcast_to(np.asarray(sg, np.float64).reshape(-1), (len(rows),))
        assert np.all(np.abs(sg) == 1.0)
        rows[:, _QUAT_FIELDS[f]] *= sg[:, None]
        out[f] = rows.reshape(a.shape)
    return out


def ba_window(seed, K, M, obs_dtype, n_fixed_extra=0, w=752, h=480, camera=None, noise_px=1.0,
              perturb=True, G=None):
    """A local-BA window: keyframe k at (0.15k, 0.02 sin k, 0) m with yaw
    0.01k rad; points U[-6,6]xU[-3,3]xU[3,15] m; an observation wherever the projection lands
    inside the image; pixel noise N(0, noise_px); initial poses perturbed (rot N(0,0.5 deg), trans
    N(0,2 cm)), points N(0,3 cm).  Keyframe 0 is the anchor (fixed, fixed_idx 0); the next
    `n_fixed_extra` keyframes are fixed observers too; the remaining K-1-n_fixed_extra are optimised.
    G (a unit quaternion, w x y z) turns the finished scene about the world origin: q_wc -> G q_wc, t_wc -> G t_wc, X -> G X; the
    observations do not change.  G=None leaves the scene as it always was, bit for bit.
    This is the DENSE window (nearly every keyframe sees every point, sorted observations); tests/covis_windows.py makes the sparse, shuffled kind.

    Returns dict(poses_cw [Kopt,7], fixed_cw [F,7], points [M,3], obs, gt_poses_cw, gt_points).
    """
    cam = dict(EUROC_CAMERA if camera is None else camera)
    rng = np.random.default_rng([0xBA, seed])
    pts = np.stack([rng.uniform(-6, 6, M), rng.uniform(-3, 3, M), rng.uniform(3, 15, M)], 1)
    q_wc, t_wc = [], []
    for k in range(K):
        q_wc.append(_quat_from_axis_angle([0, 1, 0], 0.01 * k))
        t_wc.append(np.array([0.15 * k, 0.02 * np.sin(k), 0.0]))
    poses_cw = []
    for k in range(K):
        qi = q_wc[k] * np.array([1, -1, -1, -1.0])
        ti = -_quat_rot(qi, t_wc[k])
        poses_cw.append(np.concatenate([qi, ti]))
    poses_cw = np.array(poses_cw)
    F = 1 + n_fixed_extra
    obs = []
    for k in range(K):
        pc = _quat_rot(poses_cw[k, :4], pts) + poses_cw[k, 4:]
        u = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]
        v = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
        vis = (pc[:, 2] > 0.1) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        nz = rng.normal(0, noise_px, (M, 2)) if noise_px > 0 else np.zeros((M, 2))
        for j in np.nonzero(vis)[0]:
            obs.append((k - F if k >= F else -1, k if k < F else -1, j, 0, u[j] + nz[j, 0], v[j] + nz[j, 1]))
    obs = np.array(obs, dtype=obs_dtype)
    init = poses_cw[F:].copy()
    init_pts = pts.copy()
    if perturb:
        for i in range(len(init)):
            ax = rng.normal(0, 1, 3)
            dq = _quat_from_axis_angle(ax, np.deg2rad(rng.normal(0, 0.5)))
            init[i, :4] = _quat_mul(dq, init[i, :4])
            init[i, 4:] += rng.normal(0, 0.02, 3)
        init_pts += rng.normal(0, 0.03, init_pts.shape)
    if G is not None:
        G = _unit_G(G)
        poses_cw, init = _rotate_cw(G, poses_cw), _rotate_cw(G, init)
        pts, init_pts = _quat_rot(G, pts), _quat_rot(G, init_pts)
    return dict(poses_cw=init, fixed_cw=poses_cw[:F].copy(), points=init_pts, obs=obs,
                gt_poses_cw=poses_cw[F:].copy(), gt_points=pts, camera=cam)


def two_view_features(seed, n_points, keypoint_dtype, n_distractors=300, camera=None, dup=0.0):
    """Two keyframes looking at the same 3D points (for search_for_triangulation): returns
    dict(kp1, desc1, mp1, stereo1, kp2, desc2, mp2, pose1_wc, pose2_wc, camera).  Shared points get descriptors
    that differ in a few bits; `dup` > 0 makes that fraction of the descriptors identical copies (ties and
    competition for the same partner); flags are random."""
    cam = dict(EUROC_CAMERA if camera is None else camera)
    rng = np.random.default_rng([0x7F1, seed])
    w, h = 2.0 * cam["cx"], 2.0 * cam["cy"]
    X = np.stack([rng.uniform(-5, 5, n_points), rng.uniform(-3, 3, n_points), rng.uniform(4, 14, n_points)], 1)
    pose1 = np.concatenate([_quat_from_axis_angle([0, 1, 0], 0.02), [0.0, 0.0, 0.0]])
    pose2 = np.concatenate([_quat_from_axis_angle([0.1, 1, 0.05], -0.03), [0.45, 0.03, 0.05]])

    def project(pose_wc):
        qi = pose_wc[:4] * np.array([1, -1, -1, -1.0])
        pc = _quat_rot(qi, X - pose_wc[4:])
        return np.stack([cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"], cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]], 1), pc[:, 2]

    uv1, z1 = project(pose1)
    uv2, z2 = project(pose2)
    ok = (z1 > 0.5) & (z2 > 0.5) & (uv1[:, 0] > 0) & (uv1[:, 0] < w) & (uv1[:, 1] > 0) & (uv1[:, 1] < h) & \
         (uv2[:, 0] > 0) & (uv2[:, 0] < w) & (uv2[:, 1] > 0) & (uv2[:, 1] < h)
    uv1, uv2 = uv1[ok], uv2[ok]
    m = len(uv1)
    d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    if dup > 0:
        k = int(dup * m)
        d[rng.permutation(m)[:k]] = d[rng.integers(0, max(m // 20, 1), k)]
    flips = rng.random((m, 256)) < 0.03
    d2 = np.packbits(np.unpackbits(d, axis=1, bitorder="little") ^ flips.astype(np.uint8), axis=1, bitorder="little")
    out = {}
    for name, uv, dd in (("1", uv1, d), ("2", uv2, d2)):
        nd = n_distractors
        kp = np.zeros(m + nd, keypoint_dtype)
        kp["x"] = np.concatenate([uv[:, 0] + rng.normal(0, 0.4, m), rng.uniform(0, w, nd)]).astype(np.float32)
        kp["y"] = np.concatenate([uv[:, 1] + rng.normal(0, 0.4, m), rng.uniform(0, h, nd)]).astype(np.float32)
        desc = np.concatenate([dd, rng.integers(0, 256, (nd, 32), dtype=np.uint8)])
        perm = rng.permutation(m + nd)
        out["kp" + name] = kp[perm]; out["desc" + name] = desc[perm]
        out["mp" + name] = (rng.random(m + nd) < 0.3).astype(np.uint8)
    out["stereo1"] = (rng.random(len(out["kp1"])) < 0.5).astype(np.uint8)
    out["pose1_wc"] = pose1; out["pose2_wc"] = pose2; out["camera"] = cam
    return out


def fuse_scene(seed, n_points, n_kfs, n_feat, keypoint_dtype, camera=None, far_fraction=0.1):
    """Map points + target keyframes for the fuse search (search_in_neighbors.rs:273-343): keyframe t sits at
    (0.2t, 0.03 sin t, 0) m with a small yaw; every keyframe sees ~60 % of the points as features (pixel noise
    N(0,1.5), ~4 % descriptor bits flipped), the rest of its n_feat features are random.  Some points lie behind
    the cameras or project outside the image; `far_fraction` of them sit 400-4000 m away so that the depth-scaled
    radius leaves its lower clamp.  Returns dict(positions, mp_desc, kf_poses_wc, kf_feat_offset, kps, descs, camera)."""
    cam = dict(EUROC_CAMERA if camera is None else camera)
    rng = np.random.default_rng([0xF05E, seed])
    w, h = 2.0 * cam["cx"], 2.0 * cam["cy"]
    z = rng.uniform(2, 20, n_points)
    far = rng.random(n_points) < far_fraction
    z[far] = rng.uniform(400, 4000, far.sum())
    z[rng.random(n_points) < 0.05] *= -1.0
    X = np.stack([rng.uniform(-0.9, 1.1, n_points) * z * cam["cx"] / cam["fx"], rng.uniform(-0.9, 1.1, n_points) * z * cam["cy"] / cam["fy"], z], 1)
    mp_desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    poses, kps, descs, off = [], [], [], [0]
    for t in range(n_kfs):
        pose = np.concatenate([_quat_from_axis_angle([0.05, 1, 0.02], 0.015 * t), [0.2 * t, 0.03 * np.sin(t), 0.0]])
        poses.append(pose)
        qi = pose[:4] * np.array([1, -1, -1, -1.0])
        pc = _quat_rot(qi, X - pose[4:])
        with np.errstate(divide="ignore", invalid="ignore"):
            u = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]; v = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
        vis = np.nonzero((pc[:, 2] > 0) & (u >= 0) & (u < w) & (v >= 0) & (v < h) & (rng.random(n_points) < 0.6))[0]
        vis = vis[:n_feat]
        m = len(vis)
        kp = np.zeros(n_feat, keypoint_dtype)
        kp["x"] = np.concatenate([u[vis] + rng.normal(0, 1.5, m), rng.uniform(0, w, n_feat - m)]).astype(np.float32)
        kp["y"] = np.concatenate([v[vis] + rng.normal(0, 1.5, m), rng.uniform(0, h, n_feat - m)]).astype(np.float32)
        kp["octave"] = rng.integers(0, 8, n_feat)
        flips = rng.random((m, 256)) < 0.04
        d = np.packbits(np.unpackbits(mp_desc[vis], axis=1, bitorder="little") ^ flips.astype(np.uint8), axis=1, bitorder="little")
        d = np.concatenate([d, rng.integers(0, 256, (n_feat - m, 32), dtype=np.uint8)])
        perm = rng.permutation(n_feat)
        kps.append(kp[perm]); descs.append(d[perm]); off.append(off[-1] + n_feat)
    return dict(positions=X, mp_desc=mp_desc, kf_poses_wc=np.array(poses), kf_feat_offset=np.array(off, np.int32),
                kps=np.concatenate(kps) if kps else np.zeros(0, keypoint_dtype),
                descs=np.concatenate(descs) if descs else np.zeros((0, 32), np.uint8), camera=cam)


def vocabulary(seed, k=10, depth=3, ragged=False):
    """A synthetic DBoW2-style vocabulary tree (the real ORBvoc.txt is not in the build): node 0 is the root; every
    inner node has k children whose descriptors are the parent's with ~12 % of the bits flipped (so that descents are
    meaningful), leaves carry an IDF-like weight.  Nodes are numbered in the order a DBoW2 text file lists them
    (depth-first, children contiguous).  `ragged`: child counts vary from 1 to 2k (more than the 16 lanes a
    descriptor gets), some branches stop early, a few nodes name a parent that comes later (never linked).
    Returns (parent u32 [n], is_leaf u8 [n], desc u8 [n,32], weight f64 [n])."""
    rng = np.random.default_rng([0xB0, seed])
    parent, leaf, desc, weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]

    def grow(pid, pdesc, level):
        nc = int(rng.integers(1, 2 * k + 1)) if ragged else k
        for _ in range(nc):
            flips = rng.random(256) < 0.12
            d = np.packbits(np.unpackbits(pdesc, bitorder="little") ^ flips.astype(np.uint8), bitorder="little")
            nid = len(parent)
            stop = level + 1 >= depth or (ragged and level >= 1 and rng.random() < 0.2)
            parent.append(pid); leaf.append(1 if stop else 0); desc.append(d)
            weight.append(float(rng.uniform(0.5, 12.0)) if stop else 0.0)
            if not stop:
                grow(nid, d, level + 1)

    grow(0, rng.integers(0, 256, 32, dtype=np.uint8), 0)
    parent = np.array(parent, np.uint32); leaf = np.array(leaf, np.uint8)
    if ragged:   # forward references: load_from_text never links these (mod.rs:196-198)
        for nid in rng.permutation(np.arange(1, len(parent) - 5))[:5]:
            parent[nid] = nid + 3
    return parent, leaf, np.array(desc, np.uint8), np.array(weight, np.float64)


def bow_database(seed, n_keyframes, words_per_kf=1000, n_words=100000, revisit=None, noise=0.08, n_duplicates=0, other_map_every=0,
                 bad_every=0, short_lists_every=0, reach=6):
    """BowVectors of keyframes along a trajectory, for place recognition at scale without descriptors.  Keyframe i stands at place p_i
    (= i, except inside the revisited stretch `revisit` = (first id, length, place it returns to): there p_i = place + (i - first)).
    Every place owns words_per_kf / 8 words of the vocabulary [0, n_words); a keyframe sees the words of the 8 places around its own, so
    neighbours share 7/8 of them and a revisiting keyframe shares them with keyframes far back in id; a fraction `noise` of its words is
    replaced by random ones.  Weights are a per-word IDF-like value times a per-observation jitter, L1-normalised in ascending word id.
      n_duplicates: that many keyframes (outside the revisit stretch, spread over the ids) get the exact BowVector of their predecessor
                    — equal scores for two ids;
      other_map_every / bad_every: every such id (> 0) lies in map 1 / is bad;
      short_lists_every: every such id has only itself and its predecessor in its connected list (too few for a threshold).
    connected[i]: what get_connected_keyframes (detector.rs:232-262) holds for keyframe i — itself and the ids within `reach` of it —
    in a seeded random order standing in for the HashSet's.
    Returns dict(ids u64 [N], maps i32 [N], bad bool [N], words / weights: lists of N arrays, connected: list of N lists of int)."""
    rng = np.random.default_rng([0xB0DB, seed])
    N = int(n_keyframes)
    per_place = max(words_per_kf // 8, 1)
    place = np.arange(N, dtype=np.int64)
    if revisit is not None:
        first, length, back_to = revisit
        place[first:first + length] = back_to + np.arange(min(length, N - first))
    n_places = int(place.max()) + 8 if N else 8
    idf = rng.uniform(0.5, 12.0, n_words)
    # the words of place p: per_place draws (duplicates inside a keyframe's 8 places fall away in the union)
    place_words = rng.integers(0, n_words, (n_places + 8, per_place), dtype=np.int64)
    words, weights = [], []
    for i in range(N):
        w = place_words[place[i]:place[i] + 8].reshape(-1).copy()
        swap = rng.random(len(w)) < noise
        w[swap] = rng.integers(0, n_words, int(swap.sum()))
        w = np.unique(w)
        v = idf[w] * rng.uniform(0.9, 1.1, len(w))
        t = float(np.cumsum(v)[-1]) if len(v) else 0.0      # the norm added in ascending word id (cumsum is sequential), as orbx_bow_vectors sums it
        words.append(w.astype(np.uint32)); weights.append(v / t if t > 0.0 else v)
    if n_duplicates and N > 2:
        lo, hi = (1, N) if revisit is None else (1, revisit[0])
        for j in np.linspace(lo, max(hi - 1, lo), n_duplicates).astype(int):
            if 0 < j < N:
                words[j] = words[j - 1].copy(); weights[j] = weights[j - 1].copy()
    ids = np.arange(N, dtype=np.uint64)
    maps = np.zeros(N, np.int32); bad = np.zeros(N, bool)
    if other_map_every:
        maps[other_map_every::other_map_every] = 1
    if bad_every:
        bad[bad_every::bad_every] = True
    connected = []
    for i in range(N):
        if short_lists_every and i % short_lists_every == short_lists_every - 1:
            c = [i] + ([i - 1] if i else [])
        else:
            c = list(range(max(0, i - reach), min(N, i + reach + 1)))
        connected.append([int(c[k]) for k in rng.permutation(len(c))])
    return dict(ids=ids, maps=maps, bad=bad, words=words, weights=weights, connected=connected)


def write_vocabulary_text(path, parent, is_leaf, desc, weight, k=10, depth=3, junk_lines=True):
    """DBoW2 text format as load_from_text reads it (mod.rs:101-116): header 'k L scoring weighting', then
    'parent_id is_leaf d0..d31 weight' per node (root excluded).  junk_lines adds short lines that the loader skips."""
    with open(path, "w") as f:
        f.write("%d %d 0 0\n" % (k, depth))
        for i in range(1, len(parent)):
            if junk_lines and i % 97 == 0:
                f.write("# %d short line\n\n" % i)
            f.write("%d %d %s %r \n" % (parent[i], is_leaf[i], " ".join(str(int(b)) for b in desc[i]), float(weight[i])))


def png_encode(img, filters="cycle", bit_depth=8, alpha=False, level=6):
    """A PNG file (bytes) of a greyscale image, written with zlib only: `filters` = 'cycle' (row y uses filter type
    y % 5, exercising None/Sub/Up/Average/Paeth), 'none', or an int 0..4; bit_depth 8 or 16 (16: value*257, so the
    high byte is the 8-bit value); alpha adds an opaque alpha channel (colour type 4)."""
    import struct
    import zlib
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    px = img.astype(np.uint16)
    chans = [px * 257 if bit_depth == 16 else px]
    if alpha:
        chans.append(np.full_like(px, 65535 if bit_depth == 16 else 255))
    inter = np.stack(chans, -1)                                            # [h, w, c]
    raw = inter.astype(">u2").view(np.uint8).reshape(h, -1) if bit_depth == 16 else inter.astype(np.uint8).reshape(h, -1)
    bpp = len(chans) * (bit_depth // 8)
    rows = []
    prev = np.zeros(raw.shape[1], np.int32)
    for y in range(h):
        cur = raw[y].astype(np.int32)
        ft = y % 5 if filters == "cycle" else (0 if filters == "none" else int(filters))
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - a
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - ((a + prev) >> 1)
        else:
            p = a + prev - c
            pa, pb, pc = np.abs(p - a), np.abs(p - prev), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
            f = cur - pred
        rows.append(bytes([ft]) + (f & 255).astype(np.uint8).tobytes())
        prev = cur

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", w, h, bit_depth, 4 if alpha else 0, 0, 0, 0)
    z = zlib.compress(b"".join(rows), level)
    half = len(z) // 2                                                     # two IDAT chunks: the stream may be split anywhere
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"tEXt", b"Comment\x00synthetic") + chunk(b"IDAT", z[:half]) + \
        chunk(b"IDAT", z[half:]) + chunk(b"IEND", b"")


def write_euroc_mav0(root, n_frames, seed=0, w=752, h=480, camera=None):
    """A synthetic EuRoC `mav0` directory (cam0/cam1 data.csv + data/*.png + sensor.yaml in the dataset's own layout)
    holding stereo_pair(seed, i) for i < n_frames.  Returns the list of (left, right) arrays written."""
    import os
    cam = dict(EUROC_CAMERA if camera is None else camera)
    pairs = []
    t0 = 1403636579763555584
    # T_BS of the two cameras: cam1 displaced by the baseline along cam0's x axis, both slightly rotated vs. the body
    R = _quat_rot(_quat_from_axis_angle([0.2, -0.1, 1.0], 1.57), np.eye(3)).T
    t_b_c0 = np.array([-0.0216, -0.0647, 0.0098])
    t_b_c1 = t_b_c0 + R @ np.array([cam["baseline"], 0.0, 0.0])
    for c, t in ((0, t_b_c0), (1, t_b_c1)):
        d = os.path.join(root, "cam%d" % c, "data")
        os.makedirs(d, exist_ok=True)
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
        with open(os.path.join(root, "cam%d" % c, "sensor.yaml"), "w") as f:
            f.write("# General sensor definitions.\nsensor_type: camera\ncomment: VI-Sensor cam%d (MT9M034)\n\n" % c)
            f.write("# Sensor extrinsics wrt. the body-frame.\nT_BS:\n  cols: 4\n  rows: 4\n  data: [")
            f.write(",\n         ".join(", ".join(repr(float(v)) for v in T[r]) for r in range(4)))
            f.write("]\n\n# Camera specific definitions.\nrate_hz: 20\nresolution: [%d, %d]\ncamera_model: pinhole\n" % (w, h))
            f.write("intrinsics: [%r, %r, %r, %r] #fu, fv, cu, cv\n" % (cam["fx"], cam["fy"], cam["cx"], cam["cy"]))
            f.write("distortion_model: radial-tangential\ndistortion_coefficients: [0.0, 0.0, 0.0, 0.0]\n")
    rows = []
    for i in range(n_frames):
        L, Rr = stereo_pair(seed, i, w, h)
        pairs.append((L, Rr))
        ts = t0 + 50000000 * i
        name = "%d.png" % ts
        rows.append("%d,%s" % (ts, name))
        for c, img in ((0, L), (1, Rr)):
            with open(os.path.join(root, "cam%d" % c, "data", name), "wb") as f:
                f.write(png_encode(img, filters="cycle" if i % 2 == 0 else (i % 5)))
    for c in (0, 1):
        with open(os.path.join(root, "cam%d" % c, "data.csv"), "w") as f:
            f.write("#timestamp [ns],filename\n" + "\r\n".join(rows) + "\n")
    return pairs


def inertial_window(seed, K, M, obs_dtype, n_fixed=2, dt=0.25, w=752, h=480, camera=None, noise_px=1.0, stereo_fraction=0.5, G=None,
                    euroc_yaw=None):
    """A local inertial-BA window (local_inertial_ba.rs): K consecutive keyframes dt apart on a smooth accelerating
    trajectory (T_wc poses, world velocities, per-keyframe biases), `n_fixed` older keyframes that only observe (T_cw),
    M points.  The preintegrated deltas of edge (k, k+1) are the exact ones of the ground-truth states
    (dR = Ri^T Rj, dv = Ri^T (vj - vi - g dt), dp = Ri^T (pj - pi - vi dt - g dt^2 / 2), imu_factors.rs:66-103) plus a
    little noise; initial states are perturbed.  obs[i]["_pad"] bit 0 marks stereo observations.
    G (a unit quaternion) turns the finished window about the world origin — poses, velocities, fixed observers and points — and the
    deltas dv, dp are then computed again from the turned ground truth against the same world gravity (0, 0, -9.81), with the same
    noise, so the IMU edges stay consistent (dR does not change).  euroc_yaw = a yaw in rad turns it by G euroc_orientation(yaw)
    instead: the cameras then look horizontally and gravity lies in the image plane, as on EuRoC.  G=None and euroc_yaw=None leave the
    window as it always was, bit for bit.
    Returns dict(poses_wc, velocities, biases, fixed_cw, points, obs, edge_kf, preint, camera, gt_*)."""
    cam = dict(EUROC_CAMERA if camera is None else camera)
    rng = np.random.default_rng([0x1BA, seed])
    g = np.array([0.0, 0.0, -9.81])
    tt = (np.arange(-n_fixed, K)) * dt

    def pos(t):
        return np.array([0.6 * t + 0.05 * t * t, 0.08 * np.sin(1.3 * t), 0.03 * np.cos(0.9 * t)])

    def velo(t):
        return np.array([0.6 + 0.1 * t, 0.08 * 1.3 * np.cos(1.3 * t), -0.03 * 0.9 * np.sin(0.9 * t)])

    q_wc = [_quat_mul(_quat_from_axis_angle([0, 1, 0], 0.04 * t), _quat_from_axis_angle([1, 0, 0], 0.02 * np.sin(t))) for t in tt]
    p_wc = [pos(t) for t in tt]
    v_w = [velo(t) for t in tt]
    pts = np.stack([rng.uniform(-5, 7, M), rng.uniform(-3, 3, M), rng.uniform(3, 14, M)], 1)
    obs = []
    for idx in range(len(tt)):
        qi = q_wc[idx] * np.array([1, -1, -1, -1.0])
        pc = _quat_rot(qi, pts - p_wc[idx])
        u = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]; v = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
        vis = (pc[:, 2] > 0.1) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        nz = rng.normal(0, noise_px, (M, 2)) if noise_px > 0 else np.zeros((M, 2))
        st = rng.random(M) < stereo_fraction
        for j in np.nonzero(vis)[0]:
            k = idx - n_fixed
            obs.append((k if k >= 0 else -1, idx if k < 0 else -1, j, int(st[j]), u[j] + nz[j, 0], v[j] + nz[j, 1]))
    obs = np.array(obs, dtype=obs_dtype)
    fixed_cw = []
    for idx in range(n_fixed):
        qi = q_wc[idx] * np.array([1, -1, -1, -1.0])
        fixed_cw.append(np.concatenate([qi, -_quat_rot(qi, p_wc[idx])]))
    gt_poses = np.array([np.concatenate([q_wc[n_fixed + k], p_wc[n_fixed + k]]) for k in range(K)])
    gt_vel = np.array(v_w[n_fixed:])
    edge_kf, preint, noise = [], [], []

    def deltas(gt_poses, gt_vel, k):
        qic = gt_poses[k, :4] * np.array([1, -1, -1, -1.0])
        dv = _quat_rot(qic, gt_vel[k + 1] - gt_vel[k] - g * dt)
        dp = _quat_rot(qic, gt_poses[k + 1, 4:] - gt_poses[k, 4:] - gt_vel[k] * dt - 0.5 * g * dt * dt)
        return dv, dp

    for k in range(K - 1):
        qi, qj = gt_poses[k, :4], gt_poses[k + 1, :4]
        qic = qi * np.array([1, -1, -1, -1.0])
        dR = _quat_mul(qic, qj)
        dv, dp = deltas(gt_poses, gt_vel, k)
        dR = _quat_mul(dR, _quat_from_axis_angle(rng.normal(0, 1, 3), rng.normal(0, 2e-3)))
        edge_kf.append((k, k + 1))
        noise.append((rng.normal(0, 5e-3, 3), rng.normal(0, 2e-3, 3)))
        preint.append(np.concatenate([dR / np.linalg.norm(dR), dv + noise[k][0], dp + noise[k][1], [dt]]))
    poses = gt_poses.copy()
    for k in range(K):
        dq = _quat_from_axis_angle(rng.normal(0, 1, 3), np.deg2rad(rng.normal(0, 0.4)))
        poses[k, :4] = _quat_mul(dq, poses[k, :4])
        poses[k, 4:] += rng.normal(0, 0.02, 3)
    vel = gt_vel + rng.normal(0, 0.05, (K, 3))
    bias = np.concatenate([rng.normal(0, 2e-3, (K, 3)), rng.normal(0, 2e-2, (K, 3))], 1)
    fixed_cw = np.array(fixed_cw).reshape(-1, 7)
    init_pts = pts + rng.normal(0, 0.03, (M, 3))
    if euroc_yaw is not None:
        G = _quat_mul(np.array([1.0, 0.0, 0.0, 0.0]) if G is None else _unit_G(G), euroc_orientation(euroc_yaw))
    if G is not None:
        G = _unit_G(G)
        gt_poses, poses, fixed_cw = _rotate_wc(G, gt_poses), _rotate_wc(G, poses), _rotate_cw(G, fixed_cw)
        gt_vel, vel = _quat_rot(G, gt_vel), _quat_rot(G, vel)
        pts, init_pts = _quat_rot(G, pts), _quat_rot(G, init_pts)
        for k in range(K - 1):
            dv, dp = deltas(gt_poses, gt_vel, k)
            preint[k][4:7] = dv + noise[k][0]
            preint[k][7:10] = dp + noise[k][1]
    return dict(poses_wc=poses, velocities=vel, biases=bias, fixed_cw=fixed_cw, points=init_pts,
                obs=obs, edge_kf=np.array(edge_kf, np.int32).reshape(-1, 2), preint=np.array(preint).reshape(-1, 11), camera=cam,
                gt_poses_wc=gt_poses, gt_velocities=gt_vel, gt_points=pts)


def keypoint_precision(window):
    """The window with its pixel coordinates rounded to f32 and widened again — what the reference's observations are: kp.pt() is a
    cv::Point2f, widened to f64 when the problem is collected (local_ba_lm.rs:870-872)."""
    w = dict(window)
    o = np.array(window["obs"], copy=True)
    o["u"] = o["u"].astype(np.float32).astype(np.float64); o["v"] = o["v"].astype(np.float32).astype(np.float64)
    w["obs"] = o
    return w


def write_ba_batch_file(path, windows, obs_dtype):
    """`windows` (dicts of ba_window) in the layout tests/cpp/ba_batch_driver.cpp reads: int32 W, then per window int32 K, F, M, N |
    poses_cw [K][7] | fixed_cw [F][7] | points [M][3] | obs [N] (orbx_ba_obs)."""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(windows)))
        for w in windows:
            poses = np.ascontiguousarray(w["poses_cw"], np.float64).reshape(-1, 7)
            fixed = np.ascontiguousarray(w["fixed_cw"], np.float64).reshape(-1, 7)
            pts = np.ascontiguousarray(w["points"], np.float64).reshape(-1, 3)
            obs = np.ascontiguousarray(w["obs"], obs_dtype)
            f.write(struct.pack("<iiii", len(poses), len(fixed), len(pts), len(obs)))
            for a in (poses, fixed, pts, obs):
                f.write(a.tobytes())


def read_ba_batch_results(path, windows):
    """out.bin of tests/cpp/ba_batch_driver.cpp -> list of dicts (status, iterations, initial_error, final_error, poses_wc, points)."""
    import struct
    out = []
    with open(path, "rb") as f:
        for w in windows:
            K = len(np.asarray(w["poses_cw"]).reshape(-1, 7)); M = len(np.asarray(w["points"]).reshape(-1, 3))
            status, iters = struct.unpack("<ii", f.read(8))
            e0, e1 = struct.unpack("<dd", f.read(16))
            poses = np.frombuffer(f.read(56 * K), np.float64).reshape(K, 7)
            pts = np.frombuffer(f.read(24 * M), np.float64).reshape(M, 3)
            out.append(dict(status=status, iterations=iters, initial_error=e0, final_error=e1, poses_wc=poses, points=pts))
    return out


def pnp_problem(seed, n, outlier_frac, prior_rot_deg, prior_trans_m, noise_px=0.5, camera=EUROC_CAMERA, w=752, h=480, G=None):
    """A PnP-RANSAC scene (solve_pnp_ransac_detailed, src/geometry/pnp.rs:100-134).  Ground truth T_wc: a rotation of up to 0.5 rad
    about a random axis, position U[-2,2]^3 m.  Each point is drawn as a pixel U[4, w-4] x U[4, h-4] at depth U[1,20] m and
    back-projected, so the points cover the image.  Inlier observations carry Gaussian noise of sigma noise_px with its length
    clipped at 2 px; round(outlier_frac * n) outliers are displaced 30-200 px from their true projection in a random direction —
    a wide margin on both sides of the 8-px threshold.  The prior is the truth turned by prior_rot_deg about a random axis and
    moved by prior_trans_m in a random direction.  G (a unit quaternion) turns the finished scene about the world origin (truth,
    prior and points; the observations do not change); G=None leaves it as it always was, bit for bit.
    Returns points3d [n,3] f64 (world), points2d [n,2] f32, prior_wc / pose_wc [7] (qw,qx,qy,qz,tx,ty,tz), inliers [n] bool, camera."""
    rng = np.random.default_rng(seed)
    cam = camera
    q_wc = _quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.0, 0.5))
    t_wc = rng.uniform(-2.0, 2.0, 3)
    u = rng.uniform(4.0, w - 4.0, n); v = rng.uniform(4.0, h - 4.0, n); d = rng.uniform(1.0, 20.0, n)
    Xc = np.stack([(u - cam["cx"]) / cam["fx"] * d, (v - cam["cy"]) / cam["fy"] * d, d], 1)
    Xw = _quat_rot(q_wc, Xc) + t_wc
    e = rng.normal(0.0, noise_px, (n, 2))
    e *= np.minimum(1.0, 2.0 / np.maximum(np.linalg.norm(e, axis=1), 1e-300))[:, None]
    uv = np.stack([u, v], 1) + e
    inliers = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        ang = rng.uniform(0.0, 2.0 * np.pi, n_out); mag = rng.uniform(30.0, 200.0, n_out)
        uv[idx] = np.stack([u[idx], v[idx]], 1) + np.stack([np.cos(ang), np.sin(ang)], 1) * mag[:, None]
        inliers[idx] = False
    dq = _quat_from_axis_angle(rng.normal(size=3), np.deg2rad(prior_rot_deg))
    dt = rng.normal(size=3)
    dt *= prior_trans_m / np.linalg.norm(dt)
    q_prior = _quat_mul(dq, q_wc)
    pose_wc, prior_wc = np.concatenate([q_wc, t_wc]), np.concatenate([q_prior / np.linalg.norm(q_prior), t_wc + dt])
    if G is not None:
        G = _unit_G(G)
        pose_wc, prior_wc, Xw = _rotate_wc(G, pose_wc), _rotate_wc(G, prior_wc), _quat_rot(G, Xw)
    return dict(points3d=Xw, points2d=uv.astype(np.float32), pose_wc=pose_wc, prior_wc=prior_wc, inliers=inliers, camera=dict(cam))


# EuRoC cam0 in the world frame, roughly: the optical axis horizontal (camera z -> world x), image right -> world -y, image down ->
# world -z
_EUROC_R_WC = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def _quat_from_R(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2.0, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2.0, R[1, 0] - R[0, 1])
    q = np.array([w, x, y, z])
    return q / np.linalg.norm(q)


def _quat_conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def pose_inertial_problem(seed, n, outlier_frac, stereo_frac, init_rot_deg, init_trans_m, near_identity=False, noise_px=0.5, dt=0.05,
                          imu_noise=0.0, camera=EUROC_CAMERA, w=752, h=480, G=None):
    """A pose-inertial scene (pose_inertial_optimization, src/optimizer/pose_inertial_optim.rs:94-216; the tracker's call,
    src/tracking/tracker.rs:476-546).  The previous keyframe: R_i within 0.05 rad of the identity (near_identity) or a EuRoC-like
    orientation (optical axis horizontal, any heading, up to 0.2 rad of tilt), position U[-2,2]^3 m, velocity N(0, 0.5) m/s.  The true
    motion over dt: angular velocity N(0, 0.5) rad/s per axis, acceleration N(0, 1) m/s^2 (0.2 times that near the identity, where
    R_j stays within 0.05 rad), so R_j = R_i Exp(omega dt), v_j = v_i + a dt, p_j = p_i + v_i dt + a dt^2 / 2.  The preintegration
    is the exact one of that motion — delta_rot = R_i^T R_j, delta_vel = R_i^T (v_j - v_i - g dt), delta_pos = R_i^T (p_j - p_i -
    v_i dt - g dt^2 / 2) (imu_factors.rs:84-95), so the truth has a zero IMU residual — plus N(0, imu_noise) on delta_vel / delta_pos.
    Observations of frame j are drawn as pnp_problem draws them (pixels over the image at depth U[1,20] m, inlier noise of sigma
    noise_px clipped at 2 px, round(outlier_frac * n) outliers displaced 30-200 px); round(stereo_frac * n) of them are stereo.  The
    initial pose is the truth turned by init_rot_deg about a random axis and moved by init_trans_m; the initial velocity is the truth
    plus N(0, 0.05); the bias N(0, 1e-3) gyro / N(0, 1e-2) accel (never zero).  G (a unit quaternion) turns the finished scene about
    the world origin (both frames' poses and velocities, the truth, the points) and computes delta_vel / delta_pos again from the turned
    states against the same world gravity, with the same noise (delta_rot does not change); G=None leaves it as it always was, bit for
    bit.
    Returns pose_wc / velocity / bias (initial state), prev_kf_pose_wc / prev_kf_velocity, preint [11] (delta_rot qw,qx,qy,qz |
    delta_vel | delta_pos | dt), points3d [n,3] f64, points2d [n,2] f32, is_stereo [n] u8, true_pose_wc / true_velocity, inliers [n]
    bool, camera."""
    rng = np.random.default_rng(seed)
    cam = camera
    g = np.array([0.0, 0.0, -9.81])
    if near_identity:
        q_i = _quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.0, 0.02))
    else:
        yaw = _quat_from_axis_angle([0.0, 0.0, 1.0], rng.uniform(-np.pi, np.pi))
        tilt = _quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.0, 0.2))
        q_i = _quat_mul(_quat_mul(yaw, tilt), _quat_from_R(_EUROC_R_WC))
    p_i = rng.uniform(-2.0, 2.0, 3)
    v_i = rng.normal(0.0, 0.5, 3)
    sc = 0.2 if near_identity else 1.0
    omega = rng.normal(0.0, 0.5 * sc, 3)
    acc = rng.normal(0.0, sc, 3)
    ang = np.linalg.norm(omega) * dt
    q_j = _quat_mul(q_i, _quat_from_axis_angle(omega, ang)) if ang > 0 else q_i.copy()
    q_j = q_j / np.linalg.norm(q_j)
    v_j = v_i + acc * dt
    p_j = p_i + v_i * dt + 0.5 * acc * dt * dt
    qic = _quat_conj(q_i)
    dq = _quat_mul(qic, q_j)
    nv = rng.normal(0.0, imu_noise, 3)
    dv = _quat_rot(qic, v_j - v_i - g * dt) + nv
    npos = rng.normal(0.0, imu_noise, 3)
    dp = _quat_rot(qic, p_j - p_i - v_i * dt - 0.5 * g * dt * dt) + npos
    preint = np.concatenate([dq / np.linalg.norm(dq), dv, dp, [dt]])
    u = rng.uniform(4.0, w - 4.0, n); v = rng.uniform(4.0, h - 4.0, n); d = rng.uniform(1.0, 20.0, n)
    Xc = np.stack([(u - cam["cx"]) / cam["fx"] * d, (v - cam["cy"]) / cam["fy"] * d, d], 1)
    Xw = _quat_rot(q_j, Xc) + p_j
    e = rng.normal(0.0, noise_px, (n, 2))
    e *= np.minimum(1.0, 2.0 / np.maximum(np.linalg.norm(e, axis=1), 1e-300))[:, None]
    uv = np.stack([u, v], 1) + e
    inliers = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        a = rng.uniform(0.0, 2.0 * np.pi, n_out); mag = rng.uniform(30.0, 200.0, n_out)
        uv[idx] = np.stack([u[idx], v[idx]], 1) + np.stack([np.cos(a), np.sin(a)], 1) * mag[:, None]
        inliers[idx] = False
    stereo = np.zeros(n, np.uint8)
    n_st = int(round(stereo_frac * n))
    if n_st:
        stereo[rng.choice(n, n_st, replace=False)] = 1
    q0 = _quat_mul(_quat_from_axis_angle(rng.normal(size=3), np.deg2rad(init_rot_deg)), q_j)
    dt0 = rng.normal(size=3)
    dt0 *= init_trans_m / np.linalg.norm(dt0)
    bias = np.concatenate([rng.normal(0.0, 1e-3, 3), rng.normal(0.0, 1e-2, 3)])
    bias[bias == 0.0] = 1e-6
    pose_wc, velocity = np.concatenate([q0 / np.linalg.norm(q0), p_j + dt0]), v_j + rng.normal(0.0, 0.05, 3)
    prev_wc, true_wc = np.concatenate([q_i, p_i]), np.concatenate([q_j, p_j])
    if G is not None:
        G = _unit_G(G)
        pose_wc, prev_wc, true_wc = _rotate_wc(G, pose_wc), _rotate_wc(G, prev_wc), _rotate_wc(G, true_wc)
        velocity, v_i, v_j, Xw = _quat_rot(G, velocity), _quat_rot(G, v_i), _quat_rot(G, v_j), _quat_rot(G, Xw)
        qic = _quat_conj(prev_wc[:4])
        preint = preint.copy()
        preint[4:7] = _quat_rot(qic, v_j - v_i - g * dt) + nv
        preint[7:10] = _quat_rot(qic, true_wc[4:] - prev_wc[4:] - v_i * dt - 0.5 * g * dt * dt) + npos
    return dict(pose_wc=pose_wc, velocity=velocity, bias=bias, prev_kf_pose_wc=prev_wc, prev_kf_velocity=v_i, preint=preint, points3d=Xw,
                points2d=uv.astype(np.float32), is_stereo=stereo, true_pose_wc=true_wc, true_velocity=v_j,
                inliers=inliers, camera=dict(cam))
