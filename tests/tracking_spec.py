"""Specification of orbx_track_frames (include/orbx.h) in numpy f64: the numeric part of track_local_map (tracker.rs:863-988,
mode 1) and track_with_motion_model (:1086-1192, mode 0) up to and after PnP.

project()  the projection, one IEEE operation at a time in the order the header states: the pose inverted with se3.rs:56-63's
           operation order, nalgebra's quaternion-vector product plus the translation, then fx * x / z + cx;
search()   the per-map-point decisions; the descriptor search itself is oracle.guided_match (the reference of orbx_guided_match);
gather()   the accepted points as correspondences in ascending map-point order;
finish()   status, matched and the pose rule, given what PnP returned for the gathered arrays.
PnP itself is not restated here: the GPU tests compose (PnP on these gathered arrays = what the fused call hands through).
"""
import numpy as np

OK, NO_MODEL, TOO_FEW_CORRESPONDENCES, TOO_FEW_INLIERS = 0, 1, 2, 3
PNP_NO_MODEL = 1
MOTION_MODEL, LOCAL_MAP = 0, 1
GRID_COLS, GRID_ROWS = 64, 48
BEHIND, NONE = -2, -1


def default_config(mode, **kw):
    c = dict(mode=mode, radius=15.0, img_w=752.0, img_h=480.0, min_correspondences=10 if mode == MOTION_MODEL else 4,
             min_inliers=10 if mode == MOTION_MODEL else 0)
    c.update(kw)
    return c


def _qv(w, x, y, z, v0, v1, v2):
    """nalgebra UnitQuaternion * Vector3: t = 2 (q.v x v); v' = t * w + q.v x t + v"""
    t0 = 2.0 * (y * v2 - z * v1); t1 = 2.0 * (z * v0 - x * v2); t2 = 2.0 * (x * v1 - y * v0)
    c0 = y * t2 - z * t1; c1 = z * t0 - x * t2; c2 = x * t1 - y * t0
    return t0 * w + c0 + v0, t1 * w + c1 + v1, t2 * w + c2 + v2


def project(cam, pose_wc, positions):
    """(z, u, v) [m] f64 of the points in the camera of pose_wc (T_wc); u, v are meaningless where z <= 0."""
    p = np.asarray(pose_wc, np.float64).reshape(7)
    X = np.asarray(positions, np.float64).reshape(-1, 3)
    w, x, y, z = p[0], -p[1], -p[2], -p[3]
    r0, r1, r2 = _qv(w, x, y, z, p[4], p[5], p[6])
    tx, ty, tz = -r0, -r1, -r2
    a0, a1, a2 = _qv(w, x, y, z, X[:, 0], X[:, 1], X[:, 2])
    xc = a0 + tx; yc = a1 + ty; zc = a2 + tz
    with np.errstate(all="ignore"):
        u = np.float64(cam["fx"]) * xc / zc + np.float64(cam["cx"])
        v = np.float64(cam["fy"]) * yc / zc + np.float64(cam["cy"])
    return zc, u, v


def margins(cam, cfg, pose_wc, positions):
    """The smallest distance of any decision argument from its decision point: z from 0; for the points in front, the four
    cell-range arguments (u -+ r) * 64 / w, (v -+ r) * 48 / h from the nearest integer (floor / ceil), and — mode 0 — u, v from
    0, 2cx, 2cy.  inf without points."""
    z, u, v = project(cam, pose_wc, positions)
    if len(z) == 0:
        return np.inf
    m = np.abs(z).min()
    f = z > 0.0
    if f.any():
        u, v = u[f], v[f]
        winv = GRID_COLS / cfg["img_w"]; hinv = GRID_ROWS / cfg["img_h"]
        for a in ((u - cfg["radius"]) * winv, (u + cfg["radius"]) * winv, (v - cfg["radius"]) * hinv, (v + cfg["radius"]) * hinv):
            m = min(m, np.abs(a - np.rint(a)).min())
        if cfg["mode"] == MOTION_MODEL:
            for a, lim in ((u, 2.0 * cam["cx"]), (v, 2.0 * cam["cy"])):
                m = min(m, np.abs(a).min(), np.abs(a - lim).min())
    return float(m)


def search(oracle, cam, cfg, kp, desc, positions, mp_desc, pose_wc):
    """match [m] int32: the keypoint index, NONE (in front, not accepted) or BEHIND (z <= 0)."""
    positions = np.asarray(positions, np.float64).reshape(-1, 3)
    mp_desc = np.asarray(mp_desc, np.uint8).reshape(-1, 32)
    z, u, v = project(cam, pose_wc, positions)
    out = np.full(len(z), BEHIND, np.int32)
    front = ~(z <= 0.0)                                                       # tracker.rs:872, :1109
    out[front] = NONE
    q = front.copy()
    if cfg["mode"] == MOTION_MODEL:                                           # :1121
        w, h = 2.0 * cam["cx"], 2.0 * cam["cy"]
        q &= ~((u < 0.0) | (u >= w) | (v < 0.0) | (v >= h))
    ids = np.flatnonzero(q)
    if len(ids):
        idx, _ = oracle.guided_match(kp, desc, cfg["img_w"], cfg["img_h"], np.stack([u[ids], v[ids]], 1), mp_desc[ids], cfg["radius"],
                                     cfg["mode"])
        out[ids] = idx
    return out


def gather(kp, positions, match):
    """the correspondences of one frame, ascending map-point order (:917-922, :1152-1156)"""
    positions = np.asarray(positions, np.float64).reshape(-1, 3)
    mp_idx = np.flatnonzero(match >= 0).astype(np.int32)
    feat_idx = match[mp_idx].astype(np.int32)
    pts2d = np.stack([kp["x"][feat_idx], kp["y"][feat_idx]], 1).astype(np.float32) if len(mp_idx) else np.zeros((0, 2), np.float32)
    return dict(mp_idx=mp_idx, feat_idx=feat_idx, points3d=positions[mp_idx].copy(), points2d=pts2d)


def finish(cfg, n_feat, match, g, prior_wc, pnp_pose, pnp_inlier, pnp_status, pnp_n_inliers):
    """(record, pose, matched): the rules behind PnP (:937, :955-988, :1173-1191)."""
    n_corr = len(g["mp_idx"])
    n_front = int((match >= NONE).sum())
    matched = np.full(n_feat, -1, np.int32)
    pose = np.asarray(pnp_pose, np.float64).copy()
    status, n_inl = OK, int(pnp_n_inliers)
    if n_corr < cfg["min_correspondences"]:
        status, n_inl = TOO_FEW_CORRESPONDENCES, 0
    elif n_inl < cfg["min_inliers"]:
        status = TOO_FEW_INLIERS
    elif pnp_status == PNP_NO_MODEL:
        status = NO_MODEL
    if status != TOO_FEW_CORRESPONDENCES:
        for i in range(n_corr):                                               # in order: the later correspondence overwrites
            if pnp_inlier[i]:
                matched[g["feat_idx"][i]] = g["mp_idx"][i]
    if status in (TOO_FEW_CORRESPONDENCES, TOO_FEW_INLIERS):
        pose = np.asarray(prior_wc, np.float64).copy()
    return dict(status=status, n_in_front=n_front, n_correspondences=n_corr, n_inliers=n_inl), pose, matched


def search_and_gather(oracle, cam, cfg, frames):
    """frames [(kp, desc, positions, mp_desc, search_pose_wc, prior_wc), ...] -> (offsets [B+1] int32, [match], [gathered])"""
    ms, gs = [], []
    for kp, desc, pos, md, sp, _ in frames:
        m = search(oracle, cam, cfg, kp, desc, pos, md, sp)
        ms.append(m); gs.append(gather(kp, pos, m))
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([len(g["mp_idx"]) for g in gs])
    return off, ms, gs
