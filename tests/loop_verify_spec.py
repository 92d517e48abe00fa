"""numpy f64 restatement of loop-candidate verification (include/orbx.h: orbx_verify_loop_candidates, orbx_sim3_ransac_batch;
the reference's corrector.rs:116-378 and sim3_solver.rs:63-266).  Test infrastructure only: the product never imports it.

It is written independently of the kernels: the matcher is the reference's two nested loops, Horn's rotation goes through
numpy.linalg.svd (the kernels use a one-sided Jacobi), sums are numpy's.  Besides the result it reports how far every discrete
decision was from its threshold (`margin`) and how well conditioned every sample's SVD was (`cond`), so that a test can tell a
scene on which two correct implementations must agree from one on which they need not."""
import numpy as np

from pnp_spec import sample, se3_inverse

OK, TOO_FEW_POINTS, TOO_FEW_MATCHES, TOO_FEW_PAIRS, NO_MODEL, TOO_FEW_INLIERS, TOO_FEW_VERIFIED = range(7)
NODE_NONE = 0xFFFFFFFF
U32_MAX = 4294967295
IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])

SIM3_DEFAULTS = dict(max_iterations=300, inlier_threshold=0.075, min_inliers=15, fix_scale=True, probability=0.99, seed=0)
VERIFY_DEFAULTS = dict(min_stereo_points=20, min_matches=15, min_pairs=15, min_inliers=15, min_verified=50, match_max_dist=50,
                       match_ratio=0.7, chi2=5.991, scale_factor=1.2)

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def _best_two(d1, desc2, candidates):
    """corrector.rs:281-296: (best, second, best_j) over the candidates in the given order"""
    best, second, best_j = U32_MAX, U32_MAX, 0
    cand = np.asarray(candidates, np.int64)
    dists = _POP[np.bitwise_xor(desc2[cand], d1[None, :])].sum(1).tolist() if len(cand) else []      # hamming_distance (:321-327), row by row
    for j, dist in zip(cand.tolist(), dists):
        if dist < best:
            second, best, best_j = best, dist, j
        elif dist < second:
            second = dist
    return best, second, best_j


def match_features(desc1, desc2, node1=None, node2=None, max_dist=50, ratio=0.7):
    """match_features_bow (:229-306).  Returns [(i, j, dist)] in ascending i [spec]."""
    n1, n2 = len(desc1), len(desc2)
    out = []
    lists = None
    if node1 is not None and node2 is not None:
        lists = {}
        for j in range(n2):
            if int(node2[j]) != NODE_NONE:
                lists.setdefault(int(node2[j]), []).append(j)
    for i in range(n1):
        if lists is None:
            cand = range(n2)
        else:
            cand = lists.get(int(node1[i]), []) if int(node1[i]) != NODE_NONE else []
            if not cand:
                continue
        best, second, bj = _best_two(desc1[i], desc2, cand)
        if best < max_dist and float(best) < ratio * float(second):
            out.append((i, bj, best))
    return out


# ---- poses ------------------------------------------------------------------------------------------------------------
def quat_rot(q, v):
    """nalgebra's UnitQuaternion * Vector3, one operation at a time: t = 2 (q_v x v); (t w + q_v x t) + v"""
    w, x, y, z = float(q[0]), float(q[1]), float(q[2]), float(q[3])
    v0, v1, v2 = float(v[0]), float(v[1]), float(v[2])
    t0 = 2.0 * (y * v2 - z * v1); t1 = 2.0 * (z * v0 - x * v2); t2 = 2.0 * (x * v1 - y * v0)
    c0 = y * t2 - z * t1; c1 = z * t0 - x * t2; c2 = x * t1 - y * t0
    return np.array([t0 * w + c0 + v0, t1 * w + c1 + v1, t2 * w + c2 + v2])


def transform_point(pose, p):
    r = quat_rot(pose[:4], p)
    return np.array([r[0] + pose[4], r[1] + pose[5], r[2] + pose[6]])


# ---- stage 3 ----------------------------------------------------------------------------------------------------------
def horn(p1, p2, fix_scale):
    """compute_sim3_horn (:157-227) -> (R, scale, M = scale R, t, sigma2 / sigma1) or None"""
    c1, c2 = p1.sum(0) / len(p1), p2.sum(0) / len(p2)
    a, b = p1 - c1, p2 - c2
    scale = 1.0
    if not fix_scale:
        sa, sb = float((a * a).sum()), float((b * b).sum())
        if sa < 1e-10:
            return None
        scale = float(np.sqrt(sb / sa))
    H = a.T @ b
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(V @ U.T) >= 0 else -1.0])
    R = V @ D @ U.T
    M = scale * R
    t = c2 - M @ c1
    return R, scale, M, t, (float(S[1] / S[0]) if S[0] > 0 else 0.0)


def err2(M, t, p1, p2):
    d = p1 @ M.T + t - p2
    return (d * d).sum(1)


def quat_from_R(R):
    """[spec] w >= 0"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q) / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def _rel(values, thr):
    """smallest relative distance of any value to the threshold"""
    return float(np.min(np.abs(values - thr)) / thr) if len(values) else np.inf


def sim3_ransac(p1, p2, cfg=None):
    """compute_sim3_ransac (:63-145) with all max_iterations hypotheses evaluated (the reference's adaptive bound never shortens its
    loop).  Returns a dict: status (0 OK / 1 NO_MODEL), sim3 [8], inlier [n] u8, best_hypothesis, ransac_inliers, n_inliers,
    refined, mse, M, t, margin, cond."""
    c = dict(SIM3_DEFAULTS); c.update(cfg or {})
    p1 = np.asarray(p1, np.float64).reshape(-1, 3); p2 = np.asarray(p2, np.float64).reshape(-1, 3)
    n = len(p1)
    thr2 = c["inlier_threshold"] * c["inlier_threshold"]
    out = dict(status=1, sim3=IDENTITY.copy(), inlier=np.zeros(n, np.uint8), best_hypothesis=-1, ransac_inliers=0, n_inliers=0, refined=0,
               mse=0.0, M=np.eye(3), t=np.zeros(3), margin=np.inf, cond=np.inf)
    if n < 3 or n < c["min_inliers"]:
        return out
    best, best_h, best_model = 0, -1, None
    for h in range(c["max_iterations"]):
        idx = sample(c["seed"], h, n, 3)
        if idx is None:
            continue
        m = horn(p1[idx], p2[idx], c["fix_scale"])
        if m is None:
            continue
        out["cond"] = min(out["cond"], m[4])
        e = err2(m[2], m[3], p1, p2)
        out["margin"] = min(out["margin"], _rel(e, thr2))
        k = int((e < thr2).sum())
        if k > best:
            best, best_h, best_model = k, h, m
    out["best_hypothesis"], out["ransac_inliers"] = best_h, best
    if best_h < 0:
        return out
    R, scale, M, t, _ = best_model
    e = err2(M, t, p1, p2)
    inl = e < thr2
    refined = 0
    if best >= c["min_inliers"]:
        m = horn(p1[inl], p2[inl], c["fix_scale"])
        if m is not None:
            e2 = err2(m[2], m[3], p1, p2)
            out["margin"] = min(out["margin"], _rel(e2, thr2))
            if int((e2 < thr2).sum()) >= best:
                R, scale, M, t, _ = m
                e, inl, refined = e2, e2 < thr2, 1
    k = int(inl.sum())
    out["n_inliers"], out["refined"] = k, refined
    if k < c["min_inliers"]:
        return out
    out.update(status=0, sim3=np.concatenate([quat_from_R(R), t, [scale]]), inlier=inl.astype(np.uint8), mse=float(e[inl].sum() / k), M=M, t=t)
    return out


# ---- the whole call ---------------------------------------------------------------------------------------------------
def verify_pair(cam, cur, loop, cfg=None, sim3_cfg=None):
    """One (current keyframe, loop keyframe) pair.  cur / loop: dicts with desc [n,32] u8, points_cam [n,3], has_point [n],
    pose_wc [7], optional node [n] u32; loop also kp (x, y, octave fields).  cam: dict fx, fy, cx, cy.  Returns a dict with status,
    matches [(i, j, dist)], feature_matches [k,2], pts_current, pts_loop [k,3], inlier [k], sim3 [8], the record fields, margin,
    cond."""
    c = dict(VERIFY_DEFAULTS); c.update(cfg or {})
    out = dict(status=OK, matches=[], feature_matches=np.zeros((0, 2), np.int32), pts_current=np.zeros((0, 3)), pts_loop=np.zeros((0, 3)),
               inlier=np.zeros(0, np.uint8), sim3=IDENTITY.copy(), n_matches=0, n_pairs=0, best_hypothesis=0, ransac_inliers=0, n_inliers=0,
               refined=0, n_verified=0, mse=0.0, margin=np.inf, cond=np.inf)
    if int(np.count_nonzero(cur["has_point"])) < c["min_stereo_points"] or int(np.count_nonzero(loop["has_point"])) < c["min_stereo_points"]:
        out["status"] = TOO_FEW_POINTS
        return out
    n1, n2 = cur.get("node"), loop.get("node")
    out["matches"] = match_features(cur["desc"], loop["desc"], n1, n2, c["match_max_dist"], c["match_ratio"])
    out["n_matches"] = len(out["matches"])
    if out["n_matches"] < c["min_matches"]:
        out["status"] = TOO_FEW_MATCHES
        return out
    fm = [(i, j) for i, j, _ in out["matches"] if cur["has_point"][i] and loop["has_point"][j]]
    out["feature_matches"] = np.array(fm, np.int32).reshape(-1, 2)
    out["pts_current"] = np.array([transform_point(cur["pose_wc"], cur["points_cam"][i]) for i, _ in fm]).reshape(-1, 3)
    out["pts_loop"] = np.array([transform_point(loop["pose_wc"], loop["points_cam"][j]) for _, j in fm]).reshape(-1, 3)
    out["n_pairs"] = len(fm)
    out["inlier"] = np.zeros(len(fm), np.uint8)
    if len(fm) < c["min_pairs"]:
        out["status"] = TOO_FEW_PAIRS
        return out
    s = sim3_ransac(out["pts_current"], out["pts_loop"], sim3_cfg)
    out["margin"], out["cond"] = s["margin"], s["cond"]
    for k in ("best_hypothesis", "ransac_inliers", "n_inliers", "refined"):
        out[k] = s[k]
    if s["status"] != 0:
        out["status"] = NO_MODEL
        return out
    out["sim3"], out["inlier"], out["mse"] = s["sim3"], s["inlier"], s["mse"]
    if s["n_inliers"] < c["min_inliers"]:
        out["status"] = TOO_FEW_INLIERS
        return out
    # verify_by_reprojection (:330-378) over all gathered matches
    inv = se3_inverse(np.asarray(loop["pose_wc"], np.float64))
    good = 0
    for (i, j), x in zip(fm, out["pts_current"]):
        p = transform_point(inv, s["M"] @ x + s["t"])
        if p[2] <= 0.0:
            continue
        u = cam["fx"] * p[0] / p[2] + cam["cx"]; v = cam["fy"] * p[1] / p[2] + cam["cy"]
        du = u - float(loop["kp"]["x"][j]); dv = v - float(loop["kp"]["y"][j])
        sc = c["scale_factor"] ** min(max(int(loop["kp"]["octave"][j]), 0), 31)           # include/orbx.h: octave clamped to 0..31
        thr = c["chi2"] * sc * sc
        e = du * du + dv * dv
        out["margin"] = min(out["margin"], abs(e - thr) / thr, abs(p[2]) / max(np.linalg.norm(p), 1e-300))
        if e < thr:
            good += 1
    out["n_verified"] = good
    if good < c["min_verified"]:
        out["status"] = TOO_FEW_VERIFIED
    return out
