"""Independent numpy restatement of the PnP-RANSAC specification (include/orbx.h: orbx_pnp_ransac).

Test infrastructure only: the product never imports it.  It follows the specification step by step — the sampler in np.uint64
arithmetic, the hypotheses' Levenberg-Marquardt vectorised over hypotheses (the Jacobian written out analytically rather than
through the BA's pose block), OpenCV's float inlier test, the sequential walk with RANSACUpdateNumIters in plain Python, the
refinement over the best hypothesis' inliers, and the detailed pass of pnp.rs:110-125.
"""
import math

import numpy as np

OK, NO_MODEL, TOO_FEW, OVER_MAX_N = 0, 1, 2, 3
DEFAULTS = dict(max_iterations=100, reproj_error=8.0, confidence=0.99, model_points=5, hypothesis_iterations=10, refine_iterations=20,
                seed=0)
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_DRAWS = 64


# ---- step 1: the sampler -------------------------------------------------------------------------------------------------
def sampler_draws(seed, h, n):
    """The 64 raw indices of hypothesis h: idx = ((splitmix64(seed + golden * (h*64 + a + 1)) >> 32) * n) >> 32, a = 0..63."""
    a = np.arange(_DRAWS, dtype=np.uint64)
    x = np.uint64(seed) + _GOLDEN * (np.uint64(h * 64) + a + np.uint64(1))
    z = (x ^ (x >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)


def sample(seed, h, n, m):
    """The first m distinct draws of hypothesis h, or None when 64 draws do not give m."""
    out = []
    for i in sampler_draws(seed, h, n):
        i = int(i)
        if i not in out:
            out.append(i)
            if len(out) == m:
                return out
    return None


# ---- poses ---------------------------------------------------------------------------------------------------------------
def quat_R(q):
    """[...,4] (w,x,y,z) -> [...,3,3]"""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)], -2)


def quat_mul(a, b):
    w1, x1, y1, z1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    w2, x2, y2, z2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def quat_rot(q, v):
    """nalgebra's UnitQuaternion * Vector3: v + w t + q_v x t, t = 2 q_v x v (broadcasts)"""
    qv = q[..., 1:]
    t = 2.0 * np.cross(qv, v)
    return v + q[..., :1] * t + np.cross(qv, t)


def se3_inverse(p):
    """(q, t) of a 7-vector -> its inverse (q*, -(q* t))"""
    p = np.asarray(p, np.float64)
    qi = p[..., :4] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([qi, -quat_rot(qi, p[..., 4:])], -1)


def exp_so3(w):
    """UnitQuaternion::from_scaled_axis of [...,3]: exp of the pure quaternion w/2, identity when |w/2|^2 <= eps^2"""
    v = w / 2.0
    nn = (v * v).sum(-1)
    n = np.sqrt(nn)
    with np.errstate(all="ignore"):
        s = np.sin(n) / n
    q = np.concatenate([np.cos(n)[..., None], v * s[..., None]], -1)
    small = nn <= np.finfo(np.float64).eps ** 2
    q[small] = [1.0, 0.0, 0.0, 0.0]
    return q


# ---- step 2 / 5: Levenberg-Marquardt ---------------------------------------------------------------------------------------
def _camera_frame(q, t, X):
    """X_c = R X + t for poses [B] and points [B,k,3], written as the kernels write it (one operation at a time, left to right)"""
    R = quat_R(q)
    out = []
    for r in range(3):
        out.append(R[:, r, 0, None] * X[..., 0] + R[:, r, 1, None] * X[..., 1] + R[:, r, 2, None] * X[..., 2] + t[:, r, None])
    return out


def _residuals(cam, q, t, X, uv, use):
    """r = pi(X_c) - (u, v) [B,k,2], J = d r / d (omega, upsilon) with the left perturbation [B,k,2,6], and which points count
    (use and not |z| < 1e-6)"""
    x, y, z = _camera_frame(q, t, X)
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    with np.errstate(all="ignore"):
        iz = 1.0 / z
        xn, yn = x * iz, y * iz
        r = np.stack([fx * xn + cx - uv[..., 0], fy * yn + cy - uv[..., 1]], -1)
        # d pi / d X_c times d X_c / d delta = [-[X_c]x | I]
        Ju = np.stack([-fx * xn * yn, fx * (1.0 + xn * xn), -fx * yn, fx * iz, np.zeros_like(x), -fx * xn * iz], -1)
        Jv = np.stack([-fy * (1.0 + yn * yn), fy * xn * yn, fy * xn, np.zeros_like(x), fy * iz, -fy * yn * iz], -1)
    valid = use & ~(np.abs(z) < 1e-6)
    J = np.stack([Ju, Jv], -2)
    return np.where(valid[..., None], r, 0.0), np.where(valid[..., None, None], J, 0.0)


def _cost(cam, q, t, X, uv, use):
    r, _ = _residuals(cam, q, t, X, uv, use)
    return (r * r).sum((-1, -2))


def _solve(H, rhs, lam):
    """(H + lam diag(max(H_ii, 1e-6))) d = rhs by Cholesky, batched; ok = every pivot positive"""
    B = len(H)
    A = H.copy()
    i6 = np.arange(6)
    A[:, i6, i6] = A[:, i6, i6] + lam[:, None] * np.fmax(A[:, i6, i6], 1e-6)
    L = np.zeros_like(A)
    ok = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            a = A[:, j, j] - (L[:, j, :j] ** 2).sum(-1)
            ok &= a > 0.0
            L[:, j, j] = np.sqrt(np.where(a > 0.0, a, 1.0))
            for i in range(j + 1, 6):
                L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / L[:, j, j]
        y = np.zeros((B, 6))
        for i in range(6):
            y[:, i] = (rhs[:, i] - (L[:, i, :i] * y[:, :i]).sum(-1)) / L[:, i, i]
        d = np.zeros((B, 6))
        for i in range(5, -1, -1):
            d[:, i] = (y[:, i] - (L[:, i + 1:, i] * d[:, i + 1:]).sum(-1)) / L[:, i, i]
    return d, ok


def lm(cam, q, t, X, uv, use, iterations):
    """The project's LM rule (oracle/ba_ref.cpp lm_loop) for B independent problems: lambda 1e-3; stop on a failed Cholesky, on
    |delta| < 1e-10 or after `iterations`; accept a trial of lower cost (lambda / 10, >= 1e-10), else lambda * 10 (<= 1e10)."""
    q = q.copy(); t = t.copy()
    B = len(q)
    lam = np.full(B, 1e-3)
    active = np.ones(B, bool)
    iters = np.zeros(B, int)
    for it in range(iterations):
        if not active.any():
            break
        iters[active] = it + 1
        r, J = _residuals(cam, q, t, X, uv, use)
        H = np.einsum("bkri,bkrj->bij", J, J)
        g = np.einsum("bkri,bkr->bi", J, r)
        cost = (r * r).sum((-1, -2))
        d, ok = _solve(H, -g, lam)
        with np.errstate(invalid="ignore"):
            active &= ok & ~(np.sqrt((d * d).sum(-1)) < 1e-10)
        e = exp_so3(np.where(active[:, None], d[:, :3], 0.0))
        qt = quat_mul(e, q)
        tt = quat_rot(e, t) + d[:, 3:]
        with np.errstate(invalid="ignore"):
            acc = active & (_cost(cam, qt, tt, X, uv, use) < cost)
        rej = active & ~acc
        q[acc] = qt[acc]; t[acc] = tt[acc]
        lam[acc] = np.maximum(lam[acc] * 0.1, 1e-10)
        lam[rej] = np.minimum(lam[rej] * 10.0, 1e10)
    return q, t, iters


# ---- step 3: OpenCV's inlier test ------------------------------------------------------------------------------------------
def inlier_counts(cam, q, t, X, uv, reproj_error):
    """mask [B,n]: (float)(du^2 + dv^2) <= (float)reproj_error^2, du, dv in f64, no z test"""
    B = len(q)
    x, y, z = _camera_frame(q, t, np.broadcast_to(X, (B,) + X.shape))
    with np.errstate(all="ignore"):
        iz = 1.0 / z
        du = cam["fx"] * (x * iz) + cam["cx"] - uv[:, 0]
        dv = cam["fy"] * (y * iz) + cam["cy"] - uv[:, 1]
        return (du * du + dv * dv).astype(np.float32) <= np.float32(reproj_error * reproj_error)


# ---- step 4: the walk ------------------------------------------------------------------------------------------------------
def ransac_update_num_iters(p, ep, model_points, max_iters):
    """OpenCV's RANSACUpdateNumIters (calib3d/src/ptsetreg.cpp); cvRound = nearest, ties to even"""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, 2.2250738585072014e-308)
    denom = 1.0 - math.pow(1.0 - ep, model_points)
    if denom < 2.2250738585072014e-308:
        return 0
    num = math.log(num)
    denom = math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(round(num / denom))


def walk(counts, n, model_points, confidence, max_iterations):
    """(best, best_h, hypotheses_evaluated): OpenCV's sequential loop over counts evaluated beforehand"""
    best, best_h, niters, h = 0, -1, max_iterations, 0
    while h < niters:
        if counts[h] > max(best, model_points - 1):
            best, best_h = int(counts[h]), h
            niters = ransac_update_num_iters(confidence, (n - best) / n, model_points, niters)
        h += 1
    return best, best_h, h


# ---- steps 5-7 -------------------------------------------------------------------------------------------------------------
def detailed(cam, pose_wc, X, uv, reproj_error):
    """pnp.rs:110-125 with the returned T_wc: err = sqrt(du^2 + dv^2), +inf where z <= 0; inlier = err < reproj_error"""
    cw = se3_inverse(pose_wc)
    pc = quat_rot(cw[:4], X) + cw[4:]
    with np.errstate(all="ignore"):
        u = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]
        v = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
        du = u - uv[:, 0]; dv = v - uv[:, 1]
        err = np.sqrt(du * du + dv * dv)
    err = np.where(pc[:, 2] <= 0.0, np.inf, err)
    with np.errstate(invalid="ignore"):
        return err, err < reproj_error


def solve(cam, points3d, points2d, prior_wc, cfg=None, max_n=None):
    """One problem.  points2d are taken as f32 (cv::Point2f) and promoted.  Returns a dict with the orbx_pnp_result fields, pose
    (T_wc, 7), inlier_mask, reproj_errors and the per-hypothesis counts."""
    c = dict(DEFAULTS, **(cfg or {}))
    X = np.ascontiguousarray(points3d, np.float64).reshape(-1, 3)
    uv = np.asarray(points2d, np.float32).reshape(-1, 2).astype(np.float64)
    prior = np.asarray(prior_wc, np.float64).reshape(7)
    n, m, H = len(X), c["model_points"], c["max_iterations"]
    out = dict(status=OK, ransac_inliers=0, best_hypothesis=-1, hypotheses_evaluated=0, refine_iterations=0, counts=None)
    pose = prior.copy()
    if n < 4:
        out["status"] = TOO_FEW
    elif max_n is not None and n > max_n:
        out["status"] = OVER_MAX_N
    else:
        if n <= m:
            samples = [list(range(n))]
        else:
            samples = [sample(c["seed"], h, n, m) for h in range(H)]
        valid = np.array([s is not None for s in samples])
        k = min(n, m)
        idx = np.array([s if s is not None else list(range(k)) for s in samples])
        cw = se3_inverse(prior)
        B = len(samples)
        q0 = np.repeat(cw[None, :4], B, 0); t0 = np.repeat(cw[None, 4:], B, 0)
        qh, th, _ = lm(cam, q0, t0, X[idx], uv[idx], np.ones(idx.shape, bool), c["hypothesis_iterations"])
        masks = inlier_counts(cam, qh, th, X, uv, c["reproj_error"])
        counts = np.where(valid, masks.sum(1), 0)
        out["counts"] = counts
        if n <= m:
            best, best_h, evaluated = int(counts[0]), 0, 1
        else:
            best, best_h, evaluated = walk(counts, n, m, c["confidence"], H)
        out.update(ransac_inliers=best, best_hypothesis=best_h, hypotheses_evaluated=evaluated)
        if best_h < 0:
            out["status"] = NO_MODEL
        else:
            use = masks[best_h][None, :]
            qr, tr, it = lm(cam, qh[best_h:best_h + 1], th[best_h:best_h + 1], X[None], uv[None], use, c["refine_iterations"])
            out["refine_iterations"] = int(it[0])
            pose = se3_inverse(np.concatenate([qr[0], tr[0]]))
    err, mask = detailed(cam, pose, X, uv, c["reproj_error"])
    out.update(pose=pose, inlier_mask=mask, reproj_errors=err, n_inliers=int(mask.sum()))
    out["final_rms"] = float(np.sqrt((err[mask] ** 2).sum() / mask.sum())) if mask.any() else 0.0
    return out


def rotation_angle(pa, pb):
    """angle of q_a q_b^-1 (radians) between two 7-vector poses"""
    qa = np.asarray(pa[:4], np.float64); qb = np.asarray(pb[:4], np.float64) * np.array([1.0, -1.0, -1.0, -1.0])
    d = quat_mul(qa, qb)
    return float(2.0 * np.arctan2(np.linalg.norm(d[1:]), abs(d[0])))
