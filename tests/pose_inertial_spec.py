"""Independent numpy restatement of pose-inertial optimization (src/optimizer/pose_inertial_optim.rs:94-216; include/orbx.h:
orbx_pose_inertial_optimize).

Test infrastructure only: the product never imports it.  It follows the reference operation for operation in f64: nalgebra's
scaled_axis / from_scaled_axis and quaternion products, compute_imu_residual (imu_factors.rs:66-103), the visual rows of
compute_reprojection_error_with_jacobian (:250-349) vectorised over observations, J^T J and J^T r of the stacked Jacobian, the damping,
nalgebra's partial-pivoting LU and its solve in plain Python, the additive update and the reclassification of every observation with
compute_reprojection_error (:227-248).
"""
import math

import numpy as np

OK, TOO_FEW, SINGULAR = 0, 1, 2
DEFAULTS = dict(max_iterations=4, chi2_mono_init=12.0, chi2_stereo_init=15.6, chi2_mono_final=5.991, chi2_stereo_final=7.815,
                imu_weight=1.0)
GRAVITY = np.array([0.0, 0.0, -9.81])          # imu/sample.rs:6
EPS = 1e-6                                     # :405
_F64_EPS = 2.220446049250313e-16


# ---- nalgebra's unit quaternion (w, x, y, z) ------------------------------------------------------------------------------
def scaled_axis(q):
    """UnitQuaternion::scaled_axis: axis() (the imaginary part, negated when w < 0, divided by its norm) * angle()
    (atan2(|imag|, |w|) * 2); zero when the imaginary part is zero."""
    v = np.array([q[1], q[2], q[3]], np.float64)
    if not (q[0] >= 0.0):
        v = -v
    n = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if not (n > 0.0):
        return np.zeros(3)
    ang = math.atan2(n, abs(q[0])) * 2.0
    return np.array([v[0] / n * ang, v[1] / n * ang, v[2] / n * ang])


def from_scaled_axis(r):
    """UnitQuaternion::from_scaled_axis = exp of the pure quaternion r / 2 (the identity when |r/2|^2 <= eps^2)."""
    v = np.array([r[0] / 2.0, r[1] / 2.0, r[2] / 2.0])
    nn = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if nn <= _F64_EPS * _F64_EPS:
        return np.array([1.0, 0.0, 0.0, 0.0])
    n = math.sqrt(nn)
    s = 1.0 * math.sin(n) / n
    return np.array([1.0 * math.cos(n), v[0] * s, v[1] * s, v[2] * s])


def conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def qrot(q, v):
    """UnitQuaternion * Vector3 (nalgebra: t = 2 imag x v; v + w t + imag x t); v may be [..., 3]"""
    v = np.asarray(v, np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    t0 = 2.0 * (q[2] * z - q[3] * y); t1 = 2.0 * (q[3] * x - q[1] * z); t2 = 2.0 * (q[1] * y - q[2] * x)
    c0 = q[2] * t2 - q[3] * t1; c1 = q[3] * t0 - q[1] * t2; c2 = q[1] * t1 - q[2] * t0
    return np.stack([t0 * q[0] + c0 + x, t1 * q[0] + c1 + y, t2 * q[0] + c2 + z], -1)


def rotation_angle(a, b):
    """angle of q_a * conj(q_b) in radians (poses [7] or quaternions [4])"""
    d = qmul(np.asarray(a, np.float64)[:4], conj(np.asarray(b, np.float64)[:4]))
    return 2.0 * math.atan2(np.linalg.norm(d[1:]), abs(d[0]))


# ---- the parameters and the residuals --------------------------------------------------------------------------------------
def params_from_state(pose_wc, velocity, bias):
    """[scaled_axis(q_wc) | t_wc | v | b_g | b_a] (:110-134)"""
    return np.concatenate([scaled_axis(pose_wc[:4]), np.asarray(pose_wc[4:7], np.float64), np.asarray(velocity, np.float64),
                           np.asarray(bias, np.float64)])


def extract_pose(params):
    """(:219-224) -> [7] T_wc"""
    return np.concatenate([from_scaled_axis(params[0:3]), params[3:6]])


def imu_residual(prev_pose_wc, prev_velocity, pose_wc, velocity, preint):
    """compute_imu_residual (imu_factors.rs:66-103): [Log(dR^T R_i^T R_j) | R_i^T (v_j - v_i - g dt) - dv |
    R_i^T (p_j - p_i - v_i dt - g dt^2 / 2) - dp]; preint [11] = delta_rot qw,qx,qy,qz | delta_vel | delta_pos | dt"""
    dt = preint[10]
    ri, rj = np.asarray(prev_pose_wc[:4], np.float64), np.asarray(pose_wc[:4], np.float64)
    pi, pj = np.asarray(prev_pose_wc[4:7], np.float64), np.asarray(pose_wc[4:7], np.float64)
    vi, vj = np.asarray(prev_velocity, np.float64), np.asarray(velocity, np.float64)
    ric = conj(ri)
    err = qmul(qmul(conj(preint[0:4]), ric), rj)
    rr = scaled_axis(err)
    rv = qrot(ric, vj - vi - GRAVITY * dt) - preint[4:7]
    rp = qrot(ric, pj - pi - vi * dt - 0.5 * GRAVITY * dt * dt) - preint[7:10]
    return np.concatenate([rr, rv, rp])


def _project(cam, pose_wc, X):
    """pose_cw = pose_wc.inverse(); p_cam = pose_cw.transform_point(X) for X [n,3]"""
    qcw = conj(pose_wc[:4])
    tcw = -qrot(qcw, pose_wc[4:7])
    p = qrot(qcw, X)
    return p + tcw


def reprojection_errors(cam, pose_wc, X, uv):
    """compute_reprojection_error (:227-248) for every observation: uv - (fx x / z + cx, fy y / z + cy), (100, 100) where
    z <= 0.001"""
    p = _project(cam, pose_wc, X)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    behind = z <= 0.001
    with np.errstate(divide="ignore", invalid="ignore"):
        e0 = uv[:, 0] - (cam["fx"] * x / z + cam["cx"])
        e1 = uv[:, 1] - (cam["fy"] * y / z + cam["cy"])
    e0 = np.where(behind, 100.0, e0); e1 = np.where(behind, 100.0, e1)
    return e0, e1


def visual_rows(cam, pose_wc, X, uv):
    """compute_reprojection_error_with_jacobian (:250-349) as written: e [n,2] and the 2x6 blocks [n,2,6] (the camera-frame block
    applied to the world-frame parameters); (100, 100) and a zero block where z <= 0.001"""
    p = _project(cam, pose_wc, X)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    fx, fy, cx, cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    behind = z <= 0.001
    with np.errstate(divide="ignore", invalid="ignore"):
        z_inv = 1.0 / z
        z_inv_sq = z_inv * z_inv
        e = np.stack([uv[:, 0] - (fx * x * z_inv + cx), uv[:, 1] - (fy * y * z_inv + cy)], 1)
        xy, x_sq, y_sq = x * y, x * x, y * y
        zero = np.zeros_like(x)
        J = np.stack([np.stack([-fx * xy * z_inv_sq, fx * (1.0 + x_sq * z_inv_sq), -fx * y * z_inv, fx * z_inv, zero, -fx * x * z_inv_sq], 1),
                      np.stack([-fy * (1.0 + y_sq * z_inv_sq), fy * xy * z_inv_sq, fy * x * z_inv, zero, fy * z_inv, -fy * y * z_inv_sq], 1)], 1)
    e[behind] = 100.0
    J[behind] = 0.0
    return e, J


# ---- nalgebra's LU ---------------------------------------------------------------------------------------------------------
def lu_solve(A, b):
    """nalgebra DMatrix::lu().solve(b): partial pivoting (the first largest |value| of the column, icamax), gauss_step (the column
    scaled by 1 / diag, then y = -pivot_k * l + y), P b, the unit lower solve, the upper solve (b_i / diag, then b_r = -x_i U_ri + b_r).
    None when a pivot is exactly zero (nalgebra's solve then fails on that diagonal)."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    n = len(b)
    for i in range(n):
        piv, best = i, abs(A[i, i])
        for r in range(i + 1, n):
            if abs(A[r, i]) > best:
                best, piv = abs(A[r, i]), r
        diag = A[piv, i]
        if diag == 0.0:
            return None
        if piv != i:
            A[[i, piv]] = A[[piv, i]]
            b[[i, piv]] = b[[piv, i]]
        inv = 1.0 / diag
        for r in range(i + 1, n):
            l = A[r, i] * inv
            A[r, i] = l
            for c in range(i + 1, n):
                A[r, c] = -A[i, c] * l + A[r, c]
            b[r] = -b[i] * l + b[r]
    for i in range(n - 1, -1, -1):
        x = b[i] / A[i, i]
        b[i] = x
        for r in range(i):
            b[r] = -x * A[r, i] + b[r]
    return b


# ---- the optimization --------------------------------------------------------------------------------------------------------
def solve(camera, pose_wc, velocity, bias, prev_kf_pose_wc, prev_kf_velocity, preint, points3d, points2d, is_stereo, cfg=None):
    """pose_inertial_optimization (:94-216).  points2d are taken as f32 and widened (the tracker's kp.pt()), is_stereo nonzero =
    stereo.  Returns dict(pose [7], velocity [3], bias [6], num_inliers, num_observations, iterations, inlier_mask [n] bool, status,
    margin = the smallest |chi2 - threshold| / threshold over every chi2 the reclassification evaluated (inf without any))."""
    c = dict(DEFAULTS)
    c.update(cfg or {})
    cam = camera
    X = np.ascontiguousarray(points3d, np.float64).reshape(-1, 3)
    uv = np.asarray(points2d, np.float32).reshape(-1, 2).astype(np.float64)
    st = np.asarray(is_stereo).reshape(-1) != 0
    preint = np.asarray(preint, np.float64)
    prev = np.asarray(prev_kf_pose_wc, np.float64)
    prev_v = np.asarray(prev_kf_velocity, np.float64)
    n = len(X)
    params = params_from_state(np.asarray(pose_wc, np.float64), velocity, bias)
    mask = np.ones(n, bool)
    iterations, status, margin = 0, OK, math.inf
    M, w = c["max_iterations"], c["imu_weight"]
    for it in range(M):
        iterations = it + 1
        progress = it / max(M - 1, 1)
        chi2_mono = c["chi2_mono_init"] * (1.0 - progress) + c["chi2_mono_final"] * progress
        chi2_stereo = c["chi2_stereo_init"] * (1.0 - progress) + c["chi2_stereo_final"] * progress
        pose = extract_pose(params)
        vel = params[6:9]
        e, Jv = visual_rows(cam, pose, X[mask], uv[mask])
        num_active = int(mask.sum())
        r0 = imu_residual(prev, prev_v, pose, vel, preint)
        Ji = np.zeros((9, 15))
        for j in range(15):
            pp = params.copy()
            pp[j] += EPS
            Ji[:, j] = (imu_residual(prev, prev_v, extract_pose(pp), pp[6:9], preint) - r0) / EPS * w
        if num_active < 5:
            status = TOO_FEW
            break
        J = np.zeros((2 * num_active + 9, 15))
        J[:2 * num_active, :6] = Jv.reshape(-1, 6)
        J[2 * num_active:] = Ji
        res = np.concatenate([e.reshape(-1), r0 * w])
        g = J.T @ res
        H = J.T @ J
        for i in range(15):
            H[i, i] += 1e-3 * max(H[i, i], 1e-6)
        delta = lu_solve(H, -g)
        if delta is None:
            status = SINGULAR
            break
        params = params + delta
        pose = extract_pose(params)
        e0, e1 = reprojection_errors(cam, pose, X, uv)
        chi2 = e0 * e0 + e1 * e1
        thr = np.where(st, chi2_stereo, chi2_mono)
        mask = chi2 < thr
        if n:
            with np.errstate(invalid="ignore"):
                m = np.abs(chi2 - thr) / thr
            margin = min(margin, float(np.nanmin(m)) if np.isfinite(m).any() else 0.0)
    return dict(pose=extract_pose(params), velocity=params[6:9].copy(), bias=params[9:15].copy(), num_inliers=int(mask.sum()),
                num_observations=n, iterations=iterations, inlier_mask=mask, status=status, margin=margin)


def solve_scene(s, cfg=None):
    """solve() on a synth.pose_inertial_problem scene"""
    return solve(s["camera"], s["pose_wc"], s["velocity"], s["bias"], s["prev_kf_pose_wc"], s["prev_kf_velocity"], s["preint"],
                 s["points3d"], s["points2d"], s["is_stereo"], cfg)
