// pose_dev.hpp — device math shared by the bundle-adjustment kernels (ba_kernels.hip), the PnP-RANSAC kernels (pnp_kernels.hip),
// pose-inertial optimization (pose_inertial_kernels.hip), the tracker's projection (track_kernels.hip) and loop verification
// (loop_verify_kernels.hip): the camera descriptor, quaternion / rotation / SE3 helpers, the 2x6 pose block of one observation
// and the 9-d IMU preintegration residual.
// Device code only, inside an anonymous namespace: each translation unit that includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct BaCam {
  double fx, fy, cx, cy, huber;
  int zero_behind;   // solve_global_ba: Jacobian rows are zero where z_c <= 0.001 (global_ba.rs:561-563)
  int inertial;      // solve_inertial_ba: T_wc pose parameters, the Jacobian forms of local_inertial_ba.rs:735-804,
                     // no Huber on the 100-px penalty, Huber threshold per observation (o_flag bit 0 = stereo)
  double huber_stereo;
  const int* o_flag;
};

// ---- small device math ---------------------------------------------------------------------------------------
__device__ __forceinline__ void quat_to_R(const double* q, double* R) {
  const double w = q[0], i = q[1], j = q[2], k = q[3];
  const double ww = w * w, ii = i * i, jj = j * j, kk = k * k;
  const double ij = i * j * 2.0, wk = w * k * 2.0, wj = w * j * 2.0;
  const double ik = i * k * 2.0, jk = j * k * 2.0, wi = w * i * 2.0;
  R[0] = ww + ii - jj - kk; R[1] = ij - wk;           R[2] = wj + ik;
  R[3] = wk + ij;           R[4] = ww - ii + jj - kk; R[5] = jk - wi;
  R[6] = ik - wj;           R[7] = wi + jk;           R[8] = ww - ii - jj + kk;
}

// local_ba_lm.rs:648-662 then R|t (12 doubles)
// nalgebra UnitQuaternion::from_scaled_axis = exp of the pure quaternion r/2 (identity when |r/2|^2 <= eps^2)
__device__ __forceinline__ void dev_q_from_scaled_axis(const double* r, double* q) {
  const double v0 = r[0] / 2.0, v1 = r[1] / 2.0, v2 = r[2] / 2.0;
  const double nn = v0 * v0 + v1 * v1 + v2 * v2;
  const double eps = 2.220446049250313e-16;
  if (nn <= eps * eps) { q[0] = 1.0; q[1] = q[2] = q[3] = 0.0; return; }
  const double n = sqrt(nn), s = 1.0 * sin(n) / n;
  q[0] = 1.0 * cos(n); q[1] = v0 * s; q[2] = v1 * s; q[3] = v2 * s;
}
__device__ __forceinline__ void dev_q_rot(const double* q, const double* v, double* o) {   // UnitQuaternion * Vector3
  const double t0 = 2.0 * (q[2] * v[2] - q[3] * v[1]), t1 = 2.0 * (q[3] * v[0] - q[1] * v[2]), t2 = 2.0 * (q[1] * v[1] - q[2] * v[0]);
  const double c0 = q[2] * t2 - q[3] * t1, c1 = q[3] * t0 - q[1] * t2, c2 = q[1] * t1 - q[2] * t0;
  o[0] = t0 * q[0] + c0 + v[0]; o[1] = t1 * q[0] + c1 + v[1]; o[2] = t2 * q[0] + c2 + v[2];
}
// SE3::inverse (se3.rs:56-63) of the pose wc = (q | t): conjugate, then -(q^-1 * t).  q / t may be wc's own storage.
__device__ __forceinline__ void se3_inverse7(const double* wc, double* q, double* t) {
  const double qi[4] = {wc[0], -wc[1], -wc[2], -wc[3]};
  double r[3];
  dev_q_rot(qi, wc + 4, r);
  q[0] = qi[0]; q[1] = qi[1]; q[2] = qi[2]; q[3] = qi[3];
  t[0] = -r[0]; t[1] = -r[1]; t[2] = -r[2];
}
// SE3::transform_point: q * p + t
__device__ __forceinline__ void se3_transform_point(const double* pose7, const double* p, double* o) {
  double r[3];
  dev_q_rot(pose7, p, r);
  o[0] = r[0] + pose7[4]; o[1] = r[1] + pose7[5]; o[2] = r[2] + pose7[6];
}
__device__ __forceinline__ void dev_q_mul(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// The 2x6 pose block A and the 2x3 point block B of one observation (both * sqrt(w)) from its four "projective" numbers —
// x, y of the point in the camera frame, 1/z, and the square root of the Huber weight — and the keyframe's R|t: no division, no
// square root.  piz == 0 marks an observation whose Jacobian rows are zero (|z| < 1e-6, or behind the camera in the global /
// inertial forms).  obs_terms itself goes through this function, so every kernel that rebuilds the blocks from the stored
// (x, y, 1/z, sqrt w) gets the same bits the build kernel used for V and g_l.
// J_pose (:239-254), J_point (:281-287); inertial: local_inertial_ba.rs:735-804.
// Round 4: the entries as products of six shared factors (f_x sqrt w, f_y sqrt w, those times 1/z, x/z, y/z) instead of each entry's own
// chain of four or five multiplications as the reference writes them — 28 double-precision operations where there were 70, in every
// per-observation kernel (these kernels issue f64 operations and little else).  The values agree with the literal form to rounding.
// The inertial form's point block is the same expression; its pose block is the visual one with the opposite sign (the perturbation
// is applied on the other side), so one body serves both.  A[4] and A[9] are structurally zero: the callers skip their products.
__device__ __forceinline__ void obs_jac_from_proj(const BaCam& cam, const double* Rt, double x, double y, double piz, double sw,
                                                  double* __restrict__ A, double* __restrict__ B) {
  // (piz == 0 comes with sw == 0 — obs_terms sets both or neither, an empty Schur slot is all zeros — and then every entry below is
  // 0 * finite: no test, no branch, so that two observations' blocks can be scheduled into each other)
  const double fs = cam.fx * sw, gs = cam.fy * sw, fz = fs * piz, gz = gs * piz, xz = x * piz, yz = y * piz;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    B[c] = fz * fma(xz, Rt[6 + c], -Rt[c]);                // -(1/z) (f_x R_0c - f_x (x/z) R_2c) sqrt w
    B[3 + c] = gz * fma(yz, Rt[6 + c], -Rt[3 + c]);
  }
  const double sg = cam.inertial ? -1.0 : 1.0;
  const double fa = sg * fs, ga = sg * gs, fza = sg * fz, gza = sg * gz;
  A[2] = yz * fa;                    A[0] = xz * A[2];                  A[1] = -(fma(xz, xz, 1.0) * fa);
  A[3] = -fza;                       A[4] = 0.0;                        A[5] = xz * fza;
  A[8] = -(xz * ga);                 A[7] = yz * A[8];                  A[6] = fma(yz, yz, 1.0) * ga;
  A[9] = 0.0;                        A[10] = -gza;                      A[11] = yz * gza;
}

// ---- inertial terms shared by the inertial BA (ba_kernels.hip) and pose-inertial optimization (pose_inertial_kernels.hip) --------
// src/optimizer/imu_factors.rs:66-103

__device__ __forceinline__ void dev_scaled_axis(const double* q, double* o) {   // nalgebra UnitQuaternion::scaled_axis
  double v0 = q[1], v1 = q[2], v2 = q[3];
  if (!(q[0] >= 0.0)) { v0 = -v0; v1 = -v1; v2 = -v2; }
  const double n = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
  if (n > 0.0) {
    const double ang = atan2(n, fabs(q[0])) * 2.0;
    o[0] = v0 / n * ang; o[1] = v1 / n * ang; o[2] = v2 / n * ang;
  } else { o[0] = o[1] = o[2] = 0.0; }
}

// si / sj: pose (6) + velocity (3) of the two keyframes
__device__ __forceinline__ void imu_residual_dev(const double* si, const double* sj, const double* pre, double* r9) {
  const double dt = pre[10];
  double ri[4], rj[4];
  dev_q_from_scaled_axis(si, ri);
  dev_q_from_scaled_axis(sj, rj);
  const double ric[4] = {ri[0], -ri[1], -ri[2], -ri[3]}, drc[4] = {pre[0], -pre[1], -pre[2], -pre[3]};
  double t[4], err[4];
  dev_q_mul(drc, ric, t);
  dev_q_mul(t, rj, err);                                                  // imu_factors.rs:85
  dev_scaled_axis(err, r9);
  const double g[3] = {0.0, 0.0, -9.81};                                  // imu/sample.rs:6
  double a[3], b[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) a[i] = sj[6 + i] - si[6 + i] - g[i] * dt;   // :89
  dev_q_rot(ric, a, b);
#pragma unroll
  for (int i = 0; i < 3; ++i) r9[3 + i] = b[i] - pre[4 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) a[i] = sj[3 + i] - si[3 + i] - si[6 + i] * dt - 0.5 * g[i] * dt * dt;   // :93-94
  dev_q_rot(ric, a, b);
#pragma unroll
  for (int i = 0; i < 3; ++i) r9[6 + i] = b[i] - pre[7 + i];
}

// The same residual with keyframe i's rotation given as the unit quaternion qi (w,x,y,z) instead of a scaled axis: the previous
// keyframe's pose reaches pose_inertial_optimization as an SE3 (pose_inertial_optim.rs:94-216), and a round trip through the scaled
// axis would not return its bits.  si supplies translation (3..5) and velocity (6..8).  The body is imu_residual_dev's after its
// first conversion; it is written out rather than shared because routing imu_residual_dev through it reorders the operands of two
// additions in the BA kernels' code.
__device__ __forceinline__ void imu_residual_qi(const double* qi, const double* si, const double* sj, const double* pre, double* r9) {
  const double dt = pre[10];
  double rj[4];
  dev_q_from_scaled_axis(sj, rj);
  const double ric[4] = {qi[0], -qi[1], -qi[2], -qi[3]}, drc[4] = {pre[0], -pre[1], -pre[2], -pre[3]};
  double t[4], err[4];
  dev_q_mul(drc, ric, t);
  dev_q_mul(t, rj, err);
  dev_scaled_axis(err, r9);
  const double g[3] = {0.0, 0.0, -9.81};
  double a[3], b[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) a[i] = sj[6 + i] - si[6 + i] - g[i] * dt;
  dev_q_rot(ric, a, b);
#pragma unroll
  for (int i = 0; i < 3; ++i) r9[3 + i] = b[i] - pre[4 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) a[i] = sj[3 + i] - si[3 + i] - si[6 + i] * dt - 0.5 * g[i] * dt * dt;
  dev_q_rot(ric, a, b);
#pragma unroll
  for (int i = 0; i < 3; ++i) r9[6 + i] = b[i] - pre[7 + i];
}

}  // namespace
