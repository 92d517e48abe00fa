// pnp_kernels.hip — PnP-RANSAC pose estimation on gfx950, all f64.
//
// Replaces solve_pnp_ransac / solve_pnp_ransac_detailed (src/geometry/pnp.rs:29-134): cv::solvePnPRansac with the reference's
// arguments (:71-84) + Rodrigues + the reprojection-error pass of the detailed form (:110-125).  OpenCV's internals are not
// reproduced; the specification the kernels implement keeps its structure and is stated in DESIGN.md §2 and include/orbx.h.
// tests/pnp_spec.py restates it independently in numpy.
//
// Three launches per call, every problem of a batch in each:
//
//   pnp_hypothesis_kernel  one lane per (problem, hypothesis): the counter-based sampler, then Levenberg-Marquardt on the
//                          model_points sample from the prior (6x6 normal equations and Cholesky in registers); writes the
//                          hypothesis' T_cw (R | t | q, 16 doubles) and whether it exists, and clears its inlier count
//   pnp_score_kernel       workgroups over tiles of a problem's correspondences (one to four per lane, in registers); the
//                          hypotheses are staged in LDS 128 at a time, every lane tests its correspondences under each, counts
//                          are reduced per wave (ballot + popcount) and per workgroup in LDS, then added with one integer
//                          atomic per hypothesis and workgroup: the counts do not depend on the order the workgroups run in
//   pnp_refine_kernel      one workgroup per problem: OpenCV's sequential best-model walk over the counts (one lane), the best
//                          hypothesis' inlier mask, LM over those inliers with fixed-order block reductions (no float atomics:
//                          a result is reproducible to the bit), the detailed pass and the result record
//
// A problem's arithmetic never depends on the problem's position in a batch or on the batch around it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "block_dev.hpp"
#include "orbx_internal.hpp"
#include "pose_dev.hpp"
#include "ransac_dev.hpp"

namespace {

constexpr int PNP_MAX_H = 1024;          // hypotheses per problem (max_iterations)
constexpr int PNP_MAX_M = 8;             // model_points
constexpr int PNP_HS = 16;               // doubles per hypothesis slot: R (9, row-major) | t (3) | q (4) of T_cw
constexpr int PNP_SCORE_THREADS = 256;
constexpr int PNP_CHUNK = 128;           // hypotheses staged in LDS at a time (12 KB)
constexpr int PNP_REFINE_THREADS = 256;
constexpr int PNP_NRED = 28;             // LM sums: H upper triangle (21) | rhs (6) | cost

struct PnpPose { double q[4], t[3]; };

__device__ __forceinline__ BaCam pnp_bacam(const orbx_camera& c) {
  BaCam b{};
  b.fx = c.fx; b.fy = c.fy; b.cx = c.cx; b.cy = c.cy;
  return b;
}

// T_cw of a T_wc pose (se3.rs:56-63 with nalgebra's quaternion-vector product)
__device__ __forceinline__ PnpPose pnp_inverse7(const double* wc) {
  PnpPose o;
  se3_inverse7(wc, o.q, o.t);
  return o;
}

__device__ __forceinline__ void pnp_Rt(const PnpPose& P, double* Rt) {
  quat_to_R(P.q, Rt);
  Rt[9] = P.t[0]; Rt[10] = P.t[1]; Rt[11] = P.t[2];
}

// X_c = R X + t, one IEEE operation at a time, left to right (tests/pnp_spec.py writes the same expression)
__device__ __forceinline__ void pnp_xform(const double* Rt, double X0, double X1, double X2, double& x, double& y, double& z) {
  x = Rt[0] * X0 + Rt[1] * X1 + Rt[2] * X2 + Rt[9];
  y = Rt[3] * X0 + Rt[4] * X1 + Rt[5] * X2 + Rt[10];
  z = Rt[6] * X0 + Rt[7] * X1 + Rt[8] * X2 + Rt[11];
}

// OpenCV's inlier test (usac / ptsetreg: the squared error compared as float against the float threshold), no z test; NaN fails
__device__ __forceinline__ bool pnp_is_inlier(const orbx_camera& cam, const double* Rt, double X0, double X1, double X2, double u,
                                              double v, float thr2) {
  double x, y, z;
  pnp_xform(Rt, X0, X1, X2, x, y, z);
  const double iz = 1.0 / z;
  const double du = cam.fx * (x * iz) + cam.cx - u, dv = cam.fy * (y * iz) + cam.cy - v;
  return (float)(du * du + dv * dv) <= thr2;
}

// One correspondence's share of the normal equations at R|t: r = pi(R X + t) - (u, v), J = d r / d delta with delta = (omega, upsilon)
// applied on the left (R <- Exp(omega) R, t <- Exp(omega) t + upsilon): the visual BA's pose block with sqrt w = 1, negated (that block
// is d (obs - pi) / d delta).  Nothing where |z| < 1e-6.  s = H upper triangle row-major (21) | -J^T r (6) | |r|^2.
__device__ __forceinline__ void pnp_accum(const BaCam& bc, const double* Rt, double X0, double X1, double X2, double u, double v,
                                          double (&s)[PNP_NRED]) {
  double x, y, z;
  pnp_xform(Rt, X0, X1, X2, x, y, z);
  if (fabs(z) < 1e-6) return;
  const double iz = 1.0 / z;
  const double r0 = bc.fx * (x * iz) + bc.cx - u, r1 = bc.fy * (y * iz) + bc.cy - v;
  double A[12], B[6];
  obs_jac_from_proj(bc, Rt, x, y, iz, 1.0, A, B);
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) s[k++] += A[i] * A[j] + A[6 + i] * A[6 + j];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) s[21 + i] += A[i] * r0 + A[6 + i] * r1;   // -J^T r = A^T r
  s[27] += r0 * r0 + r1 * r1;
}

// |r|^2 alone (the trial cost)
__device__ __forceinline__ double pnp_cost(const orbx_camera& cam, const double* Rt, double X0, double X1, double X2, double u, double v) {
  double x, y, z;
  pnp_xform(Rt, X0, X1, X2, x, y, z);
  if (fabs(z) < 1e-6) return 0.0;
  const double iz = 1.0 / z;
  const double r0 = cam.fx * (x * iz) + cam.cx - u, r1 = cam.fy * (y * iz) + cam.cy - v;
  return r0 * r0 + r1 * r1;
}

// (H + lambda diag(max(H_ii, 1e-6))) d = rhs by Cholesky; false on a pivot that is not positive (NaN included)
__device__ __forceinline__ bool pnp_solve6(const double (&s)[PNP_NRED], double lambda, double (&d)[6]) {
  double L[6][6];
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) { L[j][i] = s[k]; L[i][j] = s[k]; ++k; }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) L[i][i] = L[i][i] + lambda * fmax(L[i][i], 1e-6);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double a = L[j][j];
#pragma unroll
    for (int c = 0; c < j; ++c) a = a - L[j][c] * L[j][c];
    if (!(a > 0.0)) return false;
    L[j][j] = sqrt(a);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = L[i][j];
#pragma unroll
      for (int c = 0; c < j; ++c) t = t - L[i][c] * L[j][c];
      L[i][j] = t / L[j][j];
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double t = s[21 + i];
#pragma unroll
    for (int c = 0; c < i; ++c) t = t - L[i][c] * y[c];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int c = i + 1; c < 6; ++c) t = t - L[c][i] * d[c];
    d[i] = t / L[i][i];
  }
  return true;
}

__device__ __forceinline__ double pnp_norm6(const double (&d)[6]) {
  return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
}

// R <- Exp(omega) R, t <- Exp(omega) t + upsilon
__device__ __forceinline__ PnpPose pnp_apply(const PnpPose& P, const double (&d)[6]) {
  PnpPose o;
  double e[4], r[3];
  dev_q_from_scaled_axis(d, e);
  dev_q_mul(e, P.q, o.q);
  dev_q_rot(e, P.t, r);
  o.t[0] = r[0] + d[3]; o.t[1] = r[1] + d[4]; o.t[2] = r[2] + d[5];
  return o;
}

// OpenCV's RANSACUpdateNumIters (calib3d/src/ptsetreg.cpp); cvRound = nearest, ties to even
__device__ __forceinline__ int pnp_update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = fmin(fmax(p, 0.0), 1.0);
  ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1.0 - p, 2.2250738585072014e-308);
  double denom = 1.0 - pow(1.0 - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0.0 || -num >= (double)max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

// ---- kernels -----------------------------------------------------------------------------------------------------

// grid (P, ceil(H / 64)), 64 lanes: lane = hypothesis.  hyp [P][H][16], cnt / ok [P][H].
__global__ __launch_bounds__(64) void pnp_hypothesis_kernel(orbx_camera cam, orbx_pnp_config cfg, int max_n, const int* __restrict__ off,
                                                            const double* __restrict__ pts3d, const float* __restrict__ pts2d,
                                                            const double* __restrict__ priors, double* __restrict__ hyp,
                                                            int* __restrict__ cnt, int* __restrict__ ok) {
  const int p = blockIdx.x, h = blockIdx.y * 64 + threadIdx.x, H = cfg.max_iterations, m = cfg.model_points;
  if (h >= H) return;
  const int base = off[p], n = off[p + 1] - base;
  const size_t slot = (size_t)p * H + h;
  int idx[PNP_MAX_M];
#pragma unroll
  for (int j = 0; j < PNP_MAX_M; ++j) idx[j] = j;
  bool valid = n >= 4 && n <= max_n;
  if (valid) valid = n > m ? ransac_sample<PNP_MAX_M>(cfg.seed, h, n, m, idx) : h == 0;   // 4 <= n <= m: one hypothesis from all points [spec]
  const int mu = n > m ? m : n;
  const BaCam bc = pnp_bacam(cam);
  PnpPose cur = pnp_inverse7(priors + 7 * (size_t)p);
  if (valid) {
    double lambda = 1e-3;
    for (int it = 0; it < cfg.hypothesis_iterations; ++it) {
      double Rt[12], s[PNP_NRED];
      pnp_Rt(cur, Rt);
#pragma unroll
      for (int k = 0; k < PNP_NRED; ++k) s[k] = 0.0;
#pragma unroll
      for (int k = 0; k < PNP_MAX_M; ++k) {
        if (k >= mu) break;
        const size_t i = (size_t)base + idx[k];
        pnp_accum(bc, Rt, pts3d[3 * i], pts3d[3 * i + 1], pts3d[3 * i + 2], (double)pts2d[2 * i], (double)pts2d[2 * i + 1], s);
      }
      double d[6];
      if (!pnp_solve6(s, lambda, d)) break;
      if (pnp_norm6(d) < 1e-10) break;
      const PnpPose trial = pnp_apply(cur, d);
      double tRt[12], tc = 0.0;
      pnp_Rt(trial, tRt);
#pragma unroll
      for (int k = 0; k < PNP_MAX_M; ++k) {
        if (k >= mu) break;
        const size_t i = (size_t)base + idx[k];
        tc += pnp_cost(cam, tRt, pts3d[3 * i], pts3d[3 * i + 1], pts3d[3 * i + 2], (double)pts2d[2 * i], (double)pts2d[2 * i + 1]);
      }
      if (tc < s[27]) { cur = trial; lambda = fmax(lambda * 0.1, 1e-10); }
      else lambda = fmin(lambda * 10.0, 1e10);
    }
  }
  double* o = hyp + slot * PNP_HS;
  pnp_Rt(cur, o);
#pragma unroll
  for (int k = 0; k < 4; ++k) o[12 + k] = cur.q[k];
  cnt[slot] = 0;
  ok[slot] = valid ? 1 : 0;
}

// grid (P, tiles), 256 threads; a tile = 256 * PL consecutive correspondences of one problem, lane t holds t, t + 256, ...
template <int PL>
__global__ __launch_bounds__(PNP_SCORE_THREADS) void pnp_score_kernel(orbx_camera cam, int H, float thr2, int max_n, const int* __restrict__ off,
                                                                      const double* __restrict__ pts3d, const float* __restrict__ pts2d,
                                                                      const double* __restrict__ hyp, const int* __restrict__ ok,
                                                                      int* __restrict__ cnt) {
  __shared__ double sRt[PNP_CHUNK * 12];
  __shared__ int sOk[PNP_CHUNK];
  __shared__ int sCnt[PNP_SCORE_THREADS / 64][PNP_CHUNK];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = off[p], n = off[p + 1] - base;
  const int i0 = blockIdx.y * (PNP_SCORE_THREADS * PL);
  if (n < 4 || n > max_n || i0 >= n) return;                              // (uniform over the workgroup)
  double X[PL][3], U[PL][2];
  bool have[PL];
#pragma unroll
  for (int k = 0; k < PL; ++k) {
    const int i = i0 + k * PNP_SCORE_THREADS + tid;
    have[k] = i < n;
    const size_t g = (size_t)base + (have[k] ? i : 0);
    X[k][0] = pts3d[3 * g]; X[k][1] = pts3d[3 * g + 1]; X[k][2] = pts3d[3 * g + 2];
    U[k][0] = (double)pts2d[2 * g]; U[k][1] = (double)pts2d[2 * g + 1];
  }
  const double* hp = hyp + (size_t)p * H * PNP_HS;
  for (int c0 = 0; c0 < H; c0 += PNP_CHUNK) {
    const int nc = min(PNP_CHUNK, H - c0);
    __syncthreads();                                                      // (the previous chunk's LDS is no longer read)
    for (int e = tid; e < nc * 12; e += PNP_SCORE_THREADS) sRt[e] = hp[(size_t)(c0 + e / 12) * PNP_HS + e % 12];
    for (int e = tid; e < nc; e += PNP_SCORE_THREADS) sOk[e] = ok[(size_t)p * H + c0 + e];
    __syncthreads();
    for (int hh = 0; hh < nc; ++hh) {
      if (!sOk[hh]) continue;
      const double* Rt = sRt + 12 * hh;
      int c = 0;
#pragma unroll
      for (int k = 0; k < PL; ++k) {
        const bool in = have[k] && pnp_is_inlier(cam, Rt, X[k][0], X[k][1], X[k][2], U[k][0], U[k][1], thr2);
        c += __popcll(__ballot(in));
      }
      if (lane == 0) sCnt[wave][hh] = c;
    }
    __syncthreads();
    for (int hh = tid; hh < nc; hh += PNP_SCORE_THREADS) {
      if (!sOk[hh]) continue;
      int s = 0;
#pragma unroll
      for (int w = 0; w < PNP_SCORE_THREADS / 64; ++w) s += sCnt[w][hh];
      if (s) atomicAdd(cnt + (size_t)p * H + c0 + hh, s);
    }
  }
}

// grid P, 256 threads: select + refine + detailed pass of one problem
__global__ __launch_bounds__(PNP_REFINE_THREADS) void pnp_refine_kernel(orbx_camera cam, orbx_pnp_config cfg, int max_n, float thr2,
                                                                        const int* __restrict__ off, const double* __restrict__ pts3d,
                                                                        const float* __restrict__ pts2d, const double* __restrict__ priors,
                                                                        const double* __restrict__ hyp, const int* __restrict__ cnt,
                                                                        const int* __restrict__ ok, double* __restrict__ poses_out,
                                                                        uint8_t* __restrict__ inl_out, double* __restrict__ err_out,
                                                                        orbx_pnp_result* __restrict__ results) {
  __shared__ double s_w[(PNP_REFINE_THREADS / 64) * PNP_NRED];
  __shared__ double s_Rt[12], s_tRt[12];
  __shared__ PnpPose s_cur, s_trial;
  __shared__ int s_sel[4];                   // status, best, best_h, evaluated
  __shared__ int s_go, s_iters;
  const int p = blockIdx.x, tid = threadIdx.x, H = cfg.max_iterations, m = cfg.model_points;
  const int base = off[p], n = off[p + 1] - base;
  const double* prior = priors + 7 * (size_t)p;
  const BaCam bc = pnp_bacam(cam);
  if (tid == 0) {
    int status = ORBX_PNP_OK, best = 0, best_h = -1, evaluated = 0;
    const int* c = cnt + (size_t)p * H;
    const int* v = ok + (size_t)p * H;
    if (n < 4) status = ORBX_PNP_TOO_FEW;
    else if (n > max_n) status = ORBX_PNP_OVER_MAX_N;
    else if (n <= m) { best_h = 0; best = c[0]; evaluated = 1; }
    else {
      int niters = H, hh = 0;
      for (; hh < niters; ++hh) {                                         // OpenCV's loop, over the counts of the parallel evaluation
        const int g = v[hh] ? c[hh] : 0;
        if (g > max(best, m - 1)) {
          best = g; best_h = hh;
          niters = pnp_update_num_iters(cfg.confidence, (double)(n - best) / n, m, niters);
        }
      }
      evaluated = hh;
      if (best_h < 0) status = ORBX_PNP_NO_MODEL;
    }
    s_sel[0] = status; s_sel[1] = best; s_sel[2] = best_h; s_sel[3] = evaluated;
    if (status == ORBX_PNP_OK) {
      const double* hp = hyp + ((size_t)p * H + best_h) * PNP_HS;
      for (int k = 0; k < 12; ++k) s_Rt[k] = hp[k];
      for (int k = 0; k < 4; ++k) s_cur.q[k] = hp[12 + k];
      for (int k = 0; k < 3; ++k) s_cur.t[k] = hp[9 + k];
    }
    s_iters = 0;
  }
  __syncthreads();
  const int status = s_sel[0];
  if (status == ORBX_PNP_OK) {
    // the best hypothesis' inliers, with the scoring kernel's expression: the refinement's point set (kept in inl_out until the detailed pass)
    for (int i = tid; i < n; i += PNP_REFINE_THREADS) {
      const size_t g = (size_t)base + i;
      inl_out[g] = pnp_is_inlier(cam, s_Rt, pts3d[3 * g], pts3d[3 * g + 1], pts3d[3 * g + 2], (double)pts2d[2 * g], (double)pts2d[2 * g + 1], thr2);
    }
    double lambda = 1e-3;                                                 // (every thread keeps the same lambda)
    for (int it = 0; it < cfg.refine_iterations; ++it) {
      __syncthreads();
      if (tid == 0) { pnp_Rt(s_cur, s_Rt); s_iters = it + 1; }
      __syncthreads();
      double s[PNP_NRED];
#pragma unroll
      for (int k = 0; k < PNP_NRED; ++k) s[k] = 0.0;
      for (int i = tid; i < n; i += PNP_REFINE_THREADS) {
        const size_t g = (size_t)base + i;
        if (inl_out[g]) pnp_accum(bc, s_Rt, pts3d[3 * g], pts3d[3 * g + 1], pts3d[3 * g + 2], (double)pts2d[2 * g], (double)pts2d[2 * g + 1], s);
      }
      block_sum<PNP_REFINE_THREADS, PNP_NRED>(s, s_w);
      if (tid == 0) {
        double d[6];
        s_go = 0;
        if (pnp_solve6(s, lambda, d) && !(pnp_norm6(d) < 1e-10)) {
          s_trial = pnp_apply(s_cur, d);
          pnp_Rt(s_trial, s_tRt);
          s_go = 1;
        }
      }
      __syncthreads();
      if (!s_go) break;
      double tc[1] = {0.0};
      for (int i = tid; i < n; i += PNP_REFINE_THREADS) {
        const size_t g = (size_t)base + i;
        if (inl_out[g]) tc[0] += pnp_cost(cam, s_tRt, pts3d[3 * g], pts3d[3 * g + 1], pts3d[3 * g + 2], (double)pts2d[2 * g], (double)pts2d[2 * g + 1]);
      }
      block_sum<PNP_REFINE_THREADS, 1>(tc, s_w);
      if (tc[0] < s[27]) { if (tid == 0) s_cur = s_trial; lambda = fmax(lambda * 0.1, 1e-10); }
      else lambda = fmin(lambda * 10.0, 1e10);
    }
    __syncthreads();
  }
  // the pose handed back (T_wc): the refined one inverted, or the prior's bytes
  double* po = poses_out + 7 * (size_t)p;
  if (tid == 0) {
    if (status == ORBX_PNP_OK) {                                          // T_wc = (q_cw^-1, -(q_cw^-1 t_cw))
      const double cw[7] = {s_cur.q[0], s_cur.q[1], s_cur.q[2], s_cur.q[3], s_cur.t[0], s_cur.t[1], s_cur.t[2]};
      se3_inverse7(cw, po, po + 4);
    } else {
      for (int k = 0; k < 7; ++k) po[k] = prior[k];
    }
    // the detailed pass works from the returned T_wc, inverted again, as the reference does (pnp.rs:112-114)
    s_trial = pnp_inverse7(po);
  }
  __syncthreads();
  // detailed pass (pnp.rs:110-125): err = sqrt(du^2 + dv^2) with u = fx x / z + cx, +inf where z <= 0; inlier = err < reproj_error
  double acc[2] = {0.0, 0.0};                                             // inliers, sum err^2 over them
  const PnpPose T = s_trial;
  for (int i = tid; i < n; i += PNP_REFINE_THREADS) {
    const size_t g = (size_t)base + i;
    const double X[3] = {pts3d[3 * g], pts3d[3 * g + 1], pts3d[3 * g + 2]};
    double pc[3];
    dev_q_rot(T.q, X, pc);
    pc[0] = pc[0] + T.t[0]; pc[1] = pc[1] + T.t[1]; pc[2] = pc[2] + T.t[2];
    double err = INFINITY;
    bool in = false;
    if (!(pc[2] <= 0.0)) {
      const double u = cam.fx * pc[0] / pc[2] + cam.cx, v = cam.fy * pc[1] / pc[2] + cam.cy;
      const double du = u - (double)pts2d[2 * g], dv = v - (double)pts2d[2 * g + 1];
      err = sqrt(du * du + dv * dv);
      in = err < cfg.reproj_error;
    }
    err_out[g] = err;
    inl_out[g] = in ? 1 : 0;
    if (in) { acc[0] += 1.0; acc[1] += err * err; }
  }
  block_sum<PNP_REFINE_THREADS, 2>(acc, s_w);
  if (tid == 0) {
    orbx_pnp_result r;
    r.status = status;
    r.n_inliers = (int)acc[0];
    r.ransac_inliers = s_sel[1];
    r.best_hypothesis = s_sel[2];
    r.hypotheses_evaluated = s_sel[3];
    r.refine_iterations = s_iters;
    r.final_rms = acc[0] > 0.0 ? sqrt(acc[1] / acc[0]) : 0.0;
    results[p] = r;
  }
}

int pnp_check_config(orbx_handle* h, const orbx_pnp_config* c, const char* who) {
  if (!c || c->max_iterations < 1 || c->max_iterations > PNP_MAX_H || c->model_points < 4 || c->model_points > PNP_MAX_M ||
      !(c->reproj_error > 0.0) || !(c->confidence >= 0.0 && c->confidence <= 1.0) || c->hypothesis_iterations < 0 ||
      c->hypothesis_iterations > 1000 || c->refine_iterations < 0 || c->refine_iterations > 1000)
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: configuration out of range (include/orbx.h: orbx_pnp_config)", who);
  return ORBX_OK;
}

// The three launches on the handle's stream; every pointer is device memory.
int pnp_launch(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* cfg, int P, int max_n, const int* d_off,
               const double* d_pts3d, const float* d_pts2d, const double* d_priors, double* d_poses, uint8_t* d_inl,
               double* d_err, orbx_pnp_result* d_res) {
  const int H = cfg->max_iterations;
  const size_t slots = (size_t)P * H;
  if (int rc = orbx_reserve(h, h->ws_pnp[0], slots * (PNP_HS * sizeof(double) + 2 * sizeof(int)))) return rc;
  double* d_hyp = (double*)h->ws_pnp[0].p;
  int* d_cnt = (int*)(d_hyp + slots * PNP_HS);
  int* d_ok = d_cnt + slots;
  const float thr2 = (float)(cfg->reproj_error * cfg->reproj_error);
  const orbx_camera c = *cam;
  const orbx_pnp_config g = *cfg;
  orbx_launch(h, "pnp_hypothesis_kernel", false, pnp_hypothesis_kernel, dim3(P, (H + 63) / 64), dim3(64), 0, c, g, max_n, d_off, d_pts3d, d_pts2d, d_priors, d_hyp, d_cnt, d_ok);
  if (max_n >= 4) {
    // one correspondence per lane while that leaves the chip short of workgroups (a single problem spreads over many CUs), four
    // per lane for large batches (a quarter of the atomics and of the LDS staging)
    const int t1 = (max_n + PNP_SCORE_THREADS - 1) / PNP_SCORE_THREADS;
    const bool wide = (long long)P * t1 >= 4LL * h->n_cu;
    orbx_launch(h, "pnp_score_kernel", false, wide ? pnp_score_kernel<4> : pnp_score_kernel<1>, dim3(P, wide ? (max_n + 4 * PNP_SCORE_THREADS - 1) / (4 * PNP_SCORE_THREADS) : t1),
                dim3(PNP_SCORE_THREADS), 0, c, H, thr2, max_n, d_off, d_pts3d, d_pts2d, d_hyp, d_ok, d_cnt);
  }
  orbx_launch(h, "pnp_refine_kernel", false, pnp_refine_kernel, dim3(P), dim3(PNP_REFINE_THREADS), 0, c, g, max_n, thr2, d_off, d_pts3d, d_pts2d, d_priors, d_hyp, d_cnt, d_ok,
              d_poses, d_inl, d_err, d_res);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

}  // namespace

int orbx_pnp_check_config(orbx_handle* h, const orbx_pnp_config* c, const char* who) { return pnp_check_config(h, c, who); }

extern "C" {

void orbx_default_pnp_config(orbx_pnp_config* c) {
  if (!c) return;
  c->max_iterations = 100;        // pnp.rs:78
  c->reproj_error = 8.0;          // :79
  c->confidence = 0.99;           // :80
  c->model_points = 5;            // [spec] OpenCV's model size for SOLVEPNP_ITERATIVE
  c->hypothesis_iterations = 10;  // [spec]
  c->refine_iterations = 20;      // [spec] OpenCV's extrinsic LM
  c->seed = 0;
}

int orbx_pnp_ransac_batch_device(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* cfg, int n_problems, int max_n,
                                 const int* d_offsets, const double* d_pts3d, const float* d_pts2d, const double* d_priors_wc,
                                 double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out, orbx_pnp_result* d_results) {
  if (!h) return ORBX_ERR_INVALID;
  if (int rc = pnp_check_config(h, cfg, "orbx_pnp_ransac_batch_device")) return rc;
  if (!cam || n_problems < 0 || max_n < 0 || (n_problems > 0 && (!d_offsets || !d_priors_wc || !d_poses_wc_out || !d_results)) ||
      (max_n > 0 && (!d_pts3d || !d_pts2d || !d_inlier_out || !d_err_out)))
    return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pnp_ransac_batch_device: bad argument");
  if (n_problems == 0) return ORBX_OK;
  ORBX_HIP(h, hipSetDevice(h->device));
  return pnp_launch(h, cam, cfg, n_problems, max_n, d_offsets, d_pts3d, d_pts2d, d_priors_wc, d_poses_wc_out, d_inlier_out, d_err_out, d_results);
}

int orbx_pnp_ransac_batch(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* cfg, int n_problems, const int* offsets,
                          const double* pts3d, const float* pts2d, const double* priors_wc, double* poses_wc_out,
                          uint8_t* inlier_out, double* err_out, orbx_pnp_result* results) {
  if (!h) return ORBX_ERR_INVALID;
  if (int rc = pnp_check_config(h, cfg, "orbx_pnp_ransac_batch")) return rc;
  if (!cam || n_problems < 0 || (n_problems > 0 && (!offsets || !priors_wc || !poses_wc_out || !results)))
    return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pnp_ransac_batch: bad argument");
  if (n_problems == 0) return ORBX_OK;
  int max_n = 0;
  if (int rc = orbx_check_offsets(h, "orbx_pnp_ransac_batch", "offsets", "problem", n_problems, offsets, &max_n)) return rc;
  const size_t N = (size_t)offsets[n_problems], P = (size_t)n_problems;
  if (N > 0 && (!pts3d || !pts2d || !inlier_out || !err_out)) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pnp_ransac_batch: bad argument");
  ORBX_HIP(h, hipSetDevice(h->device));
  // one blob each way: [offsets | pts3d | priors | pts2d] up, [poses | err | results | inliers] down
  Carve in, out;
  const size_t o_off = in.take(4 * (P + 1)), o_p3 = in.take(24 * N), o_pr = in.take(56 * P), o_p2 = in.take(8 * N);
  const size_t o_po = out.take(56 * P), o_er = out.take(8 * N), o_rs = out.take(sizeof(orbx_pnp_result) * P), o_in = out.take(N);
  HostCall c;
  if (int rc = orbx_host_call_begin(h, h->pin_pnp, h->ws_pnp[1], in.off, out.off, c)) return rc;
  uint8_t *hi = c.hi, *ho = c.ho, *di = c.di, *dout = c.dout;
  std::memcpy(hi + o_off, offsets, 4 * (P + 1));
  if (N) std::memcpy(hi + o_p3, pts3d, 24 * N);
  std::memcpy(hi + o_pr, priors_wc, 56 * P);
  if (N) std::memcpy(hi + o_p2, pts2d, 8 * N);
  if (int rc = orbx_host_call_upload(h, c)) return rc;
  if (int rc = pnp_launch(h, cam, cfg, n_problems, max_n, (const int*)(di + o_off), (const double*)(di + o_p3), (const float*)(di + o_p2),
                          (const double*)(di + o_pr), (double*)(dout + o_po), dout + o_in, (double*)(dout + o_er),
                          (orbx_pnp_result*)(dout + o_rs)))
    return rc;
  if (int rc = orbx_host_call_download(h, c, out.off)) return rc;
  std::memcpy(poses_wc_out, ho + o_po, 56 * P);
  std::memcpy(results, ho + o_rs, sizeof(orbx_pnp_result) * P);
  if (N) { std::memcpy(err_out, ho + o_er, 8 * N); std::memcpy(inlier_out, ho + o_in, N); }
  return ORBX_OK;
}

int orbx_pnp_ransac(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* cfg, int n, const double* pts3d,
                    const float* pts2d, const double* prior_wc, double* pose_wc_out, uint8_t* inlier_out, double* err_out,
                    orbx_pnp_result* result) {
  if (!h) return ORBX_ERR_INVALID;
  if (n < 0 || !prior_wc || !pose_wc_out || !result) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pnp_ransac: bad argument");
  const int offsets[2] = {0, n};
  return orbx_pnp_ransac_batch(h, cam, cfg, 1, offsets, pts3d, pts2d, prior_wc, pose_wc_out, inlier_out, err_out, result);
}

}  // extern "C"
