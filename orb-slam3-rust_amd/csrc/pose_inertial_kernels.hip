// pose_inertial_kernels.hip — pose-inertial optimization for tracking on gfx950, all f64.
//
// Replaces pose_inertial_optimization (src/optimizer/pose_inertial_optim.rs:94-216) as refine_with_imu calls it
// (src/tracking/tracker.rs:476-546).  The specification is the reference's loop, restated in include/orbx.h and DESIGN.md §2;
// tests/pose_inertial_spec.py restates it independently in numpy.
//
// One launch per call, one 256-thread workgroup per problem running all of that problem's iterations:
//   - every lane walks its strided observations in a fixed order and accumulates the 21 upper entries of the visual J^T J, the 6
//     of J^T r and the count of masked-in observations in registers; lanes 0-15 of the last wave evaluate the IMU residual at the
//     parameters and at the 15 forward-difference points
//   - a fixed-order reduction: a shuffle tree inside each wave, then the four wave totals in wave order
//   - wave 0 assembles the 15x15 system in registers (lane r holds row r and the right-hand side), damps it and runs nalgebra's
//     partial-pivoting LU and the two triangular solves with cross-lane reads (v_readlane); lanes 0-14 add delta to the parameters in LDS
//   - every lane reclassifies its observations at the new pose; the mask lives in the caller's inlier_out (no LDS in proportion
//     to n, so no limit on n); the count is a ballot + popcount per wave
// Every reduction has a fixed order, so a problem's result does not depend on the batch around it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbx_internal.hpp"
#include "pose_dev.hpp"

namespace {

constexpr int PI_THREADS = 256;
constexpr int PI_WAVES = PI_THREADS / 64;
constexpr int PI_MAX_ITER = 64;
constexpr int PI_NRED = 28;              // visual sums: J^T J upper triangle (21) | J^T r (6) | masked-in count
constexpr double PI_EPS = 1e-6;          // pose_inertial_optim.rs:405

struct PiArgs {
  const int* off;
  const double* pts3d;
  const float* pts2d;
  const uint8_t* stereo;
  const double *pose, *vel, *bias, *prev_pose, *prev_vel, *preint;
  double *pose_out, *vel_out, *bias_out;
  uint8_t* inl;
  orbx_pose_inertial_result* res;
};

// index of entry (a, b), a <= b, of the 6x6 upper triangle, row by row
__host__ __device__ constexpr int pi_ut(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }

// x of lane k, k the same in every lane (v_readlane: no LDS round trip, unlike a shuffle)
__device__ __forceinline__ double pi_lane(double x, int k) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), k), hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
  return __hiloint2double(hi, lo);
}

// T_cw of the parameters' pose: q_cw = conj(from_scaled_axis(par[0..3])), t_cw = -(q_cw * t_wc)  (extract_pose, se3.rs:56-63)
__device__ __forceinline__ void pi_pose_cw(const double* par, double* qcw, double* tcw) {
  double wc[7];
  dev_q_from_scaled_axis(par, wc);
  wc[4] = par[3]; wc[5] = par[4]; wc[6] = par[5];
  se3_inverse7(wc, qcw, tcw);
}

// p_cam = q_cw * X + t_cw (SE3::transform_point)
__device__ __forceinline__ void pi_xform(const double* qcw, const double* tcw, const double* __restrict__ X, double* p) {
  const double x[3] = {X[0], X[1], X[2]};
  dev_q_rot(qcw, x, p);
  p[0] = p[0] + tcw[0]; p[1] = p[1] + tcw[1]; p[2] = p[2] + tcw[2];
}

// grid P, 256 threads: every iteration of one problem
__global__ __launch_bounds__(PI_THREADS) void pose_inertial_kernel(orbx_camera cam, orbx_pose_inertial_config cfg, PiArgs a) {
  __shared__ double s_par[16];
  __shared__ double s_w[PI_WAVES][PI_NRED];
  __shared__ double s_imu[16][9];              // [0] r(params), [1 + j] r(params + eps e_j)
  __shared__ int s_cnt[PI_WAVES];
  __shared__ int s_stop;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = a.off[p], n = a.off[p + 1] - base;
  const double* X = a.pts3d + 3 * (size_t)base;
  const float* uv = a.pts2d + 2 * (size_t)base;
  const uint8_t* st = a.stereo + base;
  uint8_t* inl = a.inl + base;
  if (tid == 0) {
    const double* q = a.pose + 7 * (size_t)p;
    dev_scaled_axis(q, s_par);
    for (int k = 0; k < 3; ++k) s_par[3 + k] = q[4 + k];
    for (int k = 0; k < 3; ++k) s_par[6 + k] = a.vel[3 * (size_t)p + k];
    for (int k = 0; k < 6; ++k) s_par[9 + k] = a.bias[6 * (size_t)p + k];
    s_par[15] = 0.0;
    s_stop = 0;
  }
  for (int i = tid; i < n; i += PI_THREADS) inl[i] = 1;     // inlier_mask = vec![true; n]
  // the IMU lanes keep the previous keyframe's state and the preintegration in registers
  const bool imu_lane = wave == PI_WAVES - 1 && lane < 16;
  double qi[4] = {1.0, 0.0, 0.0, 0.0}, si[9] = {}, pre[11] = {};
  if (imu_lane) {
    for (int k = 0; k < 4; ++k) qi[k] = a.prev_pose[7 * (size_t)p + k];
    for (int k = 0; k < 3; ++k) si[3 + k] = a.prev_pose[7 * (size_t)p + 4 + k];
    for (int k = 0; k < 3; ++k) si[6 + k] = a.prev_vel[3 * (size_t)p + k];
    for (int k = 0; k < 11; ++k) pre[k] = a.preint[11 * (size_t)p + k];
  }
  const double w_imu = cfg.imu_weight;
  int iterations = 0, status = ORBX_POSE_INERTIAL_OK, reclassified = 0;
  __syncthreads();
  double qcw[4], tcw[3];
  pi_pose_cw(s_par, qcw, tcw);
  for (int it = 0; it < cfg.max_iterations; ++it) {
    iterations = it + 1;
    const double progress = (double)it / (double)max(cfg.max_iterations - 1, 1);
    const double chi2_mono = cfg.chi2_mono_init * (1.0 - progress) + cfg.chi2_mono_final * progress;
    const double chi2_stereo = cfg.chi2_stereo_init * (1.0 - progress) + cfg.chi2_stereo_final * progress;
    // ---- visual rows of the masked-in observations (compute_reprojection_error_with_jacobian, :250-349)
    double s[PI_NRED];
#pragma unroll
    for (int k = 0; k < PI_NRED; ++k) s[k] = 0.0;
    for (int i = tid; i < n; i += PI_THREADS) {
      if (!inl[i]) continue;
      s[27] += 1.0;
      double pc[3];
      pi_xform(qcw, tcw, X + 3 * (size_t)i, pc);
      if (pc[2] <= 0.001) continue;                          // e = (100, 100), a zero block: nothing to add
      const double x = pc[0], y = pc[1], z = pc[2];
      const double z_inv = 1.0 / z, z_inv_sq = z_inv * z_inv;
      const double e0 = (double)uv[2 * i] - (cam.fx * x * z_inv + cam.cx);
      const double e1 = (double)uv[2 * i + 1] - (cam.fy * y * z_inv + cam.cy);
      const double xy = x * y, x_sq = x * x, y_sq = y * y;
      const double J0[6] = {-cam.fx * xy * z_inv_sq, cam.fx * (1.0 + x_sq * z_inv_sq), -cam.fx * y * z_inv,
                            cam.fx * z_inv, 0.0, -cam.fx * x * z_inv_sq};
      const double J1[6] = {-cam.fy * (1.0 + y_sq * z_inv_sq), cam.fy * xy * z_inv_sq, cam.fy * x * z_inv,
                            0.0, cam.fy * z_inv, -cam.fy * y * z_inv_sq};
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = r; c < 6; ++c) s[pi_ut(r, c)] += J0[r] * J0[c] + J1[r] * J1[c];
        s[21 + r] += J0[r] * e0 + J1[r] * e1;
      }
    }
    // ---- IMU residual at the parameters and at the 15 forward-difference points (:396-428)
    if (imu_lane) {
      double sj[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) sj[k] = s_par[k];
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if (lane == 1 + k) sj[k] = sj[k] + PI_EPS;           // lanes 10-15 perturb a bias, which r does not read
      double r9[9];
      imu_residual_qi(qi, si, sj, pre, r9);
#pragma unroll
      for (int k = 0; k < 9; ++k) s_imu[lane][k] = r9[k];
    }
    // ---- fixed-order reduction: shuffle tree per wave, wave totals through LDS
#pragma unroll
    for (int k = 0; k < PI_NRED; ++k) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) s[k] += __shfl_xor(s[k], o);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < PI_NRED; ++k) s_w[wave][k] = s[k];
    }
    __syncthreads();
    if (wave == 0) {
      double t[PI_NRED];
#pragma unroll
      for (int k = 0; k < PI_NRED; ++k) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < PI_WAVES; ++w) v += s_w[w][k];
        t[k] = v;
      }
      int stop = 0;
      if (t[27] < 5.0) stop = 1;                              // num_active < 5 (:153-156)
      double delta = 0.0;
      if (!stop) {
        // lane r < 15 assembles row r of [H | -g]: the visual block, then the 9 IMU rows (:159-161), then the damping (:164-168)
        const int r = lane < 15 ? lane : 0;
        double Jr[9], rw[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          rw[k] = s_imu[0][k] * w_imu;
          Jr[k] = (s_imu[1 + r][k] - s_imu[0][k]) / PI_EPS * w_imu;
        }
        double row[16];
#pragma unroll
        for (int c = 0; c < 15; ++c) {
          double h = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q)
            if (c < 6 && q == r) h = t[pi_ut(min(q, c), max(q, c))];
          double hi = 0.0;
#pragma unroll
          for (int k = 0; k < 9; ++k) hi += Jr[k] * ((s_imu[1 + c][k] - s_imu[0][k]) / PI_EPS * w_imu);
          row[c] = h + hi;
        }
        double g = 0.0, gi = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q)
          if (q == r) g = t[21 + q];
#pragma unroll
        for (int k = 0; k < 9; ++k) gi += Jr[k] * rw[k];
        g = g + gi;
        row[15] = -g;
#pragma unroll
        for (int c = 0; c < 15; ++c)
          if (c == r) row[c] = row[c] + 1e-3 * fmax(row[c], 1e-6);
        if (lane >= 15) {
#pragma unroll
          for (int c = 0; c < 16; ++c) row[c] = 0.0;
        }
        // nalgebra LU (partial pivoting: the first largest |value| of the column) and its solve: P, unit lower, upper
#pragma unroll
        for (int i = 0; i < 15; ++i) {
          int piv = i;
          double best = fabs(pi_lane(row[i], i));
#pragma unroll
          for (int q = i + 1; q < 15; ++q) {
            const double v = fabs(pi_lane(row[i], q));
            if (v > best) { best = v; piv = q; }
          }
          piv = __builtin_amdgcn_readfirstlane(piv);
          const double diag = pi_lane(row[i], piv);
          if (diag == 0.0) { stop = 2; break; }
          double prow[16];
#pragma unroll
          for (int c = i; c < 16; ++c) {
            prow[c] = pi_lane(row[c], piv);
            const double ic = pi_lane(row[c], i);
            if (lane == piv) row[c] = ic;
          }
          if (lane == i) {
#pragma unroll
            for (int c = i; c < 16; ++c) row[c] = prow[c];
          }
          const double inv_diag = 1.0 / diag;
          if (lane > i && lane < 15) {
            const double l = row[i] * inv_diag;
#pragma unroll
            for (int c = i + 1; c < 16; ++c) row[c] = -prow[c] * l + row[c];
          }
        }
        if (!stop) {
#pragma unroll
          for (int i = 14; i >= 0; --i) {
            const double x = pi_lane(row[15], i) / pi_lane(row[i], i);
            if (lane == i) row[15] = x;
            if (lane < i) row[15] = -x * row[i] + row[15];
          }
          delta = row[15];
        }
      }
      if (!stop && lane < 15) s_par[lane] = s_par[lane] + delta;   // params += delta (:177)
      if (lane == 0) s_stop = stop;
    }
    __syncthreads();
    const int stop = s_stop;
    if (stop) { status = stop == 1 ? ORBX_POSE_INERTIAL_TOO_FEW : ORBX_POSE_INERTIAL_SINGULAR; break; }
    // ---- reclassify every observation at the new pose (compute_reprojection_error, :227-248; :180-186)
    pi_pose_cw(s_par, qcw, tcw);
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += PI_THREADS) {
      const int i = i0 + tid;
      bool in = false;
      if (i < n) {
        double pc[3];
        pi_xform(qcw, tcw, X + 3 * (size_t)i, pc);
        double e0 = 100.0, e1 = 100.0;
        if (!(pc[2] <= 0.001)) {
          e0 = (double)uv[2 * i] - (cam.fx * pc[0] / pc[2] + cam.cx);
          e1 = (double)uv[2 * i + 1] - (cam.fy * pc[1] / pc[2] + cam.cy);
        }
        in = e0 * e0 + e1 * e1 < (st[i] ? chi2_stereo : chi2_mono);
        inl[i] = in ? 1 : 0;
      }
      cnt += __popcll(__ballot(in));
    }
    if (lane == 0) s_cnt[wave] = cnt;
    reclassified = 1;
  }
  __syncthreads();
  if (tid == 0) {
    int inliers = n;                                          // the mask as initialised
    if (reclassified) {
      inliers = 0;
      for (int w = 0; w < PI_WAVES; ++w) inliers += s_cnt[w];
    }
    double q[4];
    dev_q_from_scaled_axis(s_par, q);
    double* po = a.pose_out + 7 * (size_t)p;
    for (int k = 0; k < 4; ++k) po[k] = q[k];
    for (int k = 0; k < 3; ++k) po[4 + k] = s_par[3 + k];
    for (int k = 0; k < 3; ++k) a.vel_out[3 * (size_t)p + k] = s_par[6 + k];
    for (int k = 0; k < 6; ++k) a.bias_out[6 * (size_t)p + k] = s_par[9 + k];
    orbx_pose_inertial_result r;
    r.status = status;
    r.num_inliers = inliers;
    r.num_observations = n;
    r.iterations = iterations;
    a.res[p] = r;
  }
}

int pi_check_config(orbx_handle* h, const orbx_pose_inertial_config* c, const char* who) {
  if (!c || c->max_iterations < 0 || c->max_iterations > PI_MAX_ITER || !(c->chi2_mono_init > 0.0) || !(c->chi2_stereo_init > 0.0) ||
      !(c->chi2_mono_final > 0.0) || !(c->chi2_stereo_final > 0.0) || !std::isfinite(c->imu_weight) || !(c->imu_weight >= 0.0))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: configuration out of range (include/orbx.h: orbx_pose_inertial_config)", who);
  return ORBX_OK;
}

int pi_launch(orbx_handle* h, const orbx_camera* cam, const orbx_pose_inertial_config* cfg, int P, const PiArgs& a) {
  orbx_launch(h, "pose_inertial_kernel", false, pose_inertial_kernel, dim3(P), dim3(PI_THREADS), 0, *cam, *cfg, a);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

}  // namespace

extern "C" {

void orbx_default_pose_inertial_config(orbx_pose_inertial_config* c) {
  if (!c) return;
  c->max_iterations = 4;          // pose_inertial_optim.rs:37
  c->chi2_mono_init = 12.0;       // :38
  c->chi2_stereo_init = 15.6;     // :39
  c->chi2_mono_final = 5.991;     // :40
  c->chi2_stereo_final = 7.815;   // :41
  c->imu_weight = 1.0;            // :42
}

int orbx_pose_inertial_batch_device(orbx_handle* h, const orbx_camera* cam, const orbx_pose_inertial_config* cfg, int n_problems,
                                    const int* d_offsets, const double* d_pts3d, const float* d_pts2d, const uint8_t* d_is_stereo,
                                    const double* d_poses_wc, const double* d_velocities, const double* d_biases,
                                    const double* d_prev_kf_poses_wc, const double* d_prev_kf_velocities, const double* d_preints,
                                    double* d_poses_out, double* d_velocities_out, double* d_biases_out, uint8_t* d_inlier_out,
                                    orbx_pose_inertial_result* d_results) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_pose_inertial_batch_device", [&]() -> int {
    if (int rc = pi_check_config(h, cfg, "orbx_pose_inertial_batch_device")) return rc;
    if (!cam || n_problems < 0 ||
        (n_problems > 0 && (!d_offsets || !d_pts3d || !d_pts2d || !d_is_stereo || !d_poses_wc || !d_velocities || !d_biases ||
                            !d_prev_kf_poses_wc || !d_prev_kf_velocities || !d_preints || !d_poses_out || !d_velocities_out ||
                            !d_biases_out || !d_inlier_out || !d_results)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pose_inertial_batch_device: bad argument");
    if (n_problems == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    const PiArgs a{d_offsets, d_pts3d, d_pts2d, d_is_stereo, d_poses_wc, d_velocities, d_biases, d_prev_kf_poses_wc, d_prev_kf_velocities,
                   d_preints, d_poses_out, d_velocities_out, d_biases_out, d_inlier_out, d_results};
    return pi_launch(h, cam, cfg, n_problems, a);
  });
}

int orbx_pose_inertial_batch(orbx_handle* h, const orbx_camera* cam, const orbx_pose_inertial_config* cfg, int n_problems,
                             const int* offsets, const double* pts3d, const float* pts2d, const uint8_t* is_stereo,
                             const double* poses_wc, const double* velocities, const double* biases, const double* prev_kf_poses_wc,
                             const double* prev_kf_velocities, const double* preints, double* poses_out, double* velocities_out,
                             double* biases_out, uint8_t* inlier_out, orbx_pose_inertial_result* results) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_pose_inertial_batch", [&]() -> int {
    if (int rc = pi_check_config(h, cfg, "orbx_pose_inertial_batch")) return rc;
    if (!cam || n_problems < 0 ||
        (n_problems > 0 && (!offsets || !poses_wc || !velocities || !biases || !prev_kf_poses_wc || !prev_kf_velocities || !preints ||
                            !poses_out || !velocities_out || !biases_out || !results)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pose_inertial_batch: bad argument");
    if (n_problems == 0) return ORBX_OK;
    if (int rc = orbx_check_offsets(h, "orbx_pose_inertial_batch", "offsets", "problem", n_problems, offsets)) return rc;
    const size_t N = (size_t)offsets[n_problems], P = (size_t)n_problems;
    if (N > 0 && (!pts3d || !pts2d || !is_stereo)) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pose_inertial_batch: bad argument");
    ORBX_HIP(h, hipSetDevice(h->device));
    // one blob each way: [offsets | pts3d | poses | velocities | biases | prev poses | prev velocities | preints | pts2d | is_stereo] up,
    // [poses | velocities | biases | results | inliers] down
    Carve in, out;
    const size_t o_off = in.take(4 * (P + 1)), o_p3 = in.take(24 * N), o_po = in.take(56 * P), o_ve = in.take(24 * P), o_bi = in.take(48 * P),
                 o_pp = in.take(56 * P), o_pv = in.take(24 * P), o_pr = in.take(88 * P), o_p2 = in.take(8 * N), o_st = in.take(N);
    const size_t d_po = out.take(56 * P), d_ve = out.take(24 * P), d_bi = out.take(48 * P), d_rs = out.take(sizeof(orbx_pose_inertial_result) * P),
                 d_in = out.take(N);
    HostCall c;
    if (int rc = orbx_host_call_begin(h, h->pin_pi, h->ws_pi, in.off, out.off, c)) return rc;
    uint8_t *hi = c.hi, *ho = c.ho, *di = c.di, *dout = c.dout;
    std::memcpy(hi + o_off, offsets, 4 * (P + 1));
    if (N) std::memcpy(hi + o_p3, pts3d, 24 * N);
    std::memcpy(hi + o_po, poses_wc, 56 * P);
    std::memcpy(hi + o_ve, velocities, 24 * P);
    std::memcpy(hi + o_bi, biases, 48 * P);
    std::memcpy(hi + o_pp, prev_kf_poses_wc, 56 * P);
    std::memcpy(hi + o_pv, prev_kf_velocities, 24 * P);
    std::memcpy(hi + o_pr, preints, 88 * P);
    if (N) { std::memcpy(hi + o_p2, pts2d, 8 * N); std::memcpy(hi + o_st, is_stereo, N); }
    if (int rc = orbx_host_call_upload(h, c)) return rc;
    const PiArgs a{(const int*)(di + o_off), (const double*)(di + o_p3), (const float*)(di + o_p2), di + o_st, (const double*)(di + o_po),
                   (const double*)(di + o_ve), (const double*)(di + o_bi), (const double*)(di + o_pp), (const double*)(di + o_pv),
                   (const double*)(di + o_pr), (double*)(dout + d_po), (double*)(dout + d_ve), (double*)(dout + d_bi), dout + d_in,
                   (orbx_pose_inertial_result*)(dout + d_rs)};
    if (int rc = pi_launch(h, cam, cfg, n_problems, a)) return rc;
    if (int rc = orbx_host_call_download(h, c, inlier_out ? out.off : d_in)) return rc;   // the inlier flags travel only when asked for
    std::memcpy(poses_out, ho + d_po, 56 * P);
    std::memcpy(velocities_out, ho + d_ve, 24 * P);
    std::memcpy(biases_out, ho + d_bi, 48 * P);
    std::memcpy(results, ho + d_rs, sizeof(orbx_pose_inertial_result) * P);
    if (N && inlier_out) std::memcpy(inlier_out, ho + d_in, N);
    return ORBX_OK;
  });
}

int orbx_pose_inertial_optimize(orbx_handle* h, const orbx_camera* cam, const orbx_pose_inertial_config* cfg, const double* pose_wc,
                                const double* velocity, const double* bias, const double* prev_kf_pose_wc, const double* prev_kf_velocity,
                                const double* preint, int n, const double* pts3d, const float* pts2d, const uint8_t* is_stereo,
                                double* pose_out, double* velocity_out, double* bias_out, uint8_t* inlier_out,
                                orbx_pose_inertial_result* result) {
  if (!h) return ORBX_ERR_INVALID;
  if (n < 0) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_pose_inertial_optimize: bad argument");
  const int offsets[2] = {0, n};
  return orbx_pose_inertial_batch(h, cam, cfg, 1, offsets, pts3d, pts2d, is_stereo, pose_wc, velocity, bias, prev_kf_pose_wc,
                                  prev_kf_velocity, preint, pose_out, velocity_out, bias_out, inlier_out, result);
}

}  // extern "C"
