// triangulate_kernels.hip — the pair loop of triangulate_from_neighbors (src/local_mapping/triangulation.rs:184-293):
// parallax test, method choice, triangulate_dlt (:715-760), validate_triangulation (:776-850), one pair per thread, and the
// ordered compaction of the accepted points.  f64 throughout; -ffp-contract=off keeps every expression one IEEE operation at a time.
#include <cmath>

#include "block_dev.hpp"
#include "orbx_internal.hpp"

namespace {

// UnitQuaternion::to_rotation_matrix, row-major
__device__ __forceinline__ void quat_to_R(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (w * y + x * z);
  R[3] = 2.0 * (w * z + x * y);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);         R[7] = 2.0 * (w * x + y * z);         R[8] = w * w - x * x - y * y + z * z;
}

// per pose in LDS: R_wc [0,9) | R_cw [9,18) | t_cw [18,21) | t_wc [21,24)
#define TRI_POSE_WORDS 24
__device__ __forceinline__ void pose_tables(const double* pose, double* s) {
  quat_to_R(pose, s);
  const double qi[4] = {pose[0], -pose[1], -pose[2], -pose[3]};                 // SE3::inverse: (q^-1, -(q^-1 t))
  quat_to_R(qi, s + 9);
  for (int r = 0; r < 3; ++r) {
    s[18 + r] = -(s[9 + 3 * r] * pose[4] + s[9 + 3 * r + 1] * pose[5] + s[9 + 3 * r + 2] * pose[6]);
    s[21 + r] = pose[4 + r];
  }
}

__device__ __forceinline__ void mat_vec(const double* R, const double* v, double* o) {
  o[0] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  o[1] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  o[2] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
}

// Right singular vector of the smallest singular value of the 4x4 A by one-sided (Hestenes) Jacobi: plane rotations of column
// pairs until the columns are orthogonal; their norms are then the singular values and the accumulated rotations V the right
// singular vectors.  Works on A itself, never on A^T A, so the small singular value keeps its relative accuracy.  Fixed sweeps
// (a 4x4 converges quadratically: 5 or 6 are enough, 10 are spent), fully unrolled inside a sweep so A and V stay in registers.
__device__ __forceinline__ void null_vector4(double A[4][4], double* v) {
  double V[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < 10; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { alpha += A[k][p] * A[k][p]; beta += A[k][q] * A[k][q]; gamma += A[k][p] * A[k][q]; }
        if (gamma == 0.0) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));   // (zeta^2 = inf gives t = 0)
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double ap = A[k][p], aq = A[k][q];
          A[k][p] = c * ap - s * aq; A[k][q] = s * ap + c * aq;
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
        }
      }
  }
  double best = 0.0;
  int bj = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double nj = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) nj += A[k][j] * A[k][j];
    if (j == 0 || nj < best) { best = nj; bj = j; }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = bj == 0 ? V[k][0] : bj == 1 ? V[k][1] : bj == 2 ? V[k][2] : V[k][3];
}

#define TRI_F64_MAX 1.7976931348623157e308

__global__ __launch_bounds__(256) void tri_triangulate_kernel(TriCommon C, TriNeighbour one, const TriNeighbour* __restrict__ many,
                                                              uint16_t* __restrict__ status, double* __restrict__ points) {
  __shared__ double s_pose[2][TRI_POSE_WORDS];
  __shared__ TriNeighbour s_nb;
  if (threadIdx.x == 0) s_nb = many ? many[blockIdx.y] : one;
  __syncthreads();
  if (threadIdx.x < 2) pose_tables(threadIdx.x == 0 ? C.pose1 : s_nb.pose2, s_pose[threadIdx.x]);   // once per workgroup
  __syncthreads();
  const TriNeighbour& N = s_nb;
  const int np = N.n_pairs_dev ? *N.n_pairs_dev : N.n_pairs;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= np) return;
  const size_t slot = (size_t)N.out_base + (size_t)i;
  const int i1 = N.pairs[2 * (size_t)i], i2 = N.pairs[2 * (size_t)i + 1];
  double p[3] = {0.0, 0.0, 0.0};
  unsigned st = ORBX_TRI_CREATED, method = ORBX_TRI_METHOD_DLT;
  auto finish = [&]() {
    status[slot] = (uint16_t)(st | (method << 8));
    points[3 * slot] = p[0]; points[3 * slot + 1] = p[1]; points[3 * slot + 2] = p[2];
  };
  if (i1 < 0 || i1 >= C.n1 || i2 < 0 || i2 >= N.n2) { st = ORBX_TRI_BAD_INDEX; finish(); return; }
  const double* P1 = s_pose[0]; const double* P2 = s_pose[1];
  const orbx_keypoint k1 = C.kp1[i1], k2 = N.kp2[i2];
  const bool has1 = C.has1 && C.has1[i1], has2 = N.has2 && N.has2[i2];                  // :186-187
  double s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
  if (has1) { s1[0] = C.pts1[3 * (size_t)i1]; s1[1] = C.pts1[3 * (size_t)i1 + 1]; s1[2] = C.pts1[3 * (size_t)i1 + 2]; }
  if (has2) { s2[0] = N.pts2[3 * (size_t)i2]; s2[1] = N.pts2[3 * (size_t)i2 + 1]; s2[2] = N.pts2[3 * (size_t)i2 + 2]; }
  const double u1 = (double)k1.x, v1 = (double)k1.y, u2 = (double)k2.x, v2 = (double)k2.y;
  const double xn1[3] = {(u1 - C.cam.cx) / C.cam.fx, (v1 - C.cam.cy) / C.cam.fy, 1.0};  // :194-203
  const double xn2[3] = {(u2 - C.cam.cx) / C.cam.fx, (v2 - C.cam.cy) / C.cam.fy, 1.0};
  double r1[3], r2[3];
  mat_vec(P1, xn1, r1); mat_vec(P2, xn2, r2);
  const double cos_par = (r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2]) /
                         (sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]) * sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]));   // :208
  const double c1 = has1 ? cos(2.0 * atan(C.cam.baseline / 2.0 / s1[2])) : TRI_F64_MAX;     // :211-218
  const double c2 = has2 ? cos(2.0 * atan(C.cam.baseline / 2.0 / s2[2])) : TRI_F64_MAX;
  const double cs = fmin(c1, c2);                                                        // :220-224
  bool have = false;
  if (cos_par < cs && cos_par > 0.0 && (has1 || has2 || cos_par < C.min_parallax_cos)) {  // :227-229
    double A[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                                        // rows of [R_cw | t_cw] (:726-743)
      const double a0 = j < 3 ? P1[9 + j] : P1[18], a1 = j < 3 ? P1[12 + j] : P1[19], a2 = j < 3 ? P1[15 + j] : P1[20];
      const double b0 = j < 3 ? P2[9 + j] : P2[18], b1 = j < 3 ? P2[12 + j] : P2[19], b2 = j < 3 ? P2[15 + j] : P2[20];
      A[0][j] = xn1[0] * a2 - a0; A[1][j] = xn1[1] * a2 - a1;
      A[2][j] = xn2[0] * b2 - b0; A[3][j] = xn2[1] * b2 - b1;
    }
    double v[4];
    null_vector4(A, v);
    if (fabs(v[3]) < 1e-10) { st = ORBX_TRI_DLT_DEGENERATE; finish(); return; }          // :751
    p[0] = v[0] / v[3]; p[1] = v[1] / v[3]; p[2] = v[2] / v[3];
    have = true;
  } else if (has1) {
    if (c1 < c2) { method = ORBX_TRI_METHOD_STEREO_CURRENT; mat_vec(P1, s1, p); p[0] += P1[21]; p[1] += P1[22]; p[2] += P1[23]; have = true; }   // :239-241
    else if (has2) { method = ORBX_TRI_METHOD_STEREO_NEIGHBOUR; mat_vec(P2, s2, p); p[0] += P2[21]; p[1] += P2[22]; p[2] += P2[23]; have = true; }
  } else if (has2) {
    method = ORBX_TRI_METHOD_STEREO_NEIGHBOUR; mat_vec(P2, s2, p); p[0] += P2[21]; p[1] += P2[22]; p[2] += P2[23]; have = true;   // :247-249
  }
  if (!have) { st = ORBX_TRI_SKIPPED; method = ORBX_TRI_METHOD_DLT; finish(); return; }  // :245, :252
  // validate_triangulation (:776-850)
  double pc1[3], pc2[3];
  mat_vec(P1 + 9, p, pc1); pc1[0] += P1[18]; pc1[1] += P1[19]; pc1[2] += P1[20];
  mat_vec(P2 + 9, p, pc2); pc2[0] += P2[18]; pc2[1] += P2[19]; pc2[2] += P2[20];
  if (pc1[2] <= 0.0 || pc2[2] <= 0.0) { st = ORBX_TRI_REJ_DEPTH; finish(); return; }     // :794 (NaN passes, as there)
  {
    const double ex = C.cam.fx * pc1[0] / pc1[2] + C.cam.cx - u1, ey = C.cam.fy * pc1[1] / pc1[2] + C.cam.cy - v1;
    if ((ex * ex + ey * ey) / 1.0 > (has1 ? C.reproj_stereo : C.reproj_mono)) { st = ORBX_TRI_REJ_REPROJ1; finish(); return; }   // :808
  }
  {
    const double ex = C.cam.fx * pc2[0] / pc2[2] + C.cam.cx - u2, ey = C.cam.fy * pc2[1] / pc2[2] + C.cam.cy - v2;
    if ((ex * ex + ey * ey) / 1.0 > (has2 ? C.reproj_stereo : C.reproj_mono)) { st = ORBX_TRI_REJ_REPROJ2; finish(); return; }   // :821
  }
  const double a0 = p[0] - P1[21], a1 = p[1] - P1[22], a2 = p[2] - P1[23], b0 = p[0] - P2[21], b1 = p[1] - P2[22], b2 = p[2] - P2[23];
  const double d1 = sqrt(a0 * a0 + a1 * a1 + a2 * a2), d2 = sqrt(b0 * b0 + b1 * b1 + b2 * b2);   // :826-829
  if (d1 < 1e-6 || d2 < 1e-6) { st = ORBX_TRI_REJ_DIST; finish(); return; }
  const double ratio_dist = d2 / d1;
  const double w1 = (k1.octave >= 0 && k1.octave < 32) ? C.pow12[k1.octave] : pow(1.2, (double)k1.octave);
  const double w2 = (k2.octave >= 0 && k2.octave < 32) ? C.pow12[k2.octave] : pow(1.2, (double)k2.octave);
  const double ratio_oct = w1 / w2;                                                      // :841
  if (ratio_dist * C.scale_factor < ratio_oct || ratio_dist > ratio_oct * C.scale_factor) st = ORBX_TRI_REJ_SCALE;   // :843-844
  finish();
}

// Ordered compaction: one workgroup walks the neighbours in order and each neighbour's pairs in the search's order, 1024 at a
// time; a CREATED pair's place in the list is the running count plus its rank among the CREATED pairs of its chunk (BlockAppend,
// block_dev.hpp: integer only), so the list has the reference's creation order and the same input gives the same bytes.
__global__ __launch_bounds__(1024) void tri_compact_kernel(const TriNeighbour* __restrict__ nbs, int T, const uint16_t* __restrict__ status,
                                                           const double* __restrict__ points, int cap, int* __restrict__ head,
                                                           int* __restrict__ out_nb, int* __restrict__ out_i1, int* __restrict__ out_i2,
                                                           double* __restrict__ out_pts) {
  __shared__ int wave_tot[16 * 2];
  const int tid = threadIdx.x;
  BlockAppend<1024, 2> app(wave_tot);                                        // [0] CREATED: the list goes on over the neighbours, [1] triangulated
  for (int t = 0; t < T; ++t) {
    const int np = nbs[t].n_pairs_dev ? *nbs[t].n_pairs_dev : nbs[t].n_pairs;
    const size_t base = (size_t)nbs[t].out_base;
    const int* pairs = nbs[t].pairs;
    const int start = app.total[0];
    app.total[1] = 0;
    for (int c0 = 0; c0 < np; c0 += 1024) {
      const int i = c0 + tid;
      const unsigned st = i < np ? (status[base + i] & 0xffu) : (unsigned)ORBX_TRI_SKIPPED;
      const bool fl[2] = {st == ORBX_TRI_CREATED,
                          i < np && st != ORBX_TRI_SKIPPED && st != ORBX_TRI_DLT_DEGENERATE && st != ORBX_TRI_BAD_INDEX};   // :260
      int at[2];
      app.round(fl, at);
      if (fl[0]) {
        const int o = at[0];
        if (o < cap) {
          out_nb[o] = t; out_i1[o] = pairs[2 * (size_t)i]; out_i2[o] = pairs[2 * (size_t)i + 1];
          out_pts[3 * (size_t)o] = points[3 * (base + i)]; out_pts[3 * (size_t)o + 1] = points[3 * (base + i) + 1];
          out_pts[3 * (size_t)o + 2] = points[3 * (base + i) + 2];
        }
      }
    }
    if (tid == 0) { head[1 + 4 * t] = 0; head[2 + 4 * t] = np; head[3 + 4 * t] = app.total[1]; head[4 + 4 * t] = app.total[0] - start; }
  }
  if (tid == 0) head[0] = app.total[0];
}

}  // namespace

void tri_common_fill(TriCommon* c, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial) {
  c->cam = *cam;
  c->min_parallax_cos = is_inertial ? std::cos(cfg->min_parallax_inertial) : std::cos(cfg->min_parallax_visual);   // :110-114
  c->reproj_mono = cfg->max_reproj_error_mono; c->reproj_stereo = cfg->max_reproj_error_stereo; c->scale_factor = cfg->scale_ratio_factor;
  for (int o = 0; o < 32; ++o) c->pow12[o] = std::pow(1.2, (double)o);                  // scale_factor.powf(octave), :838-841
}

int launch_triangulate_pairs(orbx_handle* h, const TriCommon& c, const TriNeighbour& one, const TriNeighbour* d_many, int T, int max_pairs,
                             uint16_t* d_status, double* d_points) {
  if (T <= 0 || max_pairs <= 0) return ORBX_OK;
  orbx_launch(h, "tri_triangulate_kernel", false, tri_triangulate_kernel, dim3((max_pairs + 255) / 256, T), dim3(256), 0, c, one, d_many, d_status, d_points);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

int launch_triangulate_compact(orbx_handle* h, const TriNeighbour* d_many, int T, const uint16_t* d_status, const double* d_points, int cap,
                               int* d_head, int* d_out_nb, int* d_out_idx1, int* d_out_idx2, double* d_out_points) {
  orbx_launch(h, "tri_compact_kernel", false, tri_compact_kernel, dim3(1), dim3(1024), 0, d_many, T, d_status, d_points, cap, d_head, d_out_nb, d_out_idx1, d_out_idx2, d_out_points);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

extern "C" {

void orbx_default_triangulation_config(orbx_triangulation_config* cfg) {
  if (!cfg) return;
  cfg->num_neighbors = 10; cfg->max_descriptor_dist = 50; cfg->min_baseline_ratio = 0.01;
  cfg->min_parallax_inertial = std::acos(0.9996); cfg->min_parallax_visual = std::acos(0.9998);
  cfg->max_reproj_error_mono = 5.991; cfg->max_reproj_error_stereo = 7.8; cfg->scale_ratio_factor = 1.5;
}

int orbx_triangulate_pairs_device(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                                  const orbx_keypoint* d_kp1, const double* d_points_cam1, const uint8_t* d_has_point1, int n1,
                                  const double* pose1_wc, const orbx_keypoint* d_kp2, const double* d_points_cam2,
                                  const uint8_t* d_has_point2, int n2, const double* pose2_wc, const int* d_pairs, int n_pairs,
                                  double* d_out_points, uint16_t* d_out_status) {
  if (!h) return ORBX_ERR_INVALID;
  if (!cam || !cfg || n1 < 0 || n2 < 0 || n_pairs < 0 || !pose1_wc || !pose2_wc || (n1 > 0 && !d_kp1) || (n2 > 0 && !d_kp2) ||
      ((d_points_cam1 == nullptr) != (d_has_point1 == nullptr)) || ((d_points_cam2 == nullptr) != (d_has_point2 == nullptr)) ||
      (n_pairs > 0 && (!d_pairs || !d_out_points || !d_out_status)))
    return orbx_fail(h, ORBX_ERR_INVALID, "orbx_triangulate_pairs_device: bad argument");
  if (n_pairs == 0) return ORBX_OK;
  ORBX_HIP(h, hipSetDevice(h->device));
  TriCommon c{};
  tri_common_fill(&c, cam, cfg, is_inertial);
  c.kp1 = d_kp1; c.pts1 = d_points_cam1; c.has1 = d_has_point1; c.n1 = n1;
  memcpy(c.pose1, pose1_wc, sizeof(c.pose1));
  TriNeighbour nb{};
  nb.kp2 = d_kp2; nb.pts2 = d_points_cam2; nb.has2 = d_has_point2; nb.n2 = n2;
  memcpy(nb.pose2, pose2_wc, sizeof(nb.pose2));
  nb.pairs = d_pairs; nb.n_pairs_dev = nullptr; nb.n_pairs = n_pairs; nb.out_base = 0;
  return launch_triangulate_pairs(h, c, nb, nullptr, 1, n_pairs, d_out_status, d_out_points);
}

int orbx_triangulate_pairs(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                           const orbx_keypoint* kp1, const double* points_cam1, const uint8_t* has_point1, int n1, const double* pose1_wc,
                           const orbx_keypoint* kp2, const double* points_cam2, const uint8_t* has_point2, int n2, const double* pose2_wc,
                           const int* pairs, int n_pairs, double* out_points, uint16_t* out_status) {
  if (!h) return ORBX_ERR_INVALID;
  if (!cam || !cfg || n1 < 0 || n2 < 0 || n_pairs < 0 || !pose1_wc || !pose2_wc || (n1 > 0 && !kp1) || (n2 > 0 && !kp2) ||
      ((points_cam1 == nullptr) != (has_point1 == nullptr)) || ((points_cam2 == nullptr) != (has_point2 == nullptr)) ||
      (n_pairs > 0 && (!pairs || !out_points || !out_status)))
    return orbx_fail(h, ORBX_ERR_INVALID, "orbx_triangulate_pairs: bad argument");
  for (int i = 0; i < n_pairs; ++i)
    if (pairs[2 * (size_t)i] < 0 || pairs[2 * (size_t)i] >= n1 || pairs[2 * (size_t)i + 1] < 0 || pairs[2 * (size_t)i + 1] >= n2)
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_triangulate_pairs: pair %d = (%d, %d) is out of range (n1 %d, n2 %d)", i, pairs[2 * (size_t)i],
                       pairs[2 * (size_t)i + 1], n1, n2);
  if (n_pairs == 0) return ORBX_OK;
  ORBX_HIP(h, hipSetDevice(h->device));
  const size_t N1 = (size_t)std::max(n1, 1), N2 = (size_t)std::max(n2, 1), NP = (size_t)n_pairs;
  Carve in;
  const size_t i_kp1 = in.take(sizeof(orbx_keypoint) * N1), i_kp2 = in.take(sizeof(orbx_keypoint) * N2), i_p1 = in.take(24 * N1), i_p2 = in.take(24 * N2),
               i_pr = in.take(8 * NP), i_h1 = in.take(N1), i_h2 = in.take(N2);
  OutputPlan out;
  const auto p_op = out.add(out_points, 3 * NP);
  const auto p_st = out.add(out_status, NP);
  if (int rc = out.begin(h, h->pin_io, h->ws_io.host_blob, in.off)) return rc;
  uint8_t *hi = out.call.hi, *di = out.call.di;
  if (n1 > 0) memcpy(hi + i_kp1, kp1, sizeof(orbx_keypoint) * (size_t)n1);
  if (n2 > 0) memcpy(hi + i_kp2, kp2, sizeof(orbx_keypoint) * (size_t)n2);
  if (n1 > 0 && points_cam1) { memcpy(hi + i_p1, points_cam1, 24 * (size_t)n1); memcpy(hi + i_h1, has_point1, (size_t)n1); }
  if (n2 > 0 && points_cam2) { memcpy(hi + i_p2, points_cam2, 24 * (size_t)n2); memcpy(hi + i_h2, has_point2, (size_t)n2); }
  memcpy(hi + i_pr, pairs, 8 * NP);
  if (int rc = orbx_host_call_upload(h, out.call)) return rc;
  if (int rc = orbx_triangulate_pairs_device(h, cam, cfg, is_inertial, (const orbx_keypoint*)(di + i_kp1), points_cam1 ? (const double*)(di + i_p1) : nullptr,
                                             points_cam1 ? di + i_h1 : nullptr, n1, pose1_wc, (const orbx_keypoint*)(di + i_kp2),
                                             points_cam2 ? (const double*)(di + i_p2) : nullptr, points_cam2 ? di + i_h2 : nullptr, n2, pose2_wc,
                                             (const int*)(di + i_pr), n_pairs, out.dev(p_op), out.dev(p_st)))
    return rc;
  return out.finish(h);
}

}  // extern "C"
