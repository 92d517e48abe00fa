// global_ba_kernels.hip — global bundle adjustment over a whole map on gfx950, all f64.
//
// orbx_ba_solve_global_map[_obs32[_device]]: solve_global_ba (src/optimizer/global_ba.rs:184-418) with the semantics of
// orbx_ba_solve_global (ba_kernels.hip), for more optimised keyframes than the local-window solver's kernels hold (128): up to
// GBA_MAX_K.  The window solver keeps R|t of every keyframe in LDS, a [M][K] slot map and a reduced system planned for n <= 768; none of
// that is here.  R|t [K][12] lives in global memory and is read per observation, the lists are per-point observer lists and
// per-keyframe observation lists only, and the reduced system S (6K x 6K, lower triangle, row-major, the right-hand side as row n) is
// factored in global memory.
//
// Once per call:
//   gba_ingest_kernel    index check of every observation (either wire format), observations per point and per keyframe
//   gba_scan_kernel      pt_start, kf_start
//   gba_place_kernel     observation index -> its point's segment
//   gba_order_kernel     per point: the segment into input order; o_kf / o_pt / o_uv in point-major order
//   gba_kfplace_kernel   point-major index -> its keyframe's segment
//   gba_kforder_kernel   per keyframe: the segment into ascending order; kf_obs / kf_pt
// One LM iteration:
//   gba_pose_kernel      R|t of the current parameters, iteration counter
//   gba_build_kernel     one thread per map point: residual, Huber weight, V, g_l, the damped V* = L L^T, M = L^-1, V*^-1 g_l, M g_l;
//                        per observation the six numbers (x, y, 1/z, sqrt w, r0, r1) and Z = W M^T (6 x 3), so that
//                        W_a V*^-1 W_b^T = Z_a Z_b^T
//   gba_kf_schur_kernel  one workgroup per block row i of S: zeroes the row, U_i*, g_p, b_red in a fixed order, then walks keyframe
//                        i's observations in list order and subtracts Z_a Z_b^T from block (i, kf(b)) for every observer b of the
//                        observation's point with kf(b) <= i.  Wave w owns the block columns with kf % 16 == w and lane e the entry e
//                        of a block, so every entry of S is only ever touched by one lane, in list order: no atomics, fixed sums
//   gba_panel_kernel     per 64-column panel: every workgroup (one wave) factors the diagonal block in LDS (workgroup 0 stores it), then
//                        solves its 64 rows below the panel, one thread per row, the right-hand side being the last row
//   gba_syrk_kernel      per panel: the trailing update S22 -= L21 L21^T of the lower 64 x 64 blocks on v_mfma_f64_16x16x4_f64
//   gba_back_kernel      per panel, last to first: L^T x = y
//   gba_pose_trial_kernel  trial poses and their R|t, |delta_p|^2, |p|^2 per keyframe
//   gba_backsub_kernel   one thread per map point: delta_l = -(V*^-1 g_l + M^T sum Z^T delta_p), the trial point, trial residuals
//   gba_decide_kernel    the sums in a fixed tree, accept / reject, lambda, stop tests (global_ba.rs = local_ba_lm.rs:1004-1056)
// and gba_finish_kernel: the result record and the current parameters into the output blob.
//
// Launches per factorisation with p = ceil(6K / 64) panels: a panel launch and a backward-substitution launch per panel and a trailing
// update behind every panel but the last, 3 p - 1: 38 at K = 129 (p = 13), 281 at K = 999 (p = 94), 290 at K = 1025 (p = 97);
// 16-column panels would be 385 panels there.
//
// The per-observation arithmetic (obs_terms, pose_to_Rt, the point matrices) restates ba_kernels.hip's device functions: they are
// private copies, so that ba_kernels.hip compiles to the code it compiled to before.
#include <algorithm>
#include <cmath>

#include "block_dev.hpp"
#include "orbx_internal.hpp"
#include "pose_dev.hpp"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int GBA_MAX_K = 2048;      // optimised keyframes per call: S [6K + 1][6K] doubles = 1.2 GB there
constexpr int GBA_NB = 64;           // columns per panel
constexpr int GBA_KF_THREADS = 1024, GBA_KF_WAVES = GBA_KF_THREADS / 64;

struct GbaState {
  double lambda, cur_sq, final_sq, init_sq, gtol, ptol;
  int done, iters, sel;
  int bad;        // 0, or INT_MAX - (index of the first observation with an index out of range)
  int fail;       // this iteration's factorisation met a pivot that is not positive
  int pad_;
};

// What every kernel of a solve reads: sizes and device pointers (passed by value).
struct GbaArgs {
  int K, M, N, n, ld;                 // n = 6K; ld: doubles per row of S (n rounded up to the panel width)
  int obs32;                          // the caller's observations are orbx_ba_obs32
  GbaState* S;
  double *P0, *P1;                    // the two parameter buffers [6K | 3M]
  const double* Rt_fix;               // [2][12]: the anchor, the identity
  const void* obs_raw;
  int *pt_cnt, *pt_start, *kf_cnt, *kf_start, *kf_fill;
  int *obs_tmp, *kf_tmp, *o_kf, *o_pt, *kf_obs, *kf_pt;
  double *o_uv, *oP, *Z;
  double *Rt_cur, *Rt_trial;
  double *Mz, *vg, *mg, *pt_chi2, *pt_glsq, *pt_dsq, *pt_psq, *pt_tchi;
  double *kf_gsq, *kf_dsq, *kf_psq;
  double *dp, *Sg;
  double *Ld;                         // [panels][64][64]: the factored diagonal blocks (the workgroups of a panel launch all read the unfactored one in S)
};
__device__ __forceinline__ double* gba_cur(const GbaArgs& a) { return a.S->sel ? a.P1 : a.P0; }
__device__ __forceinline__ double* gba_trial(const GbaArgs& a) { return a.S->sel ? a.P0 : a.P1; }

// se3_from_params (local_ba_lm.rs:648-662) then R|t (ba_kernels.hip: pose_to_Rt, visual form)
__device__ __forceinline__ void gba_pose_to_Rt(const double* p, double* o) {
  double q[4];
  const double angle = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  if (angle > 1e-10) {
    double a0 = p[0] / angle, a1 = p[1] / angle, a2 = p[2] / angle;
    const double n = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    a0 /= n; a1 /= n; a2 /= n;
    const double s = sin(angle / 2.0), c = cos(angle / 2.0);
    q[0] = c; q[1] = a0 * s; q[2] = a1 * s; q[3] = a2 * s;
  } else {
    q[0] = 1; q[1] = q[2] = q[3] = 0;
  }
  quat_to_R(q, o);
  o[9] = p[3]; o[10] = p[4]; o[11] = p[5];
}

// One observation (ba_kernels.hip: obs_terms, global form): the point in the camera frame, chi2 with the Huber weight, and with
// want_jac the weighted residual, 1/z and sqrt w (both zero where the Jacobian rows are: |z| < 1e-6 or z <= 0.001, global_ba.rs:561-563)
struct GbaObs { double x, y, piz, sw, r0, r1, chi; };
__device__ __forceinline__ void gba_obs_terms(const BaCam& cam, const double* Rt, const double* X, double u, double v, bool want_jac, GbaObs& o) {
  const double x = fma(Rt[0], X[0], fma(Rt[1], X[1], fma(Rt[2], X[2], Rt[9])));
  const double y = fma(Rt[3], X[0], fma(Rt[4], X[1], fma(Rt[5], X[2], Rt[10])));
  const double z = fma(Rt[6], X[0], fma(Rt[7], X[1], fma(Rt[8], X[2], Rt[11])));
  o.x = x; o.y = y; o.piz = 0.0; o.sw = 0.0; o.r0 = 0.0; o.r1 = 0.0;
  const bool behind = z <= 0.001;
  const double zi = 1.0 / z;
  double e0 = 100.0, e1 = 100.0;
  if (!behind) { e0 = u - fma(cam.fx * x, zi, cam.cx); e1 = v - fma(cam.fy * y, zi, cam.cy); }
  const double s2 = fma(e0, e0, e1 * e1);
  double sw = 1.0;
  if (s2 <= cam.huber * cam.huber) o.chi = s2;
  else {
    const double en = sqrt(s2);
    o.chi = cam.huber * en;
    if (want_jac) sw = sqrt(cam.huber / en);
  }
  if (!want_jac) return;
  o.r0 = e0 * sw; o.r1 = e1 * sw;
  if (!(fabs(z) < 1e-6 || behind)) { o.piz = zi; o.sw = sw; }
}
__device__ __forceinline__ const double* gba_obs_Rt(const GbaArgs& a, const double* Rt_kf, int k) {
  return k >= 0 ? Rt_kf + 12 * (size_t)k : a.Rt_fix + 12 * (size_t)(-1 - k);
}

// ---- once per call: the lists ---------------------------------------------------------------------------------------------------
// (kf, mp) of observation i: kf >= 0 an optimised keyframe, -1 the anchor, -2 the identity pose (an observation that names neither,
// local_ba_lm.rs:569), -3 out of range.  The rules are the window solver's with F = 1 (ba_kernels.hip: ba_obs_ids, ba_prep_count_kernel),
// so that the two global entry points answer the same for the same array: in the 32-byte form ANY kf_idx < 0 names a fixed observer,
// fixed_idx 0 the anchor, ANY fixed_idx < 0 the identity pose, fixed_idx >= 1 is out of range; in the 16-byte form kf_idx -1 is the
// anchor, -2 the identity pose (-1 - F), anything below out of range.
__device__ __forceinline__ int2 gba_obs_ids(const GbaArgs& a, int i) {
  int kf, fx, mp;
  if (a.obs32) {
    const int2 q = *reinterpret_cast<const int2*>(reinterpret_cast<const orbx_ba_obs32*>(a.obs_raw) + i);
    const int f = -1 - q.x;
    kf = q.x >= 0 ? q.x : -1; fx = (q.x >= 0 || f == 1) ? -1 : f; mp = q.y;
  } else {
    const int4 q = *reinterpret_cast<const int4*>(reinterpret_cast<const orbx_ba_obs*>(a.obs_raw) + i);
    kf = q.x; fx = q.y; mp = q.z;
  }
  if (mp < 0 || mp >= a.M || kf >= a.K || (kf < 0 && fx >= 1)) return make_int2(-3, mp);
  return make_int2(kf >= 0 ? kf : (fx == 0 ? -1 : -2), mp);
}
__global__ __launch_bounds__(256) void gba_ingest_kernel(GbaArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  const int2 q = gba_obs_ids(a, i);
  if (q.x == -3) { atomicMax(&a.S->bad, 0x7fffffff - i); return; }
  atomicAdd(&a.pt_cnt[q.y], 1);
  if (q.x >= 0) atomicAdd(&a.kf_cnt[q.x], 1);
}
// one workgroup: exclusive scans; the counters are left zeroed for the place passes.  An index out of range ends the solve here.
__global__ __launch_bounds__(1024) void gba_scan_kernel(GbaArgs a) {
  __shared__ int s_wave[16];
  const int tid = threadIdx.x;
  if (a.S->bad != 0) {                                                      // (uniform: written by the launch before)
    __syncthreads();
    if (tid == 0) a.S->done = 1;
    return;
  }
  {
    BlockScan<1024> scan(s_wave);
    for (int j0 = 0; j0 < a.M; j0 += 1024) {
      const int j = j0 + tid;
      const int c = j < a.M ? a.pt_cnt[j] : 0;
      if (j < a.M) a.pt_cnt[j] = 0;
      const int at = scan.round(c);
      if (j < a.M) a.pt_start[j] = at;
    }
    if (tid == 0) a.pt_start[a.M] = scan.total;
  }
  BlockScan<1024> scan(s_wave);
  for (int k0 = 0; k0 < a.K; k0 += 1024) {
    const int k = k0 + tid;
    const int c = k < a.K ? a.kf_cnt[k] : 0;
    const int at = scan.round(c);
    if (k < a.K) a.kf_start[k] = at;
  }
  if (tid == 0) a.kf_start[a.K] = scan.total;
}
__global__ __launch_bounds__(256) void gba_place_kernel(GbaArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (a.S->done || i >= a.N) return;
  const int mp = gba_obs_ids(a, i).y;
  a.obs_tmp[a.pt_start[mp] + atomicAdd(&a.pt_cnt[mp], 1)] = i;
}
// one thread per map point: its observation indices into ascending (= input) order by counting, for each, the smaller ones
__global__ __launch_bounds__(256) void gba_order_kernel(GbaArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (a.S->done || j >= a.M) return;
  const int s = a.pt_start[j], cnt = a.pt_start[j + 1] - s;
  const int* __restrict__ tmp = a.obs_tmp + s;
  for (int e = 0; e < cnt; ++e) {
    const int idx = tmp[e];
    int rank = 0;
    for (int k = 0; k < cnt; ++k) rank += tmp[k] < idx ? 1 : 0;
    const size_t t = (size_t)(s + rank);
    a.o_kf[t] = gba_obs_ids(a, idx).x;
    a.o_pt[t] = j;
    if (a.obs32) {                                                          // f32 -> f64: exact, the host's `as f64`
      const float2 f = *reinterpret_cast<const float2*>(&reinterpret_cast<const orbx_ba_obs32*>(a.obs_raw)[idx].u);
      a.o_uv[2 * t] = (double)f.x; a.o_uv[2 * t + 1] = (double)f.y;
    } else {
      const orbx_ba_obs* o = reinterpret_cast<const orbx_ba_obs*>(a.obs_raw) + idx;
      a.o_uv[2 * t] = o->u; a.o_uv[2 * t + 1] = o->v;
    }
  }
}
__global__ __launch_bounds__(256) void gba_kfplace_kernel(GbaArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (a.S->done || t >= a.N) return;
  const int k = a.o_kf[t];
  if (k >= 0) a.kf_tmp[a.kf_start[k] + atomicAdd(&a.kf_fill[k], 1)] = t;
}
// one workgroup per keyframe: its observations (point-major indices) into ascending order, and their map points
__global__ __launch_bounds__(256) void gba_kforder_kernel(GbaArgs a) {
  const int k = blockIdx.x;
  if (a.S->done) return;
  const int s = a.kf_start[k], cnt = a.kf_start[k + 1] - s;
  const int* __restrict__ tmp = a.kf_tmp + s;
  for (int e = threadIdx.x; e < cnt; e += 256) {
    const int t = tmp[e];
    int rank = 0;
    for (int q = 0; q < cnt; ++q) rank += tmp[q] < t ? 1 : 0;
    a.kf_obs[s + rank] = t;
    a.kf_pt[s + rank] = a.o_pt[t];
  }
}

// ---- one LM iteration -----------------------------------------------------------------------------------------------------------
// iter < 0: the pass that only computes the initial error (no iteration is counted)
__global__ __launch_bounds__(256) void gba_pose_kernel(GbaArgs a, int iter) {
  if (a.S->done) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) { if (iter >= 0) a.S->iters = iter + 1; a.S->fail = 0; }      // local_ba_lm.rs:1017
  if (k >= a.K) return;
  gba_pose_to_Rt(gba_cur(a) + 6 * (size_t)k, a.Rt_cur + 12 * (size_t)k);
}

__global__ __launch_bounds__(256) void gba_build_kernel(GbaArgs a, BaCam cam) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (a.S->done || j >= a.M) return;
  const double lambda = a.S->lambda;
  const double* Xp = gba_cur(a) + 6 * (size_t)a.K + 3 * (size_t)j;
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  const int t0 = a.pt_start[j], t1 = a.pt_start[j + 1];
  double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, chi = 0.0;
  for (int t = t0; t < t1; ++t) {
    const int k = a.o_kf[t];
    const double* Rt = gba_obs_Rt(a, a.Rt_cur, k);
    GbaObs o;
    gba_obs_terms(cam, Rt, X, a.o_uv[2 * (size_t)t], a.o_uv[2 * (size_t)t + 1], true, o);
    double* q = a.oP + 6 * (size_t)t;
    q[0] = o.x; q[1] = o.y; q[2] = o.piz; q[3] = o.sw; q[4] = o.r0; q[5] = o.r1;
    chi += o.chi;
    double A[12], B[6];
    obs_jac_from_proj(cam, Rt, o.x, o.y, o.piz, o.sw, A, B);
    V[0] = fma(B[0], B[0], fma(B[3], B[3], V[0]));
    V[1] = fma(B[0], B[1], fma(B[3], B[4], V[1]));
    V[2] = fma(B[0], B[2], fma(B[3], B[5], V[2]));
    V[3] = fma(B[1], B[1], fma(B[4], B[4], V[3]));
    V[4] = fma(B[1], B[2], fma(B[4], B[5], V[4]));
    V[5] = fma(B[2], B[2], fma(B[5], B[5], V[5]));
    g[0] = fma(B[0], o.r0, fma(B[3], o.r1, g[0]));
    g[1] = fma(B[1], o.r0, fma(B[4], o.r1, g[1]));
    g[2] = fma(B[2], o.r0, fma(B[5], o.r1, g[2]));
  }
  // damped V* = V + lambda max(diag, 1e-6) (:1031-1034) = L L^T, M = L^-1 (m00, m10, m11, m20, m21, m22), V*^-1 = M^T M
  const double a_ = V[0] + lambda * fmax(V[0], 1e-6), b_ = V[1], c_ = V[2];
  const double d_ = V[3] + lambda * fmax(V[3], 1e-6), e_ = V[4], f_ = V[5] + lambda * fmax(V[5], 1e-6);
  const double m00 = 1.0 / sqrt(a_), l10 = b_ * m00, l20 = c_ * m00;
  const double m11 = 1.0 / sqrt(fmax(d_ - l10 * l10, 0.0)), l21 = (e_ - l20 * l10) * m11;
  const double m22 = 1.0 / sqrt(fmax(f_ - l20 * l20 - l21 * l21, 0.0));
  const double m10 = -(l10 * m00) * m11, m21 = -(l21 * m11) * m22, m20 = -(l20 * m00 + l21 * m10) * m22;
  double* Mz = a.Mz + 6 * (size_t)j;
  Mz[0] = m00; Mz[1] = m10; Mz[2] = m11; Mz[3] = m20; Mz[4] = m21; Mz[5] = m22;
  const double mg0 = m00 * g[0], mg1 = m10 * g[0] + m11 * g[1], mg2 = m20 * g[0] + m21 * g[1] + m22 * g[2];       // M g_l
  a.mg[3 * (size_t)j] = mg0; a.mg[3 * (size_t)j + 1] = mg1; a.mg[3 * (size_t)j + 2] = mg2;
  a.vg[3 * (size_t)j] = m00 * mg0 + m10 * mg1 + m20 * mg2;                                                     // V*^-1 g_l = M^T M g_l
  a.vg[3 * (size_t)j + 1] = m11 * mg1 + m21 * mg2;
  a.vg[3 * (size_t)j + 2] = m22 * mg2;
  a.pt_chi2[j] = chi;
  a.pt_glsq[j] = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
  // Z = W M^T, W = A^T B (6 x 3), of every observation by an optimised keyframe
  for (int t = t0; t < t1; ++t) {
    const int k = a.o_kf[t];
    if (k < 0) continue;
    const double* q = a.oP + 6 * (size_t)t;
    double A[12], B[6];
    obs_jac_from_proj(cam, a.Rt_cur + 12 * (size_t)k, q[0], q[1], q[2], q[3], A, B);
    double* Zt = a.Z + 18 * (size_t)t;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double w0 = A[r] * B[0] + A[6 + r] * B[3], w1 = A[r] * B[1] + A[6 + r] * B[4], w2 = A[r] * B[2] + A[6 + r] * B[5];
      Zt[3 * r] = w0 * m00;
      Zt[3 * r + 1] = w0 * m10 + w1 * m11;
      Zt[3 * r + 2] = w0 * m20 + w1 * m21 + w2 * m22;
    }
  }
}

// Block row i of S.  Lane e of a wave: e < 36 the entry (e / 6, e % 6) of a 6 x 6 block, 36 <= e < 42 g_p, 42 <= e < 48 b_red.
__global__ __launch_bounds__(GBA_KF_THREADS) void gba_kf_schur_kernel(GbaArgs a, BaCam cam) {
  __shared__ double s_part[GBA_KF_WAVES][48];
  __shared__ double s_sum[48];
  __shared__ double s_Rt[12];
  if (a.S->done) return;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.n, ld = a.ld;
  double* __restrict__ Sg = a.Sg;
  // the row's blocks (i, 0 .. i): zero
  const int width = 6 * (i + 1);
  for (int e = tid; e < 6 * width; e += GBA_KF_THREADS) Sg[(size_t)(6 * i + e / width) * ld + e % width] = 0.0;
  if (tid < 12) s_Rt[tid] = a.Rt_cur[12 * (size_t)i + tid];
  __syncthreads();
  const int q0 = a.kf_start[i], q1 = a.kf_start[i + 1];
  // U_i = sum A^T A, g_p = sum A^T r, b_red = sum Z (M g_l): wave w takes the list entries w, w + 16, ...; the waves' sums in wave order
  {
    double acc = 0.0;
    const int ra = lane < 36 ? lane / 6 : (lane < 42 ? lane - 36 : (lane < 48 ? lane - 42 : 0)), rb = lane < 36 ? lane % 6 : 0;
    for (int q = q0 + wave; q < q1; q += GBA_KF_WAVES) {
      const int t = a.kf_obs[q];
      const double* p = a.oP + 6 * (size_t)t;
      double A[12], B[6];
      obs_jac_from_proj(cam, s_Rt, p[0], p[1], p[2], p[3], A, B);
      if (lane < 36) acc += A[ra] * A[rb] + A[6 + ra] * A[6 + rb];
      else if (lane < 42) acc += A[ra] * p[4] + A[6 + ra] * p[5];
      else if (lane < 48) {
        const double* Zt = a.Z + 18 * (size_t)t + 3 * ra;
        const double* mg = a.mg + 3 * (size_t)a.kf_pt[q];
        acc += Zt[0] * mg[0] + Zt[1] * mg[1] + Zt[2] * mg[2];
      }
    }
    if (lane < 48) s_part[wave][lane] = acc;
    __syncthreads();
    if (tid < 48) {
      double s = 0.0;
      for (int w = 0; w < GBA_KF_WAVES; ++w) s += s_part[w][tid];
      s_sum[tid] = s;
    }
    __syncthreads();
    if (tid < 36 && rb <= ra) {
      double u = s_sum[tid];
      if (ra == rb) u += a.S->lambda * fmax(u, 1e-6);                        // :1031-1034
      Sg[(size_t)(6 * i + ra) * ld + 6 * i + rb] = u;
    }
    if (tid < 6) Sg[(size_t)n * ld + 6 * i + tid] = -s_sum[36 + tid] + s_sum[42 + tid];   // the right-hand side: -g_p + b_red
    if (tid == 0) {
      double s = 0.0;
      for (int r = 0; r < 6; ++r) s += s_sum[36 + r] * s_sum[36 + r];
      a.kf_gsq[i] = s;
    }
    __syncthreads();
  }
  // S(i, kb) -= Z_a Z_b^T over keyframe i's observations a in list order and the observers b of a's point in point-major order
  const int ea = lane / 6, eb = lane % 6;
  for (int qc = q0; qc < q1; qc += 64) {
    const int qm = min(qc + lane, q1 - 1);
    const int my_t = a.kf_obs[qm], my_j = a.kf_pt[qm];
    const int my_s = a.pt_start[my_j], my_e = a.pt_start[my_j + 1];
    const int cnt = min(64, q1 - qc);
    for (int qq = 0; qq < cnt; ++qq) {
      const int ta = __shfl(my_t, qq), s = __shfl(my_s, qq), e = __shfl(my_e, qq);
      double za0 = 0.0, za1 = 0.0, za2 = 0.0;
      if (lane < 36) { const double* Za = a.Z + 18 * (size_t)ta + 3 * ea; za0 = Za[0]; za1 = Za[1]; za2 = Za[2]; }
      for (int tc = s; tc < e; tc += 64) {
        const int t = tc + lane;
        const int kb = t < e ? a.o_kf[t] : -1;
        unsigned long long hits = __ballot(kb >= 0 && kb <= i && (kb & (GBA_KF_WAVES - 1)) == wave);
        while (hits) {
          const int l = __ffsll((long long)hits) - 1;
          hits &= hits - 1;
          const int kbl = __shfl(kb, l);
          if (lane < 36 && (kbl < i || eb <= ea)) {
            const double* Zb = a.Z + 18 * (size_t)(tc + l) + 3 * eb;
            double* dst = Sg + (size_t)(6 * i + ea) * ld + 6 * kbl + eb;
            *dst -= za0 * Zb[0] + za1 * Zb[1] + za2 * Zb[2];
          }
        }
      }
    }
  }
}

// Panel c0, one wave per workgroup: the diagonal 64 x 64 block (rows / columns beyond n: the identity) is factored in LDS by every
// workgroup — thread r owns row r, left-looking — and stored by workgroup 0; then L21 = S21 L11^-T for the workgroup's 64 rows below
// the panel, thread r solving row r against the packed factor (row n is the right-hand side).  The rows live in LDS, not in
// registers: a row of 64 doubles per thread with both loops unrolled made the compiler spill 3800 registers (460 us per launch).
constexpr int GBA_PANEL_ROWS = 64;
__global__ __launch_bounds__(64) void gba_panel_kernel(GbaArgs a, int c0) {
  __shared__ double U[GBA_NB][GBA_NB + 1];                 // the diagonal block while it is factored, then the workgroup's rows
  __shared__ double Dp[GBA_NB * (GBA_NB + 1) / 2];         // L11, lower triangle packed by rows
  __shared__ double rinv[GBA_NB];
  if (a.S->done || a.S->fail) return;
  const int n = a.n, ld = a.ld, tid = threadIdx.x;
  double* __restrict__ Sg = a.Sg;
  const int nb = min(GBA_NB, n - c0);
  for (int e = tid; e < GBA_NB * GBA_NB; e += 64) {
    const int r = e / GBA_NB, c = e % GBA_NB;
    double v = r == c ? 1.0 : 0.0;
    if (c0 + r < n && c <= r) v = Sg[(size_t)(c0 + r) * ld + c0 + c];
    U[r][c] = v;
  }
  __syncthreads();
  // left-looking: column k of L from the finished columns before it — sums that only read, one store per entry
  __shared__ double s_piv;
  bool ok = true;
  for (int k = 0; k < GBA_NB; ++k) {
    double s = 0.0;
    if (tid >= k) {
      s = U[tid][k];
#pragma unroll 4
      for (int m = 0; m < k; ++m) s = fma(-U[tid][m], U[k][m], s);
      if (tid == k) s_piv = s;
    }
    __syncthreads();
    const double d = s_piv;
    if (!(d > 0.0)) { ok = false; break; }                                  // (uniform: every thread reads the same pivot)
    const double ri = 1.0 / sqrt(d);
    if (tid == k) { U[k][k] = d * ri; rinv[k] = ri; }
    else if (tid > k) U[tid][k] = s * ri;
    __syncthreads();
  }
  if (!ok) { if (blockIdx.x == 0 && tid == 0) a.S->fail = 1; return; }
  for (int c = 0; c <= tid; ++c) Dp[tid * (tid + 1) / 2 + c] = U[tid][c];
  if (blockIdx.x == 0)
    for (int e = tid; e < GBA_NB * GBA_NB; e += 64) a.Ld[(size_t)(c0 / GBA_NB) * GBA_NB * GBA_NB + e] = U[e / GBA_NB][e % GBA_NB];
  __syncthreads();
  // the workgroup's rows: the rows below the panel in order, then the right-hand side
  const int first = blockIdx.x * GBA_PANEL_ROWS, below = max(0, n - (c0 + GBA_NB));
  for (int e = tid; e < GBA_PANEL_ROWS * GBA_NB; e += 64) {
    const int r = e / GBA_NB, c = e % GBA_NB, i = first + r;
    const int row = i < below ? c0 + GBA_NB + i : (i == below ? n : -1);
    U[r][c] = row >= 0 && c < nb ? Sg[(size_t)row * ld + c0 + c] : 0.0;
  }
  __syncthreads();
  for (int k = 0; k < GBA_NB; ++k) {
    double s = U[tid][k];
    const double* Lk = Dp + k * (k + 1) / 2;
#pragma unroll 4
    for (int m = 0; m < k; ++m) s = fma(-U[tid][m], Lk[m], s);
    U[tid][k] = s * rinv[k];
  }
  __syncthreads();
  for (int e = tid; e < GBA_PANEL_ROWS * GBA_NB; e += 64) {
    const int r = e / GBA_NB, c = e % GBA_NB, i = first + r;
    const int row = i < below ? c0 + GBA_NB + i : (i == below ? n : -1);
    if (row >= 0 && c < nb) Sg[(size_t)row * ld + c0 + c] = U[r][c];
  }
}

// Trailing update behind panel c0: the lower 64 x 64 blocks (bi >= bj) of rows [c0 + 64, n] x columns [c0 + 64, n) lose L_bi L_bj^T.
// Four waves, each 16 rows x 64 columns: four tiles of v_mfma_f64_16x16x4_f64 (lane l feeds A[l & 15][l >> 4], B[l >> 4][l & 15] and
// holds C[(l >> 4) + 4 q][l & 15] in register q).  Every entry belongs to one lane: no atomics.
__global__ __launch_bounds__(256) void gba_syrk_kernel(GbaArgs a, int c0) {
  constexpr int KC = 32, PITCH = KC + 2;
  __shared__ double As[GBA_NB][PITCH], Bs[GBA_NB][PITCH];
  if (a.S->done || a.S->fail) return;
  const int n = a.n, ld = a.ld, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* __restrict__ Sg = a.Sg;
  int bi = 0, rem = blockIdx.x;
  while (rem > bi) { rem -= bi + 1; ++bi; }
  const int bj = rem;
  const int r0 = c0 + GBA_NB * (1 + bi), cb0 = c0 + GBA_NB * (1 + bj);
  double4_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int kc = 0; kc < GBA_NB; kc += KC) {
    __syncthreads();
    for (int e = tid; e < GBA_NB * KC; e += 256) {
      const int r = e / KC, c = e % KC;
      As[r][c] = r0 + r <= n ? Sg[(size_t)(r0 + r) * ld + c0 + kc + c] : 0.0;
      Bs[r][c] = cb0 + r <= n ? Sg[(size_t)(cb0 + r) * ld + c0 + kc + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KC / 4; ++q) {
      const double av = As[16 * wave + (lane & 15)][(lane >> 4) + 4 * q];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[16 * t + (lane & 15)][(lane >> 4) + 4 * q], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int col = cb0 + 16 * t + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = r0 + 16 * wave + (lane >> 4) + 4 * q;
      if (row <= n && col < n && col <= row) Sg[(size_t)row * ld + col] -= acc[t][q];
    }
  }
}

// Backward substitution, panel c0 (the launches run from the last panel to the first): x_p from L11^T x_p = y_p by wave 0 of every
// workgroup, then y[c] -= sum_k L[c0 + k][c] x_p[k] for the workgroup's columns c < c0.  y is row n of S.
__global__ __launch_bounds__(256) void gba_back_kernel(GbaArgs a, int c0) {
  __shared__ double D[GBA_NB][GBA_NB + 1];
  __shared__ double xs[GBA_NB];
  if (a.S->done || a.S->fail) return;
  const int n = a.n, ld = a.ld, tid = threadIdx.x;
  double* __restrict__ Sg = a.Sg;
  double* __restrict__ y = Sg + (size_t)n * ld;
  const int nb = min(GBA_NB, n - c0);
  for (int e = tid; e < GBA_NB * GBA_NB; e += 256) {
    const int r = e / GBA_NB, c = e % GBA_NB;
    D[r][c] = c <= r ? a.Ld[(size_t)(c0 / GBA_NB) * GBA_NB * GBA_NB + e] : 0.0;
  }
  __syncthreads();
  if (tid < 64) {
    double yi = tid < nb ? y[c0 + tid] : 0.0, xi = 0.0;
    for (int k = GBA_NB - 1; k >= 0; --k) {
      const double xk = __shfl(yi, k) / D[k][k];
      if (tid == k) xi = xk;
      if (tid < k) yi = fma(-D[k][tid], xk, yi);
    }
    xs[tid] = xi;
    if (blockIdx.x == 0 && tid < nb) a.dp[c0 + tid] = xi;
  }
  __syncthreads();
  const int c = blockIdx.x * 256 + tid;
  if (c >= c0) return;
  double v = y[c];
  for (int k = 0; k < nb; ++k) v = fma(-Sg[(size_t)(c0 + k) * ld + c], xs[k], v);
  y[c] = v;
}

__global__ __launch_bounds__(256) void gba_pose_trial_kernel(GbaArgs a) {
  if (a.S->done || a.S->fail) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.K) return;
  const double* cur = gba_cur(a) + 6 * (size_t)k;
  double* tr = gba_trial(a) + 6 * (size_t)k;
  double d2 = 0.0, p2 = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double d = a.dp[6 * (size_t)k + r];
    tr[r] = cur[r] + d;                                                     // :1046
    d2 += d * d; p2 += cur[r] * cur[r];
  }
  a.kf_dsq[k] = d2; a.kf_psq[k] = p2;
  gba_pose_to_Rt(tr, a.Rt_trial + 12 * (size_t)k);
}

// delta_l = V*^-1 (-g_l - sum W^T delta_p) = -(V*^-1 g_l + M^T sum Z^T delta_p); the trial point and its residuals (:1047-1048)
__global__ __launch_bounds__(256) void gba_backsub_kernel(GbaArgs a, BaCam cam) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (a.S->done || a.S->fail || j >= a.M) return;
  const int t0 = a.pt_start[j], t1 = a.pt_start[j + 1];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int t = t0; t < t1; ++t) {
    const int k = a.o_kf[t];
    if (k < 0) continue;
    const double* Zt = a.Z + 18 * (size_t)t;
    const double* d = a.dp + 6 * (size_t)k;
#pragma unroll
    for (int r = 0; r < 6; ++r) { s0 = fma(Zt[3 * r], d[r], s0); s1 = fma(Zt[3 * r + 1], d[r], s1); s2 = fma(Zt[3 * r + 2], d[r], s2); }
  }
  const double* Mz = a.Mz + 6 * (size_t)j;
  const double* vg = a.vg + 3 * (size_t)j;
  const double dl[3] = {-(vg[0] + (Mz[0] * s0 + Mz[1] * s1 + Mz[3] * s2)), -(vg[1] + (Mz[2] * s1 + Mz[4] * s2)), -(vg[2] + Mz[5] * s2)};
  const double* Xp = gba_cur(a) + 6 * (size_t)a.K + 3 * (size_t)j;
  double* Xt = gba_trial(a) + 6 * (size_t)a.K + 3 * (size_t)j;
  const double X[3] = {Xp[0] + dl[0], Xp[1] + dl[1], Xp[2] + dl[2]};
  Xt[0] = X[0]; Xt[1] = X[1]; Xt[2] = X[2];
  a.pt_dsq[j] = dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2];
  a.pt_psq[j] = Xp[0] * Xp[0] + Xp[1] * Xp[1] + Xp[2] * Xp[2];
  double chi = 0.0;
  for (int t = t0; t < t1; ++t) {
    GbaObs o;
    gba_obs_terms(cam, gba_obs_Rt(a, a.Rt_trial, a.o_kf[t]), X, a.o_uv[2 * (size_t)t], a.o_uv[2 * (size_t)t + 1], false, o);
    chi += o.chi;
  }
  a.pt_tchi[j] = chi;
}

// sum of v over the workgroup's 1024 threads in a fixed tree
__device__ __forceinline__ double gba_block_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int s = 512; s >= 1; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}
// initial_only: the call enqueued no iteration; the current error is the initial error
__global__ __launch_bounds__(1024) void gba_decide_kernel(GbaArgs a, int initial_only, const volatile int* __restrict__ abort_flag) {
  __shared__ double sh[1024];
  GbaState* S = a.S;
  if (S->done) return;
  const int tid = threadIdx.x;
  const bool fail = S->fail != 0;
  double c = 0.0, g = 0.0, tc = 0.0, d = 0.0, p = 0.0;
  for (int j = tid; j < a.M; j += 1024) {
    c += a.pt_chi2[j]; g += a.pt_glsq[j];
    if (!initial_only && !fail) { tc += a.pt_tchi[j]; d += a.pt_dsq[j]; p += a.pt_psq[j]; }
  }
  if (!initial_only)
    for (int k = tid; k < a.K; k += 1024) {
      g += a.kf_gsq[k];
      if (!fail) { d += a.kf_dsq[k]; p += a.kf_psq[k]; }
    }
  const double cur_sq = gba_block_sum(c, sh), gsq = gba_block_sum(g, sh), trial_sq = gba_block_sum(tc, sh), dsq = gba_block_sum(d, sh), psq = gba_block_sum(p, sh);
  if (tid != 0) return;
  if (initial_only || S->iters == 1) S->init_sq = cur_sq;                     // the initial error (:1000-1001) is the first iteration's current error
  S->cur_sq = cur_sq;
  S->final_sq = cur_sq;
  if (initial_only) return;
  if (sqrt(gsq) < S->gtol) { S->done = 1; return; }                           // :1027-1029
  if (fail) { S->done = 1; return; }                                          // :1036-1039
  const double dnorm = sqrt(dsq), pnorm = sqrt(psq);
  if (dnorm < S->ptol * (pnorm + S->ptol)) { S->done = 1; return; }           // :1041-1044
  if (trial_sq < cur_sq) {                                                    // :1050-1055
    S->sel ^= 1;
    S->final_sq = trial_sq;
    S->lambda = fmax(S->lambda * 0.1, 1e-10);
  } else {
    S->lambda = fmin(S->lambda * 10.0, 1e10);
  }
  if (abort_flag && *abort_flag) S->done = 1;                                 // should_stop at the top of the next iteration (:1013)
}

// out: [0] iterations [1] final_sq [2] initial chi2 [3] bad-index code [8...] the current parameters
__global__ __launch_bounds__(256) void gba_finish_kernel(GbaArgs a, double* __restrict__ out) {
  const GbaState* S = a.S;
  const size_t np = 6 * (size_t)a.K + 3 * (size_t)a.M;
  const double* cur = gba_cur(a);
  if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = (double)S->iters; out[1] = S->final_sq; out[2] = S->init_sq; out[3] = (double)S->bad; }
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < np; i += (size_t)gridDim.x * 256) out[8 + i] = cur[i];
}

// ---- host helpers (ba_kernels.hip keeps its own in its anonymous namespace) --------------------------------------------------------
void gba_quat_rotate(const double* q, const double* v, double* o) {
  const double t[3] = {2.0 * (q[2] * v[2] - q[3] * v[1]), 2.0 * (q[3] * v[0] - q[1] * v[2]), 2.0 * (q[1] * v[1] - q[2] * v[0])};
  const double c[3] = {q[2] * t[2] - q[3] * t[1], q[3] * t[0] - q[1] * t[2], q[1] * t[1] - q[2] * t[0]};
  for (int i = 0; i < 3; ++i) o[i] = t[i] * q[0] + c[i] + v[i];
}
void gba_quat_to_R(const double* q, double* R) {
  const double w = q[0], i = q[1], j = q[2], k = q[3];
  const double ww = w * w, ii = i * i, jj = j * j, kk = k * k;
  const double ij = i * j * 2.0, wk = w * k * 2.0, wj = w * j * 2.0, ik = i * k * 2.0, jk = j * k * 2.0, wi = w * i * 2.0;
  R[0] = ww + ii - jj - kk; R[1] = ij - wk; R[2] = wj + ik;
  R[3] = wk + ij; R[4] = ww - ii + jj - kk; R[5] = jk - wi;
  R[6] = ik - wj; R[7] = wi + jk; R[8] = ww - ii - jj + kk;
}
// local_ba_lm.rs:642-645 + nalgebra scaled_axis()
void gba_se3_to_params(const double* pose7, double* p6) {
  const double w = pose7[0];
  double v[3] = {pose7[1], pose7[2], pose7[3]};
  if (!(w >= 0.0)) { v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
  const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (n > 0.0) {
    const double ang = std::atan2(n, std::fabs(w)) * 2.0;
    for (int i = 0; i < 3; ++i) p6[i] = v[i] / n * ang;
  } else p6[0] = p6[1] = p6[2] = 0.0;
  p6[3] = pose7[4]; p6[4] = pose7[5]; p6[5] = pose7[6];
}
// local_ba_lm.rs:648-662 then SE3::inverse (se3.rs:56-63) -> T_wc
void gba_params_to_pose_wc(const double* p6, double* out7) {
  double q[4];
  const double angle = std::sqrt(p6[0] * p6[0] + p6[1] * p6[1] + p6[2] * p6[2]);
  if (angle > 1e-10) {
    double a[3] = {p6[0] / angle, p6[1] / angle, p6[2] / angle};
    const double n = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double s = std::sin(angle / 2.0), c = std::cos(angle / 2.0);
    q[0] = c; q[1] = a[0] / n * s; q[2] = a[1] / n * s; q[3] = a[2] / n * s;
  } else { q[0] = 1; q[1] = q[2] = q[3] = 0; }
  const double qi[4] = {q[0], -q[1], -q[2], -q[3]};
  double rt[3];
  gba_quat_rotate(qi, p6 + 3, rt);
  out7[0] = qi[0]; out7[1] = qi[1]; out7[2] = qi[2]; out7[3] = qi[3];
  out7[4] = -rt[0]; out7[5] = -rt[1]; out7[6] = -rt[2];
}

}  // namespace

int gba_max_keyframes() { return GBA_MAX_K; }

// The whole-map solve.  The caller (orbx_api.hip) has checked the pointers, K >= 1, M >= 1, N >= 1 and that no collective is installed.
// obs (32-byte) or obs32 (16-byte) is given; on_device: obs32 is device memory, ordered on the handle's stream.
int gba_solve(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_ba_config* cfg, int K, const double* poses_cw,
              const double* fixed_pose_cw, int M, double* points, int N, const orbx_ba_obs* obs, const orbx_ba_obs32* obs32, bool on_device,
              orbx_should_stop_fn should_stop, void* user, double* poses_wc_out, int* iterations, double* initial_error, double* final_error) {
  if (K > GBA_MAX_K)
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: at most %d optimised keyframes per call (K = %d)", who, GBA_MAX_K, K);
  if ((size_t)N > (size_t)0x7fffffff / 18) return orbx_fail(h, ORBX_ERR_INVALID, "%s: at most %d observations per call", who, 0x7fffffff / 18);
  hipStream_t st = h->stream;
  const int n = 6 * K, ld = (n + GBA_NB - 1) / GBA_NB * GBA_NB;
  const size_t np = 6 * (size_t)K + 3 * (size_t)M, k1 = (size_t)K, m1 = (size_t)M, n1 = (size_t)N;
  const size_t obs_bytes = on_device ? 0 : (obs32 ? sizeof(orbx_ba_obs32) : sizeof(orbx_ba_obs)) * n1;
  // the input blob: state | R|t of the anchor and the identity | parameters | the observations as they were handed over
  Carve ci;
  const size_t i_state = ci.take(sizeof(GbaState)), i_fix = ci.take(8 * 24), i_p0 = ci.take(8 * np), i_obs = ci.take(obs_bytes);
  const size_t out_bytes = 8 * (8 + np);
  // the arena: what the launches make
  Carve ca;
  const size_t a_cnt = ca.take(4 * (m1 + 2 * k1 + 1));                      // pt_cnt [M] | kf_cnt [K] | kf_fill [K]: zeroed per call
  const size_t a_pt_start = ca.take(4 * (m1 + 1)), a_kf_start = ca.take(4 * (k1 + 1));
  const size_t a_obs_tmp = ca.take(4 * n1), a_kf_tmp = ca.take(4 * n1), a_o_kf = ca.take(4 * n1), a_o_pt = ca.take(4 * n1), a_kf_obs = ca.take(4 * n1), a_kf_pt = ca.take(4 * n1);
  const size_t a_o_uv = ca.take(16 * n1), a_oP = ca.take(48 * n1), a_Z = ca.take(144 * n1);
  const size_t a_p1 = ca.take(8 * np), a_Rt = ca.take(2 * 96 * k1);
  const size_t a_pt = ca.take(8 * 17 * m1);                                 // Mz 6 | vg 3 | mg 3 | chi2 | glsq | dsq | psq | tchi
  const size_t a_kf = ca.take(8 * 3 * k1), a_dp = ca.take(8 * (size_t)ld), a_Ld = ca.take(8 * (size_t)ld * GBA_NB);
  const size_t sys_bytes = 8 * ((size_t)n + 1) * (size_t)ld;

  HostCall call{};
  if (int rc = orbx_host_call_begin(h, h->pin_gba, h->ws_gba.blobs, ci.off, out_bytes, call)) return rc;
  if (int rc = orbx_reserve(h, h->ws_gba.arena, ca.off)) return rc;
  if (int rc = orbx_reserve(h, h->ws_gba.system, sys_bytes)) return rc;
  if (!h->h_abort) {
    ORBX_HIP(h, hipHostMalloc((void**)&h->h_abort, 64));
    ORBX_HIP(h, hipHostGetDevicePointer((void**)&h->d_abort, h->h_abort, 0));
  }
  *h->h_abort = 0;

  GbaState s0{};
  s0.lambda = 1e-3; s0.gtol = cfg->gradient_tolerance; s0.ptol = cfg->param_tolerance;     // :1006-1010
  std::memcpy(call.hi + i_state, &s0, sizeof(s0));
  double* fix = (double*)(call.hi + i_fix);
  const double ident[7] = {1, 0, 0, 0, 0, 0, 0};
  for (int f = 0; f < 2; ++f) {
    const double* p = f == 0 ? fixed_pose_cw : ident;
    gba_quat_to_R(p, fix + 12 * f);
    fix[12 * f + 9] = p[4]; fix[12 * f + 10] = p[5]; fix[12 * f + 11] = p[6];
  }
  double* p0 = (double*)(call.hi + i_p0);
  for (int k = 0; k < K; ++k) gba_se3_to_params(poses_cw + 7 * (size_t)k, p0 + 6 * (size_t)k);
  std::memcpy(p0 + 6 * k1, points, 8 * 3 * m1);
  if (obs_bytes) std::memcpy(call.hi + i_obs, obs32 ? (const void*)obs32 : (const void*)obs, obs_bytes);
  if (int rc = orbx_host_call_upload(h, call)) return rc;

  uint8_t* ar = (uint8_t*)h->ws_gba.arena.p;
  ORBX_HIP(h, hipMemsetAsync(ar + a_cnt, 0, 4 * (m1 + 2 * k1 + 1), st));
  GbaArgs a{};
  a.K = K; a.M = M; a.N = N; a.n = n; a.ld = ld; a.obs32 = obs32 ? 1 : 0;
  a.S = (GbaState*)(call.di + i_state); a.P0 = (double*)(call.di + i_p0); a.P1 = (double*)(ar + a_p1);
  a.Rt_fix = (const double*)(call.di + i_fix);
  a.obs_raw = on_device ? (const void*)obs32 : (const void*)(call.di + i_obs);
  a.pt_cnt = (int*)(ar + a_cnt); a.kf_cnt = a.pt_cnt + m1; a.kf_fill = a.kf_cnt + k1;
  a.pt_start = (int*)(ar + a_pt_start); a.kf_start = (int*)(ar + a_kf_start);
  a.obs_tmp = (int*)(ar + a_obs_tmp); a.kf_tmp = (int*)(ar + a_kf_tmp); a.o_kf = (int*)(ar + a_o_kf); a.o_pt = (int*)(ar + a_o_pt);
  a.kf_obs = (int*)(ar + a_kf_obs); a.kf_pt = (int*)(ar + a_kf_pt);
  a.o_uv = (double*)(ar + a_o_uv); a.oP = (double*)(ar + a_oP); a.Z = (double*)(ar + a_Z);
  a.Rt_cur = (double*)(ar + a_Rt); a.Rt_trial = a.Rt_cur + 12 * k1;
  double* pt = (double*)(ar + a_pt);
  a.Mz = pt; a.vg = pt + 6 * m1; a.mg = pt + 9 * m1; a.pt_chi2 = pt + 12 * m1; a.pt_glsq = pt + 13 * m1; a.pt_dsq = pt + 14 * m1; a.pt_psq = pt + 15 * m1; a.pt_tchi = pt + 16 * m1;
  double* kf = (double*)(ar + a_kf);
  a.kf_gsq = kf; a.kf_dsq = kf + k1; a.kf_psq = kf + 2 * k1;
  a.dp = (double*)(ar + a_dp); a.Ld = (double*)(ar + a_Ld); a.Sg = (double*)h->ws_gba.system.p;
  const BaCam bc{cam->fx, cam->fy, cam->cx, cam->cy, cfg->huber_threshold, 1, 0, 0.0, nullptr};

  const dim3 b256(256), gN((N + 255) / 256), gM((M + 255) / 256), gK((K + 255) / 256);
  orbx_launch(h, "gba_ingest_kernel", false, gba_ingest_kernel, gN, b256, 0, a);
  orbx_launch(h, "gba_scan_kernel", false, gba_scan_kernel, dim3(1), dim3(1024), 0, a);
  orbx_launch(h, "gba_place_kernel", false, gba_place_kernel, gN, b256, 0, a);
  orbx_launch(h, "gba_order_kernel", false, gba_order_kernel, gM, b256, 0, a);
  orbx_launch(h, "gba_kfplace_kernel", false, gba_kfplace_kernel, gN, b256, 0, a);
  orbx_launch(h, "gba_kforder_kernel", false, gba_kforder_kernel, dim3(K), b256, 0, a);

  const int panels = (n + GBA_NB - 1) / GBA_NB;
  bool any_iteration = false, stopped = false;
  for (int iter = 0; iter < cfg->max_iterations; ++iter) {                   // :1012
    if (should_stop && should_stop(user)) { stopped = true; break; }        // :1013
    any_iteration = true;
    orbx_launch(h, "gba_pose_kernel", false, gba_pose_kernel, gK, b256, 0, a, iter);
    orbx_launch(h, "gba_build_kernel", false, gba_build_kernel, gM, b256, 0, a, bc);
    orbx_launch(h, "gba_kf_schur_kernel", false, gba_kf_schur_kernel, dim3(K), dim3(GBA_KF_THREADS), 0, a, bc);
    for (int p = 0; p < panels; ++p) {
      const int c0 = p * GBA_NB;
      const int below = std::max(0, n - (c0 + GBA_NB)) + 1;                 // the rows below the panel and the right-hand side
      orbx_launch(h, "gba_panel_kernel", false, gba_panel_kernel, dim3((below + GBA_PANEL_ROWS - 1) / GBA_PANEL_ROWS), dim3(64), 0, a, c0);
      const int nbt = (n + 1 - (c0 + GBA_NB) + GBA_NB - 1) / GBA_NB;        // 64-row blocks of the trailing rows [c0 + 64, n]
      if (c0 + GBA_NB < n) orbx_launch(h, "gba_syrk_kernel", false, gba_syrk_kernel, dim3(nbt * (nbt + 1) / 2), b256, 0, a, c0);
    }
    for (int p = panels - 1; p >= 0; --p) {
      const int c0 = p * GBA_NB;
      orbx_launch(h, "gba_back_kernel", false, gba_back_kernel, dim3(std::max(1, (c0 + 255) / 256)), b256, 0, a, c0);
    }
    orbx_launch(h, "gba_pose_trial_kernel", false, gba_pose_trial_kernel, gK, b256, 0, a);
    orbx_launch(h, "gba_backsub_kernel", false, gba_backsub_kernel, gM, b256, 0, a, bc);
    orbx_launch(h, "gba_decide_kernel", false, gba_decide_kernel, dim3(1), dim3(1024), 0, a, 0, (const volatile int*)h->d_abort);
  }
  if (!any_iteration) {
    orbx_launch(h, "gba_pose_kernel", false, gba_pose_kernel, gK, b256, 0, a, -1);
    orbx_launch(h, "gba_build_kernel", false, gba_build_kernel, gM, b256, 0, a, bc);
    orbx_launch(h, "gba_decide_kernel", false, gba_decide_kernel, dim3(1), dim3(1024), 0, a, 1, (const volatile int*)nullptr);
  }
  orbx_launch(h, "gba_finish_kernel", false, gba_finish_kernel, dim3((unsigned)std::min<size_t>(256, (np + 255) / 256)), b256, 0, a, (double*)call.dout);
  ORBX_HIP(h, hipMemcpyAsync(call.ho, call.dout, out_bytes, hipMemcpyDeviceToHost, st));
  // while the enqueued iterations drain, keep asking should_stop: a stop requested now ends the solve at the next iteration boundary
  if (should_stop && !stopped) {
    while (hipStreamQuery(st) == hipErrorNotReady)
      if (should_stop(user)) { *(volatile int*)h->h_abort = 1; break; }
  }
  ORBX_HIP(h, hipStreamSynchronize(st));
  ORBX_HIP(h, hipGetLastError());

  const double* o = (const double*)call.ho;
  if (o[3] != 0.0) {
    const int i = 0x7fffffff - (int)o[3];
    if (on_device) return orbx_fail(h, ORBX_ERR_INVALID, "%s: observation %d (device memory): index out of range (K %d, M %d)", who, i, K, M);
    int kfi, fxi, mpi;
    if (obs32) { kfi = obs32[i].kf_idx >= 0 ? obs32[i].kf_idx : -1; fxi = obs32[i].kf_idx >= 0 ? -1 : -1 - obs32[i].kf_idx; mpi = obs32[i].mp_idx; }
    else { kfi = obs[i].kf_idx; fxi = obs[i].fixed_idx; mpi = obs[i].mp_idx; }
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: observation %d: index out of range (kf %d/%d, fixed %d/1, mp %d/%d)", who, i, kfi, K, fxi, mpi, M);
  }
  const int iters = (int)o[0];
  const double nres = 2.0 * (double)N;
  *iterations = iters;
  *initial_error = std::sqrt(o[2]) / std::sqrt(nres);                         // :1000-1001
  *final_error = std::sqrt(iters > 0 ? o[1] : o[2]) / std::sqrt(nres);        // :1059-1060
  const double* params = o + 8;
  for (int k = 0; k < K; ++k) gba_params_to_pose_wc(params + 6 * (size_t)k, poses_wc_out + 7 * (size_t)k);
  std::memcpy(points, params + 6 * k1, 8 * 3 * m1);
  return ORBX_OK;
}
