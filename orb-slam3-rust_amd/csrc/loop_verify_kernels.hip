// loop_verify_kernels.hip — verify_loop_candidate (src/loop_closing/corrector.rs:116-204) for a batch of (current keyframe, loop
// keyframe) pairs, and compute_sim3_ransac (src/loop_closing/sim3_solver.rs:63-145) on its own, with no host synchronisation
// inside.  The specification is stated in include/orbx.h and DESIGN.md §2; tests/loop_verify_spec.py restates it in numpy.
//
//   lv_match_kernel       grid (tiles of LV_TILE current rows) x pairs, brute-force pairs.  A block keeps its tile of current
//                         descriptors in LDS and streams the loop keyframe's descriptors once.  Per row a lane keeps a packed best
//                         key (distance << 22 | loop feature) and a second distance; two partial results (k_a, s_a), (k_b, s_b)
//                         merge by best = min(k_a, k_b), second = min(max(d_a, d_b), s_a, s_b) — exactly the sequential rule of
//                         :285-296, the repeated best distance that becomes the second included, in any merge order
//                         FeatureVector pairs run the same kernel with every distance between features of different nodes masked
//                         out (node ids in LDS / one per lane): :252-263 is the same walk over fewer candidates.  A per-node walk
//                         needs the loop keyframe's features sorted by node, which cost more on the host than the masked pass
//                         costs on the device
//   lv_resolve_kernel     one workgroup per pair: the stereo-point guard, the ratio test, the matches in ascending current index
//                         (BlockAppend, block_dev.hpp), those with two stereo points into the pair list with their world points
//   sim3_hypothesis_kernel  one lane per (problem, hypothesis): sampler, Horn with a one-sided Jacobi SVD in registers, M | t
//   sim3_score_kernel     workgroups over (tiles of a problem's points) x (chunks of its hypotheses, staged in LDS), ballot + popcount
//                         per wave, one integer add per hypothesis and workgroup
//   sim3_final_kernel     one workgroup per problem: arg-max, mask, refit over the winner's inliers with fixed-order block sums,
//                         recount, mse, the Sim3 and the record
//   lv_finish_kernel      one workgroup per pair: the reprojection count over all gathered matches, status, the record
// The only atomics are integer adds: every output is a deterministic function of the pair's inputs alone.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "block_dev.hpp"
#include "guided_search_dev.hpp"
#include "orbx_internal.hpp"
#include "pose_dev.hpp"
#include "ransac_dev.hpp"

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_TILE = 16;               // current rows per block, as tref_nn_kernel's measured choice
constexpr int LV_IDX_BITS = 22;           // a best key is distance << 22 | loop feature: distances need 9 bits
constexpr int LV_MAX_FEAT = 1 << LV_IDX_BITS;
constexpr unsigned LV_IDX_MASK = (unsigned)LV_MAX_FEAT - 1u;
constexpr unsigned LV_NONE = 1023u;       // the distance field of "no candidate yet" (a real distance is <= 256): u32::MAX of :281-282
constexpr int S3_MAX_H = 1024;            // hypotheses per problem (max_iterations)
constexpr int S3_HS = 12;                 // doubles per hypothesis: M = scale * R (9, row-major) | t (3)
constexpr int S3_CHUNK = 32;              // hypotheses per scoring workgroup, staged in LDS (3 KB)
constexpr int S3_THREADS = 256;
constexpr int LV_PRE = 8;                 // ints per pair left by lv_resolve_kernel: status, n_matches, n_pairs, start, n for Sim3

// one pair as the kernels see it
struct LvItem {
  const uint8_t* c_desc; const double* c_pts; const uint8_t* c_has;
  const orbx_keypoint* l_kp; const uint8_t* l_desc; const double* l_pts; const uint8_t* l_has;
  const uint32_t* c_node; const uint32_t* l_node;   // FeatureVector form: one node id per feature; else both NULL
  double pose_c[7], pose_l[7];
  int n1, n2, out_off, pad_;
};

struct LvArgs {
  orbx_camera cam;
  orbx_loop_verify_config cfg;
  double pow_scale[32];    // scale_factor^octave from the host's pow
  const LvItem* items;
  uint2* best;             // [N1] (best key, second distance) per current feature
  int* pre;                // [B][LV_PRE]
  orbx_dmatch* matches; int* fm; double* pts_c; double* pts_l; uint8_t* inl; double* sim3;
  const double* model;     // [B][12] the returned M | t
  const orbx_sim3_result* sres;
  orbx_loop_verify_result* results;
};

// ---- stage 1: the matchers -------------------------------------------------------------------------------------

template <bool FV>
__global__ __launch_bounds__(LV_THREADS) void lv_match_kernel(LvArgs A) {
  __shared__ unsigned long long sq[LV_TILE][4];
  __shared__ unsigned snode[LV_TILE];
  __shared__ unsigned redk[LV_THREADS / 64][LV_TILE], reds[LV_THREADS / 64][LV_TILE];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LvItem* it = A.items + b;
  const int n1 = it->n1, n2 = it->n2, q0 = blockIdx.x * LV_TILE;
  if ((it->c_node != nullptr) != FV || q0 >= n1) return;                    // (uniform over the workgroup)
  const int rows = min(LV_TILE, n1 - q0);
  const uint8_t* cd = it->c_desc;
  // rows past the keyframe's end repeat its last row; their results are not written
  for (int k = tid; k < LV_TILE * 4; k += LV_THREADS) {
    const int r = k >> 2, c = k & 3;
    sq[r][c] = reinterpret_cast<const unsigned long long*>(cd + (size_t)(q0 + min(r, rows - 1)) * 32)[c];
  }
  if (FV && tid < LV_TILE) snode[tid] = it->c_node[q0 + min(tid, rows - 1)];
  __syncthreads();
  const uint8_t* ld = it->l_desc;
  unsigned rk[LV_TILE], rs[LV_TILE];
#pragma unroll
  for (int r = 0; r < LV_TILE; ++r) { rk[r] = 0xffffffffu; rs[r] = LV_NONE; }
  for (int j = tid; j < n2; j += LV_THREADS) {
    // the tile is read from LDS again for every loop feature: hoisted out of this loop it would take 8 registers per row
    asm volatile("" ::: "memory");
    const Desc256 tr = load_desc(ld + (size_t)j * 32);
    const unsigned nj = FV ? it->l_node[j] : 0u;
#pragma unroll
    for (int r = 0; r < LV_TILE; ++r) {
      unsigned d = (unsigned)(__popcll(tr.w[0] ^ sq[r][0]) + __popcll(tr.w[1] ^ sq[r][1]) + __popcll(tr.w[2] ^ sq[r][2]) +
                              __popcll(tr.w[3] ^ sq[r][3]));
      // another node, or a feature in no list: not a candidate (a masked distance never becomes a best or a second)
      if (FV) d = (nj == snode[r] && nj != 0xffffffffu) ? d : LV_NONE;
      rs[r] = min(rs[r], max(rk[r] >> LV_IDX_BITS, d));
      rk[r] = min(rk[r], (d << LV_IDX_BITS) | (unsigned)j);
    }
  }
#pragma unroll
  for (int r = 0; r < LV_TILE; ++r) {
    unsigned key = rk[r], sec = rs[r];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned ok = (unsigned)__shfl_xor((int)key, off), os = (unsigned)__shfl_xor((int)sec, off);
      sec = min(min(sec, os), max(key >> LV_IDX_BITS, ok >> LV_IDX_BITS));
      key = min(key, ok);
    }
    if (lane == 0) { redk[wave][r] = key; reds[wave][r] = sec; }
  }
  __syncthreads();
  if (tid < rows) {
    unsigned key = redk[0][tid], sec = reds[0][tid];
#pragma unroll
    for (int w = 1; w < LV_THREADS / 64; ++w) {
      const unsigned ok = redk[w][tid], os = reds[w][tid];
      sec = min(min(sec, os), max(key >> LV_IDX_BITS, ok >> LV_IDX_BITS));
      key = min(key, ok);
    }
    A.best[(size_t)it->out_off + q0 + tid] = make_uint2(key, sec);
  }
}

// ---- stages 0 and 2 --------------------------------------------------------------------------------------------

// (the two-flag append and the block sums are written out here: on BlockAppend / block_sum (block_dev.hpp) this kernel measured
// 0.5 us, 3 %, slower than this text — profiles/block_primitives_ab.txt)
__global__ __launch_bounds__(LV_THREADS) void lv_resolve_kernel(LvArgs A) {
  __shared__ int wave_m[LV_THREADS / 64], wave_c[LV_THREADS / 64];
  __shared__ int run_m, run_c;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LvItem* it = A.items + b;
  const int n1 = it->n1, n2 = it->n2;
  const size_t k0 = (size_t)it->out_off;
  int* pre = A.pre + (size_t)b * LV_PRE;
  // stage 0: the stereo points of both keyframes (:127-134)
  int c1 = 0, c2 = 0;
  for (int i = tid; i < n1; i += LV_THREADS) c1 += it->c_has[i] != 0;
  for (int i = tid; i < n2; i += LV_THREADS) c2 += it->l_has[i] != 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) { c1 += __shfl_xor(c1, off); c2 += __shfl_xor(c2, off); }
  if (lane == 0) { wave_m[wave] = c1; wave_c[wave] = c2; }
  if (tid == 0) { run_m = 0; run_c = 0; }
  __syncthreads();
  c1 = wave_m[0] + wave_m[1] + wave_m[2] + wave_m[3];
  c2 = wave_c[0] + wave_c[1] + wave_c[2] + wave_c[3];
  __syncthreads();
  if (c1 < A.cfg.min_stereo_points || c2 < A.cfg.min_stereo_points) {       // (uniform over the workgroup)
    if (tid == 0) { pre[0] = ORBX_LOOP_TOO_FEW_POINTS; pre[1] = 0; pre[2] = 0; pre[3] = it->out_off; pre[4] = 0; }
    return;
  }
  for (int base = 0; base < n1; base += LV_THREADS) {
    const int i = base + tid;
    bool fm = false, fc = false;
    int j = 0;
    unsigned d = 0;
    if (i < n1) {
      const uint2 ks = A.best[k0 + i];
      j = (int)(ks.x & LV_IDX_MASK); d = ks.x >> LV_IDX_BITS;
      const double second = ks.y >= LV_NONE ? 4294967295.0 : (double)ks.y;
      fm = d < A.cfg.match_max_dist && (double)d < A.cfg.match_ratio * second;     // :298
      fc = fm && it->c_has[i] != 0 && it->l_has[j] != 0;                       // :151-158
    }
    const unsigned long long mm = __ballot(fm), mc = __ballot(fc);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) { wave_m[wave] = __popcll(mm); wave_c[wave] = __popcll(mc); }
    __syncthreads();
    int om = run_m, oc = run_c;
    for (int w = 0; w < wave; ++w) { om += wave_m[w]; oc += wave_c[w]; }
    if (fm) {
      orbx_dmatch dm;
      dm.query_idx = i; dm.train_idx = j; dm.img_idx = 0; dm.distance = (float)d;
      A.matches[k0 + om + __popcll(mm & below)] = dm;
    }
    if (fc) {
      const size_t o = k0 + oc + __popcll(mc & below);
      A.fm[2 * o] = i; A.fm[2 * o + 1] = j;
      double w3[3];
      se3_transform_point(it->pose_c, it->c_pts + 3 * (size_t)i, w3);                     // :161
      A.pts_c[3 * o] = w3[0]; A.pts_c[3 * o + 1] = w3[1]; A.pts_c[3 * o + 2] = w3[2];
      se3_transform_point(it->pose_l, it->l_pts + 3 * (size_t)j, w3);                     // :162
      A.pts_l[3 * o] = w3[0]; A.pts_l[3 * o + 1] = w3[1]; A.pts_l[3 * o + 2] = w3[2];
    }
    __syncthreads();
    if (tid == 0) {
      run_m += wave_m[0] + wave_m[1] + wave_m[2] + wave_m[3];
      run_c += wave_c[0] + wave_c[1] + wave_c[2] + wave_c[3];
    }
    __syncthreads();
  }
  if (tid == 0) {
    int status = ORBX_LOOP_OK;
    if (run_m < A.cfg.min_matches) status = ORBX_LOOP_TOO_FEW_MATCHES;        // :139
    else if (run_c < A.cfg.min_pairs) status = ORBX_LOOP_TOO_FEW_PAIRS;       // :178
    pre[0] = status; pre[1] = run_m; pre[2] = status == ORBX_LOOP_TOO_FEW_MATCHES ? 0 : run_c; pre[3] = it->out_off;
    pre[4] = status == ORBX_LOOP_OK ? run_c : 0;
  }
}

// ---- stage 3: Sim3-RANSAC --------------------------------------------------------------------------------------

struct S3Args {
  orbx_sim3_config cfg;
  int max_n, stride;                       // start / count are read at [p * stride]
  const int* start; const int* count;      // count == NULL: start is an offsets array [P+1]
  const double* pts1; const double* pts2;
  double* hyp; int* hcnt; int* hok;        // [P][H][12], [P][H], [P][H]
  double* model;                           // [P][12] the returned M | t
  double* sim3; uint8_t* inl; orbx_sim3_result* results;
};

__device__ __forceinline__ void s3_problem(const S3Args& S, int p, int& base, int& n) {
  base = S.start[(size_t)p * S.stride];
  n = S.count ? S.count[(size_t)p * S.stride] : S.start[p + 1] - base;
}
__device__ __forceinline__ bool s3_runs(const S3Args& S, int n) {            // sim3_solver.rs:69-75
  return n >= 3 && n >= S.cfg.min_inliers && n <= S.max_n;
}

#define S3_ROT(p, q)                                                                                       \
  {                                                                                                        \
    const double al = A[p][0] * A[p][0] + A[p][1] * A[p][1] + A[p][2] * A[p][2];                           \
    const double be = A[q][0] * A[q][0] + A[q][1] * A[q][1] + A[q][2] * A[q][2];                           \
    const double ga = A[p][0] * A[q][0] + A[p][1] * A[q][1] + A[p][2] * A[q][2];                           \
    if (ga != 0.0 && fabs(ga) > 1e-16 * (sqrt(al) * sqrt(be))) {                                           \
      const double ze = (be - al) / (2.0 * ga);                                                            \
      const double t = copysign(1.0, ze) / (fabs(ze) + sqrt(1.0 + ze * ze));                               \
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;                                                 \
      _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                                      \
        const double x = A[p][r], y = A[q][r];                                                             \
        A[p][r] = c * x - s * y; A[q][r] = s * x + c * y;                                                  \
        const double vx = V[p][r], vy = V[q][r];                                                           \
        V[p][r] = c * vx - s * vy; V[q][r] = s * vx + c * vy;                                              \
      }                                                                                                    \
      rot = true;                                                                                          \
    }                                                                                                      \
  }
#define S3_SWAP(p, q)                                                                                      \
  {                                                                                                        \
    _Pragma("unroll") for (int r = 0; r < 3; ++r) {                                                        \
      double x = A[p][r]; A[p][r] = A[q][r]; A[q][r] = x;                                                  \
      x = V[p][r]; V[p][r] = V[q][r]; V[q][r] = x;                                                         \
    }                                                                                                      \
    const double x = nn[p]; nn[p] = nn[q]; nn[q] = x;                                                      \
  }

// The rotation of Horn's method from H = sum a b^T (row-major): R = V diag(1, 1, det(V U^T)) U^T of H = U S V^T (sim3_solver.rs:
// 196-212).  That R is the one proper rotation with R u1 = v1 and R u2 = v2, so R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T needs
// only the two leading singular pairs.  One-sided Jacobi on H's columns (H V = U S; V stays orthonormal whatever H's rank); u2 is
// re-orthogonalised against u1 and, where H has rank 1, replaced by any unit vector orthogonal to u1; H = 0 gives the identity.
__device__ void s3_rotation(const double* H, double* R) {
  double A[3][3], V[3][3], nn[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { A[c][r] = H[3 * r + c]; V[c][r] = r == c ? 1.0 : 0.0; }
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rot = false;
    S3_ROT(0, 1) S3_ROT(0, 2) S3_ROT(1, 2)
    if (!rot) break;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) nn[c] = A[c][0] * A[c][0] + A[c][1] * A[c][1] + A[c][2] * A[c][2];
  if (nn[0] < nn[1]) S3_SWAP(0, 1)
  if (nn[1] < nn[2]) S3_SWAP(1, 2)
  if (nn[0] < nn[1]) S3_SWAP(0, 1)
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
  if (!(nn[0] > 0.0) || !(nn[0] < INFINITY)) return;
  const double s1 = sqrt(nn[0]);
  const double u1[3] = {A[0][0] / s1, A[0][1] / s1, A[0][2] / s1};
  double u2[3];
  {
    const double d = u1[0] * A[1][0] + u1[1] * A[1][1] + u1[2] * A[1][2];
    u2[0] = A[1][0] - d * u1[0]; u2[1] = A[1][1] - d * u1[1]; u2[2] = A[1][2] - d * u1[2];
    double wn = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
    if (!(wn > 1e-28 * nn[0])) {                                            // rank 1: any direction orthogonal to u1
      const double a0 = fabs(u1[0]), a1 = fabs(u1[1]), a2 = fabs(u1[2]);
      const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
      const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
      const double f = k == 0 ? u1[0] : (k == 1 ? u1[1] : u1[2]);
      u2[0] = e[0] - f * u1[0]; u2[1] = e[1] - f * u1[1]; u2[2] = e[2] - f * u1[2];
      wn = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
    }
    const double w = sqrt(wn);
    u2[0] /= w; u2[1] /= w; u2[2] /= w;
  }
  const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  const double v3[3] = {V[0][1] * V[1][2] - V[0][2] * V[1][1], V[0][2] * V[1][0] - V[0][0] * V[1][2], V[0][0] * V[1][1] - V[0][1] * V[1][0]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = V[0][r] * u1[c] + V[1][r] * u2[c] + v3[r] * u3[c];
  }
}

// Horn's steps after the sums (:176-226): scale, M = scale * R, t = c2 - M c1.  False where the scale is undefined (:183).
__device__ __forceinline__ bool s3_model(const double* H, double sa, double sb, const double* c1, const double* c2, bool fix_scale,
                                         double* R, double& scale, double* Mt) {
  scale = 1.0;
  if (!fix_scale) {
    if (sa < 1e-10) return false;
    scale = sqrt(sb / sa);
  }
  s3_rotation(H, R);
#pragma unroll
  for (int k = 0; k < 9; ++k) Mt[k] = scale * R[k];
#pragma unroll
  for (int r = 0; r < 3; ++r) Mt[9 + r] = c2[r] - (Mt[3 * r] * c1[0] + Mt[3 * r + 1] * c1[1] + Mt[3 * r + 2] * c1[2]);
  return true;
}

// |M p1 + t - p2|^2, one IEEE operation at a time, left to right (tests/loop_verify_spec.py writes the same expression)
__device__ __forceinline__ double s3_err2(const double* Mt, const double* p1, const double* p2) {
  const double x = Mt[0] * p1[0] + Mt[1] * p1[1] + Mt[2] * p1[2] + Mt[9] - p2[0];
  const double y = Mt[3] * p1[0] + Mt[4] * p1[1] + Mt[5] * p1[2] + Mt[10] - p2[1];
  const double z = Mt[6] * p1[0] + Mt[7] * p1[1] + Mt[8] * p1[2] + Mt[11] - p2[2];
  return x * x + y * y + z * z;
}

// grid (P, ceil(H / 64)), 64 lanes: lane = hypothesis
__global__ __launch_bounds__(64) void sim3_hypothesis_kernel(S3Args S) {
  const int p = blockIdx.x, h = blockIdx.y * 64 + threadIdx.x, H = S.cfg.max_iterations;
  if (h >= H) return;
  int base, n;
  s3_problem(S, p, base, n);
  const size_t slot = (size_t)p * H + h;
  int idx[3] = {0, 0, 0};
  bool valid = s3_runs(S, n) && ransac_sample<3>(S.cfg.seed, h, n, 3, idx);
  double Mt[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Mt[k] = 0.0;
  if (valid) {
    double a[3][3], bb[3][3], c1[3], c2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t g = (size_t)base + (k == 0 ? idx[0] : (k == 1 ? idx[1] : idx[2]));
#pragma unroll
      for (int r = 0; r < 3; ++r) { a[k][r] = S.pts1[3 * g + r]; bb[k][r] = S.pts2[3 * g + r]; }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) { c1[r] = (a[0][r] + a[1][r] + a[2][r]) / 3.0; c2[r] = (bb[0][r] + bb[1][r] + bb[2][r]) / 3.0; }
    double Hm[9], sa = 0.0, sb = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) Hm[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int r = 0; r < 3; ++r) { a[k][r] = a[k][r] - c1[r]; bb[k][r] = bb[k][r] - c2[r]; }
      sa += a[k][0] * a[k][0] + a[k][1] * a[k][1] + a[k][2] * a[k][2];
      sb += bb[k][0] * bb[k][0] + bb[k][1] * bb[k][1] + bb[k][2] * bb[k][2];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Hm[3 * r + c] += a[k][r] * bb[k][c];
      }
    }
    double R[9], scale;
    valid = s3_model(Hm, sa, sb, c1, c2, S.cfg.fix_scale != 0, R, scale, Mt);
  }
  double* o = S.hyp + slot * S3_HS;
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = Mt[k];
  S.hcnt[slot] = 0;
  S.hok[slot] = valid ? 1 : 0;
}

// grid (P, tiles of 256 points, chunks of S3_CHUNK hypotheses): a single problem of a thousand points still spreads over the chip
__global__ __launch_bounds__(S3_THREADS) void sim3_score_kernel(S3Args S, double thr2) {
  __shared__ double sM[S3_CHUNK * S3_HS];
  __shared__ int sOk[S3_CHUNK];
  __shared__ int sCnt[S3_THREADS / 64][S3_CHUNK];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, H = S.cfg.max_iterations;
  int base, n;
  s3_problem(S, p, base, n);
  const int i = blockIdx.y * S3_THREADS + tid, c0 = blockIdx.z * S3_CHUNK;
  if (!s3_runs(S, n) || blockIdx.y * S3_THREADS >= n || c0 >= H) return;   // (uniform over the workgroup)
  const bool have = i < n;
  const size_t g = (size_t)base + (have ? i : 0);
  const double p1[3] = {S.pts1[3 * g], S.pts1[3 * g + 1], S.pts1[3 * g + 2]};
  const double p2[3] = {S.pts2[3 * g], S.pts2[3 * g + 1], S.pts2[3 * g + 2]};
  const double* hp = S.hyp + ((size_t)p * H + c0) * S3_HS;
  const int nc = min(S3_CHUNK, H - c0);
  for (int e = tid; e < nc * S3_HS; e += S3_THREADS) sM[e] = hp[e];
  for (int e = tid; e < nc; e += S3_THREADS) sOk[e] = S.hok[(size_t)p * H + c0 + e];
  __syncthreads();
  for (int hh = 0; hh < nc; ++hh) {
    if (!sOk[hh]) continue;
    const bool in = have && s3_err2(sM + S3_HS * hh, p1, p2) < thr2;         // :253
    const int c = __popcll(__ballot(in));
    if (lane == 0) sCnt[wave][hh] = c;
  }
  __syncthreads();
  for (int hh = tid; hh < nc; hh += S3_THREADS) {
    if (!sOk[hh]) continue;
    int s = 0;
#pragma unroll
    for (int w = 0; w < S3_THREADS / 64; ++w) s += sCnt[w][hh];
    if (s) atomicAdd(S.hcnt + (size_t)p * H + c0 + hh, s);
  }
}

// UnitQuaternion::from_rotation_matrix's branches, normalised, [spec] w >= 0
__device__ __forceinline__ void s3_quat(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
    q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
    q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
    q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
  }
  const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sg = q[0] < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = sg * q[k] / nq;
}

// grid P, 256 threads
__global__ __launch_bounds__(S3_THREADS) void sim3_final_kernel(S3Args S, double thr2) {
  __shared__ double s_w[(S3_THREADS / 64) * 11];
  __shared__ unsigned long long s_key[S3_THREADS / 64];
  __shared__ double s_M[12], s_M2[12], s_R[9], s_scale;
  __shared__ int s_go;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, H = S.cfg.max_iterations;
  int base, n;
  s3_problem(S, p, base, n);
  const bool runs = s3_runs(S, n);
  // the winner: most inliers, lowest h on ties (:100)
  unsigned long long key = 0;
  if (runs) {
    for (int h = tid; h < H; h += S3_THREADS) {
      const size_t slot = (size_t)p * H + h;
      if (S.hok[slot]) key = max(key, ((unsigned long long)(unsigned)S.hcnt[slot] << 10) | (unsigned long long)(S3_MAX_H - 1 - h));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, o));
  if (lane == 0) s_key[wave] = key;
  __syncthreads();
  key = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
  const int best_cnt = (int)(key >> 10), best_h = best_cnt > 0 ? S3_MAX_H - 1 - (int)(key & 1023ull) : -1;
  int status = ORBX_SIM3_NO_MODEL, n_inl = 0, refined = 0;
  double mse = 0.0;
  if (best_h >= 0) {                                                        // (uniform over the workgroup)
    if (tid < 12) s_M[tid] = S.hyp[((size_t)p * H + best_h) * S3_HS + tid];
    if (tid == 0) s_go = 0;
    __syncthreads();
    // the winner's inliers and their squared error (:98; the scoring kernel's expression)
    double acc[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += S3_THREADS) {
      const size_t g = (size_t)base + i;
      const double e = s3_err2(s_M, S.pts1 + 3 * g, S.pts2 + 3 * g);
      const bool in = e < thr2;
      S.inl[g] = in ? 1 : 0;
      if (in) { acc[0] += 1.0; acc[1] += e; }
    }
    block_sum<S3_THREADS, 2>(acc, s_w);
    n_inl = (int)acc[0];
    double err_sum = acc[1];
    if (n_inl >= S.cfg.min_inliers) {                                       // :120: Horn over the inliers
      double cs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += S3_THREADS) {
        const size_t g = (size_t)base + i;
        if (S.inl[g]) {
#pragma unroll
          for (int r = 0; r < 3; ++r) { cs[r] += S.pts1[3 * g + r]; cs[3 + r] += S.pts2[3 * g + r]; }
        }
      }
      block_sum<S3_THREADS, 6>(cs, s_w);
#pragma unroll
      for (int r = 0; r < 6; ++r) cs[r] = cs[r] / (double)n_inl;
      double hs[11];
#pragma unroll
      for (int k = 0; k < 11; ++k) hs[k] = 0.0;
      for (int i = tid; i < n; i += S3_THREADS) {
        const size_t g = (size_t)base + i;
        if (S.inl[g]) {
          double a[3], bb[3];
#pragma unroll
          for (int r = 0; r < 3; ++r) { a[r] = S.pts1[3 * g + r] - cs[r]; bb[r] = S.pts2[3 * g + r] - cs[3 + r]; }
#pragma unroll
          for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) hs[3 * r + c] += a[r] * bb[c];
          }
          hs[9] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
          hs[10] += bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2];
        }
      }
      block_sum<S3_THREADS, 11>(hs, s_w);
      if (tid == 0) {
        double R[9], scale, Mt[12];
        if (s3_model(hs, hs[9], hs[10], cs, cs + 3, S.cfg.fix_scale != 0, R, scale, Mt)) {
#pragma unroll
          for (int k = 0; k < 12; ++k) s_M2[k] = Mt[k];
#pragma unroll
          for (int k = 0; k < 9; ++k) s_R[k] = R[k];
          s_scale = scale;
          s_go = 1;
        }
      }
      __syncthreads();
      if (s_go) {
        double acc2[2] = {0.0, 0.0};
        for (int i = tid; i < n; i += S3_THREADS) {
          const size_t g = (size_t)base + i;
          const double e = s3_err2(s_M2, S.pts1 + 3 * g, S.pts2 + 3 * g);
          if (e < thr2) { acc2[0] += 1.0; acc2[1] += e; }
        }
        block_sum<S3_THREADS, 2>(acc2, s_w);
        if ((int)acc2[0] >= n_inl) {                                        // :133
          refined = 1; n_inl = (int)acc2[0]; err_sum = acc2[1];
          for (int i = tid; i < n; i += S3_THREADS) {
            const size_t g = (size_t)base + i;
            S.inl[g] = s3_err2(s_M2, S.pts1 + 3 * g, S.pts2 + 3 * g) < thr2 ? 1 : 0;
          }
        }
      }
    }
    if (n_inl >= S.cfg.min_inliers) { status = ORBX_SIM3_OK; mse = err_sum / (double)n_inl; }   // :144, :262
  }
  __syncthreads();
  if (status != ORBX_SIM3_OK && n <= S.max_n) {
    for (int i = tid; i < n; i += S3_THREADS) S.inl[(size_t)base + i] = 0;
  }
  if (tid == 0) {
    double* so = S.sim3 + 8 * (size_t)p;
    double* mo = S.model + 12 * (size_t)p;
    if (status == ORBX_SIM3_OK) {
      const double* Mt = refined ? s_M2 : s_M;
      double R[9], scale = 1.0, q[4];
      if (refined) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = s_R[k];
        scale = s_scale;
      } else {
        // a hypothesis slot holds M = scale * R: the scale is a row's length, 1 exactly when it is fixed
        if (!S.cfg.fix_scale) scale = sqrt(Mt[0] * Mt[0] + Mt[1] * Mt[1] + Mt[2] * Mt[2]);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = S.cfg.fix_scale ? Mt[k] : Mt[k] / scale;
      }
      s3_quat(R, q);
      so[0] = q[0]; so[1] = q[1]; so[2] = q[2]; so[3] = q[3]; so[4] = Mt[9]; so[5] = Mt[10]; so[6] = Mt[11]; so[7] = scale;
#pragma unroll
      for (int k = 0; k < 12; ++k) mo[k] = Mt[k];
    } else {
      so[0] = 1.0; so[1] = 0.0; so[2] = 0.0; so[3] = 0.0; so[4] = 0.0; so[5] = 0.0; so[6] = 0.0; so[7] = 1.0;
#pragma unroll
      for (int k = 0; k < 12; ++k) mo[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    }
    orbx_sim3_result r;
    r.status = status; r.best_hypothesis = best_h; r.ransac_inliers = best_cnt; r.n_inliers = n_inl; r.refined = refined; r.reserved_ = 0;
    r.mse = mse;
    S.results[p] = r;
  }
}

// ---- stage 4 and the record ------------------------------------------------------------------------------------

__global__ __launch_bounds__(LV_THREADS) void lv_finish_kernel(LvArgs A) {
  __shared__ int wave_c[LV_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const LvItem* it = A.items + b;
  const int* pre = A.pre + (size_t)b * LV_PRE;
  const size_t k0 = (size_t)it->out_off;
  const orbx_sim3_result sr = A.sres[b];
  int status = pre[0];
  const int n_pairs = pre[2];
  if (status == ORBX_LOOP_OK) {
    if (sr.status != ORBX_SIM3_OK) status = ORBX_LOOP_NO_MODEL;
    else if (sr.n_inliers < A.cfg.min_inliers) status = ORBX_LOOP_TOO_FEW_INLIERS;   // corrector.rs:185
  }
  int verified = 0;
  if (status == ORBX_LOOP_OK) {                                             // (uniform over the workgroup)
    const double* Mt = A.model + 12 * (size_t)b;
    double cw[7];
    se3_inverse7(it->pose_l, cw, cw + 4);                                   // loop_kf.pose.inverse()
    int c = 0;
    for (int k = tid; k < n_pairs; k += LV_THREADS) {                       // :340-375, over all gathered matches
      const double* x = A.pts_c + 3 * (k0 + k);
      const double y[3] = {Mt[0] * x[0] + Mt[1] * x[1] + Mt[2] * x[2] + Mt[9], Mt[3] * x[0] + Mt[4] * x[1] + Mt[5] * x[2] + Mt[10],
                           Mt[6] * x[0] + Mt[7] * x[1] + Mt[8] * x[2] + Mt[11]};
      double pc[3];
      se3_transform_point(cw, y, pc);
      if (pc[2] <= 0.0) continue;
      const double u = A.cam.fx * pc[0] / pc[2] + A.cam.cx, v = A.cam.fy * pc[1] / pc[2] + A.cam.cy;
      const orbx_keypoint kp = it->l_kp[A.fm[2 * (k0 + k) + 1]];
      const double du = u - (double)kp.x, dv = v - (double)kp.y;
      const double s = A.pow_scale[min(max(kp.octave, 0), 31)];
      if (du * du + dv * dv < A.cfg.chi2 * s * s) ++c;                       // :368-371
    }
    verified = block_sum<LV_THREADS>(c, wave_c);
    if (verified < A.cfg.min_verified) status = ORBX_LOOP_TOO_FEW_VERIFIED;  // :193
  } else if (status <= ORBX_LOOP_TOO_FEW_PAIRS) {
    for (int k = tid; k < n_pairs; k += LV_THREADS) A.inl[k0 + k] = 0;
  }
  if (tid == 0) {
    orbx_loop_verify_result r;
    const bool ran = status >= ORBX_LOOP_NO_MODEL || status == ORBX_LOOP_OK;
    const bool model = ran && status != ORBX_LOOP_NO_MODEL;
    r.status = status; r.n_matches = pre[1]; r.n_pairs = n_pairs;
    r.best_hypothesis = ran ? sr.best_hypothesis : 0; r.ransac_inliers = ran ? sr.ransac_inliers : 0; r.n_inliers = ran ? sr.n_inliers : 0;
    r.refined = ran ? sr.refined : 0; r.n_verified = verified; r.mse = model ? sr.mse : 0.0;
    A.results[b] = r;
  }
}

int s3_check_config(orbx_handle* h, const orbx_sim3_config* c, const char* who) {
  if (!c || c->max_iterations < 1 || c->max_iterations > S3_MAX_H || !(c->inlier_threshold > 0.0) || c->min_inliers < 3 ||
      !(c->probability >= 0.0 && c->probability <= 1.0))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: configuration out of range (include/orbx.h: orbx_sim3_config)", who);
  return ORBX_OK;
}

int lv_check_config(orbx_handle* h, const orbx_loop_verify_config* c, const char* who) {
  if (!c || c->min_stereo_points < 0 || c->min_matches < 0 || c->min_pairs < 0 || c->min_inliers < 0 || c->min_verified < 0 ||
      c->match_max_dist > 256 || !(c->match_ratio > 0.0) || !(c->chi2 > 0.0) || !(c->scale_factor > 0.0))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: configuration out of range (include/orbx.h: orbx_loop_verify_config)", who);
  return s3_check_config(h, &c->sim3, who);
}

// The workspace of s3_launch for P problems of H hypotheses: hyp [P * H][S3_HS] | hcnt [P * H], hok [P * H] | model [P][12].
struct S3Ws {
  size_t hyp, hcnt, model, bytes;
};
S3Ws s3_ws(int P, int H) {
  const size_t slots = (size_t)P * H;
  Carve c;
  S3Ws w;
  w.hyp = c.take(slots * S3_HS * sizeof(double)); w.hcnt = c.take(slots * 2 * sizeof(int)); w.model = c.take((size_t)P * 12 * sizeof(double));
  w.bytes = c.off;
  return w;
}

// The three launches on the handle's stream; ws has s3_ws(P, H).bytes bytes; every pointer is device memory.
int s3_launch(orbx_handle* h, S3Args S, int P, uint8_t* ws) {
  const int H = S.cfg.max_iterations;
  const S3Ws lay = s3_ws(P, H);
  S.hyp = (double*)(ws + lay.hyp);
  S.hcnt = (int*)(ws + lay.hcnt);
  S.hok = S.hcnt + (size_t)P * H;
  S.model = (double*)(ws + lay.model);
  const double thr2 = S.cfg.inlier_threshold * S.cfg.inlier_threshold;      // :245
  orbx_launch(h, "sim3_hypothesis_kernel", false, sim3_hypothesis_kernel, dim3(P, (H + 63) / 64), dim3(64), 0, S);
  if (S.max_n >= 3)
    orbx_launch(h, "sim3_score_kernel", true, sim3_score_kernel, dim3(P, (S.max_n + S3_THREADS - 1) / S3_THREADS, (H + S3_CHUNK - 1) / S3_CHUNK), dim3(S3_THREADS), 0, S, thr2);
  orbx_launch(h, "sim3_final_kernel", true, sim3_final_kernel, dim3(P), dim3(S3_THREADS), 0, S, thr2);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

}  // namespace

int loop_verify_enqueue(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int B,
                        const LoopVerifyPair* pairs, orbx_dmatch* d_matches, int* d_feature_matches, double* d_pts_current,
                        double* d_pts_loop, uint8_t* d_inlier, double* d_sim3, orbx_loop_verify_result* d_results) {
  if (int rc = lv_check_config(h, cfg, who)) return rc;
  if (!cam || !pairs || B < 1) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  int max_n1 = 0;
  size_t N1 = 0, fv_n1 = 0, fv_n2 = 0;
  bool any_bf = false, any_fv = false;
  for (int b = 0; b < B; ++b) {
    const LoopVerifyPair& p = pairs[b];
    if (p.n1 < 0 || p.n2 < 0 || p.n1 > LV_MAX_FEAT || p.n2 > LV_MAX_FEAT || p.out_off < 0 ||
        (p.n1 > 0 && (!p.c_desc || !p.c_pts || !p.c_has)) || (p.n2 > 0 && (!p.l_kp || !p.l_desc || !p.l_pts || !p.l_has)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument at pair %d (at most %d features per keyframe)", who, b, LV_MAX_FEAT);
    max_n1 = std::max(max_n1, p.n1);
    N1 = std::max(N1, (size_t)p.out_off + (size_t)p.n1);
    if (p.c_node && p.l_node) { any_fv = true; fv_n1 += (size_t)p.n1; fv_n2 += (size_t)p.n2; } else any_bf = true;
  }
  if (!d_sim3 || !d_results || (N1 > 0 && (!d_matches || !d_feature_matches || !d_pts_current || !d_pts_loop || !d_inlier)))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  ORBX_HIP(h, hipSetDevice(h->device));
  // the item table and the FeatureVector tables go up through the upload ring, so that the caller's arrays are free when the call
  // returns
  Carve up;
  const size_t o_it = up.take(sizeof(LvItem) * (size_t)B), o_node = up.take(4 * (fv_n1 + fv_n2));
  uint8_t *hs, *ds;
  if (int rc = orbx_ring_begin(h, h->ring_lv, h->ws_lv[2], up.off, &hs, &ds)) return rc;
  size_t n_at = 0;
  for (int b = 0; b < B; ++b) {
    const LoopVerifyPair& p = pairs[b];
    LvItem it{};
    it.c_desc = p.c_desc; it.c_pts = p.c_pts; it.c_has = p.c_has;
    it.l_kp = p.l_kp; it.l_desc = p.l_desc; it.l_pts = p.l_pts; it.l_has = p.l_has;
    std::memcpy(it.pose_c, p.pose_c, sizeof(it.pose_c)); std::memcpy(it.pose_l, p.pose_l, sizeof(it.pose_l));
    it.n1 = p.n1; it.n2 = p.n2; it.out_off = p.out_off;
    if (p.c_node && p.l_node) {                                             // the node ids travel with the items
      uint32_t* hn = (uint32_t*)(hs + o_node) + n_at;
      if (p.n1) std::memcpy(hn, p.c_node, 4 * (size_t)p.n1);
      if (p.n2) std::memcpy(hn + p.n1, p.l_node, 4 * (size_t)p.n2);
      it.c_node = (const uint32_t*)(ds + o_node) + n_at;
      it.l_node = it.c_node + p.n1;
      n_at += (size_t)p.n1 + (size_t)p.n2;
    }
    ((LvItem*)(hs + o_it))[b] = it;
  }
  if (int rc = orbx_ring_commit(h, h->ring_lv, h->ws_lv[2], up.off)) return rc;
  const S3Ws s3 = s3_ws(B, cfg->sim3.max_iterations);
  Carve ws;
  const size_t o_best = ws.take(8 * N1), o_pre = ws.take(4 * LV_PRE * (size_t)B), o_sres = ws.take(sizeof(orbx_sim3_result) * (size_t)B),
               o_s3 = ws.take(s3.bytes);
  if (int rc = orbx_reserve(h, h->ws_lv[0], ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_lv[0].p;
  LvArgs A{};
  A.cam = *cam; A.cfg = *cfg;
  for (int o = 0; o < 32; ++o) A.pow_scale[o] = std::pow(cfg->scale_factor, (double)o);
  A.items = (const LvItem*)(ds + o_it);
  A.best = (uint2*)(w + o_best); A.pre = (int*)(w + o_pre);
  A.matches = d_matches; A.fm = d_feature_matches; A.pts_c = d_pts_current; A.pts_l = d_pts_loop; A.inl = d_inlier; A.sim3 = d_sim3;
  A.sres = (const orbx_sim3_result*)(w + o_sres); A.results = d_results;
  S3Args S{};
  S.cfg = cfg->sim3; S.max_n = max_n1; S.stride = LV_PRE; S.start = A.pre + 3; S.count = A.pre + 4;
  S.pts1 = d_pts_current; S.pts2 = d_pts_loop; S.sim3 = d_sim3; S.inl = d_inlier; S.results = (orbx_sim3_result*)(w + o_sres);
  A.model = (const double*)(w + o_s3 + s3.model);
  const dim3 match_grid((max_n1 + LV_TILE - 1) / LV_TILE, B);
  if (any_bf && max_n1 > 0) orbx_launch(h, "lv_match_kernel", false, lv_match_kernel<false>, match_grid, dim3(LV_THREADS), 0, A);
  if (any_fv && max_n1 > 0) orbx_launch(h, "lv_match_kernel_fv", any_bf, lv_match_kernel<true>, match_grid, dim3(LV_THREADS), 0, A);
  orbx_launch(h, "lv_resolve_kernel", max_n1 > 0, lv_resolve_kernel, dim3(B), dim3(LV_THREADS), 0, A);
  ORBX_HIP(h, hipGetLastError());
  if (int rc = s3_launch(h, S, B, w + o_s3)) return rc;
  orbx_launch(h, "lv_finish_kernel", true, lv_finish_kernel, dim3(B), dim3(LV_THREADS), 0, A);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

extern "C" {

void orbx_default_sim3_config(orbx_sim3_config* c) {
  if (!c) return;
  c->max_iterations = 300;        // sim3_solver.rs:29
  c->inlier_threshold = 0.075;    // :30
  c->min_inliers = 15;            // :31
  c->fix_scale = 1;               // :32
  c->probability = 0.99;          // :33
  c->seed = 0;
}

void orbx_default_loop_verify_config(orbx_loop_verify_config* c) {
  if (!c) return;
  c->min_stereo_points = 20;      // corrector.rs:132
  c->min_matches = 15;            // :139
  c->min_pairs = 15;              // :178
  c->min_inliers = 15;            // :185
  c->min_verified = 50;           // :193
  c->match_max_dist = 50;         // :266
  c->match_ratio = 0.7;
  c->chi2 = 5.991;                // :338
  c->scale_factor = 1.2;          // :368
  orbx_default_sim3_config(&c->sim3);
}

int orbx_sim3_ransac_batch_device(orbx_handle* h, const orbx_sim3_config* cfg, int n_problems, int max_n, const int* d_offsets,
                                  const double* d_pts1, const double* d_pts2, double* d_sim3, uint8_t* d_inlier,
                                  orbx_sim3_result* d_results) {
  static const char* who = "orbx_sim3_ransac_batch_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = s3_check_config(h, cfg, who)) return rc;
    if (n_problems < 0 || max_n < 0 || (n_problems > 0 && (!d_offsets || !d_sim3 || !d_results)) || (max_n > 0 && (!d_pts1 || !d_pts2 || !d_inlier)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (n_problems == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    if (int rc = orbx_reserve(h, h->ws_lv[0], s3_ws(n_problems, cfg->max_iterations).bytes)) return rc;
    S3Args S{};
    S.cfg = *cfg; S.max_n = max_n; S.stride = 1; S.start = d_offsets; S.count = nullptr;
    S.pts1 = d_pts1; S.pts2 = d_pts2; S.sim3 = d_sim3; S.inl = d_inlier; S.results = d_results;
    return s3_launch(h, S, n_problems, (uint8_t*)h->ws_lv[0].p);
  });
}

int orbx_sim3_ransac_batch(orbx_handle* h, const orbx_sim3_config* cfg, int n_problems, const int* offsets, const double* pts1,
                           const double* pts2, double* sim3, uint8_t* inlier, orbx_sim3_result* results) {
  static const char* who = "orbx_sim3_ransac_batch";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = s3_check_config(h, cfg, who)) return rc;
    if (n_problems < 0 || (n_problems > 0 && (!offsets || !sim3 || !results))) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (n_problems == 0) return ORBX_OK;
    int max_n = 0;
    if (int rc = orbx_check_offsets(h, who, "offsets", "problem", n_problems, offsets, &max_n)) return rc;
    const size_t N = (size_t)offsets[n_problems], P = (size_t)n_problems;
    if (N > 0 && (!pts1 || !pts2 || !inlier)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    // one blob each way: [offsets | pts1 | pts2] up, [sim3 | results | inliers] down
    Carve in, out;
    const size_t i_of = in.take(4 * (P + 1)), i_p1 = in.take(24 * N), i_p2 = in.take(24 * N);
    const size_t o_s3 = out.take(64 * P), o_rs = out.take(sizeof(orbx_sim3_result) * P), o_in = out.take(N);
    HostCall c;
    if (int rc = orbx_host_call_begin(h, h->pin_lv, h->ws_lv[3], in.off, out.off, c)) return rc;
    uint8_t *hi = c.hi, *ho = c.ho, *di = c.di, *dout = c.dout;
    std::memcpy(hi + i_of, offsets, 4 * (P + 1));
    if (N) { std::memcpy(hi + i_p1, pts1, 24 * N); std::memcpy(hi + i_p2, pts2, 24 * N); }
    if (int rc = orbx_host_call_upload(h, c)) return rc;
    if (int rc = orbx_sim3_ransac_batch_device(h, cfg, n_problems, max_n, (const int*)(di + i_of), (const double*)(di + i_p1),
                                               (const double*)(di + i_p2), (double*)(dout + o_s3), dout + o_in, (orbx_sim3_result*)(dout + o_rs)))
      return rc;
    if (int rc = orbx_host_call_download(h, c, out.off)) return rc;
    std::memcpy(sim3, ho + o_s3, 64 * P);
    std::memcpy(results, ho + o_rs, sizeof(orbx_sim3_result) * P);
    if (N) std::memcpy(inlier, ho + o_in, N);
    return ORBX_OK;
  });
}

int orbx_verify_loop_candidates_device(orbx_handle* h, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int n_pairs,
                                       const uint8_t* d_cur_desc, const double* d_cur_points_cam, const uint8_t* d_cur_has_point,
                                       const uint32_t* cur_node, const int* cur_offsets, const double* cur_poses_wc,
                                       const orbx_keypoint* d_loop_kp, const uint8_t* d_loop_desc, const double* d_loop_points_cam,
                                       const uint8_t* d_loop_has_point, const uint32_t* loop_node, const int* loop_offsets,
                                       const double* loop_poses_wc, orbx_dmatch* d_matches, int* d_feature_matches,
                                       double* d_pts_current, double* d_pts_loop, uint8_t* d_inlier, double* d_sim3,
                                       orbx_loop_verify_result* d_results) {
  static const char* who = "orbx_verify_loop_candidates_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = lv_check_config(h, cfg, who)) return rc;
    if (!cam || n_pairs < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (n_pairs == 0) return ORBX_OK;
    if (int rc = orbx_check_offsets(h, who, "cur_offsets", "pair", n_pairs, cur_offsets, nullptr, LV_MAX_FEAT)) return rc;
    if (int rc = orbx_check_offsets(h, who, "loop_offsets", "pair", n_pairs, loop_offsets, nullptr, LV_MAX_FEAT)) return rc;
    if (!cur_poses_wc || !loop_poses_wc) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    std::vector<LoopVerifyPair> pairs((size_t)n_pairs);
    for (int b = 0; b < n_pairs; ++b) {
      LoopVerifyPair& p = pairs[(size_t)b];
      const size_t c0 = (size_t)cur_offsets[b], l0 = (size_t)loop_offsets[b];
      p.c_desc = d_cur_desc ? d_cur_desc + 32 * c0 : nullptr; p.c_pts = d_cur_points_cam ? d_cur_points_cam + 3 * c0 : nullptr;
      p.c_has = d_cur_has_point ? d_cur_has_point + c0 : nullptr; p.c_node = cur_node ? cur_node + c0 : nullptr;
      p.n1 = cur_offsets[b + 1] - cur_offsets[b];
      p.l_kp = d_loop_kp ? d_loop_kp + l0 : nullptr; p.l_desc = d_loop_desc ? d_loop_desc + 32 * l0 : nullptr;
      p.l_pts = d_loop_points_cam ? d_loop_points_cam + 3 * l0 : nullptr; p.l_has = d_loop_has_point ? d_loop_has_point + l0 : nullptr;
      p.l_node = loop_node ? loop_node + l0 : nullptr;
      p.n2 = loop_offsets[b + 1] - loop_offsets[b];
      std::memcpy(p.pose_c, cur_poses_wc + 7 * (size_t)b, 56); std::memcpy(p.pose_l, loop_poses_wc + 7 * (size_t)b, 56);
      p.out_off = cur_offsets[b];
    }
    return loop_verify_enqueue(h, who, cam, cfg, n_pairs, pairs.data(), d_matches, d_feature_matches, d_pts_current, d_pts_loop, d_inlier,
                               d_sim3, d_results);
  });
}

int orbx_verify_loop_candidates(orbx_handle* h, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int n_pairs,
                                const uint8_t* cur_desc, const double* cur_points_cam, const uint8_t* cur_has_point,
                                const uint32_t* cur_node, const int* cur_offsets, const double* cur_poses_wc, const orbx_keypoint* loop_kp,
                                const uint8_t* loop_desc, const double* loop_points_cam, const uint8_t* loop_has_point,
                                const uint32_t* loop_node, const int* loop_offsets, const double* loop_poses_wc, orbx_dmatch* matches,
                                int* feature_matches, double* pts_current, double* pts_loop, uint8_t* inlier, double* sim3,
                                orbx_loop_verify_result* results) {
  static const char* who = "orbx_verify_loop_candidates";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = lv_check_config(h, cfg, who)) return rc;
    if (!cam || n_pairs < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (n_pairs == 0) return ORBX_OK;
    if (int rc = orbx_check_offsets(h, who, "cur_offsets", "pair", n_pairs, cur_offsets, nullptr, LV_MAX_FEAT)) return rc;
    if (int rc = orbx_check_offsets(h, who, "loop_offsets", "pair", n_pairs, loop_offsets, nullptr, LV_MAX_FEAT)) return rc;
    const size_t B = (size_t)n_pairs, N1 = (size_t)cur_offsets[B], N2 = (size_t)loop_offsets[B];
    if (!cur_poses_wc || !loop_poses_wc || !sim3 || !results || (N1 > 0 && (!cur_desc || !cur_points_cam || !cur_has_point || !matches ||
        !feature_matches || !pts_current || !pts_loop || !inlier)) || (N2 > 0 && (!loop_kp || !loop_desc || !loop_points_cam || !loop_has_point)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    // one blob each way: [cur desc | cur points | cur has | loop kp | loop desc | loop points | loop has] up,
    // [sim3 | records | matches | feature matches | pts current | pts loop | inliers] down
    Carve in, out;
    const size_t i_cd = in.take(32 * N1), i_cp = in.take(24 * N1), i_ch = in.take(N1), i_lk = in.take(sizeof(orbx_keypoint) * N2), i_ld = in.take(32 * N2),
                 i_lp = in.take(24 * N2), i_lh = in.take(N2);
    const size_t o_s3 = out.take(64 * B), o_rs = out.take(sizeof(orbx_loop_verify_result) * B), o_ma = out.take(sizeof(orbx_dmatch) * N1),
                 o_fm = out.take(8 * N1), o_pc = out.take(24 * N1), o_pl = out.take(24 * N1), o_in = out.take(N1);
    HostCall c;
    if (int rc = orbx_host_call_begin(h, h->pin_lv, h->ws_lv[1], in.off, out.off, c)) return rc;
    uint8_t *hi = c.hi, *ho = c.ho, *di = c.di, *dout = c.dout;
    if (N1) { std::memcpy(hi + i_cd, cur_desc, 32 * N1); std::memcpy(hi + i_cp, cur_points_cam, 24 * N1); std::memcpy(hi + i_ch, cur_has_point, N1); }
    if (N2) {
      std::memcpy(hi + i_lk, loop_kp, sizeof(orbx_keypoint) * N2); std::memcpy(hi + i_ld, loop_desc, 32 * N2);
      std::memcpy(hi + i_lp, loop_points_cam, 24 * N2); std::memcpy(hi + i_lh, loop_has_point, N2);
    }
    if (int rc = orbx_host_call_upload(h, c)) return rc;
    if (int rc = orbx_verify_loop_candidates_device(h, cam, cfg, n_pairs, di + i_cd, (const double*)(di + i_cp), di + i_ch, cur_node, cur_offsets,
                                                    cur_poses_wc, (const orbx_keypoint*)(di + i_lk), di + i_ld, (const double*)(di + i_lp), di + i_lh,
                                                    loop_node, loop_offsets, loop_poses_wc, (orbx_dmatch*)(dout + o_ma), (int*)(dout + o_fm),
                                                    (double*)(dout + o_pc), (double*)(dout + o_pl), dout + o_in, (double*)(dout + o_s3),
                                                    (orbx_loop_verify_result*)(dout + o_rs)))
      return rc;
    if (int rc = orbx_host_call_download(h, c, out.off)) return rc;
    std::memcpy(sim3, ho + o_s3, 64 * B);
    std::memcpy(results, ho + o_rs, sizeof(orbx_loop_verify_result) * B);
    for (size_t b = 0; b < B; ++b) {
      const size_t k0 = (size_t)cur_offsets[b], nm = (size_t)results[b].n_matches, np = (size_t)results[b].n_pairs;
      if (nm) std::memcpy(matches + k0, ho + o_ma + sizeof(orbx_dmatch) * k0, sizeof(orbx_dmatch) * nm);
      if (np) {
        std::memcpy(feature_matches + 2 * k0, ho + o_fm + 8 * k0, 8 * np);
        std::memcpy(pts_current + 3 * k0, ho + o_pc + 24 * k0, 24 * np);
        std::memcpy(pts_loop + 3 * k0, ho + o_pl + 24 * k0, 24 * np);
        std::memcpy(inlier + k0, ho + o_in + k0, np);
      }
    }
    return ORBX_OK;
  });
}

}  // extern "C"
