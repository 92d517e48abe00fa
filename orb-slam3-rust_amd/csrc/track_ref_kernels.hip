// track_ref_kernels.hip — the numeric part of track_with_reference_kf (src/tracking/tracker.rs:992-1064) for a batch of frames,
// each against its own reference keyframe (orbx_track_reference[_device], orbx_keyframe_track_reference), with no host
// synchronisation inside.
//
// Four launches around PnP's three (pnp_kernels.hip, unchanged):
//   tref_nn_kernel        grid (tiles of TREF_TILE keyframe rows) x frames.  A block keeps its tile of keyframe descriptors in LDS
//                         and streams the frame's descriptors once; every Hamming distance is computed once and feeds both minima:
//                         the row minimum (keyframe feature -> frame feature) stays in registers and is reduced inside the block, the
//                         column minimum (frame feature -> keyframe feature) is merged across blocks by atomicMin on a packed key
//                         (distance << 32 | keyframe index).  A minimum over that key is "smallest distance, then lowest index"
//                         whatever order the blocks arrive in: the result is the sequential rule's, bit for bit.
//   tref_resolve_kernel   one workgroup per frame: the mutual pairs in ascending keyframe index (BlockAppend, block_dev.hpp) into d_matches,
//                         those with a live map point into a pair list, and the two counts
//   tref_gather_kernel    one workgroup per frame: offsets[b] = the earlier frames' correspondences, then the pair list into PnP's
//                         layout (positions, keypoint positions, indices)
//   (PnP)
//   tref_finish_kernel    status, the prior's bytes where there were too few correspondences, the record
// The only atomics are those integer minima: every output is a deterministic function of the inputs.
#include <algorithm>
#include <cmath>

#include "block_dev.hpp"
#include "guided_search_dev.hpp"
#include "orbx_internal.hpp"

namespace {

constexpr int TREF_THREADS = 256;
// keyframe rows per block.  Measured at 2000 x 2000: tref_nn_kernel takes 23 / 37 / 68 / 131 us for one frame and
// 170 / 167 / 185 / 258 us for 64 frames at 16 / 32 / 64 / 128 rows — the column atomics (nt x ceil(nq / tile) per frame) do not
// bind it, the number of blocks one frame spreads over does.  (-DTREF_TILE=n builds another height for that comparison.)
#ifndef TREF_TILE
#define TREF_TILE 16
#endif
constexpr int TREF_TILE_LOG = TREF_TILE == 16 ? 4 : TREF_TILE == 32 ? 5 : TREF_TILE == 64 ? 6 : TREF_TILE == 128 ? 7 : -1;
static_assert(TREF_TILE_LOG > 0, "TREF_TILE is 16, 32, 64 or 128");
// a row minimum is one 32-bit key (distance << 22 | frame feature): distances need 9 bits, so a frame holds at most 2^22 features
constexpr int TREF_IDX_BITS = 22;
constexpr int TREF_MAX_FEAT = 1 << TREF_IDX_BITS;
constexpr unsigned TREF_IDX_MASK = (unsigned)TREF_MAX_FEAT - 1u;

struct TrefArgs {
  int min_corr, max_feat, fc_stride;
  // inputs
  const orbx_keypoint* kp; const uint8_t* desc; const int* feat_start; const int* feat_count;
  const TrackRefItem* items; const double* positions; const uint8_t* valid; const double* priors;
  // workspace: row_best [K] (distance << 22 | frame feature), col_best [B][max_feat] (distance << 32 | keyframe feature),
  // pairs [K][2] (keyframe feature, frame feature) of the correspondences, counts [B][2] (n_matches, n_correspondences)
  unsigned* row_best; unsigned long long* col_best; int* pairs; int* counts;
  // outputs
  orbx_dmatch* matches; int* offsets; double* pts3d; float* pts2d; int* kf_idx; int* feat_idx; double* poses_out;
  const orbx_pnp_result* pnp_res; orbx_track_ref_result* results;
};

// a count outside [0, max_feat] is a frame without features
__device__ __forceinline__ int tref_feat_count(const TrefArgs& A, int b) {
  const int n = A.feat_count[(size_t)b * A.fc_stride];
  return (n < 0 || n > A.max_feat) ? 0 : n;
}

__global__ __launch_bounds__(TREF_THREADS) void tref_nn_kernel(TrefArgs A) {
  __shared__ unsigned long long sq[TREF_TILE][4];
  __shared__ unsigned red[TREF_THREADS / 64][TREF_TILE];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TrackRefItem it = A.items[b];
  const int q0 = blockIdx.x * TREF_TILE;
  if (q0 >= it.n) return;                                                      // (uniform over the workgroup)
  const int rows = min(TREF_TILE, it.n - q0);
  // rows past the keyframe's end repeat its last row: an equal distance under a higher index never wins a minimum
  for (int k = tid; k < TREF_TILE * 4; k += TREF_THREADS) {
    const int r = k >> 2, c = k & 3;
    sq[r][c] = reinterpret_cast<const unsigned long long*>(it.kf_desc + (size_t)(q0 + min(r, rows - 1)) * 32)[c];
  }
  __syncthreads();
  const int nt = tref_feat_count(A, b);
  const uint8_t* desc = A.desc + (nt > 0 ? (size_t)A.feat_start[b] * 32 : 0);
  unsigned long long* col = A.col_best + (size_t)b * A.max_feat;
  unsigned rk[TREF_TILE];
#pragma unroll
  for (int r = 0; r < TREF_TILE; ++r) rk[r] = 0xffffffffu;
  for (int j = tid; j < nt; j += TREF_THREADS) {
    // the tile is read from LDS again for every frame feature: hoisted out of this loop it would take 8 registers per row
    asm volatile("" ::: "memory");
    const Desc256 tr = load_desc(desc + (size_t)j * 32);
    unsigned ck = 0xffffffffu;
#pragma unroll
    for (int r = 0; r < TREF_TILE; ++r) {
      const unsigned d = (unsigned)(__popcll(tr.w[0] ^ sq[r][0]) + __popcll(tr.w[1] ^ sq[r][1]) + __popcll(tr.w[2] ^ sq[r][2]) +
                                    __popcll(tr.w[3] ^ sq[r][3]));
      rk[r] = min(rk[r], (d << TREF_IDX_BITS) | (unsigned)j);
      ck = min(ck, (d << TREF_TILE_LOG) | (unsigned)r);
    }
    atomicMin(&col[j], ((unsigned long long)(ck >> TREF_TILE_LOG) << 32) | (unsigned)(q0 + (int)(ck & (TREF_TILE - 1))));
  }
#pragma unroll
  for (int r = 0; r < TREF_TILE; ++r) {
    unsigned key = rk[r];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, off));
    if (lane == 0) red[wave][r] = key;
  }
  __syncthreads();
  if (tid < rows) {
    unsigned key = red[0][tid];
#pragma unroll
    for (int w = 1; w < TREF_THREADS / 64; ++w) key = min(key, red[w][tid]);
    A.row_best[(size_t)it.kf_off + q0 + tid] = key;
  }
}

// (i, row_best[i]) is a match iff col_best[row_best[i]] == i; ascending i
__global__ __launch_bounds__(TREF_THREADS) void tref_resolve_kernel(TrefArgs A) {
  __shared__ int wave_tot[(TREF_THREADS / 64) * 2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const TrackRefItem it = A.items[b];
  const int nt = tref_feat_count(A, b);
  const int nq = nt > 0 ? it.n : 0;
  const size_t k0 = (size_t)it.kf_off;
  const unsigned long long* col = A.col_best + (size_t)b * A.max_feat;
  BlockAppend<TREF_THREADS, 2> app(wave_tot);                                  // [0] matches, [1] correspondences
  for (int base = 0; base < nq; base += TREF_THREADS) {
    const int i = base + tid;
    bool fl[2] = {false, false};
    bool &fm = fl[0], &fc = fl[1];
    int j = 0;
    unsigned d = 0;
    if (i < nq) {
      const unsigned key = A.row_best[k0 + i];
      j = (int)(key & TREF_IDX_MASK); d = key >> TREF_IDX_BITS;
      fm = (int)(unsigned)(col[j] & 0xffffffffull) == i;
      fc = fm && A.valid[k0 + i] != 0;
    }
    int at[2];
    app.round(fl, at);
    if (fm) {
      orbx_dmatch dm;
      dm.query_idx = i; dm.train_idx = j; dm.img_idx = 0; dm.distance = (float)d;
      A.matches[k0 + at[0]] = dm;
    }
    if (fc) {
      const size_t o = k0 + at[1];
      A.pairs[2 * o] = i; A.pairs[2 * o + 1] = j;
    }
  }
  if (tid == 0) { A.counts[2 * b] = app.total[0]; A.counts[2 * b + 1] = app.total[1]; }
}

__global__ __launch_bounds__(TREF_THREADS) void tref_gather_kernel(TrefArgs A, int B) {
  __shared__ int wave_tot[TREF_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  // offsets[b]: the correspondences of the frames before this one
  int part = 0;
  for (int j = tid; j < b; j += TREF_THREADS) part += A.counts[2 * j + 1];
  const int base = block_sum<TREF_THREADS>(part, wave_tot);
  const int n_corr = A.counts[2 * b + 1];
  if (tid == 0) {
    A.offsets[b] = base;
    if (b == B - 1) A.offsets[B] = base + n_corr;
  }
  if (n_corr == 0) return;
  const size_t k0 = (size_t)A.items[b].kf_off;
  const orbx_keypoint* kp = A.kp + (size_t)A.feat_start[b];                       // n_corr > 0: the frame has features
  for (int k = tid; k < n_corr; k += TREF_THREADS) {
    const int i = A.pairs[2 * (k0 + k)], j = A.pairs[2 * (k0 + k) + 1];
    const size_t o = (size_t)base + k, m = k0 + i;
    A.pts3d[3 * o] = A.positions[3 * m]; A.pts3d[3 * o + 1] = A.positions[3 * m + 1]; A.pts3d[3 * o + 2] = A.positions[3 * m + 2];   // :1039
    A.pts2d[2 * o] = kp[j].x; A.pts2d[2 * o + 1] = kp[j].y;                                                                        // :1041-1042
    A.kf_idx[o] = i; A.feat_idx[o] = j;
  }
}

__global__ __launch_bounds__(64) void tref_finish_kernel(TrefArgs A, int B) {
  const int b = blockIdx.x * 8 + (threadIdx.x >> 3), t = threadIdx.x & 7;
  if (b >= B) return;
  const int n_corr = A.counts[2 * b + 1];
  const orbx_pnp_result pr = A.pnp_res[b];
  int status = ORBX_TRACK_OK, n_inl = pr.n_inliers;
  if (n_corr < A.min_corr) { status = ORBX_TRACK_TOO_FEW_CORRESPONDENCES; n_inl = 0; }   // :1051
  else if (pr.status == ORBX_PNP_NO_MODEL) status = ORBX_TRACK_NO_MODEL;
  if (status == ORBX_TRACK_TOO_FEW_CORRESPONDENCES && t < 7) A.poses_out[7 * (size_t)b + t] = A.priors[7 * (size_t)b + t];
  if (t == 7) {
    orbx_track_ref_result r;
    r.status = status; r.n_matches = A.counts[2 * b]; r.n_correspondences = n_corr; r.n_inliers = n_inl;
    A.results[b] = r;
  }
}

// what can be refused before anything is enqueued
int tref_check(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_corr, int B, const char* who) {
  if (int rc = orbx_pnp_check_config(h, pnp_cfg, who)) return rc;
  if (!cam) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  if (min_corr < 4) return orbx_fail(h, ORBX_ERR_INVALID, "%s: min_correspondences must be at least 4 (tracker.rs:1051; PnP's own minimum)", who);
  if (B < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: n_frames must not be negative", who);
  return ORBX_OK;
}

// The launches on the handle's stream; every pointer of A is device memory.
int tref_launch(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int B, int max_kf, size_t K, TrefArgs A, uint8_t* d_inl,
                double* d_err, orbx_pnp_result* d_pnp) {
  const size_t mf = (size_t)A.max_feat;
  Carve ws;
  const size_t o_col = ws.take(8 * (size_t)B * mf), o_row = ws.take(4 * K), o_pairs = ws.take(8 * K), o_cnt = ws.take(8 * (size_t)B);
  if (int rc = orbx_reserve(h, h->ws_tref[0], ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_tref[0].p;
  A.col_best = (unsigned long long*)(w + o_col); A.row_best = (unsigned*)(w + o_row); A.pairs = (int*)(w + o_pairs); A.counts = (int*)(w + o_cnt);
  A.pnp_res = d_pnp;
  if (max_kf > 0 && mf > 0) {
    {
      ProfScope ps(h, "tref_col_init");
      ORBX_HIP(h, hipMemsetAsync(A.col_best, 0xff, 8 * (size_t)B * mf, h->stream));
    }
    orbx_launch(h, "tref_nn_kernel", true, tref_nn_kernel, dim3((max_kf + TREF_TILE - 1) / TREF_TILE, B), dim3(TREF_THREADS), 0, A);
  }
  orbx_launch(h, "tref_resolve_kernel", max_kf > 0 && mf > 0, tref_resolve_kernel, dim3(B), dim3(TREF_THREADS), 0, A);
  orbx_launch(h, "tref_gather_kernel", true, tref_gather_kernel, dim3(B), dim3(TREF_THREADS), 0, A, B);
  ORBX_HIP(h, hipGetLastError());
  if (int rc = orbx_pnp_ransac_batch_device(h, cam, pnp_cfg, B, max_kf, A.offsets, A.pts3d, A.pts2d, A.priors, A.poses_out, d_inl, d_err, d_pnp))
    return rc;
  orbx_launch(h, "tref_finish_kernel", true, tref_finish_kernel, dim3((B + 7) / 8), dim3(64), 0, A, B);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

}  // namespace

int track_reference_enqueue(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                            int B, const orbx_keypoint* d_kp, const uint8_t* d_desc, const int* d_feat_start, const int* d_feat_count,
                            int feat_count_stride, int max_feat, const TrackRefItem* items, const double* positions, const uint8_t* valid,
                            bool pos_on_host, const double* d_priors_wc, orbx_dmatch* d_matches, int* d_offsets, double* d_pts3d, float* d_pts2d,
                            int* d_kf_idx, int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                            orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results) {
  int max_kf = 0;
  size_t K = 0;
  for (int b = 0; b < B; ++b) { max_kf = std::max(max_kf, items[b].n); K = std::max(K, (size_t)items[b].kf_off + (size_t)items[b].n); }
  if (max_feat < 0 || max_feat > TREF_MAX_FEAT || feat_count_stride < 1 || !d_feat_start || !d_feat_count || !d_priors_wc || !d_offsets ||
      !d_poses_wc_out || !d_pnp_results || !d_results || (max_feat > 0 && (!d_kp || !d_desc)) ||
      (K > 0 && (!positions || !valid || !d_matches || !d_pts3d || !d_pts2d || !d_kf_idx || !d_feat_idx || !d_inlier_out || !d_err_out)))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (max_feat <= %d)", who, TREF_MAX_FEAT);
  ORBX_HIP(h, hipSetDevice(h->device));
  // the item table (and host-side positions / valid) go up through the upload ring, so that the caller's arrays are free when the
  // call returns
  UploadPlan up;
  const size_t o_it = up.put(items, sizeof(TrackRefItem) * (size_t)B), o_pos = up.put(positions, pos_on_host ? 24 * K : 0), o_val = up.put(valid, pos_on_host ? K : 0);
  if (int rc = up.send(h, h->ring_tref, h->ws_tref[2])) return rc;
  uint8_t* const ds = up.device;
  TrefArgs A{};
  A.min_corr = min_correspondences; A.max_feat = max_feat; A.fc_stride = feat_count_stride;
  A.kp = d_kp; A.desc = d_desc; A.feat_start = d_feat_start; A.feat_count = d_feat_count;
  A.items = (const TrackRefItem*)(ds + o_it);
  A.positions = pos_on_host ? (const double*)(ds + o_pos) : positions;
  A.valid = pos_on_host ? (const uint8_t*)(ds + o_val) : valid;
  A.priors = d_priors_wc;
  A.matches = d_matches; A.offsets = d_offsets; A.pts3d = d_pts3d; A.pts2d = d_pts2d; A.kf_idx = d_kf_idx; A.feat_idx = d_feat_idx;
  A.poses_out = d_poses_wc_out; A.results = d_results;
  return tref_launch(h, cam, pnp_cfg, B, max_kf, K, A, d_inlier_out, d_err_out, d_pnp_results);
}

extern "C" {

int orbx_track_reference_device(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                                int n_frames, const orbx_keypoint* d_kp, const uint8_t* d_desc, const int* d_feat_start,
                                const int* d_feat_count, int feat_count_stride, int max_feat, const uint8_t* d_kf_desc,
                                const double* d_kf_positions, const uint8_t* d_kf_valid, const int* kf_offsets,
                                const double* d_priors_wc, orbx_dmatch* d_matches, int* d_offsets, double* d_pts3d, float* d_pts2d,
                                int* d_kf_idx, int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                                orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results) {
  static const char* who = "orbx_track_reference_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = tref_check(h, cam, pnp_cfg, min_correspondences, n_frames, who)) return rc;
    if (n_frames == 0) return ORBX_OK;
    if (int rc = orbx_check_offsets(h, who, "kf_offsets", "frame", n_frames, kf_offsets)) return rc;
    if (kf_offsets[n_frames] > 0 && !d_kf_desc) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    std::vector<TrackRefItem> items((size_t)n_frames);
    for (int b = 0; b < n_frames; ++b) {
      items[(size_t)b].kf_desc = d_kf_desc + 32 * (size_t)kf_offsets[b];
      items[(size_t)b].kf_off = kf_offsets[b];
      items[(size_t)b].n = kf_offsets[b + 1] - kf_offsets[b];
    }
    return track_reference_enqueue(h, who, cam, pnp_cfg, min_correspondences, n_frames, d_kp, d_desc, d_feat_start, d_feat_count, feat_count_stride,
                                   max_feat, items.data(), d_kf_positions, d_kf_valid, false, d_priors_wc, d_matches, d_offsets, d_pts3d, d_pts2d,
                                   d_kf_idx, d_feat_idx, d_poses_wc_out, d_inlier_out, d_err_out, d_pnp_results, d_results);
  });
}

int orbx_track_reference(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences, int n_frames,
                         const orbx_keypoint* kp, const uint8_t* desc, const int* feat_offsets, const uint8_t* kf_desc,
                         const double* kf_positions, const uint8_t* kf_valid, const int* kf_offsets, const double* priors_wc,
                         orbx_dmatch* matches, int* offsets, double* pts3d, float* pts2d, int* kf_idx, int* feat_idx,
                         double* poses_wc_out, uint8_t* inlier_out, double* err_out, orbx_pnp_result* pnp_results,
                         orbx_track_ref_result* results) {
  static const char* who = "orbx_track_reference";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = tref_check(h, cam, pnp_cfg, min_correspondences, n_frames, who)) return rc;
    if (n_frames == 0) return ORBX_OK;
    int max_feat = 0, max_kf = 0;
    if (int rc = orbx_check_offsets(h, who, "kf_offsets", "frame", n_frames, kf_offsets, &max_kf)) return rc;
    if (int rc = orbx_check_offsets(h, who, "feat_offsets", "frame", n_frames, feat_offsets, &max_feat)) return rc;
    const size_t B = (size_t)n_frames;
    const size_t NF = (size_t)feat_offsets[B], K = (size_t)kf_offsets[B];
    if (max_feat > TREF_MAX_FEAT || !priors_wc || !offsets || !poses_wc_out || !pnp_results || !results || (NF > 0 && (!kp || !desc)) ||
        (K > 0 && (!kf_desc || !kf_positions || !kf_valid || !matches || !pts3d || !pts2d || !kf_idx || !feat_idx || !inlier_out || !err_out)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (at most %d features per frame)", who, TREF_MAX_FEAT);
    ORBX_HIP(h, hipSetDevice(h->device));
    // one blob each way: [kp | desc | keyframe desc | positions | valid | priors | feat_start | feat_count | items] up,
    // [offsets | pts3d | pts2d | kf_idx | feat_idx | poses | err | pnp records | records | matches | inliers] down
    Carve in, out;
    const size_t i_kp = in.take(sizeof(orbx_keypoint) * NF), i_de = in.take(32 * NF), i_kd = in.take(32 * K), i_po = in.take(24 * K), i_va = in.take(K),
                 i_pr = in.take(56 * B), i_fs = in.take(4 * B), i_fc = in.take(4 * B), i_it = in.take(sizeof(TrackRefItem) * B);
    const size_t o_of = out.take(4 * (B + 1)), o_p3 = out.take(24 * K), o_p2 = out.take(8 * K), o_ki = out.take(4 * K), o_fi = out.take(4 * K),
                 o_ps = out.take(56 * B), o_er = out.take(8 * K), o_pn = out.take(sizeof(orbx_pnp_result) * B),
                 o_rs = out.take(sizeof(orbx_track_ref_result) * B), o_ma = out.take(sizeof(orbx_dmatch) * K), o_in = out.take(K);
    HostCall c;
    if (int rc = orbx_host_call_begin(h, h->pin_tref, h->ws_tref[1], in.off, out.off, c)) return rc;
    uint8_t *hi = c.hi, *ho = c.ho, *di = c.di, *dout = c.dout;
    if (NF) { std::memcpy(hi + i_kp, kp, sizeof(orbx_keypoint) * NF); std::memcpy(hi + i_de, desc, 32 * NF); }
    if (K) { std::memcpy(hi + i_kd, kf_desc, 32 * K); std::memcpy(hi + i_po, kf_positions, 24 * K); std::memcpy(hi + i_va, kf_valid, K); }
    std::memcpy(hi + i_pr, priors_wc, 56 * B);
    for (size_t b = 0; b < B; ++b) {
      ((int*)(hi + i_fs))[b] = feat_offsets[b];
      ((int*)(hi + i_fc))[b] = feat_offsets[b + 1] - feat_offsets[b];
      TrackRefItem it;
      it.kf_desc = di + i_kd + 32 * (size_t)kf_offsets[b]; it.kf_off = kf_offsets[b]; it.n = kf_offsets[b + 1] - kf_offsets[b];
      ((TrackRefItem*)(hi + i_it))[b] = it;
    }
    if (int rc = orbx_host_call_upload(h, c)) return rc;
    TrefArgs A{};
    A.min_corr = min_correspondences; A.max_feat = max_feat; A.fc_stride = 1;
    A.kp = (const orbx_keypoint*)(di + i_kp); A.desc = di + i_de; A.feat_start = (const int*)(di + i_fs); A.feat_count = (const int*)(di + i_fc);
    A.items = (const TrackRefItem*)(di + i_it); A.positions = (const double*)(di + i_po); A.valid = di + i_va; A.priors = (const double*)(di + i_pr);
    A.matches = (orbx_dmatch*)(dout + o_ma); A.offsets = (int*)(dout + o_of); A.pts3d = (double*)(dout + o_p3); A.pts2d = (float*)(dout + o_p2);
    A.kf_idx = (int*)(dout + o_ki); A.feat_idx = (int*)(dout + o_fi); A.poses_out = (double*)(dout + o_ps);
    A.results = (orbx_track_ref_result*)(dout + o_rs);
    if (int rc = tref_launch(h, cam, pnp_cfg, n_frames, max_kf, K, A, dout + o_in, (double*)(dout + o_er), (orbx_pnp_result*)(dout + o_pn))) return rc;
    if (int rc = orbx_host_call_download(h, c, out.off)) return rc;
    std::memcpy(offsets, ho + o_of, 4 * (B + 1));
    std::memcpy(poses_wc_out, ho + o_ps, 56 * B);
    std::memcpy(pnp_results, ho + o_pn, sizeof(orbx_pnp_result) * B);
    std::memcpy(results, ho + o_rs, sizeof(orbx_track_ref_result) * B);
    const size_t N = (size_t)offsets[B];
    if (N) {
      std::memcpy(pts3d, ho + o_p3, 24 * N); std::memcpy(pts2d, ho + o_p2, 8 * N); std::memcpy(kf_idx, ho + o_ki, 4 * N);
      std::memcpy(feat_idx, ho + o_fi, 4 * N); std::memcpy(err_out, ho + o_er, 8 * N); std::memcpy(inlier_out, ho + o_in, N);
    }
    for (size_t b = 0; b < B; ++b) {
      const size_t n = (size_t)results[b].n_matches;
      if (n) std::memcpy(matches + kf_offsets[b], ho + o_ma + sizeof(orbx_dmatch) * (size_t)kf_offsets[b], sizeof(orbx_dmatch) * n);
    }
    return ORBX_OK;
  });
}

}  // extern "C"
