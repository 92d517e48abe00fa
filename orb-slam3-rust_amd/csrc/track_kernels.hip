// track_kernels.hip — the numeric part of the tracker's per-frame step for a batch of frames (orbx_track_frames[_device]).
//
// Replaces, for B frames in one call and with no host synchronisation inside:
//   src/tracking/tracker.rs:863-988    track_local_map        (mode 1): project, grid search with ratio test, gather, PnP, matched
//   src/tracking/tracker.rs:1086-1192  track_with_motion_model (mode 0): project, bounds test, grid search, gather, PnP
//
// Four launches around PnP's three (pnp_kernels.hip, unchanged):
//   track_grid_build_kernel   one workgroup per frame: the FeatureGrid as a counting sort (guided_search_dev.hpp), matched = -1
//   track_search_kernel       one wave per map point, frames as grid.y: projection (one IEEE operation at a time, every lane
//                             computes the same numbers) + guided_search_wave — the search guided_match_kernel runs
//   track_gather_kernel       one workgroup per frame: offsets[b] = sum of the earlier frames' counts, then the ordered
//                             compaction of the frame's matches (BlockAppend, block_dev.hpp) into PnP's layout
//   (PnP)
//   track_finish_kernel       one workgroup per frame: status, matched[feat] (the later inlier wins: atomicMax on the
//                             correspondence index), the prior's bytes where the tracker falls back to it
// The only atomics are integer counters and that max: every output is a deterministic function of the inputs.
#include <algorithm>
#include <cmath>

#include "block_dev.hpp"
#include "guided_search_dev.hpp"
#include "orbx_internal.hpp"
#include "pose_dev.hpp"

namespace {

constexpr int TRK_THREADS = 256;

// a count outside [0, max_feat] is searched as no features at all
__device__ __forceinline__ int track_feat_count(const TrackArgs& A, int b) {
  const int n = A.feat_count[(size_t)b * A.fc_stride];
  return (n < 0 || n > A.max_feat) ? 0 : n;
}

__global__ __launch_bounds__(GG_THREADS) void track_grid_build_kernel(TrackArgs A) {
  const int b = blockIdx.x;
  const int n = track_feat_count(A, b);
  const size_t f0 = (size_t)b * A.max_feat;
  const orbx_keypoint* kp = A.kp + (n > 0 ? (size_t)A.feat_start[b] : 0);
  grid_build_body(kp, n, A.winv, A.hinv, A.cell_start + (size_t)b * (GG_CELLS + 1), A.sorted_idx + f0, A.cell_of + f0);
  for (int i = threadIdx.x; i < A.max_feat; i += GG_THREADS) { A.matched[f0 + i] = -1; A.owner[f0 + i] = -1; }
  if (threadIdx.x == 0) { A.counts[2 * b] = 0; A.counts[2 * b + 1] = 0; }
}

// match[m] = the keypoint index, -1 (in front, no match) or -2 (behind the camera)
__global__ __launch_bounds__(TRK_THREADS) void track_search_kernel(TrackArgs A) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int m0 = A.mp_off[b], nm = A.mp_off[b + 1] - m0;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nm) return;
  const size_t m = (size_t)m0 + i;
  double cw[7], pc[3];
  se3_inverse7(A.search_poses + 7 * (size_t)b, cw, cw + 4);                 // pose.inverse()
  se3_transform_point(cw, A.positions + 3 * m, pc);
  const double x = pc[0], y = pc[1], z = pc[2];
  int res = -2;
  if (!(z <= 0.0)) {                                                        // tracker.rs:872, :1109
    res = -1;
    const double u = A.cam.fx * x / z + A.cam.cx;                           // :877-878, :1114-1115
    const double v = A.cam.fy * y / z + A.cam.cy;
    const double width = 2.0 * A.cam.cx, height = 2.0 * A.cam.cy;           // :1119-1120
    if (!(A.mode == 0 && (u < 0.0 || u >= width || v < 0.0 || v >= height))) {   // :1121 (mode 0 only)
      const int n = track_feat_count(A, b);
      const size_t f0 = (size_t)b * A.max_feat;
      const uint8_t* desc = A.desc + (n > 0 ? (size_t)A.feat_start[b] * 32 : 0);
      const Desc256 dq = load_desc(A.mp_desc + m * 32);
      unsigned rd;
      res = guided_search_wave(desc, A.cell_start + (size_t)b * (GG_CELLS + 1), A.sorted_idx + f0, A.cell_of + f0, u, v, dq, A.radius,
                               A.winv, A.hinv, A.mode, lane, &rd);
    }
  }
  if (lane == 0) {
    A.match[m] = res;
    if (res >= -1) atomicAdd(&A.counts[2 * b + 1], 1);
    if (res >= 0) atomicAdd(&A.counts[2 * b], 1);
  }
}

__global__ __launch_bounds__(TRK_THREADS) void track_gather_kernel(TrackArgs A, int B) {
  __shared__ int wave_tot[TRK_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  // offsets[b]: the correspondences of the frames before this one
  int part = 0;
  for (int j = tid; j < b; j += TRK_THREADS) part += A.counts[2 * j];
  BlockAppend<TRK_THREADS, 1> app(wave_tot);
  app.total[0] = block_sum<TRK_THREADS>(part, wave_tot);
  if (tid == 0) {
    A.offsets[b] = app.total[0];
    if (b == B - 1) A.offsets[B] = app.total[0] + A.counts[2 * b];
  }
  const int m0 = A.mp_off[b], nm = A.mp_off[b + 1] - m0;
  const orbx_keypoint* kp = A.kp + (track_feat_count(A, b) > 0 ? (size_t)A.feat_start[b] : 0);
  for (int base = 0; base < nm; base += TRK_THREADS) {
    const int i = base + tid;
    const int f = i < nm ? A.match[(size_t)m0 + i] : -1;
    const size_t o = (size_t)app.round(f >= 0);
    if (f >= 0) {
      const size_t m = (size_t)m0 + i;
      A.pts3d[3 * o] = A.positions[3 * m]; A.pts3d[3 * o + 1] = A.positions[3 * m + 1]; A.pts3d[3 * o + 2] = A.positions[3 * m + 2];   // :919
      A.pts2d[2 * o] = kp[f].x; A.pts2d[2 * o + 1] = kp[f].y;                                                                        // :920
      A.mp_idx[o] = i; A.feat_idx[o] = f;                                                                                            // :921
    }
  }
}

__global__ __launch_bounds__(TRK_THREADS) void track_finish_kernel(TrackArgs A) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n_corr = A.counts[2 * b], n_front = A.counts[2 * b + 1];
  const orbx_pnp_result pr = A.pnp_res[b];
  int status = ORBX_TRACK_OK, n_inl = pr.n_inliers;
  if (n_corr < A.min_corr) { status = ORBX_TRACK_TOO_FEW_CORRESPONDENCES; n_inl = 0; }   // :937, :1173
  else if (n_inl < A.min_inl) status = ORBX_TRACK_TOO_FEW_INLIERS;                        // :1186
  else if (pr.status == ORBX_PNP_NO_MODEL) status = ORBX_TRACK_NO_MODEL;
  if (status != ORBX_TRACK_TOO_FEW_CORRESPONDENCES) {
    // :960-973: matched[feat] = the map point of the inlier on it; the reference's loop overwrites, so the later one stays
    const size_t base = (size_t)A.offsets[b], f0 = (size_t)b * A.max_feat;
    for (int i = tid; i < n_corr; i += TRK_THREADS)
      if (A.inl[base + i]) atomicMax(&A.owner[f0 + A.feat_idx[base + i]], i);
    __threadfence();
    __syncthreads();
    for (int i = tid; i < n_corr; i += TRK_THREADS) {
      if (!A.inl[base + i]) continue;
      const int f = A.feat_idx[base + i];
      if (__hip_atomic_load(&A.owner[f0 + f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i) A.matched[f0 + f] = A.mp_idx[base + i];
    }
  }
  if ((status == ORBX_TRACK_TOO_FEW_CORRESPONDENCES || status == ORBX_TRACK_TOO_FEW_INLIERS) && tid < 7)
    A.poses_out[7 * (size_t)b + tid] = A.priors[7 * (size_t)b + tid];
  if (tid == 0) {
    orbx_track_result r;
    r.status = status; r.n_in_front = n_front; r.n_correspondences = n_corr; r.n_inliers = n_inl;
    A.results[b] = r;
  }
}

}  // namespace

// what can be refused before anything is enqueued; *max_mp: the most map points of a frame
int track_check(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* c, const orbx_pnp_config* pnp_cfg, int B, const int* mp_offsets,
                int* max_mp, const char* who) {
  if (int rc = orbx_pnp_check_config(h, pnp_cfg, who)) return rc;
  if (!cam || !c || (c->mode != 0 && c->mode != 1) || !(c->radius >= 0.0) || !std::isfinite(c->radius) || !(c->img_w > 0.0) ||
      !std::isfinite(c->img_w) || !(c->img_h > 0.0) || !std::isfinite(c->img_h) || c->min_correspondences < 4 || c->min_inliers < 0)
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: configuration out of range (include/orbx.h: orbx_track_config)", who);
  if (B <= 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: n_frames must be positive", who);
  return orbx_check_offsets(h, who, "mp_offsets", "frame", B, mp_offsets, max_mp);
}

// The launches on the handle's stream; every pointer is device memory (d_mp_off included: the callers upload it).
int track_launch(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg, int B, int max_mp,
                 size_t M, TrackArgs A, uint8_t* d_inl, double* d_err, orbx_pnp_result* d_pnp) {
  const size_t mf = (size_t)A.max_feat;
  Carve ws;
  const size_t o_cs = ws.take(4 * (size_t)B * (GG_CELLS + 1)), o_si = ws.take(4 * B * mf), o_ow = ws.take(4 * B * mf), o_cn = ws.take(8 * (size_t)B),
               o_ma = ws.take(4 * M), o_co = ws.take(2 * B * mf);
  if (int rc = orbx_reserve(h, h->ws_track[0], ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_track[0].p;
  A.cell_start = (int*)(w + o_cs); A.sorted_idx = (int*)(w + o_si); A.owner = (int*)(w + o_ow); A.counts = (int*)(w + o_cn);
  A.match = (int*)(w + o_ma); A.cell_of = (unsigned short*)(w + o_co);
  A.cam = *cam;
  A.mode = cfg->mode; A.min_corr = cfg->min_correspondences; A.min_inl = cfg->min_inliers; A.radius = cfg->radius;
  A.winv = (double)GG_COLS / (cfg->img_w - 0.0); A.hinv = (double)GG_ROWS / (cfg->img_h - 0.0);   // tracking_frame.rs:58-59
  A.inl = d_inl; A.pnp_res = d_pnp;
  orbx_launch(h, "track_grid_build_kernel", false, track_grid_build_kernel, dim3(B), dim3(GG_THREADS), 0, A);
  if (max_mp > 0) orbx_launch(h, "track_search_kernel", true, track_search_kernel, dim3((max_mp + 3) / 4, B), dim3(TRK_THREADS), 0, A);
  orbx_launch(h, "track_gather_kernel", true, track_gather_kernel, dim3(B), dim3(TRK_THREADS), 0, A, B);
  ORBX_HIP(h, hipGetLastError());
  if (int rc = orbx_pnp_ransac_batch_device(h, cam, pnp_cfg, B, max_mp, A.offsets, A.pts3d, A.pts2d, A.priors, A.poses_out, d_inl, d_err, d_pnp))
    return rc;
  orbx_launch(h, "track_finish_kernel", true, track_finish_kernel, dim3(B), dim3(TRK_THREADS), 0, A);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

extern "C" {

void orbx_default_track_config(int mode, orbx_track_config* c) {
  if (!c) return;
  c->mode = mode;
  c->radius = 15.0;                                  // tracker.rs:881, :1091
  c->img_w = 752.0; c->img_h = 480.0;
  c->min_correspondences = mode == 0 ? 10 : 4;       // :1173, :937
  c->min_inliers = mode == 0 ? 10 : 0;               // :1186
}

int orbx_track_frames_device(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                             int n_frames, const orbx_keypoint* d_kp, const uint8_t* d_desc, const int* d_feat_start,
                             const int* d_feat_count, int feat_count_stride, int max_feat, const double* d_positions,
                             const uint8_t* d_mp_desc, const int* mp_offsets, const double* d_search_poses_wc, const double* d_priors_wc, int* d_offsets,
                             double* d_pts3d, float* d_pts2d, int* d_mp_idx, int* d_feat_idx, double* d_poses_wc_out,
                             uint8_t* d_inlier_out, double* d_err_out, orbx_pnp_result* d_pnp_results, int* d_matched,
                             orbx_track_result* d_results) {
  if (!h) return ORBX_ERR_INVALID;
  int max_mp = 0;
  if (int rc = track_check(h, cam, cfg, pnp_cfg, n_frames, mp_offsets, &max_mp, "orbx_track_frames_device")) return rc;
  const int B = n_frames;
  const int M = mp_offsets[B];
  if (max_feat < 0 || feat_count_stride < 1 || !d_feat_start || !d_feat_count || !d_search_poses_wc || !d_priors_wc || !d_offsets || !d_poses_wc_out ||
      !d_pnp_results || !d_results || (max_feat > 0 && (!d_kp || !d_desc || !d_matched)) ||
      (M > 0 && (!d_positions || !d_mp_desc || !d_pts3d || !d_pts2d || !d_mp_idx || !d_feat_idx || !d_inlier_out || !d_err_out)))
    return orbx_fail(h, ORBX_ERR_INVALID, "orbx_track_frames_device: bad argument");
  ORBX_HIP(h, hipSetDevice(h->device));
  // mp_offsets goes up through the upload ring, so that the caller's array is free when the call returns
  const size_t ob = 4 * ((size_t)B + 1);
  uint8_t *hs, *ds;
  if (int rc = orbx_ring_begin(h, h->ring_track, h->ws_track[2], ob, &hs, &ds)) return rc;
  std::memcpy(hs, mp_offsets, ob);
  if (int rc = orbx_ring_commit(h, h->ring_track, h->ws_track[2], ob)) return rc;
  TrackArgs A{};
  A.max_feat = max_feat; A.fc_stride = feat_count_stride;
  A.kp = d_kp; A.desc = d_desc; A.feat_start = d_feat_start; A.feat_count = d_feat_count;
  A.positions = d_positions; A.mp_desc = d_mp_desc; A.mp_off = (const int*)ds;
  A.search_poses = d_search_poses_wc; A.priors = d_priors_wc;
  A.offsets = d_offsets; A.pts3d = d_pts3d; A.pts2d = d_pts2d; A.mp_idx = d_mp_idx; A.feat_idx = d_feat_idx;
  A.poses_out = d_poses_wc_out; A.matched = d_matched; A.results = d_results;
  return track_launch(h, cam, cfg, pnp_cfg, B, max_mp, (size_t)M, A, d_inlier_out, d_err_out, d_pnp_results);
}

int orbx_track_frames(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                      int n_frames, const orbx_keypoint* kp, const uint8_t* desc, const int* feat_offsets, const double* positions,
                      const uint8_t* mp_desc, const int* mp_offsets, const double* search_poses_wc, const double* priors_wc,
                      int* offsets, double* pts3d, float* pts2d, int* mp_idx, int* feat_idx, double* poses_wc_out,
                      uint8_t* inlier_out, double* err_out, orbx_pnp_result* pnp_results, int* matched, orbx_track_result* results) {
  if (!h) return ORBX_ERR_INVALID;
  int max_feat = 0, max_mp = 0;
  if (int rc = track_check(h, cam, cfg, pnp_cfg, n_frames, mp_offsets, &max_mp, "orbx_track_frames")) return rc;
  if (int rc = orbx_check_offsets(h, "orbx_track_frames", "feat_offsets", "frame", n_frames, feat_offsets, &max_feat)) return rc;
  const size_t B = (size_t)n_frames;
  const size_t NF = (size_t)feat_offsets[B], M = (size_t)mp_offsets[B], mf = (size_t)max_feat;
  if (!search_poses_wc || !priors_wc || !offsets || !poses_wc_out || !pnp_results || !results || (NF > 0 && (!kp || !desc || !matched)) ||
      (M > 0 && (!positions || !mp_desc || !pts3d || !pts2d || !mp_idx || !feat_idx || !inlier_out || !err_out)))
    return orbx_fail(h, ORBX_ERR_INVALID, "orbx_track_frames: bad argument");
  ORBX_HIP(h, hipSetDevice(h->device));
  // one blob each way: [kp | desc | positions | mp_desc | search poses | priors | feat_start | feat_count | mp_offsets] up,
  // [offsets | pts3d | pts2d | mp_idx | feat_idx | poses | err | pnp records | matched | records | inliers] down
  Carve in, out;
  const size_t i_kp = in.take(sizeof(orbx_keypoint) * NF), i_de = in.take(32 * NF), i_po = in.take(24 * M), i_md = in.take(32 * M),
               i_sp = in.take(56 * B), i_pr = in.take(56 * B), i_fs = in.take(4 * B), i_fc = in.take(4 * B), i_mo = in.take(4 * (B + 1));
  const size_t o_of = out.take(4 * (B + 1)), o_p3 = out.take(24 * M), o_p2 = out.take(8 * M), o_mi = out.take(4 * M), o_fi = out.take(4 * M),
               o_ps = out.take(56 * B), o_er = out.take(8 * M), o_pn = out.take(sizeof(orbx_pnp_result) * B), o_ma = out.take(4 * B * mf),
               o_rs = out.take(sizeof(orbx_track_result) * B), o_in = out.take(M);
  HostCall c;
  if (int rc = orbx_host_call_begin(h, h->pin_track, h->ws_track[1], in.off, out.off, c)) return rc;
  uint8_t *hi = c.hi, *ho = c.ho, *di = c.di, *dout = c.dout;
  if (NF) { std::memcpy(hi + i_kp, kp, sizeof(orbx_keypoint) * NF); std::memcpy(hi + i_de, desc, 32 * NF); }
  if (M) { std::memcpy(hi + i_po, positions, 24 * M); std::memcpy(hi + i_md, mp_desc, 32 * M); }
  std::memcpy(hi + i_sp, search_poses_wc, 56 * B);
  std::memcpy(hi + i_pr, priors_wc, 56 * B);
  for (size_t b = 0; b < B; ++b) {
    ((int*)(hi + i_fs))[b] = feat_offsets[b];
    ((int*)(hi + i_fc))[b] = feat_offsets[b + 1] - feat_offsets[b];
  }
  std::memcpy(hi + i_mo, mp_offsets, 4 * (B + 1));
  if (int rc = orbx_host_call_upload(h, c)) return rc;
  TrackArgs A{};
  A.max_feat = max_feat; A.fc_stride = 1;
  A.kp = (const orbx_keypoint*)(di + i_kp); A.desc = di + i_de; A.feat_start = (const int*)(di + i_fs); A.feat_count = (const int*)(di + i_fc);
  A.positions = (const double*)(di + i_po); A.mp_desc = di + i_md; A.mp_off = (const int*)(di + i_mo);
  A.search_poses = (const double*)(di + i_sp); A.priors = (const double*)(di + i_pr);
  A.offsets = (int*)(dout + o_of); A.pts3d = (double*)(dout + o_p3); A.pts2d = (float*)(dout + o_p2); A.mp_idx = (int*)(dout + o_mi);
  A.feat_idx = (int*)(dout + o_fi); A.poses_out = (double*)(dout + o_ps); A.matched = (int*)(dout + o_ma);
  A.results = (orbx_track_result*)(dout + o_rs);
  if (int rc = track_launch(h, cam, cfg, pnp_cfg, n_frames, max_mp, M, A, dout + o_in, (double*)(dout + o_er), (orbx_pnp_result*)(dout + o_pn)))
    return rc;
  if (int rc = orbx_host_call_download(h, c, out.off)) return rc;
  std::memcpy(offsets, ho + o_of, 4 * (B + 1));
  std::memcpy(poses_wc_out, ho + o_ps, 56 * B);
  std::memcpy(pnp_results, ho + o_pn, sizeof(orbx_pnp_result) * B);
  std::memcpy(results, ho + o_rs, sizeof(orbx_track_result) * B);
  const size_t N = (size_t)offsets[B];
  if (N) {
    std::memcpy(pts3d, ho + o_p3, 24 * N); std::memcpy(pts2d, ho + o_p2, 8 * N); std::memcpy(mp_idx, ho + o_mi, 4 * N);
    std::memcpy(feat_idx, ho + o_fi, 4 * N); std::memcpy(err_out, ho + o_er, 8 * N); std::memcpy(inlier_out, ho + o_in, N);
  }
  for (size_t b = 0; b < B; ++b) {
    const size_t n = (size_t)(feat_offsets[b + 1] - feat_offsets[b]);
    if (n) std::memcpy(matched + feat_offsets[b], ho + o_ma + 4 * b * mf, 4 * n);
  }
  return ORBX_OK;
}

}  // extern "C"
