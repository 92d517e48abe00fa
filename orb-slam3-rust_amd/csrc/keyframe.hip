// keyframe.hip — orbx_keyframe: the payload of NewKeyFrameMsg (src/system/messages.rs:19-51) with the feature arrays kept
// in device memory, so that what Tracking hands to Local Mapping — keypoints, descriptors, stereo points, map-point
// associations of a processed frame — feeds the descriptor searches of local mapping (guided match, triangulation search,
// fuse search: SURVEY.md §8f rows 1 and 3) without a D2H / H2D round trip of 60 bytes per feature per search.
// Host code only: the searches themselves are the *_device entry points of orbx_api.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "orbx_internal.hpp"

// ---- the neighbour loop of triangulate_from_neighbors (triangulation.rs:117-294), shared by orbx_keyframe_triangulate_from_neighbors
// and orbx_map_create_points[_device] (map_store_kernels.hip): which neighbours are searched and where their tables and scratch
// lie (plan), the tables themselves (fill), the launches (launch).  The callers differ in where the flags come from and in how the
// tables travel.

void tri_nb_plan(const orbx_camera* cam, const orbx_keyframe* cur, const orbx_keyframe* const* kfs, int T, TriNbPlan& P) {
  P.n1 = cur->n;
  const bool grid_ok = tri_grid_dims(cam, &P.cols, &P.rows);
  for (int t = 0; t < T; ++t) {
    const double dx = kfs[t]->pose_wc[4] - cur->pose_wc[4], dy = kfs[t]->pose_wc[5] - cur->pose_wc[5], dz = kfs[t]->pose_wc[6] - cur->pose_wc[6];
    if (std::sqrt(dx * dx + dy * dy + dz * dz) < cam->baseline) continue;                  // :137-141
    if (P.n1 == 0 || kfs[t]->n == 0) continue;
    const bool bow = cur->has_nodes && kfs[t]->has_nodes;                                   // :145
    if (!bow && !grid_ok) continue;
    P.orig.push_back(t);
    P.max_n2 = std::max(P.max_n2, kfs[t]->n);
  }
  const size_t Ts = P.orig.size(), n1 = (size_t)P.n1;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 15) & ~(size_t)15; return o; };
  P.sl.resize(Ts);
  P.o_items = take(sizeof(TriBatchItem) * Ts); P.o_nbs = take(sizeof(TriNeighbour) * Ts);
  for (size_t k = 0; k < Ts; ++k) {
    const orbx_keyframe* kf = kfs[P.orig[k]];
    P.sl[k].bow = cur->has_nodes && kf->has_nodes;
    if (P.sl[k].bow) { P.sl[k].sorted = take(4 * (size_t)kf->n); P.sl[k].lo = take(4 * n1); P.sl[k].hi = take(4 * n1); }
  }
  P.up_bytes = off;
  off = 0;
  for (size_t k = 0; k < Ts; ++k) {
    const size_t n2 = (size_t)kfs[P.orig[k]]->n;
    TriNbPlan::Slices& s = P.sl[k];
    if (!s.bow) { s.cell_start = take(4 * 4100); s.sorted = take(4 * n2); s.cell_of = take(2 * n2); }
    s.prop = take(4 * n1); s.owner = take(4 * n2); s.pairs = take(8 * n1); s.n_out = take(16); s.taken = take(n2);
  }
  P.o_status = take(2 * Ts * n1); P.o_points = take(24 * Ts * n1);
  P.ws_bytes = off;
}

// host side of the step: epipolar geometry per neighbour, candidate ranges where both keyframes carry nodes
void tri_nb_fill(const TriNbPlan& P, const orbx_camera* cam, const orbx_triangulation_config* cfg, const orbx_keyframe* cur, const orbx_keyframe* const* kfs,
                 const uint8_t* d_mp1, const uint8_t* const* d_mp2, uint8_t* up, uint8_t* d_up, uint8_t* d_ws) {
  const int n1 = P.n1;
  TriBatchItem* items = (TriBatchItem*)(up + P.o_items);
  TriNeighbour* nbs = (TriNeighbour*)(up + P.o_nbs);
  for (size_t k = 0; k < P.orig.size(); ++k) {
    const orbx_keyframe* kf = kfs[P.orig[k]];
    const TriNbPlan::Slices& s = P.sl[k];
    TriBatchItem it{};
    double ep[2];
    orbx_triangulation_geometry(cam, cur->pose_wc, kf->pose_wc, ep, it.A.F);
    it.A.epx = ep[0]; it.A.epy = ep[1];
    it.A.cols = s.bow ? 0 : P.cols; it.A.rows = s.bow ? 0 : P.rows; it.A.max_dist = cfg->max_descriptor_dist; it.A.n1 = n1; it.A.n2 = kf->n;
    it.A.kp1 = cur->d_kp; it.A.desc1 = cur->d_desc; it.A.mp1 = d_mp1; it.A.stereo1 = cur->d_has_point;
    it.A.kp2 = kf->d_kp; it.A.desc2 = kf->d_desc;
    it.A.sorted_idx = (const int*)((s.bow ? d_up : d_ws) + s.sorted);
    it.A.taken = d_ws + s.taken;
    if (s.bow) {
      it.A.rng_lo = (const int*)(d_up + s.lo); it.A.rng_hi = (const int*)(d_up + s.hi);
      int* sorted = (int*)(up + s.sorted); int* lo = (int*)(up + s.lo); int* hi = (int*)(up + s.hi);
      if (kf->n > 0) memcpy(sorted, kf->node_sorted.data(), 4 * (size_t)kf->n);
      orbx_node_ranges(cur->node.data(), n1, kf->node.data(), kf->node_sorted.data(), kf->node_m, lo, hi);   // the features of keyframe 2 in feature i's node (:577-581)
    } else {
      it.A.cell_start = (const int*)(d_ws + s.cell_start); it.A.cell_of = (const unsigned short*)(d_ws + s.cell_of);
    }
    it.mp2 = d_mp2[P.orig[k]];
    it.prop = (int*)(d_ws + s.prop); it.owner = (int*)(d_ws + s.owner); it.pairs = (int*)(d_ws + s.pairs); it.n_out = (int*)(d_ws + s.n_out);
    items[k] = it;
    TriNeighbour nb{};
    nb.kp2 = kf->d_kp; nb.pts2 = kf->d_points; nb.has2 = kf->d_has_point; nb.n2 = kf->n;
    memcpy(nb.pose2, kf->pose_wc, sizeof(nb.pose2));
    nb.pairs = it.pairs; nb.n_pairs_dev = it.n_out; nb.n_pairs = 0; nb.out_base = (int)k * n1;
    nbs[k] = nb;
  }
}

// the searches, the pair loop and the ordered compaction on the handle's stream, behind the upload of the tables
int tri_nb_launch(orbx_handle* h, const TriNbPlan& P, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial, const orbx_keyframe* cur,
                  const uint8_t* d_up, uint8_t* d_ws, int cap, int* d_head, int* d_out_nb, int* d_out_idx1, int* d_out_idx2, double* d_out_points) {
  const int Ts = (int)P.orig.size();
  TriCommon c{};
  tri_common_fill(&c, cam, cfg, is_inertial);
  c.kp1 = cur->d_kp; c.pts1 = cur->d_points; c.has1 = cur->d_has_point; c.n1 = P.n1;
  memcpy(c.pose1, cur->pose_wc, sizeof(c.pose1));
  const TriNeighbour* d_nbs = (const TriNeighbour*)(d_up + P.o_nbs);
  uint16_t* d_status = (uint16_t*)(d_ws + P.o_status);
  double* d_points = (double*)(d_ws + P.o_points);
  if (int rc = launch_search_for_triangulation_batch(h, (const TriBatchItem*)(d_up + P.o_items), Ts, P.n1, P.max_n2)) return rc;
  if (int rc = launch_triangulate_pairs(h, c, TriNeighbour{}, d_nbs, Ts, P.n1, d_status, d_points)) return rc;
  return launch_triangulate_compact(h, d_nbs, Ts, d_status, d_points, cap, d_head, d_out_nb, d_out_idx1, d_out_idx2, d_out_points);
}

extern "C" {

int orbx_keyframe_create(orbx_handle* h, const orbx_keypoint* d_kp, const uint8_t* d_desc, int n, const double* d_points_cam,
                         const uint8_t* d_has_point, uint64_t keyframe_id, uint64_t timestamp_ns, const double* pose_wc,
                         orbx_keyframe** out) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_keyframe_create", [&]() -> int {
    if (!out || n < 0 || (n > 0 && (!d_kp || !d_desc)) || ((d_points_cam == nullptr) != (d_has_point == nullptr)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_create: bad argument");
    *out = nullptr;
    ORBX_HIP(h, hipSetDevice(h->device));
    orbx_keyframe* kf = new orbx_keyframe();
    kf->h = h; kf->id = keyframe_id; kf->timestamp_ns = timestamp_ns; kf->n = n;
    if (pose_wc) memcpy(kf->pose_wc, pose_wc, sizeof(kf->pose_wc));
    kf->mp_ids.assign((size_t)n, -1);
    const size_t n1 = (size_t)(n > 0 ? n : 1);
    Carve blk;
    const size_t o_kp = blk.take(sizeof(orbx_keypoint) * n1), o_desc = blk.take(32 * n1), o_pts = blk.take(24 * n1), o_has = blk.take(n1), o_mp = blk.take(n1),
                 o_slot = blk.take(4 * n1), o_uniq = blk.take(4 * n1), total = blk.off;
    if (hipMalloc((void**)&kf->block, total) != hipSuccess) { delete kf; return orbx_fail(h, ORBX_ERR_HIP, "orbx_keyframe_create: out of device memory"); }
    kf->d_kp = (orbx_keypoint*)(kf->block + o_kp); kf->d_desc = kf->block + o_desc; kf->d_points = (double*)(kf->block + o_pts);
    kf->d_has_point = kf->block + o_has; kf->d_mp_flag = kf->block + o_mp; kf->d_mp_slot = (int*)(kf->block + o_slot);
    kf->d_mp_uniq = (int*)(kf->block + o_uniq);
    hipStream_t st = h->stream;
    hipError_t e = hipMemsetAsync(kf->block + o_pts, 0, total - o_pts, st);       // points (0,0,0), no stereo point, no map point
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(kf->d_kp, d_kp, sizeof(orbx_keypoint) * (size_t)n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(kf->d_desc, d_desc, 32 * (size_t)n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && n > 0 && d_points_cam) e = hipMemcpyAsync(kf->d_points, d_points_cam, 24 * (size_t)n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && n > 0 && d_has_point) e = hipMemcpyAsync(kf->d_has_point, d_has_point, (size_t)n, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) { hipFree(kf->block); delete kf; return orbx_fail(h, ORBX_ERR_HIP, "orbx_keyframe_create: %s", hipGetErrorString(e)); }
    *out = kf;
    return ORBX_OK;
  });
}

void orbx_keyframe_destroy(orbx_keyframe* kf) {
  if (!kf) return;
  hipSetDevice(kf->h->device);
  hipStreamSynchronize(kf->h->stream);
  if (kf->block) hipFree(kf->block);
  delete kf;
}

int orbx_keyframe_info(const orbx_keyframe* kf, int* n_features, uint64_t* keyframe_id, uint64_t* timestamp_ns, double* pose_wc) {
  if (!kf) return ORBX_ERR_INVALID;
  if (n_features) *n_features = kf->n;
  if (keyframe_id) *keyframe_id = kf->id;
  if (timestamp_ns) *timestamp_ns = kf->timestamp_ns;
  if (pose_wc) memcpy(pose_wc, kf->pose_wc, sizeof(kf->pose_wc));
  return ORBX_OK;
}

int orbx_keyframe_set_pose(orbx_keyframe* kf, const double* pose_wc) {
  if (!kf || !pose_wc) return ORBX_ERR_INVALID;
  memcpy(kf->pose_wc, pose_wc, sizeof(kf->pose_wc));
  return ORBX_OK;
}

int orbx_keyframe_set_map_points(orbx_keyframe* kf, const int64_t* mp_ids) {
  if (!kf || (kf->n > 0 && !mp_ids)) return ORBX_ERR_INVALID;
  orbx_handle* h = kf->h;
  return orbx_guard(h, "orbx_keyframe_set_map_points", [&]() -> int {
    ORBX_HIP(h, hipSetDevice(h->device));
    std::vector<uint8_t> flag((size_t)kf->n);
    for (int i = 0; i < kf->n; ++i) { kf->mp_ids[(size_t)i] = mp_ids[i]; flag[(size_t)i] = mp_ids[i] >= 0 ? 1 : 0; }
    if (kf->n > 0) {
      ORBX_HIP(h, hipMemcpyAsync(kf->d_mp_flag, flag.data(), (size_t)kf->n, hipMemcpyHostToDevice, h->stream));
      ORBX_HIP(h, hipStreamSynchronize(h->stream));                     // flag is a local
    }
    return ORBX_OK;
  });
}

int orbx_keyframe_get_map_points(const orbx_keyframe* kf, int64_t* mp_ids) {
  if (!kf || (kf->n > 0 && !mp_ids)) return ORBX_ERR_INVALID;
  if (kf->n > 0) memcpy(mp_ids, kf->mp_ids.data(), sizeof(int64_t) * (size_t)kf->n);
  return ORBX_OK;
}

int orbx_keyframe_download(const orbx_keyframe* kf, orbx_keypoint* kp, uint8_t* desc, double* points_cam, uint8_t* has_point) {
  if (!kf) return ORBX_ERR_INVALID;
  orbx_handle* h = kf->h;
  if (kf->n == 0) return ORBX_OK;
  ORBX_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)kf->n;
  if (kp) ORBX_HIP(h, hipMemcpyAsync(kp, kf->d_kp, sizeof(orbx_keypoint) * n, hipMemcpyDeviceToHost, h->stream));
  if (desc) ORBX_HIP(h, hipMemcpyAsync(desc, kf->d_desc, 32 * n, hipMemcpyDeviceToHost, h->stream));
  if (points_cam) ORBX_HIP(h, hipMemcpyAsync(points_cam, kf->d_points, 24 * n, hipMemcpyDeviceToHost, h->stream));
  if (has_point) ORBX_HIP(h, hipMemcpyAsync(has_point, kf->d_has_point, n, hipMemcpyDeviceToHost, h->stream));
  ORBX_HIP(h, hipStreamSynchronize(h->stream));
  return ORBX_OK;
}

const orbx_keypoint* orbx_keyframe_device_keypoints(const orbx_keyframe* kf) { return kf ? kf->d_kp : nullptr; }
const uint8_t* orbx_keyframe_device_descriptors(const orbx_keyframe* kf) { return kf ? kf->d_desc : nullptr; }

// ---- the searches of tracking / local mapping on device-resident keyframes ------------------------------------------------

int orbx_keyframe_guided_match(orbx_handle* h, const orbx_keyframe* kf, double img_w, double img_h, const double* q_uv,
                               const uint8_t* q_desc, int nq, double radius, int mode, int* out_idx, uint32_t* out_dist) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_keyframe_guided_match", [&]() -> int {
    if (!kf || kf->h != h || nq < 0 || (nq > 0 && (!q_uv || !q_desc || !out_idx || !out_dist)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_guided_match: bad argument (a keyframe belongs to the handle that made it)");
    if (nq == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    // only the queries travel (48 B each up, 8 B each down); the frame's n x 60 B of features stay where they are
    const size_t NQ = (size_t)nq;
    Carve in;
    const size_t i_uv = in.take(16 * NQ), i_qd = in.take(32 * NQ);
    OutputPlan out;
    const auto p_idx = out.add(out_idx, NQ);
    const auto p_dist = out.add(out_dist, NQ);
    if (int rc = out.begin(h, h->pin_io, h->ws_io.host_blob, in.off)) return rc;
    memcpy(out.call.hi + i_uv, q_uv, 16 * NQ);
    memcpy(out.call.hi + i_qd, q_desc, 32 * NQ);
    if (int rc = orbx_host_call_upload(h, out.call)) return rc;
    if (int rc = orbx_guided_match_device(h, kf->d_kp, kf->d_desc, kf->n, img_w, img_h, (const double*)(out.call.di + i_uv), out.call.di + i_qd, nq, radius, mode,
                                          out.dev(p_idx), out.dev(p_dist)))
      return rc;
    return out.finish(h);
  });
}

int orbx_keyframe_search_for_triangulation(orbx_handle* h, const orbx_camera* cam, const orbx_keyframe* kf1, const orbx_keyframe* kf2,
                                           unsigned max_dist, int* out_pairs, int* n_out) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_keyframe_search_for_triangulation", [&]() -> int {
    if (!cam || !kf1 || !kf2 || kf1->h != h || kf2->h != h || !n_out || (kf1->n > 0 && !out_pairs))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_search_for_triangulation: bad argument");
    *n_out = 0;
    if (kf1->n == 0 || kf2->n == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    OutputPlan out;                                                       // nothing goes up: the count and the pairs come down
    const auto p_n = out.add(n_out, 1);
    const auto p_pr = out.add(out_pairs, 2 * (size_t)kf1->n, true);
    if (int rc = out.begin(h, h->pin_io, h->ws_io.host_blob)) return rc;
    // map_point_ids[i].is_some() = the keyframe's map-point flags, points_cam[i].is_some() = its stereo flags (triangulation.rs:401-527)
    if (int rc = orbx_search_for_triangulation_device(h, cam, kf1->d_kp, kf1->d_desc, kf1->d_mp_flag, kf1->d_has_point, kf1->n, kf2->d_kp,
                                                      kf2->d_desc, kf2->d_mp_flag, kf2->n, kf1->pose_wc, kf2->pose_wc, max_dist, out.dev(p_pr), out.dev(p_n)))
      return rc;
    if (int rc = out.finish(h)) return rc;
    return out.copy(h, p_pr, 2 * (size_t)*n_out);
  });
}

int orbx_keyframe_set_feature_nodes(orbx_keyframe* kf, const uint32_t* node) {
  if (!kf) return ORBX_ERR_INVALID;
  return orbx_guard(kf->h, "orbx_keyframe_set_feature_nodes", [&]() -> int {
    kf->has_nodes = false; kf->node.clear(); kf->node_sorted.clear(); kf->node_m = 0;
    if (!node) return ORBX_OK;
    const int n = kf->n;
    kf->node.assign(node, node + n);
    kf->node_sorted.resize((size_t)n);
    kf->node_m = orbx_sort_by_node(node, n, kf->node_sorted.data());
    kf->has_nodes = true;
    return ORBX_OK;
  });
}

// triangulate_from_neighbors (triangulation.rs:71-308) without get_neighbor_keyframes and the map mutation: see include/orbx.h.
int orbx_keyframe_triangulate_from_neighbors(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                                             const orbx_keyframe* cur, const orbx_keyframe* const* kfs, int T, int cap, int* out_neighbour,
                                             int* out_idx1, int* out_idx2, double* out_points, int* n_out, int* stats) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_keyframe_triangulate_from_neighbors", [&]() -> int {
    if (!cam || !cfg || !cur || cur->h != h || !n_out || T < 0 || T > 256 || cap < 0 || cfg->max_descriptor_dist > 256 || (T > 0 && (!kfs || !stats)) ||
        (cap > 0 && (!out_neighbour || !out_idx1 || !out_idx2 || !out_points)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_triangulate_from_neighbors: bad argument (T <= 256; max_descriptor_dist <= 256; a keyframe belongs to the handle that made it)");
    *n_out = 0;
    for (int t = 0; t < T; ++t)
      if (!kfs[t] || kfs[t]->h != h)
        return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_triangulate_from_neighbors: keyframe %d is null or of another handle", t);
    if (T == 0) return ORBX_OK;
    memset(stats, 0, sizeof(int) * 4 * (size_t)T);
    TriNbPlan P;
    tri_nb_plan(cam, cur, kfs, T, P);
    const int Ts = (int)P.orig.size();
    if (Ts == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    // ---- up: items | neighbours | FeatureVector tables; down: head | the lists; the scratch stays in its own workspace
    const size_t Tz = (size_t)Ts, capd = std::min((size_t)cap, Tz * (size_t)P.n1);
    Carve in;
    in.take(P.up_bytes);
    OutputPlan out;
    const auto p_head = out.add((int*)nullptr, 1 + 4 * Tz);
    const auto p_nb = out.add((int*)nullptr, capd);
    const auto p_pts = out.add(out_points, 3 * capd, true);
    const auto p_i1 = out.add(out_idx1, capd, true);
    const auto p_i2 = out.add(out_idx2, capd, true);
    if (int rc = out.begin(h, h->pin_io, h->ws_io.host_blob, in.off)) return rc;
    if (int rc = orbx_reserve(h, h->ws_io.nb_scratch, P.ws_bytes)) return rc;
    uint8_t* d_ws = (uint8_t*)h->ws_io.nb_scratch.p;
    std::vector<const uint8_t*> mp2((size_t)T);
    for (int t = 0; t < T; ++t) mp2[(size_t)t] = kfs[t]->d_mp_flag;
    // map_point_ids[i].is_some() = the keyframes' map-point flags (triangulation.rs:94-107, :401-527)
    tri_nb_fill(P, cam, cfg, cur, kfs, cur->d_mp_flag, mp2.data(), out.call.hi, out.call.di, d_ws);
    if (int rc = orbx_host_call_upload(h, out.call)) return rc;
    if (int rc = tri_nb_launch(h, P, cam, cfg, is_inertial, cur, out.call.di, d_ws, (int)capd, out.dev(p_head), out.dev(p_nb), out.dev(p_i1), out.dev(p_i2),
                               out.dev(p_pts)))
      return rc;
    if (int rc = out.finish(h)) return rc;
    const int* head = out.host(p_head);
    for (int k = 0; k < Ts; ++k) {
      int* s4 = stats + 4 * (size_t)P.orig[(size_t)k];
      s4[0] = 1; s4[1] = head[2 + 4 * k]; s4[2] = head[3 + 4 * k]; s4[3] = head[4 + 4 * k];
    }
    *n_out = head[0];
    const size_t nw = std::min((size_t)head[0], capd);
    const int* nb_k = out.host(p_nb);
    for (size_t i = 0; i < nw; ++i) out_neighbour[i] = P.orig[(size_t)nb_k[i]];
    for (int rc : {out.copy(h, p_i1, nw), out.copy(h, p_i2, nw), out.copy(h, p_pts, 3 * nw)})
      if (rc) return rc;
    return ORBX_OK;
  });
}

// track_with_reference_kf (tracker.rs:992-1064) against resident keyframes: see include/orbx.h.  The launches are
// track_ref_kernels.hip's; each frame's item points at its keyframe's descriptors where they lie.
int orbx_keyframe_track_reference(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                                  int n_frames, const orbx_keyframe* const* kfs, const orbx_keypoint* d_kp, const uint8_t* d_desc,
                                  const int* d_feat_start, const int* d_feat_count, int feat_count_stride, int max_feat,
                                  const double* kf_positions, const uint8_t* kf_valid, const int* kf_offsets, const double* d_priors_wc,
                                  orbx_dmatch* d_matches, int* d_offsets, double* d_pts3d, float* d_pts2d, int* d_kf_idx,
                                  int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                                  orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results) {
  static const char* who = "orbx_keyframe_track_reference";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = orbx_pnp_check_config(h, pnp_cfg, who)) return rc;
    if (!cam || min_correspondences < 4 || n_frames < 0 || (n_frames > 0 && (!kfs || !kf_offsets)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (min_correspondences >= 4, n_frames >= 0)", who);
    if (n_frames == 0) return ORBX_OK;
    if (kf_offsets[0] != 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: kf_offsets[0] must be 0", who);
    std::vector<TrackRefItem> items((size_t)n_frames);
    for (int b = 0; b < n_frames; ++b) {
      const orbx_keyframe* kf = kfs[b];
      if (!kf || kf->h != h) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d is null or of another handle", who, b);
      if (kf_offsets[b + 1] - kf_offsets[b] != kf->n)
        return orbx_fail(h, ORBX_ERR_INVALID, "%s: kf_offsets gives keyframe %d %d rows, it has %d features", who, b, kf_offsets[b + 1] - kf_offsets[b], kf->n);
      items[(size_t)b].kf_desc = kf->d_desc; items[(size_t)b].kf_off = kf_offsets[b]; items[(size_t)b].n = kf->n;
    }
    return track_reference_enqueue(h, who, cam, pnp_cfg, min_correspondences, n_frames, d_kp, d_desc, d_feat_start, d_feat_count, feat_count_stride,
                                   max_feat, items.data(), kf_positions, kf_valid, true, d_priors_wc, d_matches, d_offsets, d_pts3d, d_pts2d, d_kf_idx,
                                   d_feat_idx, d_poses_wc_out, d_inlier_out, d_err_out, d_pnp_results, d_results);
  });
}

int orbx_keyframe_fuse_search(orbx_handle* h, const orbx_camera* cam, const double* positions, const uint8_t* mp_desc, int P,
                              const orbx_keyframe* const* kfs, int T, double radius_scale, unsigned desc_threshold, int* out_idx,
                              uint32_t* out_dist) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_keyframe_fuse_search", [&]() -> int {
    if (!cam || P < 0 || T < 0 || (P > 0 && (!positions || !mp_desc)) || (T > 0 && !kfs) || (P > 0 && T > 0 && (!out_idx || !out_dist)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_fuse_search: bad argument");
    if (P == 0 || T == 0) return ORBX_OK;
    std::vector<double> poses(7 * (size_t)T);
    size_t n = 0;
    for (int t = 0; t < T; ++t) {
      if (!kfs[t] || kfs[t]->h != h) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_fuse_search: keyframe %d is null or of another handle", t);
      n += (size_t)kfs[t]->n;
      memcpy(&poses[7 * (size_t)t], kfs[t]->pose_wc, 56);
    }
    ORBX_HIP(h, hipSetDevice(h->device));
    const size_t N = std::max(n, (size_t)1), Pz = (size_t)P, pt = Pz * (size_t)T;
    // the map points and the offsets travel in the blob; the target keyframes' features go side by side, device to device
    Carve in, side;
    const size_t i_pos = in.take(24 * Pz), i_md = in.take(32 * Pz), i_off = in.take(4 * ((size_t)T + 1));
    const size_t g_kps = side.take(sizeof(orbx_keypoint) * N), g_ds = side.take(32 * N);
    OutputPlan out;
    const auto p_idx = out.add(out_idx, pt);
    const auto p_dist = out.add(out_dist, pt);
    if (int rc = out.begin(h, h->pin_io, h->ws_io.host_blob, in.off)) return rc;
    if (int rc = orbx_reserve(h, h->ws_io.kf_gather, side.off)) return rc;
    uint8_t *hi = out.call.hi, *di = out.call.di;
    orbx_keypoint* d_kps = (orbx_keypoint*)((uint8_t*)h->ws_io.kf_gather.p + g_kps);
    uint8_t* d_descs = (uint8_t*)h->ws_io.kf_gather.p + g_ds;
    int* off = (int*)(hi + i_off);
    off[0] = 0;
    hipStream_t st = h->stream;
    for (int t = 0; t < T; ++t) {
      off[t + 1] = off[t] + kfs[t]->n;
      if (kfs[t]->n > 0) {
        ORBX_HIP(h, hipMemcpyAsync(d_kps + off[t], kfs[t]->d_kp, sizeof(orbx_keypoint) * (size_t)kfs[t]->n, hipMemcpyDeviceToDevice, st));
        ORBX_HIP(h, hipMemcpyAsync(d_descs + 32 * (size_t)off[t], kfs[t]->d_desc, 32 * (size_t)kfs[t]->n, hipMemcpyDeviceToDevice, st));
      }
    }
    memcpy(hi + i_pos, positions, 24 * Pz);
    memcpy(hi + i_md, mp_desc, 32 * Pz);
    if (int rc = orbx_host_call_upload(h, out.call)) return rc;
    if (int rc = orbx_fuse_search_device(h, cam, (const double*)(di + i_pos), di + i_md, P, poses.data(), (const int*)(di + i_off), d_kps, d_descs, T, radius_scale,
                                         desc_threshold, out.dev(p_idx), out.dev(p_dist)))
      return rc;
    return out.finish(h);
  });
}

int orbx_keyframe_verify_loop_candidates(orbx_handle* h, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int n_pairs,
                                         const orbx_keyframe* const* cur_kfs, const orbx_keyframe* const* loop_kfs, orbx_dmatch* matches,
                                         int* feature_matches, double* pts_current, double* pts_loop, uint8_t* inlier, double* sim3,
                                         orbx_loop_verify_result* results) {
  static const char* who = "orbx_keyframe_verify_loop_candidates";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (!cam || !cfg || n_pairs < 0 || (n_pairs > 0 && (!cur_kfs || !loop_kfs || !sim3 || !results)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (n_pairs == 0) return ORBX_OK;
    const size_t B = (size_t)n_pairs;
    std::vector<LoopVerifyPair> pairs(B);
    size_t N1 = 0;
    for (size_t b = 0; b < B; ++b) {
      const orbx_keyframe* c = cur_kfs[b];
      const orbx_keyframe* l = loop_kfs[b];
      if (!c || !l || c->h != h || l->h != h || N1 + (size_t)c->n > 0x7fffffffu)
        return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad keyframe at pair %d (a keyframe belongs to the handle that made it)", who, (int)b);
      LoopVerifyPair& p = pairs[b];
      p.c_desc = c->d_desc; p.c_pts = c->d_points; p.c_has = c->d_has_point; p.c_node = c->has_nodes ? c->node.data() : nullptr; p.n1 = c->n;
      p.l_kp = l->d_kp; p.l_desc = l->d_desc; p.l_pts = l->d_points; p.l_has = l->d_has_point; p.l_node = l->has_nodes ? l->node.data() : nullptr;
      p.n2 = l->n;
      memcpy(p.pose_c, c->pose_wc, sizeof(p.pose_c)); memcpy(p.pose_l, l->pose_wc, sizeof(p.pose_l));
      p.out_off = (int)N1;
      N1 += (size_t)c->n;
    }
    if (N1 > 0 && (!matches || !feature_matches || !pts_current || !pts_loop || !inlier)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    // the outputs in one device block: [sim3 | records | matches | feature matches | pts current | pts loop | inliers]
    Carve out;
    const size_t o_s3 = out.take(64 * B), o_rs = out.take(sizeof(orbx_loop_verify_result) * B), o_ma = out.take(sizeof(orbx_dmatch) * N1),
                 o_fm = out.take(8 * N1), o_pc = out.take(24 * N1), o_pl = out.take(24 * N1), o_in = out.take(N1);
    if (int rc = orbx_reserve(h, h->ws_lv[1], out.off)) return rc;
    uint8_t* d = (uint8_t*)h->ws_lv[1].p;
    if (int rc = loop_verify_enqueue(h, who, cam, cfg, n_pairs, pairs.data(), (orbx_dmatch*)(d + o_ma), (int*)(d + o_fm), (double*)(d + o_pc),
                                     (double*)(d + o_pl), d + o_in, (double*)(d + o_s3), (orbx_loop_verify_result*)(d + o_rs)))
      return rc;
    ORBX_HIP(h, hipMemcpyAsync(sim3, d + o_s3, 64 * B, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipMemcpyAsync(results, d + o_rs, sizeof(orbx_loop_verify_result) * B, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    for (size_t b = 0; b < B; ++b) {                                          // only what the records count travels
      const size_t k0 = (size_t)pairs[b].out_off, nm = (size_t)results[b].n_matches, np = (size_t)results[b].n_pairs;
      if (nm) ORBX_HIP(h, hipMemcpyAsync(matches + k0, d + o_ma + sizeof(orbx_dmatch) * k0, sizeof(orbx_dmatch) * nm, hipMemcpyDeviceToHost, h->stream));
      if (np) {
        ORBX_HIP(h, hipMemcpyAsync(feature_matches + 2 * k0, d + o_fm + 8 * k0, 8 * np, hipMemcpyDeviceToHost, h->stream));
        ORBX_HIP(h, hipMemcpyAsync(pts_current + 3 * k0, d + o_pc + 24 * k0, 24 * np, hipMemcpyDeviceToHost, h->stream));
        ORBX_HIP(h, hipMemcpyAsync(pts_loop + 3 * k0, d + o_pl + 24 * k0, 24 * np, hipMemcpyDeviceToHost, h->stream));
        ORBX_HIP(h, hipMemcpyAsync(inlier + k0, d + o_in + k0, np, hipMemcpyDeviceToHost, h->stream));
      }
    }
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    return ORBX_OK;
  });
}

// phase 4 of search_in_neighbors (search_in_neighbors.rs:139-150) on resident keyframes: see include/orbx.h.  The launches are
// mappoint_kernels.hip's; the keyframe table points at every keyframe's descriptors where they lie.
int orbx_keyframe_refresh_map_points(orbx_handle* h, int M, const double* positions, const int* obs_start, const int* obs_kf,
                                     const int* obs_feat, const orbx_keyframe* const* kfs, int T, double scale_range, uint8_t* mp_desc,
                                     double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records) {
  static const char* who = "orbx_keyframe_refresh_map_points";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (M < 0 || T < 0 || (T > 0 && !kfs)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    std::vector<MapPointKf> tab((size_t)T);
    for (int t = 0; t < T; ++t) {
      if (!kfs[t] || kfs[t]->h != h) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d is null or of another handle", who, t);
      tab[(size_t)t].desc = kfs[t]->d_desc; tab[(size_t)t].n = kfs[t]->n; tab[(size_t)t].pad_ = 0;
      memcpy(tab[(size_t)t].centre, kfs[t]->pose_wc + 4, sizeof(tab[(size_t)t].centre));
    }
    if (M == 0) return ORBX_OK;
    return mp_refresh_host_call(h, who, M, positions, obs_start, obs_kf, obs_feat, T, tab.data(), nullptr, nullptr, scale_range, mp_desc, normals,
                                min_distance, max_distance, records);
  });
}

}  // extern "C"
