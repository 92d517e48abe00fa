// orbx.hpp — C++17 host-side mirror of the reference crate's interface for the hot path, header-only, on top
// of the C ABI (orbx.h).  The reference is compiled Rust and Rust is not in this toolchain, so this is the
// compiled-language form of the thin shim INTEGRATION.md describes: same names, argument meaning and error
// behaviour as the reference (file:line relative to the reference crate root):
//
//   orbx::CameraModel                       src/tracking/frame/camera.rs:3-10
//   orbx::FeatureSet / StereoFrame          src/tracking/frame/stereo.rs:15-29
//   orbx::StereoProcessor::create/process   stereo.rs:37-66     (`new` is a keyword in C++)
//   orbx::descriptor_distance               stereo.rs:166-175
//   orbx::bf_match_crosscheck               src/tracking/tracker.rs:1001-1010
//   orbx::FeatureGrid-guided search         src/tracking/tracking_frame.rs:52-128, tracker.rs:880-923, :1126-1157
//   orbx::SE3                               src/geometry/se3.rs:5-8 (unit quaternion w,x,y,z + translation)
//   orbx::LocalBAConfigLM                   src/optimizer/local_ba_lm.rs:96-119
//   orbx::VisualObservation/ProblemData/ResultData   local_ba_lm.rs:48-93
//   orbx::solve_visual_ba                   local_ba_lm.rs:912-1098
//   orbx::PnPResult / solve_pnp_ransac_detailed    src/geometry/pnp.rs:12-20, :100-134
//   orbx::PoseInertialConfig/Result, PoseObservation, pose_inertial_optimization   src/optimizer/pose_inertial_optim.rs:19-216
//   orbx::KeyFrameDatabase / Candidate       src/atlas/keyframe_db.rs:22-95
//   orbx::LoopDetectorConfig / LoopCandidate / ConsistencyChecker / KeyFrameDatabase::detect_loop_candidates
//                                           src/loop_closing/detector.rs:17-167, :185-368
//
// Errors: the reference propagates `anyhow::Error` with `?` — here orbx::Error is thrown; where the
// reference returns `None` (solve_visual_ba) std::nullopt is returned.  Everything computes on the GPU.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <deque>
#include <functional>
#include <optional>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "orbx.h"

namespace orbx {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error("orbx error " + std::to_string(c) + ": " + m), code(c) {}
};

// ORB-SLAM3 matching thresholds, stereo.rs:10-12
constexpr uint32_t TH_HIGH = 100, TH_LOW = 50;
constexpr float NN_RATIO = 0.75f;

struct CameraModel {   // camera.rs:3-10
  double fx, fy, cx, cy, baseline;
  orbx_camera c() const { return orbx_camera{fx, fy, cx, cy, baseline}; }
};

using KeyPoint = orbx_keypoint;
using DMatch = orbx_dmatch;

struct FeatureSet {   // stereo.rs:15-19
  std::vector<KeyPoint> keypoints;
  std::vector<uint8_t> descriptors;   // keypoints.size() rows of 32 bytes
};

struct StereoFrame {   // stereo.rs:21-29
  FeatureSet left_features, right_features;
  std::vector<DMatch> matches_lr;
  std::vector<std::optional<std::array<double, 3>>> points_cam;   // per left keypoint
  uint64_t timestamp_ns = 0;
};

// RAII owner of one orbx_handle (one HIP stream on one device).  Not thread-safe, like `&mut self`.
class Handle {
 public:
  Handle(const CameraModel& cam, int n_features, int device = 0, int max_w = 1920, int max_h = 1080, int max_batch = 1) {
    if (orbx_abi_version() != ORBX_ABI_VERSION)       // the library on the loader's path was built from another orbx.h: struct strides differ
      throw Error(ORBX_ERR_INVALID, "liborbx_hip.so has ABI version " + std::to_string(orbx_abi_version()) + ", this caller was compiled against " + std::to_string(ORBX_ABI_VERSION));
    orbx_orb_params p;
    orbx_default_orb_params(n_features, &p);
    const orbx_camera c = cam.c();
    const int rc = orbx_create(&c, &p, device, max_w, max_h, max_batch, &h_);
    if (rc != ORBX_OK) throw Error(rc, orbx_last_error(nullptr));
    n_features_ = n_features;
  }
  Handle(orbx_handle* adopted, int n_features) : h_(adopted), n_features_(n_features) {}   // takes over a handle made through the C ABI (or none)
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h_(o.h_), n_features_(o.n_features_) { o.h_ = nullptr; }
  ~Handle() { if (h_) orbx_destroy(h_); }
  orbx_handle* get() const { return h_; }
  int n_features() const { return n_features_; }
  void check(int rc) const { if (rc != ORBX_OK) throw Error(rc, orbx_last_error(h_)); }

 private:
  orbx_handle* h_ = nullptr;
  int n_features_ = 0;
};

class StereoProcessor {   // stereo.rs:31-66
 public:
  // = StereoProcessor::new(camera, n_features) -> Result<Self>
  static StereoProcessor create(const CameraModel& camera, int n_features, int device = 0) {
    return StereoProcessor(camera, n_features, device);
  }
  // = process(&mut self, left: &Mat, right: &Mat, timestamp_ns) -> Result<StereoFrame>; images are CV_8UC1 rows
  StereoFrame process(const uint8_t* left, size_t lstride, const uint8_t* right, size_t rstride, int w, int h,
                      uint64_t timestamp_ns) {
    const size_t cap = (size_t)handle_.n_features() + 2048;
    StereoFrame f;
    f.left_features.keypoints.resize(cap); f.right_features.keypoints.resize(cap);
    f.left_features.descriptors.resize(cap * 32); f.right_features.descriptors.resize(cap * 32);
    f.matches_lr.resize(cap);
    std::vector<double> pts(cap * 3);
    std::vector<uint8_t> has(cap);
    int nl = 0, nr = 0, nm = 0;
    handle_.check(orbx_process_stereo(handle_.get(), left, lstride, right, rstride, w, h, f.left_features.keypoints.data(),
                                      f.left_features.descriptors.data(), &nl, f.right_features.keypoints.data(),
                                      f.right_features.descriptors.data(), &nr, (int)cap, f.matches_lr.data(), &nm,
                                      pts.data(), has.data()));
    f.left_features.keypoints.resize(nl); f.left_features.descriptors.resize((size_t)nl * 32);
    f.right_features.keypoints.resize(nr); f.right_features.descriptors.resize((size_t)nr * 32);
    f.matches_lr.resize(nm);
    f.points_cam.resize(nl);
    for (int i = 0; i < nl; ++i)
      if (has[i]) f.points_cam[i] = std::array<double, 3>{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    f.timestamp_ns = timestamp_ns;
    return f;
  }
  Handle& handle() { return handle_; }

 private:
  StereoProcessor(const CameraModel& camera, int n_features, int device) : handle_(camera, n_features, device) {}
  Handle handle_;
};

// stereo.rs:166-175
inline uint32_t descriptor_distance(Handle& h, const uint8_t* desc1, const uint8_t* desc2) {
  uint32_t d = 0;
  h.check(orbx_hamming_batch(h.get(), desc1, desc2, 1, &d));
  return d;
}

// tracker.rs:1001-1010: BFMatcher::new(NORM_HAMMING, true).train_match(query, train)
inline std::vector<DMatch> bf_match_crosscheck(Handle& h, const std::vector<uint8_t>& query, const std::vector<uint8_t>& train) {
  const int nq = (int)(query.size() / 32), nt = (int)(train.size() / 32);
  std::vector<DMatch> out((size_t)std::max(nq, 1));
  int n = 0;
  h.check(orbx_hamming_match_crosscheck(h.get(), query.data(), nq, train.data(), nt, out.data(), &n));
  out.resize(n);
  return out;
}

// FeatureGrid::get_features_in_area + descriptor search.  mode 0 = track_with_motion_model, 1 = track_local_map.
// Returns per query the matched keypoint index or -1.
inline std::vector<int> guided_match(Handle& h, const FeatureSet& frame, double img_w, double img_h,
                                     const std::vector<std::array<double, 2>>& uv, const std::vector<uint8_t>& q_desc,
                                     double radius, int mode) {
  const int nq = (int)uv.size();
  std::vector<int> idx((size_t)std::max(nq, 1));
  std::vector<uint32_t> dist((size_t)std::max(nq, 1));
  h.check(orbx_guided_match(h.get(), frame.keypoints.data(), frame.descriptors.data(), (int)frame.keypoints.size(), img_w, img_h,
                            nq ? &uv[0][0] : nullptr, q_desc.data(), nq, radius, mode, idx.data(), dist.data()));
  idx.resize(nq);
  return idx;
}

struct SE3 {   // se3.rs:5-8; rotation as unit quaternion (w, x, y, z)
  std::array<double, 4> rotation{1, 0, 0, 0};
  std::array<double, 3> translation{0, 0, 0};
};

namespace detail {
// SE3 <-> the seven doubles of the C ABI (qw, qx, qy, qz, tx, ty, tz)
inline void push7(std::vector<double>& v, const SE3& p) { v.insert(v.end(), p.rotation.begin(), p.rotation.end()); v.insert(v.end(), p.translation.begin(), p.translation.end()); }
inline SE3 se3_from7(const double* p) { return SE3{{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}}; }
// a std::function<bool()> as the (orbx_should_stop_fn, user) pair of a solve: an empty function is the null callback, `user` its address
inline int stop_trampoline(void* user) { return (*static_cast<const std::function<bool()>*>(user))() ? 1 : 0; }
inline orbx_should_stop_fn stop_fn(const std::function<bool()>& f) { return f ? &stop_trampoline : nullptr; }
inline void* stop_user(const std::function<bool()>& f) { return const_cast<std::function<bool()>*>(&f); }
}  // namespace detail

// triangulation.rs:401-527.  has_map_point1/2: the `map_point_ids[i].is_some()` flags; has_point_cam1: the
// `points_cam1[i].is_some()` flags.  Returns (idx1, idx2) pairs in ascending idx1.
inline std::vector<std::pair<size_t, size_t>> search_for_triangulation(
    Handle& h, const FeatureSet& f1, const std::vector<uint8_t>& has_map_point1, const std::vector<uint8_t>& has_point_cam1,
    const FeatureSet& f2, const std::vector<uint8_t>& has_map_point2, const SE3& pose1, const SE3& pose2,
    const CameraModel& camera, uint32_t max_dist) {
  const int n1 = (int)f1.keypoints.size(), n2 = (int)f2.keypoints.size();
  const double p1[7] = {pose1.rotation[0], pose1.rotation[1], pose1.rotation[2], pose1.rotation[3], pose1.translation[0], pose1.translation[1], pose1.translation[2]};
  const double p2[7] = {pose2.rotation[0], pose2.rotation[1], pose2.rotation[2], pose2.rotation[3], pose2.translation[0], pose2.translation[1], pose2.translation[2]};
  std::vector<int> pairs((size_t)std::max(n1, 1) * 2);
  int n = 0;
  const orbx_camera cam = camera.c();
  h.check(orbx_search_for_triangulation(h.get(), &cam, f1.keypoints.data(), f1.descriptors.data(), has_map_point1.data(),
                                        has_point_cam1.data(), n1, f2.keypoints.data(), f2.descriptors.data(),
                                        has_map_point2.data(), n2, p1, p2, max_dist, pairs.data(), &n));
  std::vector<std::pair<size_t, size_t>> out((size_t)n);
  for (int i = 0; i < n; ++i) out[(size_t)i] = {(size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]};
  return out;
}

// The search of fuse_points_into_keyframes (search_in_neighbors.rs:273-343) for every (map point, keyframe) pair.
// keyframes[t] = (pose, features); returns best feature index per pair, row-major [point][keyframe], -1 = none.
inline std::vector<int> fuse_search(Handle& h, const std::vector<std::array<double, 3>>& positions, const std::vector<uint8_t>& mp_descriptors,
                                    const std::vector<std::pair<SE3, const FeatureSet*>>& keyframes, const CameraModel& camera,
                                    double radius_factor = 3.0, uint32_t desc_threshold = 50) {
  const int P = (int)positions.size(), T = (int)keyframes.size();
  std::vector<double> poses(7 * (size_t)T);
  std::vector<int> off((size_t)T + 1, 0);
  std::vector<KeyPoint> kps;
  std::vector<uint8_t> descs;
  for (int t = 0; t < T; ++t) {
    const SE3& s = keyframes[(size_t)t].first;
    for (int i = 0; i < 4; ++i) poses[7 * (size_t)t + i] = s.rotation[i];
    for (int i = 0; i < 3; ++i) poses[7 * (size_t)t + 4 + i] = s.translation[i];
    const FeatureSet& f = *keyframes[(size_t)t].second;
    kps.insert(kps.end(), f.keypoints.begin(), f.keypoints.end());
    descs.insert(descs.end(), f.descriptors.begin(), f.descriptors.end());
    off[(size_t)t + 1] = (int)kps.size();
  }
  double s7 = 1.2;                       // scale_factor.powi(num_levels - 1) with num_levels = 8 (:248-249, :303)
  { const double a2 = 1.2 * 1.2, a4 = a2 * a2; s7 = (1.2 * a2) * a4; }
  std::vector<int> idx((size_t)P * T, -1);
  std::vector<uint32_t> dist((size_t)P * T, 0);
  const orbx_camera cam = camera.c();
  h.check(orbx_fuse_search(h.get(), &cam, P ? positions[0].data() : nullptr, mp_descriptors.data(), P, poses.data(), off.data(),
                           kps.data(), descs.data(), T, radius_factor * s7, desc_threshold, idx.data(), dist.data()));
  return idx;
}

// Phase 4 of search_in_neighbors (search_in_neighbors.rs:139-150) for M map points in one call: compute_distinctive_descriptors
// (map.rs:880-944) and update_map_point_normal_and_depth (map.rs:716-742, map_point.rs:173-203); orbx.h has the specification.
// Point p owns observations [obs_start[p], obs_start[p+1]) of obs_kf (index into `keyframes`) / obs_feat; mp_descriptors [M*32] and
// normals [M] are the points' current values, kept where a point is not updated.  scale_range = scale_factor.powi(num_levels - 1).
struct MapPointRefresh {
  std::vector<uint8_t> mp_descriptors;                    // [M*32]
  std::vector<std::array<double, 3>> normals;
  std::vector<double> min_distance, max_distance;
  std::vector<orbx_mp_refresh_record> records;            // chosen = position in the point's observation list, -1: not updated
  size_t num_descriptors_updated() const { size_t n = 0; for (const auto& r : records) n += r.chosen >= 0; return n; }
};
inline MapPointRefresh refresh_map_points(Handle& h, const std::vector<std::array<double, 3>>& positions, const std::vector<int>& obs_start,
                                          const std::vector<int>& obs_kf, const std::vector<int>& obs_feat,
                                          const std::vector<std::pair<SE3, const FeatureSet*>>& keyframes, double scale_range,
                                          const std::vector<uint8_t>& mp_descriptors, const std::vector<std::array<double, 3>>& normals) {
  const int M = (int)positions.size(), T = (int)keyframes.size();
  if (obs_start.size() != (size_t)M + 1 || mp_descriptors.size() != 32 * (size_t)M || normals.size() != (size_t)M || obs_kf.size() != obs_feat.size())
    throw Error(ORBX_ERR_INVALID, "refresh_map_points: inconsistent array lengths");
  std::vector<double> poses(7 * (size_t)T);
  std::vector<int> off((size_t)T + 1, 0);
  std::vector<uint8_t> descs;
  for (int t = 0; t < T; ++t) {
    const SE3& s = keyframes[(size_t)t].first;
    for (int i = 0; i < 4; ++i) poses[7 * (size_t)t + i] = s.rotation[i];
    for (int i = 0; i < 3; ++i) poses[7 * (size_t)t + 4 + i] = s.translation[i];
    const FeatureSet& f = *keyframes[(size_t)t].second;
    descs.insert(descs.end(), f.descriptors.begin(), f.descriptors.end());
    off[(size_t)t + 1] = (int)(descs.size() / 32);
  }
  MapPointRefresh r{mp_descriptors, normals, std::vector<double>((size_t)M), std::vector<double>((size_t)M), std::vector<orbx_mp_refresh_record>((size_t)M)};
  h.check(orbx_refresh_map_points(h.get(), M, M ? positions[0].data() : nullptr, obs_start.data(), obs_kf.data(), obs_feat.data(), T, poses.data(),
                                  off.data(), descs.data(), scale_range, r.mp_descriptors.data(), M ? r.normals[0].data() : nullptr,
                                  r.min_distance.data(), r.max_distance.data(), r.records.data()));
  return r;
}
// The same on resident keyframes (orbx_keyframe_create): their descriptors and poses are read where they lie.
inline MapPointRefresh refresh_map_points(Handle& h, const std::vector<std::array<double, 3>>& positions, const std::vector<int>& obs_start,
                                          const std::vector<int>& obs_kf, const std::vector<int>& obs_feat,
                                          const std::vector<const orbx_keyframe*>& keyframes, double scale_range,
                                          const std::vector<uint8_t>& mp_descriptors, const std::vector<std::array<double, 3>>& normals) {
  const int M = (int)positions.size();
  if (obs_start.size() != (size_t)M + 1 || mp_descriptors.size() != 32 * (size_t)M || normals.size() != (size_t)M || obs_kf.size() != obs_feat.size())
    throw Error(ORBX_ERR_INVALID, "refresh_map_points: inconsistent array lengths");
  MapPointRefresh r{mp_descriptors, normals, std::vector<double>((size_t)M), std::vector<double>((size_t)M), std::vector<orbx_mp_refresh_record>((size_t)M)};
  h.check(orbx_keyframe_refresh_map_points(h.get(), M, M ? positions[0].data() : nullptr, obs_start.data(), obs_kf.data(), obs_feat.data(),
                                           keyframes.data(), (int)keyframes.size(), scale_range, r.mp_descriptors.data(),
                                           M ? r.normals[0].data() : nullptr, r.min_distance.data(), r.max_distance.data(), r.records.data()));
  return r;
}

struct LocalBAConfigLM {   // local_ba_lm.rs:96-119, Default :109-119
  int max_iterations = 10;
  double param_tolerance = 1e-8, gradient_tolerance = 1e-8, huber_threshold = std::sqrt(5.991);
  int max_covisible_keyframes = 20;
};

using KeyFrameId = uint64_t;   // atlas/map/types.rs:9
using MapPointId = uint64_t;   // atlas/map/types.rs:29

struct VisualObservation {   // local_ba_lm.rs:68-78
  KeyFrameId kf_id;
  MapPointId mp_id;
  std::array<double, 2> observed_uv;
  bool is_kf_optimized;
};

struct VisualBAProblemData {   // local_ba_lm.rs:48-65; poses are T_cw
  std::unordered_map<KeyFrameId, SE3> local_kf_poses;
  std::unordered_map<MapPointId, std::array<double, 3>> local_mp_positions;
  std::unordered_map<KeyFrameId, SE3> fixed_kf_poses;
  KeyFrameId anchor_kf_id = 0;
  std::vector<VisualObservation> observations;
  std::vector<KeyFrameId> optimized_kf_ids;
  std::vector<MapPointId> mp_ids;
};

struct VisualBAResultData {   // local_ba_lm.rs:81-93; optimized_poses are T_wc
  std::unordered_map<KeyFrameId, SE3> optimized_poses;
  std::unordered_map<MapPointId, std::array<double, 3>> optimized_points;
  size_t iterations = 0;
  double initial_error = 0, final_error = 0;
};

// local_ba_lm.rs:912-1098.  The id -> index re-keying is the reference's own (:928-987).
inline std::optional<VisualBAResultData> solve_visual_ba(Handle& h, const VisualBAProblemData& problem, const CameraModel& camera,
                                                         const LocalBAConfigLM& config, const std::function<bool()>& should_stop) {
  std::unordered_map<KeyFrameId, int> kf_idx, fixed_idx;
  std::unordered_map<MapPointId, int> mp_idx;
  for (size_t i = 0; i < problem.optimized_kf_ids.size(); ++i) kf_idx[problem.optimized_kf_ids[i]] = (int)i;   // :928-933
  for (size_t i = 0; i < problem.mp_ids.size(); ++i) mp_idx[problem.mp_ids[i]] = (int)i;                       // :935-940
  std::vector<double> poses, fixed, points;
  for (KeyFrameId id : problem.optimized_kf_ids) {                       // :966-977 (missing pose -> zero params = identity)
    auto it = problem.local_kf_poses.find(id);
    detail::push7(poses, it != problem.local_kf_poses.end() ? it->second : SE3{});
  }
  for (const auto& kv : problem.fixed_kf_poses) { fixed_idx[kv.first] = (int)fixed_idx.size(); detail::push7(fixed, kv.second); }
  for (MapPointId id : problem.mp_ids) {                                 // :980-987
    auto it = problem.local_mp_positions.find(id);
    const std::array<double, 3> p = it != problem.local_mp_positions.end() ? it->second : std::array<double, 3>{0, 0, 0};
    points.insert(points.end(), p.begin(), p.end());
  }
  std::vector<orbx_ba_obs> obs;
  // the reference's observed_uv are keypoint coordinates widened from f32 (:870-872): when every one of them is an f32 value — always, for
  // a problem collect_visual_ba_data made — the observations travel in the 16-byte form (orbx_ba_obs32: same result, half the upload)
  std::vector<orbx_ba_obs32> obs32;
  bool all_f32 = true;
  const int F = (int)problem.fixed_kf_poses.size();
  for (const VisualObservation& o : problem.observations) {              // :943-961
    auto m = mp_idx.find(o.mp_id);
    if (m == mp_idx.end()) continue;                                     // :947
    orbx_ba_obs b{};
    b.mp_idx = m->second; b.u = o.observed_uv[0]; b.v = o.observed_uv[1];
    auto k = o.is_kf_optimized ? kf_idx.find(o.kf_id) : kf_idx.end();
    if (k != kf_idx.end()) { b.kf_idx = k->second; b.fixed_idx = -1; }
    else { auto f = fixed_idx.find(o.kf_id); b.kf_idx = -1; b.fixed_idx = f != fixed_idx.end() ? f->second : -1; }   // :569 identity
    obs.push_back(b);
    const float uf = (float)b.u, vf = (float)b.v;
    if ((double)uf != b.u || (double)vf != b.v) all_f32 = false;
    obs32.push_back(orbx_ba_obs32{b.kf_idx >= 0 ? b.kf_idx : -1 - (b.fixed_idx >= 0 ? b.fixed_idx : F), b.mp_idx, uf, vf});
  }
  const int K = (int)problem.optimized_kf_ids.size(), M = (int)problem.mp_ids.size();
  all_f32 = all_f32 && orbx_ba_has_collective(h.get()) == 0;             // (the point-partitioned solve takes orbx_ba_obs)
  std::vector<double> out((size_t)std::max(K, 1) * 7);
  int it = 0;
  double e0 = 0, e1 = 0;
  const orbx_camera c = camera.c();
  const orbx_ba_config cfg{config.max_iterations, config.param_tolerance, config.gradient_tolerance, config.huber_threshold,
                           config.max_covisible_keyframes};
  const int rc = all_f32 ? orbx_ba_solve_visual_obs32(h.get(), &c, &cfg, K, poses.data(), F, fixed.data(), M, points.data(), (int)obs32.size(),
                                                      obs32.data(), detail::stop_fn(should_stop), detail::stop_user(should_stop), out.data(), &it, &e0, &e1)
                         : orbx_ba_solve_visual(h.get(), &c, &cfg, K, poses.data(), F, fixed.data(), M, points.data(), (int)obs.size(),
                                                obs.data(), detail::stop_fn(should_stop), detail::stop_user(should_stop), out.data(), &it, &e0, &e1);
  if (rc != ORBX_OK) return std::nullopt;                                // :923-925 and every failure -> None
  VisualBAResultData r;
  for (int i = 0; i < K; ++i) {
    const SE3 p = detail::se3_from7(&out[7 * (size_t)i]);
    r.optimized_poses[problem.optimized_kf_ids[i]] = p;                  // T_wc, :1076
  }
  for (int j = 0; j < M; ++j) r.optimized_points[problem.mp_ids[j]] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
  r.iterations = (size_t)it; r.initial_error = e0; r.final_error = e1;
  return r;
}


// ---- input side (src/io/euroc.rs) -------------------------------------------------------------------------------
struct StereoImagePair {   // euroc.rs:21-26 (Mat -> row-major u8)
  std::vector<uint8_t> left, right;
  int width = 0, height = 0;
  uint64_t timestamp_ns = 0;
};

class EurocDataset {   // euroc.rs:54-132, the image side
 public:
  explicit EurocDataset(const std::string& mav0_dir) {   // EurocDataset::new (:64-90)
    char err[512] = {0};
    const int rc = orbx_euroc_open(mav0_dir.c_str(), &d_, err, sizeof(err));
    if (rc != ORBX_OK) throw Error(rc, err);
    orbx_camera c;
    orbx_euroc_calibration(d_, &c, nullptr, &w_, &h_);
    camera_ = CameraModel{c.fx, c.fy, c.cx, c.cy, c.baseline};
  }
  EurocDataset(const EurocDataset&) = delete;
  EurocDataset& operator=(const EurocDataset&) = delete;
  ~EurocDataset() { orbx_euroc_close(d_); }
  size_t len() const { return (size_t)orbx_euroc_len(d_); }
  std::optional<uint64_t> frame_timestamp(size_t idx) const {
    uint64_t ts;
    if (orbx_euroc_frame_timestamp(d_, (int)idx, &ts) != ORBX_OK) return std::nullopt;
    return ts;
  }
  const CameraModel& camera() const { return camera_; }
  int width() const { return w_; }
  int height() const { return h_; }
  StereoImagePair stereo_pair(size_t idx) const {        // :100-132
    StereoImagePair p;
    p.width = w_; p.height = h_;
    std::vector<uint8_t> both(2 * (size_t)w_ * h_);
    const int rc = orbx_euroc_read_pairs(d_, (int)idx, 1, both.data(), 2);
    if (rc != ORBX_OK) throw Error(rc, orbx_euroc_last_error(d_));
    p.left.assign(both.begin(), both.begin() + (size_t)w_ * h_);
    p.right.assign(both.begin() + (size_t)w_ * h_, both.end());
    p.timestamp_ns = *frame_timestamp(idx);
    return p;
  }
  // `count` pairs from `first` into out[pair][2][h][w] (e.g. orbx_host_alloc memory), decoded by `threads` host threads
  void read_pairs(size_t first, size_t count, uint8_t* out, int threads) const {
    const int rc = orbx_euroc_read_pairs(d_, (int)first, (int)count, out, threads);
    if (rc != ORBX_OK) throw Error(rc, orbx_euroc_last_error(d_));
  }

 private:
  orbx_euroc* d_ = nullptr;
  CameraModel camera_{};
  int w_ = 0, h_ = 0;
};

// ---- ORB vocabulary (src/vocabulary/mod.rs) ----------------------------------------------------------------------
using BowVector = std::unordered_map<uint32_t, double>;                  // mod.rs:31
using FeatureVector = std::unordered_map<uint32_t, std::vector<size_t>>; // mod.rs:37

class OrbVocabulary {   // mod.rs:83-94; the tree lives in device memory, transform runs on the GPU
 public:
  static OrbVocabulary load_from_text(Handle& h, const std::string& path) {   // mod.rs:117-211; throws where the reference returns Err
    orbx_vocabulary* v = nullptr;
    h.check(orbx_vocab_load_text(h.get(), path.c_str(), &v));
    return OrbVocabulary(h, v);
  }
  OrbVocabulary(const OrbVocabulary&) = delete;
  OrbVocabulary& operator=(const OrbVocabulary&) = delete;
  OrbVocabulary(OrbVocabulary&& o) noexcept : h_(o.h_), v_(o.v_) { o.v_ = nullptr; }
  ~OrbVocabulary() { if (v_) orbx_vocab_destroy(v_); }
  std::pair<size_t, size_t> params() const { int k, l; orbx_vocab_info(v_, &k, &l, nullptr, nullptr); return {(size_t)k, (size_t)l}; }
  size_t num_words() const { int n; orbx_vocab_info(v_, nullptr, nullptr, nullptr, &n); return (size_t)n; }
  size_t num_nodes() const { int n; orbx_vocab_info(v_, nullptr, nullptr, &n, nullptr); return (size_t)n; }
  const orbx_vocabulary* get() const { return v_; }

  // mod.rs:296-325: descent, accumulation of the two maps and the L1 normalisation on the GPU (orbx_bow_vectors; the norm is summed
  // in ascending word id, the reference sums in HashMap order).
  std::pair<BowVector, FeatureVector> transform(const std::vector<uint8_t>& descriptors, size_t levels_up) const {
    const int n = (int)(descriptors.size() / 32);
    std::vector<uint32_t> bw((size_t)std::max(n, 1)), fn((size_t)std::max(n, 1));
    std::vector<double> bv((size_t)std::max(n, 1));
    std::vector<int> fs((size_t)n + 1), fi((size_t)std::max(n, 1));
    int nb = 0, nf = 0;
    h_->check(orbx_bow_vectors(h_->get(), v_, descriptors.data(), n, (int)levels_up, bw.data(), bv.data(), &nb, fn.data(), fs.data(), fi.data(), &nf));
    BowVector bow;
    FeatureVector feat;
    for (int i = 0; i < nb; ++i) bow[bw[(size_t)i]] = bv[(size_t)i];
    for (int i = 0; i < nf; ++i) {
      std::vector<size_t>& l = feat[fn[(size_t)i]];
      for (int t = fs[(size_t)i]; t < fs[(size_t)i + 1]; ++t) l.push_back((size_t)fi[(size_t)t]);
    }
    return {std::move(bow), std::move(feat)};
  }
  BowVector transform_bow_only(const std::vector<uint8_t>& descriptors) const { return transform(descriptors, 0).first; }   // mod.rs:330-356

  static double score(const BowVector& v1, const BowVector& v2) {          // mod.rs:357-374 (orbx_bow_score: terms in ascending word id)
    auto flat = [](const BowVector& v, std::vector<uint32_t>& k, std::vector<double>& w) {
      for (const auto& kv : v) k.push_back(kv.first);
      std::sort(k.begin(), k.end());
      for (uint32_t x : k) w.push_back(v.at(x));
    };
    std::vector<uint32_t> k1, k2; std::vector<double> w1, w2;
    flat(v1, k1, w1); flat(v2, k2, w2);
    double s = 0.0;
    if (orbx_bow_score(k1.data(), w1.data(), (int)k1.size(), k2.data(), w2.data(), (int)k2.size(), &s) != ORBX_OK) throw Error(ORBX_ERR_INVALID, "orbx_bow_score");
    return s;
  }

 private:
  OrbVocabulary(Handle& h, orbx_vocabulary* v) : h_(&h), v_(v) {}
  Handle* h_;
  orbx_vocabulary* v_;
};

// triangulation.rs:541-658: candidates restricted to the same FeatureVector node.  Pairs in ascending idx1.
inline std::vector<std::pair<size_t, size_t>> search_for_triangulation_bow(
    Handle& h, const FeatureVector& feat_vec1, const FeatureVector& feat_vec2, const FeatureSet& f1, const std::vector<uint8_t>& has_map_point1,
    const std::vector<uint8_t>& has_point_cam1, const FeatureSet& f2, const std::vector<uint8_t>& has_map_point2, const SE3& pose1,
    const SE3& pose2, const CameraModel& camera, uint32_t max_dist) {
  const int n1 = (int)f1.keypoints.size(), n2 = (int)f2.keypoints.size();
  std::vector<uint32_t> node1((size_t)n1, 0xffffffffu), node2((size_t)n2, 0xffffffffu);
  for (const auto& kv : feat_vec1) for (size_t i : kv.second) if (i < (size_t)n1) node1[i] = kv.first;
  for (const auto& kv : feat_vec2) for (size_t i : kv.second) if (i < (size_t)n2) node2[i] = kv.first;
  const double p1[7] = {pose1.rotation[0], pose1.rotation[1], pose1.rotation[2], pose1.rotation[3], pose1.translation[0], pose1.translation[1], pose1.translation[2]};
  const double p2[7] = {pose2.rotation[0], pose2.rotation[1], pose2.rotation[2], pose2.rotation[3], pose2.translation[0], pose2.translation[1], pose2.translation[2]};
  std::vector<int> pairs((size_t)std::max(n1, 1) * 2);
  int n = 0;
  const orbx_camera cam = camera.c();
  h.check(orbx_search_for_triangulation_bow(h.get(), &cam, f1.keypoints.data(), f1.descriptors.data(), has_map_point1.data(),
                                            has_point_cam1.data(), node1.data(), n1, f2.keypoints.data(), f2.descriptors.data(),
                                            has_map_point2.data(), node2.data(), n2, p1, p2, max_dist, pairs.data(), &n));
  std::vector<std::pair<size_t, size_t>> out((size_t)n);
  for (int i = 0; i < n; ++i) out[(size_t)i] = {(size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]};
  return out;
}

// ---- new map points from neighbour keyframes (src/local_mapping/triangulation.rs) ---------------------------------------
struct TriangulationConfig {   // triangulation.rs:20-52
  size_t num_neighbors = 10;
  uint32_t max_descriptor_dist = 50;                  // TH_LOW
  double min_baseline_ratio = 0.01;
  double min_parallax_inertial = std::acos(0.9996), min_parallax_visual = std::acos(0.9998);
  double max_reproj_error_mono = 5.991, max_reproj_error_stereo = 7.8, scale_ratio_factor = 1.5;
  orbx_triangulation_config c() const {
    return orbx_triangulation_config{(int)num_neighbors, max_descriptor_dist, min_baseline_ratio, min_parallax_inertial, min_parallax_visual,
                                     max_reproj_error_mono, max_reproj_error_stereo, scale_ratio_factor};
  }
};
struct TriangulationResult {   // triangulation.rs:55-61
  size_t num_new_points = 0, num_pairs_checked = 0, num_matches_found = 0, num_triangulated = 0, num_validated = 0;
};
struct NewMapPoint {           // what :286-290 consumes: create_map_point(position, descriptor_of(idx1), current) + two associate calls
  size_t neighbour_index, idx1, idx2;
  std::array<double, 3> position;
};
// The pair loop (:184-293) on pairs from any search; status[i] = ORBX_TRI_* | ORBX_TRI_METHOD_* << 8.  points_cam may be empty
// (every point None), else has_point marks the Some entries.
inline std::vector<uint16_t> triangulate_pairs(Handle& h, const CameraModel& camera, const TriangulationConfig& config, bool is_inertial,
                                               const FeatureSet& f1, const std::vector<std::array<double, 3>>& points_cam1,
                                               const std::vector<uint8_t>& has_point1, const SE3& pose1, const FeatureSet& f2,
                                               const std::vector<std::array<double, 3>>& points_cam2, const std::vector<uint8_t>& has_point2,
                                               const SE3& pose2, const std::vector<std::pair<size_t, size_t>>& pairs,
                                               std::vector<std::array<double, 3>>& points_out) {
  const double p1[7] = {pose1.rotation[0], pose1.rotation[1], pose1.rotation[2], pose1.rotation[3], pose1.translation[0], pose1.translation[1], pose1.translation[2]};
  const double p2[7] = {pose2.rotation[0], pose2.rotation[1], pose2.rotation[2], pose2.rotation[3], pose2.translation[0], pose2.translation[1], pose2.translation[2]};
  const int n = (int)pairs.size();
  std::vector<int> pr((size_t)std::max(n, 1) * 2);
  for (int i = 0; i < n; ++i) { pr[2 * (size_t)i] = (int)pairs[(size_t)i].first; pr[2 * (size_t)i + 1] = (int)pairs[(size_t)i].second; }
  std::vector<uint16_t> status((size_t)std::max(n, 1));
  points_out.assign((size_t)std::max(n, 1), std::array<double, 3>{0, 0, 0});
  const orbx_camera cam = camera.c();
  const orbx_triangulation_config cfg = config.c();
  h.check(orbx_triangulate_pairs(h.get(), &cam, &cfg, is_inertial ? 1 : 0, f1.keypoints.data(), points_cam1.empty() ? nullptr : points_cam1[0].data(),
                                 points_cam1.empty() ? nullptr : has_point1.data(), (int)f1.keypoints.size(), p1, f2.keypoints.data(),
                                 points_cam2.empty() ? nullptr : points_cam2[0].data(), points_cam2.empty() ? nullptr : has_point2.data(),
                                 (int)f2.keypoints.size(), p2, pr.data(), n, points_out[0].data(), status.data()));
  status.resize((size_t)n); points_out.resize((size_t)n);
  return status;
}
// triangulate_from_neighbors (:71-308) on device-resident keyframes (orbx_keyframe_create): `neighbours` in the order
// get_neighbor_keyframes returned them.  One library call; the list comes back in the reference's creation order.
inline std::vector<NewMapPoint> triangulate_from_neighbors(Handle& h, const CameraModel& camera, const TriangulationConfig& config, bool is_inertial,
                                                           const orbx_keyframe* current, const std::vector<const orbx_keyframe*>& neighbours,
                                                           TriangulationResult& result) {
  const int T = (int)neighbours.size();
  const orbx_camera cam = camera.c();
  const orbx_triangulation_config cfg = config.c();
  std::vector<int> stats((size_t)std::max(T, 1) * 4), nb, i1, i2;
  std::vector<double> pts;
  int n = 0;
  for (int cap = 1024;; cap = n) {
    nb.assign((size_t)cap, 0); i1.assign((size_t)cap, 0); i2.assign((size_t)cap, 0); pts.assign(3 * (size_t)cap, 0.0);
    h.check(orbx_keyframe_triangulate_from_neighbors(h.get(), &cam, &cfg, is_inertial ? 1 : 0, current, neighbours.data(), T, cap, nb.data(), i1.data(),
                                                     i2.data(), pts.data(), &n, stats.data()));
    if (n <= cap) break;
  }
  result = TriangulationResult{};
  result.num_new_points = (size_t)n; result.num_pairs_checked = (size_t)T;
  for (int t = 0; t < T; ++t) {
    result.num_matches_found += (size_t)stats[4 * (size_t)t + 1]; result.num_triangulated += (size_t)stats[4 * (size_t)t + 2];
    result.num_validated += (size_t)stats[4 * (size_t)t + 3];
  }
  std::vector<NewMapPoint> out((size_t)n);
  for (int i = 0; i < n; ++i)
    out[(size_t)i] = NewMapPoint{(size_t)nb[(size_t)i], (size_t)i1[(size_t)i], (size_t)i2[(size_t)i], {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]}};
  return out;
}

// ---- global bundle adjustment (src/optimizer/global_ba.rs) --------------------------------------------------------
struct GlobalBAConfig {   // global_ba.rs:21-46
  int max_iterations = 10;
  double param_tolerance = 1e-6, gradient_tolerance = 1e-6, huber_threshold = std::sqrt(5.991);
};

struct GlobalBAObservation {   // global_ba.rs:70-80
  KeyFrameId kf_id;
  MapPointId mp_id;
  std::array<double, 2> observed_uv;
};

struct GlobalBAProblemData {   // global_ba.rs:49-67; poses are T_cw
  std::unordered_map<KeyFrameId, SE3> kf_poses;
  std::unordered_map<MapPointId, std::array<double, 3>> mp_positions;
  std::vector<GlobalBAObservation> observations;
  std::vector<KeyFrameId> kf_ids;
  std::vector<MapPointId> mp_ids;
  KeyFrameId fixed_kf_id = 0;
};

struct GlobalBAResult {   // global_ba.rs:83-98; optimized_poses are T_wc and include the fixed keyframe
  std::unordered_map<KeyFrameId, SE3> optimized_poses;
  std::unordered_map<MapPointId, std::array<double, 3>> optimized_points;
  size_t iterations = 0;
  double initial_error = 0, final_error = 0;
};

inline SE3 se3_inverse(const SE3& p) {   // se3.rs:56-63 with nalgebra's quaternion-vector product
  const double w = p.rotation[0], x = -p.rotation[1], y = -p.rotation[2], z = -p.rotation[3];
  const double* v = p.translation.data();
  const double t[3] = {2.0 * (y * v[2] - z * v[1]), 2.0 * (z * v[0] - x * v[2]), 2.0 * (x * v[1] - y * v[0])};
  const double c[3] = {y * t[2] - z * t[1], z * t[0] - x * t[2], x * t[1] - y * t[0]};
  SE3 r;
  r.rotation = {w, x, y, z};
  for (int i = 0; i < 3; ++i) r.translation[i] = -(t[i] * w + c[i] + v[i]);
  return r;
}

struct PnPResult {   // pnp.rs:12-20; pose is T_wc
  SE3 pose;
  std::vector<bool> inlier_mask;
  std::vector<double> reproj_errors;   // +inf where the point is behind the camera
};

// pnp.rs:100-134 (solvePnPRansac with 100 iterations, 8 px, confidence 0.99, then the per-correspondence errors), as the
// specification of orbx_pnp_ransac (orbx.h) states it.  prior: T_wc; required — every reference call site passes Some, and the
// prior-free path is not implemented (std::invalid_argument).  Without a model the prior comes back, as in the reference.
inline PnPResult solve_pnp_ransac_detailed(Handle& h, const std::vector<std::array<double, 3>>& points3d,
                                           const std::vector<std::array<float, 2>>& points2d, const CameraModel& camera,
                                           const std::optional<SE3>& prior) {
  if (!prior) throw std::invalid_argument("solve_pnp_ransac_detailed: a prior pose is required");
  if (points3d.size() != points2d.size()) throw std::invalid_argument("solve_pnp_ransac_detailed: points3d / points2d differ in length");
  const int n = (int)points3d.size();
  const orbx_camera cam = camera.c();
  orbx_pnp_config cfg;
  orbx_default_pnp_config(&cfg);
  const double p7[7] = {prior->rotation[0], prior->rotation[1], prior->rotation[2], prior->rotation[3],
                        prior->translation[0], prior->translation[1], prior->translation[2]};
  double o7[7];
  std::vector<uint8_t> inl(std::max(n, 1));
  PnPResult r;
  r.reproj_errors.resize(n);
  orbx_pnp_result res;
  h.check(orbx_pnp_ransac(h.get(), &cam, &cfg, n, n ? points3d[0].data() : nullptr, n ? points2d[0].data() : nullptr, p7, o7, inl.data(),
                          n ? r.reproj_errors.data() : nullptr, &res));
  r.pose.rotation = {o7[0], o7[1], o7[2], o7[3]};
  r.pose.translation = {o7[4], o7[5], o7[6]};
  r.inlier_mask.assign(inl.begin(), inl.begin() + n);
  return r;
}

// ---- the tracker's per-frame step (orbx_track_frames, orbx.h): project the map points, search the frame's grid, gather, PnP ----
// One frame's input: its features, the map points to look for (positions and descriptors in list order), the pose they are
// projected with and PnP's prior (both T_wc).
struct TrackFrame {
  const FeatureSet* features = nullptr;
  std::vector<std::array<double, 3>> positions;
  std::vector<uint8_t> mp_descriptors;            // positions.size() rows of 32 bytes
  SE3 search_pose, prior;
};

// The tuple track_local_map returns (tracker.rs:981-988) with the arrays behind it.  matched_map_points[feature] = the index of
// the map point in the frame's list (the caller's list holds the ids).  In mode 0 (track_with_motion_model, which returns
// Option<SE3>) the pose is Some exactly when status == ORBX_TRACK_OK or ORBX_TRACK_NO_MODEL.
struct TrackResult {
  SE3 pose;
  size_t n_inliers = 0;                                         // n_correspondences where there were too few (:937-946)
  std::vector<std::optional<size_t>> matched_map_points;        // per feature
  std::vector<double> reproj_errors_full;                       // per correspondence
  std::vector<size_t> inlier_indices, outlier_indices;          // into the correspondences
  std::vector<std::array<double, 3>> points3d;                  // the correspondences, ascending map-point order
  std::vector<std::array<float, 2>> points2d;
  std::vector<int> mp_idx, feat_idx;
  orbx_track_result record{};
  orbx_pnp_result pnp{};
};

// The batch form: one upload, one download.  mode 1 = track_local_map, mode 0 = track_with_motion_model; cfg == nullptr takes
// orbx_default_track_config(mode).
inline std::vector<TrackResult> track_frames(Handle& h, const CameraModel& camera, const std::vector<TrackFrame>& frames, int mode,
                                             const orbx_track_config* cfg = nullptr) {
  const int B = (int)frames.size();
  orbx_track_config tc;
  orbx_default_track_config(mode, &tc);
  if (cfg) tc = *cfg;
  orbx_pnp_config pc;
  orbx_default_pnp_config(&pc);
  std::vector<int> fo(B + 1, 0), mo(B + 1, 0);
  std::vector<KeyPoint> kp;
  std::vector<uint8_t> desc, md;
  std::vector<double> pos, sp, pr;
  for (int b = 0; b < B; ++b) {
    const TrackFrame& f = frames[b];
    if (!f.features || f.features->descriptors.size() != 32 * f.features->keypoints.size() || f.mp_descriptors.size() != 32 * f.positions.size())
      throw std::invalid_argument("track_frames: a frame's descriptors do not match its keypoints / map points");
    kp.insert(kp.end(), f.features->keypoints.begin(), f.features->keypoints.end());
    desc.insert(desc.end(), f.features->descriptors.begin(), f.features->descriptors.end());
    for (const auto& p : f.positions) pos.insert(pos.end(), p.begin(), p.end());
    md.insert(md.end(), f.mp_descriptors.begin(), f.mp_descriptors.end());
    detail::push7(sp, f.search_pose); detail::push7(pr, f.prior);
    fo[b + 1] = (int)kp.size(); mo[b + 1] = (int)(pos.size() / 3);
  }
  const size_t NF = kp.size(), M = pos.size() / 3, Bz = (size_t)std::max(B, 1);
  std::vector<int> off(B + 1, 0), mi(std::max<size_t>(M, 1)), fi(std::max<size_t>(M, 1)), matched(std::max<size_t>(NF, 1));
  std::vector<double> p3(3 * std::max<size_t>(M, 1)), poses(7 * Bz), err(std::max<size_t>(M, 1));
  std::vector<float> p2(2 * std::max<size_t>(M, 1));
  std::vector<uint8_t> inl(std::max<size_t>(M, 1));
  std::vector<orbx_pnp_result> pres(Bz);
  std::vector<orbx_track_result> res(Bz);
  const orbx_camera cam = camera.c();
  h.check(orbx_track_frames(h.get(), &cam, &tc, &pc, B, kp.data(), desc.data(), fo.data(), pos.data(), md.data(), mo.data(), sp.data(), pr.data(),
                            off.data(), p3.data(), p2.data(), mi.data(), fi.data(), poses.data(), inl.data(), err.data(), pres.data(),
                            matched.data(), res.data()));
  std::vector<TrackResult> out(B);
  for (int b = 0; b < B; ++b) {
    TrackResult& r = out[b];
    const double* o7 = &poses[7 * (size_t)b];
    r.pose.rotation = {o7[0], o7[1], o7[2], o7[3]};
    r.pose.translation = {o7[4], o7[5], o7[6]};
    r.record = res[b]; r.pnp = pres[b];
    const bool too_few = res[b].status == ORBX_TRACK_TOO_FEW_CORRESPONDENCES;
    r.n_inliers = too_few ? (size_t)res[b].n_correspondences : (size_t)res[b].n_inliers;
    for (int f = fo[b]; f < fo[b + 1]; ++f)
      r.matched_map_points.push_back(matched[f] >= 0 ? std::optional<size_t>((size_t)matched[f]) : std::nullopt);
    for (int i = off[b]; i < off[b + 1]; ++i) {
      r.points3d.push_back({p3[3 * (size_t)i], p3[3 * (size_t)i + 1], p3[3 * (size_t)i + 2]});
      r.points2d.push_back({p2[2 * (size_t)i], p2[2 * (size_t)i + 1]});
      r.mp_idx.push_back(mi[i]); r.feat_idx.push_back(fi[i]);
      if (too_few) continue;                                    // :937-946: the three vectors stay empty
      r.reproj_errors_full.push_back(err[i]);
      (inl[i] ? r.inlier_indices : r.outlier_indices).push_back((size_t)(i - off[b]));
    }
  }
  return out;
}

// tracker.rs:863-988 on one frame: (pose, n_inliers, matched_map_points, reproj_errors_full, inlier_indices, outlier_indices).
inline TrackResult track_local_map(Handle& h, const CameraModel& camera, const FeatureSet& features,
                                   const std::vector<std::array<double, 3>>& positions, const std::vector<uint8_t>& mp_descriptors,
                                   const SE3& pose, const SE3& imu_prior) {
  return track_frames(h, camera, {TrackFrame{&features, positions, mp_descriptors, pose, imu_prior}}, 1)[0];
}

// tracker.rs:1086-1192 on one frame; the reference's Option<SE3> is Some(result.pose) when result.record.status is ORBX_TRACK_OK
// or ORBX_TRACK_NO_MODEL (fewer than 10 correspondences or inliers: None).
inline TrackResult track_with_motion_model(Handle& h, const CameraModel& camera, const FeatureSet& features,
                                           const std::vector<std::array<double, 3>>& positions, const std::vector<uint8_t>& mp_descriptors,
                                           const SE3& predicted_pose) {
  return track_frames(h, camera, {TrackFrame{&features, positions, mp_descriptors, predicted_pose, predicted_pose}}, 0)[0];
}

// ---- resident map points (orbx_map_points, orbx.h): the store, and the tracker's step with its lists made on the device ----
// A slot is an int in [0, capacity); the caller owns the id -> slot assignment (a HashMap<MapPointId, u32> with a free list).
class MapPointStore {
 public:
  MapPointStore(Handle& h, int capacity) : h_(&h) { h.check(orbx_map_points_create(h.get(), capacity, &mp_)); }
  MapPointStore(const MapPointStore&) = delete;
  MapPointStore& operator=(const MapPointStore&) = delete;
  ~MapPointStore() { if (mp_) orbx_map_points_destroy(mp_); }
  orbx_map_points* get() const { return mp_; }
  // rows into slots; an empty positions / descriptors vector leaves that field as it is (a slot's first set needs both)
  void set(const std::vector<int>& slots, const std::vector<std::array<double, 3>>& positions, const std::vector<uint8_t>& descriptors) {
    if ((!positions.empty() && positions.size() != slots.size()) || (!descriptors.empty() && descriptors.size() != 32 * slots.size()))
      throw std::invalid_argument("MapPointStore::set: one row per slot");
    h_->check(orbx_map_points_set(mp_, slots.data(), (int)slots.size(), positions.empty() ? nullptr : positions[0].data(),
                                  descriptors.empty() ? nullptr : descriptors.data()));
  }
  // the same with the rows in device memory (either may be nullptr), asynchronous on the handle's stream
  void set_device(const std::vector<int>& slots, const double* d_positions, const uint8_t* d_descriptors) {
    h_->check(orbx_map_points_set_device(mp_, slots.data(), (int)slots.size(), d_positions, d_descriptors));
  }
  void erase(const std::vector<int>& slots) { h_->check(orbx_map_points_erase(mp_, slots.data(), (int)slots.size())); }
  void download(const std::vector<int>& slots, std::vector<std::array<double, 3>>& positions, std::vector<uint8_t>& descriptors,
                std::vector<uint8_t>& live) const {
    const size_t n = slots.size();
    positions.resize(n); descriptors.resize(32 * n); live.resize(n);
    h_->check(orbx_map_points_download(mp_, slots.data(), (int)n, n ? positions[0].data() : nullptr, descriptors.data(), live.data()));
  }
  int capacity() const { int c = 0; h_->check(orbx_map_points_info(mp_, &c, nullptr)); return c; }
  int n_live() const { int n = 0; h_->check(orbx_map_points_info(mp_, nullptr, &n)); return n; }

 private:
  Handle* h_;
  orbx_map_points* mp_ = nullptr;
};

// One frame's input: its features, the pose its points are projected with and PnP's prior (both T_wc), and where its map points
// come from: resident keyframes with slot tables (orbx_keyframe_set_map_point_slots), or slots (the previous frame's matched_slot).
struct MapTrackFrame {
  const FeatureSet* features = nullptr;
  std::vector<const orbx_keyframe*> keyframes;
  std::vector<int> slots;
  SE3 search_pose, prior;
};

// TrackResult (mp_idx and matched_map_points index the frame's list) with the list's slots and matched as slots, -1 = none.
struct MapTrackResult : TrackResult {
  std::vector<int> list_slot, matched_slot;
};

// Covisibility of the resident map (orbx_map_covisibility, orbx.h): row q belongs to keyframes[queries[q]]; every index is a
// position in `keyframes`.  best rows are weight descending, then position ascending, -1 padded; n_best[q] entries are not padding.
struct Covisibility {
  int n_kfs = 0, n_best_max = 0;
  std::vector<int> weights;      // [queries][n_kfs]
  std::vector<int> best;         // [queries][n_best_max]
  std::vector<int> n_best;       // [queries]
  int weight(size_t q, size_t k) const { return weights[q * (size_t)n_kfs + k]; }
  // get_best_covisibles (keyframe.rs:313-345) of query q
  std::vector<int> best_of(size_t q) const {
    const int* row = best.data() + q * (size_t)n_best_max;
    return std::vector<int>(row, row + n_best[q]);
  }
};

inline Covisibility map_covisibility(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& queries,
                                     int n_best) {
  Covisibility c;
  c.n_kfs = (int)keyframes.size(); c.n_best_max = std::max(n_best, 0);
  const size_t Q = queries.size();
  c.weights.assign(Q * keyframes.size(), 0); c.best.assign(Q * (size_t)c.n_best_max, -1); c.n_best.assign(Q, 0);
  h.check(orbx_map_covisibility(h.get(), store.get(), c.n_kfs, keyframes.data(), (int)Q, queries.data(), n_best, c.weights.empty() ? nullptr : c.weights.data(),
                                c.best.empty() ? nullptr : c.best.data(), c.n_best.empty() ? nullptr : c.n_best.data()));
  return c;
}

// The local-map form's source: the keyframes the caller considers, per frame the index of its reference keyframe (-1: all of
// them) and the number of best covisibles taken beside it.  local_kf receives, per frame, what was chosen (-1 padded).
struct MapLocalSource {
  const std::vector<const orbx_keyframe*>* keyframes = nullptr;
  const std::vector<int>* ref_kf = nullptr;
  int n_best = 0;
  std::vector<std::vector<int>>* local_kf = nullptr;
};

// The batch form: source = ORBX_MAP_SOURCE_KEYFRAMES or ORBX_MAP_SOURCE_SLOTS for every frame of the call; mode as track_frames.
// With `local` the frames' own keyframes / slots are not read: the lists are chosen on the device (orbx_map_track_local).
inline std::vector<MapTrackResult> map_track_frames(Handle& h, const CameraModel& camera, MapPointStore& store, const std::vector<MapTrackFrame>& frames,
                                                    int source, int mode, const orbx_track_config* cfg = nullptr, const MapLocalSource* local = nullptr) {
  const int B = (int)frames.size();
  std::vector<int> kf_n;                                          // local: every keyframe's feature count
  if (local) {
    if (!local->keyframes || !local->ref_kf || (int)local->ref_kf->size() != B)
      throw std::invalid_argument("map_track_frames: one reference keyframe index per frame");
    for (const orbx_keyframe* k : *local->keyframes) {
      int n = 0;
      h.check(orbx_keyframe_info(k, &n, nullptr, nullptr, nullptr));
      kf_n.push_back(n);
    }
  }
  orbx_track_config tc;
  orbx_default_track_config(mode, &tc);
  if (cfg) tc = *cfg;
  orbx_pnp_config pc;
  orbx_default_pnp_config(&pc);
  const int capacity = store.capacity();
  std::vector<int> fo(B + 1, 0), ko(B + 1, 0), so(B + 1, 0), src;
  std::vector<const orbx_keyframe*> kfs;
  std::vector<KeyPoint> kp;
  std::vector<uint8_t> desc;
  std::vector<double> sp, pr;
  size_t M = 0;                                                   // the lists' host-known bound
  for (int b = 0; b < B; ++b) {
    const MapTrackFrame& f = frames[b];
    if (!f.features || f.features->descriptors.size() != 32 * f.features->keypoints.size())
      throw std::invalid_argument("map_track_frames: a frame's descriptors do not match its keypoints");
    kp.insert(kp.end(), f.features->keypoints.begin(), f.features->keypoints.end());
    desc.insert(desc.end(), f.features->descriptors.begin(), f.features->descriptors.end());
    detail::push7(sp, f.search_pose); detail::push7(pr, f.prior);
    fo[b + 1] = (int)kp.size();
    if (local) {
      // the host-known bound: the reference keyframe's features plus the n_best largest of the others' (all where it is -1)
      const int r = (*local->ref_kf)[b];
      size_t cand = 0;
      if (r < 0 || r >= (int)kf_n.size()) {
        for (int n : kf_n) cand += (size_t)n;
      } else {
        std::vector<int> others(kf_n);
        others.erase(others.begin() + r);
        std::sort(others.begin(), others.end(), std::greater<int>());
        cand = (size_t)kf_n[(size_t)r];
        for (size_t i = 0; i < others.size() && (int)i < local->n_best; ++i) cand += (size_t)others[i];
      }
      M += std::min(cand, (size_t)capacity);
    } else if (source == ORBX_MAP_SOURCE_KEYFRAMES) {
      size_t cand = 0;
      for (const orbx_keyframe* k : f.keyframes) {
        int n = 0;
        h.check(orbx_keyframe_info(k, &n, nullptr, nullptr, nullptr));
        cand += (size_t)n;
        kfs.push_back(k);
      }
      M += std::min(cand, (size_t)capacity);
    } else {
      src.insert(src.end(), f.slots.begin(), f.slots.end());
      M += f.slots.size();
    }
    ko[b + 1] = (int)kfs.size(); so[b + 1] = (int)src.size();
  }
  const size_t NF = kp.size(), Mz = std::max<size_t>(M, 1), Bz = (size_t)std::max(B, 1);
  std::vector<int> lo(B + 1, 0), ls(Mz), off(B + 1, 0), mi(Mz), fi(Mz), matched(std::max<size_t>(NF, 1)), mslot(std::max<size_t>(NF, 1));
  std::vector<double> p3(3 * Mz), poses(7 * Bz), err(Mz);
  std::vector<float> p2(2 * Mz);
  std::vector<uint8_t> inl(Mz);
  std::vector<orbx_pnp_result> pres(Bz);
  std::vector<orbx_track_result> res(Bz);
  const orbx_camera cam = camera.c();
  if (local) {
    const size_t stride = 1 + (size_t)std::max(local->n_best, 0);
    std::vector<int> lk(Bz * stride, -1);
    h.check(orbx_map_track_local(h.get(), &cam, &tc, &pc, store.get(), B, (int)local->keyframes->size(), local->keyframes->data(), local->ref_kf->data(),
                                 local->n_best, kp.data(), desc.data(), fo.data(), sp.data(), pr.data(), (int)M, lk.data(), lo.data(), ls.data(), off.data(),
                                 p3.data(), p2.data(), mi.data(), fi.data(), poses.data(), inl.data(), err.data(), pres.data(), matched.data(), mslot.data(),
                                 res.data()));
    if (local->local_kf) {
      local->local_kf->clear();
      for (int b = 0; b < B; ++b) local->local_kf->emplace_back(lk.begin() + (size_t)b * stride, lk.begin() + ((size_t)b + 1) * stride);
    }
  } else {
    h.check(orbx_map_track_frames(h.get(), &cam, &tc, &pc, store.get(), source, B, kfs.data(), ko.data(), src.data(), so.data(), kp.data(), desc.data(),
                                  fo.data(), sp.data(), pr.data(), (int)M, lo.data(), ls.data(), off.data(), p3.data(), p2.data(), mi.data(), fi.data(),
                                  poses.data(), inl.data(), err.data(), pres.data(), matched.data(), mslot.data(), res.data()));
  }
  std::vector<MapTrackResult> out(B);
  for (int b = 0; b < B; ++b) {
    MapTrackResult& r = out[b];
    const double* o7 = &poses[7 * (size_t)b];
    r.pose.rotation = {o7[0], o7[1], o7[2], o7[3]};
    r.pose.translation = {o7[4], o7[5], o7[6]};
    r.record = res[b]; r.pnp = pres[b];
    const bool too_few = res[b].status == ORBX_TRACK_TOO_FEW_CORRESPONDENCES;
    r.n_inliers = too_few ? (size_t)res[b].n_correspondences : (size_t)res[b].n_inliers;
    r.list_slot.assign(ls.begin() + lo[b], ls.begin() + lo[b + 1]);
    for (int f = fo[b]; f < fo[b + 1]; ++f) {
      r.matched_map_points.push_back(matched[f] >= 0 ? std::optional<size_t>((size_t)matched[f]) : std::nullopt);
      r.matched_slot.push_back(mslot[f]);
    }
    for (int i = off[b]; i < off[b + 1]; ++i) {
      r.points3d.push_back({p3[3 * (size_t)i], p3[3 * (size_t)i + 1], p3[3 * (size_t)i + 2]});
      r.points2d.push_back({p2[2 * (size_t)i], p2[2 * (size_t)i + 1]});
      r.mp_idx.push_back(mi[i]); r.feat_idx.push_back(fi[i]);
      if (too_few) continue;                                    // :937-946: the three vectors stay empty
      r.reproj_errors_full.push_back(err[i]);
      (inl[i] ? r.inlier_indices : r.outlier_indices).push_back((size_t)(i - off[b]));
    }
  }
  return out;
}

// tracker.rs:826-988 on one frame with the local map taken from the store: the distinct live slots of `keyframes` (K1 u K2, chosen
// by the caller) in first-seen order.
inline MapTrackResult track_local_map(Handle& h, const CameraModel& camera, MapPointStore& store, const FeatureSet& features,
                                      const std::vector<const orbx_keyframe*>& keyframes, const SE3& pose, const SE3& imu_prior) {
  return map_track_frames(h, camera, store, {MapTrackFrame{&features, keyframes, {}, pose, imu_prior}}, ORBX_MAP_SOURCE_KEYFRAMES, 1)[0];
}

// tracker.rs:826-988 with K1 u K2 chosen on the device as well (tracker.rs:826-843; map.rs:476-489): `keyframes` are the keyframes the
// caller considers (is_bad ones left out), ref_kf the index of the frame's reference keyframe among them (-1: none, all of them
// are taken), n_best the covisibles taken beside it.  local_kf, when given, receives [ref_kf] ++ best, -1 padded (all -1 for -1).
inline MapTrackResult track_local_map(Handle& h, const CameraModel& camera, MapPointStore& store, const FeatureSet& features,
                                      const std::vector<const orbx_keyframe*>& keyframes, int ref_kf, int n_best, const SE3& pose, const SE3& imu_prior,
                                      std::vector<int>* local_kf = nullptr) {
  const std::vector<int> ref{ref_kf};
  std::vector<std::vector<int>> chosen;
  const MapLocalSource local{&keyframes, &ref, n_best, &chosen};
  MapTrackResult r = map_track_frames(h, camera, store, {MapTrackFrame{&features, {}, {}, pose, imu_prior}}, ORBX_MAP_SOURCE_KEYFRAMES, 1, nullptr, &local)[0];
  if (local_kf) *local_kf = chosen[0];
  return r;
}

// tracker.rs:1086-1192 on one frame: `slots` = the previous frame's matched_slot (-1 entries and slots no longer live are skipped).
inline MapTrackResult track_with_motion_model(Handle& h, const CameraModel& camera, MapPointStore& store, const FeatureSet& features,
                                              const std::vector<int>& slots, const SE3& predicted_pose) {
  return map_track_frames(h, camera, store, {MapTrackFrame{&features, {}, slots, predicted_pose, predicted_pose}}, ORBX_MAP_SOURCE_SLOTS, 0)[0];
}

// ---- local BA from the resident map (orbx.h, "local BA from the resident map"): the window collected on the device ----
// Every keyframe index is a position in the `keyframes` the caller hands over (is_bad ones left out).
struct BAWindow {
  int K = 0, F = 0, M = 0, N = 0;
  std::vector<int> local_kf;                           // [1 + max_covisible], -1 padded: the anchor, then the K optimised keyframes
  std::vector<int> fixed_kf;                           // [F - 1]: the other observers, ascending
  std::vector<int> list_slot;                          // [M]: the window's points as slots; mp_idx is a position here
  std::vector<std::array<double, 3>> positions;        // [M]
  std::vector<orbx_ba_obs32> obs32;                    // [N]
};

// The host-known bounds of a collection call: rows of the point list (the bound of track_local_map's list for the reference
// `cur` with max_covisible neighbours) and of the observations (every feature of `keyframes`).
inline void ba_window_bounds(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, int cur, int max_covisible, int* list_cap,
                             int* obs_cap) {
  std::vector<int> kf_n;
  size_t all = 0;
  for (const orbx_keyframe* k : keyframes) {
    int n = 0;
    h.check(orbx_keyframe_info(k, &n, nullptr, nullptr, nullptr));
    kf_n.push_back(n); all += (size_t)n;
  }
  size_t cand = all;
  if (cur >= 0 && cur < (int)kf_n.size()) {
    std::vector<int> others(kf_n);
    others.erase(others.begin() + cur);
    std::sort(others.begin(), others.end(), std::greater<int>());
    cand = (size_t)kf_n[(size_t)cur];
    for (size_t i = 0; i < others.size() && (int)i < max_covisible; ++i) cand += (size_t)others[i];
  }
  *list_cap = (int)std::min(cand, (size_t)store.capacity());
  *obs_cap = (int)all;
}

// orbx_map_collect_ba_window_device: every output is the caller's device memory (d_counts [4], d_local_kf [1 + max_covisible],
// d_fixed_kf [keyframes.size()], d_list_slot / d_positions [list_cap], d_obs32 [obs_cap], 16-byte aligned); asynchronous.
inline void map_collect_ba_window_device(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, int cur, int max_covisible,
                                         int list_cap, int obs_cap, int* d_counts, int* d_local_kf, int* d_fixed_kf, int* d_list_slot, double* d_positions,
                                         orbx_ba_obs32* d_obs32) {
  h.check(orbx_map_collect_ba_window_device(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), cur, max_covisible, list_cap, obs_cap, d_counts,
                                            d_local_kf, d_fixed_kf, d_list_slot, d_positions, d_obs32));
}

// orbx_map_collect_ba_window: the same into host vectors, synchronous; nullopt where the reference returns None (:813-815, :884-886).
inline std::optional<BAWindow> map_collect_ba_window(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, int cur,
                                                     int max_covisible) {
  int list_cap = 0, obs_cap = 0;
  ba_window_bounds(h, store, keyframes, cur, max_covisible, &list_cap, &obs_cap);
  BAWindow w;
  int counts[4] = {0, 0, 0, 0};
  w.local_kf.assign(1 + (size_t)std::max(max_covisible, 0), -1); w.fixed_kf.assign(std::max<size_t>(keyframes.size(), 1), -1);
  w.list_slot.resize(std::max(list_cap, 1)); w.positions.resize(std::max(list_cap, 1)); w.obs32.resize(std::max(obs_cap, 1));
  const int rc = orbx_map_collect_ba_window(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), cur, max_covisible, list_cap, obs_cap, counts,
                                            w.local_kf.data(), w.fixed_kf.data(), w.list_slot.data(), w.positions[0].data(), w.obs32.data());
  if (rc == ORBX_ERR_EMPTY) return std::nullopt;
  h.check(rc);
  w.K = counts[0]; w.F = counts[1]; w.M = counts[2]; w.N = counts[3];
  w.fixed_kf.resize((size_t)w.F - 1); w.list_slot.resize((size_t)w.M); w.positions.resize((size_t)w.M); w.obs32.resize((size_t)w.N);
  return w;
}

struct BAWindowSolve {
  std::vector<SE3> poses_wc;                           // [K]: the optimised keyframes, T_wc
  size_t iterations = 0;
  double initial_error = 0, final_error = 0;
};

// orbx_ba_solve_visual_obs32_device: solve_visual_ba on flat arrays with the observations in device memory (d_obs32 [n_obs],
// 16-byte aligned, ordered on the handle's stream).  poses_cw [K] / fixed_cw [F] are T_cw; points [M] in/out.
inline std::optional<BAWindowSolve> solve_visual_ba_obs32_device(Handle& h, const CameraModel& camera, const LocalBAConfigLM& config, const std::vector<SE3>& poses_cw,
                                                                 const std::vector<SE3>& fixed_cw, std::vector<std::array<double, 3>>& points,
                                                                 const orbx_ba_obs32* d_obs32, int n_obs, const std::function<bool()>& should_stop) {
  std::vector<double> poses, fixed;
  for (const SE3& p : poses_cw) detail::push7(poses, p);
  for (const SE3& p : fixed_cw) detail::push7(fixed, p);
  const int K = (int)poses_cw.size();
  std::vector<double> out((size_t)std::max(K, 1) * 7);
  int it = 0;
  double e0 = 0, e1 = 0;
  const orbx_camera c = camera.c();
  const orbx_ba_config cfg{config.max_iterations, config.param_tolerance, config.gradient_tolerance, config.huber_threshold, config.max_covisible_keyframes};
  const int rc = orbx_ba_solve_visual_obs32_device(h.get(), &c, &cfg, K, poses.data(), (int)fixed_cw.size(), fixed.data(), (int)points.size(),
                                                   points.empty() ? nullptr : points[0].data(), n_obs, d_obs32, detail::stop_fn(should_stop), detail::stop_user(should_stop), out.data(), &it,
                                                   &e0, &e1);
  if (rc == ORBX_ERR_EMPTY) return std::nullopt;
  h.check(rc);
  BAWindowSolve r;
  for (int i = 0; i < K; ++i) {
    const SE3 p = detail::se3_from7(&out[7 * (size_t)i]);
    r.poses_wc.push_back(p);
  }
  r.iterations = (size_t)it; r.initial_error = e0; r.final_error = e1;
  return r;
}

struct MapLocalBAResult : BAWindowSolve {              // poses_wc[i] belongs to keyframes[local_kf[1 + i]]
  int K = 0, F = 0, M = 0, N = 0;
  std::vector<int> local_kf;                           // [1 + max_covisible_keyframes], -1 padded
};

// orbx_map_local_ba: local_bundle_adjustment's visual branch (local_mapper.rs:377-410) on the resident map — collected on the
// device, solved where the observations lie, the optimised positions written back into the store.  The caller applies the poses
// (orbx_keyframe_set_pose), as it applies ids.  nullopt where the reference returns None.
inline std::optional<MapLocalBAResult> map_local_ba(Handle& h, const CameraModel& camera, const LocalBAConfigLM& config, MapPointStore& store,
                                                    const std::vector<const orbx_keyframe*>& keyframes, int cur, const std::function<bool()>& should_stop) {
  const int mc = config.max_covisible_keyframes;
  MapLocalBAResult r;
  r.local_kf.assign(1 + (size_t)std::max(mc, 0), -1);
  std::vector<double> out((size_t)std::max(mc, 1) * 7);
  int counts[4] = {0, 0, 0, 0}, it = 0;
  double e0 = 0, e1 = 0;
  const orbx_camera c = camera.c();
  const orbx_ba_config cfg{config.max_iterations, config.param_tolerance, config.gradient_tolerance, config.huber_threshold, mc};
  const int rc = orbx_map_local_ba(h.get(), &c, &cfg, store.get(), (int)keyframes.size(), keyframes.data(), cur, detail::stop_fn(should_stop), detail::stop_user(should_stop),
                                   r.local_kf.data(), out.data(), counts, &it, &e0, &e1);
  if (rc == ORBX_ERR_EMPTY) return std::nullopt;
  h.check(rc);
  r.K = counts[0]; r.F = counts[1]; r.M = counts[2]; r.N = counts[3];
  for (int i = 0; i < r.K; ++i) {
    const SE3 p = detail::se3_from7(&out[7 * (size_t)i]);
    r.poses_wc.push_back(p);
  }
  r.iterations = (size_t)it; r.initial_error = e0; r.final_error = e1;
  return r;
}

// ---- observations from the resident map (orbx.h, "observations from the resident map"): lists, refresh, redundancy ----
// mp.observations derived from the slot tables.  Every keyframe index is a position in the `keyframes` the caller hands over
// (is_bad ones left out); slots are live, none twice.
struct MapObservations {
  std::vector<int> obs_start;                          // [M + 1]: point p owns rows [obs_start[p], obs_start[p + 1])
  std::vector<int> obs_kf, obs_feat;                   // the observing keyframes, ascending, and the first feature of each that names the point
  int n_observers(size_t p) const { return obs_start[p + 1] - obs_start[p]; }
  // MapPoint::should_cull's observation half (map_point.rs:140-156; found_ratio is 1.0: nothing increments its counters)
  bool too_few_observers(size_t p, int min_observations) const { return n_observers(p) < min_observations; }
};

// rows obs_kf / obs_feat must hold: every feature of `keyframes`
inline int map_observations_bound(Handle& h, const std::vector<const orbx_keyframe*>& keyframes) {
  size_t all = 0;
  for (const orbx_keyframe* k : keyframes) {
    int n = 0;
    h.check(orbx_keyframe_info(k, &n, nullptr, nullptr, nullptr));
    all += (size_t)n;
  }
  return (int)all;
}

// orbx_map_observations_device: d_obs_start [slots.size() + 1], d_obs_kf / d_obs_feat [obs_cap] are the caller's device memory — the
// arguments of orbx_refresh_map_points_device; asynchronous.
inline void map_observations_device(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& slots, int obs_cap,
                                    int* d_obs_start, int* d_obs_kf, int* d_obs_feat) {
  h.check(orbx_map_observations_device(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)slots.size(), slots.data(), obs_cap, d_obs_start, d_obs_kf,
                                       d_obs_feat));
}

// orbx_map_observations: the same into host vectors cut to their sizes, synchronous.
inline MapObservations map_observations(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& slots) {
  const int cap = map_observations_bound(h, keyframes);
  MapObservations o;
  o.obs_start.assign(slots.size() + 1, 0); o.obs_kf.resize((size_t)std::max(cap, 1)); o.obs_feat.resize((size_t)std::max(cap, 1));
  h.check(orbx_map_observations(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)slots.size(), slots.data(), cap, o.obs_start.data(),
                                o.obs_kf.data(), o.obs_feat.data()));
  o.obs_kf.resize((size_t)o.obs_start.back()); o.obs_feat.resize((size_t)o.obs_start.back());
  return o;
}

// orbx_map_refresh_points: phase 4 of search_in_neighbors (search_in_neighbors.rs:139-150) on the resident map.  normals [M] are
// the points' current normals (the store keeps none); the chosen descriptors are in the result and in the store afterwards.
inline MapPointRefresh map_refresh_points(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& slots,
                                          double scale_range, const std::vector<std::array<double, 3>>& normals) {
  const size_t M = slots.size();
  if (normals.size() != M) throw Error(ORBX_ERR_INVALID, "map_refresh_points: one normal per slot");
  MapPointRefresh r{std::vector<uint8_t>(32 * M), normals, std::vector<double>(M), std::vector<double>(M), std::vector<orbx_mp_refresh_record>(M)};
  h.check(orbx_map_refresh_points(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)M, slots.data(), scale_range, r.mp_descriptors.data(),
                                  M ? r.normals[0].data() : nullptr, r.min_distance.data(), r.max_distance.data(), r.records.data()));
  return r;
}
// orbx_map_refresh_points_device: d_mp_desc [M][32] out, d_normals [M][3] in/out (both 8-byte aligned), d_min_distance /
// d_max_distance [M], d_records [M] are the caller's device memory; asynchronous.
inline void map_refresh_points_device(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& slots,
                                      double scale_range, uint8_t* d_mp_desc, double* d_normals, double* d_min_distance, double* d_max_distance,
                                      orbx_mp_refresh_record* d_records) {
  h.check(orbx_map_refresh_points_device(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)slots.size(), slots.data(), scale_range, d_mp_desc,
                                         d_normals, d_min_distance, d_max_distance, d_records));
}

// cull_keyframes' decision (local_mapper.rs:487-583) for keyframes[candidates[i]]: the caller leaves out the current keyframe,
// roots and bad keyframes, and removes what is culled (IMU preintegration merging, the spanning tree and ids are its own).
struct KeyFrameRedundancy {
  std::vector<int> total, redundant;                   // [candidates]: features with a live point; those whose point has min_observations other observers
  std::vector<uint8_t> cull;                           // redundant / total > threshold
};
inline KeyFrameRedundancy map_keyframe_redundancy(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes,
                                                  const std::vector<int>& candidates, int min_observations = 3, double threshold = 0.9) {
  const size_t n = candidates.size();
  KeyFrameRedundancy r{std::vector<int>(n), std::vector<int>(n), std::vector<uint8_t>(n)};
  h.check(orbx_map_keyframe_redundancy(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)n, candidates.data(), min_observations, threshold,
                                       r.total.data(), r.redundant.data(), r.cull.data()));
  return r;
}
// orbx_map_keyframe_redundancy_device: d_total / d_redundant [candidates.size()] int32 and d_cull [candidates.size()] u8 are the
// caller's device memory; asynchronous.
inline void map_keyframe_redundancy_device(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& candidates,
                                           int min_observations, double threshold, int* d_total, int* d_redundant, uint8_t* d_cull) {
  h.check(orbx_map_keyframe_redundancy_device(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)candidates.size(), candidates.data(),
                                              min_observations, threshold, d_total, d_redundant, d_cull));
}

// ---- fuse and merge on the resident map (orbx.h, "fuse and merge on the resident map"; search_in_neighbors.rs:240-390) ----
// One pass fuse(src, tgt): the distinct live points of keyframes[src[..]] searched in keyframes[tgt[..]]; a match associates or
// merges; the tables of `keyframes` are rewritten where they lie.  The keyframes are not const here.
struct MapFuse {
  int P = 0, matches = 0, added = 0;                   // counts[0..2]; goner.size() is counts[3]
  std::vector<int> list_slot;                          // [P]
  std::vector<int> match;                              // [P][n_tgt]: the matched feature or -1
  std::vector<int> goner, keeper;                      // by ascending goner slot: the caller retires the goners' ids
};

inline int keyframe_features(Handle& h, const orbx_keyframe* k) {
  int n = 0;
  h.check(orbx_keyframe_info(k, &n, nullptr, nullptr, nullptr));
  return n;
}
// (rows of the list, rows of the goner lists) a pass needs: the features of keyframes[src[..]], at most the capacity; that plus the
// targets' features.  Indices out of range count nothing: the library refuses them.
inline std::pair<int, int> map_fuse_bounds(Handle& h, MapPointStore& store, const std::vector<orbx_keyframe*>& keyframes, const std::vector<int>& src,
                                           const std::vector<int>& tgt) {
  auto sum = [&](const std::vector<int>& idx) {
    long long n = 0;
    for (int i : idx)
      if (i >= 0 && (size_t)i < keyframes.size()) n += keyframe_features(h, keyframes[(size_t)i]);
    return n;
  };
  int cap = 0;
  h.check(orbx_map_points_info(store.get(), &cap, nullptr));
  const long long bound = std::min<long long>(sum(src), cap);
  return {(int)bound, (int)(bound + sum(tgt))};
}

// orbx_map_fuse_device: d_counts [4], d_list_slot [list_cap], d_match [list_cap][tgt.size()], d_goner / d_keeper [the second of
// map_fuse_bounds] are the caller's device memory; asynchronous; the store's live bytes are untouched.
inline void map_fuse_device(Handle& h, const CameraModel& camera, MapPointStore& store, const std::vector<orbx_keyframe*>& keyframes, const std::vector<int>& src,
                            const std::vector<int>& tgt, double radius_scale, unsigned desc_threshold, int list_cap, int* d_counts, int* d_list_slot, int* d_match,
                            int* d_goner, int* d_keeper) {
  const orbx_camera c = camera.c();
  h.check(orbx_map_fuse_device(h.get(), &c, store.get(), (int)keyframes.size(), keyframes.data(), (int)src.size(), src.data(), (int)tgt.size(), tgt.data(), radius_scale,
                               desc_threshold, list_cap, d_counts, d_list_slot, d_match, d_goner, d_keeper));
}

// orbx_map_fuse: the same into host vectors cut to their sizes, synchronous; the goners are erased from the store.
inline MapFuse map_fuse(Handle& h, const CameraModel& camera, MapPointStore& store, const std::vector<orbx_keyframe*>& keyframes, const std::vector<int>& src,
                        const std::vector<int>& tgt, double radius_scale, unsigned desc_threshold = 50) {
  const auto [cap, gcap] = map_fuse_bounds(h, store, keyframes, src, tgt);
  const size_t T = tgt.size();
  MapFuse r;
  int counts[4] = {0, 0, 0, 0};
  r.list_slot.resize((size_t)std::max(cap, 1)); r.match.resize((size_t)std::max(cap, 1) * std::max<size_t>(T, 1));
  r.goner.resize((size_t)std::max(gcap, 1)); r.keeper.resize((size_t)std::max(gcap, 1));
  const orbx_camera c = camera.c();
  h.check(orbx_map_fuse(h.get(), &c, store.get(), (int)keyframes.size(), keyframes.data(), (int)src.size(), src.data(), (int)T, tgt.data(), radius_scale, desc_threshold,
                        cap, counts, r.list_slot.data(), r.match.data(), r.goner.data(), r.keeper.data()));
  r.P = counts[0]; r.matches = counts[1]; r.added = counts[2];
  r.list_slot.resize((size_t)r.P); r.match.resize((size_t)r.P * T); r.goner.resize((size_t)counts[3]); r.keeper.resize((size_t)counts[3]);
  return r;
}

// orbx_map_search_in_neighbors: phases 2 to 4 of search_in_neighbors for keyframes[cur] and keyframes[neighbours[..]] (choosing them
// stays with the caller): fuse([cur], neighbours), fuse(neighbours, [cur]), one download, the goners erased, map_refresh_points on
// the affected list.  slot_normals: every slot's normal before the call, [capacity], or empty for zeros (the store keeps none).
struct MapSearchInNeighbors {
  int counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};            // pass A's {P, matches, added, goners}, then pass B's
  std::vector<int> goner_a, keeper_a, goner_b, keeper_b;
  std::vector<int> affected;                           // the distinct live slots of [cur] ++ neighbours afterwards, first seen first
  MapPointRefresh refresh;                             // in the affected list's order
  size_t num_fused() const { return goner_a.size() + goner_b.size(); }                       // SearchInNeighborsResult (search_in_neighbors.rs:43-50)
  size_t num_observations_added() const { return (size_t)counts[2] + (size_t)counts[6]; }
};
inline MapSearchInNeighbors map_search_in_neighbors(Handle& h, const CameraModel& camera, MapPointStore& store, const std::vector<orbx_keyframe*>& keyframes, int cur,
                                                    const std::vector<int>& neighbours, double radius_scale, double scale_range,
                                                    const std::vector<std::array<double, 3>>& slot_normals = {}, unsigned desc_threshold = 50) {
  int capacity = 0;
  h.check(orbx_map_points_info(store.get(), &capacity, nullptr));
  if (!slot_normals.empty() && slot_normals.size() != (size_t)capacity) throw Error(ORBX_ERR_INVALID, "map_search_in_neighbors: one normal per slot of the store");
  long long f_cur = 0, f_nb = 0;
  if (cur >= 0 && (size_t)cur < keyframes.size()) f_cur = keyframe_features(h, keyframes[(size_t)cur]);
  for (int i : neighbours)
    if (i >= 0 && (size_t)i < keyframes.size()) f_nb += keyframe_features(h, keyframes[(size_t)i]);
  const long long cap = capacity;
  const size_t gcap = (size_t)std::max<long long>(std::max(std::min(f_cur, cap) + f_nb, std::min(f_nb, cap) + f_cur), 1);
  const size_t acap = (size_t)std::max<long long>(std::min(f_cur + f_nb, cap), 1);
  MapSearchInNeighbors r;
  r.goner_a.resize(gcap); r.keeper_a.resize(gcap); r.goner_b.resize(gcap); r.keeper_b.resize(gcap); r.affected.resize(acap);
  r.refresh = MapPointRefresh{std::vector<uint8_t>(32 * acap), std::vector<std::array<double, 3>>(acap), std::vector<double>(acap), std::vector<double>(acap),
                              std::vector<orbx_mp_refresh_record>(acap)};
  int M = 0;
  const orbx_camera c = camera.c();
  h.check(orbx_map_search_in_neighbors(h.get(), &c, store.get(), (int)keyframes.size(), keyframes.data(), cur, (int)neighbours.size(), neighbours.data(), radius_scale,
                                       desc_threshold, scale_range, slot_normals.empty() ? nullptr : slot_normals[0].data(), (int)gcap, (int)acap, r.counts,
                                       r.goner_a.data(), r.keeper_a.data(), r.goner_b.data(), r.keeper_b.data(), &M, r.affected.data(), r.refresh.mp_descriptors.data(),
                                       r.refresh.normals[0].data(), r.refresh.min_distance.data(), r.refresh.max_distance.data(), r.refresh.records.data()));
  r.goner_a.resize((size_t)r.counts[3]); r.keeper_a.resize((size_t)r.counts[3]); r.goner_b.resize((size_t)r.counts[7]); r.keeper_b.resize((size_t)r.counts[7]);
  r.affected.resize((size_t)M);
  r.refresh.mp_descriptors.resize(32 * (size_t)M); r.refresh.normals.resize((size_t)M); r.refresh.min_distance.resize((size_t)M);
  r.refresh.max_distance.resize((size_t)M); r.refresh.records.resize((size_t)M);
  return r;
}

// orbx_keyframe_get_map_point_slots: the table as it lies in device memory (-1 everywhere without one): what the caller applies to its ids
inline std::vector<int> keyframe_map_point_slots(Handle& h, const orbx_keyframe* kf) {
  std::vector<int> slots((size_t)std::max(keyframe_features(h, kf), 1), -1);
  h.check(orbx_keyframe_get_map_point_slots(kf, slots.data()));
  slots.resize((size_t)keyframe_features(h, kf));
  return slots;
}

// ---- create and cull map points on the resident map (orbx.h, "create and cull map points on the resident map") ----
// orbx_keyframe_set_map_point_slots_device: the table from a device array [n] (the tracker's matched_slot row); asynchronous
inline void keyframe_set_map_point_slots_device(Handle& h, orbx_keyframe* kf, MapPointStore& store, const int* d_slots) {
  h.check(orbx_keyframe_set_map_point_slots_device(kf, store.get(), d_slots));
}

// Steps 3 and 3b of process_keyframe: the stereo points of `current` and the points triangulated with `neighbours` take free_slots
// in creation order and are written into the keyframes' tables where they lie.
struct MapCreatedPoints {
  int n_stereo = 0, n_pairs = 0, dropped = 0;           // counts[0], counts[1], counts[3]; new_slot.size() is counts[2]
  std::vector<int> new_slot, new_neighbour, new_idx1, new_idx2;        // in creation order; a stereo point has neighbour -1 and idx2 -1
  std::vector<std::array<double, 3>> new_points;
  std::vector<int> stats;                               // [T][4]: searched, matches_found, triangulated, validated
};

// orbx_map_create_points_device: every output is the caller's device memory (lists of free_slots.size() rows, d_new_desc 16-byte
// aligned); asynchronous; the store is untouched until the caller's set_device for the first counts[2] slots.
inline void map_create_points_device(Handle& h, const CameraModel& camera, const TriangulationConfig& config, bool is_inertial, MapPointStore& store,
                                     orbx_keyframe* current, const std::vector<orbx_keyframe*>& neighbours, int phases, const std::vector<int>& free_slots,
                                     int* d_counts, int* d_new_slot, int* d_new_neighbour, int* d_new_idx1, int* d_new_idx2, double* d_new_points,
                                     uint8_t* d_new_desc, int* d_stats) {
  const orbx_camera c = camera.c();
  const orbx_triangulation_config cfg = config.c();
  h.check(orbx_map_create_points_device(h.get(), &c, &cfg, is_inertial ? 1 : 0, store.get(), current, neighbours.data(), (int)neighbours.size(), phases,
                                        free_slots.data(), (int)free_slots.size(), d_counts, d_new_slot, d_new_neighbour, d_new_idx1, d_new_idx2, d_new_points,
                                        d_new_desc, d_stats));
}

// orbx_map_create_points: the same into host vectors cut to `created`, synchronous; the new points are live in the store afterwards.
inline MapCreatedPoints map_create_points(Handle& h, const CameraModel& camera, const TriangulationConfig& config, bool is_inertial, MapPointStore& store,
                                          orbx_keyframe* current, const std::vector<orbx_keyframe*>& neighbours, const std::vector<int>& free_slots,
                                          int phases = ORBX_MAP_CREATE_STEREO | ORBX_MAP_CREATE_NEIGHBOURS) {
  const size_t nf = std::max<size_t>(free_slots.size(), 1), T = neighbours.size();
  MapCreatedPoints r;
  int counts[4] = {0, 0, 0, 0};
  r.new_slot.resize(nf); r.new_neighbour.resize(nf); r.new_idx1.resize(nf); r.new_idx2.resize(nf); r.new_points.resize(nf); r.stats.resize(4 * std::max<size_t>(T, 1));
  const orbx_camera c = camera.c();
  const orbx_triangulation_config cfg = config.c();
  h.check(orbx_map_create_points(h.get(), &c, &cfg, is_inertial ? 1 : 0, store.get(), current, neighbours.data(), (int)T, phases, free_slots.data(),
                                 (int)free_slots.size(), counts, r.new_slot.data(), r.new_neighbour.data(), r.new_idx1.data(), r.new_idx2.data(),
                                 r.new_points[0].data(), r.stats.data()));
  r.n_stereo = counts[0]; r.n_pairs = counts[1]; r.dropped = counts[3];
  const size_t m = (size_t)counts[2];
  r.new_slot.resize(m); r.new_neighbour.resize(m); r.new_idx1.resize(m); r.new_idx2.resize(m); r.new_points.resize(m); r.stats.resize(4 * T);
  return r;
}

// orbx_map_remove_points (remove_map_point_full for a list): every entry of the tables of `keyframes` that names a listed slot
// becomes -1, then the slots are erased.  Returns the table entries cleared; count = false: no download, no wait, -1.
inline int map_remove_points(Handle& h, MapPointStore& store, const std::vector<orbx_keyframe*>& keyframes, const std::vector<int>& slots, bool count = true) {
  int n = -1;
  h.check(orbx_map_remove_points(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)slots.size(), slots.data(), count ? &n : nullptr));
  return n;
}

// orbx_map_cull_points (cull_map_points): the candidates observed by fewer than min_observations of `keyframes`, in their order,
// removed as map_remove_points removes them.  The grace period and is_bad are the caller's, through its choice of candidates.
inline std::vector<int> map_cull_points(Handle& h, MapPointStore& store, const std::vector<orbx_keyframe*>& keyframes, const std::vector<int>& candidates,
                                        int min_observations) {
  std::vector<int> culled(std::max<size_t>(candidates.size(), 1));
  int n = 0;
  h.check(orbx_map_cull_points(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)candidates.size(), candidates.data(), min_observations, &n,
                               culled.data()));
  culled.resize((size_t)n);
  return culled;
}

// ---- track_with_reference_kf (orbx_track_reference, orbx.h): cross-checked matching against the reference keyframe, gather, PnP ----
// One frame's input: its features, its reference keyframe's descriptors and, per keyframe feature, the map point's position and a
// validity byte (1: kf.get_map_point(i) is Some and the map still holds that point, tracker.rs:1024-1036), and PnP's prior (T_wc).
struct TrackReferenceFrame {
  const FeatureSet* features = nullptr;
  const std::vector<uint8_t>* kf_descriptors = nullptr;   // kf_positions.size() rows of 32 bytes
  std::vector<std::array<double, 3>> kf_positions;
  std::vector<uint8_t> kf_valid;
  SE3 prior;
};

struct TrackReferenceResult {
  SE3 pose;                                                     // the prior where there were too few correspondences or no model
  std::vector<DMatch> matches;                                  // every mutual match: query = keyframe feature, train = frame feature
  std::vector<std::array<double, 3>> points3d;                  // the correspondences, ascending keyframe-feature index
  std::vector<std::array<float, 2>> points2d;
  std::vector<int> kf_idx, feat_idx;
  std::vector<double> reproj_errors;                            // per correspondence
  std::vector<bool> inlier_mask;
  orbx_track_ref_result record{};
  orbx_pnp_result pnp{};
  // the reference's Option<SE3> (:1051-1063)
  std::optional<SE3> pose_or_none() const {
    return record.status == ORBX_TRACK_OK || record.status == ORBX_TRACK_NO_MODEL ? std::optional<SE3>(pose) : std::nullopt;
  }
};

// The batch form: one upload, one download.  min_correspondences below 4 throws orbx::Error (ORBX_ERR_INVALID).
inline std::vector<TrackReferenceResult> track_reference(Handle& h, const CameraModel& camera, const std::vector<TrackReferenceFrame>& frames,
                                                         int min_correspondences = 4) {
  const int B = (int)frames.size();
  orbx_pnp_config pc;
  orbx_default_pnp_config(&pc);
  std::vector<int> fo(B + 1, 0), ko(B + 1, 0);
  std::vector<KeyPoint> kp;
  std::vector<uint8_t> desc, kd, valid;
  std::vector<double> pos, pr;
  for (int b = 0; b < B; ++b) {
    const TrackReferenceFrame& f = frames[b];
    if (!f.features || !f.kf_descriptors || f.features->descriptors.size() != 32 * f.features->keypoints.size() ||
        f.kf_descriptors->size() != 32 * f.kf_positions.size() || f.kf_valid.size() != f.kf_positions.size())
      throw std::invalid_argument("track_reference: a frame's descriptors / positions / valid do not match in length");
    kp.insert(kp.end(), f.features->keypoints.begin(), f.features->keypoints.end());
    desc.insert(desc.end(), f.features->descriptors.begin(), f.features->descriptors.end());
    kd.insert(kd.end(), f.kf_descriptors->begin(), f.kf_descriptors->end());
    for (const auto& p : f.kf_positions) pos.insert(pos.end(), p.begin(), p.end());
    valid.insert(valid.end(), f.kf_valid.begin(), f.kf_valid.end());
    pr.insert(pr.end(), f.prior.rotation.begin(), f.prior.rotation.end());
    pr.insert(pr.end(), f.prior.translation.begin(), f.prior.translation.end());
    fo[b + 1] = (int)kp.size(); ko[b + 1] = (int)valid.size();
  }
  const size_t K = valid.size(), Kz = std::max<size_t>(K, 1), Bz = (size_t)std::max(B, 1);
  std::vector<DMatch> ma(Kz);
  std::vector<int> off(B + 1, 0), ki(Kz), fi(Kz);
  std::vector<double> p3(3 * Kz), poses(7 * Bz), err(Kz);
  std::vector<float> p2(2 * Kz);
  std::vector<uint8_t> inl(Kz);
  std::vector<orbx_pnp_result> pres(Bz);
  std::vector<orbx_track_ref_result> res(Bz);
  const orbx_camera cam = camera.c();
  h.check(orbx_track_reference(h.get(), &cam, &pc, min_correspondences, B, kp.data(), desc.data(), fo.data(), kd.data(), pos.data(), valid.data(),
                               ko.data(), pr.data(), ma.data(), off.data(), p3.data(), p2.data(), ki.data(), fi.data(), poses.data(), inl.data(),
                               err.data(), pres.data(), res.data()));
  std::vector<TrackReferenceResult> out(B);
  for (int b = 0; b < B; ++b) {
    TrackReferenceResult& r = out[b];
    const double* o7 = &poses[7 * (size_t)b];
    r.pose.rotation = {o7[0], o7[1], o7[2], o7[3]};
    r.pose.translation = {o7[4], o7[5], o7[6]};
    r.record = res[b]; r.pnp = pres[b];
    r.matches.assign(ma.begin() + ko[b], ma.begin() + ko[b] + res[b].n_matches);
    for (int i = off[b]; i < off[b + 1]; ++i) {
      r.points3d.push_back({p3[3 * (size_t)i], p3[3 * (size_t)i + 1], p3[3 * (size_t)i + 2]});
      r.points2d.push_back({p2[2 * (size_t)i], p2[2 * (size_t)i + 1]});
      r.kf_idx.push_back(ki[i]); r.feat_idx.push_back(fi[i]);
      r.reproj_errors.push_back(err[i]); r.inlier_mask.push_back(inl[i] != 0);
    }
  }
  return out;
}

// tracker.rs:992-1064 on one frame: Some(pose), or None with fewer than 4 correspondences.
inline std::optional<SE3> track_with_reference_kf(Handle& h, const CameraModel& camera, const FeatureSet& frame,
                                                  const std::vector<uint8_t>& kf_descriptors,
                                                  const std::vector<std::array<double, 3>>& kf_positions, const std::vector<uint8_t>& kf_valid,
                                                  const SE3& pose) {
  return track_reference(h, camera, {TrackReferenceFrame{&frame, &kf_descriptors, kf_positions, kf_valid, pose}})[0].pose_or_none();
}

// ---- loop-candidate verification (orbx_verify_loop_candidates, orbx_sim3_ransac_batch; corrector.rs:116-204, sim3_solver.rs) ----
// sim3_solver.rs:13-36 and the sampler's seed; probability is carried and has no effect, as in the reference
struct Sim3SolverConfig {
  size_t max_iterations = 300;
  double inlier_threshold = 0.075;
  size_t min_inliers = 15;
  bool fix_scale = true;
  double probability = 0.99;
  uint64_t seed = 0;
  orbx_sim3_config c() const {
    orbx_sim3_config o;
    o.max_iterations = (int)max_iterations; o.inlier_threshold = inlier_threshold; o.min_inliers = (int)min_inliers;
    o.fix_scale = fix_scale ? 1 : 0; o.probability = probability; o.seed = seed;
    return o;
  }
};
// geometry/sim3.rs:16-21: p' = scale * (rotation * p) + translation; rotation (w, x, y, z) with w >= 0
struct Sim3 {
  std::array<double, 4> rotation{1.0, 0.0, 0.0, 0.0};
  std::array<double, 3> translation{0.0, 0.0, 0.0};
  double scale = 1.0;
};
// sim3_solver.rs:39-49
struct Sim3Result {
  Sim3 sim3;
  std::vector<size_t> inliers;
  size_t num_inliers = 0;
  double mse = 0.0;
  orbx_sim3_result record{};
};

// sim3_solver.rs:63-145: the Sim3 S with points2 ~ S points1, or nullopt where the reference returns None
inline std::optional<Sim3Result> compute_sim3_ransac(Handle& h, const std::vector<std::array<double, 3>>& points1,
                                                     const std::vector<std::array<double, 3>>& points2, const Sim3SolverConfig& config) {
  if (points1.size() != points2.size()) return std::nullopt;                       // :69
  const int n = (int)points1.size();
  const int off[2] = {0, n};
  const orbx_sim3_config c = config.c();
  double s8[8];
  std::vector<uint8_t> inl((size_t)std::max(n, 1));
  orbx_sim3_result rec{};
  h.check(orbx_sim3_ransac_batch(h.get(), &c, 1, off, n ? points1[0].data() : nullptr, n ? points2[0].data() : nullptr, s8, inl.data(), &rec));
  if (rec.status != ORBX_SIM3_OK) return std::nullopt;
  Sim3Result r;
  r.sim3.rotation = {s8[0], s8[1], s8[2], s8[3]}; r.sim3.translation = {s8[4], s8[5], s8[6]}; r.sim3.scale = s8[7];
  for (int i = 0; i < n; ++i) if (inl[(size_t)i]) r.inliers.push_back((size_t)i);
  r.num_inliers = (size_t)rec.n_inliers; r.mse = rec.mse; r.record = rec;
  return r;
}
// sim3_solver.rs:318-328
inline std::optional<Sim3Result> compute_sim3_from_matches(Handle& h, const std::vector<std::array<double, 3>>& points1,
                                                           const std::vector<std::array<double, 3>>& points2, bool fix_scale) {
  Sim3SolverConfig c;
  c.fix_scale = fix_scale;
  return compute_sim3_ransac(h, points1, points2, c);
}

// What verify_loop_candidate reads of a keyframe (atlas/map.rs KeyFrame): features, stereo points (points_cam with has_point = Some),
// pose, the FeatureVector as one node id per feature (empty: none) and the map-point ids (-1 = None; empty: none)
struct LoopKeyFrame {
  const FeatureSet* features = nullptr;
  std::vector<std::array<double, 3>> points_cam;
  std::vector<uint8_t> has_point;
  SE3 pose;
  std::vector<uint32_t> feature_nodes;
  std::vector<int64_t> map_points;
};
// corrector.rs:33-45
struct VerifiedLoop {
  uint64_t current_kf_id = 0, loop_kf_id = 0;
  Sim3 sim3_current_to_loop;
  std::vector<std::pair<int64_t, int64_t>> matched_map_points;
  std::vector<std::pair<size_t, size_t>> feature_matches;
  std::vector<DMatch> matches;                                  // every ratio-test match, with or without stereo points
  std::vector<bool> inlier_mask;                                // Sim3's mask over feature_matches
  orbx_loop_verify_result record{};
};

// corrector.rs:116-204 for one candidate: the record is always written to *record_out when given; nullopt where the reference
// returns None.  Both keyframes with feature_nodes: the FeatureVector matcher, else brute force.
inline std::optional<VerifiedLoop> verify_loop_candidate(Handle& h, const CameraModel& camera, const LoopKeyFrame& current, const LoopKeyFrame& loop,
                                                         uint64_t current_kf_id = 0, uint64_t loop_kf_id = 0,
                                                         const orbx_loop_verify_config* config = nullptr, VerifiedLoop* all_out = nullptr) {
  if (!current.features || !loop.features) throw std::invalid_argument("verify_loop_candidate: a keyframe without features");
  const size_t n1 = current.features->keypoints.size(), n2 = loop.features->keypoints.size();
  if (current.features->descriptors.size() != 32 * n1 || loop.features->descriptors.size() != 32 * n2 || current.points_cam.size() != n1 ||
      current.has_point.size() != n1 || loop.points_cam.size() != n2 || loop.has_point.size() != n2 ||
      (!current.feature_nodes.empty() && current.feature_nodes.size() != n1) || (!loop.feature_nodes.empty() && loop.feature_nodes.size() != n2))
    throw std::invalid_argument("verify_loop_candidate: a keyframe's arrays do not match in length");
  orbx_loop_verify_config cfg;
  if (config) cfg = *config; else orbx_default_loop_verify_config(&cfg);
  const bool fv = !current.feature_nodes.empty() && !loop.feature_nodes.empty();
  const int co[2] = {0, (int)n1}, lo[2] = {0, (int)n2};
  double cp[7], lp[7], s8[8];
  for (int k = 0; k < 4; ++k) { cp[k] = current.pose.rotation[k]; lp[k] = loop.pose.rotation[k]; }
  for (int k = 0; k < 3; ++k) { cp[4 + k] = current.pose.translation[k]; lp[4 + k] = loop.pose.translation[k]; }
  const size_t nz = std::max<size_t>(n1, 1);
  std::vector<DMatch> ma(nz);
  std::vector<int> fm(2 * nz);
  std::vector<double> pc(3 * nz), pl(3 * nz);
  std::vector<uint8_t> inl(nz);
  orbx_loop_verify_result rec{};
  const orbx_camera cam = camera.c();
  h.check(orbx_verify_loop_candidates(h.get(), &cam, &cfg, 1, current.features->descriptors.data(), n1 ? current.points_cam[0].data() : nullptr,
                                      current.has_point.data(), fv ? current.feature_nodes.data() : nullptr, co, cp, loop.features->keypoints.data(),
                                      loop.features->descriptors.data(), n2 ? loop.points_cam[0].data() : nullptr, loop.has_point.data(),
                                      fv ? loop.feature_nodes.data() : nullptr, lo, lp, ma.data(), fm.data(), pc.data(), pl.data(), inl.data(), s8,
                                      &rec));
  VerifiedLoop v;
  v.current_kf_id = current_kf_id; v.loop_kf_id = loop_kf_id; v.record = rec;
  v.sim3_current_to_loop.rotation = {s8[0], s8[1], s8[2], s8[3]}; v.sim3_current_to_loop.translation = {s8[4], s8[5], s8[6]};
  v.sim3_current_to_loop.scale = s8[7];
  v.matches.assign(ma.begin(), ma.begin() + rec.n_matches);
  for (int k = 0; k < rec.n_pairs; ++k) {
    const size_t i = (size_t)fm[2 * (size_t)k], j = (size_t)fm[2 * (size_t)k + 1];
    v.feature_matches.emplace_back(i, j);
    v.inlier_mask.push_back(inl[(size_t)k] != 0);
    if (!current.map_points.empty() && !loop.map_points.empty() && current.map_points[i] >= 0 && loop.map_points[j] >= 0)   // :168-173
      v.matched_map_points.emplace_back(current.map_points[i], loop.map_points[j]);
  }
  if (all_out) *all_out = v;
  return rec.status == ORBX_LOOP_OK ? std::optional<VerifiedLoop>(v) : std::nullopt;
}

// global_ba.rs:184-418.  The id -> index re-keying is the reference's own (:198-229).  Observations of a map point
// that is not in mp_ids are rejected (collect_global_ba_data never emits one, :160).
// whole_map: through orbx_ba_solve_global_map, the path that takes more than 128 optimised keyframes (solve_global_ba_map below).
inline std::optional<GlobalBAResult> solve_global_ba(Handle& h, const GlobalBAProblemData& problem, const CameraModel& camera,
                                                     const GlobalBAConfig& config, const std::function<bool()>& should_stop, bool whole_map = false) {
  const size_t n_kfs = problem.kf_ids.size(), n_mps = problem.mp_ids.size();
  if (n_kfs < 2 || n_mps == 0) return std::nullopt;                      // :194-196
  size_t fixed_pos = n_kfs;
  for (size_t i = 0; i < n_kfs; ++i) if (problem.kf_ids[i] == problem.fixed_kf_id) { fixed_pos = i; break; }
  if (fixed_pos == n_kfs) return std::nullopt;                           // :199-202
  std::unordered_map<KeyFrameId, int> kf_to_param;
  std::vector<KeyFrameId> opt_ids;
  for (size_t i = 0; i < n_kfs; ++i) if (i != fixed_pos) { kf_to_param[problem.kf_ids[i]] = (int)opt_ids.size(); opt_ids.push_back(problem.kf_ids[i]); }
  std::unordered_map<MapPointId, int> mp_to_param;
  for (size_t i = 0; i < n_mps; ++i) mp_to_param[problem.mp_ids[i]] = (int)i;
  std::vector<double> poses, fixed, points;
  for (KeyFrameId id : opt_ids) { auto it = problem.kf_poses.find(id); detail::push7(poses, it != problem.kf_poses.end() ? it->second : SE3{}); }   // :232-243
  auto fit = problem.kf_poses.find(problem.fixed_kf_id);
  const SE3 fixed_pose = fit != problem.kf_poses.end() ? fit->second : SE3{};                                                             // :256-261
  detail::push7(fixed, fixed_pose);
  for (MapPointId id : problem.mp_ids) {
    auto it = problem.mp_positions.find(id);
    const std::array<double, 3> p = it != problem.mp_positions.end() ? it->second : std::array<double, 3>{0, 0, 0};
    points.insert(points.end(), p.begin(), p.end());
  }
  std::vector<orbx_ba_obs> obs;
  for (const GlobalBAObservation& o : problem.observations) {
    auto m = mp_to_param.find(o.mp_id);
    if (m == mp_to_param.end()) throw Error(ORBX_ERR_INVALID, "solve_global_ba: observation of a map point that is not in mp_ids");
    orbx_ba_obs b{};
    b.mp_idx = m->second; b.u = o.observed_uv[0]; b.v = o.observed_uv[1];
    auto k = kf_to_param.find(o.kf_id);
    if (o.kf_id == problem.fixed_kf_id) { b.kf_idx = -1; b.fixed_idx = 0; }            // :639-641
    else if (k != kf_to_param.end()) { b.kf_idx = k->second; b.fixed_idx = -1; }
    else { b.kf_idx = -1; b.fixed_idx = -1; }                                          // :649 identity
    obs.push_back(b);
  }
  const int K = (int)opt_ids.size(), M = (int)n_mps;
  std::vector<double> out((size_t)K * 7);
  int it = 0;
  double e0 = 0, e1 = 0;
  const orbx_camera c = camera.c();
  const orbx_ba_config cfg{config.max_iterations, config.param_tolerance, config.gradient_tolerance, config.huber_threshold, 0};
  const int rc = (whole_map ? orbx_ba_solve_global_map : orbx_ba_solve_global)(h.get(), &c, &cfg, K, poses.data(), fixed.data(), M, points.data(), (int)obs.size(),
                                                                              obs.data(), detail::stop_fn(should_stop), detail::stop_user(should_stop), out.data(),
                                                                              &it, &e0, &e1);
  if (rc != ORBX_OK) return std::nullopt;
  GlobalBAResult r;
  r.optimized_poses[problem.fixed_kf_id] = se3_inverse(fixed_pose);      // :386
  for (int i = 0; i < K; ++i) {
    const SE3 p = detail::se3_from7(&out[7 * (size_t)i]);
    r.optimized_poses[opt_ids[(size_t)i]] = p;
  }
  for (int j = 0; j < M; ++j) r.optimized_points[problem.mp_ids[(size_t)j]] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
  r.iterations = (size_t)it; r.initial_error = e0; r.final_error = e1;
  return r;
}

// solve_global_ba for a whole map (orbx_ba_solve_global_map): the same problem, result and semantics for up to
// orbx_ba_global_map_max_keyframes() optimised keyframes; a larger map answers nullopt as any refused solve does.
inline std::optional<GlobalBAResult> solve_global_ba_map(Handle& h, const GlobalBAProblemData& problem, const CameraModel& camera,
                                                         const GlobalBAConfig& config, const std::function<bool()>& should_stop) {
  return solve_global_ba(h, problem, camera, config, should_stop, true);
}


// ---- local inertial bundle adjustment (src/optimizer/local_inertial_ba.rs) -----------------------------------------
struct ImuBias { std::array<double, 3> gyro{0, 0, 0}, accel{0, 0, 0}; };   // imu/types.rs

struct PreintegratedState {   // imu/preintegration.rs:85-98, the fields the residual reads (imu_factors.rs:66-103)
  std::array<double, 4> delta_rot{1, 0, 0, 0};
  std::array<double, 3> delta_vel{0, 0, 0}, delta_pos{0, 0, 0};
  double dt = 0.0;
};

struct LocalInertialBAConfig {   // local_inertial_ba.rs:109-141
  int max_iterations = 10, window_size = 10;
  double huber_threshold_mono = std::sqrt(5.991), huber_threshold_stereo = std::sqrt(7.815), initial_lambda = 1e-2;
  double gyro_rw_info = 1e6, accel_rw_info = 1e4;
};

struct InertialVisualObs {   // :64-77
  KeyFrameId kf_id;
  MapPointId mp_id;
  std::array<double, 2> observed_uv;
  bool is_stereo, is_kf_in_window;
};

struct ImuEdgeData {   // :79-88
  KeyFrameId kf_i_id, kf_j_id;
  PreintegratedState preint;
};

struct InertialBAProblemData {   // :40-62; kf_poses T_wc, fixed_kf_poses T_cw
  std::unordered_map<KeyFrameId, SE3> kf_poses;
  std::unordered_map<KeyFrameId, std::array<double, 3>> kf_velocities;
  std::unordered_map<KeyFrameId, ImuBias> kf_biases;
  std::unordered_map<MapPointId, std::array<double, 3>> mp_positions;
  std::unordered_map<KeyFrameId, SE3> fixed_kf_poses;
  std::vector<InertialVisualObs> visual_observations;
  std::vector<ImuEdgeData> imu_edges;
  std::vector<KeyFrameId> opt_kf_ids;
  std::vector<MapPointId> mp_ids;
};

struct InertialBAResultData {   // :90-106; the first keyframe of the window is not reported (:1250)
  std::unordered_map<KeyFrameId, SE3> optimized_poses;
  std::unordered_map<KeyFrameId, std::array<double, 3>> optimized_velocities;
  std::unordered_map<KeyFrameId, ImuBias> optimized_biases;
  std::unordered_map<MapPointId, std::array<double, 3>> optimized_points;
  size_t iterations = 0;
  double initial_error = 0, final_error = 0;
};

// local_inertial_ba.rs:1074-1275.  The id -> index re-keying is the reference's own (:1084-1185).
inline std::optional<InertialBAResultData> solve_inertial_ba(Handle& h, const InertialBAProblemData& problem, const CameraModel& camera,
                                                             const LocalInertialBAConfig& config, const std::function<bool()>& should_stop) {
  const int K = (int)problem.opt_kf_ids.size(), M = (int)problem.mp_ids.size();
  if (K < 2) return std::nullopt;                                         // :1080-1082
  std::unordered_map<KeyFrameId, int> kf_idx, fixed_idx;
  std::unordered_map<MapPointId, int> mp_idx;
  for (int i = 0; i < K; ++i) kf_idx[problem.opt_kf_ids[(size_t)i]] = i;
  for (int i = 0; i < M; ++i) mp_idx[problem.mp_ids[(size_t)i]] = i;
  std::vector<double> poses, vel, bias, fixed, points, preint;
  for (KeyFrameId id : problem.opt_kf_ids) {                               // :1140-1174, missing entries stay zero
    auto p = problem.kf_poses.find(id);
    detail::push7(poses, p != problem.kf_poses.end() ? p->second : SE3{});
    auto v = problem.kf_velocities.find(id);
    const std::array<double, 3> vv = v != problem.kf_velocities.end() ? v->second : std::array<double, 3>{0, 0, 0};
    vel.insert(vel.end(), vv.begin(), vv.end());
    auto b = problem.kf_biases.find(id);
    const ImuBias bb = b != problem.kf_biases.end() ? b->second : ImuBias{};
    bias.insert(bias.end(), bb.gyro.begin(), bb.gyro.end());
    bias.insert(bias.end(), bb.accel.begin(), bb.accel.end());
  }
  for (const auto& kv : problem.fixed_kf_poses) { fixed_idx[kv.first] = (int)fixed_idx.size(); detail::push7(fixed, kv.second); }
  for (MapPointId id : problem.mp_ids) {
    auto it = problem.mp_positions.find(id);
    const std::array<double, 3> p = it != problem.mp_positions.end() ? it->second : std::array<double, 3>{0, 0, 0};
    points.insert(points.end(), p.begin(), p.end());
  }
  std::vector<orbx_ba_obs> obs;
  for (const InertialVisualObs& o : problem.visual_observations) {         // :1101-1120
    auto m = mp_idx.find(o.mp_id);
    if (m == mp_idx.end()) continue;
    orbx_ba_obs b{};
    b.mp_idx = m->second; b.u = o.observed_uv[0]; b.v = o.observed_uv[1]; b._pad = o.is_stereo ? 1 : 0;
    auto k = o.is_kf_in_window ? kf_idx.find(o.kf_id) : kf_idx.end();
    if (k != kf_idx.end()) { b.kf_idx = k->second; b.fixed_idx = -1; }
    else { auto f = fixed_idx.find(o.kf_id); b.kf_idx = -1; b.fixed_idx = f != fixed_idx.end() ? f->second : -1; }
    obs.push_back(b);
  }
  std::vector<int> edges;
  for (const ImuEdgeData& e : problem.imu_edges) {                         // :1123-1137
    auto i = kf_idx.find(e.kf_i_id), j = kf_idx.find(e.kf_j_id);
    if (i == kf_idx.end() || j == kf_idx.end()) continue;
    edges.push_back(i->second); edges.push_back(j->second);
    preint.insert(preint.end(), e.preint.delta_rot.begin(), e.preint.delta_rot.end());
    preint.insert(preint.end(), e.preint.delta_vel.begin(), e.preint.delta_vel.end());
    preint.insert(preint.end(), e.preint.delta_pos.begin(), e.preint.delta_pos.end());
    preint.push_back(e.preint.dt);
  }
  std::vector<double> po((size_t)K * 7), vo((size_t)K * 3), bo((size_t)K * 6);
  int it = 0;
  double e0 = 0, e1 = 0;
  const orbx_camera c = camera.c();
  const orbx_inertial_ba_config cfg{config.max_iterations, config.window_size, config.huber_threshold_mono, config.huber_threshold_stereo,
                                    config.initial_lambda, config.gyro_rw_info, config.accel_rw_info};
  const int rc = orbx_ba_solve_inertial(h.get(), &c, &cfg, K, poses.data(), vel.data(), bias.data(), (int)fixed_idx.size(), fixed.data(), M,
                                        points.data(), (int)obs.size(), obs.data(), (int)(edges.size() / 2), edges.data(), preint.data(),
                                        detail::stop_fn(should_stop), detail::stop_user(should_stop), po.data(), vo.data(),
                                        bo.data(), &it, &e0, &e1);
  if (rc != ORBX_OK) return std::nullopt;
  InertialBAResultData r;
  for (int i = 1; i < K; ++i) {                                            // skip(1), :1250
    const KeyFrameId id = problem.opt_kf_ids[(size_t)i];
    const SE3 p = detail::se3_from7(&po[7 * (size_t)i]);
    r.optimized_poses[id] = p;
    r.optimized_velocities[id] = {vo[3 * (size_t)i], vo[3 * (size_t)i + 1], vo[3 * (size_t)i + 2]};
    ImuBias b;
    for (int q = 0; q < 3; ++q) { b.gyro[q] = bo[6 * (size_t)i + q]; b.accel[q] = bo[6 * (size_t)i + 3 + q]; }
    r.optimized_biases[id] = b;
  }
  for (int j = 0; j < M; ++j) r.optimized_points[problem.mp_ids[(size_t)j]] = {points[3 * (size_t)j], points[3 * (size_t)j + 1], points[3 * (size_t)j + 2]};
  r.iterations = (size_t)it; r.initial_error = e0; r.final_error = e1;
  return r;
}

// ---- local inertial BA from the resident map (orbx.h, "local INERTIAL BA from the resident map") ----
// The window of a temporal chain (positions in `keyframes`, oldest first: collect_temporal_keyframes' result), collected on the
// device.  mp_idx of an observation carries is_stereo as ORBX_BA_OBS32_STEREO.
struct InertialBAWindow {
  int K = 0, F = 0, M = 0, N = 0;
  std::vector<int> fixed_kf;                           // [F - 1]: the other observers, ascending (fixed index 0 is the anchor chain[0])
  std::vector<int> list_slot;                          // [M]
  std::vector<std::array<double, 3>> positions;        // [M]
  std::vector<orbx_ba_obs32> obs32;                    // [N]
};

inline void inertial_window_bounds(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& chain,
                                   int* list_cap, int* obs_cap) {
  std::vector<int> kf_n;
  size_t all = 0, cand = 0;
  for (const orbx_keyframe* k : keyframes) {
    int n = 0;
    h.check(orbx_keyframe_info(k, &n, nullptr, nullptr, nullptr));
    kf_n.push_back(n); all += (size_t)n;
  }
  for (int c : chain) if (c >= 0 && c < (int)kf_n.size()) cand += (size_t)kf_n[(size_t)c];
  *list_cap = (int)std::min(cand, (size_t)store.capacity());
  *obs_cap = (int)all;
}

// orbx_map_collect_inertial_window_device: every output is the caller's device memory (d_counts [4], d_fixed_kf [keyframes.size()],
// d_list_slot / d_positions [list_cap], d_obs32 [obs_cap], 16-byte aligned); asynchronous.  false where the chain is shorter than two.
inline bool map_collect_inertial_window_device(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& chain,
                                               int list_cap, int obs_cap, int* d_counts, int* d_fixed_kf, int* d_list_slot, double* d_positions,
                                               orbx_ba_obs32* d_obs32) {
  const int rc = orbx_map_collect_inertial_window_device(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)chain.size(), chain.data(), list_cap,
                                                         obs_cap, d_counts, d_fixed_kf, d_list_slot, d_positions, d_obs32);
  if (rc == ORBX_ERR_EMPTY) return false;
  h.check(rc);
  return true;
}

// orbx_map_collect_inertial_window: the same into host vectors, synchronous; nullopt where the reference returns None (:940-942, :946-948).
inline std::optional<InertialBAWindow> map_collect_inertial_window(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes,
                                                                   const std::vector<int>& chain) {
  int list_cap = 0, obs_cap = 0;
  inertial_window_bounds(h, store, keyframes, chain, &list_cap, &obs_cap);
  InertialBAWindow w;
  int counts[4] = {0, 0, 0, 0};
  w.fixed_kf.assign(std::max<size_t>(keyframes.size(), 1), -1);
  w.list_slot.resize(std::max(list_cap, 1)); w.positions.resize(std::max(list_cap, 1)); w.obs32.resize(std::max(obs_cap, 1));
  const int rc = orbx_map_collect_inertial_window(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), (int)chain.size(), chain.data(), list_cap, obs_cap,
                                                  counts, w.fixed_kf.data(), w.list_slot.data(), w.positions[0].data(), w.obs32.data());
  if (rc == ORBX_ERR_EMPTY) return std::nullopt;
  h.check(rc);
  w.K = counts[0]; w.F = counts[1]; w.M = counts[2]; w.N = counts[3];
  w.fixed_kf.resize((size_t)w.F - 1); w.list_slot.resize((size_t)w.M); w.positions.resize((size_t)w.M); w.obs32.resize((size_t)w.N);
  return w;
}

struct MapLocalInertialBAResult {                      // row i of the three belongs to keyframes[chain[i]]; row 0 is the anchor's (the reference skips it, :1250)
  int K = 0, F = 0, M = 0, N = 0;
  std::vector<SE3> poses_wc;
  std::vector<std::array<double, 3>> velocities;
  std::vector<ImuBias> biases;
  std::vector<int> fixed_kf;                           // [F - 1]
  size_t iterations = 0;
  double initial_error = 0, final_error = 0;
};

// orbx_map_local_inertial_ba: local_bundle_adjustment's inertial branch (local_mapper.rs:343-375) on the resident map — collected on the
// device, solved where the observations lie, the optimised positions written back into the store.  velocities / biases: one per chain
// entry; edges: (i, j) positions in `chain` with their preintegrations (build_imu_edges, the caller's).  The caller applies the poses
// (orbx_keyframe_set_pose) and keeps velocities and biases.  nullopt where the reference returns None.
inline std::optional<MapLocalInertialBAResult> map_local_inertial_ba(Handle& h, const CameraModel& camera, const LocalInertialBAConfig& config, MapPointStore& store,
                                                                     const std::vector<const orbx_keyframe*>& keyframes, const std::vector<int>& chain,
                                                                     const std::vector<std::array<double, 3>>& velocities, const std::vector<ImuBias>& biases,
                                                                     const std::vector<std::array<int, 2>>& edges, const std::vector<PreintegratedState>& preints,
                                                                     const std::function<bool()>& should_stop) {
  const size_t K = chain.size();
  if (velocities.size() != K || biases.size() != K || preints.size() != edges.size()) throw std::invalid_argument("map_local_inertial_ba: inconsistent array lengths");
  std::vector<double> vel, bias, preint;
  std::vector<int> ek;
  for (size_t i = 0; i < K; ++i) {
    vel.insert(vel.end(), velocities[i].begin(), velocities[i].end());
    bias.insert(bias.end(), biases[i].gyro.begin(), biases[i].gyro.end());
    bias.insert(bias.end(), biases[i].accel.begin(), biases[i].accel.end());
  }
  for (size_t e = 0; e < edges.size(); ++e) {
    ek.push_back(edges[e][0]); ek.push_back(edges[e][1]);
    preint.insert(preint.end(), preints[e].delta_rot.begin(), preints[e].delta_rot.end());
    preint.insert(preint.end(), preints[e].delta_vel.begin(), preints[e].delta_vel.end());
    preint.insert(preint.end(), preints[e].delta_pos.begin(), preints[e].delta_pos.end());
    preint.push_back(preints[e].dt);
  }
  std::vector<double> po(std::max<size_t>(K, 1) * 7), vo(std::max<size_t>(K, 1) * 3), bo(std::max<size_t>(K, 1) * 6);
  MapLocalInertialBAResult r;
  r.fixed_kf.assign(std::max<size_t>(keyframes.size(), 1), -1);
  int counts[4] = {0, 0, 0, 0}, it = 0;
  double e0 = 0, e1 = 0;
  const orbx_camera c = camera.c();
  const orbx_inertial_ba_config cfg{config.max_iterations, config.window_size, config.huber_threshold_mono, config.huber_threshold_stereo,
                                    config.initial_lambda, config.gyro_rw_info, config.accel_rw_info};
  const int rc = orbx_map_local_inertial_ba(h.get(), &c, &cfg, store.get(), (int)keyframes.size(), keyframes.data(), (int)K, chain.data(), vel.data(), bias.data(),
                                            (int)edges.size(), ek.data(), preint.data(), detail::stop_fn(should_stop),
                                            detail::stop_user(should_stop), po.data(), vo.data(), bo.data(), r.fixed_kf.data(), counts, &it, &e0, &e1);
  if (rc == ORBX_ERR_EMPTY) return std::nullopt;
  h.check(rc);
  r.K = counts[0]; r.F = counts[1]; r.M = counts[2]; r.N = counts[3];
  r.fixed_kf.resize((size_t)r.F - 1);
  for (size_t i = 0; i < K; ++i) {
    r.poses_wc.push_back(detail::se3_from7(&po[7 * i]));
    r.velocities.push_back({vo[3 * i], vo[3 * i + 1], vo[3 * i + 2]});
    ImuBias b;
    for (int q = 0; q < 3; ++q) { b.gyro[q] = bo[6 * i + q]; b.accel[q] = bo[6 * i + 3 + q]; }
    r.biases.push_back(b);
  }
  r.iterations = (size_t)it; r.initial_error = e0; r.final_error = e1;
  return r;
}

// ---- global BA from the resident map (include/orbx.h, "global BA from the resident map"; global_ba.rs:100-181, :184-418) ----
struct GlobalBAMapProblem {                            // orbx_map_collect_global's outputs cut to their sizes
  int K = 0, M = 0, N = 0;                             // optimised keyframes (keyframes[1..]), points, observations
  std::vector<int> list_slot;                          // [M] P: the distinct live slots in first-seen order
  std::vector<std::array<double, 3>> positions;        // [M]
  std::vector<orbx_ba_obs32> obs32;                    // [N] kf_idx -1: the anchor keyframes[0]
};

inline void global_map_bounds(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, int* list_cap, int* obs_cap) {
  size_t all = 0;
  for (const orbx_keyframe* k : keyframes) {
    int n = 0;
    h.check(orbx_keyframe_info(k, &n, nullptr, nullptr, nullptr));
    all += (size_t)n;
  }
  *list_cap = (int)std::min(all, (size_t)store.capacity());
  *obs_cap = (int)all;
}

// orbx_map_collect_global_device: every output is the caller's device memory (d_counts [4], d_list_slot / d_positions [list_cap],
// d_obs32 [obs_cap], 16-byte aligned); asynchronous on the handle's stream.
inline void map_collect_global_device(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes, int list_cap, int obs_cap,
                                      int* d_counts, int* d_list_slot, double* d_positions, orbx_ba_obs32* d_obs32) {
  h.check(orbx_map_collect_global_device(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), list_cap, obs_cap, d_counts, d_list_slot, d_positions, d_obs32));
}

// orbx_map_collect_global: the same into host vectors, synchronous; nullopt where the keyframes observe no live map point (:176-178).
inline std::optional<GlobalBAMapProblem> map_collect_global(Handle& h, MapPointStore& store, const std::vector<const orbx_keyframe*>& keyframes) {
  int list_cap = 0, obs_cap = 0;
  global_map_bounds(h, store, keyframes, &list_cap, &obs_cap);
  GlobalBAMapProblem w;
  int counts[4] = {0, 0, 0, 0};
  w.list_slot.resize(std::max(list_cap, 1)); w.positions.resize(std::max(list_cap, 1)); w.obs32.resize(std::max(obs_cap, 1));
  const int rc = orbx_map_collect_global(h.get(), store.get(), (int)keyframes.size(), keyframes.data(), list_cap, obs_cap, counts, w.list_slot.data(),
                                         w.positions[0].data(), w.obs32.data());
  if (rc == ORBX_ERR_EMPTY) return std::nullopt;
  h.check(rc);
  w.K = counts[0]; w.M = counts[2]; w.N = counts[3];
  w.list_slot.resize((size_t)w.M); w.positions.resize((size_t)w.M); w.obs32.resize((size_t)w.N);
  return w;
}

struct MapGlobalBAResult {                             // poses_wc[i] belongs to keyframes[1 + i]; the anchor keyframes[0] keeps its pose (:386)
  int K = 0, M = 0, N = 0;
  std::vector<SE3> poses_wc;
  size_t iterations = 0;
  double initial_error = 0, final_error = 0;
};

// orbx_map_global_ba: run_global_ba's device half on the resident map (loop_closer.rs:237-240) — the whole map collected on the device,
// solved where the observations lie, the optimised positions written back into the store.  The caller applies the poses
// (orbx_keyframe_set_pose).  nullopt where the reference returns None.
inline std::optional<MapGlobalBAResult> map_global_ba(Handle& h, const CameraModel& camera, const GlobalBAConfig& config, MapPointStore& store,
                                                      const std::vector<const orbx_keyframe*>& keyframes, const std::function<bool()>& should_stop) {
  const size_t K = keyframes.empty() ? 0 : keyframes.size() - 1;
  std::vector<double> po(std::max<size_t>(K, 1) * 7);
  int counts[4] = {0, 0, 0, 0}, it = 0;
  double e0 = 0, e1 = 0;
  const orbx_camera c = camera.c();
  const orbx_ba_config cfg{config.max_iterations, config.param_tolerance, config.gradient_tolerance, config.huber_threshold, 0};
  const int rc = orbx_map_global_ba(h.get(), &c, &cfg, store.get(), (int)keyframes.size(), keyframes.data(), detail::stop_fn(should_stop),
                                    detail::stop_user(should_stop), po.data(), counts, &it, &e0, &e1);
  if (rc == ORBX_ERR_EMPTY) return std::nullopt;
  h.check(rc);
  MapGlobalBAResult r;
  r.K = counts[0]; r.M = counts[2]; r.N = counts[3];
  for (size_t i = 0; i < K; ++i) r.poses_wc.push_back(detail::se3_from7(&po[7 * i]));
  r.iterations = (size_t)it; r.initial_error = e0; r.final_error = e1;
  return r;
}

// ---- pose-inertial optimization for tracking (src/optimizer/pose_inertial_optim.rs) ----------------------------------
struct PoseInertialConfig {   // pose_inertial_optim.rs:19-45
  size_t max_iterations = 4;
  double chi2_mono_init = 12.0, chi2_stereo_init = 15.6, chi2_mono_final = 5.991, chi2_stereo_final = 7.815, imu_weight = 1.0;
};

struct PoseInertialResult {   // :48-62; pose is T_wc
  SE3 pose;
  std::array<double, 3> velocity{0, 0, 0};
  ImuBias bias;
  size_t num_inliers = 0, num_observations = 0, iterations = 0;
};

struct PoseObservation {   // :65-74.  uv: the keypoint's position, an f32 pair (refine_with_imu widens kp.pt() to f64, tracker.rs:508)
  std::array<float, 2> uv;
  std::array<double, 3> point_world;
  bool is_stereo;
  size_t index;
};

// pose_inertial_optim.rs:94-216, the specification of orbx_pose_inertial_optimize (orbx.h).  prev_kf_bias is ignored, as in the
// reference.  An out-of-range config (max_iterations > 64, thresholds <= 0, imu_weight negative or not finite) throws orbx::Error.
inline PoseInertialResult pose_inertial_optimization(Handle& h, const SE3& initial_pose, const std::array<double, 3>& initial_velocity,
                                                     const ImuBias& initial_bias, const SE3& prev_kf_pose,
                                                     const std::array<double, 3>& prev_kf_velocity, const ImuBias& /*prev_kf_bias*/,
                                                     const PreintegratedState& preintegrated, const std::vector<PoseObservation>& observations,
                                                     const CameraModel& camera, const PoseInertialConfig& config) {
  const int n = (int)observations.size();
  const orbx_camera cam = camera.c();
  const orbx_pose_inertial_config cfg{(int)std::min<size_t>(config.max_iterations, 1u << 30), config.chi2_mono_init, config.chi2_stereo_init,
                                      config.chi2_mono_final, config.chi2_stereo_final, config.imu_weight};
  const auto pose7 = [](const SE3& s, double* o) {
    for (int k = 0; k < 4; ++k) o[k] = s.rotation[k];
    for (int k = 0; k < 3; ++k) o[4 + k] = s.translation[k];
  };
  double pose[7], prev[7], bias[6], pre[11];
  pose7(initial_pose, pose);
  pose7(prev_kf_pose, prev);
  for (int k = 0; k < 3; ++k) { bias[k] = initial_bias.gyro[k]; bias[3 + k] = initial_bias.accel[k]; }
  for (int k = 0; k < 4; ++k) pre[k] = preintegrated.delta_rot[k];
  for (int k = 0; k < 3; ++k) { pre[4 + k] = preintegrated.delta_vel[k]; pre[7 + k] = preintegrated.delta_pos[k]; }
  pre[10] = preintegrated.dt;
  std::vector<double> p3(3 * (size_t)std::max(n, 1));
  std::vector<float> p2(2 * (size_t)std::max(n, 1));
  std::vector<uint8_t> st(std::max(n, 1));
  for (int i = 0; i < n; ++i) {
    const PoseObservation& o = observations[(size_t)i];
    for (int k = 0; k < 3; ++k) p3[3 * (size_t)i + k] = o.point_world[k];
    p2[2 * (size_t)i] = o.uv[0]; p2[2 * (size_t)i + 1] = o.uv[1];
    st[(size_t)i] = o.is_stereo ? 1 : 0;
  }
  double po[7], vo[3], bo[6];
  orbx_pose_inertial_result res;
  h.check(orbx_pose_inertial_optimize(h.get(), &cam, &cfg, pose, initial_velocity.data(), bias, prev, prev_kf_velocity.data(), pre, n,
                                      p3.data(), p2.data(), st.data(), po, vo, bo, nullptr, &res));
  PoseInertialResult r;
  r.pose.rotation = {po[0], po[1], po[2], po[3]};
  r.pose.translation = {po[4], po[5], po[6]};
  r.velocity = {vo[0], vo[1], vo[2]};
  for (int k = 0; k < 3; ++k) { r.bias.gyro[k] = bo[k]; r.bias.accel[k] = bo[3 + k]; }
  r.num_inliers = (size_t)res.num_inliers;
  r.num_observations = (size_t)res.num_observations;
  r.iterations = (size_t)res.iterations;
  return r;
}

// ---- place recognition (src/atlas/keyframe_db.rs, src/loop_closing/detector.rs) -------------------------------------------------
using KeyFrameId = uint64_t;

struct LoopDetectorConfig {   // detector.rs:17-46
  double min_score_ratio = 0.75;
  size_t consistency_threshold = 3, min_covisibles_for_threshold = 5, max_covisibles_to_check = 10, min_temporal_gap = 30;
  orbx_loop_detector_config c() const {
    return orbx_loop_detector_config{min_score_ratio, (int)consistency_threshold, (int)min_covisibles_for_threshold, (int)max_covisibles_to_check,
                                     (int)min_temporal_gap};
  }
};

struct Candidate {   // keyframe_db.rs:22-28
  KeyFrameId keyframe_id;
  size_t map_index;
  double score;
};

struct LoopCandidate {   // detector.rs:49-62; loop_covisibles is map bookkeeping, filled by the caller
  KeyFrameId current_kf_id, loop_kf_id;
  double bow_score;
  std::vector<KeyFrameId> loop_covisibles;
};

enum class BowScoring { L1 = ORBX_KFDB_SCORE_L1, Dot = ORBX_KFDB_SCORE_DOT };   // compute_bow_score with / without a vocabulary (detector.rs:371-388)

// KeyFrameDatabase (keyframe_db.rs:31-95) with the BowVectors in device memory (orbx_kfdb), and detect_loop_candidates over it.
class KeyFrameDatabase {
 public:
  explicit KeyFrameDatabase(Handle& h) : h_(&h) { h.check(orbx_kfdb_create(h.get(), &db_)); }
  KeyFrameDatabase(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
  KeyFrameDatabase(KeyFrameDatabase&& o) noexcept : h_(o.h_), db_(o.db_) { o.db_ = nullptr; }
  ~KeyFrameDatabase() { if (db_) orbx_kfdb_destroy(db_); }
  orbx_kfdb* get() const { return db_; }

  void add(KeyFrameId kf_id, const BowVector& bow, size_t map_idx, bool is_bad = false) {   // keyframe_db.rs:45-47
    std::vector<uint32_t> k; std::vector<double> w;
    flat(bow, k, w);
    h_->check(orbx_kfdb_add(db_, kf_id, (int)map_idx, is_bad ? 1 : 0, k.data(), w.data(), (int)k.size()));
  }
  // the same from sorted arrays, as orbx_bow_vectors returns them
  void add(KeyFrameId kf_id, const std::vector<uint32_t>& words, const std::vector<double>& weights, size_t map_idx, bool is_bad = false) {
    if (words.size() != weights.size()) throw std::invalid_argument("KeyFrameDatabase::add: words / weights differ in length");
    h_->check(orbx_kfdb_add(db_, kf_id, (int)map_idx, is_bad ? 1 : 0, words.data(), weights.data(), (int)words.size()));
  }
  void erase(KeyFrameId kf_id) { h_->check(orbx_kfdb_erase(db_, kf_id)); }                  // :50-52
  void set_bad(KeyFrameId kf_id, bool is_bad) { h_->check(orbx_kfdb_set_bad(db_, kf_id, is_bad ? 1 : 0)); }
  size_t size() const { int n = 0; orbx_kfdb_size(db_, &n, nullptr); return (size_t)n; }

  // keyframe_db.rs:58-94
  std::vector<Candidate> detect_candidates(const BowVector& query, std::optional<size_t> exclude_map, size_t max_results) const {
    std::vector<uint32_t> k; std::vector<double> w;
    flat(query, k, w);
    return detect_candidates(k, w, exclude_map, max_results);
  }
  std::vector<Candidate> detect_candidates(const std::vector<uint32_t>& words, const std::vector<double>& weights, std::optional<size_t> exclude_map,
                                           size_t max_results) const {
    const int cap = (int)std::min(max_results, size());
    std::vector<uint64_t> ids((size_t)std::max(cap, 1)); std::vector<int> maps((size_t)std::max(cap, 1)); std::vector<double> sc((size_t)std::max(cap, 1));
    int n = 0;
    h_->check(orbx_kfdb_detect_candidates(db_, words.data(), weights.data(), (int)words.size(), exclude_map ? (int)*exclude_map : -1, cap, ids.data(),
                                          maps.data(), sc.data(), &n));
    std::vector<Candidate> out;
    for (int i = 0; i < n; ++i) out.push_back(Candidate{ids[(size_t)i], (size_t)maps[(size_t)i], sc[(size_t)i]});
    return out;
  }
  // detector.rs:185-368; connected: get_connected_keyframes(kf_id) in iteration order (:232-262).  Every candidate is returned.
  std::vector<LoopCandidate> detect_loop_candidates(KeyFrameId kf_id, const std::vector<KeyFrameId>& connected, const LoopDetectorConfig& config,
                                                    BowScoring scoring = BowScoring::L1) const {
    const orbx_loop_detector_config c = config.c();
    const int cap = (int)size();
    std::vector<uint64_t> ids((size_t)std::max(cap, 1)); std::vector<double> sc((size_t)std::max(cap, 1));
    int n = 0;
    h_->check(orbx_kfdb_detect_loop_candidates(db_, &c, (int)scoring, kf_id, connected.data(), (int)connected.size(), cap, ids.data(), sc.data(), &n));
    std::vector<LoopCandidate> out;
    for (int i = 0; i < n && i < cap; ++i) out.push_back(LoopCandidate{kf_id, ids[(size_t)i], sc[(size_t)i], {}});
    return out;
  }

 private:
  static void flat(const BowVector& v, std::vector<uint32_t>& k, std::vector<double>& w) {
    for (const auto& kv : v) k.push_back(kv.first);
    std::sort(k.begin(), k.end());
    for (uint32_t x : k) w.push_back(v.at(x));
  }
  Handle* h_;
  orbx_kfdb* db_ = nullptr;
};

// detector.rs:68-167: host set logic, no device involved
class ConsistencyChecker {
 public:
  explicit ConsistencyChecker(const LoopDetectorConfig& config) : config_(config) {}
  std::optional<LoopCandidate> add_and_check(KeyFrameId kf_id, const std::vector<LoopCandidate>& candidates) {   // :94-146
    std::unordered_set<KeyFrameId> candidate_set;
    for (const LoopCandidate& c : candidates) {
      candidate_set.insert(c.loop_kf_id);
      for (KeyFrameId cov : c.loop_covisibles) candidate_set.insert(cov);
    }
    std::unordered_map<KeyFrameId, size_t> new_counts;
    for (KeyFrameId id : candidate_set) new_counts[id] = region_count(id) + 1;
    const LoopCandidate* best = nullptr;
    for (const LoopCandidate& c : candidates) {
      auto it = new_counts.find(c.loop_kf_id);
      if (it != new_counts.end() && it->second >= config_.consistency_threshold && (!best || c.bow_score > best->bow_score)) best = &c;
    }
    history_.emplace_back(kf_id, std::move(candidate_set));
    if (history_.size() > config_.consistency_threshold + 2) history_.pop_front();
    consistent_counts_ = std::move(new_counts);
    if (best) {
      LoopCandidate result = *best;
      clear();
      return result;
    }
    return std::nullopt;
  }
  void clear() { history_.clear(); consistent_counts_.clear(); }                                               // :163-166
  size_t history_len() const { return history_.size(); }

 private:
  size_t region_count(KeyFrameId id) const {                                                                  // :149-160
    size_t n = 0;
    for (const auto& h : history_) n += h.second.count(id);
    return n;
  }
  LoopDetectorConfig config_;
  std::deque<std::pair<KeyFrameId, std::unordered_set<KeyFrameId>>> history_;
  std::unordered_map<KeyFrameId, size_t> consistent_counts_;
};

}  // namespace orbx
