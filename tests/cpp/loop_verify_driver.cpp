// Driver for the C++ mirror of loop-candidate verification (include/orbx.hpp: LoopKeyFrame, VerifiedLoop, verify_loop_candidate,
// Sim3SolverConfig, Sim3Result, compute_sim3_ransac, compute_sim3_from_matches): reads keyframe pairs and point sets from
// <dir>/lv_in.bin, runs the mirror on every one, and writes every result to <dir>/lv_out.bin.  Run by tests/test_loop_verify_cpu.py
// (compile and link) and tests/test_loop_verify_cpp.py (results).
#include <cstdio>
#include <string>
#include <vector>

#include "orbx.hpp"

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

template <typename T>
static void wr(FILE* o, const std::vector<T>& v) {
  const uint64_t n = v.size();
  fwrite(&n, 8, 1, o);
  if (n) fwrite(v.data(), sizeof(T), n, o);
}

static void write_sim3(FILE* o, const orbx::Sim3& s) {
  fwrite(s.rotation.data(), 8, 4, o);
  fwrite(s.translation.data(), 8, 3, o);
  fwrite(&s.scale, 8, 1, o);
}

static bool read_keyframe(FILE* f, orbx::FeatureSet& fs, orbx::LoopKeyFrame& kf) {
  int n = 0, has_nodes = 0;
  double p[7];
  if (!rd(f, &n, 1) || !rd(f, &has_nodes, 1) || !rd(f, p, 7)) return false;
  fs.keypoints.resize((size_t)n); fs.descriptors.resize(32 * (size_t)n);
  kf.points_cam.resize((size_t)n); kf.has_point.resize((size_t)n); kf.map_points.resize((size_t)n);
  if (has_nodes) kf.feature_nodes.resize((size_t)n);
  kf.pose.rotation = {p[0], p[1], p[2], p[3]}; kf.pose.translation = {p[4], p[5], p[6]};
  return rd(f, fs.keypoints.data(), (size_t)n) && rd(f, fs.descriptors.data(), 32 * (size_t)n) && rd(f, kf.points_cam.data(), (size_t)n) &&
         rd(f, kf.has_point.data(), (size_t)n) && rd(f, kf.feature_nodes.data(), kf.feature_nodes.size()) && rd(f, kf.map_points.data(), (size_t)n);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/lv_in.bin").c_str(), "rb");
  if (!f) return 2;
  int B = 0, P = 0;
  double c5[5];
  if (!rd(f, &B, 1) || !rd(f, &P, 1) || !rd(f, c5, 5)) return 2;
  const orbx::CameraModel cam{c5[0], c5[1], c5[2], c5[3], c5[4]};
  std::vector<orbx::FeatureSet> feats(2 * (size_t)B);
  std::vector<orbx::LoopKeyFrame> kfs(2 * (size_t)B);
  for (size_t k = 0; k < 2 * (size_t)B; ++k) {
    if (!read_keyframe(f, feats[k], kfs[k])) return 2;
    kfs[k].features = &feats[k];
  }
  std::vector<std::vector<std::array<double, 3>>> p1((size_t)P), p2((size_t)P);
  std::vector<int> fix((size_t)P);
  for (int p = 0; p < P; ++p) {
    int n = 0;
    if (!rd(f, &n, 1) || !rd(f, &fix[p], 1)) return 2;
    p1[p].resize((size_t)n); p2[p].resize((size_t)n);
    if (!rd(f, p1[p].data(), (size_t)n) || !rd(f, p2[p].data(), (size_t)n)) return 2;
  }
  fclose(f);
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    FILE* o = fopen((dir + "/lv_out.bin").c_str(), "wb");
    if (!o) return 2;
    for (int b = 0; b < B; ++b) {
      orbx::VerifiedLoop all;
      const std::optional<orbx::VerifiedLoop> v = orbx::verify_loop_candidate(h, cam, kfs[2 * b], kfs[2 * b + 1], 100 + b, 200 + b, nullptr, &all);
      const uint8_t some = v ? 1 : 0;
      fwrite(&some, 1, 1, o);
      fwrite(&all.record, sizeof(all.record), 1, o);
      write_sim3(o, all.sim3_current_to_loop);
      fwrite(&all.current_kf_id, 8, 1, o); fwrite(&all.loop_kf_id, 8, 1, o);
      wr(o, all.matches);
      std::vector<int> fm;
      for (const auto& m : all.feature_matches) { fm.push_back((int)m.first); fm.push_back((int)m.second); }
      wr(o, fm);
      const std::vector<uint8_t> inl(all.inlier_mask.begin(), all.inlier_mask.end());
      wr(o, inl);
      std::vector<int64_t> mmp;
      for (const auto& m : all.matched_map_points) { mmp.push_back(m.first); mmp.push_back(m.second); }
      wr(o, mmp);
    }
    for (int p = 0; p < P; ++p) {
      const std::optional<orbx::Sim3Result> r = orbx::compute_sim3_from_matches(h, p1[p], p2[p], fix[p] != 0);
      const uint8_t some = r ? 1 : 0;
      fwrite(&some, 1, 1, o);
      const orbx::Sim3Result z = r ? *r : orbx::Sim3Result{};
      write_sim3(o, z.sim3);
      fwrite(&z.record, sizeof(z.record), 1, o);
      const std::vector<uint64_t> idx(z.inliers.begin(), z.inliers.end());
      wr(o, idx);
    }
    int refused = 0;
    orbx::Sim3SolverConfig bad;
    bad.max_iterations = 1025;
    try { orbx::compute_sim3_ransac(h, p1[0], p2[0], bad); } catch (const orbx::Error&) { refused = 1; }
    fwrite(&refused, 4, 1, o);
    fclose(o);
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    return 1;
  }
  printf("LOOP_VERIFY_DRIVER_OK\n");
  return 0;
}
