// Driver for the C++ mirror of the tracker's per-frame step (include/orbx.hpp: TrackFrame, TrackResult, track_frames,
// track_local_map, track_with_motion_model): reads frames from <dir>/track_in.bin, runs the batch form in both modes and the two
// single-frame functions on frame 0, and writes every result to <dir>/track_out.bin.  Run by tests/test_track_cpp.py.
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

static void write_result(FILE* o, const orbx::TrackResult& r) {
  fwrite(&r.record, sizeof(r.record), 1, o);
  fwrite(&r.pnp, sizeof(r.pnp), 1, o);
  fwrite(r.pose.rotation.data(), 8, 4, o);
  fwrite(r.pose.translation.data(), 8, 3, o);
  const uint64_t n_inl = r.n_inliers;
  fwrite(&n_inl, 8, 1, o);
  std::vector<int32_t> matched;
  for (const auto& m : r.matched_map_points) matched.push_back(m ? (int32_t)*m : -1);
  wr(o, matched); wr(o, r.mp_idx); wr(o, r.feat_idx); wr(o, r.points3d); wr(o, r.points2d); wr(o, r.reproj_errors_full);
  const std::vector<uint64_t> in(r.inlier_indices.begin(), r.inlier_indices.end()), out(r.outlier_indices.begin(), r.outlier_indices.end());
  wr(o, in); wr(o, out);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/track_in.bin").c_str(), "rb");
  if (!f) return 2;
  int B = 0;
  double c5[5];
  if (!rd(f, &B, 1) || !rd(f, c5, 5)) return 2;
  const orbx::CameraModel cam{c5[0], c5[1], c5[2], c5[3], c5[4]};
  std::vector<orbx::FeatureSet> feats((size_t)B);
  std::vector<orbx::TrackFrame> frames((size_t)B);
  for (int b = 0; b < B; ++b) {
    int n = 0, m = 0;
    double sp[7], pr[7];
    if (!rd(f, &n, 1) || !rd(f, &m, 1) || !rd(f, sp, 7) || !rd(f, pr, 7)) return 2;
    feats[b].keypoints.resize((size_t)n); feats[b].descriptors.resize(32 * (size_t)n);
    frames[b].positions.resize((size_t)m); frames[b].mp_descriptors.resize(32 * (size_t)m);
    if (!rd(f, feats[b].keypoints.data(), (size_t)n) || !rd(f, feats[b].descriptors.data(), 32 * (size_t)n) ||
        !rd(f, frames[b].positions.data(), (size_t)m) || !rd(f, frames[b].mp_descriptors.data(), 32 * (size_t)m))
      return 2;
    frames[b].features = &feats[b];
    frames[b].search_pose.rotation = {sp[0], sp[1], sp[2], sp[3]}; frames[b].search_pose.translation = {sp[4], sp[5], sp[6]};
    frames[b].prior.rotation = {pr[0], pr[1], pr[2], pr[3]}; frames[b].prior.translation = {pr[4], pr[5], pr[6]};
  }
  fclose(f);
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    FILE* o = fopen((dir + "/track_out.bin").c_str(), "wb");
    if (!o) return 2;
    for (int mode : {1, 0})
      for (const orbx::TrackResult& r : orbx::track_frames(h, cam, frames, mode)) write_result(o, r);
    const orbx::TrackFrame& f0 = frames[0];
    write_result(o, orbx::track_local_map(h, cam, feats[0], f0.positions, f0.mp_descriptors, f0.search_pose, f0.prior));
    write_result(o, orbx::track_with_motion_model(h, cam, feats[0], f0.positions, f0.mp_descriptors, f0.search_pose));
    fclose(o);
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    return 1;
  }
  printf("TRACK_DRIVER_OK\n");
  return 0;
}
