// Driver for the C++ mirror of tracking against the reference keyframe (include/orbx.hpp: TrackReferenceFrame,
// TrackReferenceResult, track_reference, track_with_reference_kf): reads frames from <dir>/tref_in.bin, runs the batch form and the
// single-frame function on every frame, and writes every result to <dir>/tref_out.bin.  Run by tests/test_track_reference_cpu.py
// (compile and link) and tests/test_track_reference_gpu.py (results).
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

static void write_pose(FILE* o, const orbx::SE3& p) {
  fwrite(p.rotation.data(), 8, 4, o);
  fwrite(p.translation.data(), 8, 3, o);
}

static void write_result(FILE* o, const orbx::TrackReferenceResult& r) {
  fwrite(&r.record, sizeof(r.record), 1, o);
  fwrite(&r.pnp, sizeof(r.pnp), 1, o);
  write_pose(o, r.pose);
  wr(o, r.matches); wr(o, r.kf_idx); wr(o, r.feat_idx); wr(o, r.points3d); wr(o, r.points2d); wr(o, r.reproj_errors);
  const std::vector<uint8_t> inl(r.inlier_mask.begin(), r.inlier_mask.end());
  wr(o, inl);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/tref_in.bin").c_str(), "rb");
  if (!f) return 2;
  int B = 0;
  double c5[5];
  if (!rd(f, &B, 1) || !rd(f, c5, 5)) return 2;
  const orbx::CameraModel cam{c5[0], c5[1], c5[2], c5[3], c5[4]};
  std::vector<orbx::FeatureSet> feats((size_t)B);
  std::vector<std::vector<uint8_t>> kf_desc((size_t)B);
  std::vector<orbx::TrackReferenceFrame> frames((size_t)B);
  for (int b = 0; b < B; ++b) {
    int n = 0, m = 0;
    double pr[7];
    if (!rd(f, &n, 1) || !rd(f, &m, 1) || !rd(f, pr, 7)) return 2;
    feats[b].keypoints.resize((size_t)n); feats[b].descriptors.resize(32 * (size_t)n);
    kf_desc[b].resize(32 * (size_t)m); frames[b].kf_positions.resize((size_t)m); frames[b].kf_valid.resize((size_t)m);
    if (!rd(f, feats[b].keypoints.data(), (size_t)n) || !rd(f, feats[b].descriptors.data(), 32 * (size_t)n) || !rd(f, kf_desc[b].data(), 32 * (size_t)m) ||
        !rd(f, frames[b].kf_positions.data(), (size_t)m) || !rd(f, frames[b].kf_valid.data(), (size_t)m))
      return 2;
    frames[b].features = &feats[b]; frames[b].kf_descriptors = &kf_desc[b];
    frames[b].prior.rotation = {pr[0], pr[1], pr[2], pr[3]}; frames[b].prior.translation = {pr[4], pr[5], pr[6]};
  }
  fclose(f);
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    FILE* o = fopen((dir + "/tref_out.bin").c_str(), "wb");
    if (!o) return 2;
    for (const orbx::TrackReferenceResult& r : orbx::track_reference(h, cam, frames)) write_result(o, r);
    for (int b = 0; b < B; ++b) {
      const std::optional<orbx::SE3> p =
          orbx::track_with_reference_kf(h, cam, feats[b], kf_desc[b], frames[b].kf_positions, frames[b].kf_valid, frames[b].prior);
      const uint8_t some = p ? 1 : 0;
      fwrite(&some, 1, 1, o);
      write_pose(o, p ? *p : orbx::SE3{});
    }
    int refused = 0;
    try { orbx::track_reference(h, cam, frames, 3); } catch (const orbx::Error&) { refused = 1; }
    fwrite(&refused, 4, 1, o);
    fclose(o);
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    return 1;
  }
  printf("TRACK_REFERENCE_DRIVER_OK\n");
  return 0;
}
