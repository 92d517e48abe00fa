// Driver for the C++ mirror of covisibility on the resident map (include/orbx.hpp: map_covisibility, Covisibility, MapLocalSource and
// the track_local_map overload that takes a reference-keyframe index): reads a store, keyframe slot tables, frames with their
// reference indices and n_best from <dir>/covisibility_in.bin, computes every keyframe's weights and best list, tracks the frames in
// one batch and frame 0 alone, and writes every result to <dir>/covisibility_out.bin.  Run by tests/test_covisibility_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "orbx.hpp"

// the three runtime calls the driver needs to place the keyframes' features on the GPU (libamdhip64; hipMemcpyHostToDevice = 1)
extern "C" {
int hipMalloc(void** p, size_t bytes);
int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);
int hipFree(void* p);
}

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

template <typename T>
static void wr(FILE* o, const std::vector<T>& v) {
  const uint64_t n = v.size();
  fwrite(&n, 8, 1, o);
  if (n) fwrite(v.data(), sizeof(T), n, o);
}

static void write_result(FILE* o, const orbx::MapTrackResult& r, const std::vector<int>& local_kf) {
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
  wr(o, r.list_slot); wr(o, r.matched_slot); wr(o, local_kf);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/covisibility_in.bin").c_str(), "rb");
  if (!f) return 2;
  int capacity = 0, n_set = 0, n_kf = 0, B = 0, n_best = 0;
  double c5[5];
  if (!rd(f, &capacity, 1) || !rd(f, &n_set, 1) || !rd(f, &n_kf, 1) || !rd(f, &B, 1) || !rd(f, &n_best, 1) || !rd(f, c5, 5)) return 2;
  const orbx::CameraModel cam{c5[0], c5[1], c5[2], c5[3], c5[4]};
  std::vector<int> slots((size_t)n_set);
  std::vector<std::array<double, 3>> positions((size_t)n_set);
  std::vector<uint8_t> descs(32 * (size_t)n_set);
  if (!rd(f, slots.data(), slots.size()) || !rd(f, positions.data(), positions.size()) || !rd(f, descs.data(), descs.size())) return 2;
  std::vector<std::vector<int>> tables((size_t)n_kf);
  for (auto& t : tables) {
    int n = 0;
    if (!rd(f, &n, 1)) return 2;
    t.resize((size_t)n);
    if (!rd(f, t.data(), t.size())) return 2;
  }
  std::vector<orbx::FeatureSet> feats((size_t)B);
  std::vector<int> ref_kf((size_t)B);
  std::vector<orbx::SE3> search((size_t)B), prior((size_t)B);
  for (int b = 0; b < B; ++b) {
    int n = 0;
    double sp[7], pr[7];
    if (!rd(f, &n, 1) || !rd(f, &ref_kf[b], 1) || !rd(f, sp, 7) || !rd(f, pr, 7)) return 2;
    feats[b].keypoints.resize((size_t)n); feats[b].descriptors.resize(32 * (size_t)n);
    if (!rd(f, feats[b].keypoints.data(), (size_t)n) || !rd(f, feats[b].descriptors.data(), 32 * (size_t)n)) return 2;
    search[b].rotation = {sp[0], sp[1], sp[2], sp[3]}; search[b].translation = {sp[4], sp[5], sp[6]};
    prior[b].rotation = {pr[0], pr[1], pr[2], pr[3]}; prior[b].translation = {pr[4], pr[5], pr[6]};
  }
  fclose(f);
  std::vector<const orbx_keyframe*> kfs;
  std::vector<void*> dev;
  int rc = 0;
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    {
      orbx::MapPointStore store(h, capacity);
      store.set(slots, positions, descs);
      // the keyframes' own features play no part here: zeroed rows of the right count
      for (const auto& t : tables) {
        const size_t n = std::max<size_t>(t.size(), 1);
        std::vector<uint8_t> zero(sizeof(orbx_keypoint) * n, 0);
        void *d_kp = nullptr, *d_desc = nullptr;
        if (hipMalloc(&d_kp, zero.size()) != 0 || hipMemcpy(d_kp, zero.data(), zero.size(), 1) != 0 || hipMalloc(&d_desc, 32 * n) != 0 ||
            hipMemcpy(d_desc, zero.data(), 32 * n, 1) != 0) { fprintf(stderr, "device upload failed\n"); exit(3); }
        dev.push_back(d_kp); dev.push_back(d_desc);
        orbx_keyframe* kf = nullptr;
        h.check(orbx_keyframe_create(h.get(), (const orbx_keypoint*)d_kp, (const uint8_t*)d_desc, (int)t.size(), nullptr, nullptr, kfs.size(), 0, nullptr, &kf));
        kfs.push_back(kf);
        h.check(orbx_keyframe_set_map_point_slots(kf, store.get(), t.data()));
      }
      FILE* o = fopen((dir + "/covisibility_out.bin").c_str(), "wb");
      if (!o) return 2;
      std::vector<int> all((size_t)n_kf);
      for (int k = 0; k < n_kf; ++k) all[(size_t)k] = k;
      const orbx::Covisibility cov = orbx::map_covisibility(h, store, kfs, all, n_best);
      wr(o, cov.weights); wr(o, cov.best); wr(o, cov.n_best);
      wr(o, cov.best_of(0));
      std::vector<orbx::MapTrackFrame> frames((size_t)B);
      for (int b = 0; b < B; ++b) { frames[b].features = &feats[b]; frames[b].search_pose = search[b]; frames[b].prior = prior[b]; }
      std::vector<std::vector<int>> chosen;
      const orbx::MapLocalSource local{&kfs, &ref_kf, n_best, &chosen};
      const std::vector<orbx::MapTrackResult> batch = orbx::map_track_frames(h, cam, store, frames, ORBX_MAP_SOURCE_KEYFRAMES, 1, nullptr, &local);
      for (int b = 0; b < B; ++b) write_result(o, batch[(size_t)b], chosen[(size_t)b]);
      std::vector<int> one;
      const orbx::MapTrackResult r0 = orbx::track_local_map(h, cam, store, feats[0], kfs, ref_kf[0], n_best, search[0], prior[0], &one);
      write_result(o, r0, one);
      fclose(o);
      for (const orbx_keyframe* k : kfs) orbx_keyframe_destroy(const_cast<orbx_keyframe*>(k));
      kfs.clear();
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    rc = 1;
  }
  for (void* p : dev) if (p) hipFree(p);
  if (rc) return rc;
  printf("COVISIBILITY_DRIVER_OK\n");
  return 0;
}
