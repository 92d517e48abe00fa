// Driver for the C++ mirror of the resident map-point store (include/orbx.hpp: MapPointStore, MapTrackFrame, MapTrackResult,
// map_track_frames and the track_local_map / track_with_motion_model overloads that take a store): reads a store, keyframe slot
// tables and frames from <dir>/map_store_in.bin, tracks every frame from its keyframes (mode 1) and then from the slots that
// matched (mode 0), runs the two single-frame overloads on frame 0, and writes every result to <dir>/map_store_out.bin.
// Run by tests/test_map_store_cpp.py.
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

static void write_result(FILE* o, const orbx::MapTrackResult& r) {
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
  wr(o, r.list_slot); wr(o, r.matched_slot);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/map_store_in.bin").c_str(), "rb");
  if (!f) return 2;
  int capacity = 0, n_set = 0, n_kf = 0, B = 0;
  double c5[5];
  if (!rd(f, &capacity, 1) || !rd(f, &n_set, 1) || !rd(f, &n_kf, 1) || !rd(f, &B, 1) || !rd(f, c5, 5)) return 2;
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
  std::vector<std::vector<int>> frame_kfs((size_t)B);
  std::vector<orbx::SE3> search((size_t)B), prior((size_t)B);
  for (int b = 0; b < B; ++b) {
    int n = 0, nk = 0;
    double sp[7], pr[7];
    if (!rd(f, &n, 1) || !rd(f, &nk, 1) || !rd(f, sp, 7) || !rd(f, pr, 7)) return 2;
    frame_kfs[b].resize((size_t)nk);
    feats[b].keypoints.resize((size_t)n); feats[b].descriptors.resize(32 * (size_t)n);
    if (!rd(f, frame_kfs[b].data(), (size_t)nk) || !rd(f, feats[b].keypoints.data(), (size_t)n) || !rd(f, feats[b].descriptors.data(), 32 * (size_t)n)) return 2;
    search[b].rotation = {sp[0], sp[1], sp[2], sp[3]}; search[b].translation = {sp[4], sp[5], sp[6]};
    prior[b].rotation = {pr[0], pr[1], pr[2], pr[3]}; prior[b].translation = {pr[4], pr[5], pr[6]};
  }
  fclose(f);
  std::vector<orbx_keyframe*> kfs;
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
      std::vector<orbx::MapTrackFrame> frames((size_t)B);
      for (int b = 0; b < B; ++b) {
        frames[b].features = &feats[b]; frames[b].search_pose = search[b]; frames[b].prior = prior[b];
        for (int k : frame_kfs[b]) frames[b].keyframes.push_back(kfs[(size_t)k]);
      }
      FILE* o = fopen((dir + "/map_store_out.bin").c_str(), "wb");
      if (!o) return 2;
      const std::vector<orbx::MapTrackResult> first = orbx::map_track_frames(h, cam, store, frames, ORBX_MAP_SOURCE_KEYFRAMES, 1);
      for (const auto& r : first) write_result(o, r);
      for (int b = 0; b < B; ++b) { frames[b].slots = first[b].matched_slot; frames[b].prior = search[b]; }
      for (const auto& r : orbx::map_track_frames(h, cam, store, frames, ORBX_MAP_SOURCE_SLOTS, 0)) write_result(o, r);
      write_result(o, orbx::track_local_map(h, cam, store, feats[0], frames[0].keyframes, search[0], prior[0]));
      write_result(o, orbx::track_with_motion_model(h, cam, store, feats[0], first[0].matched_slot, search[0]));
      const int32_t info[2] = {store.capacity(), store.n_live()};
      fwrite(info, 4, 2, o);
      fclose(o);
      for (orbx_keyframe* k : kfs) orbx_keyframe_destroy(k);
      kfs.clear();
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    rc = 1;
  }
  for (void* p : dev) if (p) hipFree(p);
  if (rc) return rc;
  printf("MAP_STORE_DRIVER_OK\n");
  return 0;
}
