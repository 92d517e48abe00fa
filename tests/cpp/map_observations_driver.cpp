// Driver for the C++ mirror of the observation calls on the resident map (include/orbx.hpp: map_observations, map_refresh_points,
// map_keyframe_redundancy): reads a store, keyframes (slot table, descriptors, pose), the slots asked for with their normals and the
// candidates from <dir>/map_obs_in.bin, runs the three calls and writes the lists, the redundancy, the refresh and the descriptors
// the store then holds to <dir>/map_obs_out.bin.  Run by tests/test_map_observations_gpu.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/map_obs_in.bin").c_str(), "rb");
  if (!f) return 2;
  int capacity = 0, n_set = 0, n_kf = 0, n_ask = 0, n_cand = 0, min_obs = 0;
  double threshold = 0.0, scale_range = 0.0;
  if (!rd(f, &capacity, 1) || !rd(f, &n_set, 1) || !rd(f, &n_kf, 1) || !rd(f, &n_ask, 1) || !rd(f, &n_cand, 1) || !rd(f, &min_obs, 1) || !rd(f, &threshold, 1) ||
      !rd(f, &scale_range, 1))
    return 2;
  std::vector<int> slots((size_t)n_set), ask((size_t)n_ask), cand((size_t)n_cand);
  std::vector<std::array<double, 3>> positions((size_t)n_set), normals((size_t)n_ask);
  std::vector<uint8_t> descs(32 * (size_t)n_set);
  if (!rd(f, slots.data(), slots.size()) || !rd(f, positions.data(), positions.size()) || !rd(f, descs.data(), descs.size()) || !rd(f, ask.data(), ask.size()) ||
      !rd(f, normals.data(), normals.size()) || !rd(f, cand.data(), cand.size()))
    return 2;
  std::vector<std::vector<int>> tables((size_t)n_kf);
  std::vector<std::vector<uint8_t>> kf_desc((size_t)n_kf);
  std::vector<std::array<double, 7>> poses((size_t)n_kf);
  std::vector<int> has_table((size_t)n_kf);
  for (int k = 0; k < n_kf; ++k) {
    int n = 0;
    if (!rd(f, &n, 1) || !rd(f, &has_table[k], 1)) return 2;
    tables[k].resize((size_t)n); kf_desc[k].resize(32 * (size_t)n);
    if (!rd(f, tables[k].data(), (size_t)n) || !rd(f, kf_desc[k].data(), kf_desc[k].size()) || !rd(f, poses[k].data(), 7)) return 2;
  }
  fclose(f);
  std::vector<const orbx_keyframe*> kfs;
  std::vector<void*> dev;
  int rc = 0;
  try {
    const orbx::CameraModel cam{458.654, 457.296, 367.215, 248.375, 0.11};
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    {
      orbx::MapPointStore store(h, capacity);
      store.set(slots, positions, descs);
      for (int k = 0; k < n_kf; ++k) {
        const size_t n = std::max<size_t>(tables[k].size(), 1);
        std::vector<uint8_t> zero(sizeof(orbx_keypoint) * n, 0), rows(32 * n, 0);
        if (!kf_desc[k].empty()) memcpy(rows.data(), kf_desc[k].data(), kf_desc[k].size());
        void *d_kp = nullptr, *d_desc = nullptr;
        if (hipMalloc(&d_kp, zero.size()) != 0 || hipMemcpy(d_kp, zero.data(), zero.size(), 1) != 0 || hipMalloc(&d_desc, rows.size()) != 0 ||
            hipMemcpy(d_desc, rows.data(), rows.size(), 1) != 0) { fprintf(stderr, "device upload failed\n"); exit(3); }
        dev.push_back(d_kp); dev.push_back(d_desc);
        orbx_keyframe* kf = nullptr;
        h.check(orbx_keyframe_create(h.get(), (const orbx_keypoint*)d_kp, (const uint8_t*)d_desc, (int)tables[k].size(), nullptr, nullptr, kfs.size(), 0,
                                     poses[k].data(), &kf));
        kfs.push_back(kf);
        if (has_table[k]) h.check(orbx_keyframe_set_map_point_slots(kf, store.get(), tables[k].data()));
      }
      FILE* o = fopen((dir + "/map_obs_out.bin").c_str(), "wb");
      if (!o) return 2;
      const orbx::MapObservations ob = orbx::map_observations(h, store, kfs, ask);
      wr(o, ob.obs_start); wr(o, ob.obs_kf); wr(o, ob.obs_feat);
      std::vector<uint8_t> few;
      for (size_t p = 0; p < ask.size(); ++p) few.push_back(ob.too_few_observers(p, min_obs) ? 1 : 0);
      wr(o, few);
      const orbx::KeyFrameRedundancy red = orbx::map_keyframe_redundancy(h, store, kfs, cand, min_obs, threshold);
      wr(o, red.total); wr(o, red.redundant); wr(o, red.cull);
      const orbx::MapPointRefresh r = orbx::map_refresh_points(h, store, kfs, ask, scale_range, normals);
      wr(o, r.mp_descriptors); wr(o, r.normals); wr(o, r.min_distance); wr(o, r.max_distance); wr(o, r.records);
      std::vector<std::array<double, 3>> p_after;
      std::vector<uint8_t> d_after, live;
      store.download(ask, p_after, d_after, live);
      wr(o, d_after);
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
  printf("MAP_OBSERVATIONS_DRIVER_OK\n");
  return 0;
}
