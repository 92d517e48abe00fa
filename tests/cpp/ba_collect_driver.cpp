// Driver for the C++ mirror of local BA from the resident map (include/orbx.hpp: map_collect_ba_window, map_local_ba): reads a store,
// keyframes (slot table, keypoints, pose), cur and max_covisible from <dir>/ba_collect_in.bin, collects the window, runs the local BA
// and writes the window, the result and the window's positions as the store then holds them to <dir>/ba_collect_out.bin.  Run by
// tests/test_ba_collect_gpu.py.
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
  FILE* f = fopen((dir + "/ba_collect_in.bin").c_str(), "rb");
  if (!f) return 2;
  int capacity = 0, n_set = 0, n_kf = 0, cur = 0, max_cov = 0;
  double c5[5];
  if (!rd(f, &capacity, 1) || !rd(f, &n_set, 1) || !rd(f, &n_kf, 1) || !rd(f, &cur, 1) || !rd(f, &max_cov, 1) || !rd(f, c5, 5)) return 2;
  const orbx::CameraModel cam{c5[0], c5[1], c5[2], c5[3], c5[4]};
  std::vector<int> slots((size_t)n_set);
  std::vector<std::array<double, 3>> positions((size_t)n_set);
  std::vector<uint8_t> descs(32 * (size_t)n_set);
  if (!rd(f, slots.data(), slots.size()) || !rd(f, positions.data(), positions.size()) || !rd(f, descs.data(), descs.size())) return 2;
  std::vector<std::vector<int>> tables((size_t)n_kf);
  std::vector<std::vector<orbx_keypoint>> kps((size_t)n_kf);
  std::vector<std::array<double, 7>> poses((size_t)n_kf);
  for (int k = 0; k < n_kf; ++k) {
    int n = 0;
    if (!rd(f, &n, 1)) return 2;
    tables[k].resize((size_t)n); kps[k].resize((size_t)n);
    if (!rd(f, tables[k].data(), (size_t)n) || !rd(f, kps[k].data(), (size_t)n) || !rd(f, poses[k].data(), 7)) return 2;
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
      for (int k = 0; k < n_kf; ++k) {
        const size_t n = std::max<size_t>(tables[k].size(), 1);
        std::vector<uint8_t> rows(sizeof(orbx_keypoint) * n, 0), zero(32 * n, 0);
        if (!kps[k].empty()) memcpy(rows.data(), kps[k].data(), sizeof(orbx_keypoint) * kps[k].size());
        void *d_kp = nullptr, *d_desc = nullptr;
        if (hipMalloc(&d_kp, rows.size()) != 0 || hipMemcpy(d_kp, rows.data(), rows.size(), 1) != 0 || hipMalloc(&d_desc, zero.size()) != 0 ||
            hipMemcpy(d_desc, zero.data(), zero.size(), 1) != 0) { fprintf(stderr, "device upload failed\n"); exit(3); }
        dev.push_back(d_kp); dev.push_back(d_desc);
        orbx_keyframe* kf = nullptr;
        h.check(orbx_keyframe_create(h.get(), (const orbx_keypoint*)d_kp, (const uint8_t*)d_desc, (int)tables[k].size(), nullptr, nullptr, kfs.size(), 0,
                                     poses[k].data(), &kf));
        kfs.push_back(kf);
        h.check(orbx_keyframe_set_map_point_slots(kf, store.get(), tables[k].data()));
      }
      FILE* o = fopen((dir + "/ba_collect_out.bin").c_str(), "wb");
      if (!o) return 2;
      const std::optional<orbx::BAWindow> w = orbx::map_collect_ba_window(h, store, kfs, cur, max_cov);
      if (!w) { fprintf(stderr, "the window is empty\n"); exit(4); }
      const std::vector<int> counts{w->K, w->F, w->M, w->N};
      wr(o, counts); wr(o, w->local_kf); wr(o, w->fixed_kf); wr(o, w->list_slot); wr(o, w->positions); wr(o, w->obs32);
      orbx::LocalBAConfigLM cfg;
      cfg.max_covisible_keyframes = max_cov;
      const std::optional<orbx::MapLocalBAResult> r = orbx::map_local_ba(h, cam, cfg, store, kfs, cur, nullptr);
      if (!r) { fprintf(stderr, "the local BA answered None\n"); exit(4); }
      const std::vector<int> rcounts{r->K, r->F, r->M, r->N};
      wr(o, rcounts); wr(o, r->local_kf);
      std::vector<double> flat;
      for (const orbx::SE3& p : r->poses_wc) { flat.insert(flat.end(), p.rotation.begin(), p.rotation.end()); flat.insert(flat.end(), p.translation.begin(), p.translation.end()); }
      wr(o, flat);
      const std::vector<double> scalars{(double)r->iterations, r->initial_error, r->final_error};
      wr(o, scalars);
      std::vector<std::array<double, 3>> after;
      std::vector<uint8_t> d_after, live;
      store.download(w->list_slot, after, d_after, live);
      wr(o, after);
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
  printf("BA_COLLECT_DRIVER_OK\n");
  return 0;
}
