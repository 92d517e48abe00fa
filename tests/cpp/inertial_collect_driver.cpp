// Driver for the C++ mirror of local inertial BA from the resident map (include/orbx.hpp: map_collect_inertial_window,
// map_local_inertial_ba): reads a store, keyframes (slot table, keypoints, stereo bytes, pose), the chain with its velocities and biases
// and the IMU edges from <dir>/inertial_collect_in.bin, collects the window, runs the local inertial BA and writes the window, the result
// and the window's positions as the store then holds them to <dir>/inertial_collect_out.bin.  tests/test_inertial_collect_cpu.py compiles
// and links it, tests/test_inertial_collect_gpu.py runs it against the Python mirror.
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

static void* upload(const void* src, size_t bytes) {
  void* d = nullptr;
  if (hipMalloc(&d, bytes) != 0 || hipMemcpy(d, src, bytes, 1) != 0) { fprintf(stderr, "device upload failed\n"); exit(3); }
  return d;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/inertial_collect_in.bin").c_str(), "rb");
  if (!f) return 2;
  int capacity = 0, n_set = 0, n_kf = 0, n_chain = 0, n_edge = 0;
  double c5[5];
  if (!rd(f, &capacity, 1) || !rd(f, &n_set, 1) || !rd(f, &n_kf, 1) || !rd(f, &n_chain, 1) || !rd(f, &n_edge, 1) || !rd(f, c5, 5)) return 2;
  const orbx::CameraModel cam{c5[0], c5[1], c5[2], c5[3], c5[4]};
  std::vector<int> slots((size_t)n_set);
  std::vector<std::array<double, 3>> positions((size_t)n_set);
  std::vector<uint8_t> descs(32 * (size_t)n_set);
  if (!rd(f, slots.data(), slots.size()) || !rd(f, positions.data(), positions.size()) || !rd(f, descs.data(), descs.size())) return 2;
  std::vector<std::vector<int>> tables((size_t)n_kf);
  std::vector<std::vector<orbx_keypoint>> kps((size_t)n_kf);
  std::vector<std::vector<uint8_t>> has((size_t)n_kf);
  std::vector<std::array<double, 7>> poses((size_t)n_kf);
  for (int k = 0; k < n_kf; ++k) {
    int n = 0;
    if (!rd(f, &n, 1)) return 2;
    tables[k].resize((size_t)n); kps[k].resize((size_t)n); has[k].resize((size_t)n);
    if (!rd(f, tables[k].data(), (size_t)n) || !rd(f, kps[k].data(), (size_t)n) || !rd(f, has[k].data(), (size_t)n) || !rd(f, poses[k].data(), 7)) return 2;
  }
  std::vector<int> chain((size_t)n_chain);
  std::vector<std::array<double, 3>> vel((size_t)n_chain);
  std::vector<std::array<double, 6>> bias6((size_t)n_chain);
  std::vector<std::array<int, 2>> edges((size_t)n_edge);
  std::vector<std::array<double, 11>> pre11((size_t)n_edge);
  if (!rd(f, chain.data(), chain.size()) || !rd(f, vel.data(), vel.size()) || !rd(f, bias6.data(), bias6.size()) || !rd(f, edges.data(), edges.size()) ||
      !rd(f, pre11.data(), pre11.size()))
    return 2;
  fclose(f);
  std::vector<orbx::ImuBias> biases;
  for (const auto& b : bias6) biases.push_back(orbx::ImuBias{{b[0], b[1], b[2]}, {b[3], b[4], b[5]}});
  std::vector<orbx::PreintegratedState> preints;
  for (const auto& p : pre11) preints.push_back(orbx::PreintegratedState{{p[0], p[1], p[2], p[3]}, {p[4], p[5], p[6]}, {p[7], p[8], p[9]}, p[10]});
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
        std::vector<uint8_t> rows(sizeof(orbx_keypoint) * n, 0), zero(32 * n, 0), hp(n, 0);
        std::vector<double> pts(3 * n, 0.0);
        if (!kps[k].empty()) memcpy(rows.data(), kps[k].data(), sizeof(orbx_keypoint) * kps[k].size());
        if (!has[k].empty()) memcpy(hp.data(), has[k].data(), has[k].size());
        void *d_kp = upload(rows.data(), rows.size()), *d_desc = upload(zero.data(), zero.size()), *d_pts = upload(pts.data(), 8 * pts.size()),
             *d_has = upload(hp.data(), hp.size());
        dev.insert(dev.end(), {d_kp, d_desc, d_pts, d_has});
        orbx_keyframe* kf = nullptr;
        h.check(orbx_keyframe_create(h.get(), (const orbx_keypoint*)d_kp, (const uint8_t*)d_desc, (int)tables[k].size(), (const double*)d_pts, (const uint8_t*)d_has,
                                     kfs.size(), 0, poses[k].data(), &kf));
        kfs.push_back(kf);
        h.check(orbx_keyframe_set_map_point_slots(kf, store.get(), tables[k].data()));
      }
      FILE* o = fopen((dir + "/inertial_collect_out.bin").c_str(), "wb");
      if (!o) return 2;
      const std::optional<orbx::InertialBAWindow> w = orbx::map_collect_inertial_window(h, store, kfs, chain);
      if (!w) { fprintf(stderr, "the window is empty\n"); exit(4); }
      const std::vector<int> counts{w->K, w->F, w->M, w->N};
      wr(o, counts); wr(o, w->fixed_kf); wr(o, w->list_slot); wr(o, w->positions); wr(o, w->obs32);
      const std::optional<orbx::MapLocalInertialBAResult> r = orbx::map_local_inertial_ba(h, cam, orbx::LocalInertialBAConfig{}, store, kfs, chain, vel, biases, edges,
                                                                                          preints, nullptr);
      if (!r) { fprintf(stderr, "the local inertial BA answered None\n"); exit(4); }
      const std::vector<int> rcounts{r->K, r->F, r->M, r->N};
      wr(o, rcounts); wr(o, r->fixed_kf);
      std::vector<double> flat;
      for (const orbx::SE3& p : r->poses_wc) { flat.insert(flat.end(), p.rotation.begin(), p.rotation.end()); flat.insert(flat.end(), p.translation.begin(), p.translation.end()); }
      wr(o, flat); wr(o, r->velocities);
      std::vector<double> bflat;
      for (const orbx::ImuBias& b : r->biases) { bflat.insert(bflat.end(), b.gyro.begin(), b.gyro.end()); bflat.insert(bflat.end(), b.accel.begin(), b.accel.end()); }
      wr(o, bflat);
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
  printf("INERTIAL_COLLECT_DRIVER_OK\n");
  return 0;
}
