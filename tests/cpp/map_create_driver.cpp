// Driver for the C++ mirror of point creation and removal on the resident map (include/orbx.hpp: map_create_points,
// map_remove_points, map_cull_points): reads a store, the current keyframe and its neighbours (slot table, keypoints, descriptors,
// stereo points, pose, node ids) and the free slots from <dir>/map_create_in.bin; runs map_create_points (both phases), then
// map_cull_points on the new slots with min_observations = 2, and writes the results, every keyframe's table and the store to
// <dir>/map_create_out.bin.  Run by tests/test_map_create_gpu.py.
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

static std::vector<void*> g_dev;

// the keyframes go before the handle that made them (orbx_keyframe_destroy synchronises the handle's stream)
struct KeyFrames {
  std::vector<orbx_keyframe*> v;
  ~KeyFrames() { for (orbx_keyframe* k : v) orbx_keyframe_destroy(k); }
};

static void* upload(const void* src, size_t bytes) {
  void* d = nullptr;
  if (hipMalloc(&d, bytes ? bytes : 1) != 0 || (bytes && hipMemcpy(d, src, bytes, 1) != 0)) { fprintf(stderr, "device upload failed\n"); exit(3); }
  g_dev.push_back(d);
  return d;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/map_create_in.bin").c_str(), "rb");
  if (!f) return 2;
  int capacity = 0, n_set = 0, n_kf = 0, n_free = 0;
  if (!rd(f, &capacity, 1) || !rd(f, &n_set, 1) || !rd(f, &n_kf, 1) || !rd(f, &n_free, 1)) return 2;
  std::vector<int> slots((size_t)n_set), free_slots((size_t)n_free);
  std::vector<std::array<double, 3>> positions((size_t)n_set);
  std::vector<uint8_t> descs(32 * (size_t)n_set);
  if (!rd(f, slots.data(), slots.size()) || !rd(f, positions.data(), positions.size()) || !rd(f, descs.data(), descs.size()) ||
      !rd(f, free_slots.data(), free_slots.size()))
    return 2;
  int rc = 0;
  try {
    const orbx::CameraModel cam{458.654, 457.296, 367.215, 248.375, 0.11007};
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    orbx::MapPointStore store(h, capacity);
    KeyFrames owned;
    std::vector<orbx_keyframe*>& kfs = owned.v;
    store.set(slots, positions, descs);
    for (int k = 0; k < n_kf; ++k) {
      int n = 0, has_table = 0, has_nodes = 0;
      double pose[7];
      if (!rd(f, &n, 1) || !rd(f, &has_table, 1) || !rd(f, &has_nodes, 1) || !rd(f, pose, 7)) return 2;
      const size_t N = (size_t)n;
      std::vector<int> table(N);
      std::vector<uint8_t> kp(sizeof(orbx_keypoint) * N), desc(32 * N), has(N);
      std::vector<double> pts(3 * N);
      std::vector<uint32_t> node(N);
      if (!rd(f, table.data(), N) || !rd(f, kp.data(), kp.size()) || !rd(f, desc.data(), desc.size()) || !rd(f, pts.data(), pts.size()) || !rd(f, has.data(), N) ||
          !rd(f, node.data(), N))
        return 2;
      orbx_keyframe* kf = nullptr;
      h.check(orbx_keyframe_create(h.get(), (const orbx_keypoint*)upload(kp.data(), kp.size()), (const uint8_t*)upload(desc.data(), desc.size()), n,
                                   (const double*)upload(pts.data(), 8 * pts.size()), (const uint8_t*)upload(has.data(), N), (uint64_t)k, 0, pose, &kf));
      kfs.push_back(kf);
      if (has_table) h.check(orbx_keyframe_set_map_point_slots(kf, store.get(), table.data()));
      if (has_nodes) h.check(orbx_keyframe_set_feature_nodes(kf, node.data()));
    }
    fclose(f);
    FILE* o = fopen((dir + "/map_create_out.bin").c_str(), "wb");
    if (!o) return 2;
    const std::vector<orbx_keyframe*> nbs(kfs.begin() + 1, kfs.end());
    const orbx::MapCreatedPoints r = orbx::map_create_points(h, cam, orbx::TriangulationConfig{}, false, store, kfs[0], nbs, free_slots);
    wr(o, std::vector<int>{r.n_stereo, r.n_pairs, (int)r.new_slot.size(), r.dropped});
    wr(o, r.new_slot); wr(o, r.new_neighbour); wr(o, r.new_idx1); wr(o, r.new_idx2); wr(o, r.new_points); wr(o, r.stats);
    for (const orbx_keyframe* k : kfs) wr(o, orbx::keyframe_map_point_slots(h, k));
    const std::vector<int> culled = orbx::map_cull_points(h, store, kfs, r.new_slot, 2);
    wr(o, culled);
    for (const orbx_keyframe* k : kfs) wr(o, orbx::keyframe_map_point_slots(h, k));
    std::vector<int> all((size_t)capacity);
    for (int s = 0; s < capacity; ++s) all[(size_t)s] = s;
    std::vector<std::array<double, 3>> p;
    std::vector<uint8_t> d, live;
    store.download(all, p, d, live);
    wr(o, live); wr(o, p); wr(o, d);
    fclose(o);
  } catch (const std::exception& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    rc = 1;
  }
  for (void* p : g_dev) hipFree(p);
  if (rc) return rc;
  printf("MAP_CREATE_DRIVER_OK\n");
  return 0;
}
