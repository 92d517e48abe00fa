// Driver for the C++ mirror of fuse and merge on the resident map (include/orbx.hpp: map_fuse, map_search_in_neighbors,
// keyframe_map_point_slots): reads a store, keyframes (slot table, keypoints, descriptors, pose), the current keyframe, its
// neighbours and every slot's normal from <dir>/map_fuse_in.bin; builds the world twice; runs map_fuse([cur], neighbours) on the
// first and map_search_in_neighbors on the second and writes the results, every keyframe's table and the store's live bytes to
// <dir>/map_fuse_out.bin.  Run by tests/test_map_fuse_gpu.py.
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

struct Input {
  int capacity = 0, n_set = 0, n_kf = 0, cur = 0, n_nb = 0;
  double radius_scale = 0.0, scale_range = 0.0;
  std::vector<int> slots, nb, has_table;
  std::vector<std::array<double, 3>> positions, normals;
  std::vector<uint8_t> descs;
  std::vector<std::vector<int>> tables;
  std::vector<std::vector<uint8_t>> kps, kf_desc;
  std::vector<std::array<double, 7>> poses;
};

struct World {
  std::vector<orbx_keyframe*> kfs;
  std::vector<void*> dev;
  void build(orbx::Handle& h, orbx::MapPointStore& store, const Input& in) {
    store.set(in.slots, in.positions, in.descs);
    for (int k = 0; k < in.n_kf; ++k) {
      const size_t n = std::max<size_t>(in.tables[k].size(), 1);
      std::vector<uint8_t> kp(sizeof(orbx_keypoint) * n, 0), rows(32 * n, 0);
      if (!in.kps[k].empty()) memcpy(kp.data(), in.kps[k].data(), in.kps[k].size());
      if (!in.kf_desc[k].empty()) memcpy(rows.data(), in.kf_desc[k].data(), in.kf_desc[k].size());
      void *d_kp = nullptr, *d_desc = nullptr;
      if (hipMalloc(&d_kp, kp.size()) != 0 || hipMemcpy(d_kp, kp.data(), kp.size(), 1) != 0 || hipMalloc(&d_desc, rows.size()) != 0 ||
          hipMemcpy(d_desc, rows.data(), rows.size(), 1) != 0) { fprintf(stderr, "device upload failed\n"); exit(3); }
      dev.push_back(d_kp); dev.push_back(d_desc);
      orbx_keyframe* kf = nullptr;
      h.check(orbx_keyframe_create(h.get(), (const orbx_keypoint*)d_kp, (const uint8_t*)d_desc, (int)in.tables[k].size(), nullptr, nullptr, kfs.size(), 0,
                                   in.poses[k].data(), &kf));
      kfs.push_back(kf);
      if (in.has_table[k]) h.check(orbx_keyframe_set_map_point_slots(kf, store.get(), in.tables[k].data()));
    }
  }
  void dump(FILE* o, orbx::Handle& h, orbx::MapPointStore& store, int capacity) {
    for (const orbx_keyframe* k : kfs) wr(o, orbx::keyframe_map_point_slots(h, k));
    std::vector<int> all((size_t)capacity);
    for (int s = 0; s < capacity; ++s) all[(size_t)s] = s;
    std::vector<std::array<double, 3>> p;
    std::vector<uint8_t> d, live;
    store.download(all, p, d, live);
    wr(o, live); wr(o, d);
  }
  void close() {
    for (orbx_keyframe* k : kfs) orbx_keyframe_destroy(k);
    kfs.clear();
    for (void* p : dev) if (p) hipFree(p);
    dev.clear();
  }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/map_fuse_in.bin").c_str(), "rb");
  if (!f) return 2;
  Input in;
  if (!rd(f, &in.capacity, 1) || !rd(f, &in.n_set, 1) || !rd(f, &in.n_kf, 1) || !rd(f, &in.cur, 1) || !rd(f, &in.n_nb, 1) || !rd(f, &in.radius_scale, 1) ||
      !rd(f, &in.scale_range, 1))
    return 2;
  in.slots.resize((size_t)in.n_set); in.positions.resize((size_t)in.n_set); in.descs.resize(32 * (size_t)in.n_set); in.nb.resize((size_t)in.n_nb);
  in.normals.resize((size_t)in.capacity);
  if (!rd(f, in.slots.data(), in.slots.size()) || !rd(f, in.positions.data(), in.positions.size()) || !rd(f, in.descs.data(), in.descs.size()) ||
      !rd(f, in.nb.data(), in.nb.size()) || !rd(f, in.normals.data(), in.normals.size()))
    return 2;
  in.tables.resize((size_t)in.n_kf); in.kps.resize((size_t)in.n_kf); in.kf_desc.resize((size_t)in.n_kf); in.poses.resize((size_t)in.n_kf); in.has_table.resize((size_t)in.n_kf);
  for (int k = 0; k < in.n_kf; ++k) {
    int n = 0;
    if (!rd(f, &n, 1) || !rd(f, &in.has_table[k], 1)) return 2;
    in.tables[k].resize((size_t)n); in.kps[k].resize(sizeof(orbx_keypoint) * (size_t)n); in.kf_desc[k].resize(32 * (size_t)n);
    if (!rd(f, in.tables[k].data(), (size_t)n) || !rd(f, in.kps[k].data(), in.kps[k].size()) || !rd(f, in.kf_desc[k].data(), in.kf_desc[k].size()) ||
        !rd(f, in.poses[k].data(), 7))
      return 2;
  }
  fclose(f);
  int rc = 0;
  World w1, w2;
  try {
    const orbx::CameraModel cam{458.654, 457.296, 367.215, 248.375, 0.11007};
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    FILE* o = fopen((dir + "/map_fuse_out.bin").c_str(), "wb");
    if (!o) return 2;
    {
      orbx::MapPointStore store(h, in.capacity);
      w1.build(h, store, in);
      const orbx::MapFuse r = orbx::map_fuse(h, cam, store, w1.kfs, {in.cur}, in.nb, in.radius_scale);
      wr(o, std::vector<int>{r.P, r.matches, r.added, (int)r.goner.size()});
      wr(o, r.list_slot); wr(o, r.match); wr(o, r.goner); wr(o, r.keeper);
      w1.dump(o, h, store, in.capacity);
      w1.close();
    }
    {
      orbx::MapPointStore store(h, in.capacity);
      w2.build(h, store, in);
      const orbx::MapSearchInNeighbors r = orbx::map_search_in_neighbors(h, cam, store, w2.kfs, in.cur, in.nb, in.radius_scale, in.scale_range, in.normals);
      wr(o, std::vector<int>(r.counts, r.counts + 8));
      wr(o, r.goner_a); wr(o, r.keeper_a); wr(o, r.goner_b); wr(o, r.keeper_b); wr(o, r.affected);
      wr(o, r.refresh.mp_descriptors); wr(o, r.refresh.normals); wr(o, r.refresh.min_distance); wr(o, r.refresh.max_distance); wr(o, r.refresh.records);
      wr(o, std::vector<int>{(int)r.num_fused(), (int)r.num_observations_added()});
      w2.dump(o, h, store, in.capacity);
      w2.close();
    }
    fclose(o);
  } catch (const std::exception& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    rc = 1;
  }
  w1.close(); w2.close();
  if (rc) return rc;
  printf("MAP_FUSE_DRIVER_OK\n");
  return 0;
}
