// Driver for the C++ mirror of triangulate_from_neighbors (include/orbx.hpp): reads a current keyframe and its neighbours from
// <dir>/tri_in.bin, puts their features into device memory, makes orbx_keyframes, runs orbx::triangulate_from_neighbors and writes
// the new points to <dir>/tri_nb_out.bin.  Run by tests/test_triangulate_cpp.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "orbx.hpp"

// the three runtime calls the driver needs to place the features on the GPU (libamdhip64; hipMemcpyHostToDevice = 1)
extern "C" {
int hipMalloc(void** p, size_t bytes);
int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);
int hipFree(void* p);
}

struct HostKf {
  int n = 0, has_nodes = 0;
  double pose[7];
  std::vector<orbx_keypoint> kp;
  std::vector<uint8_t> desc, has, mp;
  std::vector<double> pts;
  std::vector<uint32_t> node;
};

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void* to_device(const void* src, size_t bytes) {
  void* d = nullptr;
  if (bytes == 0) return nullptr;
  if (hipMalloc(&d, bytes) != 0 || hipMemcpy(d, src, bytes, 1) != 0) { fprintf(stderr, "device upload failed\n"); exit(3); }
  return d;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  FILE* f = fopen((dir + "/tri_in.bin").c_str(), "rb");
  if (!f) return 2;
  int T = 0, inertial = 0;
  orbx::CameraModel cam{};
  double c5[5];
  if (!rd(f, &T, 1) || !rd(f, &inertial, 1) || !rd(f, c5, 5)) return 2;
  cam.fx = c5[0]; cam.fy = c5[1]; cam.cx = c5[2]; cam.cy = c5[3]; cam.baseline = c5[4];
  std::vector<HostKf> kfs((size_t)T + 1);
  for (HostKf& k : kfs) {
    if (!rd(f, &k.n, 1) || !rd(f, &k.has_nodes, 1) || !rd(f, k.pose, 7)) return 2;
    const size_t n = (size_t)k.n;
    k.kp.resize(n); k.desc.resize(32 * n); k.pts.resize(3 * n); k.has.resize(n); k.mp.resize(n); k.node.resize(k.has_nodes ? n : 0);
    if (!rd(f, k.kp.data(), n) || !rd(f, k.desc.data(), 32 * n) || !rd(f, k.pts.data(), 3 * n) || !rd(f, k.has.data(), n) || !rd(f, k.mp.data(), n) ||
        !rd(f, k.node.data(), k.node.size()))
      return 2;
  }
  fclose(f);
  try {
    orbx::Handle h(cam, 1000, 0, 752, 480, 1);
    std::vector<orbx_keyframe*> made;
    std::vector<void*> dev;
    for (size_t i = 0; i < kfs.size(); ++i) {
      const HostKf& k = kfs[i];
      const size_t n = (size_t)k.n;
      void* d_kp = to_device(k.kp.data(), sizeof(orbx_keypoint) * n); void* d_desc = to_device(k.desc.data(), 32 * n);
      void* d_pts = to_device(k.pts.data(), 24 * n); void* d_has = to_device(k.has.data(), n);
      for (void* p : {d_kp, d_desc, d_pts, d_has}) dev.push_back(p);
      orbx_keyframe* kf = nullptr;
      h.check(orbx_keyframe_create(h.get(), (const orbx_keypoint*)d_kp, (const uint8_t*)d_desc, k.n, (const double*)d_pts, (const uint8_t*)d_has, 100 + i, 0,
                                   k.pose, &kf));
      std::vector<int64_t> ids(n);
      for (size_t j = 0; j < n; ++j) ids[j] = k.mp[j] ? 7 : -1;
      if (n) h.check(orbx_keyframe_set_map_points(kf, ids.data()));
      if (k.has_nodes) h.check(orbx_keyframe_set_feature_nodes(kf, k.node.data()));
      made.push_back(kf);
    }
    orbx::TriangulationResult res;
    const std::vector<const orbx_keyframe*> nbs(made.begin() + 1, made.end());
    const std::vector<orbx::NewMapPoint> pts = orbx::triangulate_from_neighbors(h, cam, orbx::TriangulationConfig(), inertial != 0, made[0], nbs, res);
    FILE* o = fopen((dir + "/tri_nb_out.bin").c_str(), "wb");
    if (!o) return 2;
    const uint64_t head[6] = {pts.size(), res.num_new_points, res.num_pairs_checked, res.num_matches_found, res.num_triangulated, res.num_validated};
    fwrite(head, 8, 6, o);
    for (const orbx::NewMapPoint& p : pts) {
      const int32_t idx[4] = {(int32_t)p.neighbour_index, (int32_t)p.idx1, (int32_t)p.idx2, 0};
      fwrite(idx, 4, 4, o); fwrite(p.position.data(), 8, 3, o);
    }
    fclose(o);
    for (orbx_keyframe* kf : made) orbx_keyframe_destroy(kf);
    for (void* p : dev) if (p) hipFree(p);
  } catch (const orbx::Error& e) {
    fprintf(stderr, "orbx error: %s\n", e.what());
    return 1;
  }
  printf("TRIANGULATE_DRIVER_OK\n");
  return 0;
}
