// Host-only test driver for the two snapshot helpers of include/orbx_map.hpp behind the map-point refresh:
// search_in_neighbors_affected and collect_map_point_refresh.  Reads a MapSnapshot written by api.MapSnapshot.to_bytes().
//   driver <snapshot.bin> <current_kf_id> <out.bin> [neighbour ids ...]   plus one id the snapshot does not hold is appended to the request
// out.bin: [n_affected] affected ids | [n_mp, n_obs, n_kf] | mp ids | kf ids | positions f64 [n_mp][3] | obs_start i32 [n_mp+1] | obs_kf i32 | obs_feat i32
// No library call is made: it links without liborbx_hip.so and runs without a GPU (also built with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "orbx_map.hpp"

template <class T> static void take(const uint8_t*& p, std::vector<T>& v, uint64_t n) { v.resize(n); if (n) memcpy(v.data(), p, n * sizeof(T)); p += n * sizeof(T); }
template <class T> static void put(FILE* f, const T* p, size_t n) { if (n) fwrite(p, sizeof(T), n, f); }

static orbx::MapSnapshot load(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> b((size_t)n);
  if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) exit(2);
  fclose(f);
  uint64_t c[22];
  memcpy(c, b.data(), sizeof(c));                                          // 21 element counts + imu_initialized
  const uint8_t* p = b.data() + sizeof(c);
  orbx::MapSnapshot m;
  take(p, m.kf_ids, c[0]); take(p, m.kf_bad, c[1]); take(p, m.kf_pose_wc, c[2]); take(p, m.kf_n_keypoints, c[3]);
  take(p, m.kf_feat_start, c[4]); take(p, m.feat_mp_id, c[5]); take(p, m.feat_uv, c[6]); take(p, m.cov_start, c[7]);
  take(p, m.cov_kf_id, c[8]); take(p, m.mp_ids, c[9]); take(p, m.mp_bad, c[10]); take(p, m.mp_pos, c[11]);
  take(p, m.mp_obs_start, c[12]); take(p, m.mp_obs_kf_id, c[13]);
  take(p, m.kf_prev_id, c[14]); take(p, m.kf_velocity, c[15]); take(p, m.kf_bias, c[16]); take(p, m.kf_has_preint, c[17]);
  take(p, m.kf_preint, c[18]); take(p, m.feat_stereo, c[19]); take(p, m.mp_obs_feat_idx, c[20]);
  m.imu_initialized = c[21] != 0;
  m.build_index();
  return m;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <snapshot.bin> <current_kf_id> <out.bin> [neighbour ids ...]\n", argv[0]); return 2; }
  const orbx::MapSnapshot m = load(argv[1]);
  std::vector<orbx::KeyFrameId> neighbours;
  for (int i = 4; i < argc; ++i) neighbours.push_back(strtoull(argv[i], nullptr, 10));
  std::vector<orbx::MapPointId> affected = orbx::search_in_neighbors_affected(m, strtoull(argv[2], nullptr, 10), neighbours);
  FILE* f = fopen(argv[3], "wb");
  if (!f) return 2;
  const uint64_t na = affected.size();
  put(f, &na, 1); put(f, affected.data(), affected.size());
  affected.push_back(31337);                                               // a point that is gone: left out
  const orbx::MapPointRefreshData d = orbx::collect_map_point_refresh(m, affected);
  const uint64_t head[3] = {d.mp_ids.size(), d.obs_kf.size(), d.kf_ids.size()};
  put(f, head, 3); put(f, d.mp_ids.data(), d.mp_ids.size()); put(f, d.kf_ids.data(), d.kf_ids.size());
  for (const auto& p : d.positions) put(f, p.data(), 3);
  put(f, d.obs_start.data(), d.obs_start.size()); put(f, d.obs_kf.data(), d.obs_kf.size()); put(f, d.obs_feat.data(), d.obs_feat.size());
  fclose(f);
  return 0;
}
