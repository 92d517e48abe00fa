// What a caller has without orbx_refresh_map_points: a compiled loop of its specification (include/orbx.h) over the same arrays in
// host memory — the keyframes' descriptors downloaded beforehand — on `threads` host threads (points dealt out in contiguous
// ranges).  One IEEE operation at a time (built with -ffp-contract=off).  Built and loaded by scripts/map_point_refresh_rate.py.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "orbx.h"

static inline unsigned hamming(const uint8_t* a, const uint8_t* b) {
  uint64_t x[4], y[4];
  memcpy(x, a, 32); memcpy(y, b, 32);
  return (unsigned)(__builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) +
                    __builtin_popcountll(x[3] ^ y[3]));
}

extern "C" int mp_refresh_host_loop(int M, const double* positions, const int* obs_start, const int* obs_kf, const int* obs_feat, int T,
                                    const double* kf_poses_wc, const int* kf_feat_offset, const uint8_t* descs, double scale_range,
                                    uint8_t* mp_desc, double* normals, double* min_distance, double* max_distance,
                                    orbx_mp_refresh_record* records, int threads) {
  auto work = [&](int t) {
    const int lo = (int)((long long)M * t / threads), hi = (int)((long long)M * (t + 1) / threads);
    std::vector<const uint8_t*> rows;
    std::vector<int> at;
    for (int p = lo; p < hi; ++p) {
      rows.clear(); at.clear();
      double sx = 0.0, sy = 0.0, sz = 0.0, mn = INFINITY, mx = 0.0;
      unsigned n_observers = 0;
      for (int o = obs_start[p]; o < obs_start[p + 1]; ++o) {
        const int kf = obs_kf[o], feat = obs_feat[o];
        if (kf < 0 || kf >= T) continue;
        ++n_observers;
        const double dx = positions[3 * p] - kf_poses_wc[7 * kf + 4], dy = positions[3 * p + 1] - kf_poses_wc[7 * kf + 5],
                     dz = positions[3 * p + 2] - kf_poses_wc[7 * kf + 6];
        const double dist = std::sqrt((dx * dx + dy * dy) + dz * dz);
        if (dist > 1e-10) {
          sx += dx / dist; sy += dy / dist; sz += dz / dist;
          mn = dist < mn ? dist : mn; mx = dist > mx ? dist : mx;
        }
        if (feat >= 0 && feat < kf_feat_offset[kf + 1] - kf_feat_offset[kf]) {
          rows.push_back(descs + 32 * ((size_t)kf_feat_offset[kf] + (size_t)feat)); at.push_back(o - obs_start[p]);
        }
      }
      int chosen = -1;
      unsigned best = 0xffffffffu;
      for (size_t i = 0; i < rows.size(); ++i) {
        unsigned m = 0;
        for (size_t j = 0; j < rows.size(); ++j)
          if (i != j) { const unsigned d = hamming(rows[i], rows[j]); m = d > m ? d : m; }
        if (m < best) { best = m; chosen = (int)i; }
      }
      if (chosen >= 0) memcpy(mp_desc + 32 * (size_t)p, rows[(size_t)chosen], 32);
      const double norm = std::sqrt((sx * sx + sy * sy) + sz * sz);
      if (norm > 1e-10) { normals[3 * p] = sx / norm; normals[3 * p + 1] = sy / norm; normals[3 * p + 2] = sz / norm; }
      min_distance[p] = mn / scale_range; max_distance[p] = mx * scale_range;
      records[p].chosen = chosen >= 0 ? at[(size_t)chosen] : -1; records[p].best_max_dist = chosen >= 0 ? best : 0;
      records[p].n_desc = (uint32_t)rows.size(); records[p].n_observers = n_observers;
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  return 0;
}
