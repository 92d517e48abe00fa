// mappoint_kernels.hip — phase 4 of search_in_neighbors (src/local_mapping/search_in_neighbors.rs:139-150) for a batch of map
// points: Map::compute_distinctive_descriptors (src/atlas/map/map.rs:880-944) and Map::update_map_point_normal_and_depth
// (map.rs:716-742, src/atlas/map/map_point.rs:173-203).  The specification is in include/orbx.h (orbx_refresh_map_points).
//
// The keyframes are a table of T (descriptor base pointer, feature count, camera centre) uploaded per call; a descriptor row is
// read where it lies — a slice of a packed array or a resident orbx_keyframe's block.
//
//   mp_refresh_kernel       points of at most MP_SHORT observations.  One thread per observation; a workgroup owns the points whose
//                           obs_start lies in its window of MP_WIN observations and finds them by binary search in obs_start, so it
//                           stages at most MP_WIN + MP_SHORT - 1 rows.  Every thread gathers its row and its unit viewing direction
//                           into LDS once, then walks its point's other rows (all lanes of a point read the same LDS row per step:
//                           a broadcast) for the largest distance.  One thread per owned point then takes the argmin and sums the
//                           directions in list order.  A longer point is appended to the long list instead.
//   mp_refresh_long_kernel  one workgroup per listed point at a time: every thread keeps rows i0 + tid in registers while the point's
//                           rows pass through LDS in tiles of MP_LONG_THREADS, so any track length works; the argmin over
//                           (largest distance, position) is one 64-bit LDS minimum, the direction sum is thread 0's, tile by tile.
#include <algorithm>
#include <cmath>
#include <vector>

#include "orbx_internal.hpp"

namespace {

constexpr int MP_WIN = 256;                          // observations whose points a workgroup of mp_refresh_kernel owns
constexpr int MP_SHORT = 64;                         // longest point of mp_refresh_kernel
constexpr int MP_STAGE = MP_WIN + MP_SHORT - 1;      // rows a workgroup can need: a point that starts at the window's last observation
constexpr int MP_THREADS = 320;                      // >= MP_STAGE, whole waves
constexpr int MP_LONG_THREADS = 256;
constexpr int MP_MAX_OBS = 0x7fff0000;               // window arithmetic stays inside int
constexpr unsigned MP_NO_DESC = 0xffffffffu;
constexpr unsigned MP_KF_OK = 1u, MP_DESC_OK = 2u;
static_assert(MP_THREADS >= MP_STAGE && MP_THREADS % 64 == 0, "one thread per staged observation");

struct MpArgs {
  int M, N, T, long_cap;
  const double* positions; const int* obs_start; const int* obs_kf; const int* obs_feat;
  const MapPointKf* kfs;
  double scale_range;
  const uint8_t* desc_in; const double* normals_in;      // the values a point keeps; may be the outputs themselves
  uint8_t* desc_out; double* normals_out; double* min_distance; double* max_distance; orbx_mp_refresh_record* records;
  int* n_long; int* long_list;
};

// first p in [lo, hi) with off[p] >= v
__device__ __forceinline__ int mp_lower_bound(const int* off, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (off[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ unsigned mp_hamming(const unsigned long long* a, const unsigned long long* b) {
  return (unsigned)(__popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]));
}

// One observation of point p: which of (keyframe found, descriptor row exists) hold, the row's address, and
// dir = (dx, dy, dz) / dist | dist, with dist = 0 for an observer that is missing or not farther than 1e-10.
__device__ __forceinline__ unsigned mp_observe(const MpArgs& A, int o, double px, double py, double pz, const unsigned long long** row, double* dir) {
  const int kf = A.obs_kf[o], feat = A.obs_feat[o];
  dir[0] = dir[1] = dir[2] = dir[3] = 0.0;
  if ((unsigned)kf >= (unsigned)A.T) return 0u;
  const MapPointKf K = A.kfs[kf];
  const double dx = px - K.centre[0], dy = py - K.centre[1], dz = pz - K.centre[2];
  const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
  if (dist > 1e-10) { dir[0] = dx / dist; dir[1] = dy / dist; dir[2] = dz / dist; dir[3] = dist; }
  if ((unsigned)feat >= (unsigned)K.n) return MP_KF_OK;
  *row = reinterpret_cast<const unsigned long long*>(K.desc + (size_t)feat * 32);
  return MP_KF_OK | MP_DESC_OK;
}

// The direction sum of map_point.rs:179-192, one observer at a time in list order.
struct MpSum {
  double sx = 0.0, sy = 0.0, sz = 0.0, mn = INFINITY, mx = 0.0;
  __device__ __forceinline__ void add(const double* dir) {
    const double dist = dir[3];
    if (dist > 1e-10) {
      sx += dir[0]; sy += dir[1]; sz += dir[2];
      mn = dist < mn ? dist : mn;
      mx = dist > mx ? dist : mx;
    }
  }
};

// Everything a point's call writes.  row: the chosen descriptor (chosen >= 0).
__device__ __forceinline__ void mp_write_point(const MpArgs& A, int p, int chosen, unsigned best, unsigned n_desc, unsigned n_observers,
                                               const unsigned long long* row, const MpSum& s) {
  const unsigned long long* keep = chosen >= 0 ? row : reinterpret_cast<const unsigned long long*>(A.desc_in + (size_t)p * 32);
  unsigned long long* dout = reinterpret_cast<unsigned long long*>(A.desc_out + (size_t)p * 32);
  if (keep != dout) { dout[0] = keep[0]; dout[1] = keep[1]; dout[2] = keep[2]; dout[3] = keep[3]; }
  const double norm = sqrt((s.sx * s.sx + s.sy * s.sy) + s.sz * s.sz);
  double nx, ny, nz;
  if (norm > 1e-10) { nx = s.sx / norm; ny = s.sy / norm; nz = s.sz / norm; }
  else { nx = A.normals_in[3 * (size_t)p]; ny = A.normals_in[3 * (size_t)p + 1]; nz = A.normals_in[3 * (size_t)p + 2]; }
  A.normals_out[3 * (size_t)p] = nx; A.normals_out[3 * (size_t)p + 1] = ny; A.normals_out[3 * (size_t)p + 2] = nz;
  A.min_distance[p] = s.mn / A.scale_range;
  A.max_distance[p] = s.mx * A.scale_range;
  orbx_mp_refresh_record r;
  r.chosen = chosen; r.best_max_dist = best; r.n_desc = n_desc; r.n_observers = n_observers;
  A.records[p] = r;
}

__global__ __launch_bounds__(MP_THREADS) void mp_refresh_kernel(MpArgs A) {
  __shared__ unsigned long long s_row[MP_STAGE][4];
  __shared__ double s_dir[MP_STAGE][4];
  __shared__ unsigned s_max[MP_STAGE];                 // largest distance to the point's other rows; MP_NO_DESC: no row
  __shared__ unsigned s_flag[MP_STAGE];
  const int tid = threadIdx.x, base = blockIdx.x * MP_WIN;
  const int p_lo = mp_lower_bound(A.obs_start, 0, A.M, base), p_hi = mp_lower_bound(A.obs_start, p_lo, A.M, base + MP_WIN);
  // this thread's observation and the owned point it belongs to: the last one that starts at or before it
  const int o = base + tid;
  int s = 0, e = 0;
  bool mine = false;
  if (tid < MP_STAGE && o < A.N && p_lo < p_hi) {
    const int p = mp_lower_bound(A.obs_start, p_lo, p_hi, o + 1) - 1;
    if (p >= p_lo) {
      s = A.obs_start[p]; e = A.obs_start[p + 1];
      mine = o < e && e - s <= MP_SHORT;
      if (mine) {
        const unsigned long long* row = nullptr;
        const unsigned f = mp_observe(A, o, A.positions[3 * (size_t)p], A.positions[3 * (size_t)p + 1], A.positions[3 * (size_t)p + 2], &row, s_dir[tid]);
        s_flag[tid] = f;
        if (f & MP_DESC_OK) { s_row[tid][0] = row[0]; s_row[tid][1] = row[1]; s_row[tid][2] = row[2]; s_row[tid][3] = row[3]; }
      }
    }
  }
  __syncthreads();
  if (mine) {
    unsigned mx = MP_NO_DESC;
    if (s_flag[tid] & MP_DESC_OK) {
      mx = 0;
      for (int j = s - base; j < e - base; ++j)
        if (j != tid && (s_flag[j] & MP_DESC_OK)) mx = max(mx, mp_hamming(s_row[tid], s_row[j]));
    }
    s_max[tid] = mx;
  }
  __syncthreads();
  for (int p = p_lo + tid; p < p_hi; p += MP_THREADS) {
    const int ps = A.obs_start[p], n = A.obs_start[p + 1] - ps;
    if (n > MP_SHORT) {
      const int slot = atomicAdd(A.n_long, 1);
      if (slot < A.long_cap) A.long_list[slot] = p;
      continue;
    }
    int chosen = -1;
    unsigned best = MP_NO_DESC, n_desc = 0, n_observers = 0;
    MpSum sum;
    for (int k = 0; k < n; ++k) {
      const int j = ps - base + k;
      const unsigned f = s_flag[j];
      if (f & MP_DESC_OK) {
        ++n_desc;
        if (s_max[j] < best) { best = s_max[j]; chosen = k; }        // strict: the earliest of equal maxima
      }
      if (f & MP_KF_OK) { ++n_observers; sum.add(s_dir[j]); }
    }
    mp_write_point(A, p, chosen, chosen >= 0 ? best : 0u, n_desc, n_observers, s_row[chosen >= 0 ? ps - base + chosen : 0], sum);
  }
}

__global__ __launch_bounds__(MP_LONG_THREADS) void mp_refresh_long_kernel(MpArgs A) {
  __shared__ unsigned long long s_row[MP_LONG_THREADS][4];
  __shared__ double s_dir[MP_LONG_THREADS][4];
  __shared__ unsigned s_flag[MP_LONG_THREADS];
  __shared__ unsigned long long s_key;                 // min over rows of (largest distance << 32 | position)
  __shared__ unsigned s_cnt;
  const int tid = threadIdx.x;
  const int n_long = min(*A.n_long, A.long_cap);
  for (int li = blockIdx.x; li < n_long; li += gridDim.x) {
    const int p = A.long_list[li];
    const int s = max(A.obs_start[p], 0), n = min(A.obs_start[p + 1], A.N) - s;
    const double px = A.positions[3 * (size_t)p], py = A.positions[3 * (size_t)p + 1], pz = A.positions[3 * (size_t)p + 2];
    if (tid == 0) { s_key = ~0ull; s_cnt = 0; }
    // ---- descriptors: rows i0 + tid in registers against every row, tile by tile
    for (int i0 = 0; i0 < n; i0 += MP_LONG_THREADS) {
      const int i = i0 + tid;
      unsigned long long w[4] = {0, 0, 0, 0};
      bool have = false;
      if (i < n) {
        const unsigned long long* row = nullptr;
        double dir[4];
        have = (mp_observe(A, s + i, px, py, pz, &row, dir) & MP_DESC_OK) != 0;
        if (have) { w[0] = row[0]; w[1] = row[1]; w[2] = row[2]; w[3] = row[3]; }
      }
      unsigned mx = 0;
      for (int j0 = 0; j0 < n; j0 += MP_LONG_THREADS) {
        __syncthreads();                                                   // the tile before is read, s_key is set
        unsigned f = 0;
        if (j0 + tid < n) {
          const unsigned long long* row = nullptr;
          double dir[4];
          f = mp_observe(A, s + j0 + tid, px, py, pz, &row, dir);
          if (f & MP_DESC_OK) { s_row[tid][0] = row[0]; s_row[tid][1] = row[1]; s_row[tid][2] = row[2]; s_row[tid][3] = row[3]; }
        }
        s_flag[tid] = f;
        __syncthreads();
        if (have) {
          const int m = min(MP_LONG_THREADS, n - j0);
          for (int k = 0; k < m; ++k)
            if ((s_flag[k] & MP_DESC_OK) && j0 + k != i) mx = max(mx, mp_hamming(w, s_row[k]));
        }
      }
      if (have) {
        atomicMin(&s_key, ((unsigned long long)mx << 32) | (unsigned)i);
        atomicAdd(&s_cnt, 1u);
      }
    }
    // ---- directions: computed by all threads, summed by thread 0 in list order
    MpSum sum;
    unsigned n_observers = 0;
    for (int k0 = 0; k0 < n; k0 += MP_LONG_THREADS) {
      __syncthreads();
      unsigned f = 0;
      if (k0 + tid < n) {
        const unsigned long long* row = nullptr;
        f = mp_observe(A, s + k0 + tid, px, py, pz, &row, s_dir[tid]);
      }
      s_flag[tid] = f;
      __syncthreads();
      if (tid == 0) {
        const int m = min(MP_LONG_THREADS, n - k0);
        for (int k = 0; k < m; ++k)
          if (s_flag[k] & MP_KF_OK) { ++n_observers; sum.add(s_dir[k]); }
      }
    }
    __syncthreads();                                                       // every row's minimum is in s_key
    if (tid == 0) {
      const unsigned n_desc = s_cnt;
      const int chosen = n_desc ? (int)(unsigned)(s_key & 0xffffffffu) : -1;
      const unsigned long long* row = nullptr;
      if (chosen >= 0) { double dir[4]; mp_observe(A, s + chosen, px, py, pz, &row, dir); }
      mp_write_point(A, p, chosen, n_desc ? (unsigned)(s_key >> 32) : 0u, n_desc, n_observers, row, sum);
    }
    __syncthreads();                                                       // before the next point resets s_key
  }
}

}  // namespace

int mp_refresh_enqueue(orbx_handle* h, const char* who, int M, int n_obs, const double* d_positions, const int* d_obs_start,
                       const int* d_obs_kf, const int* d_obs_feat, int T, const MapPointKf* kfs, double scale_range,
                       const uint8_t* d_desc_in, const double* d_normals_in, uint8_t* d_mp_desc, double* d_normals, double* d_min_distance,
                       double* d_max_distance, orbx_mp_refresh_record* d_records) {
  if (M < 1 || n_obs < 0 || n_obs > MP_MAX_OBS || T < 0 || !d_positions || !d_obs_start || (n_obs > 0 && (!d_obs_kf || !d_obs_feat)) ||
      (T > 0 && !kfs) || !d_desc_in || !d_normals_in || !d_mp_desc || !d_normals || !d_min_distance || !d_max_distance || !d_records)
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (at most %d observations)", who, MP_MAX_OBS);
  for (int t = 0; t < T; ++t)
    if (kfs[t].n < 0 || (kfs[t].n > 0 && !kfs[t].desc)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad keyframe %d", who, t);
  ORBX_HIP(h, hipSetDevice(h->device));
  // the keyframe table goes up through the upload ring, so that the caller's arrays are free when the call returns
  const size_t tab_bytes = sizeof(MapPointKf) * (size_t)std::max(T, 1);
  uint8_t *hs, *ds;
  if (int rc = orbx_ring_begin(h, h->ring_mp, h->ws_mp[2], tab_bytes, &hs, &ds)) return rc;
  if (T > 0) std::memcpy(hs, kfs, sizeof(MapPointKf) * (size_t)T);
  if (int rc = orbx_ring_commit(h, h->ring_mp, h->ws_mp[2], tab_bytes)) return rc;
  const int long_cap = n_obs / (MP_SHORT + 1);                                // no more points than this are longer than MP_SHORT
  Carve ws;
  const size_t o_cnt = ws.take(sizeof(int)), o_list = ws.take(sizeof(int) * (size_t)long_cap);
  if (int rc = orbx_reserve(h, h->ws_mp[0], ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_mp[0].p;
  MpArgs A{};
  A.M = M; A.N = n_obs; A.T = T; A.long_cap = long_cap;
  A.positions = d_positions; A.obs_start = d_obs_start; A.obs_kf = d_obs_kf; A.obs_feat = d_obs_feat;
  A.kfs = (const MapPointKf*)ds;
  A.scale_range = scale_range;
  A.desc_in = d_desc_in; A.normals_in = d_normals_in;
  A.desc_out = d_mp_desc; A.normals_out = d_normals; A.min_distance = d_min_distance; A.max_distance = d_max_distance; A.records = d_records;
  A.n_long = (int*)(w + o_cnt); A.long_list = (int*)(w + o_list);
  ORBX_HIP(h, hipMemsetAsync(A.n_long, 0, sizeof(int), h->stream));
  // the window that holds obs_start == n_obs (trailing points without observations) is launched too
  orbx_launch(h, "mp_refresh_kernel", false, mp_refresh_kernel, dim3(n_obs / MP_WIN + 1), dim3(MP_THREADS), 0, A);
  if (long_cap > 0) orbx_launch(h, "mp_refresh_long_kernel", true, mp_refresh_long_kernel, dim3(std::min(long_cap, 4 * h->n_cu)), dim3(MP_LONG_THREADS), 0, A);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

int mp_refresh_host_call(orbx_handle* h, const char* who, int M, const double* positions, const int* obs_start, const int* obs_kf,
                         const int* obs_feat, int T, MapPointKf* kfs, const int* kf_feat_offset, const uint8_t* descs, double scale_range,
                         uint8_t* mp_desc, double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records) {
  if (int rc = orbx_check_offsets(h, who, "obs_start", "point", M, obs_start)) return rc;
  const size_t P = (size_t)M, N = (size_t)obs_start[M], F = kf_feat_offset ? (size_t)kf_feat_offset[T] : 0;
  if (!positions || !mp_desc || !normals || !min_distance || !max_distance || !records || (N > 0 && (!obs_kf || !obs_feat)) || (F > 0 && !descs))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  ORBX_HIP(h, hipSetDevice(h->device));
  // one blob each way: [positions | obs_start | obs_kf | obs_feat | mp_desc | normals | descs] up,
  // [mp_desc | normals | min_distance | max_distance | records] down
  Carve in, out;
  const size_t i_pos = in.take(24 * P), i_os = in.take(4 * (P + 1)), i_ok = in.take(4 * N), i_of = in.take(4 * N), i_md = in.take(32 * P),
               i_nr = in.take(24 * P), i_ds = in.take(32 * F);
  const size_t o_md = out.take(32 * P), o_nr = out.take(24 * P), o_mn = out.take(8 * P), o_mx = out.take(8 * P),
               o_rc = out.take(sizeof(orbx_mp_refresh_record) * P);
  HostCall c;
  if (int rc = orbx_host_call_begin(h, h->pin_mp, h->ws_mp[1], in.off, out.off, c)) return rc;
  uint8_t *hi = c.hi, *ho = c.ho, *di = c.di, *dout = c.dout;
  std::memcpy(hi + i_pos, positions, 24 * P);
  std::memcpy(hi + i_os, obs_start, 4 * (P + 1));
  if (N) { std::memcpy(hi + i_ok, obs_kf, 4 * N); std::memcpy(hi + i_of, obs_feat, 4 * N); }
  std::memcpy(hi + i_md, mp_desc, 32 * P);
  std::memcpy(hi + i_nr, normals, 24 * P);
  if (F) {
    std::memcpy(hi + i_ds, descs, 32 * F);
    for (int t = 0; t < T; ++t) kfs[t].desc = di + i_ds + 32 * (size_t)kf_feat_offset[t];
  }
  if (int rc = orbx_host_call_upload(h, c)) return rc;
  if (int rc = mp_refresh_enqueue(h, who, M, (int)N, (const double*)(di + i_pos), (const int*)(di + i_os), (const int*)(di + i_ok),
                                  (const int*)(di + i_of), T, kfs, scale_range, di + i_md, (const double*)(di + i_nr), dout + o_md,
                                  (double*)(dout + o_nr), (double*)(dout + o_mn), (double*)(dout + o_mx), (orbx_mp_refresh_record*)(dout + o_rc)))
    return rc;
  if (int rc = orbx_host_call_download(h, c, out.off)) return rc;
  std::memcpy(mp_desc, ho + o_md, 32 * P);
  std::memcpy(normals, ho + o_nr, 24 * P);
  std::memcpy(min_distance, ho + o_mn, 8 * P);
  std::memcpy(max_distance, ho + o_mx, 8 * P);
  std::memcpy(records, ho + o_rc, sizeof(orbx_mp_refresh_record) * P);
  return ORBX_OK;
}

// the table of the packed forms: keyframe t owns rows [kf_feat_offset[t], kf_feat_offset[t + 1]) of descs (NULL: filled by
// mp_refresh_host_call once the rows have a device address), its camera centre is the translation of its T_wc
static int mp_packed_table(orbx_handle* h, const char* who, int T, const double* kf_poses_wc, const int* kf_feat_offset, const uint8_t* d_descs,
                           std::vector<MapPointKf>& kfs) {
  if (T < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  kfs.assign((size_t)T, MapPointKf{});
  if (T == 0) return ORBX_OK;
  if (!kf_poses_wc) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  if (int rc = orbx_check_offsets(h, who, "kf_feat_offset", "keyframe", T, kf_feat_offset)) return rc;
  for (int t = 0; t < T; ++t) {
    MapPointKf& k = kfs[(size_t)t];
    k.desc = d_descs ? d_descs + 32 * (size_t)kf_feat_offset[t] : nullptr;
    k.n = kf_feat_offset[t + 1] - kf_feat_offset[t];
    std::memcpy(k.centre, kf_poses_wc + 7 * (size_t)t + 4, sizeof(k.centre));
  }
  return ORBX_OK;
}

extern "C" {

int orbx_refresh_map_points_device(orbx_handle* h, int M, int n_obs, const double* d_positions, const int* d_obs_start, const int* d_obs_kf,
                                   const int* d_obs_feat, int T, const double* kf_poses_wc, const int* kf_feat_offset, const uint8_t* d_descs,
                                   double scale_range, uint8_t* d_mp_desc, double* d_normals, double* d_min_distance, double* d_max_distance,
                                   orbx_mp_refresh_record* d_records) {
  static const char* who = "orbx_refresh_map_points_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (M < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (M == 0) return ORBX_OK;
    std::vector<MapPointKf> kfs;
    if (int rc = mp_packed_table(h, who, T, kf_poses_wc, kf_feat_offset, d_descs, kfs)) return rc;
    if (T > 0 && kf_feat_offset[T] > 0 && !d_descs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    return mp_refresh_enqueue(h, who, M, n_obs, d_positions, d_obs_start, d_obs_kf, d_obs_feat, T, kfs.data(), scale_range, d_mp_desc, d_normals,
                              d_mp_desc, d_normals, d_min_distance, d_max_distance, d_records);
  });
}

int orbx_refresh_map_points(orbx_handle* h, int M, const double* positions, const int* obs_start, const int* obs_kf, const int* obs_feat, int T,
                            const double* kf_poses_wc, const int* kf_feat_offset, const uint8_t* descs, double scale_range, uint8_t* mp_desc,
                            double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records) {
  static const char* who = "orbx_refresh_map_points";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (M < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (M == 0) return ORBX_OK;
    std::vector<MapPointKf> kfs;
    if (int rc = mp_packed_table(h, who, T, kf_poses_wc, kf_feat_offset, nullptr, kfs)) return rc;
    return mp_refresh_host_call(h, who, M, positions, obs_start, obs_kf, obs_feat, T, kfs.data(), T > 0 ? kf_feat_offset : nullptr, descs,
                                scale_range, mp_desc, normals, min_distance, max_distance, records);
  });
}

}  // extern "C"
