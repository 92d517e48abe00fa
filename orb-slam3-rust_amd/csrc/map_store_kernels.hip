// map_store_kernels.hip — orbx_map_points: map points resident on the device, and the calls that turn "these keyframes" or "these
// slots" into a frame's list of map points without a host round trip (include/orbx.h, "resident map points").
//
// Replaces, per frame and with no host synchronisation inside:
//   src/tracking/tracker.rs:826-867    track_local_map: get_map_points_from_keyframes (map.rs:492-504), the lookups, the two arrays
//   src/tracking/tracker.rs:1093-1102  track_with_motion_model: the previous frame's matched points, looked up
//   src/tracking/tracker.rs:1024-1036  track_with_reference_kf: kf.get_map_point(i) and the map lookup per keyframe feature
//
// The selection is three launches over (chunk of MS_CHUNK candidates, frame); a candidate is one feature of one of the frame's
// keyframes (or one entry of its slot array), numbered in walking order:
//   map_mark_kernel   (keyframes only) slot of every candidate; first[frame][slot] = atomicMin(candidate number) — the table says
//                     where a slot was first seen, whatever the execution order
//   map_flag_kernel   a candidate survives iff the table holds its own number; the survivor puts the table's entry back to EMPTY,
//                     so that a call leaves the table as it found it and costs what its candidates cost, not what the map holds;
//                     per chunk the number of survivors
//   map_emit_kernel   a chunk's base = the survivors of all chunks before it (earlier frames, then earlier chunks; block_sum);
//                     ordered compaction inside the chunk behind it (BlockScan); list_slot, positions and descriptors gathered
// Every frame has a table of its own ([frame][capacity]), so frames of one call that share keyframes do not meet.  The only atomics
// are that integer min: every output is a deterministic function of the inputs.
//
// Covisibility (map.rs:339-386, :476-489; tracker.rs:826-843) counts, for a marked set of keyframes, how many of its live slots
// every other keyframe observes, and ranks the result:
//   cov_mark_kernel   (chunk of a member keyframe's features, member) mark[query][slot] = 1 for live slots; run again with 0 behind
//                     the count, so that a call leaves the table as it found it (plain stores of one value: no atomics)
//   cov_count_kernel  (keyframe k, group of COV_Q queries) walks k's de-duplicated slot table once, tests live and each query's
//                     marks, block_sum -> weights[q][k]; 0 where k is the query itself
//   cov_rank_kernel   one workgroup per query: rank(i) = #{j : w_j > w_i or (w_j == w_i and j < i)}; i goes to best[rank] when
//                     w_i > 0 and rank < n_best
//   cov_seg_kernel    one workgroup per frame: [reference] ++ best (or every keyframe) as the MapSeg / n_cand arrays that the three
//                     selection launches read, which then run unchanged; the segments' bases by BlockScan, a round per 256
// A keyframe's observed set counts a slot once: orbx_keyframe_set_map_point_slots keeps, beside the table, a copy with every repeat
// set to -1 (d_mp_uniq), so distinctness costs nothing per (query, keyframe).
//
// The local-BA window (local_ba_lm.rs:665-726, :800-897; local_mapper.rs:377-410) is one query's covisibility and one frame's
// selection, unchanged, and five launches behind them:
//   bac_index_kernel    index[slot] = position in P for the list's entries (row 0 of `first`, EMPTY between calls)
//   bac_count_kernel    (chunk of a keyframe's features, keyframe) over ALL keyframes of the call: the features whose slot — the
//                       table WITH repeats: every feature is an observation — is in range, live and indexed; per chunk the count
//   bac_order_kernel    one workgroup: every keyframe's role (anchor / optimised i / fixed j / none), the fixed keyframes by ascending
//                       position (BlockAppend), where every observer's observations start (BlockScan in observer order), K F M N
//   bac_emit_kernel     (chunk, keyframe) ordered compaction behind the observer's earlier chunks; one 16-byte store per observation
//   bac_restore_kernel  index[slot] = EMPTY again: the call leaves the table as it found it
// orbx_map_local_ba hands the observations to the solver where they lie (ba_kernels.hip: BaWinHost::obs_on_device) and scatters the
// optimised positions back through map_scatter_kernel.
// The INERTIAL window (local_inertial_ba.rs:366-429, :933-1030; local_mapper.rs:343-375) is one frame's selection over the temporal
// chain the caller names and the same five launches: bac_order_kernel<true> takes the roles from the chain (chain[0] the anchor,
// chain[i] window keyframe i), bac_emit_kernel<true> ORs has_point[feature] != 0 into mp_idx (ORBX_BA_OBS32_STEREO).
// orbx_map_local_inertial_ba hands them to the inertial solver where they lie and scatters the positions back the same way.
// Both windows are one host path: WinPlan (bac_plan / bic_plan check and size a covisible window / a chain), win_enqueue (the kind's
// selection, then the five launches), win_collect_host (the host forms) and win_local_ba (collect, download, poses, solve, write back).
// Every extern "C" entry point runs its body inside orbx_guard (orbx_internal.hpp): no C++ exception crosses the C boundary.
// The host code states three things once each (orbx_internal.hpp): a launch with its profiling scope is orbx_launch(h, label, chained,
// kernel, grid, block, lds, args...); the host tables of a device form are the pieces of an UploadPlan (put, then send, or begin /
// commit around what is made in place) on ring_map; the outputs of a host form are the pieces of an OutputPlan (add, begin, dev,
// finish, copy for a length the download tells).  Every workspace is a named member of orbx_handle::ws_map (MapWorkspaces).
// mp.observations (map_point.rs:140-156), the inverse of the slot tables, is derived the same way for the points a call names:
// the lists behind orbx_map_observations and orbx_map_refresh_points (search_in_neighbors.rs:139-150) and the counts behind
// orbx_map_keyframe_redundancy (local_mapper.rs:487-583); the kernels are described where they stand ("observations", below).
// The fuse and merge phases of search_in_neighbors (search_in_neighbors.rs:240-390, map.rs:770-868) act on the tables themselves:
// orbx_map_fuse[_device] and orbx_map_search_in_neighbors; the kernels are described where they stand ("fuse and merge", below).
// New points and removed ones are written into the tables the same way (local_mapper.rs:208-268, :421-469, map.rs:609-631):
// orbx_keyframe_set_map_point_slots_device, orbx_map_create_points[_device], orbx_map_remove_points, orbx_map_cull_points; the
// kernels are described where they stand ("creation and removal", below).
// The sums, the ordered append and the scans of counts are block_dev.hpp's: every thread of a workgroup reaches each of them.
#include <algorithm>
#include <memory>
#include <numeric>
#include <vector>

#include "block_dev.hpp"
#include "fuse_search_dev.hpp"
#include "orbx_internal.hpp"
#include "pose_dev.hpp"

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_PER = 4;                        // consecutive candidates per thread
constexpr int MS_CHUNK = MS_THREADS * MS_PER;    // candidates per workgroup
constexpr int MS_EMPTY = 0x7f7f7f7f;             // (one byte repeated: the tables are filled by a memset when they are allocated)

// One keyframe of one frame: its slot table (NULL: no table, every feature -1), the number of its first candidate, its features.
struct MapSeg {
  const int* slots;
  int base, n;
};
struct MapRefItem {
  const int* slots;
  int off, n;
};

struct SelArgs {
  int source, capacity, n_chunk;
  const uint8_t* live; const double* pos; const uint8_t* desc;
  const MapSeg* segs; const int* seg_off;        // keyframes: frame b's segments are [seg_off[b], seg_off[b+1])
  const int* src; const int* src_off;            // slots: frame b's entries are src[src_off[b] .. src_off[b+1])
  const int* n_cand;                             // [B]
  int* first; int* cand; int* chunk_count;
  int* list_off; int* list_slot; double* out_pos; uint8_t* out_desc;
};

__global__ __launch_bounds__(MS_THREADS) void map_mark_kernel(SelArgs A) {
  const int b = blockIdx.y, C = A.n_cand[b];
  const int p0 = blockIdx.x * MS_CHUNK + threadIdx.x * MS_PER;
  int* cand = A.cand + (size_t)b * A.n_chunk * MS_CHUNK;
  int* first = A.first + (size_t)b * A.capacity;
  int s = A.seg_off[b];
  const int s1 = A.seg_off[b + 1];
#pragma unroll
  for (int k = 0; k < MS_PER; ++k) {
    const int p = p0 + k;
    int slot = -1;
    if (p < C) {
      while (s < s1 && p >= A.segs[s].base + A.segs[s].n) ++s;            // (p < C: it ends inside the frame's segments)
      if (s < s1) {
        const MapSeg g = A.segs[s];
        if (g.slots) slot = g.slots[p - g.base];
      }
      if (slot < 0 || slot >= A.capacity || !A.live[slot]) slot = -1;
      else atomicMin(&first[slot], p);
    }
    cand[p] = slot;
  }
}

__global__ __launch_bounds__(MS_THREADS) void map_flag_kernel(SelArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int b = blockIdx.y, C = A.n_cand[b];
  const int p0 = blockIdx.x * MS_CHUNK + threadIdx.x * MS_PER;
  int* cand = A.cand + (size_t)b * A.n_chunk * MS_CHUNK;
  int n = 0;
  if (A.source == ORBX_MAP_SOURCE_KEYFRAMES) {
    int* first = A.first + (size_t)b * A.capacity;
#pragma unroll
    for (int k = 0; k < MS_PER; ++k) {
      const int p = p0 + k, slot = cand[p];
      if (slot < 0) continue;
      // only the candidate the table names writes it (back to EMPTY); the others read its number or EMPTY, never their own
      if (__hip_atomic_load(&first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p) {
        __hip_atomic_store(&first[slot], MS_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++n;
      } else {
        cand[p] = -1;
      }
    }
  } else {
    const int* src = A.src + A.src_off[b];
#pragma unroll
    for (int k = 0; k < MS_PER; ++k) {
      const int p = p0 + k;
      int slot = p < C ? src[p] : -1;
      if (slot < 0 || slot >= A.capacity || !A.live[slot]) slot = -1;
      cand[p] = slot;
      n += slot >= 0;
    }
  }
  n = block_sum<MS_THREADS>(n, wave_tot);
  if (threadIdx.x == 0) A.chunk_count[b * A.n_chunk + blockIdx.x] = n;
}

__global__ __launch_bounds__(MS_THREADS) void map_emit_kernel(SelArgs A, int B) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int me = b * A.n_chunk + blockIdx.x;
  int part = 0;
  for (int j = tid; j < me; j += MS_THREADS) part += A.chunk_count[j];
  const int base = block_sum<MS_THREADS>(part, wave_tot);
  if (tid == 0) {
    if (blockIdx.x == 0) A.list_off[b] = base;
    if (me == B * A.n_chunk - 1) A.list_off[B] = base + A.chunk_count[me];
  }
  const int* cand = A.cand + (size_t)b * A.n_chunk * MS_CHUNK + (size_t)blockIdx.x * MS_CHUNK + tid * MS_PER;
  int slot[MS_PER], n = 0;
#pragma unroll
  for (int k = 0; k < MS_PER; ++k) { slot[k] = cand[k]; n += slot[k] >= 0; }
  size_t o = (size_t)BlockScan<MS_THREADS>(wave_tot, base).round(n);
#pragma unroll
  for (int k = 0; k < MS_PER; ++k) {
    const int s = slot[k];
    if (s < 0) continue;
    A.list_slot[o] = s;
    A.out_pos[3 * o] = A.pos[3 * (size_t)s]; A.out_pos[3 * o + 1] = A.pos[3 * (size_t)s + 1]; A.out_pos[3 * o + 2] = A.pos[3 * (size_t)s + 2];
    const uint4* d = (const uint4*)(A.desc + 32 * (size_t)s);
    uint4* q = (uint4*)(A.out_desc + 32 * o);
    q[0] = d[0]; q[1] = d[1];
    ++o;
  }
}

// matched (an index into the frame's list, -1 = none) mapped through the list to slots
__global__ __launch_bounds__(MS_THREADS) void map_matched_slot_kernel(const int* matched, const int* list_off, const int* list_slot, int max_feat,
                                                                      int* matched_slot) {
  const int b = blockIdx.y, f = blockIdx.x * MS_THREADS + threadIdx.x;
  if (f >= max_feat) return;
  const size_t i = (size_t)b * max_feat + f;
  const int m = matched[i];
  matched_slot[i] = m >= 0 ? list_slot[list_off[b] + m] : -1;
}

// set / erase: row i of the call goes to slot slots[i] (no slot twice: the host has checked)
__global__ __launch_bounds__(MS_THREADS) void map_scatter_kernel(const int* slots, int n, const double* pos_in, const uint8_t* desc_in, int live_value,
                                                                 double* pos, uint8_t* desc, uint8_t* live) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= n) return;
  const size_t s = (size_t)slots[i];
  if (pos_in) { pos[3 * s] = pos_in[3 * (size_t)i]; pos[3 * s + 1] = pos_in[3 * (size_t)i + 1]; pos[3 * s + 2] = pos_in[3 * (size_t)i + 2]; }
  if (desc_in) {
    const uint32_t* d = (const uint32_t*)(desc_in + 32 * (size_t)i);       // (the caller's rows: 4-byte aligned, no more is asked)
    uint32_t* q = (uint32_t*)(desc + 32 * s);
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = d[k];
  }
  live[s] = (uint8_t)live_value;
}

// tracker.rs:1024-1036 per keyframe feature: valid = the feature has a slot and the slot is live; its position, else zeros
__global__ __launch_bounds__(MS_THREADS) void map_ref_gather_kernel(const MapRefItem* items, const uint8_t* live, const double* pos, int capacity,
                                                                    double* out_pos, uint8_t* out_valid) {
  const MapRefItem it = items[blockIdx.y];
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= it.n) return;
  const int s = it.slots ? it.slots[i] : -1;
  const bool ok = s >= 0 && s < capacity && live[s];
  const size_t o = (size_t)it.off + i;
  out_valid[o] = ok ? 1 : 0;
  out_pos[3 * o] = ok ? pos[3 * (size_t)s] : 0.0; out_pos[3 * o + 1] = ok ? pos[3 * (size_t)s + 1] : 0.0; out_pos[3 * o + 2] = ok ? pos[3 * (size_t)s + 2] : 0.0;
}

// ---- covisibility ------------------------------------------------------------------------------------------------------

constexpr int COV_Q = 4;                         // queries one count workgroup serves: a keyframe's table and live bytes are read once for all of them
constexpr int COV_TILE = 1024;                   // weights of a row the ranking workgroup holds in LDS at a time

// One keyframe of a call: its slot table, the same with repeats set to -1 (both NULL: no table), its features.
struct CovKf {
  const int* slots; const int* uniq;
  int n, pad_;
};
// Keyframe `kf` belongs to query q's marked set.  (The public calls mark one keyframe per query; the kernels do not care.)
struct CovMember {
  int kf, q;
};
struct CovArgs {
  int capacity, n_kfs, n_q, n_best;
  const uint8_t* live; const CovKf* kfs; const CovMember* members;
  const int* self;                               // [n_q] the keyframe whose weight is 0 in row q (the query itself), -1: none
  uint8_t* mark; int* weights; int* best; int* n_best_out;
};

__global__ __launch_bounds__(MS_THREADS) void cov_mark_kernel(CovArgs A, int value) {
  const CovMember m = A.members[blockIdx.y];
  const CovKf kf = A.kfs[m.kf];
  if (!kf.uniq) return;
  uint8_t* mark = A.mark + (size_t)m.q * A.capacity;
#pragma unroll
  for (int k = 0; k < MS_PER; ++k) {
    const int i = blockIdx.x * MS_CHUNK + k * MS_THREADS + threadIdx.x;
    if (i >= kf.n) continue;
    const int s = kf.uniq[i];
    if (s >= 0 && s < A.capacity && (value == 0 || A.live[s])) mark[s] = (uint8_t)value;
  }
}

__global__ __launch_bounds__(MS_THREADS) void cov_count_kernel(CovArgs A) {
  __shared__ int wave_tot[(MS_THREADS / 64) * COV_Q];
  const int k = blockIdx.x, q0 = blockIdx.y * COV_Q, nq = min(COV_Q, A.n_q - q0);
  const CovKf kf = A.kfs[k];
  const uint8_t* mark = A.mark + (size_t)q0 * A.capacity;
  int c[COV_Q];
#pragma unroll
  for (int j = 0; j < COV_Q; ++j) c[j] = 0;
  if (kf.uniq) {
    for (int i = threadIdx.x; i < kf.n; i += MS_THREADS) {
      const int s = kf.uniq[i];
      if (s < 0 || s >= A.capacity || !A.live[s]) continue;
#pragma unroll
      for (int j = 0; j < COV_Q; ++j)
        if (j < nq) c[j] += mark[(size_t)j * A.capacity + s];
    }
  }
  block_sum<MS_THREADS, COV_Q>(c, wave_tot);
#pragma unroll
  for (int j = 0; j < COV_Q; ++j)
    if (j < nq && (int)threadIdx.x == j) A.weights[(size_t)(q0 + j) * A.n_kfs + k] = A.self[q0 + j] == k ? 0 : c[j];
}

__global__ __launch_bounds__(MS_THREADS) void cov_rank_kernel(CovArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  __shared__ int tile[COV_TILE];
  const int q = blockIdx.x, n = A.n_kfs, tid = threadIdx.x;
  const int* w = A.weights + (size_t)q * n;
  int* best = A.best ? A.best + (size_t)q * A.n_best : nullptr;
  int positive = 0;
  for (int i0 = 0; i0 < n; i0 += MS_THREADS) {
    const int i = i0 + tid;
    const int wi = i < n ? w[i] : 0;
    positive += wi > 0;
    if (!best) continue;                                                   // (the same in every thread)
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += COV_TILE) {                             // the row through LDS, COV_TILE weights at a time: every lane reads the same word
      __syncthreads();
      for (int t = tid; t < COV_TILE; t += MS_THREADS) tile[t] = j0 + t < n ? w[j0 + t] : 0;
      __syncthreads();
      if (wi > 0) {
        const int m = min(COV_TILE, n - j0);
        for (int t = 0; t < m; ++t) {
          const int wj = tile[t];
          rank += wj > wi || (wj == wi && j0 + t < i);
        }
      }
    }
    if (wi > 0 && rank < A.n_best) best[rank] = i;
  }
  positive = block_sum<MS_THREADS>(positive, wave_tot);
  const int kept = min(positive, A.n_best);                                // ranks [0, kept) are taken, each by one keyframe: the positive weights outrank the zeros
  if (A.n_best_out && threadIdx.x == 0) A.n_best_out[q] = kept;
  if (best)
    for (int j = kept + threadIdx.x; j < A.n_best; j += MS_THREADS) best[j] = -1;
}

// Frame b's keyframes as selection segments [seg_off[b], seg_off[b+1]): ref >= 0: the reference keyframe, then row b of best (-1:
// a segment without candidates); ref == -1: every keyframe of the call in order.  The segments' bases by an ordered scan.
__global__ __launch_bounds__(MS_THREADS) void cov_seg_kernel(CovArgs A, const int* ref, const int* seg_off, MapSeg* segs, int* n_cand, int* local_kf) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int r = ref[b], so = seg_off[b], S = seg_off[b + 1] - so;
  BlockScan<MS_THREADS> scan(wave_tot);
  for (int j0 = 0; j0 < S; j0 += MS_THREADS) {                             // (S is the block's: every thread takes every round)
    const int j = j0 + tid;
    int kfi = -1;
    if (j < S) kfi = r < 0 ? j : j == 0 ? r : A.best[(size_t)b * A.n_best + (j - 1)];
    CovKf kf{nullptr, nullptr, 0, 0};
    if (kfi >= 0) kf = A.kfs[kfi];
    const int base = scan.round(kf.n);
    if (j < S) {
      segs[so + j] = MapSeg{kf.slots, base, kf.n};
      if (local_kf && r >= 0) local_kf[(size_t)b * (1 + A.n_best) + j] = kfi;
    }
  }
  if (tid == 0) n_cand[b] = scan.total;
  if (local_kf && r < 0)
    for (int j = tid; j < 1 + A.n_best; j += MS_THREADS) local_kf[(size_t)b * (1 + A.n_best) + j] = -1;
}

// ---- local BA window (include/orbx.h, "local BA from the resident map"; local_ba_lm.rs:665-726, :800-897) ----------------

constexpr int BAC_NONE = 0x7fffffff;             // role of a keyframe that observes none of the window's points

// One keyframe of a collection call: its slot table WITH repeats (NULL: no table) and its keypoints (28-byte rows).
struct BacKf {
  const int* slots; const orbx_keypoint* kp;
  int n, pad_;
  const uint8_t* has_point;                      // [n] the keyframe's stereo bytes (the inertial window's emit only)
};
struct BacArgs {
  int capacity, n_kfs, n_chunk, n_local;         // n_local = 1 + max_covisible: entries of local_kf
  const uint8_t* live; const BacKf* kfs;
  const int* list_off; const int* list_slot;     // the selection's outputs: M = list_off[1]
  int* index;                                    // the store's first-sighting table, row 0: EMPTY outside the launches below
  int* chunk_count;                              // [n_kfs][n_chunk]
  int* kf_count; int* role; int* obs_base;       // [n_kfs]: c(k); the kf_idx its observations carry (BAC_NONE: none); where they start
  const int* local_kf;                           // [n_local], -1 padded (cov_seg_kernel); the inertial window: chain [n_local], oldest first
  int* counts; int* fixed_kf; orbx_ba_obs32* obs;
};

// index[slot] = position in P ...
__global__ __launch_bounds__(MS_THREADS) void bac_index_kernel(BacArgs A) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i < A.list_off[1]) A.index[A.list_slot[i]] = i;
}
// ... and back to EMPTY: the call leaves the table as it found it
__global__ __launch_bounds__(MS_THREADS) void bac_restore_kernel(BacArgs A) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i < A.list_off[1]) A.index[A.list_slot[i]] = MS_EMPTY;
}

// does feature i of `kf` observe a point of the window?  -> its mp_idx, or -1
__device__ __forceinline__ int bac_mp_idx(const BacArgs& A, const BacKf& kf, int i) {
  if (i >= kf.n) return -1;
  const int s = kf.slots[i];
  if (s < 0 || s >= A.capacity || !A.live[s]) return -1;
  const int m = A.index[s];
  return m == MS_EMPTY ? -1 : m;
}

__global__ __launch_bounds__(MS_THREADS) void bac_count_kernel(BacArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int k = blockIdx.y;
  const BacKf kf = A.kfs[k];
  const int p0 = blockIdx.x * MS_CHUNK + threadIdx.x * MS_PER;
  int n = 0;
  if (kf.slots) {
#pragma unroll
    for (int j = 0; j < MS_PER; ++j) n += bac_mp_idx(A, kf, p0 + j) >= 0;
  }
  n = block_sum<MS_THREADS>(n, wave_tot);
  if (threadIdx.x == 0) A.chunk_count[k * A.n_chunk + blockIdx.x] = n;
}

// One workgroup: every keyframe's role, the fixed keyframes by position, where every observer's observations start, the counts.
// CHAIN: the inertial window (local_inertial_ba.rs:930-1030).  local_kf is the temporal chain, every entry a keyframe: chain[0] the
// anchor (-1), chain[i] window keyframe i — the anchor keeps window index 0, which no observation carries — and K counts all of them.
template <bool CHAIN>
__global__ __launch_bounds__(MS_THREADS) void bac_order_kernel(BacArgs A) {
  __shared__ int lds[MS_THREADS / 64];
  const int tid = threadIdx.x, n = A.n_kfs;
  for (int k = tid; k < n; k += MS_THREADS) {
    int c = 0;
    for (int j = 0; j < A.n_chunk; ++j) c += A.chunk_count[k * A.n_chunk + j];
    A.kf_count[k] = c; A.role[k] = BAC_NONE;
  }
  __syncthreads();
  int n_loc = 0;                                                           // local_kf's entries before the padding: each names another keyframe
  for (int j = tid; j < A.n_local; j += MS_THREADS) {
    const int k = A.local_kf[j];
    if (k >= 0) { A.role[k] = CHAIN && j > 0 ? j : j - 1; ++n_loc; }      // anchor -1, optimised keyframe i: i - 1 (chain[i]: i)
  }
  n_loc = block_sum<MS_THREADS>(n_loc, lds);                               // (its barriers order the roles before the reads below)
  BlockAppend<MS_THREADS, 1> fixed(lds);
  for (int k0 = 0; k0 < n; k0 += MS_THREADS) {                             // the other observers, ascending position
    const int k = k0 + tid;
    const bool f = k < n && A.role[k] == BAC_NONE && A.kf_count[k] > 0;
    const int at = fixed.round(f);
    if (f) { A.fixed_kf[at] = k; A.role[k] = -2 - at; }
  }
  const int n_fixed = fixed.total[0], n_obs = n_loc + n_fixed;
  for (int k = n_fixed + tid; k < n; k += MS_THREADS) A.fixed_kf[k] = -1;
  __syncthreads();                                                         // fixed_kf is read below by other threads than wrote it
  BlockScan<MS_THREADS> start(lds);
  for (int o0 = 0; o0 < n_obs; o0 += MS_THREADS) {                         // exclusive scan of the counts in observer order (n_obs is the block's)
    const int o = o0 + tid;
    const int k = o >= n_obs ? -1 : o < n_loc ? A.local_kf[o] : A.fixed_kf[o - n_loc];
    const int at = start.round(k >= 0 ? A.kf_count[k] : 0);
    if (k >= 0) A.obs_base[k] = at;
  }
  if (tid == 0) { A.counts[0] = CHAIN ? n_loc : n_loc - 1; A.counts[1] = 1 + n_fixed; A.counts[2] = A.list_off[1]; A.counts[3] = start.total; }
}

// (chunk, keyframe): ordered compaction of the chunk's counted features behind the observer's earlier chunks
// STEREO: the inertial window: mp_idx carries has_point[feature] != 0 in ORBX_BA_OBS32_STEREO.  A thread's MS_PER features are four
// consecutive bytes at a multiple of four: ONE dword load beside the 28-byte rows, not four byte gathers (the array is a 256-byte
// aligned part of the keyframe's block, padded to a multiple of 256: the dword that holds feature n - 1 lies inside it).
template <bool STEREO>
__global__ __launch_bounds__(MS_THREADS) void bac_emit_kernel(BacArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int k = blockIdx.y, tid = threadIdx.x;
  const int role = A.role[k];
  if (role == BAC_NONE || A.kf_count[k] == 0) return;                      // (the same in every thread: k is the block's, both written by an earlier launch)
  const BacKf kf = A.kfs[k];
  int base = A.obs_base[k];
  for (int j = 0; j < (int)blockIdx.x; ++j) base += A.chunk_count[k * A.n_chunk + j];
  const int p0 = blockIdx.x * MS_CHUNK + tid * MS_PER;
  int mp[MS_PER], n = 0;
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) { mp[j] = bac_mp_idx(A, kf, p0 + j); n += mp[j] >= 0; }
  static_assert(MS_PER == 4, "a thread's stereo bytes are one dword");
  const unsigned has = STEREO && n > 0 ? *(const unsigned*)(kf.has_point + p0) : 0u;   // (n > 0: p0 < kf.n)
  // Not BlockScan: its barrier in front of the store, which this single use of wave_tot does not need, measured 0.02 to 0.17 us of
  // 7 to 9 us in every row (profiles/block_scan_ab.txt).  The parent's text, with the shared wave step.
  const int lane = tid & 63, wave = tid >> 6;
  const int incl = wave_inclusive_scan(n);
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  size_t o = (size_t)base + (incl - n);
  for (int w = 0; w < wave; ++w) o += wave_tot[w];
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) {
    if (mp[j] < 0) continue;
    const float* xy = (const float*)(kf.kp + (p0 + j));                    // 28-byte rows: two dword loads
    int4 v;
    v.x = role; v.y = STEREO && ((has >> (8 * j)) & 0xffu) ? mp[j] | ORBX_BA_OBS32_STEREO : mp[j]; v.z = __float_as_int(xy[0]); v.w = __float_as_int(xy[1]);
    *(int4*)(A.obs + o) = v;
    ++o;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// slots [n] of a set / erase call: in range, and (once) none twice
int ms_check_slots(orbx_map_points* mp, const char* who, const int* slots, int n, bool once) {
  orbx_handle* h = mp->h;
  if (n < 0 || (n > 0 && !slots)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  if (++mp->gen == 0) { std::fill(mp->stamp.begin(), mp->stamp.end(), 0u); mp->gen = 1; }
  for (int i = 0; i < n; ++i) {
    if (slots[i] < 0 || slots[i] >= mp->capacity) return orbx_fail(h, ORBX_ERR_INVALID, "%s: slot %d (entry %d) is outside [0, %d)", who, slots[i], i, mp->capacity);
    if (once && mp->stamp[(size_t)slots[i]] == mp->gen) return orbx_fail(h, ORBX_ERR_INVALID, "%s: slot %d is listed twice (entry %d)", who, slots[i], i);
    mp->stamp[(size_t)slots[i]] = mp->gen;
  }
  return ORBX_OK;
}

// set and set_device: the slots (and the host form's rows) go up through the upload ring, then one scatter launch
int ms_set(orbx_map_points* mp, const char* who, const int* slots, int n, const double* positions, const uint8_t* desc, bool on_host) {
  orbx_handle* h = mp->h;
  if (int rc = ms_check_slots(mp, who, slots, n, true)) return rc;
  for (int i = 0; i < n; ++i)
    if (!mp->live[(size_t)slots[i]] && (!positions || !desc))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: slot %d is not live yet: its first set needs positions and descriptors", who, slots[i]);
  if (n == 0 || (!positions && !desc)) return ORBX_OK;
  ORBX_HIP(h, hipSetDevice(h->device));
  UploadPlan up;
  const size_t N = (size_t)n, o_sl = up.put(slots, 4 * N), o_po = up.put(positions, on_host && positions ? 24 * N : 0), o_de = up.put(desc, on_host && desc ? 32 * N : 0);
  if (int rc = up.send(h, h->ring_map, h->ws_map.call_tables)) return rc;
  uint8_t* const ds = up.device;
  const double* d_pos = !positions ? nullptr : on_host ? (const double*)(ds + o_po) : positions;
  const uint8_t* d_desc = !desc ? nullptr : on_host ? ds + o_de : desc;
  orbx_launch(h, "map_scatter_kernel", false, map_scatter_kernel, dim3((n + MS_THREADS - 1) / MS_THREADS), dim3(MS_THREADS), 0, (const int*)(ds + o_sl), n, d_pos, d_desc, 1,
              mp->d_pos, mp->d_desc, mp->d_live);
  ORBX_HIP(h, hipGetLastError());
  for (int i = 0; i < n; ++i)
    if (!mp->live[(size_t)slots[i]]) { mp->live[(size_t)slots[i]] = 1; ++mp->n_live; }
  return ORBX_OK;
}

// Four refusals many calls share: the store (not null, of this handle), the keyframes and the frames of a call whose launches have one grid row
// per keyframe or per frame, and the features of a call's keyframes summed (they are numbered in an int).
int ms_check_store(orbx_handle* h, const char* who, const orbx_map_points* mp) {
  return mp && mp->h == h ? (int)ORBX_OK : orbx_fail(h, ORBX_ERR_INVALID, "%s: the store is null or of another handle", who);
}
int ms_check_grid_keyframes(orbx_handle* h, const char* who, int n_kfs) {
  return n_kfs <= 0xffff ? (int)ORBX_OK : orbx_fail(h, ORBX_ERR_INVALID, "%s: at most 65535 keyframes per call (the keyframe is a grid dimension)", who);
}
int ms_check_grid_frames(orbx_handle* h, const char* who, int n_frames) {
  return n_frames <= 0xffff ? (int)ORBX_OK : orbx_fail(h, ORBX_ERR_INVALID, "%s: at most 65535 frames per call (the frame is a grid dimension)", who);
}
int ms_check_feature_total(orbx_handle* h, const char* who, long long total) {
  return total <= 0x7fffffff ? (int)ORBX_OK : orbx_fail(h, ORBX_ERR_INVALID, "%s: the keyframes hold more than 2^31 - 1 features", who);
}

// keyframe t of a selection or covisibility call: not null, of this handle, its slot table (if it has one) of this store
int ms_check_keyframe(orbx_handle* h, const char* who, const orbx_map_points* mp, const orbx_keyframe* kf, int t) {
  if (!kf || kf->h != h) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d is null or of another handle", who, t);
  if (kf->slot_store && kf->slot_store != mp) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d's slot table belongs to another store", who, t);
  return ORBX_OK;
}

// kfs [n_kfs] of a call that rewrites tables: none twice
int ms_check_no_repeat(orbx_handle* h, const char* who, int n_kfs, const orbx_keyframe* const* kfs) {
  std::vector<const orbx_keyframe*> seen(kfs, kfs + n_kfs);
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return orbx_fail(h, ORBX_ERR_INVALID, "%s: a keyframe is listed twice in kfs[] (their tables are rewritten)", who);
  return ORBX_OK;
}

// ... and each as ms_check_keyframe asks
int ms_check_distinct(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs) {
  for (int t = 0; t < n_kfs; ++t)
    if (int rc = ms_check_keyframe(h, who, mp, kfs[t], t)) return rc;
  return ms_check_no_repeat(h, who, n_kfs, kfs);
}

// erase behind its checks: d_slots [n] already lies in device memory; the live bytes and their host mirror
int ms_erase_launch(orbx_handle* h, orbx_map_points* mp, const int* d_slots, const int* slots, int n) {
  orbx_launch(h, "map_scatter_kernel", false, map_scatter_kernel, dim3((n + MS_THREADS - 1) / MS_THREADS), dim3(MS_THREADS), 0, d_slots, n, (const double*)nullptr,
              (const uint8_t*)nullptr, 0, mp->d_pos, mp->d_desc, mp->d_live);
  ORBX_HIP(h, hipGetLastError());
  for (int i = 0; i < n; ++i)
    if (mp->live[(size_t)slots[i]]) { mp->live[(size_t)slots[i]] = 0; --mp->n_live; }
  return ORBX_OK;
}

// the list outputs of a selection whose lists hold at most `total` rows (src_missing: the slot form without its source array)
int ms_check_list_outputs(orbx_handle* h, const char* who, int total, const int* d_list_off, const int* d_list_slot, const double* d_positions,
                          const uint8_t* d_mp_desc, bool src_missing = false) {
  if (!d_list_off || (total > 0 && (!d_list_slot || !d_positions || !d_mp_desc)) || ((uintptr_t)d_mp_desc & 15) || (total > 0 && src_missing))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (d_mp_desc is 16-byte aligned)", who);
  return ORBX_OK;
}

// What a selection call is, checked and sized on the host: per frame the candidates and the bound of its list.
struct SelPlan {
  std::vector<MapSeg> segs;
  std::vector<int> seg_off, n_cand, bound_off;       // bound_off [B+1]: offsets of the lists' host-known bounds
  int max_cand = 0, max_bound = 0;
};

int ms_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int source, int B, const orbx_keyframe* const* kfs, const int* kf_offsets,
            const int* src_offsets, SelPlan& P) {
  if (int rc = ms_check_store(h, who, mp)) return rc;
  if (B <= 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: n_frames must be positive", who);
  if (int rc = ms_check_grid_frames(h, who, B)) return rc;
  if (source != ORBX_MAP_SOURCE_KEYFRAMES && source != ORBX_MAP_SOURCE_SLOTS) return orbx_fail(h, ORBX_ERR_INVALID, "%s: unknown source kind %d", who, source);
  P.n_cand.assign((size_t)B, 0); P.bound_off.assign((size_t)B + 1, 0); P.seg_off.assign((size_t)B + 1, 0);
  long long total = 0;
  if (source == ORBX_MAP_SOURCE_KEYFRAMES) {
    if (int rc = orbx_check_offsets(h, who, "kf_offsets", "frame", B, kf_offsets)) return rc;
    if (kf_offsets[B] > 0 && !kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    P.segs.reserve((size_t)kf_offsets[B]);
    for (int b = 0; b < B; ++b) {
      long long c = 0;
      for (int t = kf_offsets[b]; t < kf_offsets[b + 1]; ++t) {
        const orbx_keyframe* kf = kfs[t];
        if (int rc = ms_check_keyframe(h, who, mp, kf, t)) return rc;
        P.segs.push_back(MapSeg{kf->slot_store ? kf->d_mp_slot : nullptr, (int)c, kf->n});
        c += kf->n;
        if (c >= MS_EMPTY) return orbx_fail(h, ORBX_ERR_INVALID, "%s: frame %d has too many candidates", who, b);
      }
      P.seg_off[(size_t)b + 1] = (int)P.segs.size();
      P.n_cand[(size_t)b] = (int)c;
      const int bound = (int)std::min<long long>(c, mp->capacity);        // distinct slots: never more than the store holds
      total += bound;
      P.max_cand = std::max(P.max_cand, (int)c); P.max_bound = std::max(P.max_bound, bound);
      P.bound_off[(size_t)b + 1] = (int)std::min<long long>(total, 0x7fffffff);
    }
  } else {
    if (int rc = orbx_check_offsets(h, who, "src_offsets", "frame", B, src_offsets, &P.max_cand)) return rc;
    for (int b = 0; b < B; ++b) { P.n_cand[(size_t)b] = src_offsets[b + 1] - src_offsets[b]; P.bound_off[(size_t)b + 1] = src_offsets[b + 1]; }
    P.max_bound = P.max_cand;                                               // no de-duplication: a list may be as long as its source
    total = src_offsets[B];
  }
  if (total > 0x7fffffff) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the lists' bounds exceed 2^31 - 1 rows", who);
  return ORBX_OK;
}

// the one fill of the first-sighting tables: calls leave them EMPTY
int ms_reserve_first(orbx_handle* h, orbx_map_points* mp, size_t rows) {
  const size_t need = 4 * rows * (size_t)mp->capacity;
  if (mp->first.bytes < need) {
    if (int rc = orbx_reserve(h, mp->first, need)) return rc;
    ORBX_HIP(h, hipMemsetAsync(mp->first.p, MS_EMPTY & 0xff, mp->first.bytes, h->stream));
  }
  return ORBX_OK;
}

// The three launches on the handle's stream, every table already in device memory (uploaded by ms_select_enqueue, or written by
// cov_seg_kernel); max_cand bounds every frame's candidates on the host.
int ms_select_launch(orbx_handle* h, orbx_map_points* mp, int source, int B, int max_cand, const MapSeg* d_segs, const int* d_seg_off, const int* d_n_cand,
                     const int* d_src_slots, const int* d_src_off, int* d_list_off, int* d_list_slot, double* d_positions, uint8_t* d_mp_desc) {
  const size_t Bz = (size_t)B;
  if (source == ORBX_MAP_SOURCE_KEYFRAMES)
    if (int rc = ms_reserve_first(h, mp, Bz)) return rc;
  const int n_chunk = std::max(1, (max_cand + MS_CHUNK - 1) / MS_CHUNK);
  Carve ws;
  const size_t o_ca = ws.take(4 * Bz * (size_t)n_chunk * MS_CHUNK), o_cc = ws.take(4 * Bz * (size_t)n_chunk);
  if (int rc = orbx_reserve(h, h->ws_map.sel_scratch, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.sel_scratch.p;
  SelArgs A{};
  A.source = source; A.capacity = mp->capacity; A.n_chunk = n_chunk;
  A.live = mp->d_live; A.pos = mp->d_pos; A.desc = mp->d_desc;
  A.segs = d_segs; A.seg_off = d_seg_off; A.n_cand = d_n_cand;
  A.src = d_src_slots; A.src_off = d_src_off;
  A.first = (int*)mp->first.p; A.cand = (int*)(w + o_ca); A.chunk_count = (int*)(w + o_cc);
  A.list_off = d_list_off; A.list_slot = d_list_slot; A.out_pos = d_positions; A.out_desc = d_mp_desc;
  const dim3 grid(n_chunk, B), block(MS_THREADS);
  if (source == ORBX_MAP_SOURCE_KEYFRAMES) orbx_launch(h, "map_mark_kernel", false, map_mark_kernel, grid, block, 0, A);
  orbx_launch(h, "map_flag_kernel", source == ORBX_MAP_SOURCE_KEYFRAMES, map_flag_kernel, grid, block, 0, A);
  orbx_launch(h, "map_emit_kernel", true, map_emit_kernel, grid, block, 0, A, B);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// The selection from host tables: they go up through the ring, then the launches.  d_src_slots and every output are device memory;
// list_cap: rows the outputs hold.
int ms_select_enqueue(orbx_handle* h, const char* who, orbx_map_points* mp, int source, int B, const SelPlan& P, const int* d_src_slots, const int* src_offsets,
                      int list_cap, int* d_list_off, int* d_list_slot, double* d_positions, uint8_t* d_mp_desc) {
  const int total = P.bound_off[(size_t)B];
  if (list_cap < total) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d is below the lists' bound %d (the sum over the frames of their candidates, "
                                         "per frame at most the capacity where keyframes are the source)", who, list_cap, total);
  if (int rc = ms_check_list_outputs(h, who, total, d_list_off, d_list_slot, d_positions, d_mp_desc, source == ORBX_MAP_SOURCE_SLOTS && !d_src_slots)) return rc;
  ORBX_HIP(h, hipSetDevice(h->device));
  const size_t Bz = (size_t)B;
  const bool from_slots = source == ORBX_MAP_SOURCE_SLOTS;
  UploadPlan up;
  const size_t o_sg = up.put(P.segs.data(), sizeof(MapSeg) * P.segs.size()), o_so = up.put(P.seg_off.data(), 4 * (Bz + 1)), o_nc = up.put(P.n_cand.data(), 4 * Bz),
               o_sr = up.put(from_slots ? src_offsets : nullptr, 4 * (Bz + 1));
  if (int rc = up.begin(h, h->ring_map, h->ws_map.call_tables)) return rc;
  if (!from_slots) std::memset(up.host + o_sr, 0, 4 * (Bz + 1));
  if (int rc = up.commit(h, h->ring_map, h->ws_map.call_tables)) return rc;
  uint8_t* const ds = up.device;
  return ms_select_launch(h, mp, source, B, P.max_cand, (const MapSeg*)(ds + o_sg), (const int*)(ds + o_so), (const int*)(ds + o_nc), d_src_slots,
                          (const int*)(ds + o_sr), d_list_off, d_list_slot, d_positions, d_mp_desc);
}

int ms_matched_slot_enqueue(orbx_handle* h, int B, int max_feat, const int* d_matched, const int* d_list_off, const int* d_list_slot, int* d_matched_slot) {
  if (max_feat <= 0) return ORBX_OK;
  orbx_launch(h, "map_matched_slot_kernel", true, map_matched_slot_kernel, dim3((max_feat + MS_THREADS - 1) / MS_THREADS, B), dim3(MS_THREADS), 0, d_matched, d_list_off,
              d_list_slot, max_feat, d_matched_slot);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// ---- covisibility, host side ---------------------------------------------------------------------------------------------

// The keyframes of a covisibility call, checked as ms_plan checks a selection's.
struct CovPlan {
  std::vector<CovKf> kfs;
  int max_n = 0;
};

int cov_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_best, CovPlan& P) {
  if (int rc = ms_check_store(h, who, mp)) return rc;
  if (n_kfs < 0 || (n_kfs > 0 && !kfs)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (n_kfs >= 0)", who);
  if (n_best < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: n_best must not be negative", who);
  P.kfs.resize((size_t)n_kfs);
  for (int t = 0; t < n_kfs; ++t) {
    const orbx_keyframe* kf = kfs[t];
    if (int rc = ms_check_keyframe(h, who, mp, kf, t)) return rc;
    P.kfs[(size_t)t] = CovKf{kf->slot_store ? kf->d_mp_slot : nullptr, kf->slot_store ? kf->d_mp_uniq : nullptr, kf->n, 0};
    P.max_n = std::max(P.max_n, kf->n);
  }
  return ORBX_OK;
}

// What cov_enqueue adds for the tracking call: frame b's segments (seg_off: host [B+1]) and what was chosen.  The three arrays it
// fills in the call's workspace are answered for ms_select_launch.
struct CovSegs {
  const int* seg_off; int* d_local_kf;
  const MapSeg* d_segs; const int* d_seg_off; const int* d_n_cand;
};

// Mark, count, clear, rank (and the segments) on the handle's stream.  query [Q]: indices into the call's keyframes, -1 (only with
// `segs`: a frame without a reference keyframe) marks nothing.  Outputs that are NULL and needed are kept in the call's workspace.
int cov_enqueue(orbx_handle* h, orbx_map_points* mp, const CovPlan& P, int Q, const int* query, int n_best, int* d_weights, int* d_best, int* d_n_best,
                CovSegs* segs) {
  ORBX_HIP(h, hipSetDevice(h->device));
  const size_t Qz = (size_t)Q, K = P.kfs.size(), n_seg = segs ? (size_t)segs->seg_off[Q] : 0;
  const bool rank = d_best || d_n_best || segs;
  std::vector<CovMember> members;
  int max_qn = 0;
  for (int q = 0; q < Q; ++q)
    if (query[q] >= 0) { members.push_back(CovMember{query[q], q}); max_qn = std::max(max_qn, P.kfs[(size_t)query[q]].n); }
  const size_t need = Qz * (size_t)mp->capacity;
  if (mp->mark.bytes < need) {                                              // the one fill of the tables: calls leave them 0
    if (int rc = orbx_reserve(h, mp->mark, need)) return rc;
    ORBX_HIP(h, hipMemsetAsync(mp->mark.p, 0, mp->mark.bytes, h->stream));
  }
  UploadPlan up;
  Carve ws;
  const size_t o_kf = up.put(P.kfs.data(), sizeof(CovKf) * K), o_me = up.put(members.data(), sizeof(CovMember) * members.size()), o_se = up.put(query, 4 * Qz),
               o_so = up.put(segs ? segs->seg_off : nullptr, segs ? 4 * (Qz + 1) : 0);
  const size_t o_we = ws.take(d_weights ? 0 : 4 * Qz * K), o_be = ws.take(d_best || !segs ? 0 : 4 * Qz * (size_t)n_best), o_sg = ws.take(sizeof(MapSeg) * n_seg),
               o_nc = ws.take(segs ? 4 * Qz : 0);
  if (int rc = up.send(h, h->ring_map, h->ws_map.cov_tables)) return rc;
  uint8_t* const ds = up.device;
  if (int rc = orbx_reserve(h, h->ws_map.cov_scratch, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.cov_scratch.p;
  CovArgs A{};
  A.capacity = mp->capacity; A.n_kfs = (int)K; A.n_q = Q; A.n_best = n_best;
  A.live = mp->d_live; A.kfs = (const CovKf*)(ds + o_kf); A.members = (const CovMember*)(ds + o_me); A.self = (const int*)(ds + o_se);
  A.mark = (uint8_t*)mp->mark.p; A.weights = d_weights ? d_weights : (int*)(w + o_we);
  A.best = d_best ? d_best : segs ? (int*)(w + o_be) : nullptr; A.n_best_out = d_n_best;
  const dim3 block(MS_THREADS), mark_grid(std::max(1, (max_qn + MS_CHUNK - 1) / MS_CHUNK), (unsigned)members.size());
  const bool marks = !members.empty() && max_qn > 0 && K > 0;
  if (marks) orbx_launch(h, "cov_mark_kernel", false, cov_mark_kernel, mark_grid, block, 0, A, 1);
  if (K > 0) orbx_launch(h, "cov_count_kernel", marks, cov_count_kernel, dim3((unsigned)K, (Q + COV_Q - 1) / COV_Q), block, 0, A);
  if (marks) orbx_launch(h, "cov_mark_kernel", true, cov_mark_kernel, mark_grid, block, 0, A, 0);
  if (rank) orbx_launch(h, "cov_rank_kernel", K > 0, cov_rank_kernel, dim3(Q), block, 0, A);
  if (segs) {
    orbx_launch(h, "cov_seg_kernel", true, cov_seg_kernel, dim3(Q), block, 0, A, A.self, (const int*)(ds + o_so), (MapSeg*)(w + o_sg), (int*)(w + o_nc), segs->d_local_kf);
    segs->d_segs = (const MapSeg*)(w + o_sg); segs->d_seg_off = (const int*)(ds + o_so); segs->d_n_cand = (const int*)(w + o_nc);
  }
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

int cov_check_queries(orbx_handle* h, const char* who, const char* name, int n, const int* idx, int n_kfs, int lowest) {
  if (n > 0 && !idx) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  for (int i = 0; i < n; ++i)
    if (idx[i] < lowest || idx[i] >= n_kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: %s[%d] = %d is outside [0, %d)", who, name, i, idx[i], n_kfs);
  return ORBX_OK;
}

// A local-map tracking call, checked and sized on the host: per frame its segments and the bound of its list — the reference
// keyframe's features plus the n_best largest of the others' (every keyframe's where ref is -1), at most the capacity.
struct LocalPlan {
  CovPlan C;
  std::vector<int> seg_off, bound_off;
  int max_cand = 0;
};

int local_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int B, int n_kfs, const orbx_keyframe* const* kfs, const int* ref_kf, int n_best,
               LocalPlan& P) {
  if (B <= 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: n_frames must be positive", who);
  if (int rc = ms_check_grid_frames(h, who, B)) return rc;
  if (int rc = cov_plan(h, who, mp, n_kfs, kfs, n_best, P.C)) return rc;
  if (int rc = cov_check_queries(h, who, "ref_kf", B, ref_kf, n_kfs, -1)) return rc;
  const size_t K = (size_t)n_kfs;
  std::vector<int> order(K), place(K);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return P.C.kfs[(size_t)a].n > P.C.kfs[(size_t)b].n; });
  std::vector<long long> top(K + 1, 0);                                    // top[i]: the i largest feature counts summed
  for (size_t i = 0; i < K; ++i) { place[(size_t)order[i]] = (int)i; top[i + 1] = top[i] + P.C.kfs[(size_t)order[i]].n; }
  P.seg_off.assign((size_t)B + 1, 0); P.bound_off.assign((size_t)B + 1, 0);
  long long total = 0, n_seg = 0;
  for (int b = 0; b < B; ++b) {
    const int r = ref_kf[b];
    long long c = top[K];
    if (r >= 0) {                                                           // the reference and the n_best largest of the others
      const size_t nb = (size_t)std::min<long long>(n_best, (long long)K - 1);
      c = (size_t)place[(size_t)r] < nb ? top[nb + 1] : top[nb] + P.C.kfs[(size_t)r].n;
    }
    if (c >= MS_EMPTY) return orbx_fail(h, ORBX_ERR_INVALID, "%s: frame %d has too many candidates", who, b);
    n_seg += r >= 0 ? 1 + (long long)n_best : (long long)K;
    total += std::min<long long>(c, mp->capacity);
    if (n_seg > 0x7fffffff || total > 0x7fffffff) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the lists' bounds exceed 2^31 - 1 rows", who);
    P.max_cand = std::max(P.max_cand, (int)c);
    P.seg_off[(size_t)b + 1] = (int)n_seg; P.bound_off[(size_t)b + 1] = (int)total;
  }
  return ORBX_OK;
}

// covisibility, segments, then the three selection launches on them
int local_select_enqueue(orbx_handle* h, const char* who, orbx_map_points* mp, int B, const LocalPlan& P, const int* ref_kf, int n_best, int list_cap,
                         int* d_local_kf, int* d_list_off, int* d_list_slot, double* d_positions, uint8_t* d_mp_desc) {
  const int total = P.bound_off[(size_t)B];
  if (list_cap < total) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d is below the lists' bound %d (per frame the reference keyframe's features plus the "
                                         "n_best largest of the others', at most the capacity)", who, list_cap, total);
  if (int rc = ms_check_list_outputs(h, who, total, d_list_off, d_list_slot, d_positions, d_mp_desc)) return rc;
  CovSegs sg{P.seg_off.data(), d_local_kf, nullptr, nullptr, nullptr};
  if (int rc = cov_enqueue(h, mp, P.C, B, ref_kf, n_best, nullptr, nullptr, nullptr, &sg)) return rc;
  return ms_select_launch(h, mp, ORBX_MAP_SOURCE_KEYFRAMES, B, P.max_cand, sg.d_segs, sg.d_seg_off, sg.d_n_cand, nullptr, nullptr, d_list_off, d_list_slot,
                          d_positions, d_mp_desc);
}

// ---- local BA window, host side --------------------------------------------------------------------------------------------

// A collection call, checked and sized on the host.  Its kind: the covisible window of local BA (cur and its max_covisible best
// neighbours, picked on the device) or the temporal chain of local inertial BA (named by the caller; chain[0] is the anchor).
// The keyframes' tables with their keypoints (the chain's: and stereo bytes), the observations' bound (every feature of kfs[]), the
// list's bound, and the kind's selection plan: one local-map frame whose reference is `cur`, or the chain as one frame of keyframes.
// ... or the whole map of global BA (global_ba.rs:100-181): every keyframe of the call is in the list, kfs[0] the anchor, kfs[i] optimised
// keyframe i - 1, no stereo bit: the chain's selection and uploaded list with the covisible window's order and emit kernels.
enum WinKind { WIN_COVISIBLE, WIN_CHAIN, WIN_GLOBAL };
struct WinPlan {
  WinKind kind = WIN_COVISIBLE;
  std::vector<BacKf> kfs;
  int n_feat = 0, max_n = 0, bound = 0;
  LocalPlan L; int cur = 0, max_covisible = 0;       // WIN_COVISIBLE
  SelPlan S; std::vector<int> chain;                 // WIN_CHAIN
  int n_local() const { return kind != WIN_COVISIBLE ? (int)chain.size() : 1 + max_covisible; }   // rows of local_kf
};

// the keyframe table and the observations' bound (each keyframe as ms_check_keyframe asks)
int win_plan_kfs(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, WinPlan& P) {
  P.kfs.resize((size_t)n_kfs);
  long long total = 0;
  for (int t = 0; t < n_kfs; ++t) {
    const orbx_keyframe* kf = kfs[t];
    if (int rc = ms_check_keyframe(h, who, mp, kf, t)) return rc;
    P.kfs[(size_t)t] = BacKf{kf->slot_store ? kf->d_mp_slot : nullptr, kf->d_kp, kf->n, 0, P.kind == WIN_CHAIN ? kf->d_has_point : nullptr};
    total += kf->n; P.max_n = std::max(P.max_n, kf->n);
  }
  if (int rc = ms_check_feature_total(h, who, total)) return rc;
  P.n_feat = (int)total;
  return ORBX_OK;
}

int bac_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int cur, int max_covisible, WinPlan& P) {
  if (n_kfs <= 0 || cur < 0 || cur >= n_kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: cur = %d is outside [0, n_kfs = %d)", who, cur, n_kfs);
  if (int rc = ms_check_grid_keyframes(h, who, n_kfs)) return rc;
  if (max_covisible < 0 || max_covisible >= MS_EMPTY / 64) return orbx_fail(h, ORBX_ERR_INVALID, "%s: max_covisible must not be negative", who);
  P.kind = WIN_COVISIBLE; P.cur = cur; P.max_covisible = max_covisible;
  if (int rc = local_plan(h, who, mp, 1, n_kfs, kfs, &cur, max_covisible, P.L)) return rc;
  P.bound = P.L.bound_off[1];
  return win_plan_kfs(h, who, mp, n_kfs, kfs, P);
}

int bic_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_chain, const int* chain, WinPlan& P) {
  if (int rc = ms_check_store(h, who, mp)) return rc;
  if (n_kfs < 0 || (n_kfs > 0 && !kfs) || n_chain < 0 || (n_chain > 0 && !chain)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  if (int rc = ms_check_grid_keyframes(h, who, n_kfs)) return rc;
  std::vector<uint8_t> in_chain((size_t)n_kfs, 0);
  for (int i = 0; i < n_chain; ++i) {
    if (chain[i] < 0 || chain[i] >= n_kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: chain[%d] = %d is outside [0, n_kfs = %d)", who, i, chain[i], n_kfs);
    if (in_chain[(size_t)chain[i]]) return orbx_fail(h, ORBX_ERR_INVALID, "%s: chain[%d] = %d is listed twice", who, i, chain[i]);
    in_chain[(size_t)chain[i]] = 1;
  }
  P.kind = WIN_CHAIN;
  if (int rc = win_plan_kfs(h, who, mp, n_kfs, kfs, P)) return rc;
  if (n_chain < 2) return orbx_fail(h, ORBX_ERR_EMPTY, "%s: the temporal window needs two keyframes", who);   // local_inertial_ba.rs:940-942
  P.chain.assign(chain, chain + n_chain);
  std::vector<const orbx_keyframe*> ck((size_t)n_chain);
  for (int i = 0; i < n_chain; ++i) ck[(size_t)i] = kfs[chain[i]];
  const int off[2] = {0, n_chain};
  if (int rc = ms_plan(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, ck.data(), off, nullptr, P.S)) return rc;
  P.bound = P.S.bound_off[1];
  return ORBX_OK;
}

// The whole map: kfs[] is the caller's list in ascending id with the bad keyframes left out (global_ba.rs:100-124)
int glb_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, WinPlan& P) {
  if (int rc = ms_check_store(h, who, mp)) return rc;
  if (n_kfs <= 0 || !kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: n_kfs must be positive", who);
  if (int rc = ms_check_grid_keyframes(h, who, n_kfs)) return rc;
  P.kind = WIN_GLOBAL;
  if (int rc = win_plan_kfs(h, who, mp, n_kfs, kfs, P)) return rc;
  P.chain.resize((size_t)n_kfs);
  std::iota(P.chain.begin(), P.chain.end(), 0);
  const int off[2] = {0, n_kfs};
  if (int rc = ms_plan(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, kfs, off, nullptr, P.S)) return rc;
  P.bound = P.S.bound_off[1];
  return ORBX_OK;
}

// Everything on the handle's stream: the kind's selection (covisibility and selection as the tracking call runs them, or the chain's),
// then the five launches above.  d_local_kf: the covisible window's output (the chain's local_kf is the uploaded chain).
int win_enqueue(orbx_handle* h, const char* who, orbx_map_points* mp, const WinPlan& P, int list_cap, int obs_cap, int* d_counts, int* d_local_kf,
                int* d_fixed_kf, int* d_list_slot, double* d_positions, orbx_ba_obs32* d_obs32) {
  const bool chain = P.kind != WIN_COVISIBLE, whole = P.kind == WIN_GLOBAL;   // chain: the list of local keyframes is the caller's, uploaded
  const int bound = P.bound, n_kfs = (int)P.kfs.size();
  if (list_cap < bound) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d is below the list's bound %d (%s, at most the capacity)", who, list_cap, bound,
                                         whole ? "the keyframes' features summed" : chain ? "the chain's features summed" : "cur's features plus the max_covisible largest of the others'");
  if (obs_cap < P.n_feat) return orbx_fail(h, ORBX_ERR_INVALID, "%s: obs_cap %d is below the observations' bound %d (the features of kfs[] summed)", who, obs_cap, P.n_feat);
  if (!d_counts || (!chain && !d_local_kf) || (!whole && !d_fixed_kf) || (bound > 0 && (!d_list_slot || !d_positions)) || (P.n_feat > 0 && !d_obs32) || ((uintptr_t)d_obs32 & 15))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (d_obs32 is 16-byte aligned)", who);
  ORBX_HIP(h, hipSetDevice(h->device));
  const size_t K = (size_t)n_kfs;
  const int n_chunk = std::max(1, (P.max_n + MS_CHUNK - 1) / MS_CHUNK);
  Carve ws;
  UploadPlan up;
  const size_t o_lo = ws.take(8), o_gd = ws.take(32 * (size_t)bound), o_cc = ws.take(4 * K * (size_t)n_chunk), o_kc = ws.take(4 * K), o_ro = ws.take(4 * K),
               o_ob = ws.take(4 * K), o_fx = ws.take(whole ? 4 * K : 0);   // (the whole map has no fixed observers to report: the order kernel's list stays here)
  const size_t u_kf = up.put(P.kfs.data(), sizeof(BacKf) * K), u_ch = up.put(P.chain.data(), 4 * P.chain.size());
  if (int rc = orbx_reserve(h, h->ws_map.win_scratch, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.win_scratch.p;
  if (int rc = up.send(h, h->ring_map, h->ws_map.win_tables)) return rc;
  uint8_t* const ds = up.device;
  // P: local = [cur] ++ best as one frame of orbx_map_track_local_device gets it, or the chain's tables in chain order (descriptors stay in the workspace)
  if (int rc = chain ? ms_select_enqueue(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, P.S, nullptr, nullptr, bound, (int*)(w + o_lo), d_list_slot, d_positions, w + o_gd)
                     : local_select_enqueue(h, who, mp, 1, P.L, &P.cur, P.max_covisible, bound, d_local_kf, (int*)(w + o_lo), d_list_slot, d_positions, w + o_gd))
    return rc;
  BacArgs A{};
  A.capacity = mp->capacity; A.n_kfs = n_kfs; A.n_chunk = n_chunk; A.n_local = P.n_local();
  A.live = mp->d_live; A.kfs = (const BacKf*)(ds + u_kf); A.list_off = (const int*)(w + o_lo); A.list_slot = d_list_slot;
  A.index = (int*)mp->first.p;                                              // (row 0; the selection has allocated it and left it EMPTY)
  A.chunk_count = (int*)(w + o_cc); A.kf_count = (int*)(w + o_kc); A.role = (int*)(w + o_ro); A.obs_base = (int*)(w + o_ob);
  A.local_kf = chain ? (const int*)(ds + u_ch) : d_local_kf; A.counts = d_counts; A.fixed_kf = whole ? (int*)(w + o_fx) : d_fixed_kf; A.obs = d_obs32;
  // order and emit are the kind's: roles from local_kf and plain mp_idx, or roles from the chain and the stereo bit
  using BacKernel = void (*)(BacArgs);
  static const BacKernel covisible[2] = {bac_order_kernel<false>, bac_emit_kernel<false>}, temporal[2] = {bac_order_kernel<true>, bac_emit_kernel<true>};
  const BacKernel* of_kind = P.kind == WIN_CHAIN ? temporal : covisible;
  const dim3 block(MS_THREADS), list_grid(std::max(1, (bound + MS_THREADS - 1) / MS_THREADS)), kf_grid(n_chunk, n_kfs);
  orbx_launch(h, "bac_index_kernel", true, bac_index_kernel, list_grid, block, 0, A);
  orbx_launch(h, "bac_count_kernel", true, bac_count_kernel, kf_grid, block, 0, A);
  orbx_launch(h, "bac_order_kernel", true, of_kind[0], dim3(1), block, 0, A);
  orbx_launch(h, "bac_emit_kernel", true, of_kind[1], kf_grid, block, 0, A);
  orbx_launch(h, "bac_restore_kernel", true, bac_restore_kernel, list_grid, block, 0, A);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// a window without a point to optimise: M == 0, and for the covisible window N == 0 (local_inertial_ba.rs:946-948)
int win_check_empty(orbx_handle* h, const char* who, const WinPlan& P, const int* counts) {
  if (P.kind == WIN_GLOBAL) return counts[2] ? (int)ORBX_OK : orbx_fail(h, ORBX_ERR_EMPTY, "%s: the keyframes observe no live map point", who);
  if (P.kind == WIN_CHAIN) return counts[2] ? (int)ORBX_OK : orbx_fail(h, ORBX_ERR_EMPTY, "%s: the chain observes no live map point", who);
  return counts[2] && counts[3] ? (int)ORBX_OK : orbx_fail(h, ORBX_ERR_EMPTY, "%s: the local keyframes observe no live map point", who);
}

// The collection into ws_map.host_blobs (d) and its first download (hp), which the call waits for: counts | local (covisible) | fixed, and
// with `rows` | P's slots | P's positions at their bounds.  The observations stay at d + o_ob.
struct WinDown { size_t o_cn, o_lk, o_fx, o_ls, o_po, o_ob; uint8_t* d; const uint8_t* hp; };
int win_collect_down(orbx_handle* h, const char* who, orbx_map_points* mp, const WinPlan& P, bool rows, WinDown& o) {
  const size_t bound = (size_t)P.bound, nl = P.kind != WIN_COVISIBLE ? 0 : (size_t)P.n_local(), K = P.kfs.size();
  ORBX_HIP(h, hipSetDevice(h->device));
  Carve out;
  o.o_cn = out.take(16); o.o_lk = out.take(4 * nl); o.o_fx = out.take(4 * K);
  const size_t head = out.off;
  o.o_ls = out.take(4 * bound); o.o_po = out.take(24 * bound);
  const size_t down = rows ? out.off : head;
  o.o_ob = out.take(16 * (size_t)P.n_feat);
  if (int rc = orbx_reserve(h, h->ws_map.host_blobs, out.off)) return rc;
  if (int rc = orbx_reserve_pinned(h, h->pin_map, down)) return rc;
  uint8_t* d = o.d = (uint8_t*)h->ws_map.host_blobs.p;
  if (int rc = win_enqueue(h, who, mp, P, P.bound, P.n_feat, (int*)(d + o.o_cn), (int*)(d + o.o_lk), (int*)(d + o.o_fx), (int*)(d + o.o_ls), (double*)(d + o.o_po),
                           (orbx_ba_obs32*)(d + o.o_ob)))
    return rc;
  o.hp = (const uint8_t*)h->pin_map.p;
  ORBX_HIP(h, hipMemcpyAsync(h->pin_map.p, d, down, hipMemcpyDeviceToHost, h->stream));
  ORBX_HIP(h, hipStreamSynchronize(h->stream));
  return ORBX_OK;
}

// The host forms of the collection: the sizes first, then as many rows as they say: two downloads, nothing sized by a bound.
int win_collect_host(orbx_handle* h, const char* who, orbx_map_points* mp, const WinPlan& P, int list_cap, int obs_cap, int* counts, int* local_kf, int* fixed_kf,
                     int* list_slot, double* positions, orbx_ba_obs32* obs32) {
  const bool chain = P.kind != WIN_COVISIBLE, whole = P.kind == WIN_GLOBAL;
  if (list_cap < P.bound || obs_cap < P.n_feat) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d / obs_cap %d are below their bounds %d / %d", who, list_cap, obs_cap, P.bound, P.n_feat);
  if (!counts || (!chain && !local_kf) || (!whole && !fixed_kf) || (P.bound > 0 && (!list_slot || !positions)) || (P.n_feat > 0 && !obs32)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  WinDown w;
  if (int rc = win_collect_down(h, who, mp, P, false, w)) return rc;
  std::memcpy(counts, w.hp + w.o_cn, 16);
  if (!whole) std::memcpy(fixed_kf, w.hp + w.o_fx, 4 * P.kfs.size());
  if (!chain) std::memcpy(local_kf, w.hp + w.o_lk, 4 * (size_t)P.n_local());
  if (int rc = win_check_empty(h, who, P, counts)) return rc;
  const size_t M = (size_t)counts[2], N = (size_t)counts[3];
  Carve rows;
  const size_t r_ls = rows.take(4 * M), r_po = rows.take(24 * M), r_ob = rows.take(16 * N);
  if (int rc = orbx_reserve_pinned(h, h->pin_map, rows.off)) return rc;
  uint8_t* hp = (uint8_t*)h->pin_map.p;
  ORBX_HIP(h, hipMemcpyAsync(hp + r_ls, w.d + w.o_ls, 4 * M, hipMemcpyDeviceToHost, h->stream));
  ORBX_HIP(h, hipMemcpyAsync(hp + r_po, w.d + w.o_po, 24 * M, hipMemcpyDeviceToHost, h->stream));
  ORBX_HIP(h, hipMemcpyAsync(hp + r_ob, w.d + w.o_ob, 16 * N, hipMemcpyDeviceToHost, h->stream));
  ORBX_HIP(h, hipStreamSynchronize(h->stream));
  std::memcpy(list_slot, hp + r_ls, 4 * M); std::memcpy(positions, hp + r_po, 24 * M); std::memcpy(obs32, hp + r_ob, 16 * N);
  return ORBX_OK;
}

// Local BA on a planned window: collect_*_ba_data (local_ba_lm.rs:800-897, local_inertial_ba.rs:930-1030) on the device with ONE
// download; solve_*_ba (:912-1098, :1074-1275) on the observations where they lie (`in`: the inertial solve's extras; its window
// keyframes' T_wc go in as they are where the visual solve takes T_cw, :825-841, :973-978); the point half of apply_*_ba_results
// (local_mapper.rs:363, :396: only a solve that iterated is applied).  The covisible window answers local_kf_out, the chain fixed_kf_out.
int win_local_ba(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_ba_config* cfg, const BaInertialHost* in, orbx_map_points* mp,
                 const orbx_keyframe* const* kfs, const WinPlan& P, orbx_should_stop_fn should_stop, void* user, int* local_kf_out, int* fixed_kf_out,
                 double* poses_wc_out, int* counts_out, int* iterations, double* initial_error, double* final_error) {
  const bool chain = P.kind == WIN_CHAIN;
  *iterations = 0; *initial_error = 0.0; *final_error = 0.0;
  WinDown w;
  if (int rc = win_collect_down(h, who, mp, P, true, w)) return rc;
  const int* cn = (const int*)(w.hp + w.o_cn);
  const int* fx = (const int*)(w.hp + w.o_fx);
  const int* local = chain ? P.chain.data() : (const int*)(w.hp + w.o_lk);   // [0] the anchor; the window: the chain's from 0, the covisible from 1
  const double* pos = (const double*)(w.hp + w.o_po);
  const int Kw = cn[0], F = cn[1], M = cn[2], N = cn[3];
  std::memcpy(counts_out, cn, 16);
  if (chain) std::memcpy(fixed_kf_out, fx, 4 * P.kfs.size());
  else std::memcpy(local_kf_out, local, 4 * (size_t)P.n_local());
  if (int rc = win_check_empty(h, who, P, cn)) return rc;
  std::vector<double> poses(7 * (size_t)std::max(Kw, 1)), fixed_cw(7 * (size_t)F), points(pos, pos + 3 * (size_t)M);
  std::vector<int> slots((const int*)(w.hp + w.o_ls), (const int*)(w.hp + w.o_ls) + M);
  for (int i = 0; i < Kw; ++i) {
    if (chain) std::memcpy(&poses[7 * (size_t)i], kfs[local[i]]->pose_wc, 56);
    else orbx_pose_inverse(kfs[local[1 + i]]->pose_wc, &poses[7 * (size_t)i]);
  }
  orbx_pose_inverse(kfs[local[0]]->pose_wc, &fixed_cw[0]);
  for (int j = 0; j + 1 < F; ++j) orbx_pose_inverse(kfs[fx[j]]->pose_wc, &fixed_cw[7 * (size_t)(j + 1)]);
  if (int rc = ba_solve_visual(h, cam, cfg, Kw, poses.data(), F, fixed_cw.data(), M, points.data(), N, nullptr, should_stop, user, poses_wc_out, iterations,
                               initial_error, final_error, false, in, (const orbx_ba_obs32*)(w.d + w.o_ob), true))
    return rc;
  if (*iterations > 0) return ms_set(mp, who, slots.data(), M, points.data(), nullptr, true);
  return ORBX_OK;
}

// Global BA on a planned whole map: collect_global_ba_data (global_ba.rs:100-181) on the device with ONE download; T_cw from the keyframes'
// own poses; the whole-map solve (global_ba_kernels.hip) on the observations where they lie; the optimised positions back into the store
// when the solve iterated.  poses_wc_out [n_kfs - 1][7]: the caller applies them (orbx_keyframe_set_pose).
int win_global_ba(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_ba_config* cfg, orbx_map_points* mp, const orbx_keyframe* const* kfs,
                  const WinPlan& P, orbx_should_stop_fn should_stop, void* user, double* poses_wc_out, int* counts_out, int* iterations, double* initial_error,
                  double* final_error) {
  *iterations = 0; *initial_error = 0.0; *final_error = 0.0;
  WinDown w;
  if (int rc = win_collect_down(h, who, mp, P, true, w)) return rc;
  const int* cn = (const int*)(w.hp + w.o_cn);
  const double* pos = (const double*)(w.hp + w.o_po);
  const int K = cn[0], M = cn[2], N = cn[3];
  std::memcpy(counts_out, cn, 16);
  if (int rc = win_check_empty(h, who, P, cn)) return rc;
  if (K < 1) return orbx_fail(h, ORBX_ERR_EMPTY, "%s: global BA needs two keyframes and a map point", who);   // global_ba.rs:194-196
  std::vector<double> poses(7 * (size_t)K), points(pos, pos + 3 * (size_t)M);
  std::vector<int> slots((const int*)(w.hp + w.o_ls), (const int*)(w.hp + w.o_ls) + M);
  double fixed_cw[7];
  orbx_pose_inverse(kfs[0]->pose_wc, fixed_cw);
  for (int i = 0; i < K; ++i) orbx_pose_inverse(kfs[1 + i]->pose_wc, &poses[7 * (size_t)i]);
  if (int rc = gba_solve(h, who, cam, cfg, K, poses.data(), fixed_cw, M, points.data(), N, nullptr, (const orbx_ba_obs32*)(w.d + w.o_ob), true, should_stop, user,
                         poses_wc_out, iterations, initial_error, final_error))
    return rc;
  if (*iterations > 0) return ms_set(mp, who, slots.data(), M, points.data(), nullptr, true);
  return ORBX_OK;
}

// ---- tracking from the store: what the keyframe / slot forms and the local-map forms share --------------------------------
// bound_off [B+1]: the offsets of the lists' host-known bounds.  select(...) enqueues the call's selection into the list outputs.

// The device form's features, poses and outputs (orbx_map_track_frames_device's, in its order).
struct MapTrackDev {
  const orbx_keypoint* d_kp; const uint8_t* d_desc; const int* d_feat_start; const int* d_feat_count; int feat_count_stride, max_feat;
  const double* d_search_poses_wc; const double* d_priors_wc;
  int* d_list_offsets; int* d_list_slot; double* d_positions; uint8_t* d_mp_desc; int* d_offsets; double* d_pts3d; float* d_pts2d; int* d_mp_idx; int* d_feat_idx;
  double* d_poses_wc_out; uint8_t* d_inlier_out; double* d_err_out; orbx_pnp_result* d_pnp_results; int* d_matched; int* d_matched_slot; orbx_track_result* d_results;
};

template <class Select>
int ms_track_device(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg, int n_frames,
                    const int* bound_off, const MapTrackDev& D, Select select) {
  int max_mp = 0;
  if (int rc = track_check(h, cam, cfg, pnp_cfg, n_frames, bound_off, &max_mp, who)) return rc;
  const int B = n_frames, M = bound_off[B];
  if (D.max_feat < 0 || D.feat_count_stride < 1 || !D.d_feat_start || !D.d_feat_count || !D.d_search_poses_wc || !D.d_priors_wc || !D.d_offsets ||
      !D.d_poses_wc_out || !D.d_pnp_results || !D.d_results || (D.max_feat > 0 && (!D.d_kp || !D.d_desc || !D.d_matched || !D.d_matched_slot)) ||
      (M > 0 && (!D.d_pts3d || !D.d_pts2d || !D.d_mp_idx || !D.d_feat_idx || !D.d_inlier_out || !D.d_err_out)))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  if (int rc = select()) return rc;
  TrackArgs A{};
  A.max_feat = D.max_feat; A.fc_stride = D.feat_count_stride;
  A.kp = D.d_kp; A.desc = D.d_desc; A.feat_start = D.d_feat_start; A.feat_count = D.d_feat_count;
  A.positions = D.d_positions; A.mp_desc = D.d_mp_desc; A.mp_off = D.d_list_offsets;
  A.search_poses = D.d_search_poses_wc; A.priors = D.d_priors_wc;
  A.offsets = D.d_offsets; A.pts3d = D.d_pts3d; A.pts2d = D.d_pts2d; A.mp_idx = D.d_mp_idx; A.feat_idx = D.d_feat_idx;
  A.poses_out = D.d_poses_wc_out; A.matched = D.d_matched; A.results = D.d_results;
  if (int rc = track_launch(h, cam, cfg, pnp_cfg, B, max_mp, (size_t)M, A, D.d_inlier_out, D.d_err_out, D.d_pnp_results)) return rc;
  return ms_matched_slot_enqueue(h, B, D.max_feat, D.d_matched, D.d_list_offsets, D.d_list_slot, D.d_matched_slot);
}

// The host form's arrays (orbx_map_track_frames's, in its order); src_slots [S] and local_kf [n_local] are the two forms' extras.
struct MapTrackHost {
  const int* src_slots; size_t S;
  const orbx_keypoint* kp; const uint8_t* desc; const int* feat_offsets; const double* search_poses_wc; const double* priors_wc;
  int list_cap;
  int* local_kf; size_t n_local;
  int* list_offsets; int* list_slot; int* offsets; double* pts3d; float* pts2d; int* mp_idx; int* feat_idx; double* poses_wc_out; uint8_t* inlier_out;
  double* err_out; orbx_pnp_result* pnp_results; int* matched; int* matched_slot; orbx_track_result* results;
};

// select(d_src_slots, d_local_kf, d_list_off, d_list_slot, d_positions, d_mp_desc)
template <class Select>
int ms_track_host(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg, int n_frames,
                  const int* bound_off, const MapTrackHost& H, Select select) {
  int max_feat = 0, max_mp = 0;
  if (int rc = track_check(h, cam, cfg, pnp_cfg, n_frames, bound_off, &max_mp, who)) return rc;
  if (int rc = orbx_check_offsets(h, who, "feat_offsets", "frame", n_frames, H.feat_offsets, &max_feat)) return rc;
  const int* feat_offsets = H.feat_offsets;
  const size_t B = (size_t)n_frames, NF = (size_t)feat_offsets[B], M = (size_t)bound_off[B], mf = (size_t)max_feat, S = H.S, NL = H.n_local;
  if (H.list_cap < 0 || (size_t)H.list_cap < M) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d is below the lists' bound %d", who, H.list_cap, (int)M);
  if (!H.search_poses_wc || !H.priors_wc || !H.list_offsets || !H.offsets || !H.poses_wc_out || !H.pnp_results || !H.results || (S > 0 && !H.src_slots) ||
      (NF > 0 && (!H.kp || !H.desc || !H.matched || !H.matched_slot)) ||
      (M > 0 && (!H.list_slot || !H.pts3d || !H.pts2d || !H.mp_idx || !H.feat_idx || !H.inlier_out || !H.err_out)))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  ORBX_HIP(h, hipSetDevice(h->device));
  // one blob each way: [kp | desc | search poses | priors | feat_start | feat_count | source slots] up,
  // [list offsets | list slots | offsets | pts3d | pts2d | mp_idx | feat_idx | poses | err | pnp records | matched | matched slots |
  //  records | inliers | local keyframes] down, and behind them the gathered positions and descriptors, which stay on the device
  Carve in;
  OutputPlan out;
  const size_t i_kp = in.take(sizeof(orbx_keypoint) * NF), i_de = in.take(32 * NF), i_sp = in.take(56 * B), i_pr = in.take(56 * B), i_fs = in.take(4 * B),
               i_fc = in.take(4 * B), i_ss = in.take(4 * S);
  // (the rows' lengths come down with the offsets: they are copied once those are known; matched / matched_slot are copied frame by frame)
  const auto p_lo = out.add(H.list_offsets, B + 1), p_ls = out.add(H.list_slot, M, true), p_of = out.add(H.offsets, B + 1);
  const auto p_p3 = out.add(H.pts3d, 3 * M, true);
  const auto p_p2 = out.add(H.pts2d, 2 * M, true);
  const auto p_mi = out.add(H.mp_idx, M, true), p_fi = out.add(H.feat_idx, M, true);
  const auto p_ps = out.add(H.poses_wc_out, 7 * B), p_er = out.add(H.err_out, M, true);
  const auto p_pn = out.add(H.pnp_results, B);
  const auto p_ma = out.add((int*)nullptr, B * mf), p_ms = out.add((int*)nullptr, B * mf);
  const auto p_rs = out.add(H.results, B);
  const auto p_in = out.add(H.inlier_out, M, true);
  const auto p_lk = out.add(H.local_kf, NL);
  const size_t o_gp = out.keep(24 * M), o_gd = out.keep(32 * M);
  if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs, in.off)) return rc;
  const HostCall& c = out.call;
  uint8_t *hi = c.hi, *di = c.di, *dout = c.dout;
  if (NF) { std::memcpy(hi + i_kp, H.kp, sizeof(orbx_keypoint) * NF); std::memcpy(hi + i_de, H.desc, 32 * NF); }
  std::memcpy(hi + i_sp, H.search_poses_wc, 56 * B);
  std::memcpy(hi + i_pr, H.priors_wc, 56 * B);
  for (size_t b = 0; b < B; ++b) {
    ((int*)(hi + i_fs))[b] = feat_offsets[b];
    ((int*)(hi + i_fc))[b] = feat_offsets[b + 1] - feat_offsets[b];
  }
  if (S) std::memcpy(hi + i_ss, H.src_slots, 4 * S);
  if (int rc = orbx_host_call_upload(h, c)) return rc;
  int* d_lo = out.dev(p_lo); int* d_ls = out.dev(p_ls);
  if (int rc = select((const int*)(di + i_ss), H.local_kf ? out.dev(p_lk) : nullptr, d_lo, d_ls, (double*)(dout + o_gp), dout + o_gd)) return rc;
  TrackArgs A{};
  A.max_feat = max_feat; A.fc_stride = 1;
  A.kp = (const orbx_keypoint*)(di + i_kp); A.desc = di + i_de; A.feat_start = (const int*)(di + i_fs); A.feat_count = (const int*)(di + i_fc);
  A.positions = (const double*)(dout + o_gp); A.mp_desc = dout + o_gd; A.mp_off = d_lo;
  A.search_poses = (const double*)(di + i_sp); A.priors = (const double*)(di + i_pr);
  A.offsets = out.dev(p_of); A.pts3d = out.dev(p_p3); A.pts2d = out.dev(p_p2); A.mp_idx = out.dev(p_mi);
  A.feat_idx = out.dev(p_fi); A.poses_out = out.dev(p_ps); A.matched = out.dev(p_ma);
  A.results = out.dev(p_rs);
  if (int rc = track_launch(h, cam, cfg, pnp_cfg, n_frames, max_mp, M, A, out.dev(p_in), out.dev(p_er), out.dev(p_pn))) return rc;
  if (int rc = ms_matched_slot_enqueue(h, n_frames, max_feat, A.matched, d_lo, d_ls, out.dev(p_ms))) return rc;
  if (int rc = out.finish(h)) return rc;
  const size_t L = (size_t)H.list_offsets[B], N = (size_t)H.offsets[B];
  if (int rc = out.copy(h, p_ls, L)) return rc;
  for (int rc : {out.copy(h, p_p3, 3 * N), out.copy(h, p_p2, 2 * N), out.copy(h, p_mi, N), out.copy(h, p_fi, N), out.copy(h, p_er, N), out.copy(h, p_in, N)})
    if (rc) return rc;
  for (size_t b = 0; b < B; ++b) {
    const size_t n = (size_t)(feat_offsets[b + 1] - feat_offsets[b]);
    if (n) { std::memcpy(H.matched + feat_offsets[b], out.host(p_ma) + b * mf, 4 * n); std::memcpy(H.matched_slot + feat_offsets[b], out.host(p_ms) + b * mf, 4 * n); }
  }
  return ORBX_OK;
}

// ---- observations (include/orbx.h, "observations from the resident map"; map_point.rs:140-156, local_mapper.rs:421-469, :487-583) ----
// mp.observations, the inverse of the slot tables, for the points a call names:
//   obs_index_kernel      index[slot] = position of the slot in the call's list (row 0 of `first`, EMPTY between calls); count = 0
//   obs_count_kernel      (chunk of a keyframe's features, keyframe) over the de-duplicated tables: an integer atomicAdd on the count
//                         of every indexed point a feature names — a sum, whatever the execution order
//   obs_part_kernel       per MS_CHUNK counts their sum; obs_scan_kernel: a chunk's base = the sums before it (block_sum), the
//                         exclusive scan inside it (BlockScan) -> obs_start, and a copy of it as every point's cursor
//   obs_append_kernel     the count kernel's walk again: (keyframe, feature) goes to the point's segment at atomicAdd(cursor), in
//                         whatever order the hardware takes the features
//   obs_rank_kernel       one thread per entry of a segment of at most OBS_SHORT: the keyframes of a segment are distinct, so the
//                         number of smaller ones is the entry's place by ascending keyframe — that fixes the bytes
//   obs_rank_long_kernel  a workgroup per longer point at a time, the segment's keyframes through LDS in tiles of MS_THREADS
//   obs_restore_kernel    index[slot] = EMPTY again
// Keyframe redundancy (cull_keyframes) needs the counts only: index, count, then
//   red_count_kernel      (chunk of a candidate's features, candidate) over the table WITH repeats: the features whose slot is live,
//                         and those of them whose point has min_observations other observers; block_sum -> the chunk's two sums
//   red_tail_kernel       one thread per candidate: the chunks summed in order, total, redundant, cull (one f64 division)
// and restore.  The candidates' distinct live slots are one frame's ORBX_MAP_SOURCE_KEYFRAMES selection, unchanged.

constexpr int OBS_SHORT = 64;                    // longest segment obs_rank_kernel orders

struct ObsArgs {
  int capacity, n_kfs, n_chunk, min_obs;
  const uint8_t* live; const CovKf* kfs;
  const int* n_list; const int* list_slot;       // the call's points: *n_list slots, none twice
  int* index;                                    // the store's first-sighting table, row 0: EMPTY outside the launches below
  int* count; int* part; int* cursor;            // [points]; [chunks of points]; [points]
  int* tmp_kf; int* tmp_feat;                    // the segments before they are ordered
  int* obs_start; int* obs_kf; int* obs_feat;
  const int* cand; int n_cand; double threshold; // redundancy
  int* chunk_tot; int* total; int* redundant; uint8_t* cull;
};

__global__ __launch_bounds__(MS_THREADS) void obs_index_kernel(ObsArgs A) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i < *A.n_list) { A.index[A.list_slot[i]] = i; A.count[i] = 0; }
}
__global__ __launch_bounds__(MS_THREADS) void obs_restore_kernel(ObsArgs A) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i < *A.n_list) A.index[A.list_slot[i]] = MS_EMPTY;
}

// does feature i of `kf` observe a point of the call (the first feature of the keyframe that names it)?  -> its position, or -1
__device__ __forceinline__ int obs_point(const ObsArgs& A, const CovKf& kf, int i) {
  if (i >= kf.n) return -1;
  const int s = kf.uniq[i];
  if (s < 0 || s >= A.capacity || !A.live[s]) return -1;
  const int p = A.index[s];
  return p == MS_EMPTY ? -1 : p;
}

__global__ __launch_bounds__(MS_THREADS) void obs_count_kernel(ObsArgs A) {
  const CovKf kf = A.kfs[blockIdx.y];
  if (!kf.uniq) return;
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) {
    const int p = obs_point(A, kf, blockIdx.x * MS_CHUNK + j * MS_THREADS + threadIdx.x);
    if (p >= 0) atomicAdd(&A.count[p], 1);
  }
}

__global__ __launch_bounds__(MS_THREADS) void obs_part_kernel(ObsArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int n = *A.n_list, p0 = blockIdx.x * MS_CHUNK + threadIdx.x * MS_PER;
  int c = 0;
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) c += p0 + j < n ? A.count[p0 + j] : 0;
  c = block_sum<MS_THREADS>(c, wave_tot);
  if (threadIdx.x == 0) A.part[blockIdx.x] = c;
}

__global__ __launch_bounds__(MS_THREADS) void obs_scan_kernel(ObsArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int n = *A.n_list, tid = threadIdx.x, p0 = blockIdx.x * MS_CHUNK + tid * MS_PER;
  int before = 0;
  for (int j = tid; j < (int)blockIdx.x; j += MS_THREADS) before += A.part[j];
  const int base = block_sum<MS_THREADS>(before, wave_tot);
  int c[MS_PER], mine = 0;
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) { c[j] = p0 + j < n ? A.count[p0 + j] : 0; mine += c[j]; }
  int at = BlockScan<MS_THREADS>(wave_tot, base).round(mine);
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) {
    if (p0 + j < n) { A.obs_start[p0 + j] = at; A.cursor[p0 + j] = at; }
    at += c[j];
    if (p0 + j + 1 == n) A.obs_start[n] = at;
  }
  if (n == 0 && blockIdx.x == 0 && tid == 0) A.obs_start[0] = 0;
}

__global__ __launch_bounds__(MS_THREADS) void obs_append_kernel(ObsArgs A) {
  const int k = blockIdx.y;
  const CovKf kf = A.kfs[k];
  if (!kf.uniq) return;
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) {
    const int i = blockIdx.x * MS_CHUNK + j * MS_THREADS + threadIdx.x;
    const int p = obs_point(A, kf, i);
    if (p < 0) continue;
    const int at = atomicAdd(&A.cursor[p], 1);
    A.tmp_kf[at] = k; A.tmp_feat[at] = i;
  }
}

__global__ __launch_bounds__(MS_THREADS) void obs_rank_kernel(ObsArgs A) {
  const int n = *A.n_list, e = blockIdx.x * MS_THREADS + threadIdx.x;
  if (e >= A.obs_start[n]) return;
  int lo = 0, hi = n;                                                      // the point that owns e: the last one that starts at or before it
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (A.obs_start[mid] <= e) lo = mid + 1; else hi = mid;
  }
  const int s = A.obs_start[lo - 1], len = A.obs_start[lo] - s;
  if (len > OBS_SHORT) return;
  const int k = A.tmp_kf[e];
  int rank = 0;
  for (int j = 0; j < len; ++j) rank += A.tmp_kf[s + j] < k;
  A.obs_kf[s + rank] = k; A.obs_feat[s + rank] = A.tmp_feat[e];
}

__global__ __launch_bounds__(MS_THREADS) void obs_rank_long_kernel(ObsArgs A) {
  __shared__ int tile[MS_THREADS];
  const int n = *A.n_list, tid = threadIdx.x;
  for (int p = blockIdx.x; p < n; p += gridDim.x) {                        // (p, s and len are the block's: every thread takes every barrier)
    const int s = A.obs_start[p], len = A.obs_start[p + 1] - s;
    if (len <= OBS_SHORT) continue;
    for (int i0 = 0; i0 < len; i0 += MS_THREADS) {
      const int i = i0 + tid;
      const int k = i < len ? A.tmp_kf[s + i] : 0;
      int rank = 0;
      for (int j0 = 0; j0 < len; j0 += MS_THREADS) {
        __syncthreads();
        tile[tid] = j0 + tid < len ? A.tmp_kf[s + j0 + tid] : 0x7fffffff;
        __syncthreads();
        const int m = min(MS_THREADS, len - j0);
        for (int t = 0; t < m; ++t) rank += tile[t] < k;
      }
      if (i < len) { A.obs_kf[s + rank] = k; A.obs_feat[s + rank] = A.tmp_feat[s + i]; }
    }
  }
}

// rows of the listed slots as the refresh reads them: positions [M][3] and the current descriptors [M][32]
__global__ __launch_bounds__(MS_THREADS) void obs_gather_kernel(const int* slots, int n, const double* pos, const uint8_t* desc, double* out_pos, uint8_t* out_desc) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= n) return;
  const size_t s = (size_t)slots[i];
  out_pos[3 * (size_t)i] = pos[3 * s]; out_pos[3 * (size_t)i + 1] = pos[3 * s + 1]; out_pos[3 * (size_t)i + 2] = pos[3 * s + 2];
  const uint32_t* d = (const uint32_t*)(desc + 32 * s);
  uint32_t* q = (uint32_t*)(out_desc + 32 * (size_t)i);
#pragma unroll
  for (int k = 0; k < 8; ++k) q[k] = d[k];
}

__global__ __launch_bounds__(MS_THREADS) void red_count_kernel(ObsArgs A) {
  __shared__ int wave_tot[(MS_THREADS / 64) * 2];
  const CovKf kf = A.kfs[A.cand[blockIdx.y]];
  int v[2] = {0, 0};
  if (kf.slots) {
#pragma unroll
    for (int j = 0; j < MS_PER; ++j) {
      const int i = blockIdx.x * MS_CHUNK + j * MS_THREADS + threadIdx.x;
      if (i >= kf.n) continue;
      const int s = kf.slots[i];
      if (s < 0 || s >= A.capacity || !A.live[s]) continue;
      ++v[0];
      const int p = A.index[s];                                            // (every live slot of a candidate is in the list)
      if (p != MS_EMPTY && A.count[p] - 1 >= A.min_obs) ++v[1];
    }
  }
  block_sum<MS_THREADS, 2>(v, wave_tot);
  if (threadIdx.x < 2) A.chunk_tot[2 * ((size_t)blockIdx.y * A.n_chunk + blockIdx.x) + threadIdx.x] = v[threadIdx.x];
}

__global__ __launch_bounds__(MS_THREADS) void red_tail_kernel(ObsArgs A) {
  const int c = blockIdx.x * MS_THREADS + threadIdx.x;
  if (c >= A.n_cand) return;
  int total = 0, red = 0;
  for (int j = 0; j < A.n_chunk; ++j) { total += A.chunk_tot[2 * ((size_t)c * A.n_chunk + j)]; red += A.chunk_tot[2 * ((size_t)c * A.n_chunk + j) + 1]; }
  A.total[c] = total; A.redundant[c] = red;
  A.cull[c] = total > 0 && (double)red / (double)total > A.threshold ? 1 : 0;     // local_mapper.rs:561-565
}

// The keyframes of an observation call, checked as covisibility checks its own, and the host-known bound of the entries.
struct ObsPlan {
  CovPlan C;
  int n_feat = 0;
};

int obs_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, ObsPlan& P) {
  if (int rc = cov_plan(h, who, mp, n_kfs, kfs, 0, P.C)) return rc;
  if (int rc = ms_check_grid_keyframes(h, who, n_kfs)) return rc;
  long long total = 0;
  for (const CovKf& k : P.C.kfs) total += k.n;
  if (total > 0x7fff0000) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the keyframes hold more than 2^31 - 65536 features", who);
  P.n_feat = (int)total;
  return ORBX_OK;
}

// slots [M] of an observation call: what orbx_map_points_set asks of its own, and live in the store's host mirror
int obs_check_slots(orbx_map_points* mp, const char* who, const int* slots, int M) {
  if (int rc = ms_check_slots(mp, who, slots, M, true)) return rc;
  for (int i = 0; i < M; ++i)
    if (!mp->live[(size_t)slots[i]]) return orbx_fail(mp->h, ORBX_ERR_INVALID, "%s: slot %d (entry %d) is not live", who, slots[i], i);
  return ORBX_OK;
}

// What obs_enqueue is asked for.  The points: `slots` (host [n_points], checked) or, where slots is NULL, a list a selection left
// in device memory (d_slots, its length in *d_n, at most n_points).  Lists: the three outputs; redundancy: cand and its outputs.
struct ObsCall {
  int n_points = 0;
  const int* slots = nullptr; const int* d_n = nullptr; const int* d_slots = nullptr;
  int* d_obs_start = nullptr; int* d_obs_kf = nullptr; int* d_obs_feat = nullptr;
  int n_cand = 0, min_obs = 0; const int* cand = nullptr; double threshold = 0.0;
  int* d_total = nullptr; int* d_redundant = nullptr; uint8_t* d_cull = nullptr;
};

// entries the lists of n_points points can hold: every feature once, and no point more often than there are keyframes
int obs_entry_bound(const ObsPlan& P, int n_points) { return (int)std::min<long long>(P.n_feat, (long long)n_points * (long long)P.C.kfs.size()); }

// Everything on the handle's stream.  The tables (keyframes, slots, candidates) go up through the ring; d_slots_out: where the
// points' slots lie in device memory afterwards; d_count_out: where their observer counts lie (until the next observation call).
int obs_enqueue(orbx_handle* h, orbx_map_points* mp, const ObsPlan& P, const ObsCall& c, const int** d_slots_out = nullptr, const int** d_count_out = nullptr) {
  ORBX_HIP(h, hipSetDevice(h->device));
  if (int rc = ms_reserve_first(h, mp, 1)) return rc;
  const size_t K = P.C.kfs.size(), Mb = (size_t)c.n_points, Nb = c.d_obs_start ? (size_t)obs_entry_bound(P, c.n_points) : 0, NC = (size_t)c.n_cand;
  const int n_chunk = std::max(1, (P.C.max_n + MS_CHUNK - 1) / MS_CHUNK), n_part = std::max(1, (int)((Mb + MS_CHUNK - 1) / MS_CHUNK));
  UploadPlan up;
  Carve ws;
  const size_t o_kf = up.put(P.C.kfs.data(), sizeof(CovKf) * K), o_n = up.put(&c.n_points, 4), o_sl = up.put(c.slots, c.slots ? 4 * Mb : 0), o_ca = up.put(c.cand, 4 * NC);
  const size_t o_cn = ws.take(4 * Mb), o_cu = ws.take(4 * Mb), o_pa = ws.take(4 * (size_t)n_part), o_tk = ws.take(4 * Nb), o_tf = ws.take(4 * Nb),
               o_ct = ws.take(8 * NC * (size_t)n_chunk);
  if (int rc = up.send(h, h->ring_map, h->ws_map.obs_tables)) return rc;
  uint8_t* const ds = up.device;
  if (int rc = orbx_reserve(h, h->ws_map.obs_scratch, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.obs_scratch.p;
  ObsArgs A{};
  A.capacity = mp->capacity; A.n_kfs = (int)K; A.n_chunk = n_chunk; A.min_obs = c.min_obs;
  A.live = mp->d_live; A.kfs = (const CovKf*)(ds + o_kf);
  A.n_list = c.slots ? (const int*)(ds + o_n) : c.d_n; A.list_slot = c.slots ? (const int*)(ds + o_sl) : c.d_slots;
  A.index = (int*)mp->first.p;
  A.count = (int*)(w + o_cn); A.part = (int*)(w + o_pa); A.cursor = (int*)(w + o_cu); A.tmp_kf = (int*)(w + o_tk); A.tmp_feat = (int*)(w + o_tf);
  A.obs_start = c.d_obs_start; A.obs_kf = c.d_obs_kf; A.obs_feat = c.d_obs_feat;
  A.cand = (const int*)(ds + o_ca); A.n_cand = c.n_cand; A.threshold = c.threshold;
  A.chunk_tot = (int*)(w + o_ct); A.total = c.d_total; A.redundant = c.d_redundant; A.cull = c.d_cull;
  if (d_slots_out) *d_slots_out = A.list_slot;
  if (d_count_out) *d_count_out = A.count;
  const dim3 block(MS_THREADS), list_grid(std::max(1, (int)((Mb + MS_THREADS - 1) / MS_THREADS))), kf_grid(n_chunk, (unsigned)K);
  const bool walk = K > 0 && P.C.max_n > 0 && Mb > 0;
  orbx_launch(h, "obs_index_kernel", false, obs_index_kernel, list_grid, block, 0, A);
  if (walk) orbx_launch(h, "obs_count_kernel", true, obs_count_kernel, kf_grid, block, 0, A);
  if (c.d_obs_start) {
    orbx_launch(h, "obs_part_kernel", true, obs_part_kernel, dim3(n_part), block, 0, A);
    orbx_launch(h, "obs_scan_kernel", true, obs_scan_kernel, dim3(n_part), block, 0, A);
    if (walk && Nb > 0) {
      orbx_launch(h, "obs_append_kernel", true, obs_append_kernel, kf_grid, block, 0, A);
      orbx_launch(h, "obs_rank_kernel", true, obs_rank_kernel, dim3((unsigned)((Nb + MS_THREADS - 1) / MS_THREADS)), block, 0, A);
      if (K > (size_t)OBS_SHORT)                                            // (a segment is never longer than the call has keyframes)
        orbx_launch(h, "obs_rank_long_kernel", true, obs_rank_long_kernel, dim3((unsigned)std::min<size_t>(Mb, 4 * (size_t)h->n_cu)), block, 0, A);
    }
  }
  if (NC) {
    orbx_launch(h, "red_count_kernel", true, red_count_kernel, dim3(n_chunk, (unsigned)NC), block, 0, A);
    orbx_launch(h, "red_tail_kernel", true, red_tail_kernel, dim3((unsigned)((NC + MS_THREADS - 1) / MS_THREADS)), block, 0, A);
  }
  orbx_launch(h, "obs_restore_kernel", true, obs_restore_kernel, list_grid, block, 0, A);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// orbx_map_observations[_device]: the checks, then the lists into device memory
int obs_lists_call(orbx_handle* h, const char* who, orbx_map_points* mp, const ObsPlan& P, int M, const int* slots, int obs_cap, int* d_obs_start, int* d_obs_kf,
                   int* d_obs_feat) {
  if (obs_cap < P.n_feat) return orbx_fail(h, ORBX_ERR_INVALID, "%s: obs_cap %d is below the observations' bound %d (the features of kfs[] summed)", who, obs_cap, P.n_feat);
  if (!d_obs_start || (P.n_feat > 0 && M > 0 && (!d_obs_kf || !d_obs_feat))) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  ObsCall c;
  c.n_points = M; c.slots = slots; c.d_obs_start = d_obs_start; c.d_obs_kf = d_obs_kf; c.d_obs_feat = d_obs_feat;
  return obs_enqueue(h, mp, P, c);
}

// orbx_map_refresh_points[_device] behind their checks: the lists, the points' rows out of the store, mappoint_kernels.hip's
// launches on them, the chosen descriptors back into the store.  Every pointer is device memory, slots a host array.
int obs_refresh_enqueue(orbx_handle* h, const char* who, orbx_map_points* mp, const ObsPlan& P, const orbx_keyframe* const* kfs, int M, const int* slots,
                        double scale_range, const double* d_normals_in, uint8_t* d_mp_desc, double* d_normals, double* d_min_distance, double* d_max_distance,
                        orbx_mp_refresh_record* d_records) {
  const size_t Mz = (size_t)M, Nb = (size_t)obs_entry_bound(P, M), T = P.C.kfs.size();
  std::vector<MapPointKf> tab(T);
  for (size_t t = 0; t < T; ++t) {
    tab[t].desc = kfs[t]->d_desc; tab[t].n = kfs[t]->n; tab[t].pad_ = 0;
    std::memcpy(tab[t].centre, kfs[t]->pose_wc + 4, sizeof(tab[t].centre));
  }
  Carve ws;
  const size_t o_os = ws.take(4 * (Mz + 1)), o_ok = ws.take(4 * Nb), o_of = ws.take(4 * Nb), o_po = ws.take(24 * Mz);
  if (int rc = orbx_reserve(h, h->ws_map.refresh_lists, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.refresh_lists.p;
  ObsCall c;
  c.n_points = M; c.slots = slots; c.d_obs_start = (int*)(w + o_os); c.d_obs_kf = (int*)(w + o_ok); c.d_obs_feat = (int*)(w + o_of);
  const int* d_slots = nullptr;
  if (int rc = obs_enqueue(h, mp, P, c, &d_slots)) return rc;
  const dim3 grid((M + MS_THREADS - 1) / MS_THREADS), block(MS_THREADS);
  orbx_launch(h, "obs_gather_kernel", true, obs_gather_kernel, grid, block, 0, d_slots, M, (const double*)mp->d_pos, (const uint8_t*)mp->d_desc, (double*)(w + o_po), d_mp_desc);
  ORBX_HIP(h, hipGetLastError());
  // the entries' host-known bound stands in for obs_start[M]: the kernels take every length from obs_start itself
  if (int rc = mp_refresh_enqueue(h, who, M, (int)Nb, (const double*)(w + o_po), c.d_obs_start, c.d_obs_kf, c.d_obs_feat, (int)T, tab.data(), scale_range, d_mp_desc,
                                  d_normals_in, d_mp_desc, d_normals, d_min_distance, d_max_distance, d_records))
    return rc;
  orbx_launch(h, "map_scatter_kernel", false, map_scatter_kernel, grid, block, 0, d_slots, M, (const double*)nullptr, (const uint8_t*)d_mp_desc, 1, mp->d_pos, mp->d_desc,
              mp->d_live);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// A redundancy call, checked and sized on the host: the keyframes, and the candidates as one frame of a selection.
struct RedPlan {
  ObsPlan O;
  SelPlan S;
};

int red_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_cand, const int* cand,
             int min_observations, RedPlan& P) {
  if (int rc = obs_plan(h, who, mp, n_kfs, kfs, P.O)) return rc;
  if (n_cand < 0 || n_cand > 0xffff) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (0 <= n_cand <= 65535)", who);
  if (min_observations < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: min_observations must not be negative", who);
  if (int rc = cov_check_queries(h, who, "cand", n_cand, cand, n_kfs, 0)) return rc;
  if (n_cand == 0) return ORBX_OK;
  std::vector<const orbx_keyframe*> ck((size_t)n_cand);
  for (int i = 0; i < n_cand; ++i) ck[(size_t)i] = kfs[cand[i]];
  const int off[2] = {0, n_cand};
  return ms_plan(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, ck.data(), off, nullptr, P.S);
}

// The candidates' distinct live slots by the selection (its gathered rows stay in the workspace), then counts and sums.
int red_enqueue(orbx_handle* h, const char* who, orbx_map_points* mp, const RedPlan& P, int n_cand, const int* cand, int min_observations, double threshold,
                int* d_total, int* d_redundant, uint8_t* d_cull) {
  if (!d_total || !d_redundant || !d_cull) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  const int bound = P.S.bound_off[1];
  Carve ws;
  const size_t o_lo = ws.take(8), o_ls = ws.take(4 * (size_t)bound), o_po = ws.take(24 * (size_t)bound), o_de = ws.take(32 * (size_t)bound);
  if (int rc = orbx_reserve(h, h->ws_map.refresh_lists, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.refresh_lists.p;
  if (int rc = ms_select_enqueue(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, P.S, nullptr, nullptr, bound, (int*)(w + o_lo), (int*)(w + o_ls), (double*)(w + o_po),
                                 w + o_de))
    return rc;
  ObsCall c;
  c.n_points = bound; c.d_n = (const int*)(w + o_lo) + 1; c.d_slots = (const int*)(w + o_ls);
  c.n_cand = n_cand; c.cand = cand; c.min_obs = min_observations; c.threshold = threshold;
  c.d_total = d_total; c.d_redundant = d_redundant; c.d_cull = d_cull;
  return obs_enqueue(h, mp, P.O, c);
}

// ---- fuse and merge (include/orbx.h, "fuse and merge on the resident map"; search_in_neighbors.rs:240-390, map.rs:770-...) ----
// One pass fuse(src, tgt) over the tables where they lie.  L is one frame's ORBX_MAP_SOURCE_KEYFRAMES selection, unchanged, with its
// gathered positions and descriptors; the marks are cov_mark_kernel's, one row per target; the observer counts obs_count_kernel's.
// A node is a slot the pass may merge: L's entry j is node j; a live slot a matched feature names that is not in L is node
// P + (the lowest j * n_tgt + t of the matches that name it).  index[slot] (row 0 of `first`) holds the node.
//   mf_begin_kernel    index[L[j]] = j; counts = {P, 0, 0, 0}
//   mf_search_kernel   (128 points, target): the mark test, then fuse_search_dev.hpp's search on the target's own arrays -> match
//   mf_name_kernel     per match the live slot its feature names (atomicMin of the node on index) or a claim (atomicMin of j on
//                      the feature's cell: the claimants of a feature meet in the lowest of them); the matches counted
//   mf_class_kernel    one workgroup: every match is an edge (j, named node) or (j, lowest claimant); minimum-label propagation with
//                      integer atomicMin to the fixed point — every node ends with the lowest node of its component
//   mf_key_kernel      per class: packed (observers, order) maximum -> the keeper; members; whether it has a claim
//   mf_goner_kernel    the members of classes of two or more that are not the keeper, through an atomic cursor;
//   mf_goner_rank_kernel  the slots are distinct, so the number of smaller ones is a goner's place: that fixes the bytes
//   mf_feat_kernel     (chunk, keyframe) over ALL keyframes: the class a feature belongs to by its entry or by a claim, and whether it
//                      names the keeper
//   mf_rewrite_kernel  (chunk, keyframe) every feature of a class walks its keyframe's features through LDS: does one name the keeper,
//                      which is the lowest of the class; the new entry; the keyframes that changed; the associations counted
//   mf_uniq_kernel     (chunk, keyframe) of a changed keyframe: d_mp_uniq again — an entry stays where no earlier feature holds it
//   mf_restore_kernel  index back to EMPTY for L and every named slot
// Every atomic is an integer min, max or add: the outputs are the same bytes whatever the execution order.

constexpr int MF_CLASS_THREADS = 1024;

struct MfTgt {                                   // one target of a pass
  const orbx_keypoint* kp; const uint8_t* desc;  // where the resident keyframe keeps them
  const int* slots;                              // its table WITH repeats
  int n, feat_off;                               // its features; where they start among the targets' features (the claim cells)
  double pose_cw[7];                             // the inverse of pose_wc, made on the host as orbx_fuse_search_device makes it
};
struct MfKf {                                    // one keyframe of kfs[] as the rewrite sees it
  int* slots; int* uniq;                         // NULL: no table
  int n, feat_off;                               // its features; where they start among all features of kfs[]
  int tgt, pad_;                                 // its place in tgt[], -1: not a target
};
struct MfArgs {
  orbx_camera cam;
  double radius_scale;
  unsigned thr;
  int capacity, n_kfs, n_tgt;
  const uint8_t* live; const uint8_t* mark;
  const MfTgt* tgts; const MfKf* kfs;
  const int* list_off; const int* list_slot; const double* list_pos; const uint8_t* list_desc;      // the selection's outputs: P = list_off[1]
  int* index;                                    // the store's first-sighting table, row 0: EMPTY outside the launches below
  int* match; int* match_e; int* edge;           // [P][n_tgt]: the feature; the live slot it names (-1: a claim, or no match); the other end's node
  int* claim;                                    // [targets' features] the lowest claimant, EMPTY: none
  int* nobs; int* label;                         // [nodes]
  unsigned long long* key; int* csize; int* cclaim;   // [nodes], read at a class's label
  int* feat_cls;                                 // [features of kfs[]] class label * 2 + (names the keeper), -1: in no class that changes a table
  int* changed;                                  // [n_kfs]
  int* cursor; int* tmp_goner; int* tmp_keeper;
  int* counts; int* goner; int* keeper;
};

__device__ __forceinline__ bool mf_live(const MfArgs& A, int s) { return s >= 0 && s < A.capacity && A.live[s]; }
// the slot behind a class's key: an entry of L (high bit: 0x7fffffff - j below it) or a slot outside it (0x7fffffff - slot)
__device__ __forceinline__ int mf_key_slot(const MfArgs& A, unsigned long long key) {
  const unsigned low = (unsigned)key;
  return (low & 0x80000000u) ? A.list_slot[0x7fffffff - (int)(low & 0x7fffffffu)] : 0x7fffffff - (int)low;
}
// node id -> (is it a node, its slot, the order half of its key)
__device__ __forceinline__ bool mf_node(const MfArgs& A, int P, int id, int* slot, unsigned* low) {
  if (id < P) { *slot = A.list_slot[id]; *low = 0x80000000u | (unsigned)(0x7fffffff - id); return true; }
  const int m = id - P;
  if (A.match[m] < 0) return false;
  const int e = A.match_e[m];
  if (e < 0 || A.index[e] != id) return false;
  *slot = e; *low = (unsigned)(0x7fffffff - e);
  return true;
}

__global__ __launch_bounds__(MS_THREADS) void mf_begin_kernel(MfArgs A, int with_index) {
  const int P = A.list_off ? A.list_off[1] : 0, i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (with_index && i < P) A.index[A.list_slot[i]] = i;
  if (i < 4) A.counts[i] = i == 0 ? P : 0;
}

__global__ __launch_bounds__(FUSE_THREADS) void mf_search_kernel(MfArgs A) {
  __shared__ FuseLds lds;
  const int P = A.list_off[1], t = blockIdx.y, j = blockIdx.x * FUSE_THREADS + threadIdx.x;
  if ((int)(blockIdx.x * FUSE_THREADS) >= P) return;                       // (the block's: every thread of a block that stays reaches the barriers)
  const MfTgt g = A.tgts[t];
  const size_t jc = (size_t)(j < P ? j : 0);
  const bool valid = j < P && !A.mark[(size_t)t * A.capacity + A.list_slot[jc]];      // :272, in front of the projection
  const unsigned long long best = fuse_search_point(A.cam, valid, A.list_pos + 3 * jc, A.list_desc + 32 * jc, A.tgts[t].pose_cw, g.kp, g.desc, g.n,
                                                    A.radius_scale, A.thr, lds);
  if (j < P) A.match[(size_t)j * A.n_tgt + t] = best == ~0ull ? -1 : (int)(unsigned)(best & 0xffffffffull);
}

__global__ __launch_bounds__(MS_THREADS) void mf_name_kernel(MfArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const int P = A.list_off[1], T = A.n_tgt, m = blockIdx.x * MS_THREADS + threadIdx.x;
  int hit = 0;
  if (m < P * T) {
    const int f = A.match[m];
    int e = -1;
    if (f >= 0) {
      const int j = m / T;
      const MfTgt& g = A.tgts[m - j * T];
      hit = 1;
      e = g.slots[f];
      if (mf_live(A, e)) atomicMin(&A.index[e], P + m);
      else { e = -1; atomicMin(&A.claim[g.feat_off + f], j); }
    }
    A.match_e[m] = e;
  }
  hit = block_sum<MS_THREADS>(hit, wave_tot);
  if (threadIdx.x == 0 && hit) atomicAdd(&A.counts[1], hit);
}

__global__ __launch_bounds__(MF_CLASS_THREADS) void mf_class_kernel(MfArgs A) {
  __shared__ int again;
  const int P = A.list_off[1], T = A.n_tgt, M = P * T, N = P + M, tid = threadIdx.x;
  for (int id = tid; id < N; id += MF_CLASS_THREADS) A.label[id] = id;
  for (int m = tid; m < M; m += MF_CLASS_THREADS) {
    const int f = A.match[m];
    int o = -1;
    if (f >= 0) {
      const int e = A.match_e[m];
      o = e >= 0 ? A.index[e] : A.claim[A.tgts[m % T].feat_off + f];
    }
    A.edge[m] = o;
  }
  __threadfence();
  for (;;) {
    __syncthreads();                                                       // (the labels and edges written above; the flag read below)
    if (tid == 0) again = 0;
    __syncthreads();
    bool moved = false;
    for (int m = tid; m < M; m += MF_CLASS_THREADS) {
      const int o = A.edge[m];
      if (o < 0) continue;
      const int a = m / T;
      const int la = __hip_atomic_load(&A.label[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int lb = __hip_atomic_load(&A.label[o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (la == lb) continue;
      const int lo = min(la, lb);
      atomicMin(&A.label[a], lo); atomicMin(&A.label[o], lo);
      atomicMin(&A.label[max(la, lb)], lo);                                // (the higher label's own node: its other members follow in the step below)
      moved = true;
    }
    __syncthreads();
    for (int id = tid; id < N; id += MF_CLASS_THREADS) {
      const int l = __hip_atomic_load(&A.label[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int ll = __hip_atomic_load(&A.label[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ll < l) { atomicMin(&A.label[id], ll); moved = true; }
    }
    if (moved) again = 1;
    __syncthreads();
    if (!again) break;                                                     // (the same in every thread: nothing writes it before the next barrier)
  }
}

__global__ __launch_bounds__(MS_THREADS) void mf_key_kernel(MfArgs A) {
  const int P = A.list_off[1], id = blockIdx.x * MS_THREADS + threadIdx.x;
  if (id >= P + P * A.n_tgt) return;
  int slot; unsigned low;
  if (mf_node(A, P, id, &slot, &low)) {
    const int c = A.label[id];
    atomicMax(&A.key[c], ((unsigned long long)(unsigned)A.nobs[id] << 32) | low);
    atomicAdd(&A.csize[c], 1);
  }
  if (id >= P && A.match[id - P] >= 0 && A.match_e[id - P] < 0) A.cclaim[A.label[(id - P) / A.n_tgt]] = 1;
}

__global__ __launch_bounds__(MS_THREADS) void mf_goner_kernel(MfArgs A) {
  const int P = A.list_off[1], id = blockIdx.x * MS_THREADS + threadIdx.x;
  if (id >= P + P * A.n_tgt) return;
  int slot; unsigned low;
  if (!mf_node(A, P, id, &slot, &low)) return;
  const int c = A.label[id];
  const unsigned long long key = A.key[c];
  if (A.csize[c] < 2 || (unsigned)key == low) return;
  const int at = atomicAdd(A.cursor, 1);
  A.tmp_goner[at] = slot; A.tmp_keeper[at] = mf_key_slot(A, key);
}

__global__ __launch_bounds__(MS_THREADS) void mf_goner_rank_kernel(MfArgs A) {
  __shared__ int tile[MS_THREADS];
  const int G = *A.cursor, tid = threadIdx.x, e = blockIdx.x * MS_THREADS + tid;
  if (blockIdx.x == 0 && tid == 0) A.counts[3] = G;
  if ((int)(blockIdx.x * MS_THREADS) >= G) return;                         // (the block's)
  const int s = e < G ? A.tmp_goner[e] : 0x7fffffff;
  int rank = 0;
  for (int j0 = 0; j0 < G; j0 += MS_THREADS) {
    __syncthreads();
    tile[tid] = j0 + tid < G ? A.tmp_goner[j0 + tid] : 0x7fffffff;
    __syncthreads();
    const int n = min(MS_THREADS, G - j0);
    for (int t = 0; t < n; ++t) rank += tile[t] < s;
  }
  if (e < G) { A.goner[rank] = s; A.keeper[rank] = A.tmp_keeper[e]; }
}

__global__ __launch_bounds__(MS_THREADS) void mf_feat_kernel(MfArgs A) {
  const MfKf kf = A.kfs[blockIdx.y];
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= kf.n) return;
  int cls = -1;
  if (kf.slots) {
    const int e = kf.slots[i];
    if (mf_live(A, e)) {
      const int id = A.index[e];
      if (id != MS_EMPTY) {
        const int c = A.label[id];
        if (A.csize[c] >= 2 || A.cclaim[c]) cls = 2 * c + (mf_key_slot(A, A.key[c]) == e ? 1 : 0);
      }
    } else if (kf.tgt >= 0) {
      const int j = A.claim[A.tgts[kf.tgt].feat_off + i];
      if (j != MS_EMPTY) cls = 2 * A.label[j];
    }
  }
  A.feat_cls[kf.feat_off + i] = cls;
}

__global__ __launch_bounds__(MS_THREADS) void mf_rewrite_kernel(MfArgs A) {
  __shared__ int tile[MS_THREADS];
  __shared__ int wave_tot[MS_THREADS / 64];
  const MfKf kf = A.kfs[blockIdx.y];
  const int tid = threadIdx.x, i = blockIdx.x * MS_THREADS + tid;
  if (!kf.slots || (int)(blockIdx.x * MS_THREADS) >= kf.n) return;         // (the block's)
  const int* cls = A.feat_cls + kf.feat_off;
  const int mine = i < kf.n ? cls[i] : -1;
  if (!__syncthreads_or(mine >= 0)) return;
  const int c = mine >> 1;
  int lowest = -1;
  bool names = false;
  for (int j0 = 0; j0 < kf.n; j0 += MS_THREADS) {
    __syncthreads();
    tile[tid] = j0 + tid < kf.n ? cls[j0 + tid] : -1;
    __syncthreads();
    if (mine < 0) continue;
    const int n = min(MS_THREADS, kf.n - j0);
    for (int t = 0; t < n; ++t) {
      const int v = tile[t];
      if (v < 0 || (v >> 1) != c) continue;
      names |= (v & 1) != 0;
      if (lowest < 0) lowest = j0 + t;
    }
  }
  int added = 0;
  if (mine >= 0) {
    const int old = kf.slots[i];
    const int now = names ? ((mine & 1) ? old : -1) : i == lowest ? mf_key_slot(A, A.key[c]) : -1;
    if (now != old) { kf.slots[i] = now; A.changed[blockIdx.y] = 1; }
    added = now >= 0 && !mf_live(A, old);
  }
  added = block_sum<MS_THREADS>(added, wave_tot);
  if (tid == 0 && added) atomicAdd(&A.counts[2], added);
}

// d_mp_uniq of the block's MS_THREADS features of one table: an entry stays where no earlier feature holds it.  Every thread of
// the block reaches the barriers; tile: LDS [MS_THREADS].
__device__ __forceinline__ void uniq_rows(const int* slots, int* uniq, int n_feat, int* tile) {
  const int tid = threadIdx.x, i = blockIdx.x * MS_THREADS + tid;
  const int s = i < n_feat ? slots[i] : -1;
  bool earlier = false;
  for (int j0 = 0; j0 <= (int)(blockIdx.x * MS_THREADS); j0 += MS_THREADS) {
    __syncthreads();
    tile[tid] = j0 + tid < n_feat ? slots[j0 + tid] : -1;
    __syncthreads();
    const int n = min(MS_THREADS, i - j0);                                 // the features before i
    for (int t = 0; t < n; ++t) earlier |= tile[t] == s;
  }
  if (i < n_feat) uniq[i] = s >= 0 && !earlier ? s : -1;
}

__global__ __launch_bounds__(MS_THREADS) void mf_uniq_kernel(MfArgs A) {
  __shared__ int tile[MS_THREADS];
  const MfKf kf = A.kfs[blockIdx.y];
  if (!kf.slots || !A.changed[blockIdx.y] || (int)(blockIdx.x * MS_THREADS) >= kf.n) return;      // (the block's)
  uniq_rows(kf.slots, kf.uniq, kf.n, tile);
}

__global__ __launch_bounds__(MS_THREADS) void mf_restore_kernel(MfArgs A) {
  const int P = A.list_off[1], id = blockIdx.x * MS_THREADS + threadIdx.x;
  if (id >= P + P * A.n_tgt) return;
  if (id < P) A.index[A.list_slot[id]] = MS_EMPTY;
  else if (A.match[id - P] >= 0 && A.match_e[id - P] >= 0) A.index[A.match_e[id - P]] = MS_EMPTY;
}

// A pass, checked and sized on the host.
struct MfPlan {
  SelPlan S;                                     // L: one frame whose keyframes are kfs[src[..]]
  std::vector<CovKf> ckfs;
  std::vector<CovMember> members;
  std::vector<MfTgt> tgts;
  std::vector<MfKf> kfs;
  int bound = 0, f_tgt = 0, n_feat = 0, max_n = 0, goner_bound = 0;
};

// what can be refused: nothing is enqueued and no keyframe touched
int mf_check(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int n_src, const int* src,
             int n_tgt, const int* tgt, unsigned desc_threshold) {
  if (!cam) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  if (int rc = ms_check_store(h, who, mp)) return rc;
  if (n_kfs < 0 || n_kfs > 0xffff || (n_kfs > 0 && !kfs)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (0 <= n_kfs <= 65535: the keyframe is a grid dimension)", who);
  if (n_src < 0 || n_tgt < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (n_src >= 0, n_tgt >= 0)", who);
  if (desc_threshold > 256) return orbx_fail(h, ORBX_ERR_INVALID, "%s: desc_threshold %u is above 256", who, desc_threshold);
  if (int rc = cov_check_queries(h, who, "src", n_src, src, n_kfs, 0)) return rc;
  if (int rc = cov_check_queries(h, who, "tgt", n_tgt, tgt, n_kfs, 0)) return rc;
  if (int rc = ms_check_distinct(h, who, mp, n_kfs, kfs)) return rc;
  std::vector<uint8_t> is_tgt((size_t)n_kfs, 0);
  for (int t = 0; t < n_tgt; ++t) {
    if (is_tgt[(size_t)tgt[t]]) return orbx_fail(h, ORBX_ERR_INVALID, "%s: tgt[%d] = %d is listed twice", who, t, tgt[t]);
    is_tgt[(size_t)tgt[t]] = 1;
  }
  return ORBX_OK;
}

// A target without a table gets one, every entry -1: what the absence of a table means to every reader, and room for associations.
int mf_give_tables(orbx_handle* h, const orbx_map_points* mp, orbx_keyframe* const* kfs, int n_tgt, const int* tgt) {
  ORBX_HIP(h, hipSetDevice(h->device));
  for (int t = 0; t < n_tgt; ++t) {
    orbx_keyframe* kf = kfs[tgt[t]];
    if (kf->slot_store) continue;
    if (kf->n > 0) {
      ORBX_HIP(h, hipMemsetAsync(kf->d_mp_slot, 0xff, 4 * (size_t)kf->n, h->stream));
      ORBX_HIP(h, hipMemsetAsync(kf->d_mp_uniq, 0xff, 4 * (size_t)kf->n, h->stream));
    }
    kf->slot_store = mp;
  }
  return ORBX_OK;
}

// behind mf_check and mf_give_tables
int mf_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int n_src, const int* src, int n_tgt, const int* tgt,
            MfPlan& P) {
  std::vector<const orbx_keyframe*> sk((size_t)n_src);
  for (int i = 0; i < n_src; ++i) sk[(size_t)i] = kfs[src[i]];
  const int off[2] = {0, n_src};
  if (int rc = ms_plan(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, sk.data(), off, nullptr, P.S)) return rc;
  P.bound = P.S.bound_off[1];
  P.ckfs.resize((size_t)n_kfs); P.kfs.resize((size_t)n_kfs); P.tgts.resize((size_t)n_tgt); P.members.resize((size_t)n_tgt);
  long long total = 0;
  for (int k = 0; k < n_kfs; ++k) {
    orbx_keyframe* kf = kfs[k];
    P.ckfs[(size_t)k] = CovKf{kf->slot_store ? kf->d_mp_slot : nullptr, kf->slot_store ? kf->d_mp_uniq : nullptr, kf->n, 0};
    P.kfs[(size_t)k] = MfKf{kf->slot_store ? kf->d_mp_slot : nullptr, kf->slot_store ? kf->d_mp_uniq : nullptr, kf->n, (int)total, -1, 0};
    total += kf->n; P.max_n = std::max(P.max_n, kf->n);
    if (int rc = ms_check_feature_total(h, who, total)) return rc;
  }
  P.n_feat = (int)total;
  long long ft = 0;
  for (int t = 0; t < n_tgt; ++t) {
    const orbx_keyframe* kf = kfs[tgt[t]];
    MfTgt& g = P.tgts[(size_t)t];
    g.kp = kf->d_kp; g.desc = kf->d_desc; g.slots = kf->d_mp_slot; g.n = kf->n; g.feat_off = (int)ft;
    orbx_pose_inverse(kf->pose_wc, g.pose_cw);
    P.kfs[(size_t)tgt[t]].tgt = t;
    P.members[(size_t)t] = CovMember{tgt[t], t};
    ft += kf->n;
  }
  P.f_tgt = (int)ft;
  if ((long long)P.bound * (1 + (long long)n_tgt) >= MS_EMPTY) return orbx_fail(h, ORBX_ERR_INVALID, "%s: too many (point, target) pairs", who);
  P.goner_bound = (int)std::min<long long>((long long)P.bound + ft, 0x7fffffff);
  return ORBX_OK;
}

// The pass on the handle's stream.  Every output is device memory; d_list_slot [bound], d_match [bound][n_tgt], d_goner / d_keeper
// [goner_bound].
int mf_enqueue(orbx_handle* h, const char* who, const orbx_camera* cam, orbx_map_points* mp, const MfPlan& P, double radius_scale, unsigned desc_threshold,
               int* d_counts, int* d_list_slot, int* d_match, int* d_goner, int* d_keeper) {
  const size_t K = P.kfs.size(), T = P.tgts.size(), B = (size_t)P.bound, Nb = B * (1 + T), Gb = (size_t)P.goner_bound;
  const bool run = B > 0 && T > 0;
  if (!d_counts || (B > 0 && !d_list_slot) || (run && (!d_match || !d_goner || !d_keeper))) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  ORBX_HIP(h, hipSetDevice(h->device));
  Carve ws;
  UploadPlan up;
  const size_t o_lo = ws.take(8), o_po = ws.take(24 * B), o_de = ws.take(32 * B);
  const size_t o_me = ws.take(run ? 4 * B * T : 0), o_ed = ws.take(run ? 4 * B * T : 0), o_la = ws.take(run ? 4 * Nb : 0), o_fc = ws.take(run ? 4 * (size_t)P.n_feat : 0),
               o_tg = ws.take(run ? 4 * Gb : 0), o_tk = ws.take(run ? 4 * Gb : 0), o_cl = ws.take(run ? 4 * (size_t)P.f_tgt : 0);
  const size_t o_zero = ws.off;                                             // zeroed before every pass: observer counts, keys, sizes, claim flags, changed, cursor
  const size_t o_no = ws.take(run ? 4 * Nb : 0), o_ke = ws.take(run ? 8 * Nb : 0), o_cs = ws.take(run ? 4 * Nb : 0), o_cc = ws.take(run ? 4 * Nb : 0),
               o_ch = ws.take(run ? 4 * K : 0), o_cu = ws.take(run ? 4 : 0);
  if (int rc = orbx_reserve(h, h->ws_map.fuse_scratch, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.fuse_scratch.p;
  MfArgs A{};
  A.counts = d_counts;
  const dim3 block(MS_THREADS);
  if (B == 0) {                                                             // no candidate: P = 0
    orbx_launch(h, "mf_begin_kernel", false, mf_begin_kernel, dim3(1), block, 0, A, 0);
    ORBX_HIP(h, hipGetLastError());
    return ORBX_OK;
  }
  if (int rc = ms_select_enqueue(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, P.S, nullptr, nullptr, P.bound, (int*)(w + o_lo), d_list_slot, (double*)(w + o_po), w + o_de))
    return rc;
  A.list_off = (const int*)(w + o_lo); A.list_slot = d_list_slot; A.list_pos = (const double*)(w + o_po); A.list_desc = w + o_de;
  A.index = (int*)mp->first.p;                                              // (row 0; the selection has allocated it and left it EMPTY)
  const dim3 list_grid((unsigned)((B + MS_THREADS - 1) / MS_THREADS));
  if (!run) {
    orbx_launch(h, "mf_begin_kernel", true, mf_begin_kernel, dim3(1), block, 0, A, 0);
    ORBX_HIP(h, hipGetLastError());
    return ORBX_OK;
  }
  const size_t need = T * (size_t)mp->capacity;
  if (mp->mark.bytes < need) {                                              // the one fill of the tables: calls leave them 0
    if (int rc = orbx_reserve(h, mp->mark, need)) return rc;
    ORBX_HIP(h, hipMemsetAsync(mp->mark.p, 0, mp->mark.bytes, h->stream));
  }
  const size_t u_ck = up.put(P.ckfs.data(), sizeof(CovKf) * K), u_me = up.put(P.members.data(), sizeof(CovMember) * T), u_tg = up.put(P.tgts.data(), sizeof(MfTgt) * T),
               u_kf = up.put(P.kfs.data(), sizeof(MfKf) * K);
  if (int rc = up.send(h, h->ring_map, h->ws_map.fuse_tables)) return rc;
  uint8_t* const ds = up.device;
  ORBX_HIP(h, hipMemsetAsync(w + o_zero, 0, ws.off - o_zero, h->stream));
  if (P.f_tgt > 0) ORBX_HIP(h, hipMemsetAsync(w + o_cl, MS_EMPTY & 0xff, 4 * (size_t)P.f_tgt, h->stream));
  A.cam = *cam; A.radius_scale = radius_scale; A.thr = desc_threshold;
  A.capacity = mp->capacity; A.n_kfs = (int)K; A.n_tgt = (int)T;
  A.live = mp->d_live; A.mark = (const uint8_t*)mp->mark.p;
  A.tgts = (const MfTgt*)(ds + u_tg); A.kfs = (const MfKf*)(ds + u_kf);
  A.match = d_match; A.match_e = (int*)(w + o_me); A.edge = (int*)(w + o_ed); A.claim = (int*)(w + o_cl);
  A.nobs = (int*)(w + o_no); A.label = (int*)(w + o_la); A.key = (unsigned long long*)(w + o_ke); A.csize = (int*)(w + o_cs); A.cclaim = (int*)(w + o_cc);
  A.feat_cls = (int*)(w + o_fc); A.changed = (int*)(w + o_ch); A.cursor = (int*)(w + o_cu); A.tmp_goner = (int*)(w + o_tg); A.tmp_keeper = (int*)(w + o_tk);
  A.goner = d_goner; A.keeper = d_keeper;
  CovArgs C{};
  C.capacity = mp->capacity; C.n_kfs = (int)K; C.n_q = (int)T; C.live = mp->d_live; C.kfs = (const CovKf*)(ds + u_ck); C.members = (const CovMember*)(ds + u_me);
  C.mark = (uint8_t*)mp->mark.p;
  ObsArgs O{};
  O.capacity = mp->capacity; O.n_kfs = (int)K; O.live = mp->d_live; O.kfs = C.kfs; O.index = A.index; O.count = A.nobs;
  int max_tn = 0;
  for (const MfTgt& g : P.tgts) max_tn = std::max(max_tn, g.n);
  const int n_chunk = std::max(1, (P.max_n + MS_CHUNK - 1) / MS_CHUNK), n_fine = std::max(1, (P.max_n + MS_THREADS - 1) / MS_THREADS);
  const dim3 mark_grid(std::max(1, (max_tn + MS_CHUNK - 1) / MS_CHUNK), (unsigned)T), pair_grid((unsigned)((B * T + MS_THREADS - 1) / MS_THREADS)),
      node_grid((unsigned)((Nb + MS_THREADS - 1) / MS_THREADS)), kf_grid(n_chunk, (unsigned)K), feat_grid(n_fine, (unsigned)K);
  orbx_launch(h, "mf_begin_kernel", true, mf_begin_kernel, list_grid, block, 0, A, 1);
  orbx_launch(h, "cov_mark_kernel", true, cov_mark_kernel, mark_grid, block, 0, C, 1);
  orbx_launch(h, "mf_search_kernel", true, mf_search_kernel, dim3((unsigned)((B + FUSE_THREADS - 1) / FUSE_THREADS), (unsigned)T), dim3(FUSE_THREADS), 0, A);
  orbx_launch(h, "cov_mark_kernel", true, cov_mark_kernel, mark_grid, block, 0, C, 0);
  orbx_launch(h, "mf_name_kernel", true, mf_name_kernel, pair_grid, block, 0, A);
  if (P.max_n > 0) orbx_launch(h, "obs_count_kernel", true, obs_count_kernel, kf_grid, block, 0, O);
  orbx_launch(h, "mf_class_kernel", true, mf_class_kernel, dim3(1), dim3(MF_CLASS_THREADS), 0, A);
  orbx_launch(h, "mf_key_kernel", true, mf_key_kernel, node_grid, block, 0, A);
  orbx_launch(h, "mf_goner_kernel", true, mf_goner_kernel, node_grid, block, 0, A);
  orbx_launch(h, "mf_goner_rank_kernel", true, mf_goner_rank_kernel, dim3((unsigned)std::max<size_t>(1, (Gb + MS_THREADS - 1) / MS_THREADS)), block, 0, A);
  if (P.max_n > 0) {
    orbx_launch(h, "mf_feat_kernel", true, mf_feat_kernel, feat_grid, block, 0, A);
    orbx_launch(h, "mf_rewrite_kernel", true, mf_rewrite_kernel, feat_grid, block, 0, A);
    orbx_launch(h, "mf_uniq_kernel", true, mf_uniq_kernel, feat_grid, block, 0, A);
  }
  orbx_launch(h, "mf_restore_kernel", true, mf_restore_kernel, node_grid, block, 0, A);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// ---- creation and removal (include/orbx.h, "create and cull map points on the resident map"; local_mapper.rs:208-268, :421-469,
// triangulation.rs:286-290, map.rs:609-631) ----
// New points are written into the tables where they lie; a keyframe's flags are derived from its table and the live bytes.
//   mc_table_kernel    a table from a device array: a value outside [-1, capacity) becomes -1; mc_uniq_one_kernel: its d_mp_uniq
//   mc_flag_kernel     (chunk, keyframe) flag = the table names a live point — what d_mp_flag is to the host-id calls
//   mc_stereo_kernel   one workgroup over the current keyframe in chunks of MS_CHUNK: the candidates (stereo point, no flag) ranked in
//                      feature order (BlockScan); candidate r takes free_slots[r]: table, flag, list row, position, descriptor
//   (the neighbour loop of keyframe.hip, reading these flags, leaves its ordered lists in the workspace)
//   mc_pair_kernel     pair e takes free_slots[S' + e]: list row, the neighbour's table, atomicMax(last[idx1], e) — an integer maximum,
//                      whatever the order; counts and stats
//   mc_last_kernel     the pair that holds last[idx1] writes the current keyframe's entry: the reference's sequential overwriting
//   mc_uniq_kernel     (block, keyframe) of a changed keyframe: d_mp_uniq again
// Removal marks the listed slots in the store's mark bytes (row 0, 0 between calls), clears every entry of the call's tables that
// names a marked slot (mr_clear_kernel: block_sum, one integer atomicAdd per block on the counter), and takes the marks back.

struct McKf {                                    // one keyframe of a creation or removal call
  int* slots; int* uniq;                         // NULL: no table (removal; creation gives every keyframe one)
  uint8_t* flag;                                 // creation: [n] scratch
  int n, pad_;
};
struct McArgs {
  int capacity, n_free, n1, cap_pairs, T;
  const uint8_t* live; const McKf* kfs;          // kfs [1 + T]: the current keyframe, then the neighbours
  const int* free_slots;                         // [n_free]
  const int* orig; const int* searched;          // searched neighbour -> its place in nbs[]; [T] the inverse, -1: not searched
  const uint8_t* has1; const double* pts1; const uint8_t* desc1;
  double pose1[7];
  const int* head; const int* p_nb; const int* p_i1; const int* p_i2; const double* p_pts;      // the neighbour loop's lists (head NULL: it did not run)
  int* last; int* changed; int* n_stereo;        // [n1], -1: none; [1 + T]; {S, S'}
  int* counts; int* new_slot; int* new_nb; int* new_i1; int* new_i2; double* new_pts; uint8_t* new_desc; int* stats;
};

__device__ __forceinline__ void mc_copy_desc(uint8_t* out, const uint8_t* in) {        // (both 16-byte aligned)
  const uint4* d = (const uint4*)in;
  uint4* q = (uint4*)out;
  q[0] = d[0]; q[1] = d[1];
}

__global__ __launch_bounds__(MS_THREADS) void mc_table_kernel(const int* in, int n, int capacity, int* slots) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= n) return;
  const int s = in[i];
  slots[i] = s >= 0 && s < capacity ? s : -1;
}

__global__ __launch_bounds__(MS_THREADS) void mc_uniq_one_kernel(const int* slots, int* uniq, int n) {
  __shared__ int tile[MS_THREADS];
  uniq_rows(slots, uniq, n, tile);
}

__global__ __launch_bounds__(MS_THREADS) void mc_flag_kernel(McArgs A) {
  const McKf kf = A.kfs[blockIdx.y];
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) {
    const int i = blockIdx.x * MS_CHUNK + j * MS_THREADS + threadIdx.x;
    if (i >= kf.n) continue;
    const int s = kf.slots[i];
    kf.flag[i] = s >= 0 && s < A.capacity && A.live[s] ? 1 : 0;
  }
}

__global__ __launch_bounds__(MS_THREADS) void mc_stereo_kernel(McArgs A) {
  __shared__ int wave_tot[MS_THREADS / 64];
  __shared__ double R[9];
  const int tid = threadIdx.x;
  const McKf kf = A.kfs[0];
  if (tid == 0) quat_to_R(A.pose1, R);
  BlockScan<MS_THREADS> scan(wave_tot);                                     // (its first barrier also covers R)
  for (int c0 = 0; c0 < A.n1; c0 += MS_CHUNK) {                             // (the bounds are the block's: every thread reaches every round)
    const int i0 = c0 + tid * MS_PER;
    bool cand[MS_PER];
    int n = 0;
#pragma unroll
    for (int k = 0; k < MS_PER; ++k) { cand[k] = i0 + k < A.n1 && A.has1[i0 + k] && !kf.flag[i0 + k]; n += cand[k]; }
    int r = scan.round(n);
#pragma unroll
    for (int k = 0; k < MS_PER; ++k) {
      if (!cand[k]) continue;
      const int i = i0 + k, at = r++;
      if (at >= A.n_free) continue;                                         // dropped: no slot, no table write, the flag stays 0
      const int slot = A.free_slots[at];
      kf.slots[i] = slot; kf.flag[i] = 1;
      A.new_slot[at] = slot; A.new_nb[at] = -1; A.new_i1[at] = i; A.new_i2[at] = -1;
      const double* p = A.pts1 + 3 * (size_t)i;                             // pose_wc * points_cam[i]: rotate, then translate
      A.new_pts[3 * (size_t)at] = R[0] * p[0] + R[1] * p[1] + R[2] * p[2] + A.pose1[4];
      A.new_pts[3 * (size_t)at + 1] = R[3] * p[0] + R[4] * p[1] + R[5] * p[2] + A.pose1[5];
      A.new_pts[3 * (size_t)at + 2] = R[6] * p[0] + R[7] * p[1] + R[8] * p[2] + A.pose1[6];
      mc_copy_desc(A.new_desc + 32 * (size_t)at, A.desc1 + 32 * (size_t)i);
    }
  }
  if (tid == 0) {
    A.n_stereo[0] = scan.total; A.n_stereo[1] = min(scan.total, A.n_free);
    if (scan.total > 0 && A.n_free > 0) A.changed[0] = 1;
  }
}

__global__ __launch_bounds__(MS_THREADS) void mc_pair_kernel(McArgs A) {
  const int e = blockIdx.x * MS_THREADS + threadIdx.x;
  const int S = A.n_stereo[0], Sp = A.n_stereo[1], N = A.head ? A.head[0] : 0;
  if (e == 0) {
    const int created = min(S + N, A.n_free);
    A.counts[0] = S; A.counts[1] = N; A.counts[2] = created; A.counts[3] = S + N - created;
  }
  if (e < 4 * A.T) {                                                        // stats [T][4]: searched, matches_found, triangulated, validated
    const int k = A.head ? A.searched[e >> 2] : -1, j = e & 3;
    A.stats[e] = k < 0 ? 0 : j == 0 ? 1 : A.head[1 + 4 * k + j];
  }
  const int g = Sp + e;
  if (e >= N || e >= A.cap_pairs || g >= A.n_free) return;
  const int t = A.orig[A.p_nb[e]], i1 = A.p_i1[e], i2 = A.p_i2[e], slot = A.free_slots[g];
  A.new_slot[g] = slot; A.new_nb[g] = t; A.new_i1[g] = i1; A.new_i2[g] = i2;
  A.new_pts[3 * (size_t)g] = A.p_pts[3 * (size_t)e]; A.new_pts[3 * (size_t)g + 1] = A.p_pts[3 * (size_t)e + 1]; A.new_pts[3 * (size_t)g + 2] = A.p_pts[3 * (size_t)e + 2];
  mc_copy_desc(A.new_desc + 32 * (size_t)g, A.desc1 + 32 * (size_t)i1);     // triangulation.rs:280
  A.kfs[1 + t].slots[i2] = slot;                                            // (a search gives a feature of the neighbour to one pair)
  A.changed[1 + t] = 1;
  atomicMax(&A.last[i1], e);
}

__global__ __launch_bounds__(MS_THREADS) void mc_last_kernel(McArgs A) {
  const int e = blockIdx.x * MS_THREADS + threadIdx.x;
  const int g = A.n_stereo[1] + e;
  if (e >= A.head[0] || e >= A.cap_pairs || g >= A.n_free) return;
  const int i1 = A.p_i1[e];
  if (A.last[i1] != e) return;                                              // triangulation.rs:289: each associate overwrites the one before
  A.kfs[0].slots[i1] = A.free_slots[g];
  A.changed[0] = 1;
}

__global__ __launch_bounds__(MS_THREADS) void mc_uniq_kernel(McArgs A) {
  __shared__ int tile[MS_THREADS];
  const McKf kf = A.kfs[blockIdx.y];
  if (!A.changed[blockIdx.y] || (int)(blockIdx.x * MS_THREADS) >= kf.n) return;                  // (the block's)
  uniq_rows(kf.slots, kf.uniq, kf.n, tile);
}

__global__ __launch_bounds__(MS_THREADS) void mr_mark_kernel(const int* slots, int n, uint8_t* mark, int value) {
  const int i = blockIdx.x * MS_THREADS + threadIdx.x;
  if (i < n) mark[slots[i]] = (uint8_t)value;                               // (repeats store the same byte)
}

__global__ __launch_bounds__(MS_THREADS) void mr_clear_kernel(const McKf* kfs, int capacity, const uint8_t* mark, int* n_cleared) {
  __shared__ int wave_tot[MS_THREADS / 64];
  const McKf kf = kfs[blockIdx.y];
  if (!kf.slots || (int)(blockIdx.x * MS_CHUNK) >= kf.n) return;            // (the block's)
  int c = 0;
#pragma unroll
  for (int j = 0; j < MS_PER; ++j) {
    const int i = blockIdx.x * MS_CHUNK + j * MS_THREADS + threadIdx.x;
    if (i >= kf.n) continue;
    const int s = kf.slots[i];
    if (s < 0 || s >= capacity || !mark[s]) continue;
    kf.slots[i] = -1; kf.uniq[i] = -1;                                      // (uniq[i] is s or -1: every occurrence goes, so clearing in place is exact)
    ++c;
  }
  c = block_sum<MS_THREADS>(c, wave_tot);
  if (threadIdx.x == 0 && c) atomicAdd(n_cleared, c);
}

// What orbx_map_create_points[_device] refuses, before anything is enqueued or any keyframe touched.
int mc_check(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_triangulation_config* cfg, orbx_map_points* mp, const orbx_keyframe* cur,
             const orbx_keyframe* const* nbs, int T, int phases, const int* free_slots, int n_free) {
  if (!cam || !cfg || T < 0 || T > 256 || cfg->max_descriptor_dist > 256 || (T > 0 && !nbs))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (0 <= T <= 256; max_descriptor_dist <= 256)", who);
  if (int rc = ms_check_store(h, who, mp)) return rc;
  if (phases < 1 || phases > (ORBX_MAP_CREATE_STEREO | ORBX_MAP_CREATE_NEIGHBOURS)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: phases = %d is outside 1..3", who, phases);
  std::vector<const orbx_keyframe*> all((size_t)T + 1);
  all[0] = cur;
  for (int t = 0; t < T; ++t) all[(size_t)t + 1] = nbs[t];
  if (int rc = ms_check_distinct(h, who, mp, T + 1, all.data())) return rc;  // (the current keyframe among its neighbours: listed twice)
  if (int rc = ms_check_slots(mp, who, free_slots, n_free, true)) return rc;
  for (int i = 0; i < n_free; ++i)
    if (mp->live[(size_t)free_slots[i]]) return orbx_fail(h, ORBX_ERR_INVALID, "%s: free_slots[%d] = %d is live", who, i, free_slots[i]);
  return ORBX_OK;
}

// Both phases on the handle's stream, behind mc_check.  Every output is device memory; the list rows hold n_free entries.
int mc_enqueue(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial, orbx_map_points* mp, orbx_keyframe* cur,
               orbx_keyframe* const* nbs, int T, int phases, const int* free_slots, int n_free, int* d_counts, int* d_new_slot, int* d_new_nb, int* d_new_i1,
               int* d_new_i2, double* d_new_pts, uint8_t* d_new_desc, int* d_stats) {
  ORBX_HIP(h, hipSetDevice(h->device));
  std::vector<orbx_keyframe*> all((size_t)T + 1);
  std::vector<int> idx((size_t)T + 1);
  all[0] = cur;
  for (int t = 0; t < T; ++t) all[(size_t)t + 1] = nbs[t];
  std::iota(idx.begin(), idx.end(), 0);
  if (int rc = mf_give_tables(h, mp, all.data(), T + 1, idx.data())) return rc;
  TriNbPlan P;
  if (phases & ORBX_MAP_CREATE_NEIGHBOURS) tri_nb_plan(cam, cur, nbs, T, P);
  const size_t K = (size_t)T + 1, Ts = P.orig.size(), n1 = (size_t)cur->n, NF = (size_t)n_free;
  const size_t capd = std::min(NF, Ts * n1);                                // pair e takes free_slots[S' + e]: no pair beyond n_free is listed
  int max_n = 0;
  size_t n_feat = 0;
  for (const orbx_keyframe* kf : all) { max_n = std::max(max_n, kf->n); n_feat += (size_t)kf->n; }
  UploadPlan up;
  Carve ws;
  // (the keyframe table, `searched` and the neighbour loop's tables are made in place: they hold addresses inside the two workspaces)
  const size_t u_kf = up.put(nullptr, sizeof(McKf) * K), u_fr = up.put(free_slots, 4 * NF), u_or = up.put(P.orig.data(), 4 * Ts), u_se = up.put(nullptr, 4 * (size_t)T),
               u_tri = up.put(nullptr, P.up_bytes);
  const size_t o_fl = ws.take(n_feat), o_la = ws.take(4 * n1), o_zero = ws.off, o_ch = ws.take(4 * K), o_ns = ws.take(8), o_zend = ws.off, o_tri = ws.take(P.ws_bytes),
               o_he = ws.take(4 * (1 + 4 * Ts)), o_nb = ws.take(4 * capd), o_i1 = ws.take(4 * capd), o_i2 = ws.take(4 * capd), o_pt = ws.take(24 * capd);
  if (int rc = up.begin(h, h->ring_map, h->ws_map.create_tables)) return rc;
  uint8_t *const hs = up.host, *const ds = up.device;
  if (int rc = orbx_reserve(h, h->ws_map.create_scratch, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.create_scratch.p;
  McKf* kt = (McKf*)(hs + u_kf);
  std::vector<const uint8_t*> mp2((size_t)T);
  size_t f = 0;
  for (size_t k = 0; k < K; ++k) {
    kt[k] = McKf{all[k]->d_mp_slot, all[k]->d_mp_uniq, w + o_fl + f, all[k]->n, 0};
    if (k > 0) mp2[k - 1] = kt[k].flag;
    f += (size_t)all[k]->n;
  }
  int* searched = (int*)(hs + u_se);
  for (int t = 0; t < T; ++t) searched[t] = -1;
  for (size_t k = 0; k < Ts; ++k) searched[P.orig[k]] = (int)k;
  if (Ts) tri_nb_fill(P, cam, cfg, cur, nbs, kt[0].flag, mp2.data(), hs + u_tri, ds + u_tri, w + o_tri);
  if (int rc = up.commit(h, h->ring_map, h->ws_map.create_tables)) return rc;
  ORBX_HIP(h, hipMemsetAsync(w + o_zero, 0, o_zend - o_zero, h->stream));
  if (n1) ORBX_HIP(h, hipMemsetAsync(w + o_la, 0xff, 4 * n1, h->stream));
  McArgs A{};
  A.capacity = mp->capacity; A.n_free = n_free; A.n1 = cur->n; A.cap_pairs = (int)capd; A.T = T;
  A.live = mp->d_live; A.kfs = (const McKf*)(ds + u_kf); A.free_slots = (const int*)(ds + u_fr); A.orig = (const int*)(ds + u_or);
  A.searched = (const int*)(ds + u_se);
  A.has1 = cur->d_has_point; A.pts1 = cur->d_points; A.desc1 = cur->d_desc;
  std::memcpy(A.pose1, cur->pose_wc, sizeof(A.pose1));
  A.p_nb = (const int*)(w + o_nb); A.p_i1 = (const int*)(w + o_i1); A.p_i2 = (const int*)(w + o_i2); A.p_pts = (const double*)(w + o_pt);
  A.last = (int*)(w + o_la); A.changed = (int*)(w + o_ch); A.n_stereo = (int*)(w + o_ns);
  A.counts = d_counts; A.new_slot = d_new_slot; A.new_nb = d_new_nb; A.new_i1 = d_new_i1; A.new_i2 = d_new_i2; A.new_pts = d_new_pts; A.new_desc = d_new_desc;
  A.stats = d_stats;
  const dim3 block(MS_THREADS);
  if (max_n > 0) orbx_launch(h, "mc_flag_kernel", false, mc_flag_kernel, dim3((max_n + MS_CHUNK - 1) / MS_CHUNK, (unsigned)K), block, 0, A);
  if ((phases & ORBX_MAP_CREATE_STEREO) && n1 > 0) orbx_launch(h, "mc_stereo_kernel", true, mc_stereo_kernel, dim3(1), block, 0, A);
  ORBX_HIP(h, hipGetLastError());
  if (Ts) {
    if (int rc = tri_nb_launch(h, P, cam, cfg, is_inertial, cur, ds + u_tri, w + o_tri, (int)capd, (int*)(w + o_he), (int*)(w + o_nb), (int*)(w + o_i1), (int*)(w + o_i2),
                               (double*)(w + o_pt)))
      return rc;
    A.head = (const int*)(w + o_he);
  }
  const dim3 pair_grid((unsigned)((std::max<size_t>({capd, 4 * (size_t)T, (size_t)1}) + MS_THREADS - 1) / MS_THREADS));
  orbx_launch(h, "mc_pair_kernel", max_n > 0, mc_pair_kernel, pair_grid, block, 0, A);
  if (capd > 0) orbx_launch(h, "mc_last_kernel", true, mc_last_kernel, pair_grid, block, 0, A);
  if (max_n > 0 && n_free > 0) orbx_launch(h, "mc_uniq_kernel", true, mc_uniq_kernel, dim3((max_n + MS_THREADS - 1) / MS_THREADS, (unsigned)K), block, 0, A);
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// orbx_map_remove_points behind its checks: marks, the tables of P's keyframes, marks back, the erase.  *d_cleared: where the
// number of cleared entries lies.
int mr_enqueue(orbx_handle* h, orbx_map_points* mp, const CovPlan& P, int n, const int* slots, const int** d_cleared) {
  ORBX_HIP(h, hipSetDevice(h->device));
  const size_t K = P.kfs.size(), N = (size_t)n;
  if (mp->mark.bytes < (size_t)mp->capacity) {                              // the one fill of the tables: calls leave them 0
    if (int rc = orbx_reserve(h, mp->mark, (size_t)mp->capacity)) return rc;
    ORBX_HIP(h, hipMemsetAsync(mp->mark.p, 0, mp->mark.bytes, h->stream));
  }
  UploadPlan up;
  const size_t u_kf = up.put(nullptr, sizeof(McKf) * K), u_sl = up.put(slots, 4 * N), u_cn = up.put(nullptr, 4);
  if (int rc = up.begin(h, h->ring_map, h->ws_map.remove_tables)) return rc;
  uint8_t *const hs = up.host, *const ds = up.device;
  McKf* kt = (McKf*)(hs + u_kf);
  for (size_t k = 0; k < K; ++k) kt[k] = McKf{const_cast<int*>(P.kfs[k].slots), const_cast<int*>(P.kfs[k].uniq), nullptr, P.kfs[k].n, 0};
  std::memset(hs + u_cn, 0, 4);
  if (int rc = up.commit(h, h->ring_map, h->ws_map.remove_tables)) return rc;
  const int* d_slots = (const int*)(ds + u_sl);
  uint8_t* mark = (uint8_t*)mp->mark.p;
  const dim3 block(MS_THREADS), list_grid((unsigned)((N + MS_THREADS - 1) / MS_THREADS));
  *d_cleared = (const int*)(ds + u_cn);
  if (K > 0 && P.max_n > 0) {
    orbx_launch(h, "mr_mark_kernel", false, mr_mark_kernel, list_grid, block, 0, d_slots, n, mark, 1);
    orbx_launch(h, "mr_clear_kernel", true, mr_clear_kernel, dim3((P.max_n + MS_CHUNK - 1) / MS_CHUNK, (unsigned)K), block, 0, (const McKf*)(ds + u_kf), mp->capacity,
                (const uint8_t*)mark, (int*)(ds + u_cn));
    orbx_launch(h, "mr_mark_kernel", true, mr_mark_kernel, list_grid, block, 0, d_slots, n, mark, 0);
  }
  return ms_erase_launch(h, mp, d_slots, slots, n);
}

// the keyframes of a removal or culling call: as the observation calls check theirs, and none twice (their tables are rewritten)
int mr_plan(orbx_handle* h, const char* who, const orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, ObsPlan& P) {
  if (int rc = obs_plan(h, who, mp, n_kfs, kfs, P)) return rc;
  return ms_check_no_repeat(h, who, n_kfs, kfs);
}

}  // namespace

extern "C" {

int orbx_map_points_create(orbx_handle* h, int capacity, orbx_map_points** out) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_map_points_create", [&]() -> int {
    if (!out || capacity < 1 || capacity >= MS_EMPTY / 64) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_map_points_create: bad argument (1 <= capacity < %d)", MS_EMPTY / 64);
    *out = nullptr;
    ORBX_HIP(h, hipSetDevice(h->device));
    std::unique_ptr<orbx_map_points> mp(new orbx_map_points());             // (freed on every way out that does not hand it over)
    mp->h = h; mp->capacity = capacity;
    mp->live.assign((size_t)capacity, 0); mp->stamp.assign((size_t)capacity, 0u);
    Carve blk;
    const size_t o_po = blk.take(24 * (size_t)capacity), o_de = blk.take(32 * (size_t)capacity), o_li = blk.take((size_t)capacity);
    if (hipMalloc((void**)&mp->block, blk.off) != hipSuccess) return orbx_fail(h, ORBX_ERR_HIP, "orbx_map_points_create: out of device memory");
    mp->d_pos = (double*)(mp->block + o_po); mp->d_desc = mp->block + o_de; mp->d_live = mp->block + o_li;
    if (hipMemsetAsync(mp->block, 0, blk.off, h->stream) != hipSuccess) { hipFree(mp->block); return orbx_fail(h, ORBX_ERR_HIP, "orbx_map_points_create: memset failed"); }
    *out = mp.release();
    return ORBX_OK;
  });
}

void orbx_map_points_destroy(orbx_map_points* mp) {
  if (!mp) return;
  hipSetDevice(mp->h->device);
  hipStreamSynchronize(mp->h->stream);
  if (mp->block) hipFree(mp->block);
  if (mp->first.p) hipFree(mp->first.p);
  if (mp->mark.p) hipFree(mp->mark.p);
  delete mp;
}

int orbx_map_points_info(const orbx_map_points* mp, int* capacity, int* n_live) {
  if (!mp) return ORBX_ERR_INVALID;
  if (capacity) *capacity = mp->capacity;
  if (n_live) *n_live = mp->n_live;
  return ORBX_OK;
}

int orbx_map_points_set(orbx_map_points* mp, const int* slots, int n, const double* positions, const uint8_t* desc) {
  if (!mp) return ORBX_ERR_INVALID;
  return orbx_guard(mp->h, "orbx_map_points_set", [&] { return ms_set(mp, "orbx_map_points_set", slots, n, positions, desc, true); });
}

int orbx_map_points_set_device(orbx_map_points* mp, const int* slots, int n, const double* d_positions, const uint8_t* d_desc) {
  if (!mp) return ORBX_ERR_INVALID;
  return orbx_guard(mp->h, "orbx_map_points_set_device", [&]() -> int {
    if (((uintptr_t)d_desc & 3) || ((uintptr_t)d_positions & 7)) return orbx_fail(mp->h, ORBX_ERR_INVALID, "orbx_map_points_set_device: d_desc is 4-byte, d_positions 8-byte aligned");
    return ms_set(mp, "orbx_map_points_set_device", slots, n, d_positions, d_desc, false);
  });
}

int orbx_map_points_erase(orbx_map_points* mp, const int* slots, int n) {
  static const char* who = "orbx_map_points_erase";
  if (!mp) return ORBX_ERR_INVALID;
  orbx_handle* h = mp->h;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = ms_check_slots(mp, who, slots, n, false)) return rc;
    if (n == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    uint8_t *hs, *ds;                                                     // (one piece, copied to its last byte and no further: no plan)
    if (int rc = orbx_ring_begin(h, h->ring_map, h->ws_map.call_tables, 4 * (size_t)n, &hs, &ds)) return rc;
    std::memcpy(hs, slots, 4 * (size_t)n);
    if (int rc = orbx_ring_commit(h, h->ring_map, h->ws_map.call_tables, 4 * (size_t)n)) return rc;
    return ms_erase_launch(h, mp, (const int*)ds, slots, n);
  });
}

int orbx_map_points_download(orbx_map_points* mp, const int* slots, int n, double* positions, uint8_t* desc, uint8_t* live) {
  static const char* who = "orbx_map_points_download";
  if (!mp) return ORBX_ERR_INVALID;
  orbx_handle* h = mp->h;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = ms_check_slots(mp, who, slots, n, false)) return rc;
    if (n == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    // tests and debugging: the whole store comes down, the rows asked for are picked on the host
    const size_t cap = (size_t)mp->capacity, bytes = (size_t)((mp->d_live + cap) - mp->block);
    if (int rc = orbx_reserve_pinned(h, h->pin_map, bytes)) return rc;
    uint8_t* hp = (uint8_t*)h->pin_map.p;
    ORBX_HIP(h, hipMemcpyAsync(hp, mp->block, bytes, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    const double* hpos = (const double*)(hp + ((uint8_t*)mp->d_pos - mp->block));
    const uint8_t* hdesc = hp + (mp->d_desc - mp->block);
    const uint8_t* hlive = hp + (mp->d_live - mp->block);
    for (int i = 0; i < n; ++i) {
      const size_t s = (size_t)slots[i];
      if (positions) std::memcpy(positions + 3 * (size_t)i, hpos + 3 * s, 24);
      if (desc) std::memcpy(desc + 32 * (size_t)i, hdesc + 32 * s, 32);
      if (live) live[i] = hlive[s];
    }
    return ORBX_OK;
  });
}

int orbx_keyframe_set_map_point_slots(orbx_keyframe* kf, const orbx_map_points* mp, const int* slots) {
  static const char* who = "orbx_keyframe_set_map_point_slots";
  if (!kf) return ORBX_ERR_INVALID;
  orbx_handle* h = kf->h;
  return orbx_guard(h, who, [&]() -> int {
    if (!slots) { kf->slot_store = nullptr; return ORBX_OK; }
    if (int rc = ms_check_store(h, who, mp)) return rc;
    for (int i = 0; i < kf->n; ++i)
      if (slots[i] < -1 || slots[i] >= mp->capacity) return orbx_fail(h, ORBX_ERR_INVALID, "%s: slot %d (feature %d) is outside [-1, %d)", who, slots[i], i, mp->capacity);
    ORBX_HIP(h, hipSetDevice(h->device));
    if (kf->n > 0) {
      // beside the table, the same with every repeat of a slot set to -1 (the first feature that names it keeps it): what
      // covisibility counts, each observed slot once
      const size_t n = (size_t)kf->n;
      std::vector<int> uniq(slots, slots + n), order(n);
      std::iota(order.begin(), order.end(), 0);
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return slots[a] < slots[b]; });
      for (size_t i = 1; i < n; ++i)
        if (slots[order[i]] == slots[order[i - 1]]) uniq[(size_t)order[i]] = -1;
      ORBX_HIP(h, hipMemcpyAsync(kf->d_mp_slot, slots, 4 * n, hipMemcpyHostToDevice, h->stream));
      ORBX_HIP(h, hipMemcpyAsync(kf->d_mp_uniq, uniq.data(), 4 * n, hipMemcpyHostToDevice, h->stream));
      ORBX_HIP(h, hipStreamSynchronize(h->stream));                       // the caller's array is free when the call returns
    }
    kf->slot_store = mp;
    return ORBX_OK;
  });
}

int orbx_map_select_points_device(orbx_handle* h, orbx_map_points* mp, int source, int n_frames, const orbx_keyframe* const* kfs, const int* kf_offsets,
                                  const int* d_src_slots, const int* src_offsets, int list_cap, int* d_list_offsets, int* d_list_slot,
                                  double* d_positions, uint8_t* d_mp_desc) {
  static const char* who = "orbx_map_select_points_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    SelPlan P;
    if (int rc = ms_plan(h, who, mp, source, n_frames, kfs, kf_offsets, src_offsets, P)) return rc;
    return ms_select_enqueue(h, who, mp, source, n_frames, P, d_src_slots, src_offsets, list_cap, d_list_offsets, d_list_slot, d_positions, d_mp_desc);
  });
}

int orbx_map_track_frames_device(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                                 orbx_map_points* mp, int source, int n_frames, const orbx_keyframe* const* kfs, const int* kf_offsets,
                                 const int* d_src_slots, const int* src_offsets, const orbx_keypoint* d_kp, const uint8_t* d_desc,
                                 const int* d_feat_start, const int* d_feat_count, int feat_count_stride, int max_feat,
                                 const double* d_search_poses_wc, const double* d_priors_wc, int list_cap, int* d_list_offsets, int* d_list_slot,
                                 double* d_positions, uint8_t* d_mp_desc, int* d_offsets, double* d_pts3d, float* d_pts2d, int* d_mp_idx,
                                 int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                                 orbx_pnp_result* d_pnp_results, int* d_matched, int* d_matched_slot, orbx_track_result* d_results) {
  static const char* who = "orbx_map_track_frames_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    SelPlan P;
    if (n_frames > 0)
      if (int rc = ms_plan(h, who, mp, source, n_frames, kfs, kf_offsets, src_offsets, P)) return rc;
    const MapTrackDev D{d_kp, d_desc, d_feat_start, d_feat_count, feat_count_stride, max_feat, d_search_poses_wc, d_priors_wc, d_list_offsets, d_list_slot,
                        d_positions, d_mp_desc, d_offsets, d_pts3d, d_pts2d, d_mp_idx, d_feat_idx, d_poses_wc_out, d_inlier_out, d_err_out, d_pnp_results,
                        d_matched, d_matched_slot, d_results};
    return ms_track_device(h, who, cam, cfg, pnp_cfg, n_frames, n_frames > 0 ? P.bound_off.data() : nullptr, D, [&] {
      return ms_select_enqueue(h, who, mp, source, n_frames, P, d_src_slots, src_offsets, list_cap, d_list_offsets, d_list_slot, d_positions, d_mp_desc);
    });
  });
}

int orbx_map_track_frames(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg, orbx_map_points* mp,
                          int source, int n_frames, const orbx_keyframe* const* kfs, const int* kf_offsets, const int* src_slots,
                          const int* src_offsets, const orbx_keypoint* kp, const uint8_t* desc, const int* feat_offsets,
                          const double* search_poses_wc, const double* priors_wc, int list_cap, int* list_offsets, int* list_slot, int* offsets,
                          double* pts3d, float* pts2d, int* mp_idx, int* feat_idx, double* poses_wc_out, uint8_t* inlier_out, double* err_out,
                          orbx_pnp_result* pnp_results, int* matched, int* matched_slot, orbx_track_result* results) {
  static const char* who = "orbx_map_track_frames";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    SelPlan P;
    if (n_frames > 0)
      if (int rc = ms_plan(h, who, mp, source, n_frames, kfs, kf_offsets, src_offsets, P)) return rc;
    const size_t S = n_frames > 0 && source == ORBX_MAP_SOURCE_SLOTS ? (size_t)src_offsets[n_frames] : 0;
    const MapTrackHost H{src_slots, S, kp, desc, feat_offsets, search_poses_wc, priors_wc, list_cap, nullptr, 0, list_offsets, list_slot, offsets, pts3d, pts2d,
                         mp_idx, feat_idx, poses_wc_out, inlier_out, err_out, pnp_results, matched, matched_slot, results};
    return ms_track_host(h, who, cam, cfg, pnp_cfg, n_frames, n_frames > 0 ? P.bound_off.data() : nullptr, H,
                         [&](const int* d_src, int*, int* d_lo, int* d_ls, double* d_gp, uint8_t* d_gd) {
                           return ms_select_enqueue(h, who, mp, source, n_frames, P, d_src, src_offsets, P.bound_off[(size_t)n_frames], d_lo, d_ls, d_gp, d_gd);
                         });
  });
}

int orbx_map_covisibility_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_queries, const int* query,
                                 int n_best, int* d_weights, int* d_best, int* d_n_best) {
  static const char* who = "orbx_map_covisibility_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    CovPlan P;
    if (int rc = cov_plan(h, who, mp, n_kfs, kfs, n_best, P)) return rc;
    if (n_queries < 0 || n_queries > 0xffff) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (0 <= n_queries <= 65535)", who);
    if (int rc = cov_check_queries(h, who, "query", n_queries, query, n_kfs, 0)) return rc;
    if (n_queries == 0 || n_kfs == 0 || (!d_weights && !d_n_best && (!d_best || n_best == 0))) return ORBX_OK;
    return cov_enqueue(h, mp, P, n_queries, query, n_best, d_weights, n_best > 0 ? d_best : nullptr, d_n_best, nullptr);
  });
}

int orbx_map_covisibility(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_queries, const int* query, int n_best,
                          int* weights, int* best, int* n_best_out) {
  static const char* who = "orbx_map_covisibility";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    CovPlan P;
    if (int rc = cov_plan(h, who, mp, n_kfs, kfs, n_best, P)) return rc;
    if (n_queries < 0 || n_queries > 0xffff) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (0 <= n_queries <= 65535)", who);
    if (int rc = cov_check_queries(h, who, "query", n_queries, query, n_kfs, 0)) return rc;
    if (n_queries == 0 || n_kfs == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    const size_t Q = (size_t)n_queries, K = (size_t)n_kfs, nb = (size_t)n_best;
    OutputPlan out;
    const auto p_we = out.add(weights, weights ? Q * K : 0), p_be = out.add(best, best ? Q * nb : 0), p_nb = out.add(n_best_out, n_best_out ? Q : 0);
    if (out.down == 0) return ORBX_OK;
    if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs)) return rc;
    if (int rc = cov_enqueue(h, mp, P, n_queries, query, n_best, weights ? out.dev(p_we) : nullptr, best && nb ? out.dev(p_be) : nullptr,
                             n_best_out ? out.dev(p_nb) : nullptr, nullptr))
      return rc;
    return out.finish(h);
  });
}

int orbx_map_track_local_device(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg, orbx_map_points* mp,
                                int n_frames, int n_kfs, const orbx_keyframe* const* kfs, const int* ref_kf, int n_best, const orbx_keypoint* d_kp,
                                const uint8_t* d_desc, const int* d_feat_start, const int* d_feat_count, int feat_count_stride, int max_feat,
                                const double* d_search_poses_wc, const double* d_priors_wc, int list_cap, int* d_local_kf, int* d_list_offsets,
                                int* d_list_slot, double* d_positions, uint8_t* d_mp_desc, int* d_offsets, double* d_pts3d, float* d_pts2d, int* d_mp_idx,
                                int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out, orbx_pnp_result* d_pnp_results,
                                int* d_matched, int* d_matched_slot, orbx_track_result* d_results) {
  static const char* who = "orbx_map_track_local_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    LocalPlan P;
    if (int rc = local_plan(h, who, mp, n_frames, n_kfs, kfs, ref_kf, n_best, P)) return rc;
    const MapTrackDev D{d_kp, d_desc, d_feat_start, d_feat_count, feat_count_stride, max_feat, d_search_poses_wc, d_priors_wc, d_list_offsets, d_list_slot,
                        d_positions, d_mp_desc, d_offsets, d_pts3d, d_pts2d, d_mp_idx, d_feat_idx, d_poses_wc_out, d_inlier_out, d_err_out, d_pnp_results,
                        d_matched, d_matched_slot, d_results};
    return ms_track_device(h, who, cam, cfg, pnp_cfg, n_frames, P.bound_off.data(), D, [&] {
      return local_select_enqueue(h, who, mp, n_frames, P, ref_kf, n_best, list_cap, d_local_kf, d_list_offsets, d_list_slot, d_positions, d_mp_desc);
    });
  });
}

int orbx_map_track_local(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg, orbx_map_points* mp,
                         int n_frames, int n_kfs, const orbx_keyframe* const* kfs, const int* ref_kf, int n_best, const orbx_keypoint* kp,
                         const uint8_t* desc, const int* feat_offsets, const double* search_poses_wc, const double* priors_wc, int list_cap, int* local_kf,
                         int* list_offsets, int* list_slot, int* offsets, double* pts3d, float* pts2d, int* mp_idx, int* feat_idx, double* poses_wc_out,
                         uint8_t* inlier_out, double* err_out, orbx_pnp_result* pnp_results, int* matched, int* matched_slot, orbx_track_result* results) {
  static const char* who = "orbx_map_track_local";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    LocalPlan P;
    if (int rc = local_plan(h, who, mp, n_frames, n_kfs, kfs, ref_kf, n_best, P)) return rc;
    const MapTrackHost H{nullptr, 0, kp, desc, feat_offsets, search_poses_wc, priors_wc, list_cap, local_kf, (size_t)n_frames * (1 + (size_t)n_best), list_offsets,
                         list_slot, offsets, pts3d, pts2d, mp_idx, feat_idx, poses_wc_out, inlier_out, err_out, pnp_results, matched, matched_slot, results};
    return ms_track_host(h, who, cam, cfg, pnp_cfg, n_frames, P.bound_off.data(), H,
                         [&](const int*, int* d_lk, int* d_lo, int* d_ls, double* d_gp, uint8_t* d_gd) {
                           return local_select_enqueue(h, who, mp, n_frames, P, ref_kf, n_best, P.bound_off[(size_t)n_frames], d_lk, d_lo, d_ls, d_gp, d_gd);
                         });
  });
}

int orbx_map_collect_ba_window_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int cur, int max_covisible,
                                      int list_cap, int obs_cap, int* d_counts, int* d_local_kf, int* d_fixed_kf, int* d_list_slot, double* d_positions,
                                      orbx_ba_obs32* d_obs32) {
  static const char* who = "orbx_map_collect_ba_window_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    WinPlan P;
    if (int rc = bac_plan(h, who, mp, n_kfs, kfs, cur, max_covisible, P)) return rc;
    return win_enqueue(h, who, mp, P, list_cap, obs_cap, d_counts, d_local_kf, d_fixed_kf, d_list_slot, d_positions, d_obs32);
  });
}

int orbx_map_collect_ba_window(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int cur, int max_covisible, int list_cap,
                               int obs_cap, int* counts, int* local_kf, int* fixed_kf, int* list_slot, double* positions, orbx_ba_obs32* obs32) {
  static const char* who = "orbx_map_collect_ba_window";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    WinPlan P;
    if (int rc = bac_plan(h, who, mp, n_kfs, kfs, cur, max_covisible, P)) return rc;
    return win_collect_host(h, who, mp, P, list_cap, obs_cap, counts, local_kf, fixed_kf, list_slot, positions, obs32);
  });
}

int orbx_map_local_ba(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs,
                      int cur, orbx_should_stop_fn should_stop, void* user, int* local_kf_out, double* poses_wc_out, int* counts_out, int* iterations,
                      double* initial_error, double* final_error) {
  static const char* who = "orbx_map_local_ba";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (!cam || !cfg || !local_kf_out || !counts_out || !iterations || !initial_error || !final_error || (cfg->max_covisible_keyframes > 0 && !poses_wc_out))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (h->allreduce || h->rccl_comm) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the partitioned solve reads its observations on the host (orbx_ba_solve_visual)", who);
    WinPlan P;
    if (int rc = bac_plan(h, who, mp, n_kfs, kfs, cur, cfg->max_covisible_keyframes, P)) return rc;
    return win_local_ba(h, who, cam, cfg, nullptr, mp, kfs, P, should_stop, user, local_kf_out, nullptr, poses_wc_out, counts_out, iterations, initial_error,
                        final_error);
  });
}

int orbx_map_collect_inertial_window_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_chain, const int* chain,
                                            int list_cap, int obs_cap, int* d_counts, int* d_fixed_kf, int* d_list_slot, double* d_positions, orbx_ba_obs32* d_obs32) {
  static const char* who = "orbx_map_collect_inertial_window_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    WinPlan P;
    if (int rc = bic_plan(h, who, mp, n_kfs, kfs, n_chain, chain, P)) return rc;
    return win_enqueue(h, who, mp, P, list_cap, obs_cap, d_counts, nullptr, d_fixed_kf, d_list_slot, d_positions, d_obs32);
  });
}

int orbx_map_collect_inertial_window(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_chain, const int* chain,
                                     int list_cap, int obs_cap, int* counts, int* fixed_kf, int* list_slot, double* positions, orbx_ba_obs32* obs32) {
  static const char* who = "orbx_map_collect_inertial_window";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    WinPlan P;
    if (int rc = bic_plan(h, who, mp, n_kfs, kfs, n_chain, chain, P)) return rc;
    return win_collect_host(h, who, mp, P, list_cap, obs_cap, counts, nullptr, fixed_kf, list_slot, positions, obs32);
  });
}

int orbx_map_local_inertial_ba(orbx_handle* h, const orbx_camera* cam, const orbx_inertial_ba_config* cfg, orbx_map_points* mp, int n_kfs,
                               const orbx_keyframe* const* kfs, int n_chain, const int* chain, const double* velocities, const double* biases, int E,
                               const int* edge_kf, const double* preint, orbx_should_stop_fn should_stop, void* user, double* poses_wc_out, double* vel_out,
                               double* bias_out, int* fixed_kf_out, int* counts_out, int* iterations, double* initial_error, double* final_error) {
  static const char* who = "orbx_map_local_inertial_ba";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (!cam || !cfg || !fixed_kf_out || !counts_out || !iterations || !initial_error || !final_error || E < 0 || (E > 0 && (!edge_kf || !preint)) ||
        (n_chain > 0 && (!velocities || !biases || !poses_wc_out || !vel_out || !bias_out)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (h->allreduce || h->rccl_comm) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the inertial solve is not partitioned: no all-reduce hook or communicator", who);
    WinPlan P;
    if (int rc = bic_plan(h, who, mp, n_kfs, kfs, n_chain, chain, P)) return rc;
    // the solver's own refusals, made before the collection is enqueued (ba_check_inertial repeats them)
    if (n_chain > BA_INERTIAL_MAX_K) return orbx_fail(h, ORBX_ERR_INVALID, "%s: at most %d keyframes per inertial window", who, BA_INERTIAL_MAX_K);
    for (int e = 0; e < E; ++e) {
      const int i = edge_kf[2 * e], j = edge_kf[2 * e + 1];
      if (i < 0 || i >= n_chain || j < 0 || j >= n_chain) return orbx_fail(h, ORBX_ERR_INVALID, "%s: IMU edge %d: keyframe index out of range", who, e);
      if (i == j) return orbx_fail(h, ORBX_ERR_INVALID, "%s: IMU edge %d: both ends are keyframe %d", who, e, i);
    }
    const orbx_ba_config vc{cfg->max_iterations, 0.0, 1e-8, cfg->huber_threshold_mono, 0};
    const BaInertialHost in{cfg, velocities, biases, E, edge_kf, preint, vel_out, bias_out};
    return win_local_ba(h, who, cam, &vc, &in, mp, kfs, P, should_stop, user, nullptr, fixed_kf_out, poses_wc_out, counts_out, iterations, initial_error,
                        final_error);
  });
}

int orbx_map_collect_global_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int list_cap, int obs_cap, int* d_counts,
                                   int* d_list_slot, double* d_positions, orbx_ba_obs32* d_obs32) {
  static const char* who = "orbx_map_collect_global_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    WinPlan P;
    if (int rc = glb_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    return win_enqueue(h, who, mp, P, list_cap, obs_cap, d_counts, nullptr, nullptr, d_list_slot, d_positions, d_obs32);
  });
}

int orbx_map_collect_global(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int list_cap, int obs_cap, int* counts,
                            int* list_slot, double* positions, orbx_ba_obs32* obs32) {
  static const char* who = "orbx_map_collect_global";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    WinPlan P;
    if (int rc = glb_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    return win_collect_host(h, who, mp, P, list_cap, obs_cap, counts, nullptr, nullptr, list_slot, positions, obs32);
  });
}

int orbx_map_global_ba(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs,
                       orbx_should_stop_fn should_stop, void* user, double* poses_wc_out, int* counts_out, int* iterations, double* initial_error,
                       double* final_error) {
  static const char* who = "orbx_map_global_ba";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (!cam || !cfg || !counts_out || !iterations || !initial_error || !final_error || (n_kfs > 1 && !poses_wc_out))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (h->allreduce || h->rccl_comm) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the whole-map solve is not partitioned: no all-reduce hook or communicator", who);
    WinPlan P;
    if (int rc = glb_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    // the solver's own refusal, made before the collection is enqueued
    if (n_kfs - 1 > gba_max_keyframes()) return orbx_fail(h, ORBX_ERR_INVALID, "%s: at most %d optimised keyframes per call (n_kfs - 1 = %d)", who, gba_max_keyframes(), n_kfs - 1);
    return win_global_ba(h, who, cam, cfg, mp, kfs, P, should_stop, user, poses_wc_out, counts_out, iterations, initial_error, final_error);
  });
}

int orbx_map_observations_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots, int obs_cap,
                                 int* d_obs_start, int* d_obs_kf, int* d_obs_feat) {
  static const char* who = "orbx_map_observations_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    ObsPlan P;
    if (int rc = obs_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    if (int rc = obs_check_slots(mp, who, slots, M)) return rc;
    return obs_lists_call(h, who, mp, P, M, slots, obs_cap, d_obs_start, d_obs_kf, d_obs_feat);
  });
}

int orbx_map_observations(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots, int obs_cap, int* obs_start,
                          int* obs_kf, int* obs_feat) {
  static const char* who = "orbx_map_observations";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    ObsPlan P;
    if (int rc = obs_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    if (int rc = obs_check_slots(mp, who, slots, M)) return rc;
    if (obs_cap < P.n_feat || !obs_start || (P.n_feat > 0 && M > 0 && (!obs_kf || !obs_feat)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (obs_cap %d must reach the observations' bound %d: the features of kfs[] summed)", who, obs_cap, P.n_feat);
    ORBX_HIP(h, hipSetDevice(h->device));
    const size_t Mz = (size_t)M, Nb = (size_t)obs_entry_bound(P, M);
    OutputPlan out;
    const auto p_os = out.add(obs_start, Mz + 1), p_ok = out.add(obs_kf, Nb, true), p_of = out.add(obs_feat, Nb, true);
    if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs)) return rc;
    if (int rc = obs_lists_call(h, who, mp, P, M, slots, P.n_feat, out.dev(p_os), out.dev(p_ok), out.dev(p_of))) return rc;
    if (int rc = out.finish(h)) return rc;
    const size_t N = (size_t)obs_start[M];                                  // the entries there are, not their bound
    if (int rc = out.copy(h, p_ok, N)) return rc;
    return out.copy(h, p_of, N);
  });
}

int orbx_map_refresh_points_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots, double scale_range,
                                   uint8_t* d_mp_desc, double* d_normals, double* d_min_distance, double* d_max_distance, orbx_mp_refresh_record* d_records) {
  static const char* who = "orbx_map_refresh_points_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    ObsPlan P;
    if (int rc = obs_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    if (int rc = obs_check_slots(mp, who, slots, M)) return rc;
    if (M == 0) return ORBX_OK;
    if (!d_mp_desc || !d_normals || !d_min_distance || !d_max_distance || !d_records || ((uintptr_t)d_mp_desc & 7) || ((uintptr_t)d_normals & 7))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (d_mp_desc and d_normals are 8-byte aligned)", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    return obs_refresh_enqueue(h, who, mp, P, kfs, M, slots, scale_range, d_normals, d_mp_desc, d_normals, d_min_distance, d_max_distance, d_records);
  });
}

int orbx_map_refresh_points(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots, double scale_range,
                            uint8_t* mp_desc, double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records) {
  static const char* who = "orbx_map_refresh_points";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    ObsPlan P;
    if (int rc = obs_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    if (int rc = obs_check_slots(mp, who, slots, M)) return rc;
    if (M == 0) return ORBX_OK;
    if (!mp_desc || !normals || !min_distance || !max_distance || !records) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    // the normals up (they are kept where no observer is far enough), one blob down: [mp_desc | normals | min | max | records]
    const size_t Mz = (size_t)M;
    Carve in;
    OutputPlan out;
    const size_t i_nr = in.take(24 * Mz);
    const auto p_md = out.add(mp_desc, 32 * Mz);
    const auto p_nr = out.add(normals, 3 * Mz), p_mn = out.add(min_distance, Mz), p_mx = out.add(max_distance, Mz);
    const auto p_rc = out.add(records, Mz);
    if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs, in.off)) return rc;
    const HostCall& c = out.call;
    std::memcpy(c.hi + i_nr, normals, 24 * Mz);
    if (int rc = orbx_host_call_upload(h, c)) return rc;
    if (int rc = obs_refresh_enqueue(h, who, mp, P, kfs, M, slots, scale_range, (const double*)(c.di + i_nr), out.dev(p_md), out.dev(p_nr), out.dev(p_mn), out.dev(p_mx),
                                     out.dev(p_rc)))
      return rc;
    return out.finish(h);
  });
}

int orbx_map_keyframe_redundancy_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_cand, const int* cand,
                                        int min_observations, double threshold, int* d_total, int* d_redundant, uint8_t* d_cull) {
  static const char* who = "orbx_map_keyframe_redundancy_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    RedPlan P;
    if (int rc = red_plan(h, who, mp, n_kfs, kfs, n_cand, cand, min_observations, P)) return rc;
    if (n_cand == 0) return ORBX_OK;
    return red_enqueue(h, who, mp, P, n_cand, cand, min_observations, threshold, d_total, d_redundant, d_cull);
  });
}

int orbx_map_keyframe_redundancy(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_cand, const int* cand,
                                 int min_observations, double threshold, int* total, int* redundant, uint8_t* cull) {
  static const char* who = "orbx_map_keyframe_redundancy";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    RedPlan P;
    if (int rc = red_plan(h, who, mp, n_kfs, kfs, n_cand, cand, min_observations, P)) return rc;
    if (n_cand == 0) return ORBX_OK;
    if (!total || !redundant || !cull) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    const size_t NC = (size_t)n_cand;
    OutputPlan out;
    const auto p_to = out.add(total, NC), p_re = out.add(redundant, NC);
    const auto p_cu = out.add(cull, NC);
    if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs)) return rc;
    if (int rc = red_enqueue(h, who, mp, P, n_cand, cand, min_observations, threshold, out.dev(p_to), out.dev(p_re), out.dev(p_cu))) return rc;
    return out.finish(h);
  });
}

int orbx_map_track_reference_device(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                                    orbx_map_points* mp, int n_frames, const orbx_keyframe* const* kfs, const orbx_keypoint* d_kp,
                                    const uint8_t* d_desc, const int* d_feat_start, const int* d_feat_count, int feat_count_stride, int max_feat,
                                    const double* d_priors_wc, double* d_kf_positions, uint8_t* d_kf_valid, orbx_dmatch* d_matches, int* d_offsets,
                                    double* d_pts3d, float* d_pts2d, int* d_kf_idx, int* d_feat_idx, double* d_poses_wc_out,
                                    uint8_t* d_inlier_out, double* d_err_out, orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results) {
  static const char* who = "orbx_map_track_reference_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = orbx_pnp_check_config(h, pnp_cfg, who)) return rc;
    if (!cam || min_correspondences < 4 || n_frames < 0 || (n_frames > 0 && !kfs))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (min_correspondences >= 4, n_frames >= 0)", who);
    if (int rc = ms_check_store(h, who, mp)) return rc;
    if (int rc = ms_check_grid_frames(h, who, n_frames)) return rc;
    if (n_frames == 0) return ORBX_OK;
    const size_t B = (size_t)n_frames;
    std::vector<TrackRefItem> items(B);
    std::vector<MapRefItem> tab(B);
    long long K = 0;
    int max_n = 0;
    for (size_t b = 0; b < B; ++b) {
      const orbx_keyframe* kf = kfs[b];
      if (!kf || kf->h != h) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d is null or of another handle", who, (int)b);
      if (kf->slot_store && kf->slot_store != mp) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d's slot table belongs to another store", who, (int)b);
      if (K + kf->n > 0x7fffffff) return orbx_fail(h, ORBX_ERR_INVALID, "%s: too many keyframe features", who);
      items[b].kf_desc = kf->d_desc; items[b].kf_off = (int)K; items[b].n = kf->n;
      tab[b] = MapRefItem{kf->slot_store ? kf->d_mp_slot : nullptr, (int)K, kf->n};
      K += kf->n; max_n = std::max(max_n, kf->n);
    }
    if (K > 0 && (!d_kf_positions || !d_kf_valid)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    if (max_n > 0) {
      uint8_t *hs, *ds;                                                   // (one piece, copied to its last byte and no further: no plan)
      if (int rc = orbx_ring_begin(h, h->ring_map, h->ws_map.ref_items, sizeof(MapRefItem) * B, &hs, &ds)) return rc;
      std::memcpy(hs, tab.data(), sizeof(MapRefItem) * B);
      if (int rc = orbx_ring_commit(h, h->ring_map, h->ws_map.ref_items, sizeof(MapRefItem) * B)) return rc;
      orbx_launch(h, "map_ref_gather_kernel", false, map_ref_gather_kernel, dim3((max_n + MS_THREADS - 1) / MS_THREADS, n_frames), dim3(MS_THREADS), 0, (const MapRefItem*)ds,
                  mp->d_live, mp->d_pos, mp->capacity, d_kf_positions, d_kf_valid);
    }
    ORBX_HIP(h, hipGetLastError());
    return track_reference_enqueue(h, who, cam, pnp_cfg, min_correspondences, n_frames, d_kp, d_desc, d_feat_start, d_feat_count, feat_count_stride,
                                   max_feat, items.data(), d_kf_positions, d_kf_valid, false, d_priors_wc, d_matches, d_offsets, d_pts3d, d_pts2d, d_kf_idx,
                                   d_feat_idx, d_poses_wc_out, d_inlier_out, d_err_out, d_pnp_results, d_results);
  });
}

int orbx_keyframe_get_map_point_slots(const orbx_keyframe* kf, int* slots) {
  if (!kf) return ORBX_ERR_INVALID;
  orbx_handle* h = kf->h;
  return orbx_guard(h, "orbx_keyframe_get_map_point_slots", [&]() -> int {
    if (kf->n > 0 && !slots) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_keyframe_get_map_point_slots: bad argument");
    if (kf->n == 0) return ORBX_OK;
    if (!kf->slot_store) { std::fill(slots, slots + kf->n, -1); return ORBX_OK; }       // no table: every feature -1
    ORBX_HIP(h, hipSetDevice(h->device));
    ORBX_HIP(h, hipMemcpyAsync(slots, kf->d_mp_slot, 4 * (size_t)kf->n, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    return ORBX_OK;
  });
}

int orbx_map_fuse_device(orbx_handle* h, const orbx_camera* cam, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int n_src, const int* src, int n_tgt,
                         const int* tgt, double radius_scale, unsigned desc_threshold, int list_cap, int* d_counts, int* d_list_slot, int* d_match, int* d_goner,
                         int* d_keeper) {
  static const char* who = "orbx_map_fuse_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = mf_check(h, who, cam, mp, n_kfs, kfs, n_src, src, n_tgt, tgt, desc_threshold)) return rc;
    long long cand = 0;                                                       // L's bound, before anything is touched: the candidates, at most the capacity
    for (int i = 0; i < n_src; ++i) cand += kfs[src[i]]->n;
    const long long bound = std::min<long long>(cand, mp->capacity);
    if (list_cap < bound) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d is below the list's bound %d (the features of kfs[src[..]], at most the capacity)", who, list_cap, (int)bound);
    if (!d_counts || (bound > 0 && !d_list_slot) || (bound > 0 && n_tgt > 0 && (!d_match || !d_goner || !d_keeper))) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (int rc = mf_give_tables(h, mp, kfs, n_tgt, tgt)) return rc;
    MfPlan P;
    if (int rc = mf_plan(h, who, mp, n_kfs, kfs, n_src, src, n_tgt, tgt, P)) return rc;
    return mf_enqueue(h, who, cam, mp, P, radius_scale, desc_threshold, d_counts, d_list_slot, d_match, d_goner, d_keeper);
  });
}

int orbx_map_fuse(orbx_handle* h, const orbx_camera* cam, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int n_src, const int* src, int n_tgt, const int* tgt,
                  double radius_scale, unsigned desc_threshold, int list_cap, int* counts, int* list_slot, int* match, int* goner, int* keeper) {
  static const char* who = "orbx_map_fuse";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = mf_check(h, who, cam, mp, n_kfs, kfs, n_src, src, n_tgt, tgt, desc_threshold)) return rc;
    long long cand = 0;
    for (int i = 0; i < n_src; ++i) cand += kfs[src[i]]->n;
    const long long bound = std::min<long long>(cand, mp->capacity);
    if (list_cap < bound) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d is below the list's bound %d (the features of kfs[src[..]], at most the capacity)", who, list_cap, (int)bound);
    if (!counts || (bound > 0 && !list_slot) || (bound > 0 && n_tgt > 0 && (!match || !goner || !keeper))) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    if (int rc = mf_give_tables(h, mp, kfs, n_tgt, tgt)) return rc;
    MfPlan P;
    if (int rc = mf_plan(h, who, mp, n_kfs, kfs, n_src, src, n_tgt, tgt, P)) return rc;
    const size_t B = (size_t)P.bound, T = (size_t)n_tgt, Gb = (size_t)P.goner_bound;
    OutputPlan out;
    const auto p_cn = out.add(counts, 4), p_go = out.add(goner, Gb, true), p_ke = out.add(keeper, Gb, true), p_ls = out.add(list_slot, B, true), p_ma = out.add(match, B * T, true);
    if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs)) return rc;
    if (int rc = mf_enqueue(h, who, cam, mp, P, radius_scale, desc_threshold, out.dev(p_cn), out.dev(p_ls), out.dev(p_ma), out.dev(p_go), out.dev(p_ke))) return rc;
    if (int rc = out.finish(h)) return rc;
    const size_t Pn = (size_t)counts[0], G = (size_t)counts[3];
    for (int rc : {out.copy(h, p_ls, Pn), out.copy(h, p_ma, Pn * T), out.copy(h, p_go, G), out.copy(h, p_ke, G)})
      if (rc) return rc;
    return G ? orbx_map_points_erase(mp, goner, (int)G) : ORBX_OK;
  });
}

int orbx_map_search_in_neighbors(orbx_handle* h, const orbx_camera* cam, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int cur, int n_nb, const int* nb,
                                 double radius_scale, unsigned desc_threshold, double scale_range, const double* slot_normals, int goner_cap, int affected_cap,
                                 int* counts, int* goner_a, int* keeper_a, int* goner_b, int* keeper_b, int* n_affected, int* affected_slot, uint8_t* mp_desc,
                                 double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records) {
  static const char* who = "orbx_map_search_in_neighbors";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (n_kfs <= 0 || cur < 0 || cur >= n_kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: cur = %d is outside [0, n_kfs = %d)", who, cur, n_kfs);
    if (int rc = mf_check(h, who, cam, mp, n_kfs, kfs, 1, &cur, n_nb, nb, desc_threshold)) return rc;
    for (int i = 0; i < n_nb; ++i)
      if (nb[i] == cur) return orbx_fail(h, ORBX_ERR_INVALID, "%s: nb[%d] is the current keyframe", who, i);
    // the three lists' bounds, before anything is touched
    long long f_nb = 0;
    for (int i = 0; i < n_nb; ++i) f_nb += kfs[nb[i]]->n;
    const long long cap = mp->capacity, f_cur = kfs[cur]->n;
    const long long gb_a = std::min(f_cur, cap) + f_nb, gb_b = std::min(f_nb, cap) + f_cur, ab = std::min(f_cur + f_nb, cap);
    if (int rc = ms_check_feature_total(h, who, f_cur + f_nb)) return rc;
    if (goner_cap < std::max(gb_a, gb_b)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: goner_cap %d is below the passes' bound %d", who, goner_cap, (int)std::max(gb_a, gb_b));
    if (affected_cap < ab) return orbx_fail(h, ORBX_ERR_INVALID, "%s: affected_cap %d is below the list's bound %d (the features of cur and nb[], at most the capacity)", who, affected_cap, (int)ab);
    if (!counts || !n_affected || (gb_a > 0 && (!goner_a || !keeper_a || !goner_b || !keeper_b)) ||
        (ab > 0 && (!affected_slot || !mp_desc || !normals || !min_distance || !max_distance || !records)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    std::vector<int> both((size_t)n_nb + 1);
    both[0] = cur;
    for (int i = 0; i < n_nb; ++i) both[(size_t)i + 1] = nb[i];
    if (int rc = mf_give_tables(h, mp, kfs, n_nb + 1, both.data())) return rc;
    MfPlan A, B;
    SelPlan S;
    if (int rc = mf_plan(h, who, mp, n_kfs, kfs, 1, &cur, n_nb, nb, A)) return rc;
    if (int rc = mf_plan(h, who, mp, n_kfs, kfs, n_nb, nb, 1, &cur, B)) return rc;
    std::vector<const orbx_keyframe*> ak((size_t)n_nb + 1);
    for (size_t i = 0; i < ak.size(); ++i) ak[i] = kfs[both[i]];
    const int aoff[2] = {0, n_nb + 1};
    if (int rc = ms_plan(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, ak.data(), aoff, nullptr, S)) return rc;
    const size_t Ta = (size_t)n_nb, Ba = (size_t)A.bound, Bb = (size_t)B.bound, Ga = (size_t)A.goner_bound, Gb = (size_t)B.goner_bound, Ab = (size_t)S.bound_off[1];
    // ONE download: counts A | counts B | goners and keepers of A, of B | the affected list; behind it what stays on the device
    OutputPlan out;
    const auto p_cn = out.add(counts, 8), p_ga = out.add(goner_a, Ga, true), p_ka = out.add(keeper_a, Ga, true), p_gb = out.add(goner_b, Gb, true),
               p_kb = out.add(keeper_b, Gb, true), p_ao = out.add((int*)nullptr, 2), p_as = out.add(affected_slot, Ab, true);
    const size_t o_la = out.keep(4 * Ba), o_ma = out.keep(4 * Ba * Ta), o_lb = out.keep(4 * Bb), o_mb = out.keep(4 * Bb), o_ap = out.keep(24 * Ab), o_ad = out.keep(32 * Ab);
    // (the refresh below is a host form of its own: it takes the pinned buffer and the blob workspace once everything is copied out of them)
    if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs)) return rc;
    uint8_t* d = out.call.dout;
    if (int rc = mf_enqueue(h, who, cam, mp, A, radius_scale, desc_threshold, out.dev(p_cn), (int*)(d + o_la), (int*)(d + o_ma), out.dev(p_ga), out.dev(p_ka))) return rc;
    if (int rc = mf_enqueue(h, who, cam, mp, B, radius_scale, desc_threshold, out.dev(p_cn) + 4, (int*)(d + o_lb), (int*)(d + o_mb), out.dev(p_gb), out.dev(p_kb))) return rc;
    if (int rc = ms_select_enqueue(h, who, mp, ORBX_MAP_SOURCE_KEYFRAMES, 1, S, nullptr, nullptr, (int)Ab, out.dev(p_ao), out.dev(p_as), (double*)(d + o_ap), d + o_ad))
      return rc;
    if (int rc = out.finish(h)) return rc;
    const size_t na = (size_t)counts[3], nbg = (size_t)counts[7], M = (size_t)out.host(p_ao)[1];
    for (int rc : {out.copy(h, p_ga, na), out.copy(h, p_ka, na), out.copy(h, p_gb, nbg), out.copy(h, p_kb, nbg), out.copy(h, p_as, M)})
      if (rc) return rc;
    *n_affected = (int)M;
    if (na) if (int rc = orbx_map_points_erase(mp, goner_a, (int)na)) return rc;
    if (nbg) if (int rc = orbx_map_points_erase(mp, goner_b, (int)nbg)) return rc;
    if (M == 0) return ORBX_OK;
    for (size_t i = 0; i < M; ++i) {
      const double* v = slot_normals ? slot_normals + 3 * (size_t)affected_slot[i] : nullptr;
      normals[3 * i] = v ? v[0] : 0.0; normals[3 * i + 1] = v ? v[1] : 0.0; normals[3 * i + 2] = v ? v[2] : 0.0;
    }
    return orbx_map_refresh_points(h, mp, n_kfs, kfs, (int)M, affected_slot, scale_range, mp_desc, normals, min_distance, max_distance, records);
  });
}

int orbx_keyframe_set_map_point_slots_device(orbx_keyframe* kf, const orbx_map_points* mp, const int* d_slots) {
  static const char* who = "orbx_keyframe_set_map_point_slots_device";
  if (!kf) return ORBX_ERR_INVALID;
  orbx_handle* h = kf->h;
  return orbx_guard(h, who, [&]() -> int {
    if (!mp || mp->h != h || !d_slots || ((uintptr_t)d_slots & 3)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the store is null or of another handle, or d_slots is null or not 4-byte aligned", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    if (kf->n > 0) {
      const dim3 grid((kf->n + MS_THREADS - 1) / MS_THREADS), block(MS_THREADS);
      orbx_launch(h, "mc_table_kernel", false, mc_table_kernel, grid, block, 0, d_slots, kf->n, mp->capacity, kf->d_mp_slot);
      orbx_launch(h, "mc_uniq_one_kernel", true, mc_uniq_one_kernel, grid, block, 0, (const int*)kf->d_mp_slot, kf->d_mp_uniq, kf->n);
      ORBX_HIP(h, hipGetLastError());
    }
    kf->slot_store = mp;
    return ORBX_OK;
  });
}

int orbx_map_create_points_device(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial, orbx_map_points* mp,
                                  orbx_keyframe* cur, orbx_keyframe* const* nbs, int T, int phases, const int* free_slots, int n_free, int* d_counts,
                                  int* d_new_slot, int* d_new_neighbour, int* d_new_idx1, int* d_new_idx2, double* d_new_points, uint8_t* d_new_desc, int* d_stats) {
  static const char* who = "orbx_map_create_points_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = mc_check(h, who, cam, cfg, mp, cur, nbs, T, phases, free_slots, n_free)) return rc;
    if (!d_counts || (T > 0 && !d_stats) || (n_free > 0 && (!d_new_slot || !d_new_neighbour || !d_new_idx1 || !d_new_idx2 || !d_new_points || !d_new_desc)) ||
        ((uintptr_t)d_new_desc & 15))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (d_new_desc is 16-byte aligned)", who);
    return mc_enqueue(h, cam, cfg, is_inertial, mp, cur, nbs, T, phases, free_slots, n_free, d_counts, d_new_slot, d_new_neighbour, d_new_idx1, d_new_idx2, d_new_points,
                      d_new_desc, d_stats);
  });
}

int orbx_map_create_points(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial, orbx_map_points* mp, orbx_keyframe* cur,
                           orbx_keyframe* const* nbs, int T, int phases, const int* free_slots, int n_free, int* counts, int* new_slot, int* new_neighbour,
                           int* new_idx1, int* new_idx2, double* new_points, int* stats) {
  static const char* who = "orbx_map_create_points";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (int rc = mc_check(h, who, cam, cfg, mp, cur, nbs, T, phases, free_slots, n_free)) return rc;
    if (!counts || (T > 0 && !stats) || (n_free > 0 && (!new_slot || !new_neighbour || !new_idx1 || !new_idx2 || !new_points)))
      return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    ORBX_HIP(h, hipSetDevice(h->device));
    // ONE download: counts | stats | the lists; the descriptors stay behind them for set_device
    const size_t NF = (size_t)n_free, Tz = (size_t)T;
    OutputPlan out;
    const auto p_cn = out.add(counts, 4), p_st = out.add(stats, 4 * Tz), p_sl = out.add(new_slot, NF, true), p_nb = out.add(new_neighbour, NF, true),
               p_i1 = out.add(new_idx1, NF, true), p_i2 = out.add(new_idx2, NF, true);
    const auto p_pt = out.add(new_points, 3 * NF, true);
    const size_t o_de = out.keep(32 * NF);
    if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs)) return rc;
    uint8_t* d_de = out.call.dout + o_de;
    if (int rc = mc_enqueue(h, cam, cfg, is_inertial, mp, cur, nbs, T, phases, free_slots, n_free, out.dev(p_cn), out.dev(p_sl), out.dev(p_nb), out.dev(p_i1), out.dev(p_i2),
                            out.dev(p_pt), d_de, out.dev(p_st)))
      return rc;
    if (int rc = out.finish(h)) return rc;
    const size_t created = (size_t)counts[2];
    if (created == 0) return ORBX_OK;
    for (int rc : {out.copy(h, p_sl, created), out.copy(h, p_nb, created), out.copy(h, p_i1, created), out.copy(h, p_i2, created), out.copy(h, p_pt, 3 * created)})
      if (rc) return rc;
    return ms_set(mp, who, free_slots, (int)created, out.dev(p_pt), d_de, false);
  });
}

int orbx_map_remove_points(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n, const int* slots, int* n_cleared) {
  static const char* who = "orbx_map_remove_points";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    ObsPlan P;
    if (int rc = mr_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    if (int rc = ms_check_slots(mp, who, slots, n, false)) return rc;
    if (n == 0) { if (n_cleared) *n_cleared = 0; return ORBX_OK; }
    const int* d_cleared = nullptr;
    if (int rc = mr_enqueue(h, mp, P.C, n, slots, &d_cleared)) return rc;
    if (!n_cleared) return ORBX_OK;
    if (int rc = orbx_reserve_pinned(h, h->pin_map, 4)) return rc;
    ORBX_HIP(h, hipMemcpyAsync(h->pin_map.p, d_cleared, 4, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    std::memcpy(n_cleared, h->pin_map.p, 4);
    return ORBX_OK;
  });
}

int orbx_map_cull_points(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* cand, int min_observations,
                         int* n_culled, int* culled) {
  static const char* who = "orbx_map_cull_points";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    ObsPlan P;
    if (int rc = mr_plan(h, who, mp, n_kfs, kfs, P)) return rc;
    if (int rc = obs_check_slots(mp, who, cand, M)) return rc;
    if (!n_culled || (M > 0 && !culled)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
    *n_culled = 0;
    if (M == 0) return ORBX_OK;
    ORBX_HIP(h, hipSetDevice(h->device));
    if (int rc = orbx_reserve_pinned(h, h->pin_map, 4 * (size_t)M)) return rc;
    ObsCall c;
    c.n_points = M; c.slots = cand;
    const int* d_count = nullptr;
    if (int rc = obs_enqueue(h, mp, P, c, nullptr, &d_count)) return rc;
    // the one download: the candidates' observer counts.  The comparison is the host's: the mirror needs the list anyway.
    ORBX_HIP(h, hipMemcpyAsync(h->pin_map.p, d_count, 4 * (size_t)M, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    const int* count = (const int*)h->pin_map.p;
    int n = 0;
    for (int i = 0; i < M; ++i)
      if (count[i] < min_observations) culled[n++] = cand[i];               // local_mapper.rs:452: strictly fewer
    *n_culled = n;
    if (n == 0) return ORBX_OK;
    const int* d_cleared = nullptr;
    return mr_enqueue(h, mp, P.C, n, culled, &d_cleared);
  });
}

}  // extern "C"
