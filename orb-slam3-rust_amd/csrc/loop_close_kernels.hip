// loop_close_kernels.hip — step 5 of LoopCloser::process_keyframe (loop_closer.rs:155-241) on the resident map: the rigid loop
// correction and the loop closer's fuse (corrector.rs:383-619: collect_correction_data, compute_correction, apply_correction,
// fuse_map_points), acting on the slot tables, the store and the keyframes' poses where they lie (include/orbx.h, "loop correction
// on the resident map").
//
// The device form is these launches on the handle's stream, with no host synchronisation inside:
//   (the N x N covisibility weights: orbx_map_covisibility_device with every keyframe as a query, LC_Q_BATCH queries a call; the
//    table stays in the call's workspace, N <= 4096 bounds it at 64 MB)
//   lc_reach_kernel      one workgroup: the keyframes within max_propagation_depth arcs of cur, level by level.  level[] and the two
//                        frontier lists are in LDS; an unreached keyframe j joins level d + 1 iff its parent is in level d or a
//                        keyframe of level d has weight >= min with it (the weights' row walked by the threads: coalesced); the set
//                        is the same whatever order the frontier is listed in.  affected[], counts = {|A|, 0, 0, 0}
//   lc_mark_kernel       (chunk of LC_CHUNK features, keyframe) index[slot] = atomicMin(feature number) over the live entries of A's tables
//   lc_flag_kernel       the feature the table names survives and puts the entry back to EMPTY; per chunk the survivors
//   lc_emit_kernel       ordered compaction behind the earlier chunks' survivors (block_sum, BlockScan) -> list_slot, counts[1]
//   lc_correct_kernel    thread i: keyframe i's pose out (corrected for A, as found otherwise), and point i of the list corrected in
//                        the store: each listed slot once, whatever number of features names it
//   lc_pair_kernel       per match the pair (table(cur)[fc], table(loop)[fl]) if both are live and differ; index[slot] = atomicMin
//                        of the slot's place in the flattened pair list: a slot's NODE is its first occurrence there; counts[2]
//   lc_nobs_kernel       (chunk, keyframe) n_observers of every node from the de-duplicated tables (integer atomicAdd)
//   lc_class_kernel      one workgroup: minimum-label propagation over the pairs to the fixed point, as mf_class_kernel does it
//   lc_key_kernel        per class the packed maximum (observers, first occurrence) -> the keeper; its size
//   lc_goner_kernel      what every node's entries become (repl[]); the goners through an atomic cursor
//   lc_goner_rank_kernel the goners are distinct slots: the number of smaller ones is a goner's place, which fixes the bytes; counts[3]
//   lc_rewrite_kernel    (chunk, keyframe) over ALL keyframes: an entry that names a goner becomes its keeper; the keyframes that changed
//   lc_uniq_kernel       (block, keyframe) of a changed keyframe: d_mp_uniq again
//   lc_restore_kernel    index back to EMPTY for every paired slot: the call leaves the store's tables as it found them
// Every atomic is an integer min, max or add, and no launch is sized by the store's capacity: the outputs are the same bytes on
// every run and a call costs what its keyframes and matches cost.
// Barriers: the two single-workgroup kernels loop to a fixed point.  Every thread of the workgroup reaches every __syncthreads();
// a loop is left on a flag read from LDS behind a barrier, which nothing writes before the next one.
#include <algorithm>
#include <cmath>
#include <vector>

#include "block_dev.hpp"
#include "orbx_internal.hpp"

namespace {

constexpr int LC_THREADS = 256;
constexpr int LC_PER = 4;                        // consecutive features per thread
constexpr int LC_CHUNK = LC_THREADS * LC_PER;    // features per workgroup
constexpr int LC_EMPTY = 0x7f7f7f7f;             // the store's first-sighting tables between calls (map_store_kernels.hip: MS_EMPTY)
constexpr int LC_MAX_KFS = 4096;                 // level[] and the frontiers are held in LDS; the weights are [n_kfs][n_kfs]
constexpr int LC_ONE_THREADS = 1024;             // the two single-workgroup kernels
constexpr int LC_Q_BATCH = 1024;                 // queries per covisibility call: the store's mark bytes are [queries][capacity]

struct LcKf {                                    // one keyframe of kfs[]
  int* slots; int* uniq;                         // its table and the same with repeats set to -1; NULL: no table
  int n, base;                                   // its features; the number of its first feature among all features of kfs[]
};

struct LcArgs {
  int capacity, n_kfs, n_chunk, cur, loop, n_matches, min_weight, max_depth;
  double qc[4], tc[3], sc;                       // C, the inverse of sim3_current_to_loop
  const uint8_t* live; double* pos;
  const LcKf* kfs; const int* parent; const double* poses_in;
  const int* weights;                            // [n_kfs][n_kfs]
  const int* matches;                            // [n_matches][2]
  int* index;                                    // the store's first-sighting table, row 0: EMPTY outside the launches below
  int* cand; int* chunk_count;                   // [n_kfs][n_chunk][LC_CHUNK], [n_kfs][n_chunk]
  int* pair;                                     // [2 n_matches] the flattened pair list, -1 where the match is no pair
  int* label; int* repl;                         // [nodes]
  int* nobs; unsigned long long* key; int* csize;   // [nodes], zeroed before the launches; key and csize read at a class's label
  int* changed;                                  // [n_kfs]
  int* cursor; int* tmp_goner; int* tmp_keeper;
  int* counts; uint8_t* affected; double* poses_out; int* list_slot; int* goner; int* keeper;
};

__device__ __forceinline__ bool lc_live(const LcArgs& A, int s) { return s >= 0 && s < A.capacity && A.live[s]; }

// q * v for a unit quaternion (w, x, y, z), nalgebra's form: t = 2 qv x v; v + w t + qv x t
__host__ __device__ inline void lc_rotate(const double* q, const double* v, double* out) {
  const double t[3] = {2.0 * (q[2] * v[2] - q[3] * v[1]), 2.0 * (q[3] * v[0] - q[1] * v[2]), 2.0 * (q[1] * v[1] - q[2] * v[0])};
  out[0] = v[0] + q[0] * t[0] + (q[2] * t[2] - q[3] * t[1]);
  out[1] = v[1] + q[0] * t[1] + (q[3] * t[0] - q[1] * t[2]);
  out[2] = v[2] + q[0] * t[2] + (q[1] * t[1] - q[2] * t[0]);
}

__global__ __launch_bounds__(LC_ONE_THREADS) void lc_reach_kernel(LcArgs A) {
  __shared__ short level[LC_MAX_KFS];
  __shared__ unsigned short front[2][LC_MAX_KFS];
  __shared__ int n_front[2];
  __shared__ int wave_tot[LC_ONE_THREADS / 64];
  const int N = A.n_kfs, tid = threadIdx.x;
  for (int k = tid; k < N; k += LC_ONE_THREADS) level[k] = k == A.cur ? 0 : -1;
  if (tid == 0) { front[0][0] = (unsigned short)A.cur; n_front[0] = 1; n_front[1] = 0; }
  int side = 0;
  for (int d = 0; d < A.max_depth; ++d) {                                  // (max_depth is the launch's: the same in every thread)
    __syncthreads();                                                       // (level d's list and its length; level[])
    const int nf = n_front[side];
    if (nf == 0) break;                                                    // (the same in every thread: nothing writes this cell before the next barrier)
    if (tid == 0) n_front[side ^ 1] = 0;
    __syncthreads();
    for (int j = tid; j < N; j += LC_ONE_THREADS) {
      if (level[j] >= 0) continue;
      const int p = A.parent[j];
      bool hit = p >= 0 && level[p] == d;                                  // (a cell another thread is moving from -1 to d + 1 is not d either way)
      for (int f = 0; f < nf && !hit; ++f) hit = A.weights[(size_t)front[side][f] * N + j] >= A.min_weight;
      if (hit) {
        level[j] = (short)(d + 1);
        front[side ^ 1][atomicAdd(&n_front[side ^ 1], 1)] = (unsigned short)j;
      }
    }
    side ^= 1;
  }
  __syncthreads();
  int n = 0;
  for (int k = tid; k < N; k += LC_ONE_THREADS) {
    const int in = level[k] >= 0;
    A.affected[k] = (uint8_t)in;
    n += in;
  }
  n = block_sum<LC_ONE_THREADS>(n, wave_tot);
  if (tid < 4) A.counts[tid] = tid == 0 ? n : 0;
}

__global__ __launch_bounds__(LC_THREADS) void lc_mark_kernel(LcArgs A) {
  const int k = blockIdx.y;
  const LcKf kf = A.kfs[k];
  const bool in = A.affected[k] && kf.slots;
  const int i0 = blockIdx.x * LC_CHUNK + threadIdx.x * LC_PER;
  int* cand = A.cand + ((size_t)k * A.n_chunk + blockIdx.x) * LC_CHUNK + threadIdx.x * LC_PER;
#pragma unroll
  for (int j = 0; j < LC_PER; ++j) {
    const int i = i0 + j;
    int slot = in && i < kf.n ? kf.slots[i] : -1;
    if (!lc_live(A, slot)) slot = -1;
    else atomicMin(&A.index[slot], kf.base + i);
    cand[j] = slot;
  }
}

__global__ __launch_bounds__(LC_THREADS) void lc_flag_kernel(LcArgs A) {
  __shared__ int wave_tot[LC_THREADS / 64];
  const int k = blockIdx.y;
  const int p0 = A.kfs[k].base + blockIdx.x * LC_CHUNK + threadIdx.x * LC_PER;
  int* cand = A.cand + ((size_t)k * A.n_chunk + blockIdx.x) * LC_CHUNK + threadIdx.x * LC_PER;
  int n = 0;
#pragma unroll
  for (int j = 0; j < LC_PER; ++j) {
    const int slot = cand[j];
    if (slot < 0) continue;
    // only the feature the table names writes it (back to EMPTY); the others read its number or EMPTY, never their own
    if (__hip_atomic_load(&A.index[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p0 + j) {
      __hip_atomic_store(&A.index[slot], LC_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ++n;
    } else {
      cand[j] = -1;
    }
  }
  n = block_sum<LC_THREADS>(n, wave_tot);
  if (threadIdx.x == 0) A.chunk_count[k * A.n_chunk + blockIdx.x] = n;
}

__global__ __launch_bounds__(LC_THREADS) void lc_emit_kernel(LcArgs A) {
  __shared__ int wave_tot[LC_THREADS / 64];
  const int tid = threadIdx.x, me = blockIdx.y * A.n_chunk + blockIdx.x;
  int part = 0;
  for (int j = tid; j < me; j += LC_THREADS) part += A.chunk_count[j];
  const int base = block_sum<LC_THREADS>(part, wave_tot);
  if (tid == 0 && me == A.n_kfs * A.n_chunk - 1) A.counts[1] = base + A.chunk_count[me];
  const int* cand = A.cand + (size_t)me * LC_CHUNK + tid * LC_PER;
  int slot[LC_PER], n = 0;
#pragma unroll
  for (int j = 0; j < LC_PER; ++j) { slot[j] = cand[j]; n += slot[j] >= 0; }
  int o = BlockScan<LC_THREADS>(wave_tot, base).round(n);
#pragma unroll
  for (int j = 0; j < LC_PER; ++j)
    if (slot[j] >= 0) A.list_slot[o++] = slot[j];
}

// compute_correction / apply_correction (:493-515, :531-545): C applied to the poses of A and, once each, to the listed points
__global__ __launch_bounds__(LC_THREADS) void lc_correct_kernel(LcArgs A) {
  const int i = blockIdx.x * LC_THREADS + threadIdx.x;
  if (i < A.n_kfs) {
    const double* p = A.poses_in + 7 * (size_t)i;
    double* o = A.poses_out + 7 * (size_t)i;
    if (A.affected[i]) {
      const double *c = A.qc, *q = p;
      double r[3];
      lc_rotate(A.qc, p + 4, r);
      o[0] = c[0] * q[0] - c[1] * q[1] - c[2] * q[2] - c[3] * q[3];
      o[1] = c[0] * q[1] + c[1] * q[0] + c[2] * q[3] - c[3] * q[2];
      o[2] = c[0] * q[2] - c[1] * q[3] + c[2] * q[0] + c[3] * q[1];
      o[3] = c[0] * q[3] + c[1] * q[2] - c[2] * q[1] + c[3] * q[0];
      for (int a = 0; a < 3; ++a) o[4 + a] = A.sc * r[a] + A.tc[a];
    } else {
      for (int a = 0; a < 7; ++a) o[a] = p[a];
    }
  }
  if (i < A.counts[1]) {
    double* p = A.pos + 3 * (size_t)A.list_slot[i];
    const double v[3] = {p[0], p[1], p[2]};
    double r[3];
    lc_rotate(A.qc, v, r);
    for (int a = 0; a < 3; ++a) p[a] = A.sc * r[a] + A.tc[a];
  }
}

__global__ __launch_bounds__(LC_THREADS) void lc_pair_kernel(LcArgs A) {
  __shared__ int wave_tot[LC_THREADS / 64];
  const int m = blockIdx.x * LC_THREADS + threadIdx.x;
  int valid = 0;
  if (m < A.n_matches) {
    const LcKf kc = A.kfs[A.cur], kl = A.kfs[A.loop];
    const int fc = A.matches[2 * (size_t)m], fl = A.matches[2 * (size_t)m + 1];
    const int a = kc.slots && fc >= 0 && fc < kc.n ? kc.slots[fc] : -1;
    const int b = kl.slots && fl >= 0 && fl < kl.n ? kl.slots[fl] : -1;
    valid = lc_live(A, a) && lc_live(A, b) && a != b;
    A.pair[2 * (size_t)m] = valid ? a : -1;
    A.pair[2 * (size_t)m + 1] = valid ? b : -1;
    if (valid) { atomicMin(&A.index[a], 2 * m); atomicMin(&A.index[b], 2 * m + 1); }
  }
  valid = block_sum<LC_THREADS>(valid, wave_tot);
  if (threadIdx.x == 0 && valid) atomicAdd(&A.counts[2], valid);
}

__global__ __launch_bounds__(LC_THREADS) void lc_nobs_kernel(LcArgs A) {
  const LcKf kf = A.kfs[blockIdx.y];
  if (!kf.uniq) return;
#pragma unroll
  for (int j = 0; j < LC_PER; ++j) {
    const int i = blockIdx.x * LC_CHUNK + j * LC_THREADS + threadIdx.x;
    if (i >= kf.n) continue;
    const int s = kf.uniq[i];
    if (!lc_live(A, s)) continue;
    const int id = A.index[s];
    if (id != LC_EMPTY) atomicAdd(&A.nobs[id], 1);
  }
}

__global__ __launch_bounds__(LC_ONE_THREADS) void lc_class_kernel(LcArgs A) {
  __shared__ int again;
  const int M = A.n_matches, tid = threadIdx.x;
  for (int id = tid; id < 2 * M; id += LC_ONE_THREADS) A.label[id] = id;
  __threadfence();
  for (;;) {
    __syncthreads();                                                       // (the labels written above; the flag read below)
    if (tid == 0) again = 0;
    __syncthreads();
    bool moved = false;
    for (int m = tid; m < M; m += LC_ONE_THREADS) {
      const int sa = A.pair[2 * (size_t)m];
      if (sa < 0) continue;
      const int a = A.index[sa], b = A.index[A.pair[2 * (size_t)m + 1]];
      const int la = __hip_atomic_load(&A.label[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int lb = __hip_atomic_load(&A.label[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (la == lb) continue;
      const int lo = min(la, lb);
      atomicMin(&A.label[a], lo); atomicMin(&A.label[b], lo);
      atomicMin(&A.label[max(la, lb)], lo);                                // (the higher label's own node: its other members follow in the step below)
      moved = true;
    }
    __syncthreads();
    for (int id = tid; id < 2 * M; id += LC_ONE_THREADS) {
      const int l = __hip_atomic_load(&A.label[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int ll = __hip_atomic_load(&A.label[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (ll < l) { atomicMin(&A.label[id], ll); moved = true; }
    }
    if (moved) again = 1;
    __syncthreads();
    if (!again) break;                                                     // (the same in every thread: nothing writes it before the next barrier)
  }
}

// id is a node iff the flattened list holds a paired slot there and that is the slot's first occurrence
__device__ __forceinline__ bool lc_node(const LcArgs& A, int id, int* slot) {
  *slot = A.pair[id];
  return *slot >= 0 && A.index[*slot] == id;
}

__global__ __launch_bounds__(LC_THREADS) void lc_key_kernel(LcArgs A) {
  const int id = blockIdx.x * LC_THREADS + threadIdx.x;
  int slot;
  if (id >= 2 * A.n_matches || !lc_node(A, id, &slot)) return;
  const int c = A.label[id];
  atomicMax(&A.key[c], ((unsigned long long)(unsigned)A.nobs[id] << 32) | (unsigned)(0x7fffffff - id));     // more observers, then the earlier occurrence
  atomicAdd(&A.csize[c], 1);
}

__global__ __launch_bounds__(LC_THREADS) void lc_goner_kernel(LcArgs A) {
  const int id = blockIdx.x * LC_THREADS + threadIdx.x;
  if (id >= 2 * A.n_matches) return;
  int slot, to = -1;
  if (lc_node(A, id, &slot)) {
    const int c = A.label[id], keeper_id = 0x7fffffff - (int)(unsigned)A.key[c];
    if (A.csize[c] >= 2 && keeper_id != id) {
      to = A.pair[keeper_id];
      const int at = atomicAdd(A.cursor, 1);
      A.tmp_goner[at] = slot; A.tmp_keeper[at] = to;
    }
  }
  A.repl[id] = to;
}

__global__ __launch_bounds__(LC_THREADS) void lc_goner_rank_kernel(LcArgs A) {
  __shared__ int tile[LC_THREADS];
  const int G = *A.cursor, tid = threadIdx.x, e = blockIdx.x * LC_THREADS + tid;
  if (blockIdx.x == 0 && tid == 0) A.counts[3] = G;
  if ((int)(blockIdx.x * LC_THREADS) >= G) return;                         // (the block's)
  const int s = e < G ? A.tmp_goner[e] : 0x7fffffff;
  int rank = 0;
  for (int j0 = 0; j0 < G; j0 += LC_THREADS) {
    __syncthreads();
    tile[tid] = j0 + tid < G ? A.tmp_goner[j0 + tid] : 0x7fffffff;
    __syncthreads();
    const int n = min(LC_THREADS, G - j0);
    for (int t = 0; t < n; ++t) rank += tile[t] < s;
  }
  if (e < G) { A.goner[rank] = s; A.keeper[rank] = A.tmp_keeper[e]; }
}

__global__ __launch_bounds__(LC_THREADS) void lc_rewrite_kernel(LcArgs A) {
  const LcKf kf = A.kfs[blockIdx.y];
  if (!kf.slots) return;
#pragma unroll
  for (int j = 0; j < LC_PER; ++j) {
    const int i = blockIdx.x * LC_CHUNK + j * LC_THREADS + threadIdx.x;
    if (i >= kf.n) continue;
    const int e = kf.slots[i];
    if (e < 0 || e >= A.capacity) continue;
    const int id = A.index[e];
    if (id == LC_EMPTY) continue;
    const int to = A.repl[id];
    if (to >= 0) { kf.slots[i] = to; A.changed[blockIdx.y] = 1; }
  }
}

// d_mp_uniq of a changed keyframe: an entry stays where no earlier feature holds it.  Every thread of a block that stays reaches the barriers.
__global__ __launch_bounds__(LC_THREADS) void lc_uniq_kernel(LcArgs A) {
  __shared__ int tile[LC_THREADS];
  const LcKf kf = A.kfs[blockIdx.y];
  if (!kf.slots || !A.changed[blockIdx.y] || (int)(blockIdx.x * LC_THREADS) >= kf.n) return;      // (the block's)
  const int tid = threadIdx.x, i = blockIdx.x * LC_THREADS + tid;
  const int s = i < kf.n ? kf.slots[i] : -1;
  bool earlier = false;
  for (int j0 = 0; j0 <= (int)(blockIdx.x * LC_THREADS); j0 += LC_THREADS) {
    __syncthreads();
    tile[tid] = j0 + tid < kf.n ? kf.slots[j0 + tid] : -1;
    __syncthreads();
    const int n = min(LC_THREADS, i - j0);                                 // the features before i
    for (int t = 0; t < n; ++t) earlier |= tile[t] == s;
  }
  if (i < kf.n) kf.uniq[i] = s >= 0 && !earlier ? s : -1;
}

__global__ __launch_bounds__(LC_THREADS) void lc_restore_kernel(LcArgs A) {
  const int id = blockIdx.x * LC_THREADS + threadIdx.x;
  if (id >= 2 * A.n_matches) return;
  const int s = A.pair[id];
  if (s >= 0) A.index[s] = LC_EMPTY;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// A call, checked and sized on the host.
struct LcPlan {
  std::vector<LcKf> kfs;
  std::vector<double> poses;                     // [n_kfs][7] as found
  double qc[4], tc[3], sc;
  int bound = 0, max_n = 0;                      // the list's bound: the features of kfs[] summed, at most the capacity
};

// What can be refused: nothing is enqueued, and store, tables and poses are untouched.  matches: the host form's array (NULL in the
// device form, where a match outside its keyframe is no pair).
int lc_plan(orbx_handle* h, const char* who, const orbx_loop_correct_config* cfg, const orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, const int* parent,
            int cur, int loop, const double* sim3, int n_matches, const int* matches, int list_cap, LcPlan& P) {
  if (!mp || mp->h != h) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the store is null or of another handle", who);
  if (!cfg || cfg->min_covisibility_weight < 0 || cfg->max_propagation_depth < 0)
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad configuration (min_covisibility_weight >= 0, max_propagation_depth >= 0)", who);
  if (n_kfs > LC_MAX_KFS) return orbx_fail(h, ORBX_ERR_INVALID, "%s: %d keyframes, at most %d (orbx_map_loop_max_keyframes)", who, n_kfs, LC_MAX_KFS);
  if (n_kfs < 0 || !kfs || !parent || !sim3 || n_matches < 0) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (n_kfs >= 0, n_matches >= 0)", who);
  if (cur < 0 || cur >= n_kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: cur = %d is outside [0, %d)", who, cur, n_kfs);
  if (loop < (n_matches == 0 ? -1 : 0) || loop >= n_kfs) return orbx_fail(h, ORBX_ERR_INVALID, "%s: loop = %d is outside [0, %d) (-1: none, with no matches)", who, loop, n_kfs);
  if (cur == loop) return orbx_fail(h, ORBX_ERR_INVALID, "%s: cur and loop are both %d", who, cur);
  for (int k = 0; k < n_kfs; ++k)
    if (parent[k] < -1 || parent[k] >= n_kfs || parent[k] == k) return orbx_fail(h, ORBX_ERR_INVALID, "%s: parent[%d] = %d is outside [-1, %d) or the keyframe itself", who, k, parent[k], n_kfs);
  for (int i = 0; i < 8; ++i)
    if (!std::isfinite(sim3[i])) return orbx_fail(h, ORBX_ERR_INVALID, "%s: sim3[%d] is not finite", who, i);
  if (!(sim3[7] > 0.0)) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the scale %g is not positive", who, sim3[7]);
  long long total = 0;
  P.kfs.resize((size_t)n_kfs); P.poses.resize(7 * (size_t)n_kfs);
  for (int k = 0; k < n_kfs; ++k) {
    orbx_keyframe* kf = kfs[k];
    if (!kf || kf->h != h) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d is null or of another handle", who, k);
    if (kf->slot_store && kf->slot_store != mp) return orbx_fail(h, ORBX_ERR_INVALID, "%s: keyframe %d's slot table belongs to another store", who, k);
    P.kfs[(size_t)k] = LcKf{kf->slot_store ? kf->d_mp_slot : nullptr, kf->slot_store ? kf->d_mp_uniq : nullptr, kf->n, (int)total};
    std::copy(kf->pose_wc, kf->pose_wc + 7, P.poses.begin() + 7 * (size_t)k);
    total += kf->n; P.max_n = std::max(P.max_n, kf->n);
    if (total >= LC_EMPTY) return orbx_fail(h, ORBX_ERR_INVALID, "%s: the keyframes hold too many features", who);
  }
  std::vector<const orbx_keyframe*> seen(kfs, kfs + n_kfs);
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return orbx_fail(h, ORBX_ERR_INVALID, "%s: a keyframe is listed twice in kfs[] (their tables are rewritten)", who);
  if (n_matches > 0) {
    if (n_matches >= LC_EMPTY / 2) return orbx_fail(h, ORBX_ERR_INVALID, "%s: too many matches", who);
    if (!kfs[cur]->slot_store || !kfs[loop]->slot_store) return orbx_fail(h, ORBX_ERR_INVALID, "%s: cur or loop has no slot table, and there are matches", who);
    for (int m = 0; matches && m < n_matches; ++m)
      if (matches[2 * m] < 0 || matches[2 * m] >= kfs[cur]->n || matches[2 * m + 1] < 0 || matches[2 * m + 1] >= kfs[loop]->n)
        return orbx_fail(h, ORBX_ERR_INVALID, "%s: match %d = (%d, %d) is outside its keyframes' features (%d, %d)", who, m, matches[2 * m], matches[2 * m + 1], kfs[cur]->n, kfs[loop]->n);
  }
  P.bound = (int)std::min<long long>(total, mp->capacity);
  if (list_cap < P.bound) return orbx_fail(h, ORBX_ERR_INVALID, "%s: list_cap %d is below the list's bound %d (the features of kfs[] summed, at most the capacity)", who, list_cap, P.bound);
  // C = sim3^-1 (sim3.rs:144-154): R_c = R^-1, s_c = 1 / s, t_c = -(R_c t) * s_c
  P.qc[0] = sim3[0]; P.qc[1] = -sim3[1]; P.qc[2] = -sim3[2]; P.qc[3] = -sim3[3];
  P.sc = 1.0 / sim3[7];
  double r[3];
  lc_rotate(P.qc, sim3 + 4, r);
  for (int a = 0; a < 3; ++a) P.tc[a] = -r[a] * P.sc;
  return ORBX_OK;
}

// The call on the handle's stream.  Every output is device memory.
int lc_enqueue(orbx_handle* h, const char* who, const orbx_loop_correct_config* cfg, orbx_map_points* mp, const LcPlan& P, orbx_keyframe* const* kfs, const int* parent,
               int cur, int loop, int n_matches, const int* d_matches, int* d_counts, uint8_t* d_affected, double* d_poses_wc, int* d_list_slot, int* d_goner, int* d_keeper) {
  const size_t N = P.kfs.size(), M = (size_t)n_matches;
  if (!d_counts || !d_affected || !d_poses_wc || (P.bound > 0 && !d_list_slot) || (M > 0 && (!d_matches || !d_goner || !d_keeper)))
    return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  ORBX_HIP(h, hipSetDevice(h->device));
  const int n_chunk = std::max(1, (P.max_n + LC_CHUNK - 1) / LC_CHUNK);
  const size_t need = 4 * (size_t)mp->capacity;
  if (mp->first.bytes < need) {                                             // the one fill of the first-sighting table: calls leave it EMPTY
    if (int rc = orbx_reserve(h, mp->first, need)) return rc;
    ORBX_HIP(h, hipMemsetAsync(mp->first.p, LC_EMPTY & 0xff, mp->first.bytes, h->stream));
  }
  Carve ws;
  const size_t o_we = ws.take(4 * N * N), o_ca = ws.take(4 * N * (size_t)n_chunk * LC_CHUNK), o_cc = ws.take(4 * N * (size_t)n_chunk), o_pa = ws.take(8 * M),
               o_la = ws.take(8 * M), o_re = ws.take(8 * M), o_tg = ws.take(4 * M), o_tk = ws.take(4 * M);
  const size_t o_zero = ws.off;                                             // zeroed before every call: observer counts, keys, sizes, changed, cursor
  const size_t o_no = ws.take(8 * M), o_ke = ws.take(16 * M), o_cs = ws.take(8 * M), o_ch = ws.take(4 * N), o_cu = ws.take(4);
  if (int rc = orbx_reserve(h, h->ws_map.loop_scratch, ws.off)) return rc;
  uint8_t* w = (uint8_t*)h->ws_map.loop_scratch.p;
  UploadPlan up;
  const size_t u_kf = up.put(P.kfs.data(), sizeof(LcKf) * N), u_pa = up.put(parent, 4 * N), u_po = up.put(P.poses.data(), 56 * N);
  if (int rc = up.send(h, h->ring_map, h->ws_map.loop_tables)) return rc;
  uint8_t* const ds = up.device;
  // the weights, every keyframe a query; they never leave the device
  std::vector<int> query(std::min<size_t>(N, LC_Q_BATCH));
  for (size_t q0 = 0; q0 < N; q0 += LC_Q_BATCH) {
    const size_t nq = std::min<size_t>(LC_Q_BATCH, N - q0);
    for (size_t q = 0; q < nq; ++q) query[q] = (int)(q0 + q);
    if (int rc = orbx_map_covisibility_device(h, mp, (int)N, kfs, (int)nq, query.data(), 0, (int*)(w + o_we) + q0 * N, nullptr, nullptr)) return rc;
  }
  ORBX_HIP(h, hipMemsetAsync(w + o_zero, 0, ws.off - o_zero, h->stream));
  LcArgs A{};
  A.capacity = mp->capacity; A.n_kfs = (int)N; A.n_chunk = n_chunk; A.cur = cur; A.loop = loop; A.n_matches = n_matches;
  A.min_weight = cfg->min_covisibility_weight; A.max_depth = cfg->max_propagation_depth;
  std::copy(P.qc, P.qc + 4, A.qc); std::copy(P.tc, P.tc + 3, A.tc); A.sc = P.sc;
  A.live = mp->d_live; A.pos = mp->d_pos;
  A.kfs = (const LcKf*)(ds + u_kf); A.parent = (const int*)(ds + u_pa); A.poses_in = (const double*)(ds + u_po);
  A.weights = (const int*)(w + o_we); A.matches = d_matches; A.index = (int*)mp->first.p;
  A.cand = (int*)(w + o_ca); A.chunk_count = (int*)(w + o_cc); A.pair = (int*)(w + o_pa); A.label = (int*)(w + o_la); A.repl = (int*)(w + o_re);
  A.nobs = (int*)(w + o_no); A.key = (unsigned long long*)(w + o_ke); A.csize = (int*)(w + o_cs); A.changed = (int*)(w + o_ch); A.cursor = (int*)(w + o_cu);
  A.tmp_goner = (int*)(w + o_tg); A.tmp_keeper = (int*)(w + o_tk);
  A.counts = d_counts; A.affected = d_affected; A.poses_out = d_poses_wc; A.list_slot = d_list_slot; A.goner = d_goner; A.keeper = d_keeper;
  const dim3 block(LC_THREADS), kf_grid(n_chunk, (unsigned)N), fine_grid(std::max(1, (P.max_n + LC_THREADS - 1) / LC_THREADS), (unsigned)N),
      node_grid((unsigned)((2 * M + LC_THREADS - 1) / LC_THREADS)), match_grid((unsigned)((M + LC_THREADS - 1) / LC_THREADS));
  orbx_launch(h, "lc_reach_kernel", true, lc_reach_kernel, dim3(1), dim3(LC_ONE_THREADS), 0, A);
  if (P.bound > 0) {
    orbx_launch(h, "lc_mark_kernel", true, lc_mark_kernel, kf_grid, block, 0, A);
    orbx_launch(h, "lc_flag_kernel", true, lc_flag_kernel, kf_grid, block, 0, A);
    orbx_launch(h, "lc_emit_kernel", true, lc_emit_kernel, kf_grid, block, 0, A);
  }
  orbx_launch(h, "lc_correct_kernel", true, lc_correct_kernel, dim3((unsigned)((std::max(N, (size_t)P.bound) + LC_THREADS - 1) / LC_THREADS)), block, 0, A);
  if (M > 0) {
    orbx_launch(h, "lc_pair_kernel", true, lc_pair_kernel, match_grid, block, 0, A);
    orbx_launch(h, "lc_nobs_kernel", true, lc_nobs_kernel, kf_grid, block, 0, A);
    orbx_launch(h, "lc_class_kernel", true, lc_class_kernel, dim3(1), dim3(LC_ONE_THREADS), 0, A);
    orbx_launch(h, "lc_key_kernel", true, lc_key_kernel, node_grid, block, 0, A);
    orbx_launch(h, "lc_goner_kernel", true, lc_goner_kernel, node_grid, block, 0, A);
    orbx_launch(h, "lc_goner_rank_kernel", true, lc_goner_rank_kernel, match_grid, block, 0, A);
    orbx_launch(h, "lc_rewrite_kernel", true, lc_rewrite_kernel, kf_grid, block, 0, A);
    orbx_launch(h, "lc_uniq_kernel", true, lc_uniq_kernel, fine_grid, block, 0, A);
    orbx_launch(h, "lc_restore_kernel", true, lc_restore_kernel, node_grid, block, 0, A);
  }
  ORBX_HIP(h, hipGetLastError());
  return ORBX_OK;
}

// The host form behind its checks: one download of the counts, affected bytes, poses, list and goner lists; the poses applied as
// orbx_keyframe_set_pose does; the goners erased as orbx_map_points_erase does.
int lc_host(orbx_handle* h, const char* who, const orbx_loop_correct_config* cfg, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, const int* parent, int cur,
            int loop, const double* sim3, int n_matches, const int* matches, int list_cap, int* counts, uint8_t* affected, double* poses_wc, int* list_slot, int* goner,
            int* keeper) {
  if (n_matches > 0 && !matches) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  LcPlan P;
  if (int rc = lc_plan(h, who, cfg, mp, n_kfs, kfs, parent, cur, loop, sim3, n_matches, matches, list_cap, P)) return rc;
  const size_t N = (size_t)n_kfs, M = (size_t)n_matches;
  if (!counts || !affected || !poses_wc || (P.bound > 0 && !list_slot) || (M > 0 && (!goner || !keeper))) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument", who);
  ORBX_HIP(h, hipSetDevice(h->device));
  OutputPlan out;
  const auto p_cn = out.add(counts, 4), p_go = out.add(goner, M, true), p_ke = out.add(keeper, M, true), p_ls = out.add(list_slot, (size_t)P.bound, true);
  const auto p_po = out.add(poses_wc, 7 * N);
  const auto p_af = out.add(affected, N);
  const size_t in_bytes = (8 * M + 255) & ~(size_t)255;
  if (int rc = out.begin(h, h->pin_map, h->ws_map.host_blobs, in_bytes)) return rc;
  if (M > 0) {
    std::memcpy(out.call.hi, matches, 8 * M);
    if (int rc = orbx_host_call_upload(h, out.call)) return rc;
  }
  if (int rc = lc_enqueue(h, who, cfg, mp, P, kfs, parent, cur, loop, n_matches, M > 0 ? (const int*)out.call.di : nullptr, out.dev(p_cn), out.dev(p_af), out.dev(p_po),
                          out.dev(p_ls), out.dev(p_go), out.dev(p_ke)))
    return rc;
  if (int rc = out.finish(h)) return rc;
  const size_t G = (size_t)counts[3];
  for (int rc : {out.copy(h, p_ls, (size_t)counts[1]), out.copy(h, p_go, G), out.copy(h, p_ke, G)})
    if (rc) return rc;
  for (size_t k = 0; k < N; ++k)
    if (affected[k]) orbx_keyframe_set_pose(kfs[k], poses_wc + 7 * k);
  return G ? orbx_map_points_erase(mp, goner, (int)G) : (int)ORBX_OK;
}

}  // namespace

extern "C" {

void orbx_default_loop_correct_config(orbx_loop_correct_config* cfg) {
  if (!cfg) return;
  cfg->min_covisibility_weight = 15;                                        // corrector.rs:97-104
  cfg->max_propagation_depth = 100;
}

int orbx_map_loop_max_keyframes(void) { return LC_MAX_KFS; }

int orbx_map_correct_loop_device(orbx_handle* h, const orbx_loop_correct_config* cfg, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, const int* parent, int cur,
                                 int loop, const double* sim3, int n_matches, const int* d_feature_matches, int list_cap, int* d_counts, uint8_t* d_affected,
                                 double* d_poses_wc, int* d_list_slot, int* d_goner, int* d_keeper) {
  static const char* who = "orbx_map_correct_loop_device";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (n_kfs == 0 && mp && mp->h == h) return ORBX_OK;
    LcPlan P;
    if (int rc = lc_plan(h, who, cfg, mp, n_kfs, kfs, parent, cur, loop, sim3, n_matches, nullptr, list_cap, P)) return rc;
    return lc_enqueue(h, who, cfg, mp, P, kfs, parent, cur, loop, n_matches, d_feature_matches, d_counts, d_affected, d_poses_wc, d_list_slot, d_goner, d_keeper);
  });
}

int orbx_map_correct_loop(orbx_handle* h, const orbx_loop_correct_config* cfg, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, const int* parent, int cur, int loop,
                          const double* sim3, int n_matches, const int* feature_matches, int list_cap, int* counts, uint8_t* affected, double* poses_wc, int* list_slot,
                          int* goner, int* keeper) {
  static const char* who = "orbx_map_correct_loop";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (n_kfs == 0 && mp && mp->h == h) return ORBX_OK;
    return lc_host(h, who, cfg, mp, n_kfs, kfs, parent, cur, loop, sim3, n_matches, feature_matches, list_cap, counts, affected, poses_wc, list_slot, goner, keeper);
  });
}

int orbx_map_close_loop(orbx_handle* h, const orbx_camera* cam, const orbx_loop_correct_config* correct_cfg, const orbx_ba_config* ba_cfg, orbx_map_points* mp, int n_kfs,
                        orbx_keyframe* const* kfs, const int* parent, int cur, int loop, const double* sim3, int n_matches, const int* feature_matches, int list_cap,
                        int* counts, uint8_t* affected, double* poses_wc, int* list_slot, int* goner, int* keeper, orbx_should_stop_fn should_stop, void* user,
                        double* poses_wc_out, int* ba_counts, int* iterations, double* initial_error, double* final_error) {
  static const char* who = "orbx_map_close_loop";
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, who, [&]() -> int {
    if (ba_cfg && !cam) return orbx_fail(h, ORBX_ERR_INVALID, "%s: bad argument (global BA needs the camera)", who);
    if (n_kfs == 0 && mp && mp->h == h) return ORBX_OK;
    if (int rc = lc_host(h, who, correct_cfg, mp, n_kfs, kfs, parent, cur, loop, sim3, n_matches, feature_matches, list_cap, counts, affected, poses_wc, list_slot, goner,
                         keeper))
      return rc;
    if (!ba_cfg) return ORBX_OK;
    return orbx_map_global_ba(h, cam, ba_cfg, mp, n_kfs, kfs, should_stop, user, poses_wc_out, ba_counts, iterations, initial_error, final_error);
  });
}

}  // extern "C"
