// kfdb_kernels.hip — orbx_kfdb: the keyframe BoW database of place recognition with its BowVectors in device memory, scored against one
// query or a batch of queries in one launch, and the reference's two searches over it:
//   KeyFrameDatabase::{add, erase, detect_candidates}     src/atlas/keyframe_db.rs:36-95   (relocalisation, all maps)
//   detect_loop_candidates                                 src/loop_closing/detector.rs:185-368 (called per keyframe by LoopCloser)
//
// Storage (grow-only, on the handle's device): one byte arena holding per entry its word ids (u32, ascending) and, behind them, its
// weights (f64); a table of (id, arena offset, n, map, flags) per slot.  erase / replace leave a tombstone (flags = 0); the arena and the
// table are compacted by a synchronous call when more than half of the slots are dead.  Nothing moves per query.
//
// Scores are the serial sums of orbx_bow_score (bow_kernels.hip) and of the dot product of keyframe_db.rs:73-79: term after term in
// ascending word id over the union, one f64 add chain per pair.  What runs in parallel is the pairs: kfdb_score_kernel stages a query in
// LDS once per workgroup and every lane walks the merge of its own entry against it, the entry streamed from global memory in 16-byte
// pieces fetched one piece ahead of use (the entry pointer only moves forward).
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "orbx_internal.hpp"

namespace {

constexpr int KFDB_MAX_WORDS = 8192;            // words of one BowVector (= BOWV_MAX of bow_kernels.hip)
constexpr int KFDB_THREADS = 256;
constexpr unsigned KFDB_LIVE = 1u, KFDB_BAD = 2u;
constexpr unsigned long long KFDB_END = 1ull << 32;   // past every u32 word id

struct KfdbEntry {                              // one slot of the device table
  unsigned long long id;
  unsigned long long off;                       // byte offset of the words inside the arena (multiple of 32); weights at off + pad32(4 n)
  int n;
  int map;
  unsigned flags;                               // KFDB_LIVE | KFDB_BAD; 0 = tombstone
  int pad_;
};
struct KfdbQuery {                              // one query of a scoring / search launch
  unsigned long long w_off, v_off;              // slot < 0: byte offsets of the query's words / weights inside the query blob
  int n;
  int slot;                                     // >= 0: the query is this entry of the database
  unsigned long long cur_id;                    // loop search: the current keyframe
  int map;                                      // loop search: its map
  int n_thr, thr_off;                           // loop search: slots scored for the threshold, in the caller's order
  int conn_n, conn_off;                         // loop search: the query's connected ids, sorted ascending
};
struct KfdbCand { unsigned long long id; double score; };

__host__ __device__ inline size_t pad32(size_t x) { return (x + 31) & ~(size_t)31; }

// ---- table / arena maintenance --------------------------------------------------------------------------------------------------
__global__ void kfdb_set_entry_kernel(KfdbEntry* table, int slot, KfdbEntry e) { table[slot] = e; }
__global__ void kfdb_set_flags_kernel(KfdbEntry* table, int slot, unsigned flags) { table[slot].flags = flags; }

// add_device: the entry's size is a device value.  n = clamp(*d_count, 0, max_n); the words / weights are copied into the slot's
// reservation (sized for max_n) and the table row written, all without the host seeing n.
__global__ __launch_bounds__(KFDB_THREADS) void kfdb_add_device_kernel(KfdbEntry* table, int slot, KfdbEntry e, uint8_t* arena,
                                                                       const uint32_t* __restrict__ word, const double* __restrict__ weight,
                                                                       const int* __restrict__ d_count, int max_n) {
  int n = *d_count;
  n = n < 0 ? 0 : (n > max_n ? max_n : n);
  uint32_t* w = reinterpret_cast<uint32_t*>(arena + e.off);
  double* v = reinterpret_cast<double*>(arena + e.off + pad32(4 * (size_t)n));
  for (int i = threadIdx.x; i < n; i += KFDB_THREADS) { w[i] = word[i]; v[i] = weight[i]; }
  if (threadIdx.x == 0) { e.n = n; table[slot] = e; }
}

// compaction: new slot s takes old slot src[s]; one workgroup per entry copies its words and weights
__global__ __launch_bounds__(KFDB_THREADS) void kfdb_compact_kernel(const KfdbEntry* __restrict__ old_table, const uint8_t* __restrict__ old_arena,
                                                                    const int* __restrict__ src, KfdbEntry* __restrict__ table,
                                                                    uint8_t* __restrict__ arena) {
  const int s = blockIdx.x;
  const KfdbEntry o = old_table[src[s]], e = table[s];
  const uint32_t* ow = reinterpret_cast<const uint32_t*>(old_arena + o.off);
  const double* ov = reinterpret_cast<const double*>(old_arena + o.off + pad32(4 * (size_t)o.n));
  uint32_t* w = reinterpret_cast<uint32_t*>(arena + e.off);
  double* v = reinterpret_cast<double*>(arena + e.off + pad32(4 * (size_t)e.n));
  for (int i = threadIdx.x; i < e.n; i += KFDB_THREADS) { w[i] = ow[i]; v[i] = ov[i]; }
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------------
// One pair: the merge of the LDS query (s_qw / s_qv, nq) with one entry (ew / ev, ne) in ascending word id over the union.
// DOT = false: OrbVocabulary::score (vocabulary/mod.rs:357-374) exactly as orbx_bow_score adds it; DOT = true: keyframe_db.rs:73-79.
// The query is read two elements ahead of the merge position and the entry one 16-byte piece ahead, so neither the LDS nor the
// global latency sits between two terms of the add chain.
template <bool DOT>
__device__ __forceinline__ double kfdb_pair(const uint32_t* s_qw, const double* s_qv, int nq, const uint32_t* __restrict__ ew,
                                            const double* __restrict__ ev, int ne) {
  int a = 0, b = 0;
  unsigned long long ka0 = nq > 0 ? s_qw[0] : KFDB_END, ka1 = nq > 1 ? s_qw[1] : KFDB_END;
  double va0 = nq > 0 ? s_qv[0] : 0.0, va1 = nq > 1 ? s_qv[1] : 0.0;
  // the current piece is a queue: its head (w0, v0) is element b, an advance shifts it down (an element picked by index b & 3 would
  // put the piece in scratch memory); the next piece waits in nw / nv
  unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  uint4 nw = make_uint4(0, 0, 0, 0);
  double2 nv0 = make_double2(0.0, 0.0), nv1 = nv0;
  if (ne > 0) {
    const uint4 c = *reinterpret_cast<const uint4*>(ew);
    const double2 c0 = *reinterpret_cast<const double2*>(ev), c1 = *reinterpret_cast<const double2*>(ev + 2);
    w0 = c.x; w1 = c.y; w2 = c.z; w3 = c.w; v0 = c0.x; v1 = c0.y; v2 = c1.x; v3 = c1.y;
  }
  if (ne > 4) { nw = *reinterpret_cast<const uint4*>(ew + 4); nv0 = *reinterpret_cast<const double2*>(ev + 4); nv1 = *reinterpret_cast<const double2*>(ev + 6); }
  double acc = 0.0;
  while (a < nq || b < ne) {
    const unsigned long long kb = b < ne ? (unsigned long long)w0 : KFDB_END;
    const double vb = v0;
    const bool only_a = ka0 < kb, only_b = kb < ka0;
    if (DOT) {
      if (!only_a && !only_b) acc += va0 * vb;                        // product, then add (-ffp-contract=off)
    } else {
      const double x = only_a ? va0 - 0.0 : (only_b ? vb : va0 - vb);  // (w1 - 0.0).abs(), w2.abs(), (w1 - w2).abs()
      acc += fabs(x);
    }
    if (!only_b) {
      ++a;
      ka0 = ka1; va0 = va1;
      const bool more = a + 1 < nq;
      ka1 = more ? (unsigned long long)s_qw[more ? a + 1 : 0] : KFDB_END;
      va1 = s_qv[more ? a + 1 : 0];
    }
    if (!only_a) {
      ++b;
      if ((b & 3) != 0) {
        w0 = w1; w1 = w2; w2 = w3; v0 = v1; v1 = v2; v2 = v3;
      } else {
        w0 = nw.x; w1 = nw.y; w2 = nw.z; w3 = nw.w; v0 = nv0.x; v1 = nv0.y; v2 = nv1.x; v3 = nv1.y;
        if (b + 4 < ne) {
          nw = *reinterpret_cast<const uint4*>(ew + b + 4);
          nv0 = *reinterpret_cast<const double2*>(ev + b + 4); nv1 = *reinterpret_cast<const double2*>(ev + b + 6);
        }
      }
    }
  }
  return DOT ? acc : 1.0 - 0.5 * acc;
}

// grid (ceil(n_slots / 256), Q): workgroup (x, q) stages query q in LDS, lane t scores slot 256 x + t.  scores [Q][n_slots]; a tombstone
// gets 0 (never read).
template <bool DOT>
__global__ __launch_bounds__(KFDB_THREADS) void kfdb_score_kernel(const KfdbEntry* __restrict__ table, const uint8_t* __restrict__ arena, int n_slots,
                                                                  const KfdbQuery* __restrict__ queries, const uint8_t* __restrict__ qblob,
                                                                  int lds_words, double* __restrict__ scores) {
  extern __shared__ double s_mem[];
  double* s_qv = s_mem;                                              // [lds_words]
  uint32_t* s_qw = reinterpret_cast<uint32_t*>(s_mem + lds_words);   // [lds_words]
  const KfdbQuery q = queries[blockIdx.y];
  const uint32_t* qw; const double* qv; int nq;
  if (q.slot >= 0) {
    const KfdbEntry e = table[q.slot];
    qw = reinterpret_cast<const uint32_t*>(arena + e.off);
    qv = reinterpret_cast<const double*>(arena + e.off + pad32(4 * (size_t)e.n));
    nq = e.n;
  } else {
    qw = reinterpret_cast<const uint32_t*>(qblob + q.w_off); qv = reinterpret_cast<const double*>(qblob + q.v_off); nq = q.n;
  }
  nq = nq < lds_words ? nq : lds_words;                              // (the host sized the LDS for the largest query: never taken)
  for (int i = threadIdx.x; i < nq; i += KFDB_THREADS) { s_qw[i] = qw[i]; s_qv[i] = qv[i]; }
  if (nq == 0 && threadIdx.x == 0) { s_qw[0] = 0; s_qv[0] = 0.0; }   // the look-ahead reads element 0 of an empty query
  __syncthreads();
  const int s = blockIdx.x * KFDB_THREADS + threadIdx.x;
  if (s >= n_slots) return;
  const KfdbEntry e = table[s];
  double r = 0.0;
  if (e.flags & KFDB_LIVE)
    r = kfdb_pair<DOT>(s_qw, s_qv, nq, reinterpret_cast<const uint32_t*>(arena + e.off),
                       reinterpret_cast<const double*>(arena + e.off + pad32(4 * (size_t)e.n)), e.n);
  scores[(size_t)blockIdx.y * n_slots + s] = r;
}

// ---- filtering --------------------------------------------------------------------------------------------------------------------
// grid (ceil(n_slots / 256), Q).  mode 0: find_candidates_above_threshold (detector.rs:301-358) under the threshold of
// compute_min_score (:265-298) — the query's own map, not connected, |id - current| >= gap, not bad, score >= threshold; mode 1:
// KeyFrameDatabase::detect_candidates (keyframe_db.rs:66-88) — not of exclude_map, score > 0.  Survivors are appended per wave (ballot,
// one atomic per wave) to cand [Q][n_slots] in no particular order; the host orders them.
__global__ __launch_bounds__(KFDB_THREADS) void kfdb_filter_kernel(const KfdbEntry* __restrict__ table, int n_slots, const KfdbQuery* __restrict__ queries,
                                                                   const int* __restrict__ thr_slots, const unsigned long long* __restrict__ conn,
                                                                   const double* __restrict__ scores, int mode, double min_score_ratio,
                                                                   int min_covisibles, unsigned long long min_gap, int exclude_map,
                                                                   KfdbCand* __restrict__ cand, int* __restrict__ counts) {
  __shared__ double s_thr;
  const KfdbQuery q = queries[blockIdx.y];
  const double* sc = scores + (size_t)blockIdx.y * n_slots;
  if (mode == 0) {
    if (threadIdx.x == 0) {
      double best = 0.0;                                             // :272
      for (int i = 0; i < q.n_thr; ++i) { const double v = sc[thr_slots[q.thr_off + i]]; if (v > best) best = v; }   // :283-286
      s_thr = q.n_thr < min_covisibles ? 0.0 : best * min_score_ratio;   // :292-297
    }
    __syncthreads();
    if (s_thr < 0.01) return;                                        // :212-215
  }
  const double thr = mode == 0 ? s_thr : 0.0;
  const int s = blockIdx.x * KFDB_THREADS + threadIdx.x;
  bool keep = false;
  KfdbCand c{0, 0.0};
  if (s < n_slots) {
    const KfdbEntry e = table[s];
    c.id = e.id; c.score = sc[s];
    if (e.flags & KFDB_LIVE) {
      if (mode == 0) {
        const unsigned long long gap = q.cur_id > e.id ? q.cur_id - e.id : e.id - q.cur_id;                          // :323-327
        keep = e.map == q.map && gap >= min_gap && !(e.flags & KFDB_BAD) && c.score >= thr;                          // :329-347
        if (keep) {                                                  // :318 connected_kfs.contains
          int lo = 0, hi = q.conn_n;
          const unsigned long long* cn = conn + q.conn_off;
          while (lo < hi) { const int mid = (lo + hi) >> 1; if (cn[mid] < e.id) lo = mid + 1; else hi = mid; }
          if (lo < q.conn_n && cn[lo] == e.id) keep = false;
        }
      } else {
        keep = (exclude_map < 0 || e.map != exclude_map) && c.score > 0.0;                                           // keyframe_db.rs:67-81
      }
    }
  }
  const unsigned long long m = __ballot(keep);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(&counts[blockIdx.y], __popcll(m));
  base = __shfl(base, 0);
  if (keep) cand[(size_t)blockIdx.y * n_slots + base + __popcll(m & ((1ull << lane) - 1ull))] = c;
}

struct HostEntry {
  unsigned long long id = 0, off = 0;
  size_t reserved = 0;        // bytes of the arena this slot owns
  int n = 0;                  // -1: a device value (add_device) the host has not seen
  int cap = 0;                // upper bound of n
  int map = 0;
  unsigned flags = 0;
};

}  // namespace

struct orbx_kfdb {
  orbx_handle* h = nullptr;
  std::vector<HostEntry> slots;
  std::unordered_map<unsigned long long, int> slot_of;   // live entries
  int n_dead = 0;
  uint8_t* d_arena = nullptr; size_t arena_bytes = 0, arena_used = 0;
  KfdbEntry* d_table = nullptr; size_t table_cap = 0;
  std::vector<void*> retired;   // arenas / tables replaced by a larger one: freed by the next synchronous call (hipFree synchronises)
  DevBuf ws_q, ws_scores, ws_cand;
  bool lds_attr[2] = {false, false};
};

namespace {

void kfdb_free_retired(orbx_kfdb* db) {
  for (void* p : db->retired) hipFree(p);
  db->retired.clear();
}

// room for one more slot and `bytes` more of arena; growth copies on the stream and retires the old allocation
int kfdb_grow(orbx_kfdb* db, size_t bytes) {
  orbx_handle* h = db->h;
  if (db->slots.size() + 1 > db->table_cap) {
    const size_t cap = std::max<size_t>(1024, 2 * db->table_cap);
    KfdbEntry* t = nullptr;
    ORBX_HIP(h, hipMalloc((void**)&t, sizeof(KfdbEntry) * cap));
    if (db->d_table) {
      ORBX_HIP(h, hipMemcpyAsync(t, db->d_table, sizeof(KfdbEntry) * db->slots.size(), hipMemcpyDeviceToDevice, h->stream));
      db->retired.push_back(db->d_table);
    }
    db->d_table = t; db->table_cap = cap;
  }
  if (db->arena_used + bytes + 64 > db->arena_bytes) {
    const size_t cap = std::max<size_t>((size_t)4 << 20, std::max(2 * db->arena_bytes, db->arena_used + bytes + 64));
    uint8_t* a = nullptr;
    ORBX_HIP(h, hipMalloc((void**)&a, cap));
    if (db->d_arena) {
      if (db->arena_used) ORBX_HIP(h, hipMemcpyAsync(a, db->d_arena, db->arena_used, hipMemcpyDeviceToDevice, h->stream));
      db->retired.push_back(db->d_arena);
    }
    db->d_arena = a; db->arena_bytes = cap;
  }
  return ORBX_OK;
}

void kfdb_tombstone(orbx_kfdb* db, int slot) {
  db->slots[(size_t)slot].flags = 0;
  db->slot_of.erase(db->slots[(size_t)slot].id);
  ++db->n_dead;
  hipLaunchKernelGGL(kfdb_set_flags_kernel, dim3(1), dim3(1), 0, db->h->stream, db->d_table, slot, 0u);
}

bool ascending(const uint32_t* w, int n) {
  for (int i = 1; i < n; ++i) if (w[i] <= w[i - 1]) return false;
  return true;
}

// Synchronous.  Live slots move to the front in slot order, every entry shrinks to its real size (the device-given sizes are read back).
int kfdb_compact(orbx_kfdb* db) {
  orbx_handle* h = db->h;
  ORBX_HIP(h, hipSetDevice(h->device));
  ORBX_HIP(h, hipStreamSynchronize(h->stream));
  kfdb_free_retired(db);
  if (db->n_dead == 0) return ORBX_OK;
  std::vector<KfdbEntry> old(db->slots.size());
  if (!old.empty()) ORBX_HIP(h, hipMemcpy(old.data(), db->d_table, sizeof(KfdbEntry) * old.size(), hipMemcpyDeviceToHost));
  std::vector<HostEntry> slots;
  std::vector<KfdbEntry> table;
  std::vector<int> src;
  size_t used = 0;
  for (size_t s = 0; s < db->slots.size(); ++s) {
    if (!(db->slots[s].flags & KFDB_LIVE)) continue;
    HostEntry e = db->slots[s];
    e.n = e.cap = old[s].n;
    e.off = used; e.reserved = pad32(4 * (size_t)e.n) + pad32(8 * (size_t)e.n);
    used += e.reserved;
    table.push_back(KfdbEntry{e.id, e.off, e.n, e.map, e.flags, 0});
    src.push_back((int)s);
    slots.push_back(e);
  }
  const size_t n = slots.size();
  const size_t tcap = std::max<size_t>(1024, 2 * n), acap = std::max<size_t>((size_t)4 << 20, 2 * used + 64);
  KfdbEntry* t = nullptr; uint8_t* a = nullptr; int* d_src = nullptr;
  ORBX_HIP(h, hipMalloc((void**)&t, sizeof(KfdbEntry) * tcap));
  if (hipMalloc((void**)&a, acap) != hipSuccess) { hipFree(t); return orbx_fail(h, ORBX_ERR_HIP, "orbx_kfdb: out of device memory"); }
  if (n) {
    if (hipMalloc((void**)&d_src, sizeof(int) * n) != hipSuccess) { hipFree(t); hipFree(a); return orbx_fail(h, ORBX_ERR_HIP, "orbx_kfdb: out of device memory"); }
    hipMemcpy(t, table.data(), sizeof(KfdbEntry) * n, hipMemcpyHostToDevice);
    hipMemcpy(d_src, src.data(), sizeof(int) * n, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(kfdb_compact_kernel, dim3((unsigned)n), dim3(KFDB_THREADS), 0, h->stream, db->d_table, db->d_arena, d_src, t, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d_src);
    if (e != hipSuccess) { hipFree(t); hipFree(a); return orbx_fail(h, ORBX_ERR_HIP, "orbx_kfdb compaction: %s", hipGetErrorString(e)); }
  }
  hipFree(db->d_table); hipFree(db->d_arena);
  db->d_table = t; db->table_cap = tcap; db->d_arena = a; db->arena_bytes = acap; db->arena_used = used;
  db->slots.swap(slots);
  db->slot_of.clear();
  for (size_t s = 0; s < n; ++s) db->slot_of[db->slots[s].id] = (int)s;
  db->n_dead = 0;
  return ORBX_OK;
}

// what every query call does first: the stream drained of earlier adds' growth copies is not needed (same stream), but retired
// allocations can go, and a database that is mostly tombstones is compacted
int kfdb_before_query(orbx_kfdb* db) {
  if (db->n_dead > 64 && (size_t)db->n_dead > db->slot_of.size()) return kfdb_compact(db);
  return ORBX_OK;
}

struct QueryHost {               // one query as the host prepares it
  int slot = -1;
  const uint32_t* w = nullptr; const double* v = nullptr; int n = 0;
  unsigned long long cur_id = 0; int map = 0;
  std::vector<int> thr_slots;
  std::vector<unsigned long long> conn;   // sorted
  bool skip = false;                      // no device work: zero candidates
};

// scores of Q queries against every slot -> db->ws_scores [Q][n_slots]; with mode >= 0 also the filter -> ws_cand, counts.
// Leaves d_counts (int [Q]) behind the scores.  Asynchronous on the stream; the host vectors it uploads from must outlive the
// caller's synchronisation, so they are kept in `keep`.
struct Launch {
  std::vector<KfdbQuery> q;
  std::vector<int> thr;
  std::vector<unsigned long long> conn;
  std::vector<uint8_t> blob;
  double* d_scores = nullptr; KfdbCand* d_cand = nullptr; int* d_counts = nullptr;
};

int kfdb_launch(orbx_kfdb* db, int scoring, const std::vector<QueryHost>& qs, int mode, const orbx_loop_detector_config* cfg, int exclude_map,
                Launch& L) {
  orbx_handle* h = db->h;
  const int Q = (int)qs.size(), n_slots = (int)db->slots.size();
  int lds_words = 1;
  size_t blob_bytes = 0;
  L.q.resize((size_t)Q);
  for (int i = 0; i < Q; ++i) {
    const QueryHost& s = qs[(size_t)i];
    KfdbQuery& q = L.q[(size_t)i];
    q = KfdbQuery{};
    q.slot = s.slot; q.cur_id = s.cur_id; q.map = s.map;
    if (s.slot >= 0) lds_words = std::max(lds_words, db->slots[(size_t)s.slot].cap);
    else {
      lds_words = std::max(lds_words, s.n);
      q.n = s.n;
      q.w_off = blob_bytes; blob_bytes += pad32(4 * (size_t)s.n);
      q.v_off = blob_bytes; blob_bytes += pad32(8 * (size_t)s.n);
    }
    q.n_thr = (int)s.thr_slots.size(); q.thr_off = (int)L.thr.size();
    L.thr.insert(L.thr.end(), s.thr_slots.begin(), s.thr_slots.end());
    q.conn_n = (int)s.conn.size(); q.conn_off = (int)L.conn.size();
    L.conn.insert(L.conn.end(), s.conn.begin(), s.conn.end());
  }
  L.blob.assign(blob_bytes, 0);
  for (int i = 0; i < Q; ++i) {
    const QueryHost& s = qs[(size_t)i];
    if (s.slot >= 0 || s.n == 0) continue;
    memcpy(L.blob.data() + L.q[(size_t)i].w_off, s.w, 4 * (size_t)s.n);
    memcpy(L.blob.data() + L.q[(size_t)i].v_off, s.v, 8 * (size_t)s.n);
  }
  lds_words = (lds_words + 3) & ~3;
  // query blob: descriptors | threshold slots | connected ids | query vectors
  const size_t o_q = 0, o_thr = pad32(o_q + sizeof(KfdbQuery) * (size_t)Q), o_conn = pad32(o_thr + 4 * L.thr.size()),
               o_blob = pad32(o_conn + 8 * L.conn.size()), q_total = o_blob + blob_bytes + 32;
  if (int rc = orbx_reserve(h, db->ws_q, q_total)) return rc;
  const size_t ns = (size_t)std::max(n_slots, 1);
  if (int rc = orbx_reserve(h, db->ws_scores, 8 * ns * (size_t)Q + 4 * (size_t)Q + 64)) return rc;
  if (mode >= 0) if (int rc = orbx_reserve(h, db->ws_cand, sizeof(KfdbCand) * ns * (size_t)Q)) return rc;
  uint8_t* dq = (uint8_t*)db->ws_q.p;
  L.d_scores = (double*)db->ws_scores.p;
  L.d_counts = (int*)(L.d_scores + ns * (size_t)Q);
  L.d_cand = (KfdbCand*)db->ws_cand.p;
  hipStream_t st = h->stream;
  ORBX_HIP(h, hipMemcpyAsync(dq + o_q, L.q.data(), sizeof(KfdbQuery) * (size_t)Q, hipMemcpyHostToDevice, st));
  if (!L.thr.empty()) ORBX_HIP(h, hipMemcpyAsync(dq + o_thr, L.thr.data(), 4 * L.thr.size(), hipMemcpyHostToDevice, st));
  if (!L.conn.empty()) ORBX_HIP(h, hipMemcpyAsync(dq + o_conn, L.conn.data(), 8 * L.conn.size(), hipMemcpyHostToDevice, st));
  if (blob_bytes) ORBX_HIP(h, hipMemcpyAsync(dq + o_blob, L.blob.data(), blob_bytes, hipMemcpyHostToDevice, st));
  ORBX_HIP(h, hipMemsetAsync(L.d_counts, 0, 4 * (size_t)Q, st));
  if (n_slots == 0) return ORBX_OK;
  const size_t lds = 12 * (size_t)lds_words;
  const bool dot = scoring == ORBX_KFDB_SCORE_DOT;
  if (lds > 48 * 1024 && !db->lds_attr[dot]) {
    ORBX_HIP(h, hipFuncSetAttribute(dot ? (const void*)kfdb_score_kernel<true> : (const void*)kfdb_score_kernel<false>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 12 * KFDB_MAX_WORDS));
    db->lds_attr[dot] = true;
  }
  const dim3 grid((unsigned)((n_slots + KFDB_THREADS - 1) / KFDB_THREADS), (unsigned)Q);
  orbx_launch(h, "kfdb_score_kernel", false, dot ? kfdb_score_kernel<true> : kfdb_score_kernel<false>, grid, dim3(KFDB_THREADS), lds, db->d_table, db->d_arena, n_slots,
              (const KfdbQuery*)(dq + o_q), dq + o_blob, lds_words, L.d_scores);
  ORBX_HIP(h, hipGetLastError());
  if (mode >= 0) {
    orbx_launch(h, "kfdb_filter_kernel", false, kfdb_filter_kernel, grid, dim3(KFDB_THREADS), 0, db->d_table, n_slots, (const KfdbQuery*)(dq + o_q), (const int*)(dq + o_thr),
                (const unsigned long long*)(dq + o_conn), L.d_scores, mode, cfg ? cfg->min_score_ratio : 0.0, cfg ? cfg->min_covisibles_for_threshold : 0,
                cfg ? (unsigned long long)cfg->min_temporal_gap : 0ull, exclude_map, L.d_cand, L.d_counts);
    ORBX_HIP(h, hipGetLastError());
  }
  return ORBX_OK;
}

// the survivors of query qi, ordered: score descending, then (SPEC CHOICE: the reference's stable sort leaves equal scores in HashMap
// order) keyframe id ascending
int kfdb_fetch_sorted(orbx_kfdb* db, const Launch& L, int qi, int count, std::vector<KfdbCand>& out) {
  orbx_handle* h = db->h;
  out.resize((size_t)count);
  if (count) ORBX_HIP(h, hipMemcpy(out.data(), L.d_cand + (size_t)qi * db->slots.size(), sizeof(KfdbCand) * (size_t)count, hipMemcpyDeviceToHost));
  std::sort(out.begin(), out.end(), [](const KfdbCand& a, const KfdbCand& b) { return a.score > b.score || (a.score == b.score && a.id < b.id); });
  return ORBX_OK;
}

bool cfg_ok(const orbx_loop_detector_config* c) {
  return c && c->consistency_threshold >= 0 && c->min_covisibles_for_threshold >= 0 && c->max_covisibles_to_check >= 0 && c->min_temporal_gap >= 0 &&
         !std::isnan(c->min_score_ratio);
}

}  // namespace

extern "C" {

void orbx_default_loop_detector_config(orbx_loop_detector_config* cfg) {
  if (!cfg) return;
  cfg->min_score_ratio = 0.75;                 // detector.rs:36-46
  cfg->consistency_threshold = 3;
  cfg->min_covisibles_for_threshold = 5;
  cfg->max_covisibles_to_check = 10;
  cfg->min_temporal_gap = 30;
}

int orbx_kfdb_create(orbx_handle* h, orbx_kfdb** out) {
  if (!h) return ORBX_ERR_INVALID;
  return orbx_guard(h, "orbx_kfdb_create", [&]() -> int {
    if (!out) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_create: bad argument");
    orbx_kfdb* db = new orbx_kfdb();
    db->h = h;
    *out = db;
    return ORBX_OK;
  });
}

void orbx_kfdb_destroy(orbx_kfdb* db) {
  if (!db) return;
  hipSetDevice(db->h->device);
  hipStreamSynchronize(db->h->stream);
  kfdb_free_retired(db);
  hipFree(db->d_arena); hipFree(db->d_table); hipFree(db->ws_q.p); hipFree(db->ws_scores.p); hipFree(db->ws_cand.p);
  delete db;
}

int orbx_kfdb_add(orbx_kfdb* db, uint64_t keyframe_id, int map_index, int is_bad, const uint32_t* word, const double* weight, int n) {
  if (!db) return ORBX_ERR_INVALID;
  orbx_handle* h = db->h;
  return orbx_guard(h, "orbx_kfdb_add", [&]() -> int {
    if (n < 0 || n > KFDB_MAX_WORDS || map_index < 0 || (n > 0 && (!word || !weight)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_add: bad argument (at most %d words, map index >= 0)", KFDB_MAX_WORDS);
    if (!ascending(word, n)) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_add: word ids must strictly ascend");
    ORBX_HIP(h, hipSetDevice(h->device));
    const size_t bytes = pad32(4 * (size_t)n) + pad32(8 * (size_t)n);
    if (int rc = kfdb_grow(db, bytes)) return rc;
    auto it = db->slot_of.find(keyframe_id);
    if (it != db->slot_of.end()) kfdb_tombstone(db, it->second);        // HashMap::insert replaces (keyframe_db.rs:45-47)
    HostEntry e;
    e.id = keyframe_id; e.off = db->arena_used; e.reserved = bytes; e.n = e.cap = n; e.map = map_index;
    e.flags = KFDB_LIVE | (is_bad ? KFDB_BAD : 0u);
    const int slot = (int)db->slots.size();
    if (n > 0) {
      ORBX_HIP(h, hipMemcpyAsync(db->d_arena + e.off, word, 4 * (size_t)n, hipMemcpyHostToDevice, h->stream));
      ORBX_HIP(h, hipMemcpyAsync(db->d_arena + e.off + pad32(4 * (size_t)n), weight, 8 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    }
    hipLaunchKernelGGL(kfdb_set_entry_kernel, dim3(1), dim3(1), 0, h->stream, db->d_table, slot, KfdbEntry{e.id, e.off, n, map_index, e.flags, 0});
    ORBX_HIP(h, hipGetLastError());
    db->slots.push_back(e); db->slot_of[keyframe_id] = slot; db->arena_used += bytes;
    if (n > 0) ORBX_HIP(h, hipStreamSynchronize(h->stream));            // the caller's buffers are free on return
    return ORBX_OK;
  });
}

int orbx_kfdb_add_device(orbx_kfdb* db, uint64_t keyframe_id, int map_index, int is_bad, const uint32_t* d_word, const double* d_weight,
                         const int* d_count, int max_n) {
  if (!db) return ORBX_ERR_INVALID;
  orbx_handle* h = db->h;
  return orbx_guard(h, "orbx_kfdb_add_device", [&]() -> int {
    if (max_n < 0 || max_n > KFDB_MAX_WORDS || map_index < 0 || !d_count || (max_n > 0 && (!d_word || !d_weight)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_add_device: bad argument (at most %d words, map index >= 0)", KFDB_MAX_WORDS);
    ORBX_HIP(h, hipSetDevice(h->device));
    const size_t bytes = pad32(4 * (size_t)max_n) + pad32(8 * (size_t)max_n);
    if (int rc = kfdb_grow(db, bytes)) return rc;
    auto it = db->slot_of.find(keyframe_id);
    if (it != db->slot_of.end()) kfdb_tombstone(db, it->second);
    HostEntry e;
    e.id = keyframe_id; e.off = db->arena_used; e.reserved = bytes; e.n = -1; e.cap = max_n; e.map = map_index;
    e.flags = KFDB_LIVE | (is_bad ? KFDB_BAD : 0u);
    const int slot = (int)db->slots.size();
    hipLaunchKernelGGL(kfdb_add_device_kernel, dim3(1), dim3(KFDB_THREADS), 0, h->stream, db->d_table, slot, KfdbEntry{e.id, e.off, 0, map_index, e.flags, 0},
                       db->d_arena, d_word, d_weight, d_count, max_n);
    ORBX_HIP(h, hipGetLastError());
    db->slots.push_back(e); db->slot_of[keyframe_id] = slot; db->arena_used += bytes;
    return ORBX_OK;
  });
}

int orbx_kfdb_erase(orbx_kfdb* db, uint64_t keyframe_id) {
  if (!db) return ORBX_ERR_INVALID;
  return orbx_guard(db->h, "orbx_kfdb_erase", [&]() -> int {
    auto it = db->slot_of.find(keyframe_id);
    if (it == db->slot_of.end()) return ORBX_OK;                        // HashMap::remove of an absent key (keyframe_db.rs:50-52)
    orbx_handle* h = db->h;
    ORBX_HIP(h, hipSetDevice(h->device));
    kfdb_tombstone(db, it->second);
    ORBX_HIP(h, hipGetLastError());
    return ORBX_OK;
  });
}

int orbx_kfdb_set_bad(orbx_kfdb* db, uint64_t keyframe_id, int is_bad) {
  if (!db) return ORBX_ERR_INVALID;
  orbx_handle* h = db->h;
  return orbx_guard(h, "orbx_kfdb_set_bad", [&]() -> int {
    auto it = db->slot_of.find(keyframe_id);
    if (it == db->slot_of.end()) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_set_bad: no such keyframe");
    ORBX_HIP(h, hipSetDevice(h->device));
    HostEntry& e = db->slots[(size_t)it->second];
    e.flags = KFDB_LIVE | (is_bad ? KFDB_BAD : 0u);
    hipLaunchKernelGGL(kfdb_set_flags_kernel, dim3(1), dim3(1), 0, h->stream, db->d_table, it->second, e.flags);
    ORBX_HIP(h, hipGetLastError());
    return ORBX_OK;
  });
}

int orbx_kfdb_size(const orbx_kfdb* db, int* n_entries, int* n_slots) {
  if (!db) return ORBX_ERR_INVALID;
  if (n_entries) *n_entries = (int)db->slot_of.size();
  if (n_slots) *n_slots = (int)db->slots.size();
  return ORBX_OK;
}

int orbx_kfdb_compact(orbx_kfdb* db) {
  if (!db) return ORBX_ERR_INVALID;
  return orbx_guard(db->h, "orbx_kfdb_compact", [&] { return kfdb_compact(db); });
}

int orbx_kfdb_download(orbx_kfdb* db, uint64_t keyframe_id, uint32_t* word, double* weight, int cap, int* n, int* map_index, int* is_bad) {
  if (!db) return ORBX_ERR_INVALID;
  orbx_handle* h = db->h;
  return orbx_guard(h, "orbx_kfdb_download", [&]() -> int {
    if (!n || cap < 0) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_download: bad argument");
    auto it = db->slot_of.find(keyframe_id);
    if (it == db->slot_of.end()) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_download: no such keyframe");
    ORBX_HIP(h, hipSetDevice(h->device));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    kfdb_free_retired(db);
    HostEntry& e = db->slots[(size_t)it->second];
    KfdbEntry t;
    ORBX_HIP(h, hipMemcpy(&t, db->d_table + it->second, sizeof(t), hipMemcpyDeviceToHost));
    e.n = t.n;
    *n = t.n;
    if (map_index) *map_index = e.map;
    if (is_bad) *is_bad = (e.flags & KFDB_BAD) ? 1 : 0;
    if (t.n > cap) return orbx_fail(h, ORBX_ERR_CAPACITY, "orbx_kfdb_download: %d words, capacity %d", t.n, cap);
    if (t.n > 0 && (!word || !weight)) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_download: bad argument");
    if (t.n > 0) {
      ORBX_HIP(h, hipMemcpy(word, db->d_arena + t.off, 4 * (size_t)t.n, hipMemcpyDeviceToHost));
      ORBX_HIP(h, hipMemcpy(weight, db->d_arena + t.off + pad32(4 * (size_t)t.n), 8 * (size_t)t.n, hipMemcpyDeviceToHost));
    }
    return ORBX_OK;
  });
}

int orbx_kfdb_score(orbx_kfdb* db, int scoring, const uint32_t* q_word, const double* q_weight, int nq, uint64_t* ids, double* scores, int cap,
                    int* n_out) {
  if (!db) return ORBX_ERR_INVALID;
  orbx_handle* h = db->h;
  return orbx_guard(h, "orbx_kfdb_score", [&]() -> int {
    if ((scoring != ORBX_KFDB_SCORE_L1 && scoring != ORBX_KFDB_SCORE_DOT) || nq < 0 || nq > KFDB_MAX_WORDS || (nq > 0 && (!q_word || !q_weight)) || !n_out ||
        cap < 0 || (cap > 0 && (!ids || !scores)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_score: bad argument");
    if (!ascending(q_word, nq)) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_score: word ids must strictly ascend");
    const int n = (int)db->slot_of.size();
    *n_out = n;
    if (n > cap) return orbx_fail(h, ORBX_ERR_CAPACITY, "orbx_kfdb_score: %d entries, capacity %d", n, cap);
    ORBX_HIP(h, hipSetDevice(h->device));
    if (int rc = kfdb_before_query(db)) return rc;
    std::vector<QueryHost> qs(1);
    qs[0].w = q_word; qs[0].v = q_weight; qs[0].n = nq;
    Launch L;
    if (int rc = kfdb_launch(db, scoring, qs, -1, nullptr, -1, L)) return rc;
    std::vector<double> all(db->slots.size());
    if (!all.empty()) ORBX_HIP(h, hipMemcpyAsync(all.data(), L.d_scores, 8 * all.size(), hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    kfdb_free_retired(db);
    std::vector<std::pair<unsigned long long, int>> order;               // live entries in ascending keyframe id
    order.reserve((size_t)n);
    for (const auto& kv : db->slot_of) order.emplace_back(kv.first, kv.second);
    std::sort(order.begin(), order.end());
    for (int i = 0; i < n; ++i) { ids[i] = order[(size_t)i].first; scores[i] = all[(size_t)order[(size_t)i].second]; }
    return ORBX_OK;
  });
}

int orbx_kfdb_detect_candidates(orbx_kfdb* db, const uint32_t* q_word, const double* q_weight, int nq, int exclude_map, int max_results,
                                uint64_t* ids, int* map_indices, double* scores, int* n_out) {
  if (!db) return ORBX_ERR_INVALID;
  orbx_handle* h = db->h;
  return orbx_guard(h, "orbx_kfdb_detect_candidates", [&]() -> int {
    if (nq < 0 || nq > KFDB_MAX_WORDS || (nq > 0 && (!q_word || !q_weight)) || !n_out || max_results < 0 || (max_results > 0 && (!ids || !scores)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_detect_candidates: bad argument");
    if (!ascending(q_word, nq)) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_detect_candidates: word ids must strictly ascend");
    *n_out = 0;
    ORBX_HIP(h, hipSetDevice(h->device));
    if (int rc = kfdb_before_query(db)) return rc;
    std::vector<QueryHost> qs(1);
    qs[0].w = q_word; qs[0].v = q_weight; qs[0].n = nq;
    Launch L;
    if (int rc = kfdb_launch(db, ORBX_KFDB_SCORE_DOT, qs, 1, nullptr, exclude_map < 0 ? -1 : exclude_map, L)) return rc;
    int count = 0;
    ORBX_HIP(h, hipMemcpyAsync(&count, L.d_counts, 4, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    kfdb_free_retired(db);
    std::vector<KfdbCand> c;
    if (int rc = kfdb_fetch_sorted(db, L, 0, count, c)) return rc;
    const int m = std::min(count, max_results);                          // cands.truncate(max_results), keyframe_db.rs:92
    for (int i = 0; i < m; ++i) {
      ids[i] = c[(size_t)i].id; scores[i] = c[(size_t)i].score;
      if (map_indices) map_indices[i] = db->slots[(size_t)db->slot_of[c[(size_t)i].id]].map;
    }
    *n_out = m;
    return ORBX_OK;
  });
}

int orbx_kfdb_detect_loop_candidates_batch(orbx_kfdb* db, const orbx_loop_detector_config* cfg, int scoring, int n_queries, const uint64_t* current_ids,
                                           const int* connected_offsets, const uint64_t* connected, int cap, uint64_t* ids, double* scores,
                                           int* counts) {
  if (!db) return ORBX_ERR_INVALID;
  orbx_handle* h = db->h;
  return orbx_guard(h, "orbx_kfdb_detect_loop_candidates_batch", [&]() -> int {
    if (!cfg_ok(cfg) || (scoring != ORBX_KFDB_SCORE_L1 && scoring != ORBX_KFDB_SCORE_DOT) || n_queries < 0 || cap < 0 ||
        (n_queries > 0 && (!current_ids || !connected_offsets || !counts)) || (n_queries > 0 && cap > 0 && (!ids || !scores)))
      return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_detect_loop_candidates: bad argument");
    if (n_queries == 0) return ORBX_OK;
    if (connected_offsets[0] != 0) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_detect_loop_candidates: connected_offsets must ascend from 0");
    for (int q = 0; q < n_queries; ++q)
      if (connected_offsets[q + 1] < connected_offsets[q])
        return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_detect_loop_candidates: connected_offsets must ascend from 0");
    if (connected_offsets[n_queries] > 0 && !connected) return orbx_fail(h, ORBX_ERR_INVALID, "orbx_kfdb_detect_loop_candidates: bad argument");
    ORBX_HIP(h, hipSetDevice(h->device));
    if (int rc = kfdb_before_query(db)) return rc;
    // the host's part: which queries exist, and which connected ids the threshold walk scores (detector.rs:276-290, in the given order)
    std::vector<QueryHost> qs;
    std::vector<int> launch_of((size_t)n_queries, -1);
    for (int q = 0; q < n_queries; ++q) {
      counts[q] = 0;
      auto it = db->slot_of.find(current_ids[q]);
      if (it == db->slot_of.end()) continue;                             // :195-198: unknown keyframe -> no candidates
      QueryHost s;
      s.slot = it->second; s.cur_id = current_ids[q]; s.map = db->slots[(size_t)s.slot].map;
      const uint64_t* cn = connected + connected_offsets[q];
      const int nc = connected_offsets[q + 1] - connected_offsets[q];
      for (int i = 0; i < nc && (int)s.thr_slots.size() < cfg->max_covisibles_to_check; ++i) {                          // :277-279
        auto ct = db->slot_of.find(cn[i]);
        if (ct == db->slot_of.end() || db->slots[(size_t)ct->second].map != s.map) continue;                            // :281 map.get_keyframe
        s.thr_slots.push_back(ct->second);
      }
      s.conn.assign(cn, cn + nc);
      std::sort(s.conn.begin(), s.conn.end());
      launch_of[(size_t)q] = (int)qs.size();
      qs.push_back(std::move(s));
    }
    if (qs.empty()) return ORBX_OK;
    Launch L;
    if (int rc = kfdb_launch(db, scoring, qs, 0, cfg, -1, L)) return rc;
    std::vector<int> cnt(qs.size());
    ORBX_HIP(h, hipMemcpyAsync(cnt.data(), L.d_counts, 4 * cnt.size(), hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(h, hipStreamSynchronize(h->stream));
    kfdb_free_retired(db);
    std::vector<KfdbCand> c;
    for (int q = 0; q < n_queries; ++q) {
      const int li = launch_of[(size_t)q];
      if (li < 0) continue;
      if (int rc = kfdb_fetch_sorted(db, L, li, cnt[(size_t)li], c)) return rc;
      counts[q] = cnt[(size_t)li];
      const int m = std::min(cnt[(size_t)li], cap);
      for (int i = 0; i < m; ++i) { ids[(size_t)q * cap + i] = c[(size_t)i].id; scores[(size_t)q * cap + i] = c[(size_t)i].score; }
    }
    return ORBX_OK;
  });
}

int orbx_kfdb_detect_loop_candidates(orbx_kfdb* db, const orbx_loop_detector_config* cfg, int scoring, uint64_t current_id, const uint64_t* connected,
                                     int n_connected, int cap, uint64_t* ids, double* scores, int* count) {
  if (!db) return ORBX_ERR_INVALID;
  if (!count || n_connected < 0) return orbx_fail(db->h, ORBX_ERR_INVALID, "orbx_kfdb_detect_loop_candidates: bad argument");
  const int off[2] = {0, n_connected};
  return orbx_kfdb_detect_loop_candidates_batch(db, cfg, scoring, 1, &current_id, off, connected, cap, ids, scores, count);
}

}  // extern "C"
