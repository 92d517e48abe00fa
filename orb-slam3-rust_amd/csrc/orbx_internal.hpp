// orbx_internal.hpp — shared host-side declarations of the HIP library (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/orbx.h"

#define ORBX_MAX_LEVELS 8

// Persistent host workers of a handle (the batch BA call's per-window preprocessing: creating and joining 16 threads per call cost
// more than the 0.4 ms of work each of them then did).  run(items, want, f) calls f(0..items-1), each index once, on the calling thread
// and up to `want` workers, and returns when all are done; an exception inside f is reported by the return value (false), never thrown
// across the workers.  Not reentrant: one run() at a time per pool (a handle is used by one thread at a time, orbx.h).
class OrbxWorkPool {
 public:
  explicit OrbxWorkPool(int workers) {
    for (int i = 0; i < workers; ++i) th_.emplace_back([this, i] { loop(i); });      // std::system_error if a thread cannot be created
  }
  ~OrbxWorkPool() {
    { std::lock_guard<std::mutex> g(m_); quit_ = true; ++gen_; }
    go_.notify_all();
    for (auto& t : th_) t.join();
  }
  int workers() const { return (int)th_.size(); }
  bool run(int items, int want, const std::function<void(int)>& f) {
    want = want < 0 ? 0 : (want > (int)th_.size() ? (int)th_.size() : want);
    {
      std::lock_guard<std::mutex> g(m_);
      job_ = &f; items_ = items; want_ = want; active_ = want; failed_ = false;
      next_.store(0, std::memory_order_relaxed);
      ++gen_;
    }
    if (want > 0) go_.notify_all();
    take();
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [&] { return active_ == 0; });
    job_ = nullptr;
    return !failed_;
  }

 private:
  void take() {
    try { for (int i; (i = next_.fetch_add(1, std::memory_order_relaxed)) < items_;) (*job_)(i); }
    catch (...) { std::lock_guard<std::mutex> g(m_); failed_ = true; }
  }
  void loop(int idx) {
    unsigned long long seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> g(m_);
        go_.wait(g, [&] { return gen_ != seen; });
        seen = gen_;
        if (quit_) return;
        if (idx >= want_) continue;                                     // this round runs on fewer workers
      }
      take();
      { std::lock_guard<std::mutex> g(m_); if (--active_ == 0) done_.notify_one(); }
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable go_, done_;
  const std::function<void(int)>* job_ = nullptr;
  std::atomic<int> next_{0};
  int items_ = 0, want_ = 0, active_ = 0;
  unsigned long long gen_ = 0;
  bool quit_ = false, failed_ = false;
};

// One persistent helper thread of a handle: start(f) hands it a job and returns, wait() blocks until the job is done.  (The second half of
// a large BA batch runs on it: creating and joining a std::thread per call was 40-70 us of a 3.5 ms call.)  One job at a time.
class OrbxHelperThread {
 public:
  OrbxHelperThread() : th_([this] { loop(); }) {}                          // std::system_error if the thread cannot be created
  ~OrbxHelperThread() {
    { std::lock_guard<std::mutex> g(m_); quit_ = true; }
    cv_.notify_all();
    th_.join();
  }
  void start(std::function<void()> f) {
    { std::lock_guard<std::mutex> g(m_); job_ = std::move(f); busy_ = true; }
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> g(m_);
    cv_.wait(g, [&] { return !busy_; });
  }

 private:
  void loop() {
    for (;;) {
      std::function<void()> f;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return quit_ || (busy_ && job_); });
        if (quit_) return;
        f = std::move(job_); job_ = nullptr;
      }
      try { f(); } catch (...) {}                                        // (the job reports its own errors; nothing may escape a thread)
      { std::lock_guard<std::mutex> g(m_); busy_ = false; }
      cv_.notify_all();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::function<void()> job_;
  bool busy_ = false, quit_ = false;
  std::thread th_;                                                        // last: starts when every other member exists
};

// ---- launch descriptors shared by host code and kernels ------------------------------------------
// Geometry of one pyramid level inside the per-image pyramid / blur slots (identical layout).
struct OrbLevelGeom {
  int w, h;            // level size
  int pitch;           // row pitch in bytes inside the slots (multiple of 64)
  int quota;           // n_l, features wanted on this level (Appendix A.3)
  float scale;         // scaleFactor^l as f32
  unsigned off;        // byte offset of the level inside one image's slot (multiple of 256)
  unsigned cand_off;   // element offset of the level's candidate region inside one image's slot
  unsigned cand_cap;   // worst-case number of NMS survivors of the level
  int btiles_x, btile_start;   // blur tiles (64x16 over the whole level)
  int ftiles_x, ftile_start;   // FAST tiles (64x16 over the border-filtered region [31,w-31)x[31,h-31))
  // describe tiles (describe_tile_kernel): the keypoint region [31, w-32] x [31, h-32] cut into dt_nx x dt_ny rectangles of dt_tw x dt_th
  // keypoint positions; tile of a keypoint = ((x - 31) / dt_tw, (y - 31) / dt_th), the divisions by __umulhi with dt_mx / dt_my
  int dt_nx, dt_ny, dt_tw, dt_th, dt_start;
  unsigned dt_mx, dt_my;
};
struct OrbGeom {
  int n_levels;
  int btiles_total, ftiles_total;
  int fast_threshold;
  unsigned slot_bytes;   // bytes of one image's pyramid (and blur) slot
  unsigned cand_total;   // candidate slots per image (sum of cand_cap)
  int dt_total;          // describe tiles per image (all levels); 0: the image size does not admit them (describe_fused_kernel then)
  OrbLevelGeom lv[ORBX_MAX_LEVELS];
};
// Where level images live: level 0 is the caller's image when it is 4-byte aligned with a pitch
// that is a multiple of 4, otherwise a copy in the pyramid slot; levels >= 1 are in the slot.
struct OrbSrc {
  const uint8_t* l0;
  size_t l0_img_stride;   // bytes between consecutive images at level 0
  int l0_pitch;
  int pad_;
  uint8_t* pyr;
  uint8_t* blur;          // blurred levels: set by orbx_debug_read_level(which = 1) only (the product path keeps no blurred pyramid)
};

// device status word bits (sticky, cleared by orbx_check_status)
#define ORBX_ST_KP_OVERFLOW 1u   // more keypoints than cap_kp
#define ORBX_ST_INTERNAL 2u

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// ---- host staging shared by the batched forms ("Host staging"; the functions are beside orbx_reserve in orbx_api.hip) ----
// Byte offsets inside one buffer, 256-byte aligned pieces: take(bytes) answers where the piece starts, `off` is the total so far.
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};
// Grow-only pinned host memory (orbx_reserve_pinned).
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
// Two pinned slots used in turn for the small host tables of a device form, so that the caller's arrays are free when the call
// returns; ev[i] is recorded behind the upload that read slot i (orbx_ring_begin / orbx_ring_commit).
struct UploadRing {
  PinnedBuf slot[2];
  hipEvent_t ev[2] = {nullptr, nullptr};
  int next = 0;
};
// One host form's blobs: [in_bytes | out_bytes] in a pinned buffer (hi, ho) and at the same offsets in a workspace (di, dout).
struct HostCall {
  uint8_t* hi; uint8_t* ho; uint8_t* di; uint8_t* dout;
  size_t in_bytes;
};

// The resident map's grow-only workspaces (map_store_kernels.hip), one per role.  A call family reserves its own members only, so two
// live buffers of one stream never overlap; where families share a member, the member says so.
struct MapWorkspaces {
  DevBuf sel_scratch;     // selection: candidates and chunk counts
  DevBuf host_blobs;      // every host form's input / output blobs, and the window collection of the BA drivers (shared by all of them: a host form waits for its download before it returns)
  DevBuf call_tables;     // the selection's tables, orbx_map_points_set's slots and rows, orbx_map_points_erase's slots (shared: each goes up through ring_map and is read by the launches behind it)
  DevBuf ref_items;       // the reference-keyframe form's item table
  DevBuf cov_scratch;     // covisibility: weights, best lists and the segments made from them
  DevBuf cov_tables;      // covisibility: the call's keyframe table and queries
  DevBuf win_scratch;     // BA-window collection: list offsets, gathered descriptors, chunk counts, roles and bases
  DevBuf win_tables;      // BA-window collection: the call's keyframe table and chain
  DevBuf obs_scratch;     // observations: counts, cursors, block sums and the unordered entries; the redundancy call's chunk sums
  DevBuf obs_tables;      // observations: the call's keyframe table, slots and candidates
  DevBuf refresh_lists;   // orbx_map_refresh_points: the lists and the gathered positions; orbx_map_keyframe_redundancy: the candidates' list and gathered rows (shared: neither call runs inside the other)
  DevBuf fuse_scratch;    // fuse and merge: L's gathered rows, matches, edges, claims, per-node and per-feature scratch
  DevBuf fuse_tables;     // fuse and merge: the call's keyframe and target tables
  DevBuf create_tables;   // point creation: the call's tables (keyframes, free slots, the neighbour loop's)
  DevBuf create_scratch;  // point creation: flags, last-writer cells and the neighbour loop's scratch and lists
  DevBuf remove_tables;   // point removal: the call's keyframe table and slots, the counter
  DevBuf loop_scratch;    // loop correction (loop_close_kernels.hip): the N x N weights, candidates and chunk counts, pairs, per-node scratch
  DevBuf loop_tables;     // loop correction: the call's keyframe table, parents and poses
  template <class F>
  void for_each(F&& f) {   // every member, so that orbx_destroy frees what is added here
    for (DevBuf* b : {&sel_scratch, &host_blobs, &call_tables, &ref_items, &cov_scratch, &cov_tables, &win_scratch, &win_tables, &obs_scratch, &obs_tables,
                      &refresh_lists, &fuse_scratch, &fuse_tables, &create_tables, &create_scratch, &remove_tables, &loop_scratch, &loop_tables})
      f(*b);
  }
};
static_assert(sizeof(MapWorkspaces) == 18 * sizeof(DevBuf), "MapWorkspaces::for_each lists every member");

// The grow-only workspaces of the single-problem matchers and searches (orbx_api.hip, keyframe.hip, bow_kernels.hip,
// triangulate_kernels.hip), one per role.  A host form holds host_blob from its upload to its download; whatever it calls in between
// owns another member.
struct IoWorkspaces {
  DevBuf host_blob;       // every single-problem host form's input / output blob: orbx_stereo_match, orbx_hamming_match_crosscheck, orbx_hamming_batch, orbx_guided_match, orbx_search_for_triangulation[_bow], orbx_fuse_search, orbx_triangulate_pairs, orbx_bow_transform, orbx_bow_vectors and the orbx_keyframe_* searches (shared by all of them: a host form waits for its download before it returns, and none calls another host form)
  DevBuf fuse_poses;      // orbx_fuse_search_device: the inverse keyframe poses, up through ring_io (its callers orbx_fuse_search and orbx_keyframe_fuse_search hold host_blob and kf_gather)
  DevBuf bow_scratch;     // orbx_bow_vectors_device: word, leaf, node and weight per descriptor (its caller orbx_bow_vectors holds host_blob)
  DevBuf nb_scratch;      // orbx_keyframe_triangulate_from_neighbors: the searches' scratch, pair status and points (tri_nb_plan's ws_bytes); its tables and lists are in host_blob
  DevBuf kf_gather;       // orbx_keyframe_fuse_search: the target keyframes' features side by side (device-to-device; never leaves the device)
  DevBuf pair_images;     // orbx_process_stereo: the image pair
  DevBuf pair_out;        // orbx_process_stereo: the pair's output block (mirrored by pin_stage; both addresses are part of the captured graph)
  template <class F>
  void for_each(F&& f) {   // every member, so that orbx_destroy frees what is added here
    for (DevBuf* b : {&host_blob, &fuse_poses, &bow_scratch, &nb_scratch, &kf_gather, &pair_images, &pair_out}) f(*b);
  }
};
static_assert(sizeof(IoWorkspaces) == 7 * sizeof(DevBuf), "IoWorkspaces::for_each lists every member");

// The grow-only workspaces of the whole-map global BA (global_ba_kernels.hip), one per role; nothing is sized by the keyframe cap.
struct GlobalBaWorkspaces {
  DevBuf blobs;           // the call's input blob (state, fixed poses, parameters, host observations) and output blob (result record, parameters)
  DevBuf arena;           // lists, per-observation and per-point build results, trial parameters, the factored diagonal blocks
  DevBuf system;          // the reduced system S [6K + 1][6K rounded up to 64]: lower triangle, the right-hand side as the last row
  template <class F>
  void for_each(F&& f) {   // every member, so that orbx_destroy frees what is added here
    for (DevBuf* b : {&blobs, &arena, &system}) f(*b);
  }
};
static_assert(sizeof(GlobalBaWorkspaces) == 3 * sizeof(DevBuf), "GlobalBaWorkspaces::for_each lists every member");

struct KernelTimer {
  std::string name;
  std::vector<hipEvent_t> ev;  // start/stop pairs of the current call
  float ms = 0.f;
  int launches = 0;
};

struct orbx_handle {
  int device = -1;
  int n_cu = 256;                 // compute units of the device (persistent launches size their grids by it)
  hipStream_t stream = nullptr;
  orbx_camera cam{};
  orbx_orb_params orb{};
  int max_w = 0, max_h = 0, max_batch = 0;
  std::string err;
  unsigned* d_status = nullptr;
  unsigned* h_status = nullptr;   // pinned
  PinnedBuf pin_stage;            // pinned mirror of the single-pair output block (orbx_process_stereo)
  // hipGraph of the device part of orbx_process_stereo (launch-bound: ~20 short launches per frame); valid for
  // one (w, h, cap, buffer addresses) configuration, re-captured when any of them changes
  hipGraphExec_t pair_graph = nullptr;
  int pg_w = 0, pg_h = 0, pg_cap = 0, pg_calls = 0;
  void* pg_img = nullptr;
  void* pg_out = nullptr;
  // cached level geometry + resize tables for the last image size
  int geom_w = 0, geom_h = 0;
  OrbGeom geom{};
  DevBuf resize_tab;                     // per level l>=1: xtab[w_l], ytab[h_l] packed (ofs<<16 | c1)
  std::vector<unsigned> resize_tab_off;  // element offsets: [2*l] x table, [2*l+1] y table
  unsigned btile_tab_off = 0, ftile_tab_off = 0, dtile_tab_off = 0;   // tile -> (level, tx, ty) tables of the blur / FAST / describe launches, same buffer
  OrbSrc last_src{};                               // where the level images of the last extraction live, and how many images it held:
  bool xcd_next_reversed = false;                  // set by launch_orb_extract: the image order of the launch after its last one (the matcher's, in orbx_process_stereo_batch_device)
  int last_n_images = 0;                           // orbx_debug_read_level(which = 1) blurs them on demand (the product path keeps no blurred pyramid)
  // grow-only workspaces
  DevBuf ws_pyr, ws_blur, ws_cand, ws_counters, ws_sel, ws_sel2, ws_match;
  IoWorkspaces ws_io;                    // the single-problem matchers and searches, and orbx_process_stereo's two blocks
  PinnedBuf pin_io;                      // pinned staging of the single-problem host forms (one upload, one download)
  UploadRing ring_io;                    // orbx_fuse_search_device's inverse poses on their way to ws_io.fuse_poses
  DevBuf ws_dtile;                       // [image][describe tile] (begin, end) inside the level's spatially ordered keypoint list (rank_select_kernel)
  DevBuf ws_ba_in, ws_ba_arena, ws_ba_out;   // ba_solve_batch: input blob (descriptors, states, parameters | observations), scratch arena, output blob
  DevBuf ws_ba_imu, ws_ba_s15;             // ... inertial: IMU edges, preintegrations and records; the 15-d reduced system
  DevBuf ws_ba_debug;                      // ba_debug_blocks / ba_debug_imu_residual
  DevBuf ws_pnp[2];                      // PnP-RANSAC: [0] hypotheses + counts (pnp_kernels.hip), [1] the host forms' input / output blobs
  PinnedBuf pin_pnp;                     // pinned staging of orbx_pnp_ransac_batch (one upload, one download)
  DevBuf ws_pi;                          // pose-inertial optimization: the host forms' input / output blob (pose_inertial_kernels.hip)
  PinnedBuf pin_pi;                      // pinned staging of orbx_pose_inertial_batch
  DevBuf ws_track[3];                    // frame tracking (track_kernels.hip): [0] grids, matches and counters, [1] the host form's input / output blobs, [2] mp_offsets of the device form
  PinnedBuf pin_track;                   // pinned staging of orbx_track_frames
  UploadRing ring_track;                 // orbx_track_frames_device's mp_offsets on their way to ws_track[2]
  DevBuf ws_tref[3];                     // reference-keyframe tracking (track_ref_kernels.hip): [0] minima, pairs and counters, [1] the host form's input / output blobs, [2] the call's item table (and the keyframe form's positions / valid)
  PinnedBuf pin_tref;                    // pinned staging of orbx_track_reference
  UploadRing ring_tref;                  // the device forms' item table (and the keyframe form's positions / valid) on their way to ws_tref[2]
  DevBuf ws_lv[4];                       // loop verification (loop_verify_kernels.hip): [0] minima, counters, hypotheses and models, [1] the host forms' input / output blobs, [2] the call's item table and node ids, [3] the standalone Sim3 host form's blobs
  PinnedBuf pin_lv;                      // pinned staging of the host forms
  UploadRing ring_lv;                    // the item table and the node ids on their way to ws_lv[2]
  DevBuf ws_mp[3];                       // map-point refresh (mappoint_kernels.hip): [0] the long points' counter and list, [1] the host forms' input / output blobs, [2] the call's keyframe table
  PinnedBuf pin_mp;                      // pinned staging of the host forms
  UploadRing ring_mp;                    // the keyframe table on its way to ws_mp[2]
  MapWorkspaces ws_map;                  // resident map points (map_store_kernels.hip)
  PinnedBuf pin_map;                     // pinned staging of the resident map's host forms and orbx_map_points_download
  UploadRing ring_map;                   // every resident-map call's tables on their way to its *_tables workspace
  GlobalBaWorkspaces ws_gba;             // whole-map global BA (global_ba_kernels.hip)
  PinnedBuf pin_gba;                     // pinned staging of its one upload and one download
  // pipelined host-batch path: copy streams, events, double-buffered staging
  hipStream_t s_in = nullptr, s_out = nullptr;
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_comp[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
  DevBuf ws_pipe[2][8];
  // BA
  orbx_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;
  void* rccl_comm = nullptr;                               // ncclComm_t of the point-partitioned solve (orbx_ba_init_rccl / orbx_ba_set_rccl_comm)
  orbx_handle* ba_aux = nullptr;                           // second stream + workspaces of orbx_ba_solve_visual_batch (half of a large batch runs there)
  bool rccl_owned = false;
  PinnedBuf pin_ba_in, pin_ba_out;                         // pinned mirrors of the batch input / output blobs (ba_solve_batch)
  int* h_abort = nullptr;    int* d_abort = nullptr;       // pinned, device-visible: should_stop() seen while the iterations drain
  OrbxWorkPool* ba_pool = nullptr;                         // host workers of the batch preprocessing (created by the first large batch)
  OrbxHelperThread* ba_helper = nullptr;                   // drives the second half of a large batch (orbx_ba_solve_visual_batch)
  hipEvent_t ba_up_event = nullptr;                        // recorded by the first half of a batch once its uploads are enqueued (BaCallOpts)
  // profiling
  bool profiling = false;
  std::string prof_only;   // non-empty: only this kernel's launches are bracketed (orbx_set_profiling_only)
  std::vector<KernelTimer> timers;
  std::vector<hipEvent_t> event_pool;
  size_t event_next = 0;
  hipEvent_t prof_tail = nullptr;          // end event of the last profiling scope (may start the next one)
};

// A keyframe with its feature arrays in device memory (keyframe.hip; the slot table: map_store_kernels.hip).
struct orbx_map_points;
struct orbx_keyframe {
  orbx_handle* h = nullptr;
  uint64_t id = 0, timestamp_ns = 0;
  double pose_wc[7] = {1, 0, 0, 0, 0, 0, 0};
  int n = 0;
  uint8_t* block = nullptr;          // one device allocation: kp | desc | points_cam | has_point | mp_flag | mp_slot | mp_uniq
  orbx_keypoint* d_kp = nullptr;
  uint8_t* d_desc = nullptr;
  double* d_points = nullptr;
  uint8_t* d_has_point = nullptr;
  uint8_t* d_mp_flag = nullptr;
  int* d_mp_slot = nullptr;          // per feature the slot of its map point in slot_store, -1 = None (orbx_keyframe_set_map_point_slots)
  int* d_mp_uniq = nullptr;          // d_mp_slot with every repeat of a slot inside the keyframe set to -1: the keyframe's observed set, each slot once (covisibility)
  const orbx_map_points* slot_store = nullptr;   // the store the table was set against; NULL: no table (every feature -1)
  std::vector<int64_t> mp_ids;       // matched_map_points (host side: ids are map bookkeeping), -1 = None
  // FeatureVector as one node id per feature (orbx_keyframe_set_feature_nodes): host copy, and the feature indices sorted by
  // (node, index) with the features in no list cut off the end — every node's list in push order (vocabulary/mod.rs:309)
  bool has_nodes = false;
  std::vector<uint32_t> node;
  std::vector<int> node_sorted;
  int node_m = 0;
};

// Map points resident on the device (map_store_kernels.hip; the loop closer acts on the same store: loop_close_kernels.hip).
struct orbx_map_points {
  orbx_handle* h = nullptr;
  int capacity = 0, n_live = 0;
  uint8_t* block = nullptr;            // one device allocation: positions | descriptors | live
  double* d_pos = nullptr;
  uint8_t* d_desc = nullptr;
  uint8_t* d_live = nullptr;
  std::vector<uint8_t> live;           // host mirror of d_live: every change goes through set / set_device / erase, whose slots are host arrays
  std::vector<unsigned> stamp;         // per slot the last call that named it (a slot listed twice in one call is refused)
  unsigned gen = 0;
  DevBuf first;                        // [frames][capacity] first-sighting tables, EMPTY between calls
  DevBuf mark;                         // [queries][capacity] bytes: covisibility's marked sets, 0 between calls (never shared with `first`)
};

int orbx_fail(orbx_handle* h, int code, const char* fmt, ...);
// The body of an extern "C" entry point: no C++ exception may cross the C boundary (ctypes, Rust); h == nullptr: the code alone.
// Every entry point that can allocate host memory runs inside it.  Left bare, because they allocate none: getters, destroy / close
// and default-configuration calls, orbx_vocab_nodes, orbx_bow_score, orbx_keyframe_set_pose / get_map_points / download, the thin
// wrappers of guarded calls (orbx_kfdb_detect_loop_candidates, orbx_pose_inertial_optimize, orbx_ba_solve_inertial_obs32[_device]),
// and among the single-problem matchers and searches orbx_stereo_match[_batch_device], orbx_hamming_match_crosscheck[_device],
// orbx_hamming_batch[_device], orbx_guided_match[_device], orbx_search_for_triangulation[_device] and orbx_triangulate_pairs[_device]:
// their tables are made in pinned staging.  (orbx_search_for_triangulation_bow sorts, orbx_fuse_search[_device] and the extraction
// calls may grow host tables: guarded.)
template <class F>
int orbx_guard(orbx_handle* h, const char* who, F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return h ? orbx_fail(h, ORBX_ERR_HIP, "%s: out of host memory", who) : (int)ORBX_ERR_HIP;
  } catch (...) {
    return h ? orbx_fail(h, ORBX_ERR_HIP, "%s: unexpected C++ exception", who) : (int)ORBX_ERR_HIP;
  }
}
// pose.inverse() of a T_wc given as (qw, qx, qy, qz, tx, ty, tz): se3.rs:56-63 with nalgebra's quaternion-vector product, one IEEE
// operation at a time (include/orbx.hpp's se3_inverse)
inline void orbx_pose_inverse(const double* p, double* out) {
  const double w = p[0], x = -p[1], y = -p[2], z = -p[3];
  const double* v = p + 4;
  const double t[3] = {2.0 * (y * v[2] - z * v[1]), 2.0 * (z * v[0] - x * v[2]), 2.0 * (x * v[1] - y * v[0])};
  const double c[3] = {y * t[2] - z * t[1], z * t[0] - x * t[2], x * t[1] - y * t[0]};
  out[0] = w; out[1] = x; out[2] = y; out[3] = z;
  for (int i = 0; i < 3; ++i) out[4 + i] = -(t[i] * w + c[i] + v[i]);
}
// A FeatureVector given as one node id per feature, as one sorted array: sorted [n] receives the feature indices by (node, index)
// ascending, which is every node's list in push order (vocabulary/mod.rs:309); the features in no list (node 0xffffffff) sort last and
// are cut off: the answer is how many remain.
inline int orbx_sort_by_node(const uint32_t* node, int n, int* sorted) {
  for (int i = 0; i < n; ++i) sorted[i] = i;
  std::stable_sort(sorted, sorted + n, [&](int a, int b) { return node[a] < node[b]; });
  int m = n;
  while (m > 0 && node[sorted[m - 1]] == 0xffffffffu) --m;
  return m;
}
// ... and for every feature i of keyframe 1 the range [lo[i], hi[i]) of sorted [m] that holds keyframe 2's features in feature i's
// node (triangulation.rs:577-581); empty (0, 0) where feature i is in no list
inline void orbx_node_ranges(const uint32_t* node1, int n1, const uint32_t* node2, const int* sorted, int m, int* lo, int* hi) {
  for (int i = 0; i < n1; ++i) {
    lo[i] = hi[i] = 0;
    const uint32_t key = node1[i];
    if (key == 0xffffffffu) continue;
    const int* b = std::lower_bound(sorted, sorted + m, key, [&](int a, uint32_t k) { return node2[a] < k; });
    const int* e = std::upper_bound(b, sorted + m, key, [&](uint32_t k, int a) { return k < node2[a]; });
    lo[i] = (int)(b - sorted); hi[i] = (int)(e - sorted);
  }
}
int orbx_reserve(orbx_handle* h, DevBuf& b, size_t bytes);
// Grow-only, in steps of 1 MiB.  A buffer that is replaced may still be read or written by a copy on the handle's stream: the stream is
// synchronised before it is freed (so a host form may call this, a device form may not).
int orbx_reserve_pinned(orbx_handle* h, PinnedBuf& b, size_t bytes);
// begin: takes the ring's next slot, waits for the upload that last read it (the only wait: the slot is then idle and grows without
// synchronising the stream), reserves `dev` and answers both bases; the caller fills host[0, bytes), where it may store pointers into
// device[0, bytes).  commit: enqueues the copy on the handle's stream, then records the slot's event behind it.
int orbx_ring_begin(orbx_handle* h, UploadRing& r, DevBuf& dev, size_t bytes, uint8_t** host, uint8_t** device);
int orbx_ring_commit(orbx_handle* h, UploadRing& r, const DevBuf& dev, size_t bytes);
// The skeleton of a host form: begin reserves pin and dev for in_bytes + out_bytes and sets c; the caller fills c.hi; upload is the one
// host-to-device copy of the input blob; download copies out[0, bytes) back and synchronises the stream, the call's only wait.
int orbx_host_call_begin(orbx_handle* h, PinnedBuf& pin, DevBuf& dev, size_t in_bytes, size_t out_bytes, HostCall& c);
int orbx_host_call_upload(orbx_handle* h, const HostCall& c);
int orbx_host_call_download(orbx_handle* h, const HostCall& c, size_t bytes);

// The host tables of a device form, every piece stated once.  put(src, bytes) reserves a 256-byte aligned piece as Carve does and
// answers its offset; with a null source or no bytes it reserves and copies nothing (the caller fills the piece in place, through
// `host`).  begin: orbx_ring_begin for the pieces' total, then the copies into the slot; `host` and `device` are the two bases.
// commit: orbx_ring_commit of the same bytes.  send: both.  A plan holds CAP copied pieces: one more fails begin, none is dropped.
struct UploadPlan {
  static constexpr int CAP = 8;
  struct Piece { size_t off; const void* src; size_t bytes; };
  Carve c;
  Piece piece[CAP];
  int n = 0;
  uint8_t* host = nullptr;
  uint8_t* device = nullptr;
  size_t put(const void* src, size_t bytes) {
    const size_t o = c.take(bytes);
    if (src && bytes) { if (n < CAP) piece[n] = Piece{o, src, bytes}; ++n; }
    return o;
  }
  int begin(orbx_handle* h, UploadRing& r, DevBuf& dev) {
    if (n > CAP) return orbx_fail(h, ORBX_ERR_HIP, "internal: an upload plan of %d pieces holds %d", n, CAP);
    if (int rc = orbx_ring_begin(h, r, dev, c.off, &host, &device)) return rc;
    for (int i = 0; i < n; ++i) std::memcpy(host + piece[i].off, piece[i].src, piece[i].bytes);
    return ORBX_OK;
  }
  int commit(orbx_handle* h, UploadRing& r, const DevBuf& dev) { return orbx_ring_commit(h, r, dev, c.off); }
  int send(orbx_handle* h, UploadRing& r, DevBuf& dev) {
    if (int rc = begin(h, r, dev)) return rc;
    return commit(h, r, dev);
  }
};

// The outputs of a host form, every piece stated once.  add(dst, count) reserves count elements in the blob that comes down and
// answers the piece; keep(bytes) reserves what stays on the device, behind everything that comes down.  begin: orbx_host_call_begin
// for in_bytes and the pieces' total; from then on dev(p) is where the launches write piece p (an address inside HostCall::dout, which
// does not exist before the total is known).  finish: orbx_host_call_download of the added pieces, then every piece with a
// destination is copied to it whole.  A piece added with `later` is left to copy(p, n): n <= count elements, a number the download
// itself tells (host(p) is the pinned copy).  A plan holds CAP pieces: one more fails begin, none is dropped.
struct OutputPlan {
  static constexpr int CAP = 16;
  template <class T> struct Piece { int i; };
  struct Rec { size_t off, bytes; void* dst; bool later; };
  Carve c;
  size_t down = 0;
  Rec rec[CAP];
  int n = 0;
  HostCall call{};
  template <class T>
  Piece<T> add(T* dst, size_t count, bool later = false) {
    const size_t bytes = sizeof(T) * count, o = c.take(bytes);
    down = c.off;
    if (n < CAP) rec[n] = Rec{o, bytes, dst, later};
    return Piece<T>{n++};
  }
  size_t keep(size_t bytes) { return c.take(bytes); }
  int begin(orbx_handle* h, PinnedBuf& pin, DevBuf& dev, size_t in_bytes = 0) {
    if (n > CAP) return orbx_fail(h, ORBX_ERR_HIP, "internal: an output plan of %d pieces holds %d", n, CAP);
    return orbx_host_call_begin(h, pin, dev, in_bytes, c.off, call);
  }
  template <class T> T* dev(Piece<T> p) const { return (T*)(call.dout + rec[p.i].off); }
  template <class T> const T* host(Piece<T> p) const { return (const T*)(call.ho + rec[p.i].off); }
  int finish(orbx_handle* h) {
    if (int rc = orbx_host_call_download(h, call, down)) return rc;
    for (int i = 0; i < n; ++i)
      if (rec[i].dst && rec[i].bytes && !rec[i].later) std::memcpy(rec[i].dst, call.ho + rec[i].off, rec[i].bytes);
    return ORBX_OK;
  }
  template <class T>
  int copy(orbx_handle* h, Piece<T> p, size_t count) {
    const Rec& r = rec[p.i];
    if (sizeof(T) * count > r.bytes) return orbx_fail(h, ORBX_ERR_HIP, "internal: %zu elements copied out of an output piece of %zu bytes", count, r.bytes);
    if (count) std::memcpy(r.dst, call.ho + r.off, sizeof(T) * count);
    return ORBX_OK;
  }
};
// CSR offsets off[0..n]: non-null, off[0] == 0, ascending, no span above `cap`; ORBX_OK or ORBX_ERR_INVALID (the message names who, the
// array and the `unit` counted, such as "frame").  *max_span, when given, receives the largest off[i + 1] - off[i].
int orbx_check_offsets(orbx_handle* h, const char* who, const char* name, const char* unit, int n, const int* off, int* max_span = nullptr,
                       int cap = 0x7fffffff);

#define ORBX_HIP(h, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return orbx_fail((h), ORBX_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                       __FILE__, __LINE__);                                                 \
  } while (0)

// profiling scope: records a start/stop event pair on the handle's stream around a launch when profiling is on
struct ProfScope {
  orbx_handle* h;
  int idx;
  ProfScope(orbx_handle* h, const char* name, bool chained = false);
  ~ProfScope();
};
// One launch on the handle's stream inside its profiling scope.  The label is the kernel's plain name, whichever instantiation or
// kernel pointer is launched; hipGetLastError is the caller's, once per group of launches.
template <class Kernel, class... Args>
inline void orbx_launch(orbx_handle* h, const char* label, bool chained, Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, const Args&... args) {
  ProfScope ps(h, label, chained);
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, h->stream, args...);
}

// ---- kernel launchers (defined in the .hip files) --------------------------------------------------
// matcher (match_kernels.hip)
// (pairs_reversed: the one-workgroup-per-pair matcher walks the pairs downwards — the launch after an extraction whose last launch walked upwards)
int launch_stereo_match(orbx_handle* h, int batch, const orbx_keypoint* d_kp, const uint8_t* d_desc,
                        const int* d_nkp, int cap_kp, orbx_dmatch* d_matches, int* d_nmatches,
                        double* d_points, uint8_t* d_has_point, bool pairs_reversed = false);
int launch_crosscheck(orbx_handle* h, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                      orbx_dmatch* d_out, int* d_n_out);
int launch_hamming_batch(orbx_handle* h, const uint8_t* d_a, const uint8_t* d_b, int n, uint32_t* d_out);
int launch_guided_match(orbx_handle* h, const orbx_keypoint* d_kp, const uint8_t* d_desc, int n, double img_w, double img_h,
                        const double* d_q_uv, const uint8_t* d_q_desc, int nq, double radius, int mode, int* d_out_idx,
                        uint32_t* d_out_dist);
int launch_search_for_triangulation(orbx_handle* h, const orbx_camera* cam, const double* F9, const double* epipole,
                                    const orbx_keypoint* d_kp1, const uint8_t* d_desc1, const uint8_t* d_mp1,
                                    const uint8_t* d_stereo1, int n1, const orbx_keypoint* d_kp2, const uint8_t* d_desc2,
                                    const uint8_t* d_mp2, int n2, unsigned max_dist, int* d_pairs, int* d_n_out);
int launch_search_for_triangulation_bow(orbx_handle* h, const double* F9, const double* epipole, const orbx_keypoint* d_kp1,
                                        const uint8_t* d_desc1, const uint8_t* d_mp1, const uint8_t* d_stereo1, int n1,
                                        const orbx_keypoint* d_kp2, const uint8_t* d_desc2, const uint8_t* d_mp2, int n2,
                                        const int* d_sorted_idx, const int* d_rng_lo, const int* d_rng_hi, unsigned max_dist,
                                        int* d_pairs, int* d_n_out);
struct TriArgs {
  double F[9];                 // fundamental matrix, row-major (host, triangulation.rs:670-683)
  double epx, epy;             // epipole of camera 1 in image 2 (:418-426)
  int cols, rows;              // 32-px grid over image 2 (:339-346, :437-438)
  unsigned max_dist;
  int n1, n2;
  const orbx_keypoint* kp1; const uint8_t* desc1; const uint8_t* mp1; const uint8_t* stereo1;
  const orbx_keypoint* kp2; const uint8_t* desc2;
  const int* cell_start; const int* sorted_idx; const unsigned short* cell_of;
  uint8_t* taken;              // per feature of keyframe 2: has a map point (mp2) or has been matched
  // FeatureVector mode (search_for_triangulation_bow, :541-658): candidates of feature i1 are sorted_idx[rng_lo[i1] ..
  // rng_hi[i1]) = the features of keyframe 2 in the same vocabulary node, ascending; no grid (cell_of == nullptr)
  const int* rng_lo; const int* rng_hi;
};
// One neighbour of the batched search (launch_search_for_triangulation_batch): the single search's arguments plus the workspace slices
// the three kernels use.  Only neighbours that are searched are listed (n1 > 0, n2 > 0): the caller leaves the skipped ones out.
struct TriBatchItem {
  TriArgs A;
  const uint8_t* mp2;          // the neighbour's map-point flags (copied into A.taken by the build step)
  int* prop; int* owner; int* pairs; int* n_out;
};
// grid side of image 2 (triangulation.rs:434-438); false when the image is empty
bool tri_grid_dims(const orbx_camera* cam, int* cols, int* rows);
// epipole of camera 1 in image 2 and the fundamental matrix (orbx_api.hip; triangulation.rs:418-431, :661-683)
void orbx_triangulation_geometry(const orbx_camera* cam, const double* pose1_wc, const double* pose2_wc, double* ep2, double* F9);
// d_items [T] in device memory (already uploaded on the handle's stream), every one with n1 > 0 and n2 > 0; max_n1 / max_n2 over them
int launch_search_for_triangulation_batch(orbx_handle* h, const TriBatchItem* d_items, int T, int max_n1, int max_n2);

// ---- pair triangulation (triangulate_kernels.hip; triangulation.rs:186-277, :715-850) ----
// what all pairs of a call share: camera, gates, keyframe 1
struct TriCommon {
  orbx_camera cam;
  double min_parallax_cos, reproj_mono, reproj_stereo, scale_factor;
  double pow12[32];            // 1.2^octave from the host's pow, so that the scale gate compares the host's bits
  const orbx_keypoint* kp1; const double* pts1; const uint8_t* has1; int n1;
  double pose1[7];
};
// keyframe 2 and the pairs to evaluate; results go to slots [out_base, out_base + n_pairs) of the status / point arrays
struct TriNeighbour {
  const orbx_keypoint* kp2; const double* pts2; const uint8_t* has2; int n2;
  double pose2[7];
  const int* pairs;            // [n][2] (idx1, idx2)
  const int* n_pairs_dev;      // the count where a search left it on the device, else NULL and n_pairs holds it
  int n_pairs, out_base;
};
void tri_common_fill(TriCommon* c, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial);
// `one` by value (d_many = NULL, T = 1) or T neighbours in device memory; max_pairs bounds every neighbour's pair count
int launch_triangulate_pairs(orbx_handle* h, const TriCommon& c, const TriNeighbour& one, const TriNeighbour* d_many, int T, int max_pairs,
                             uint16_t* d_status, double* d_points);
// ordered compaction of the CREATED pairs (neighbour, then pair order) and the per-neighbour counters:
// d_head [1 + 4T] = n_created | per neighbour (unused, matches_found, triangulated, validated); lists of `cap` entries
int launch_triangulate_compact(orbx_handle* h, const TriNeighbour* d_many, int T, const uint16_t* d_status, const double* d_points, int cap,
                               int* d_head, int* d_out_nb, int* d_out_idx1, int* d_out_idx2, double* d_out_points);
// ---- the neighbour loop of triangulate_from_neighbors (keyframe.hip; triangulation.rs:117-294) ----
// What the loop is for one current keyframe and its neighbours, made on the host: the neighbours that are searched, and byte offsets
// into two device blocks — the uploaded tables (items | neighbours | FeatureVector tables: up_bytes) and the scratch (ws_bytes).
struct TriNbPlan {
  struct Slices { size_t sorted, lo, hi, cell_start, prop, owner, pairs, n_out, cell_of, taken; bool bow; };
  std::vector<int> orig;       // searched neighbour k -> index in kfs[]
  std::vector<Slices> sl;      // [searched]
  int n1 = 0, max_n2 = 0, cols = 0, rows = 0;
  size_t up_bytes = 0, ws_bytes = 0, o_items = 0, o_nbs = 0, o_status = 0, o_points = 0;
};
void tri_nb_plan(const orbx_camera* cam, const orbx_keyframe* cur, const orbx_keyframe* const* kfs, int T, TriNbPlan& P);
// the tables into up [up_bytes] (host), as they will lie at d_up; d_mp1 / d_mp2 [T]: the map-point flags of cur / kfs[t] (device)
void tri_nb_fill(const TriNbPlan& P, const orbx_camera* cam, const orbx_triangulation_config* cfg, const orbx_keyframe* cur, const orbx_keyframe* const* kfs,
                 const uint8_t* d_mp1, const uint8_t* const* d_mp2, uint8_t* up, uint8_t* d_up, uint8_t* d_ws);
// searches, pair loop, ordered compaction (the lists of `cap` rows; d_head [1 + 4 * searched], d_out_nb counts searched neighbours)
int tri_nb_launch(orbx_handle* h, const TriNbPlan& P, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial, const orbx_keyframe* cur,
                  const uint8_t* d_up, uint8_t* d_ws, int cap, int* d_head, int* d_out_nb, int* d_out_idx1, int* d_out_idx2, double* d_out_points);
int launch_fuse_search(orbx_handle* h, const orbx_camera* cam, const double* d_positions, const uint8_t* d_mp_desc, int P,
                       const double* d_kf_pose_cw, const int* d_kf_off, const orbx_keypoint* d_kps, const uint8_t* d_descs,
                       int T, double radius_scale, unsigned desc_threshold, int* d_out_idx, uint32_t* d_out_dist);
// ---- frame tracking against map points (track_kernels.hip; tracker.rs:863-988, :1086-1192) ----
// What the four launches around PnP read and write; every pointer is device memory.
struct TrackArgs {
  orbx_camera cam;
  int mode, min_corr, min_inl, max_feat, fc_stride;
  double radius, winv, hinv;
  // inputs
  const orbx_keypoint* kp; const uint8_t* desc; const int* feat_start; const int* feat_count;
  const double* positions; const uint8_t* mp_desc; const int* mp_off;
  const double* search_poses; const double* priors;
  // workspace: per frame cell_start [GG_CELLS+1], sorted_idx / cell_of / owner [max_feat], counts (n_corr, n_front); match [M]
  int* cell_start; int* sorted_idx; unsigned short* cell_of; int* owner; int* counts; int* match;
  // outputs
  int* offsets; double* pts3d; float* pts2d; int* mp_idx; int* feat_idx; double* poses_out;
  const uint8_t* inl; const orbx_pnp_result* pnp_res; int* matched; orbx_track_result* results;
};
// what can be refused before anything is enqueued; *max_mp: the most map points of a frame (mp_offsets is a host array: the lists'
// offsets, or where the lists are made on the device the offsets of their host-known bounds)
int track_check(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* c, const orbx_pnp_config* pnp_cfg, int B, const int* mp_offsets,
                int* max_mp, const char* who);
// The launches on the handle's stream (A.mp_off is device memory); max_mp bounds a frame's list, M the sum of the lists.
int track_launch(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg, int B, int max_mp,
                 size_t M, TrackArgs A, uint8_t* d_inl, double* d_err, orbx_pnp_result* d_pnp);
// orbx_pnp_config's range check (pnp_kernels.hip), for callers that enqueue work ahead of PnP's own launches
int orbx_pnp_check_config(orbx_handle* h, const orbx_pnp_config* c, const char* who);
// ---- tracking against the reference keyframe (track_ref_kernels.hip; tracker.rs:992-1064) ----
// Frame b's reference keyframe: its descriptors wherever they lie in device memory (a slice of a packed array or a resident
// orbx_keyframe's block) and where its rows start in the packed per-keyframe-feature arrays (positions, valid, matches).
struct TrackRefItem {
  const uint8_t* kf_desc;
  int kf_off, n;
};
// The device forms behind orbx_track_reference_device / orbx_keyframe_track_reference: items [B] is a host array (copied before
// the call returns); positions / valid [K] are device arrays, or host arrays that travel with the items (pos_on_host).
int track_reference_enqueue(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                            int B, const orbx_keypoint* d_kp, const uint8_t* d_desc, const int* d_feat_start, const int* d_feat_count,
                            int feat_count_stride, int max_feat, const TrackRefItem* items, const double* positions, const uint8_t* valid,
                            bool pos_on_host, const double* d_priors_wc, orbx_dmatch* d_matches, int* d_offsets, double* d_pts3d, float* d_pts2d,
                            int* d_kf_idx, int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                            orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results);
// ---- loop-candidate verification (loop_verify_kernels.hip; corrector.rs:116-204) ----
// One (current keyframe, loop keyframe) pair: where its feature arrays lie in device memory, its poses, its FeatureVectors as
// host arrays (both given: the FeatureVector matcher, else brute force) and where its rows start in the packed outputs.
struct LoopVerifyPair {
  const uint8_t* c_desc; const double* c_pts; const uint8_t* c_has; const uint32_t* c_node; int n1;
  const orbx_keypoint* l_kp; const uint8_t* l_desc; const double* l_pts; const uint8_t* l_has; const uint32_t* l_node; int n2;
  double pose_c[7], pose_l[7];
  int out_off;
};
// The device form behind orbx_verify_loop_candidates_device / orbx_keyframe_verify_loop_candidates: pairs [B] is a host array
// (copied, with the node ids, before the call returns); every output is device memory.
int loop_verify_enqueue(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int B,
                        const LoopVerifyPair* pairs, orbx_dmatch* d_matches, int* d_feature_matches, double* d_pts_current,
                        double* d_pts_loop, uint8_t* d_inlier, double* d_sim3, orbx_loop_verify_result* d_results);
// ---- map-point refresh (mappoint_kernels.hip; search_in_neighbors.rs:139-150, map.rs:716-742, :880-944) ----
// One keyframe of a call: its descriptor rows wherever they lie in device memory (a slice of a packed array or a resident
// orbx_keyframe's block), how many there are, and its camera centre (the translation of T_wc).
struct MapPointKf {
  const uint8_t* desc;
  int n, pad_;
  double centre[3];
};
// The device form behind orbx_refresh_map_points_device and the host forms: kfs [T] is a host array (copied before the call
// returns), everything else device memory.  A point keeps d_desc_in / d_normals_in where it is not updated; they may be the
// outputs themselves.  n_obs = obs_start[M].
int mp_refresh_enqueue(orbx_handle* h, const char* who, int M, int n_obs, const double* d_positions, const int* d_obs_start,
                       const int* d_obs_kf, const int* d_obs_feat, int T, const MapPointKf* kfs, double scale_range,
                       const uint8_t* d_desc_in, const double* d_normals_in, uint8_t* d_mp_desc, double* d_normals, double* d_min_distance,
                       double* d_max_distance, orbx_mp_refresh_record* d_records);
// The host forms: one upload, the launches, one download.  kfs [T] carries counts and centres; with kf_feat_offset / descs given
// (the packed form) the rows travel too and kfs[t].desc is set here, else (resident keyframes) it is set by the caller.
int mp_refresh_host_call(orbx_handle* h, const char* who, int M, const double* positions, const int* obs_start, const int* obs_kf,
                         const int* obs_feat, int T, MapPointKf* kfs, const int* kf_feat_offset, const uint8_t* descs, double scale_range,
                         uint8_t* mp_desc, double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records);
// extractor (orb_kernels.hip)
int orb_prepare_geometry(orbx_handle* h, int w, int h_px);
int launch_orb_extract(orbx_handle* h, const uint8_t* d_images, int n_images, int w, int h_px,
                       size_t stride, orbx_keypoint* d_kp, uint8_t* d_desc, int* d_nkp, int cap_kp);
// BA (ba_kernels.hip)
int ba_solve_visual(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                    const double* poses_cw, int F, const double* fixed_poses_cw, int M,
                    double* points, int N, const orbx_ba_obs* obs, orbx_should_stop_fn should_stop,
                    void* user, double* poses_wc_out, int* iterations, double* initial_error,
                    double* final_error, bool global_mode = false, const struct BaInertialHost* inr = nullptr,
                    const orbx_ba_obs32* obs32 = nullptr,    // obs32: the 16-byte form of the observations, used instead of obs when given
                    bool obs_on_device = false);             // ... and it lies in device memory of the handle's device, ordered on its stream
// whole-map global BA (global_ba_kernels.hip): orbx_ba_solve_global's semantics for up to gba_max_keyframes() optimised keyframes.  obs or
// obs32 is given; on_device: obs32 is device memory ordered on the handle's stream.  The caller has checked the pointers, K, M, N >= 1
// and that no collective is installed.
int gba_max_keyframes();
int gba_solve(orbx_handle* h, const char* who, const orbx_camera* cam, const orbx_ba_config* cfg, int K, const double* poses_cw,
              const double* fixed_pose_cw, int M, double* points, int N, const orbx_ba_obs* obs, const orbx_ba_obs32* obs32, bool on_device,
              orbx_should_stop_fn should_stop, void* user, double* poses_wc_out, int* iterations, double* initial_error, double* final_error);
// one window of a batch as the caller hands it over (orbx_ba_solve_visual_batch); status: ORBX_OK or ORBX_ERR_EMPTY
struct BaWinHost {
  int K, F, M, N;
  const double* poses_cw; const double* fixed_poses_cw; double* points; const orbx_ba_obs* obs;
  double* poses_wc_out; int* iterations; double* initial_error; double* final_error;
  int status;
  const orbx_ba_obs32* obs32 = nullptr;       // the 16-byte form of the observations (orbx.h): used instead of obs when given
  bool obs_on_device = false;                 // obs / obs32 is device memory, written by work already enqueued on the handle's stream: copied
                                              // device to device into the blob; no host path may read it (one window, no collective)
};
// What one ba_solve_batch call is told about the batch it is a half of (orbx_ba_solve_visual_batch builds one per half; default: none).
// The two halves of a batch share one PCIe link: the second half's uploads are ordered behind the first half's (its kernels then start
// as early as they can, and the second half's bytes travel under them).  The first half records its handle's ba_up_event on its stream
// once its uploads are enqueued and sets *gate_signal; the second half waits for *gate_wait, then makes its stream wait for gate_event.
struct BaCallOpts {
  int pool_cap = 0;                          // > 0: at most this many threads for the preprocessing (two halves share the cores)
  int peer_windows = 0;                      // windows of the other half, solved at the same time on the peer handle's stream (launch-shape heuristics count them)
  std::atomic<int>* gate_signal = nullptr;
  std::atomic<int>* gate_wait = nullptr;
  hipEvent_t gate_event = nullptr;
};
int ba_solve_batch(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int W, BaWinHost* win,
                   orbx_should_stop_fn should_stop, void* user, bool global_mode = false, const struct BaInertialHost* inr = nullptr,
                   bool single_call = false, const BaCallOpts& opts = BaCallOpts());
// in-place sum of `n` doubles over the ranks of the handle's communicator, ordered on `st` (ncclAllReduce, orbx_api.hip)
int orbx_rccl_allreduce_sum(orbx_handle* h, double* d_buf, size_t n, hipStream_t st);
// destroys the handle's communicator if the library owns it, and clears it
void orbx_rccl_drop(orbx_handle* h);
int ba_debug_imu_residual(orbx_handle* h, int K, const double* poses_wc, const double* velocities, int E, const int* edge_kf,
                          const double* preint, double* out);
int ba_debug_blocks(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K, const double* poses_cw, int F,
                    const double* fixed_poses_cw, int M, const double* points, int N, const orbx_ba_obs* obs, int global_mode,
                    double* out);
// the extra inputs / outputs of solve_inertial_ba (local_inertial_ba.rs:1074-1275) for ba_solve_visual's inertial mode
struct BaInertialHost {
  const orbx_inertial_ba_config* cfg;
  const double* velocities;   // [K][3]
  const double* biases;       // [K][6]
  int E;
  const int* edge_kf;         // [E][2]
  const double* preint;       // [E][11]
  double* vel_out;            // [K][3]
  double* bias_out;           // [K][6]
};
constexpr int BA_INERTIAL_MAX_K = 51;   // keyframes of an inertial window: BA_MAX_N / 15 (ba_kernels.hip), for callers that refuse before they enqueue
