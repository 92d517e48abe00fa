/*
 * orbx.h — C ABI of the MI355X-native hot path of jurmy24/orb-slam3-rust.
 *
 * This is the drop-in boundary.  The reference has no FFI layer of
 * its own: the path sits behind ordinary Rust `pub fn`s whose arguments are OpenCV
 * wrapper types.  Each entry point below names the reference interface it replaces
 * (file:line relative to the reference crate root); INTEGRATION.md shows the Rust
 * `extern "C"` block and the shim that re-creates the original signatures on top.
 *
 * Conventions
 *   - return 0 (ORBX_OK) on success, a negative ORBX_ERR_* otherwise;
 *     orbx_last_error(h) gives a human-readable message for the last failure
 *     (maps to `anyhow::Error` / `None` on the Rust side).
 *   - plain pointers and sizes only; no C++ or torch types.
 *   - the caller owns every buffer; capacities go in, counts come out.
 *     A result that does not fit its capacity is an error (ORBX_ERR_CAPACITY),
 *     never a silent truncation.
 *   - a handle is NOT thread-safe (mirrors `&mut self`, stereo.rs:52); use one
 *     handle per thread.  Each handle owns one HIP stream on its device.
 *   - `*_device` entry points take device pointers (memory of the handle's GPU)
 *     and are asynchronous on the handle's stream unless stated.  That stream is
 *     non-blocking: inputs produced on another stream must be complete (or ordered
 *     with an event against orbx_stream()) before the call, and must stay allocated
 *     until the work has run; the others take
 *     host pointers, copy in/out, and return when the results are in the buffers.
 *   - there is NO CPU fallback: every entry point fails with ORBX_ERR_NO_DEVICE
 *     when no gfx950 device can be opened (the host-only orbx_euroc_* / orbx_png_*
 *     input functions need no device).
 *   - one environment switch, read by the first call and without effect on results:
 *     ORBX_NO_GRAPH=1 keeps orbx_process_stereo on eager launches instead of a captured hipGraph.
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  ORBX_OK = 0,
  ORBX_ERR_INVALID = -1,   /* bad argument (null pointer, size out of range)        */
  ORBX_ERR_NO_DEVICE = -2, /* no usable HIP device / wrong architecture             */
  ORBX_ERR_HIP = -3,       /* a HIP runtime call failed (see orbx_last_error)       */
  ORBX_ERR_CAPACITY = -4,  /* a result did not fit the capacity the caller gave     */
  ORBX_ERR_NUMERIC = -5,   /* BA: reduced system not positive definite (LU failure
                              in the reference, local_ba_lm.rs:1036-1039)           */
  ORBX_ERR_EMPTY = -6      /* BA: no parameters or no residuals -> reference returns
                              None (local_ba_lm.rs:923-925)                         */
};

/* = tracking::frame::CameraModel, src/tracking/frame/camera.rs:3-10 */
typedef struct {
  double fx, fy, cx, cy, baseline;
} orbx_camera;

/* = the nine cv::ORB::create arguments, src/tracking/frame/stereo.rs:38-48.
 * The reference's configuration and its neighbourhood are implemented: any n_features,
 * 1 <= n_levels <= 8, scale_factor in (1, 1.5], fast_threshold 1..254; edge_threshold 31,
 * first_level 0, wta_k 2, score_type 0 (HARRIS_SCORE), patch_size 31 are fixed;
 * other values -> ORBX_ERR_INVALID. */
typedef struct {
  int n_features;
  float scale_factor;
  int n_levels, edge_threshold, first_level, wta_k, score_type, patch_size, fast_threshold;
} orbx_orb_params;

/* = cv::KeyPoint as seen through opencv::core::KeyPoint (28 bytes) */
typedef struct {
  float x, y, size, angle, response;
  int octave, class_id;
} orbx_keypoint;

/* = cv::DMatch (16 bytes); field order of the Rust struct literal at stereo.rs:149-154 */
typedef struct {
  int query_idx, train_idx, img_idx;
  float distance;
} orbx_dmatch;

typedef struct orbx_handle orbx_handle;

const char* orbx_version(void);
/* Layout version of this header's structs and entry points: bumped whenever a struct grows or a signature changes (2: orbx_ba_window
 * gained `obs32`, so its array stride changed).  orbx_abi_version() is what the loaded library was built with; a caller compiled against
 * another ORBX_ABI_VERSION must not call it (the C++ and Python mirrors check at handle creation / load time, and the Rust shim of
 * INTEGRATION.md does the same in StereoProcessor::new). */
#define ORBX_ABI_VERSION 2
int orbx_abi_version(void);
const char* orbx_last_error(const orbx_handle* h);

/* Fills *p with the reference's ORB configuration (stereo.rs:38-48) for n_features. */
void orbx_default_orb_params(int n_features, orbx_orb_params* p);

/* Replaces StereoProcessor::new (stereo.rs:37-50).  `max_batch` = the largest number of
 * stereo pairs one *_batch_device call will carry (>= 1); max_w/max_h bound image size. */
int orbx_create(const orbx_camera* cam, const orbx_orb_params* orb, int device, int max_w,
                int max_h, int max_batch, orbx_handle** out);
void orbx_destroy(orbx_handle* h);

/* The handle's hipStream_t (as void*), so a host framework can order its own work
 * (copies, collectives) against the library's. */
void* orbx_stream(orbx_handle* h);
int orbx_synchronize(orbx_handle* h);

/* ---- per-frame feature pipeline ------------------------------------------------ */

/* Replaces StereoProcessor::process (stereo.rs:52-66) for one stereo pair held in host
 * memory: extract L, extract R (cv::ORB::detectAndCompute, stereo.rs:68-78), match
 * (stereo.rs:80-161), triangulate (stereo.rs:186-216).
 *   left/right: CV_8UC1 rows of `w` pixels, row strides in bytes.
 *   kpL/kpR [cap_kp], descL/descR [cap_kp*32], matches [cap_kp], points_cam [cap_kp*3],
 *   has_point [cap_kp] (1 = Some, 0 = None; points_cam is (0,0,0) where 0). */
int orbx_process_stereo(orbx_handle* h, const uint8_t* left, size_t lstride, const uint8_t* right,
                        size_t rstride, int w, int h_px, orbx_keypoint* kpL, uint8_t* descL,
                        int* nL, orbx_keypoint* kpR, uint8_t* descR, int* nR, int cap_kp,
                        orbx_dmatch* matches, int* n_matches, double* points_cam,
                        uint8_t* has_point);

/* Same path for `batch` stereo pairs resident in device memory (the throughput form).
 *   d_images: [batch][2][h_px][stride] u8, left then right of each pair.
 *   d_kp [batch][2][cap_kp], d_desc [batch][2][cap_kp][32], d_nkp [batch][2],
 *   d_matches [batch][cap_kp], d_nmatches [batch], d_points [batch][cap_kp][3],
 *   d_has_point [batch][cap_kp].
 * Asynchronous; call orbx_check_status (synchronises) before trusting the results. */
int orbx_process_stereo_batch_device(orbx_handle* h, const uint8_t* d_images, int batch, int w,
                                     int h_px, size_t stride, orbx_keypoint* d_kp,
                                     uint8_t* d_desc, int* d_nkp, int cap_kp,
                                     orbx_dmatch* d_matches, int* d_nmatches, double* d_points,
                                     uint8_t* d_has_point);

/* The same path for `batch` stereo pairs held in HOST memory (layouts as above, all arrays on the host).
 * The batch is cut into chunks of at most `max_batch` pairs; the upload of chunk i+1, the kernels of chunk i and
 * the download of chunk i-1 run concurrently on three HIP streams (double-buffered device staging).  The copies
 * only overlap when the host buffers are page-locked: allocate them with orbx_host_alloc (or register them).
 * Synchronous: returns when every result is in the host arrays. */
int orbx_process_stereo_batch(orbx_handle* h, const uint8_t* images, int batch, int w, int h_px,
                              size_t stride, orbx_keypoint* kp, uint8_t* desc, int* nkp, int cap_kp,
                              orbx_dmatch* matches, int* nmatches, double* points, uint8_t* has_point);
/* Page-locked host memory for the call above (hipHostMalloc / hipHostFree). */
void* orbx_host_alloc(size_t bytes);
void orbx_host_free(void* p);

/* Extraction alone (= detect_features, stereo.rs:68-78) for `n_images` device images
 * [n_images][h_px][stride]; outputs as above with one slot per image. */
int orbx_extract_batch_device(orbx_handle* h, const uint8_t* d_images, int n_images, int w,
                              int h_px, size_t stride, orbx_keypoint* d_kp, uint8_t* d_desc,
                              int* d_nkp, int cap_kp);

/* Synchronises the stream and returns the sticky device-side status of the calls
 * since the last check (ORBX_OK or ORBX_ERR_CAPACITY ...), then clears it. */
int orbx_check_status(orbx_handle* h);

/* ---- matchers ------------------------------------------------------------------- */

/* = StereoProcessor::match_features + triangulate (stereo.rs:80-161, 186-216) on feature
 * sets the caller already has (host memory).  Uses the handle's CameraModel. */
int orbx_stereo_match(orbx_handle* h, const orbx_keypoint* kpL, const uint8_t* descL, int nL,
                      const orbx_keypoint* kpR, const uint8_t* descR, int nR,
                      orbx_dmatch* matches, int* n_matches, double* points_cam,
                      uint8_t* has_point);

/* Device form, `batch` independent pairs; per-pair slots of cap_kp as in
 * orbx_process_stereo_batch_device. */
int orbx_stereo_match_batch_device(orbx_handle* h, int batch, const orbx_keypoint* d_kp,
                                   const uint8_t* d_desc, const int* d_nkp, int cap_kp,
                                   orbx_dmatch* d_matches, int* d_nmatches, double* d_points,
                                   uint8_t* d_has_point);

/* = BFMatcher::new(NORM_HAMMING, crossCheck=true).train_match(query, train)
 * (src/tracking/tracker.rs:1001-1010): mutual nearest neighbours, ascending query index,
 * lowest index wins distance ties.  q [nq][32], t [nt][32], out [nq] (host memory). */
int orbx_hamming_match_crosscheck(orbx_handle* h, const uint8_t* q, int nq, const uint8_t* t,
                                  int nt, orbx_dmatch* out, int* n_out);
int orbx_hamming_match_crosscheck_device(orbx_handle* h, const uint8_t* d_q, int nq,
                                         const uint8_t* d_t, int nt, orbx_dmatch* d_out,
                                         int* d_n_out);

/* = descriptor_distance (stereo.rs:166-175) over n_pairs rows: out[i] = popcount(a[i]^b[i])
 * over 32 bytes.  Host memory. */
int orbx_hamming_batch(orbx_handle* h, const uint8_t* a, const uint8_t* b, int n_pairs,
                       uint32_t* out);
int orbx_hamming_batch_device(orbx_handle* h, const uint8_t* d_a, const uint8_t* d_b, int n_pairs,
                              uint32_t* d_out);

/* Guided matching = FeatureGrid::new + get_features_in_area (src/tracking/tracking_frame.rs:52-128,
 * 64x48 cells over img_w x img_h) followed by the tracker's descriptor search over the candidates:
 *   mode 0  track_with_motion_model (src/tracking/tracker.rs:1126-1157): smallest distance < 100;
 *   mode 1  track_local_map (tracker.rs:880-923): best <= 100 and, with more than one candidate,
 *           best <= 0.75 * second.
 * Ties go to the first candidate in the reference's visiting order (cells row-major, keypoint index
 * ascending inside a cell).  kp/desc: the frame's n features; q_uv [nq][2] f64 projected positions,
 * q_desc [nq][32] map-point descriptors; out_idx [nq] = keypoint index or -1, out_dist [nq].
 * Keypoint and query coordinates must be finite.  Host and device forms. */
int orbx_guided_match(orbx_handle* h, const orbx_keypoint* kp, const uint8_t* desc, int n, double img_w,
                      double img_h, const double* q_uv, const uint8_t* q_desc, int nq, double radius,
                      int mode, int* out_idx, uint32_t* out_dist);
int orbx_guided_match_device(orbx_handle* h, const orbx_keypoint* d_kp, const uint8_t* d_desc, int n,
                             double img_w, double img_h, const double* d_q_uv, const uint8_t* d_q_desc,
                             int nq, double radius, int mode, int* d_out_idx, uint32_t* d_out_dist);

/* = search_for_triangulation (src/local_mapping/triangulation.rs:401-527): matches between the features of two
 * keyframes that have no map point yet, inside a 100-px grid neighbourhood (32-px cells), gated by the distance to
 * the epipole (features without stereo depth) and to the epipolar line (chi2 3.84), smallest Hamming distance
 * < max_dist, greedy one-to-one in ascending index of keyframe 1.
 *   mp1 [n1] / mp2 [n2]: 1 = the feature already has a map point; stereo1 [n1]: 1 = points_cam is Some;
 *   pose1_wc / pose2_wc: 7 doubles (qw,qx,qy,qz,tx,ty,tz), camera-to-world as the Map stores them;
 *   out_pairs [n1][2] = (idx1, idx2) ascending idx1.  Host memory.  Uses the camera given here (image size is
 *   2cx x 2cy as in the reference, :434-435).  A camera whose image has no 32-px cell (u32(2cx) or u32(2cy) == 0) is
 *   refused with ORBX_ERR_INVALID, here and in the device-resident and keyframe forms. */
int orbx_search_for_triangulation(orbx_handle* h, const orbx_camera* cam, const orbx_keypoint* kp1,
                                  const uint8_t* desc1, const uint8_t* mp1, const uint8_t* stereo1, int n1,
                                  const orbx_keypoint* kp2, const uint8_t* desc2, const uint8_t* mp2, int n2,
                                  const double* pose1_wc, const double* pose2_wc, unsigned max_dist,
                                  int* out_pairs, int* n_out);

/* Device-resident form: every array in device memory (keypoints and descriptors as the extractor left them), poses on the
 * host; asynchronous on the handle's stream.  d_pairs [n1][2], d_n_out [1]. */
int orbx_search_for_triangulation_device(orbx_handle* h, const orbx_camera* cam, const orbx_keypoint* d_kp1,
                                         const uint8_t* d_desc1, const uint8_t* d_mp1, const uint8_t* d_stereo1, int n1,
                                         const orbx_keypoint* d_kp2, const uint8_t* d_desc2, const uint8_t* d_mp2, int n2,
                                         const double* pose1_wc, const double* pose2_wc, unsigned max_dist,
                                         int* d_pairs, int* d_n_out);

/* = search_for_triangulation_bow (src/local_mapping/triangulation.rs:541-658): as above, but the candidates of a
 * feature are the features of keyframe 2 in the same FeatureVector node instead of a grid neighbourhood.
 *   node1 [n1] / node2 [n2]: the FeatureVector key of each feature (the out_node of orbx_bow_transform), 0xffffffff
 *   for a feature in no list.  The reference walks feat_vec1 in HashMap order; features of different nodes never
 *   compete, so the set of pairs does not depend on that order — here they come out in ascending idx1. */
int orbx_search_for_triangulation_bow(orbx_handle* h, const orbx_camera* cam, const orbx_keypoint* kp1,
                                      const uint8_t* desc1, const uint8_t* mp1, const uint8_t* stereo1,
                                      const uint32_t* node1, int n1, const orbx_keypoint* kp2, const uint8_t* desc2,
                                      const uint8_t* mp2, const uint32_t* node2, int n2, const double* pose1_wc,
                                      const double* pose2_wc, unsigned max_dist, int* out_pairs, int* n_out);

/* ---- ORB vocabulary (src/vocabulary/mod.rs) ------------------------------------------------------------------
 * orbx_vocab_load_text = OrbVocabulary::load_from_text (:117-211): DBoW2 text format, "k L scoring weighting" then
 * one line per node "parent_id is_leaf d0 .. d31 weight"; lines with fewer than 35 fields are skipped, a field that
 * does not parse fails the load (ORBX_ERR_INVALID + message), node ids are sequential from 1, a node is linked to its
 * parent only when the parent id is smaller than its own.  orbx_vocab_create takes the same nodes as arrays
 * (index 0 = root, ignored).  The tables live on the handle's device until orbx_vocab_destroy. */
typedef struct orbx_vocabulary orbx_vocabulary;
int orbx_vocab_load_text(orbx_handle* h, const char* path, orbx_vocabulary** out);
int orbx_vocab_create(orbx_handle* h, int n_nodes, const uint32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                      const double* weight, int k, int l, orbx_vocabulary** out);
void orbx_vocab_destroy(orbx_vocabulary* v);
int orbx_vocab_info(const orbx_vocabulary* v, int* k, int* l, int* n_nodes, int* n_words);   /* params/num_nodes/num_words */
int orbx_vocab_nodes(const orbx_vocabulary* v, uint32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight);

/* The per-descriptor part of OrbVocabulary::transform (:296-325): descent to the leaf taking the closest child at
 * every node (first child on ties, :230-248), then `levels_up` parents up (:262-275).
 *   out_word [n] word id (0 for a terminal node that is not flagged leaf, :247), out_leaf [n] leaf node id,
 *   out_node [n] FeatureVector key, out_weight [n] the leaf's weight.  BowVector = sum of out_weight per out_word,
 *   L1-normalised; FeatureVector = feature indices grouped by out_node — both left to the caller.
 * _device: descriptors and outputs in device memory, asynchronous on the handle's stream. */
int orbx_bow_transform(orbx_handle* h, const orbx_vocabulary* v, const uint8_t* desc, int n, int levels_up,
                       uint32_t* out_word, uint32_t* out_leaf, uint32_t* out_node, double* out_weight);
int orbx_bow_transform_device(orbx_handle* h, const orbx_vocabulary* v, const uint8_t* d_desc, int n, int levels_up,
                              uint32_t* d_word, uint32_t* d_leaf, uint32_t* d_node, double* d_weight);

/* The two maps OrbVocabulary::transform returns (mod.rs:296-325; transform_bow_only :327-355 is the first alone), built on the
 * device from the per-descriptor results above:
 *   BowVector     bow_word [n_bow] ascending word ids, bow_weight [n_bow]: per word the sum of its features' leaf weights in feature
 *                 order, then L1-normalised (:316-321; the norm is summed in ascending word order — the reference's HashMap order
 *                 is unspecified);
 *   FeatureVector fv_node [n_fv] ascending node ids, the features of node i = fv_index[fv_start[i] .. fv_start[i+1]) ascending.
 * Arrays are sized for n entries (fv_start n+1); at most 8192 descriptors per call.  _device: everything in device memory,
 * d_counts [2] = {n_bow, n_fv}, asynchronous.  orbx_bow_score = OrbVocabulary::score (:357-374) on two such BowVectors (host
 * arithmetic, no handle needed; word ids must ascend). */
int orbx_bow_vectors(orbx_handle* h, const orbx_vocabulary* v, const uint8_t* desc, int n, int levels_up, uint32_t* bow_word,
                     double* bow_weight, int* n_bow, uint32_t* fv_node, int* fv_start, int* fv_index, int* n_fv);
int orbx_bow_vectors_device(orbx_handle* h, const orbx_vocabulary* v, const uint8_t* d_desc, int n, int levels_up,
                            uint32_t* d_bow_word, double* d_bow_weight, uint32_t* d_fv_node, int* d_fv_start, int* d_fv_index,
                            int* d_counts);
int orbx_bow_score(const uint32_t* word1, const double* weight1, int n1, const uint32_t* word2, const double* weight2, int n2,
                   double* score);

/* = the search of fuse_points_into_keyframes (src/local_mapping/search_in_neighbors.rs:273-343, with
 * KeyFrame::get_features_in_area, src/atlas/map/keyframe.rs:408-443) for every (map point, target keyframe) pair:
 * project the point with the keyframe's inverse pose, skip it behind the camera or outside [0,2cx)x[0,2cy), radius
 * = clamp(radius_scale * depth / fx, 10, 50), best = smallest Hamming distance < desc_threshold among the keyframe's
 * keypoints inside the circle (lowest index on ties).  The map mutation that consumes the result (:345-383) stays
 * on the host; it changes neither positions nor descriptors, so all pairs can be searched up front.
 *   positions [P][3], mp_desc [P][32]; kf_poses_wc [T][7] (qw,qx,qy,qz,tx,ty,tz; the Map's camera-to-world pose);
 *   kf_feat_offset [T+1]: keyframe t owns kps/descs[kf_feat_offset[t] .. kf_feat_offset[t+1]);
 *   radius_scale = config.radius_factor * scale_factor.powi(num_levels - 1) (:303);
 *   out_idx [P][T] = feature index inside the keyframe or -1; out_dist [P][T] (0 where -1).  Host memory. */
int orbx_fuse_search(orbx_handle* h, const orbx_camera* cam, const double* positions, const uint8_t* mp_desc, int P,
                     const double* kf_poses_wc, const int* kf_feat_offset, const orbx_keypoint* kps, const uint8_t* descs,
                     int T, double radius_scale, unsigned desc_threshold, int* out_idx, uint32_t* out_dist);

/* Device-resident form of orbx_fuse_search: positions, descriptors, keypoints, offsets and outputs in device memory, the
 * keyframe poses on the host (they are inverted there); asynchronous on the handle's stream. */
int orbx_fuse_search_device(orbx_handle* h, const orbx_camera* cam, const double* d_positions, const uint8_t* d_mp_desc, int P,
                            const double* kf_poses_wc, const int* d_kf_feat_offset, const orbx_keypoint* d_kps,
                            const uint8_t* d_descs, int T, double radius_scale, unsigned desc_threshold, int* d_out_idx,
                            uint32_t* d_out_dist);

/* ---- keyframe hand-off with device-resident features (src/system/messages.rs:19-51) --------------------------------
 * orbx_keyframe = the payload of NewKeyFrameMsg — keyframe id, timestamp, T_wc pose, keypoints, descriptors, stereo points
 * (`points_cam`, None where has_point is 0) and the map-point associations (`matched_map_points`) — with the four feature
 * arrays held in device memory.  It is made straight from the device outputs of the extractor (device-to-device copies on the
 * handle's stream, asynchronous: slot `b` of orbx_process_stereo_batch_device is d_kp + b*2*cap_kp etc., n = nkp[b][0]), so the
 * features a frame was just given never leave the GPU between `process` and the searches local mapping runs on them.
 * The ids of the associations are map bookkeeping and stay on the host; the device holds the is_some() flags the searches
 * read.  d_points_cam / d_has_point may both be NULL (monocular: every point None).  A keyframe belongs to the handle
 * that made it and must be destroyed before it.  */
typedef struct orbx_keyframe orbx_keyframe;
int orbx_keyframe_create(orbx_handle* h, const orbx_keypoint* d_kp, const uint8_t* d_desc, int n, const double* d_points_cam,
                         const uint8_t* d_has_point, uint64_t keyframe_id, uint64_t timestamp_ns, const double* pose_wc,
                         orbx_keyframe** out);
void orbx_keyframe_destroy(orbx_keyframe* kf);
int orbx_keyframe_info(const orbx_keyframe* kf, int* n_features, uint64_t* keyframe_id, uint64_t* timestamp_ns, double* pose_wc);
int orbx_keyframe_set_pose(orbx_keyframe* kf, const double* pose_wc);                 /* after BA / pose refinement       */
int orbx_keyframe_set_map_points(orbx_keyframe* kf, const int64_t* mp_ids);           /* [n], -1 = None                   */
int orbx_keyframe_get_map_points(const orbx_keyframe* kf, int64_t* mp_ids);
/* host copies for consumers that still want Vector<KeyPoint> / Mat (any pointer may be NULL) */
int orbx_keyframe_download(const orbx_keyframe* kf, orbx_keypoint* kp, uint8_t* desc, double* points_cam, uint8_t* has_point);
const orbx_keypoint* orbx_keyframe_device_keypoints(const orbx_keyframe* kf);
const uint8_t* orbx_keyframe_device_descriptors(const orbx_keyframe* kf);
/* The searches on device-resident keyframes; semantics, tie rules and results exactly those of orbx_guided_match,
 * orbx_search_for_triangulation (kf1 = the new keyframe, its stereo flags = has_point; poses = the keyframes' own) and
 * orbx_fuse_search (radius_scale as there) — only the small inputs (queries, map points) and the results cross PCIe. */
int orbx_keyframe_guided_match(orbx_handle* h, const orbx_keyframe* kf, double img_w, double img_h, const double* q_uv,
                               const uint8_t* q_desc, int nq, double radius, int mode, int* out_idx, uint32_t* out_dist);
int orbx_keyframe_search_for_triangulation(orbx_handle* h, const orbx_camera* cam, const orbx_keyframe* kf1,
                                           const orbx_keyframe* kf2, unsigned max_dist, int* out_pairs, int* n_out);
int orbx_keyframe_fuse_search(orbx_handle* h, const orbx_camera* cam, const double* positions, const uint8_t* mp_desc, int P,
                              const orbx_keyframe* const* kfs, int T, double radius_scale, unsigned desc_threshold,
                              int* out_idx, uint32_t* out_dist);

/* ---- new map points from neighbour keyframes (src/local_mapping/triangulation.rs) ------------------------------------------
 * The pair loop of triangulate_from_neighbors (CreateNewMapPoints, :117-294): for every (idx1, idx2) a search returned — the
 * parallax test (:186-224), the choice between a DLT point and a stereo-depth point (:226-253), triangulate_dlt (:715-760; the
 * null vector of the 4x4 system by one-sided Jacobi in f64) and validate_triangulation (:776-850).  All arithmetic is f64 on the
 * device; keypoint coordinates are the f32 of orbx_keypoint widened. */
/* = TriangulationConfig, triangulation.rs:20-52.  num_neighbors and min_baseline_ratio are carried for the caller (the reference's
 * loop does not read them either); max_descriptor_dist goes to the search and must be <= 256 (the largest Hamming distance of two
 * 256-bit descriptors; the limit of orbx_search_for_triangulation's max_dist), else ORBX_ERR_INVALID. */
typedef struct {
  int num_neighbors;
  unsigned max_descriptor_dist;
  double min_baseline_ratio, min_parallax_inertial, min_parallax_visual, max_reproj_error_mono, max_reproj_error_stereo,
      scale_ratio_factor;
} orbx_triangulation_config;
/* 10, TH_LOW = 50, 0.01, acos(0.9996), acos(0.9998), 5.991, 7.8, 1.5 (:39-52) */
void orbx_default_triangulation_config(orbx_triangulation_config* cfg);
/* what became of a pair: out_status = ORBX_TRI_* | ORBX_TRI_METHOD_* << 8 */
enum {
  ORBX_TRI_CREATED = 0,          /* point accepted                                              */
  ORBX_TRI_SKIPPED = 1,          /* no triangulation method (:245, :252)                        */
  ORBX_TRI_DLT_DEGENERATE = 2,   /* |w| < 1e-10 (:751)                                          */
  ORBX_TRI_REJ_DEPTH = 3,        /* depth not positive in a camera (:794)                       */
  ORBX_TRI_REJ_REPROJ1 = 4,      /* reprojection error in camera 1 (:808)                       */
  ORBX_TRI_REJ_REPROJ2 = 5,      /* ... in camera 2 (:821)                                      */
  ORBX_TRI_REJ_DIST = 6,         /* closer than 1e-6 to a camera centre (:831)                  */
  ORBX_TRI_REJ_SCALE = 7,        /* distance ratio against octave ratio (:843)                  */
  ORBX_TRI_BAD_INDEX = 8         /* device form: pair index out of range, nothing was read      */
};
enum { ORBX_TRI_METHOD_DLT = 0, ORBX_TRI_METHOD_STEREO_CURRENT = 1, ORBX_TRI_METHOD_STEREO_NEIGHBOUR = 2 };
/* Pairs from any search (orbx_search_for_triangulation[_bow], ...) between keyframe 1 (the current one) and keyframe 2.
 *   kp [n], points_cam [n][3] + has_point [n] (1 = Some; both may be NULL: every point None), pose_wc [7] (qw,qx,qy,qz,tx,ty,tz);
 *   pairs [n_pairs][2] = (idx1, idx2); out_points [n_pairs][3] (the point wherever one was formed, else 0), out_status [n_pairs].
 * The host form rejects an index out of range with ORBX_ERR_INVALID; the device form (every array in device memory, poses on the
 * host, asynchronous on the handle's stream) marks such a pair ORBX_TRI_BAD_INDEX without reading anything for it. */
int orbx_triangulate_pairs(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                           const orbx_keypoint* kp1, const double* points_cam1, const uint8_t* has_point1, int n1, const double* pose1_wc,
                           const orbx_keypoint* kp2, const double* points_cam2, const uint8_t* has_point2, int n2, const double* pose2_wc,
                           const int* pairs, int n_pairs, double* out_points, uint16_t* out_status);
int orbx_triangulate_pairs_device(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                                  const orbx_keypoint* d_kp1, const double* d_points_cam1, const uint8_t* d_has_point1, int n1,
                                  const double* pose1_wc, const orbx_keypoint* d_kp2, const double* d_points_cam2,
                                  const uint8_t* d_has_point2, int n2, const double* pose2_wc, const int* d_pairs, int n_pairs,
                                  double* d_out_points, uint16_t* d_out_status);
/* The keyframe's FeatureVector as one node id per feature (the out_node of orbx_bow_transform, 0xffffffff = in no list): the
 * encoding orbx_search_for_triangulation_bow takes.  The keyframe keeps a host copy and the node-sorted index the search needs.
 * NULL clears it. */
int orbx_keyframe_set_feature_nodes(orbx_keyframe* kf, const uint32_t* node);
/* triangulate_from_neighbors (:71-308) for a device-resident current keyframe and its T <= 256 neighbours, in the given order, in
 * one call: the host does the baseline test (:137-141) and the epipolar geometry; the device then runs the T searches side by side
 * (the FeatureVector form where both keyframes carry nodes, :145, else the grid form; max_dist = cfg->max_descriptor_dist), the pair
 * loop over every match, and an ordered compaction of the accepted points — one upload, one download, one synchronisation.  The
 * searches read the current keyframe's map-point flags as they are at the call (the reference clones them before the loop, :94-107).
 *   out_neighbour / out_idx1 / out_idx2 [cap], out_points [cap][3]: the new points in the reference's creation order (neighbour,
 *   then the search's pair order); *n_out: how many there are — when it exceeds cap only the first cap were written and the caller
 *   calls again with more room (the convention of orbx_kfdb_detect_loop_candidates).
 *   stats [T][4] = searched (0: skipped by the baseline test or an empty keyframe), matches_found, triangulated, validated.
 * The caller then does create_map_point + the two associate calls per entry, in list order (:286-290). */
int orbx_keyframe_triangulate_from_neighbors(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                                             const orbx_keyframe* kf_current, const orbx_keyframe* const* kfs, int T, int cap,
                                             int* out_neighbour, int* out_idx1, int* out_idx2, double* out_points, int* n_out, int* stats);

/* ---- input side (src/io/euroc.rs) ------------------------------------------------------------------------------
 * Host code: the EuRoC `mav0` reader of EurocDataset::new / len / frame_timestamp / stereo_pair (:64-132,
 * load_image_list :189-211, the camera part of load_stereo_calibration :325-360) and the PNG decode that
 * cv::imread(IMREAD_GRAYSCALE) does there.  No GPU involved; outputs feed orbx_process_stereo[_batch].
 *   orbx_png_decode_gray8: non-interlaced greyscale PNG (8 or 16 bit, optional alpha) -> 8-bit rows; out == NULL
 *     returns only the size.  Anything else (palette, RGB, interlaced, damaged) is ORBX_ERR_INVALID.
 *   orbx_euroc_open: ORBX_ERR_INVALID + message in err where the reference returns Err (missing file, a timestamp
 *     that does not parse, records of different lengths, cam0/cam1 of different lengths, bad yaml).
 *   orbx_euroc_calibration: left = {fx, fy, cx, cy of cam0, baseline = |t(T_cam1_body * T_cam0_body^-1)|}.
 *   orbx_euroc_read_pairs: frames [first, first+count) decoded by `threads` host threads into out[pair][2][h][w],
 *     the layout orbx_process_stereo_batch takes (use orbx_host_alloc memory to overlap the upload). */
typedef struct orbx_euroc orbx_euroc;
int orbx_png_decode_gray8(const uint8_t* file, size_t n, uint8_t* out, size_t stride, int* w, int* h);
int orbx_euroc_open(const char* mav0_dir, orbx_euroc** out, char* err, size_t err_cap);
void orbx_euroc_close(orbx_euroc* d);
int orbx_euroc_len(const orbx_euroc* d);
const char* orbx_euroc_last_error(const orbx_euroc* d);
int orbx_euroc_frame_timestamp(const orbx_euroc* d, int idx, uint64_t* timestamp_ns);
int orbx_euroc_calibration(const orbx_euroc* d, orbx_camera* left, double* k_right4, int* w, int* h);
int orbx_euroc_read_pairs(orbx_euroc* d, int first, int count, uint8_t* out, int threads);

/* ---- local bundle adjustment ------------------------------------------------------ */

/* = LocalBAConfigLM, src/optimizer/local_ba_lm.rs:96-119 */
typedef struct {
  int max_iterations;
  double param_tolerance, gradient_tolerance, huber_threshold;
  int max_covisible_keyframes;
} orbx_ba_config;

/* One VisualObservation (local_ba_lm.rs:68-78) after the id -> index re-keying the
 * reference does at :928-961.  kf_idx >= 0: optimised keyframe (is_kf_optimized);
 * kf_idx < 0: fixed keyframe `fixed_idx` (fixed_idx < 0 = unknown id -> identity pose,
 * local_ba_lm.rs:569).  _pad: 0 for the visual solvers; bit 0 = is_stereo for orbx_ba_solve_inertial. */
typedef struct {
  int32_t kf_idx, fixed_idx, mp_idx, _pad;
  double u, v;
} orbx_ba_obs;

void orbx_default_ba_config(orbx_ba_config* c);

/* = `&dyn Fn() -> bool` of solve_visual_ba; polled once at the top of each LM iteration
 * (local_ba_lm.rs:1013).  NULL = never stop. */
typedef int (*orbx_should_stop_fn)(void* user);

/* Collective hook for the point-partitioned multi-GPU form: sum `n`
 * doubles at device pointer `d_buf` in place over all ranks, ordered on `hip_stream`.
 * The host framework implements it (torch.distributed / RCCL).  NULL = single GPU. */
typedef int (*orbx_allreduce_fn)(void* user, void* d_buf, size_t n, void* hip_stream);
int orbx_ba_set_allreduce(orbx_handle* h, orbx_allreduce_fn fn, void* user);

/* The native collective of the point-partitioned solve: RCCL over xGMI, called by the library itself —
 * ncclAllReduce(ncclDouble, ncclSum) in place on the handle's stream — so a Rust (or C) host
 * needs no framework around it.  Either
 *   orbx_rccl_unique_id (rank 0; = ncclGetUniqueId, returns the id's size, 128) + the host's own way of handing the id to
 *   the other ranks + orbx_ba_init_rccl on every rank (= ncclCommInitRank; the library owns the communicator, one per
 *   handle, destroyed with it), or
 *   orbx_ba_set_rccl_comm with an ncclComm_t the host already has (caller-owned; NULL clears).
 * A communicator takes precedence over the orbx_ba_set_allreduce hook, which stays for hosts that bring another transport
 * (the CPU tests run it over gloo).  Every rank must call the solve with the same problem and its own partition; all
 * ranks issue the same sequence of collectives whatever their own should_stop() answers: the stop decision is part of
 * what is reduced (one rank asking is enough, and all ranks then stop before the same iteration), and so is "some rank
 * holds an observation with an index out of range" (every rank returns ORBX_ERR_INVALID). */
int orbx_rccl_unique_id(uint8_t* out, size_t cap);
int orbx_ba_init_rccl(orbx_handle* h, const uint8_t* unique_id, size_t id_bytes, int rank, int world);
int orbx_ba_set_rccl_comm(orbx_handle* h, void* nccl_comm);
/* What would carry the all-reduces of a partitioned solve on this handle right now: bit 0 = an RCCL communicator
 * (orbx_ba_init_rccl / orbx_ba_set_rccl_comm), bit 1 = the orbx_ba_set_allreduce hook; 0 = none — orbx_ba_solve_visual then
 * treats the observations it is given as the WHOLE problem, so a host that partitions must check before it calls.
 * librccl is bound on first use of the three calls above (dlopen by soname: a process that already mapped a librccl.so.1,
 * e.g. PyTorch's, gets that copy); a single-GPU process never loads it. */
int orbx_ba_has_collective(orbx_handle* h);
/* What the handle's RCCL communicator spans, from the communicator itself (ncclCommCount / ncclCommUserRank): the number of ranks its
 * all-reduce sums over and this rank's index.  ORBX_ERR_INVALID without a communicator.  (bench.py prints it, so that a multi-GPU record
 * shows how many ranks RCCL really saw.) */
int orbx_ba_rccl_world(orbx_handle* h, int* n_ranks, int* rank);

/* Replaces solve_visual_ba (local_ba_lm.rs:912-1098).
 *   poses_cw [K][7]  (qw,qx,qy,qz,tx,ty,tz) T_cw of the optimised keyframes (:966-977)
 *   fixed_poses_cw [F][7]  T_cw of anchor + other fixed observers
 *   points [M][3] in/out   map-point positions (:980-987 / :1079-1089)
 *   obs [N]
 *   poses_wc_out [K][7]    optimised poses inverted back to T_wc (:1062-1077)
 * Everything is f64.  With an allreduce hook set, `obs` holds this rank's partition of the
 * observations (all observations of the points it owns); poses, points and the scalars come
 * out identical on every rank. */
int orbx_ba_solve_visual(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                         const double* poses_cw, int F, const double* fixed_poses_cw, int M,
                         double* points, int N, const orbx_ba_obs* obs,
                         orbx_should_stop_fn should_stop, void* user, double* poses_wc_out,
                         int* iterations, double* initial_error, double* final_error);

/* The same observation in 16 bytes, for callers whose pixel coordinates ARE f32 — the reference's always are: collect_visual_ba_data
 * widens `kp.pt()` (cv::Point2f) to f64 per observation (local_ba_lm.rs:870-872).  The library widens on the device instead, the same
 * exact conversion, so results are bit-identical to handing over the widened orbx_ba_obs — and half the bytes cross PCIe (the upload of
 * the observations is a fifth of a 32-window batch call).  kf_idx >= 0: optimised keyframe; kf_idx < 0: fixed observer -1 - kf_idx
 * (F = the identity pose, as fixed_idx -1 of orbx_ba_obs). */
typedef struct {
  int32_t kf_idx, mp_idx;
  float u, v;
} orbx_ba_obs32;
/* orbx_ba_solve_visual with the observations in the 16-byte form orbx_ba_obs32: f32 pixel coordinates — what the reference's are,
 * `kp.pt()` widened per observation at collect time (local_ba_lm.rs:870-872) — widened on the device, the same exact conversion, so the
 * result equals orbx_ba_solve_visual's on the widened observations bit for bit while half the bytes cross the host link (a 50-keyframe
 * window carries 2*10^5 observations: 3.2 MB instead of 6.5).  Not with an all-reduce hook / communicator installed: the partitioned
 * solve takes orbx_ba_obs. */
int orbx_ba_solve_visual_obs32(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                               const double* poses_cw, int F, const double* fixed_poses_cw, int M,
                               double* points, int N, const orbx_ba_obs32* obs32,
                               orbx_should_stop_fn should_stop, void* user, double* poses_wc_out,
                               int* iterations, double* initial_error, double* final_error);

/* orbx_ba_solve_visual_obs32 with the observations in DEVICE memory of the handle's device (16-byte aligned), written by work already
 * ordered on the handle's stream — orbx_map_collect_ba_window_device's d_obs32, or the caller's own kernels after orbx_synchronize.
 * They are copied device to device into the solver's blob, where the index checks, the grouping and the per-keyframe lists are made
 * as for host observations: the same kernels see the same bytes, so every output equals orbx_ba_solve_visual_obs32's on a host copy
 * bit for bit, and nothing crosses the host link but poses and points.  Poses, points and the scalars stay host arrays.  Not with an
 * all-reduce hook / communicator installed (the partitioned solve's host passes read the observations): ORBX_ERR_INVALID.  An
 * observation index out of range is ORBX_ERR_INVALID as ever; the message names the observation, not its contents. */
int orbx_ba_solve_visual_obs32_device(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                                      const double* poses_cw, int F, const double* fixed_poses_cw, int M,
                                      double* points, int N, const orbx_ba_obs32* d_obs32,
                                      orbx_should_stop_fn should_stop, void* user, double* poses_wc_out,
                                      int* iterations, double* initial_error, double* final_error);

/* Many independent windows in ONE call ("many BA windows": one map per stream / per robot).  Each
 * window is exactly one orbx_ba_solve_visual problem (same arguments, same LM loop, local_ba_lm.rs:1012-1056) with its own
 * LM state on the device; all windows share every kernel launch — the window is the second grid dimension — so W reduced
 * systems are factored by W workgroups at once and the point / keyframe / Schur kernels of all windows fill the chip
 * together, instead of one window's chain of short launches using about 1 % of it.  Nothing is exchanged between windows,
 * and a window's arithmetic does not depend on what else is in the batch: every window's result equals the result of
 * orbx_ba_solve_visual on it bit for bit.  Windows may differ in size.  should_stop is polled once per iteration for the
 * whole batch (and while the work drains); a window that converges early simply stops taking part.
 *   status: ORBX_OK, or ORBX_ERR_EMPTY for a window the reference answers None for (:923-925) — the call still returns
 *   ORBX_OK and solves the others (also when that window is the only one of the batch).  An observation index out of range fails
 *   the whole call (ORBX_ERR_INVALID): every window's status then carries the error, and the in/out `points` / `poses_wc_out` of
 *   windows that had already finished (the other half of a two-stream batch) hold their results — hand in the original points
 *   again when retrying.  No C++ exception leaves this call or any other orbx_ba_* entry point: allocation or thread-creation failure is an error code.
 * The all-reduce hook / RCCL communicator is not used here (independent windows need no collective).
 * A batch of 16 or more windows without a should_stop callback runs as two halves at once: the second half on an internal second
 * stream with its own workspaces, driven by a helper thread for the duration of the call, so that one half's host preprocessing and
 * transfers run under the other half's kernels (+12 % LM iterations/s at 32 windows); the halves are cut where the observation
 * count is halved; if the second stream cannot be created the whole batch runs on the first.  Results do not depend on it.  With a callback
 * (which would otherwise be called from two threads), or with per-kernel profiling on, the call keeps to one stream.
 * Observations are handed over as they are: the index checks, the per-point grouping and the per-keyframe lists are made on the
 * device (four short launches per call shared by all windows), so the host makes no pass over them.  If `obs` lies in page-locked host
 * memory (orbx_host_alloc, hipHostMalloc or a registered range — the library asks the runtime) the copy engine reads it where it lies;
 * windows whose `obs` arrays follow each other in memory travel as ONE copy.  Pageable `obs` is first copied into the handle's pinned
 * staging blob (a plain copy, on worker threads when large).  The same holds for the one-window entry points. */

typedef struct {
  int K;                        /* in: optimised keyframes                         */
  const double* poses_cw;       /* in: [K][7]                                      */
  int F;
  const double* fixed_poses_cw; /* in: [F][7]                                      */
  int M;
  double* points;               /* in/out: [M][3]                                  */
  int N;
  const orbx_ba_obs* obs;       /* in: [N] (or NULL when obs32 is given)           */
  double* poses_wc_out;         /* out: [K][7]                                     */
  int status;                   /* out                                             */
  int iterations;               /* out                                             */
  double initial_error, final_error;   /* out                                      */
  const orbx_ba_obs32* obs32;   /* in: [N], optional: used instead of obs when not NULL */
} orbx_ba_window;
int orbx_ba_solve_visual_batch(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int n_windows,
                               orbx_ba_window* windows, orbx_should_stop_fn should_stop, void* user);

/* Replaces solve_global_ba (src/optimizer/global_ba.rs:184-418): the same LM loop over ALL keyframes of the map
 * with the first one (smallest id, :116-119) fixed, and one difference in the linearisation — an observation whose
 * point is not in front of its camera (z_c <= 0.001) keeps its 100-px residual but contributes zero Jacobian rows
 * (:561-563).
 *   poses_cw [K][7]: T_cw of the K = n_kfs - 1 optimised keyframes in kf_ids order with the fixed one removed
 *   (:214-220); fixed_pose_cw [7]: T_cw of the fixed keyframe; obs[i].kf_idx < 0 (fixed_idx 0) marks it.
 *   Tolerances come from cfg (GlobalBAConfig defaults: 10 iterations, 1e-6, 1e-6, sqrt(5.991), :36-45).
 *   poses_wc_out [K][7]; the fixed keyframe's result is its input pose (:386).
 * ORBX_ERR_EMPTY where the reference returns None (:194-196, :207-209) and for N = 0, which
 * collect_global_ba_data never produces (:176-178).  The all-reduce hook applies as in orbx_ba_solve_visual. */
int orbx_ba_solve_global(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                         const double* poses_cw, const double* fixed_pose_cw, int M, double* points, int N,
                         const orbx_ba_obs* obs, orbx_should_stop_fn should_stop, void* user,
                         double* poses_wc_out, int* iterations, double* initial_error, double* final_error);

/* orbx_ba_solve_global with 16-byte observations (see orbx_ba_solve_visual_obs32): kf_idx -1 marks the fixed keyframe. */
int orbx_ba_solve_global_obs32(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                               const double* poses_cw, const double* fixed_pose_cw, int M, double* points, int N,
                               const orbx_ba_obs32* obs32, orbx_should_stop_fn should_stop, void* user,
                               double* poses_wc_out, int* iterations, double* initial_error, double* final_error);

/* Global BA over a whole map: orbx_ba_solve_global's arguments and semantics, word for word, on a path of its own that holds more
 * optimised keyframes than the local-window solver's 128 — any 1 <= K <= orbx_ba_global_map_max_keyframes() (2048: the reduced system
 * [6K + 1][6K] f64 in device memory is 1.2 GB there; the workspaces belong to the handle, grow on demand and are sized by the call's K,
 * M and N, never by the cap).  A larger K is ORBX_ERR_INVALID before anything is enqueued; a failed allocation is ORBX_ERR_HIP.
 * The calls always take this path, also for small K.  ORBX_ERR_EMPTY for K < 1, M == 0 or N == 0; ORBX_ERR_INVALID for an observation
 * index out of range (the message names the observation, poses_wc_out and points are left untouched); should_stop is polled once per
 * iteration; an iteration whose reduced system has a pivot that is not positive ends the solve with the parameters it started from.
 * Every sum has a fixed order: two runs give the same bits.  Not partitioned: with an all-reduce hook or communicator installed the
 * calls answer ORBX_ERR_INVALID.
 *   _obs32: 16-byte observations, kf_idx -1 marks the fixed keyframe; _obs32_device: the same array in device memory of the handle's
 *   device (16-byte aligned), written by work already enqueued on the handle's stream. */
int orbx_ba_solve_global_map(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                             const double* poses_cw, const double* fixed_pose_cw, int M, double* points, int N,
                             const orbx_ba_obs* obs, orbx_should_stop_fn should_stop, void* user,
                             double* poses_wc_out, int* iterations, double* initial_error, double* final_error);
int orbx_ba_solve_global_map_obs32(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                                   const double* poses_cw, const double* fixed_pose_cw, int M, double* points, int N,
                                   const orbx_ba_obs32* obs32, orbx_should_stop_fn should_stop, void* user,
                                   double* poses_wc_out, int* iterations, double* initial_error, double* final_error);
int orbx_ba_solve_global_map_obs32_device(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K,
                                          const double* poses_cw, const double* fixed_pose_cw, int M, double* points, int N,
                                          const orbx_ba_obs32* d_obs32, orbx_should_stop_fn should_stop, void* user,
                                          double* poses_wc_out, int* iterations, double* initial_error, double* final_error);
int orbx_ba_global_map_max_keyframes(void);

/* LocalInertialBAConfig (src/optimizer/local_inertial_ba.rs:109-141); orbx_default_inertial_ba_config = its Default:
 * 10 iterations, window 10, sqrt(5.991), sqrt(7.815), lambda 1e-2, gyro random-walk information 1e6, accel 1e4. */
typedef struct {
  int max_iterations;
  int window_size;               /* used by the caller when it collects the temporal window (:366-384) */
  double huber_threshold_mono, huber_threshold_stereo;
  double initial_lambda;
  double gyro_rw_info, accel_rw_info;
} orbx_inertial_ba_config;
void orbx_default_inertial_ba_config(orbx_inertial_ba_config* cfg);

/* Replaces solve_inertial_ba (src/optimizer/local_inertial_ba.rs:1074-1275): visual-inertial local BA over the K
 * keyframes of the temporal window, 15 parameters each (T_wc pose as axis-angle + translation, velocity, gyro bias,
 * accel bias), plus M map points.  Residuals: reprojection (Huber, threshold per observation mono/stereo,
 * obs[i]._pad bit 0 = is_stereo; 100-px penalty and no Jacobian where z_c <= 0.001), the 9-d preintegration
 * residual of imu_factors.rs:66-103 per IMU edge with forward-difference Jacobians (eps 1e-6, :806-861), and the
 * 6-d bias random walk per edge (:676-698).  LM as :1198-1243: initial lambda from cfg, stop on |gradient| < 1e-8
 * or a singular system, no step-size test; errors are |r| (not RMS).
 *   poses_wc [K][7], velocities [K][3], biases [K][6] (gyro xyz, accel xyz); fixed_poses_cw [F][7] (T_cw);
 *   obs: kf_idx = index into the window or -1 (+ fixed_idx); edge_kf [E][2] window indices (i earlier, j later);
 *   preint [E][11] = delta_rot (qw,qx,qy,qz), delta_vel, delta_pos, dt of PreintegratedState (preintegration.rs:85-98).
 *   The edges are any list of index pairs: i > j as well as i < j (earlier / later is time, not index order), in any
 *   order, E = 0, keyframes without an edge, a pair listed twice (its terms are then added twice, as the reference's
 *   loop over imu_edges does).  The two ends of an edge are DISTINCT keyframes: an edge with i == j is refused with
 *   ORBX_ERR_INVALID ("IMU edge %d: both ends are keyframe %d") before anything is enqueued — the reference never
 *   builds one (it pairs opt_kf_ids[i] with opt_kf_ids[i + 1]), and the entries of its 18 x 18 block would fall on
 *   each other in the system.  (orbx_debug_imu_residual, which assembles nothing, takes such an edge.)
 *   Outputs for ALL K keyframes (the reference's result maps skip index 0, :1250 — the caller's business).
 * ORBX_ERR_EMPTY where the reference returns None (K < 2, :1080-1082). */
int orbx_ba_solve_inertial(orbx_handle* h, const orbx_camera* cam, const orbx_inertial_ba_config* cfg, int K,
                           const double* poses_wc, const double* velocities, const double* biases, int F,
                           const double* fixed_poses_cw, int M, double* points, int N, const orbx_ba_obs* obs, int E,
                           const int* edge_kf, const double* preint, orbx_should_stop_fn should_stop, void* user,
                           double* poses_wc_out, double* vel_out, double* bias_out, int* iterations,
                           double* initial_error, double* final_error);

/* orbx_ba_solve_inertial with the observations in the 16-byte form.  kf_idx as in orbx_ba_obs32: >= 0 the window keyframe, < 0 the
 * fixed observer -1 - kf_idx (F = the identity pose).  is_stereo, which orbx_ba_obs carries in bit 0 of _pad, rides in mp_idx:
 * mp_idx & ORBX_BA_OBS32_STEREO is the flag and mp_idx & ~ORBX_BA_OBS32_STEREO the point index, so M >= 0x40000000 is refused
 * (ORBX_ERR_INVALID).  ONLY the inertial entry points read the bit: the visual and global forms take mp_idx whole, where a set bit
 * is an index out of range.  The decode is made on the device in the passes that group the observations; every kernel behind them
 * sees the same values, so all outputs equal orbx_ba_solve_inertial's on the widened observations (flag in _pad) bit for bit.
 * _device: d_obs32 is DEVICE memory of the handle's device (16-byte aligned), written by work already ordered on the handle's
 * stream — orbx_map_collect_inertial_window_device's d_obs32; an index out of range names the observation, not its contents.
 * Everything else — edges, refusals, ORBX_ERR_EMPTY, outputs for all K keyframes — is orbx_ba_solve_inertial's. */
#define ORBX_BA_OBS32_STEREO 0x40000000
int orbx_ba_solve_inertial_obs32(orbx_handle* h, const orbx_camera* cam, const orbx_inertial_ba_config* cfg, int K,
                                 const double* poses_wc, const double* velocities, const double* biases, int F,
                                 const double* fixed_poses_cw, int M, double* points, int N, const orbx_ba_obs32* obs32, int E,
                                 const int* edge_kf, const double* preint, orbx_should_stop_fn should_stop, void* user,
                                 double* poses_wc_out, double* vel_out, double* bias_out, int* iterations,
                                 double* initial_error, double* final_error);
int orbx_ba_solve_inertial_obs32_device(orbx_handle* h, const orbx_camera* cam, const orbx_inertial_ba_config* cfg, int K,
                                        const double* poses_wc, const double* velocities, const double* biases, int F,
                                        const double* fixed_poses_cw, int M, double* points, int N, const orbx_ba_obs32* d_obs32,
                                        int E, const int* edge_kf, const double* preint, orbx_should_stop_fn should_stop,
                                        void* user, double* poses_wc_out, double* vel_out, double* bias_out, int* iterations,
                                        double* initial_error, double* final_error);

/* ---- PnP-RANSAC pose estimation (src/geometry/pnp.rs) --------------------------------------------------------
 * Replaces solve_pnp_ransac / solve_pnp_ransac_detailed (pnp.rs:29-134): cv::solvePnPRansac(100 iterations, 8 px,
 * confidence 0.99, SOLVEPNP_ITERATIVE, useExtrinsicGuess = prior given) + Rodrigues, the result inverted back to T_wc, then the
 * per-correspondence reprojection error sqrt(du^2 + dv^2) (+inf where the camera-frame z <= 0) and the mask err < reproj_error.
 * OpenCV's internals are not reproduced; the library implements a specification with OpenCV's structure:
 *   [spec] a counter-based sampler (splitmix64 of seed + 0x9E3779B97F4A7C15 * (h*64 + a + 1); index = ((z >> 32) * n) >> 32;
 *          duplicates skipped, 64 draws at most), so that a problem's result does not depend on the batch around it;
 *   [spec] hypotheses by Levenberg-Marquardt on each model_points sample starting from the prior (every reference call site
 *          passes one) instead of EPnP: left perturbation, the visual BA's pose block, lambda 1e-3 and the project's damping rule;
 *   OpenCV's inlier test (float)(du^2 + dv^2) <= (float)reproj_error^2, its sequential best-model walk with RANSACUpdateNumIters
 *   (applied after all hypotheses were scored in parallel), and a final LM over the best model's inliers (refine_iterations);
 *   [spec] 4 <= n <= model_points: one hypothesis from all points; n < 4: TOO_FEW; no model: NO_MODEL and the prior's bytes back.
 * Poses are 7 doubles (qw,qx,qy,qz,tx,ty,tz), camera-to-world as the reference passes them. */
enum {
  ORBX_PNP_OK = 0,
  ORBX_PNP_NO_MODEL = 1,     /* no hypothesis passed the walk: pose = prior (the reference ignores solvePnPRansac's bool) */
  ORBX_PNP_TOO_FEW = 2,      /* n < 4: pose = prior (the callers guard n < 4 / n < 10 themselves)                         */
  ORBX_PNP_OVER_MAX_N = 3    /* device form: n > max_n: pose = prior                                                   */
};
/* orbx_default_pnp_config: max_iterations 100, reproj_error 8.0, confidence 0.99 (pnp.rs:71-84), model_points 5 (OpenCV's
 * model size for SOLVEPNP_ITERATIVE), hypothesis_iterations 10, refine_iterations 20 (OpenCV's extrinsic LM), seed 0.
 * Accepted ranges: 1 <= max_iterations <= 1024, 4 <= model_points <= 8, reproj_error > 0, 0 <= confidence <= 1, iteration counts
 * 0..1000; other values -> ORBX_ERR_INVALID. */
typedef struct {
  int max_iterations;
  double reproj_error, confidence;
  int model_points, hypothesis_iterations, refine_iterations;
  uint64_t seed;
} orbx_pnp_config;
/* One problem's record.  n_inliers: of the final mask (err < reproj_error); ransac_inliers: the best hypothesis' count under
 * OpenCV's test; hypotheses_evaluated: where the sequential walk ended (OpenCV's iteration count); refine_iterations: LM
 * iterations of the final refinement; final_rms: sqrt(mean err^2) over the final inliers (0 without any). */
typedef struct {
  int status, n_inliers, ransac_inliers, best_hypothesis, hypotheses_evaluated, refine_iterations;
  double final_rms;
} orbx_pnp_result;
void orbx_default_pnp_config(orbx_pnp_config* cfg);

/* One problem in host memory, synchronous.  pts3d [n][3] f64 world points, pts2d [n][2] f32 pixels (cv::Point2f), prior_wc [7]
 * (required: every reference call site passes Some), pose_wc_out [7], inlier_out [n] u8 (1 = inlier), err_out [n] f64,
 * result [1].  Every buffer is the caller's; the library copies in and out. */
int orbx_pnp_ransac(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* cfg, int n, const double* pts3d,
                    const float* pts2d, const double* prior_wc, double* pose_wc_out, uint8_t* inlier_out, double* err_out,
                    orbx_pnp_result* result);
/* n_problems independent problems in host memory, one upload and one download: problem p owns correspondences
 * [offsets[p], offsets[p+1]) of pts3d / pts2d / inlier_out / err_out (offsets [n_problems+1], ascending, offsets[0] = 0);
 * priors_wc / poses_wc_out [n_problems][7], results [n_problems].  Each problem's result equals orbx_pnp_ransac on it, byte for
 * byte.  Synchronous; caller-owned buffers. */
int orbx_pnp_ransac_batch(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* cfg, int n_problems, const int* offsets,
                          const double* pts3d, const float* pts2d, const double* priors_wc, double* poses_wc_out,
                          uint8_t* inlier_out, double* err_out, orbx_pnp_result* results);
/* The same with every array in device memory (the caller's; the library only reads the inputs and writes the outputs),
 * asynchronous on the handle's stream.  max_n: a host-known bound on the correspondences of one problem (it sizes the scoring
 * launch); a problem with more gets ORBX_PNP_OVER_MAX_N and its prior, with the detailed pass still computed.  d_offsets must be
 * ascending from 0 (they are trusted: they index the point arrays). */
int orbx_pnp_ransac_batch_device(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* cfg, int n_problems, int max_n,
                                 const int* d_offsets, const double* d_pts3d, const float* d_pts2d, const double* d_priors_wc,
                                 double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out, orbx_pnp_result* d_results);

/* ---- pose-inertial optimization for tracking (src/optimizer/pose_inertial_optim.rs) ------------------------------
 * pose_inertial_optimization (:94-216), as the tracker's refine_with_imu calls it (src/tracking/tracker.rs:476-546): the current
 * frame's 15 parameters [scaled_axis(q_wc) | t_wc | v | b_g | b_a] refined against fixed map points and the IMU preintegration
 * from the previous keyframe.  Per iteration (at most max_iterations): chi2 thresholds interpolated from *_init to *_final; two
 * visual rows per masked-in observation, e = uv - proj(T_wc^-1 X) with the reference's 2x6 camera-frame block (:250-349; (100,100)
 * and a zero block where z_c <= 0.001); the 9 rows of compute_imu_residual times imu_weight with a forward-difference Jacobian over
 * all 15 parameters (eps 1e-6); fewer than 5 masked-in observations end the loop before the solve; H = J^T J damped by
 * H_ii += 1e-3 max(H_ii, 1e-6), solved by partial-pivoting LU (an exactly zero pivot ends the loop); params += delta; every
 * observation reclassified: inlier = |e|^2 < (is_stereo ? chi2_stereo : chi2_mono).  Gravity (0, 0, -9.81).  The residual does
 * not depend on the bias, so the bias comes back with its input value.  The reference's visual block is the true derivative only
 * at R_wc = I; it is reproduced as written.
 * Poses are 7 doubles (qw,qx,qy,qz,tx,ty,tz), T_wc.  bias: gyro (3) then accel (3).  preint [11]: delta_rot qw,qx,qy,qz |
 * delta_vel | delta_pos | dt (the layout of orbx_ba_solve_inertial).  The tracker's own guard (fewer than 10 observations: no call)
 * stays the caller's. */
enum {
  ORBX_POSE_INERTIAL_OK = 0,        /* all max_iterations iterations ran                                   */
  ORBX_POSE_INERTIAL_TOO_FEW = 1,   /* the loop ended with fewer than 5 masked-in observations              */
  ORBX_POSE_INERTIAL_SINGULAR = 2   /* the loop ended on an exactly zero pivot of the LU                    */
};
/* orbx_default_pose_inertial_config: 4 iterations, chi2 12.0 / 15.6 (mono / stereo) falling to 5.991 / 7.815, imu_weight 1.0
 * (pose_inertial_optim.rs:34-45).  Accepted ranges: 0 <= max_iterations <= 64, thresholds > 0, imu_weight finite and >= 0;
 * other values -> ORBX_ERR_INVALID. */
typedef struct {
  int max_iterations;
  double chi2_mono_init, chi2_stereo_init, chi2_mono_final, chi2_stereo_final, imu_weight;
} orbx_pose_inertial_config;
/* One problem's record: why the loop ended (ORBX_POSE_INERTIAL_*), the popcount of the final mask (n when no reclassification
 * ran), n, and the iterations begun (a break counts its iteration). */
typedef struct {
  int status, num_inliers, num_observations, iterations;
} orbx_pose_inertial_result;
void orbx_default_pose_inertial_config(orbx_pose_inertial_config* cfg);

/* One problem in host memory, synchronous.  pose_wc [7], velocity [3], bias [6]: the initial state; prev_kf_pose_wc [7],
 * prev_kf_velocity [3], preint [11]; pts3d [n][3] f64 world points, pts2d [n][2] f32 pixels (the keypoints' positions), is_stereo
 * [n] u8 (nonzero: the feature has a camera-frame point).  Outputs pose_out [7], velocity_out [3], bias_out [6], inlier_out [n] u8
 * (the final mask; may be NULL), result [1]. */
int orbx_pose_inertial_optimize(orbx_handle* h, const orbx_camera* cam, const orbx_pose_inertial_config* cfg, const double* pose_wc,
                                const double* velocity, const double* bias, const double* prev_kf_pose_wc, const double* prev_kf_velocity,
                                const double* preint, int n, const double* pts3d, const float* pts2d, const uint8_t* is_stereo,
                                double* pose_out, double* velocity_out, double* bias_out, uint8_t* inlier_out,
                                orbx_pose_inertial_result* result);
/* n_problems independent problems in host memory, one upload and one download: problem p owns observations
 * [offsets[p], offsets[p+1]) of pts3d / pts2d / is_stereo / inlier_out (offsets [n_problems+1], ascending from 0, as
 * orbx_pnp_ransac_batch); poses_wc / prev_kf_poses_wc / poses_out [n_problems][7], velocities / prev_kf_velocities /
 * velocities_out [n_problems][3], biases / biases_out [n_problems][6], preints [n_problems][11], results [n_problems].  inlier_out
 * may be NULL.  Each problem's result equals orbx_pose_inertial_optimize on it, byte for byte.  Synchronous; caller-owned buffers. */
int orbx_pose_inertial_batch(orbx_handle* h, const orbx_camera* cam, const orbx_pose_inertial_config* cfg, int n_problems,
                             const int* offsets, const double* pts3d, const float* pts2d, const uint8_t* is_stereo,
                             const double* poses_wc, const double* velocities, const double* biases, const double* prev_kf_poses_wc,
                             const double* prev_kf_velocities, const double* preints, double* poses_out, double* velocities_out,
                             double* biases_out, uint8_t* inlier_out, orbx_pose_inertial_result* results);
/* The same with every array in device memory (the caller's; the library only reads the inputs and writes the outputs),
 * asynchronous on the handle's stream.  d_inlier_out is required: it holds the mask between iterations.  The layout is PnP's:
 * d_offsets / d_pts3d / d_pts2d of an orbx_pnp_ransac_batch_device call and its d_poses_wc_out (as d_poses_wc) can be passed
 * straight in, with no host round trip.  One workgroup per problem; no limit on n.  d_offsets must be ascending from 0 (they are
 * trusted: they index the observation arrays). */
int orbx_pose_inertial_batch_device(orbx_handle* h, const orbx_camera* cam, const orbx_pose_inertial_config* cfg, int n_problems,
                                    const int* d_offsets, const double* d_pts3d, const float* d_pts2d, const uint8_t* d_is_stereo,
                                    const double* d_poses_wc, const double* d_velocities, const double* d_biases,
                                    const double* d_prev_kf_poses_wc, const double* d_prev_kf_velocities, const double* d_preints,
                                    double* d_poses_out, double* d_velocities_out, double* d_biases_out, uint8_t* d_inlier_out,
                                    orbx_pose_inertial_result* d_results);

/* ---- frame tracking against map points (src/tracking/tracker.rs) ---------------------------------------------------
 * One call = the numeric part of track_local_map (tracker.rs:863-988, mode 1) or track_with_motion_model (:1086-1192, mode 0) for
 * n_frames frames at once, with no host synchronisation inside: project each frame's map points with that frame's search pose,
 * search the frame's FeatureGrid (orbx_guided_match's search, casts and tie rule included), gather the matches in map-point order
 * into PnP's layout, run orbx_pnp_ransac_batch_device on them with the per-frame prior, and write the tracker's per-feature result.
 * For every map point of a frame's list, in list order:
 *   p_cam = pose.inverse().transform_point(position) — the inverse with se3.rs:56-63's operation order, then nalgebra's
 *   quaternion-vector product plus the translation, one IEEE operation at a time; skipped if p_cam.z <= 0;
 *   u = fx * x / z + cx, v = fy * y / z + cy (camera: the one given to the call);
 *   mode 0: skipped if u < 0 || u >= 2cx || v < 0 || v >= 2cy; accepted: the smallest distance < 100;
 *   mode 1: no bounds test; accepted: best <= 100 and, with more than one candidate, !(best as f32 > 0.75 * second as f32).
 * Accepted points become correspondences in ascending list order: pts3d = the position, pts2d = the matched keypoint's (x, y),
 * mp_idx = the point's index in the frame's list, feat_idx = the keypoint's index in the frame.  Frame b owns
 * [offsets[b], offsets[b+1]) of them, packed from 0 — the layout of orbx_pnp_ransac_batch_device, whose outputs (pose, inlier mask,
 * errors, records) this call hands through.  Two map points may match one feature; both are kept.  Then
 *   matched[feat] = mp_idx of the inlier correspondence on that feature (the later correspondence where two share it), else -1.
 * Per-frame status, first condition that holds:
 *   TOO_FEW_CORRESPONDENCES  n_correspondences < min_correspondences: pose = the prior's bytes, matched all -1, n_inliers 0;
 *   TOO_FEW_INLIERS          n_inliers < min_inliers: pose = the prior's bytes;
 *   NO_MODEL                 PnP's ORBX_PNP_NO_MODEL (pose = the prior, mask and errors under it, as PnP reports them);
 *   OK.
 * The tracker's state machine, the choice of local keyframes and refine_with_imu's guard stay with the caller; the lists can be
 * made on the device from resident map points (orbx_map_track_frames_device, below). */
enum {
  ORBX_TRACK_OK = 0,
  ORBX_TRACK_NO_MODEL = 1,
  ORBX_TRACK_TOO_FEW_CORRESPONDENCES = 2,
  ORBX_TRACK_TOO_FEW_INLIERS = 3
};
/* orbx_default_track_config(mode): radius 15.0 (tracker.rs:881, :1091), the grid's image 752 x 480, and the reference's guards:
 * mode 1: min_correspondences 4, min_inliers 0 (:937); mode 0: 10 and 10 (:1173, :1186).  Accepted: mode 0 or 1, radius >= 0 and
 * finite, img_w / img_h > 0 and finite, min_correspondences >= 4 (PnP's own minimum), min_inliers >= 0; else ORBX_ERR_INVALID.
 * Both configurations (this one and orbx_pnp_config) are checked before anything is enqueued. */
typedef struct {
  int mode;
  double radius, img_w, img_h;
  int min_correspondences, min_inliers;
} orbx_track_config;
/* n_in_front: map points with p_cam.z > 0; n_correspondences: accepted matches; n_inliers: PnP's final mask. */
typedef struct {
  int status, n_in_front, n_correspondences, n_inliers;
} orbx_track_result;
void orbx_default_track_config(int mode, orbx_track_config* cfg);

/* Every array in device memory (the caller's), asynchronous on the handle's stream; mp_offsets alone is a host array.
 *   features: frame b's keypoints / descriptors are d_kp / d_desc [d_feat_start[b] .. + n_b), n_b = d_feat_count[b *
 *     feat_count_stride] — start and count are read on the device, by kernels on the handle's stream, so the extractor's slots
 *     and its device-side counts serve as they are, ordered behind the extraction with no copy and no host round trip (the left
 *     images of orbx_process_stereo_batch_device: d_feat_start[b] = 2 b cap_kp, d_feat_count = d_nkp, feat_count_stride = 2; the
 *     right images: d_nkp + 1).  feat_count_stride >= 1, in ints.  max_feat: a host-known bound on a frame's count; a frame whose
 *     count is negative or above it is searched as if it had no features (TOO_FEW_CORRESPONDENCES, zero correspondences) instead
 *     of being read past the bound;
 *   map points: d_positions [M][3] f64, d_mp_desc [M][32]; frame b's list is [mp_offsets[b], mp_offsets[b+1]), ascending from 0,
 *     M = mp_offsets[n_frames]; the array is copied before the call returns (the caller may change or free it at once);
 *   d_search_poses_wc / d_priors_wc [n_frames][7] T_wc: the pose the points are projected with and PnP's prior (mode 1: self.pose
 *     and imu_prior; mode 0: the predicted pose twice — the same pointer may be given);
 *   outputs: d_offsets [n_frames+1]; d_pts3d [M][3], d_pts2d [M][2], d_mp_idx / d_feat_idx [M], d_inlier_out [M], d_err_out [M]
 *     (entries [0, d_offsets[n_frames]) are written); d_poses_wc_out [n_frames][7]; d_pnp_results [n_frames];
 *     d_matched [n_frames][max_feat] (all of it is written); d_results [n_frames].
 * d_offsets / d_pts3d / d_pts2d / d_poses_wc_out can be passed straight into orbx_pose_inertial_batch_device. */
int orbx_track_frames_device(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                             int n_frames, const orbx_keypoint* d_kp, const uint8_t* d_desc, const int* d_feat_start,
                             const int* d_feat_count, int feat_count_stride, int max_feat, const double* d_positions,
                             const uint8_t* d_mp_desc,
                             const int* mp_offsets, const double* d_search_poses_wc, const double* d_priors_wc, int* d_offsets,
                             double* d_pts3d, float* d_pts2d, int* d_mp_idx, int* d_feat_idx, double* d_poses_wc_out,
                             uint8_t* d_inlier_out, double* d_err_out, orbx_pnp_result* d_pnp_results, int* d_matched,
                             orbx_track_result* d_results);
/* The same in host memory, synchronous, one upload and one download.  Frame b's features are kp / desc
 * [feat_offsets[b], feat_offsets[b+1]) (ascending from 0); matched is packed the same way ([feat_offsets[n_frames]]); the
 * other arrays as above.  Each frame's result equals the device form's, byte for byte. */
int orbx_track_frames(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                      int n_frames, const orbx_keypoint* kp, const uint8_t* desc, const int* feat_offsets, const double* positions,
                      const uint8_t* mp_desc, const int* mp_offsets, const double* search_poses_wc, const double* priors_wc,
                      int* offsets, double* pts3d, float* pts2d, int* mp_idx, int* feat_idx, double* poses_wc_out,
                      uint8_t* inlier_out, double* err_out, orbx_pnp_result* pnp_results, int* matched, orbx_track_result* results);

/* ---- frame tracking against the reference keyframe (src/tracking/tracker.rs:992-1064) --------------------------------
 * One call = the numeric part of track_with_reference_kf for n_frames frames at once, each against its own reference keyframe,
 * with no host synchronisation inside:
 *   1. BFMatcher(NORM_HAMMING, crossCheck = true).train_match(kf.descriptors, frame.descriptors) — query = keyframe feature,
 *      train = frame feature: the mutual nearest neighbours in ascending query index, the lowest index winning a distance tie in
 *      both directions (exactly orbx_hamming_match_crosscheck of the pair).  [spec] an empty side gives no matches (OpenCV
 *      raises an error there);
 *   2. for each match in that order: skipped unless valid[query_idx] != 0, else pts3d = positions[query_idx], pts2d = the
 *      frame keypoint's (x, y) at train_idx.  The map lookups stay with the caller: valid[i] = 1 only when
 *      kf.get_map_point(i) is Some and the map still holds that point (:1024-1036), positions[i] = that point's position;
 *   3. fewer than min_correspondences (>= 4, :1051): TOO_FEW_CORRESPONDENCES, pose = the prior's bytes, n_inliers 0;
 *   4. orbx_pnp_ransac_batch_device with the per-frame prior (:1057): NO_MODEL (pose = the prior) or OK.
 * ORBX_TRACK_TOO_FEW_INLIERS is never produced: the reference has no such guard here.  The reference's Option<SE3> is Some(pose)
 * for OK and NO_MODEL.  Every frame's result is the same bytes alone, inside any batch, and in the host form.
 * n_matches: mutual matches (with or without a map point); n_correspondences: those with valid != 0; n_inliers: PnP's mask. */
typedef struct {
  int status, n_matches, n_correspondences, n_inliers;
} orbx_track_ref_result;

/* Every array in device memory (the caller's), asynchronous on the handle's stream; kf_offsets alone is a host array.
 *   frames: d_kp / d_desc / d_feat_start / d_feat_count / feat_count_stride / max_feat as orbx_track_frames_device (counts are
 *     read on the device; a count that is negative or above max_feat is a frame without features).  max_feat <= 4194304;
 *   keyframes, packed: frame b's reference keyframe owns rows [kf_offsets[b], kf_offsets[b+1]) of d_kf_desc [K][32],
 *     d_kf_positions [K][3] f64 and d_kf_valid [K] u8 (kf_offsets [n_frames+1] ascending from 0, K = kf_offsets[n_frames]; the
 *     array is copied before the call returns).  Frames that share a keyframe repeat its rows;
 *   d_priors_wc [n_frames][7] T_wc (self.pose, :1057);
 *   outputs: d_matches [K]: frame b's mutual matches from kf_offsets[b], results[b].n_matches of them (distance = the integer
 *     distance as f32, img_idx 0); d_offsets [n_frames+1]; d_pts3d [K][3], d_pts2d [K][2], d_kf_idx / d_feat_idx [K] (the
 *     match's query_idx / train_idx), d_inlier_out [K], d_err_out [K]: frame b's correspondences are
 *     [d_offsets[b], d_offsets[b+1]), packed from 0 in ascending keyframe-feature index (entries [0, d_offsets[n_frames]) are
 *     written); d_poses_wc_out [n_frames][7]; d_pnp_results / d_results [n_frames].
 * min_correspondences < 4, n_frames < 0 or an orbx_pnp_config out of range -> ORBX_ERR_INVALID before anything is enqueued;
 * n_frames = 0 does nothing.  d_offsets / d_pts3d / d_pts2d / d_poses_wc_out can be passed straight into
 * orbx_pose_inertial_batch_device. */
int orbx_track_reference_device(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                                int n_frames, const orbx_keypoint* d_kp, const uint8_t* d_desc, const int* d_feat_start,
                                const int* d_feat_count, int feat_count_stride, int max_feat, const uint8_t* d_kf_desc,
                                const double* d_kf_positions, const uint8_t* d_kf_valid, const int* kf_offsets,
                                const double* d_priors_wc, orbx_dmatch* d_matches, int* d_offsets, double* d_pts3d, float* d_pts2d,
                                int* d_kf_idx, int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                                orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results);
/* The same in host memory, synchronous, one upload and one download.  Frame b's features are kp / desc
 * [feat_offsets[b], feat_offsets[b+1]) (ascending from 0); the other arrays as above. */
int orbx_track_reference(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences, int n_frames,
                         const orbx_keypoint* kp, const uint8_t* desc, const int* feat_offsets, const uint8_t* kf_desc,
                         const double* kf_positions, const uint8_t* kf_valid, const int* kf_offsets, const double* priors_wc,
                         orbx_dmatch* matches, int* offsets, double* pts3d, float* pts2d, int* kf_idx, int* feat_idx,
                         double* poses_wc_out, uint8_t* inlier_out, double* err_out, orbx_pnp_result* pnp_results,
                         orbx_track_ref_result* results);
/* The device form with the reference keyframes resident (orbx_keyframe): frame b is matched against kfs[b]'s descriptors where
 * they lie; a handle may be repeated.  kf_positions / kf_valid are HOST arrays packed in kfs[] order by kf_offsets (host), and
 * kf_offsets[b+1] - kf_offsets[b] must equal kfs[b]'s feature count (else ORBX_ERR_INVALID); the three and kfs are copied before
 * the call returns and travel in one upload on the handle's stream.  Frames, the prior and every output are device arrays as in
 * orbx_track_reference_device; the result equals that call's on the same rows, byte for byte. */
int orbx_keyframe_track_reference(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                                  int n_frames, const orbx_keyframe* const* kfs, const orbx_keypoint* d_kp, const uint8_t* d_desc,
                                  const int* d_feat_start, const int* d_feat_count, int feat_count_stride, int max_feat,
                                  const double* kf_positions, const uint8_t* kf_valid, const int* kf_offsets, const double* d_priors_wc,
                                  orbx_dmatch* d_matches, int* d_offsets, double* d_pts3d, float* d_pts2d, int* d_kf_idx,
                                  int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                                  orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results);

/* ---- loop-candidate verification (src/loop_closing/corrector.rs:116-204, src/loop_closing/sim3_solver.rs) -----------------
 * verify_loop_candidate for a batch of (current keyframe, loop keyframe) pairs in one call with no host synchronisation inside;
 * tests/loop_verify_spec.py restates it in numpy, DESIGN.md §2 lists the [spec] choices.  Per pair:
 *   0. has_point counts of both keyframes, either below min_stereo_points (:132): TOO_FEW_POINTS;
 *   1. match_features_bow (:229-306): for every current feature the best and the second-best Hamming distance over the loop
 *      keyframe's features (strict <, so the lowest index keeps the best and a repeated best distance becomes the second), kept iff
 *      best < match_max_dist && (double)best < match_ratio * (double)second (second = 4294967295 with a single candidate).  With
 *      node ids on both keyframes the candidates of a feature are the loop features of its node in ascending index (node
 *      0xffffffff, or a node the loop keyframe lacks: no match); else brute force.  [spec] matches come out in ascending
 *      current-feature index (the reference walks a HashMap).  Fewer than min_matches (:139): TOO_FEW_MATCHES;
 *   2. gather (:149-180): the matches whose two features both have a stereo point, world = pose_wc * points_cam (nalgebra's
 *      quaternion-vector product, then + t).  Fewer than min_pairs (:178): TOO_FEW_PAIRS;
 *   3. compute_sim3_ransac (sim3_solver.rs:63-145): see orbx_sim3_ransac_batch.  None: NO_MODEL; fewer than min_inliers
 *      (corrector.rs:185): TOO_FEW_INLIERS;
 *   4. verify_by_reprojection (:330-378) over ALL gathered matches: p = pose_loop^-1 * (M x + t); z <= 0 skipped; counted iff
 *      du^2 + dv^2 < chi2 * s * s, s = scale_factor^octave of the loop keypoint (octave clamped to 0..31).  Fewer than
 *      min_verified (:193): TOO_FEW_VERIFIED.
 * Status = the first failing guard, else OK (the reference's Some).  The outputs of the stages up to and including the failing
 * one are written; later record fields are 0, the Sim3 is the identity (1,0,0,0, 0,0,0, 1) and the mask is 0.
 * A pair's result is the same bytes alone, inside any batch, and in every form below. */
enum {
  ORBX_LOOP_OK = 0, ORBX_LOOP_TOO_FEW_POINTS = 1, ORBX_LOOP_TOO_FEW_MATCHES = 2, ORBX_LOOP_TOO_FEW_PAIRS = 3, ORBX_LOOP_NO_MODEL = 4,
  ORBX_LOOP_TOO_FEW_INLIERS = 5, ORBX_LOOP_TOO_FEW_VERIFIED = 6
};
enum { ORBX_SIM3_OK = 0, ORBX_SIM3_NO_MODEL = 1 };
/* = Sim3SolverConfig, sim3_solver.rs:13-36; orbx_default_sim3_config: 300, 0.075, 15, fix_scale 1, 0.99, seed 0.  probability is
 * carried and has no effect: the reference's loop range is built before its adaptive bound is lowered (:84, :113), so all
 * max_iterations hypotheses are always evaluated.  Accepted: 1 <= max_iterations <= 1024, inlier_threshold > 0, min_inliers >= 3,
 * 0 <= probability <= 1; other values -> ORBX_ERR_INVALID. */
typedef struct {
  int max_iterations;
  double inlier_threshold;
  int min_inliers, fix_scale;
  double probability;
  uint64_t seed;
} orbx_sim3_config;
/* The guards of corrector.rs:132 / :139 / :178 / :185 / :193 (20, 15, 15, 15, 50), the matcher's constants (:266: 50, 0.7), the
 * reprojection test's (:338, :368: 5.991, 1.2) and the solver's configuration (fix_scale = 1, :183).  Accepted: counts >= 0,
 * match_max_dist <= 256, match_ratio > 0, chi2 > 0, scale_factor > 0 and a valid sim3; else ORBX_ERR_INVALID. */
typedef struct {
  int min_stereo_points, min_matches, min_pairs, min_inliers, min_verified;
  unsigned match_max_dist;
  double match_ratio, chi2, scale_factor;
  orbx_sim3_config sim3;
} orbx_loop_verify_config;
/* best_hypothesis: the winner's index (-1: none had an inlier); ransac_inliers: its count; n_inliers: of the returned model;
 * refined: 1 when the refit over the winner's inliers was kept (:133); mse: mean squared error over the returned inliers. */
typedef struct {
  int status, best_hypothesis, ransac_inliers, n_inliers, refined, reserved_;
  double mse;
} orbx_sim3_result;
typedef struct {
  int status, n_matches, n_pairs, best_hypothesis, ransac_inliers, n_inliers, refined, n_verified;
  double mse;
} orbx_loop_verify_result;
void orbx_default_sim3_config(orbx_sim3_config* cfg);
void orbx_default_loop_verify_config(orbx_loop_verify_config* cfg);

/* compute_sim3_ransac for n_problems point sets: problem p owns rows [offsets[p], offsets[p+1]) of pts1 / pts2 [N][3] f64 and of
 * inlier [N] u8; it finds S with pts2 ~ S pts1.  sim3 [n_problems][8] = (qw,qx,qy,qz, tx,ty,tz, scale), qw >= 0 [spec].
 *   [spec] hypothesis h = the first three distinct indices of PnP's counter-based sampler (64 draws; none: no hypothesis);
 *   Horn on the sample: centroids, H = sum (p1-c1)(p2-c2)^T in sample order, R = V diag(1,1,det(V U^T)) U^T by a one-sided Jacobi
 *   SVD in f64 that completes the basis of a rank-deficient H (a 3-point H has rank <= 2; collinear points rank 1): always a
 *   proper rotation; scale 1 or sqrt(sum|b|^2 / sum|a|^2) (no hypothesis below 1e-10); M = scale * R; t = c2 - M c1;
 *   inlier: |M p1 + t - p2|^2 < inlier_threshold^2.  Winner: most inliers, lowest h on ties (:100).  With >= min_inliers: Horn
 *   over the winner's inliers, recount, kept iff the count did not fall (:133).  Fewer than min_inliers then, n < 3 or
 *   n < min_inliers (:69-75): NO_MODEL, identity, mask 0.
 * Host form: synchronous, one upload and one download.  Device form: every array in device memory, asynchronous on the
 * handle's stream; max_n bounds a problem's size (a larger one gets NO_MODEL); d_offsets ascending from 0, trusted. */
int orbx_sim3_ransac_batch(orbx_handle* h, const orbx_sim3_config* cfg, int n_problems, const int* offsets, const double* pts1,
                           const double* pts2, double* sim3, uint8_t* inlier, orbx_sim3_result* results);
int orbx_sim3_ransac_batch_device(orbx_handle* h, const orbx_sim3_config* cfg, int n_problems, int max_n, const int* d_offsets,
                                  const double* d_pts1, const double* d_pts2, double* d_sim3, uint8_t* d_inlier,
                                  orbx_sim3_result* d_results);
/* The whole verification.  Keyframes are packed: pair b's current keyframe owns rows [cur_offsets[b], cur_offsets[b+1]) of
 * cur_desc [N1][32], cur_points_cam [N1][3] f64, cur_has_point [N1] u8 and cur_node [N1] u32; its loop keyframe rows
 * [loop_offsets[b], loop_offsets[b+1]) of loop_kp, loop_desc, loop_points_cam, loop_has_point, loop_node (keyframes shared by
 * pairs repeat their rows).  cur_node / loop_node are HOST arrays in every form and may be NULL (brute force everywhere); a pair
 * uses the FeatureVector matcher iff both are given (an all-0xffffffff array is a keyframe whose FeatureVector is empty).  The
 * current keyframe's keypoints are not read.  cur_poses_wc / loop_poses_wc [n_pairs][7] and both offset arrays are host arrays.
 * Outputs, all packed from cur_offsets[b]: matches [N1] (results[b].n_matches of them: query_idx = current feature, train_idx =
 * loop feature, distance = the integer distance as f32), feature_matches [N1][2], pts_current / pts_loop [N1][3] and inlier [N1]
 * (results[b].n_pairs of them); sim3 [n_pairs][8]; results [n_pairs].  At most 4194304 features per keyframe.
 * The device form is asynchronous on the handle's stream; the host arrays are copied before it returns. */
int orbx_verify_loop_candidates(orbx_handle* h, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int n_pairs,
                                const uint8_t* cur_desc, const double* cur_points_cam, const uint8_t* cur_has_point,
                                const uint32_t* cur_node, const int* cur_offsets, const double* cur_poses_wc, const orbx_keypoint* loop_kp,
                                const uint8_t* loop_desc, const double* loop_points_cam, const uint8_t* loop_has_point,
                                const uint32_t* loop_node, const int* loop_offsets, const double* loop_poses_wc, orbx_dmatch* matches,
                                int* feature_matches, double* pts_current, double* pts_loop, uint8_t* inlier, double* sim3,
                                orbx_loop_verify_result* results);
int orbx_verify_loop_candidates_device(orbx_handle* h, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int n_pairs,
                                       const uint8_t* d_cur_desc, const double* d_cur_points_cam, const uint8_t* d_cur_has_point,
                                       const uint32_t* cur_node, const int* cur_offsets, const double* cur_poses_wc,
                                       const orbx_keypoint* d_loop_kp, const uint8_t* d_loop_desc, const double* d_loop_points_cam,
                                       const uint8_t* d_loop_has_point, const uint32_t* loop_node, const int* loop_offsets,
                                       const double* loop_poses_wc, orbx_dmatch* d_matches, int* d_feature_matches,
                                       double* d_pts_current, double* d_pts_loop, uint8_t* d_inlier, double* d_sim3,
                                       orbx_loop_verify_result* d_results);
/* The same on resident keyframes (handles may repeat): features, stereo points, poses and FeatureVectors
 * (orbx_keyframe_set_feature_nodes) are the keyframes' own.  Outputs are HOST arrays packed from the running sum of the current
 * keyframes' feature counts; only they cross PCIe.  Synchronous.  Bytes equal the packed forms' on the same rows. */
int orbx_keyframe_verify_loop_candidates(orbx_handle* h, const orbx_camera* cam, const orbx_loop_verify_config* cfg, int n_pairs,
                                         const orbx_keyframe* const* cur_kfs, const orbx_keyframe* const* loop_kfs, orbx_dmatch* matches,
                                         int* feature_matches, double* pts_current, double* pts_loop, uint8_t* inlier, double* sim3,
                                         orbx_loop_verify_result* results);

/* ---- map-point refresh: distinctive descriptor, normal and depth range (search_in_neighbors.rs:139-150) ------------
 * Phase 4 of search_in_neighbors for M map points in one call: Map::compute_distinctive_descriptors (src/atlas/map/map.rs:880-944)
 * and Map::update_map_point_normal_and_depth (map.rs:716-742, src/atlas/map/map_point.rs:173-203).  The map mutation of phases 2-3
 * stays with the caller; this call takes the observation lists as they are afterwards.  Point p owns observations
 * [obs_start[p], obs_start[p+1]) of obs_kf (index into the T keyframes of the call) and obs_feat (feature index in that keyframe).
 *   [spec] the reference iterates HashMaps here; the order is the order of the point's observation list as given.
 * Descriptor: the rows of the observations whose keyframe exists (0 <= obs_kf < T; else keyframes.get -> None) and whose feature
 * index is inside it (0 <= obs_feat < its feature count; else row() -> Err) are collected in order.  None: the point keeps its
 * descriptor, chosen = -1, best_max_dist = 0.  One: that row, best_max_dist = 0.  More: for every collected row the largest Hamming
 * distance to the other collected rows (other by position: equal rows are 0 apart); the row with the smallest such maximum, the
 * earliest on ties.  chosen is its position in the point's OBSERVATION list; n_desc the number collected.
 * Normal and depth: over every observation whose keyframe exists (the feature index does not matter), in order:
 * d = position - t_wc(keyframe), dist = sqrt((dx*dx + dy*dy) + dz*dz); if dist > 1e-10: sum += d / dist component by component,
 * min / max of dist (from +inf / 0).  norm = sqrt((sx*sx + sy*sy) + sz*sz); if norm > 1e-10 the normal becomes sum / norm, else it
 * keeps its value.  min_distance = min / scale_range, max_distance = max * scale_range, so a point without observers gets +inf and
 * 0.  scale_range = scale_factor^(num_levels - 1), computed by the caller (powi, map_point.rs:200).  n_observers = keyframes found.
 * Out-of-range obs_kf / obs_feat are not errors.  One IEEE operation at a time, no fused multiply-add. */
typedef struct {
  int32_t chosen;
  uint32_t best_max_dist, n_desc, n_observers;
} orbx_mp_refresh_record; /* 16 B */
/* Host form: synchronous, one upload and one download.  positions [M][3], obs_start [M+1] ascending from 0 (else ORBX_ERR_INVALID),
 * kf_poses_wc [T][7], kf_feat_offset [T+1] ascending from 0: keyframe t owns rows [kf_feat_offset[t], kf_feat_offset[t+1]) of descs
 * [..][32].  mp_desc [M][32] and normals [M][3] are in/out; min_distance / max_distance [M], records [M].  M == 0: ORBX_OK. */
int orbx_refresh_map_points(orbx_handle* h, int M, const double* positions, const int* obs_start, const int* obs_kf, const int* obs_feat,
                            int T, const double* kf_poses_wc, const int* kf_feat_offset, const uint8_t* descs, double scale_range,
                            uint8_t* mp_desc, double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records);
/* Device form: the same arrays in device memory (descriptor arrays 8-byte aligned), asynchronous on the handle's stream.  The
 * keyframe table — kf_poses_wc and kf_feat_offset — is HOST memory, copied before the call returns.  n_obs = obs_start[M], which
 * the host cannot read here; d_obs_start is trusted to ascend from 0 to it. */
int orbx_refresh_map_points_device(orbx_handle* h, int M, int n_obs, const double* d_positions, const int* d_obs_start, const int* d_obs_kf,
                                   const int* d_obs_feat, int T, const double* kf_poses_wc, const int* kf_feat_offset, const uint8_t* d_descs,
                                   double scale_range, uint8_t* d_mp_desc, double* d_normals, double* d_min_distance, double* d_max_distance,
                                   orbx_mp_refresh_record* d_records);
/* The same on resident keyframes: descriptors and poses (camera centre = translation of T_wc) are the keyframes' own, read where
 * they lie; the other arrays are HOST memory as in the host form.  Only the points, their lists and the results cross PCIe.
 * Synchronous.  A keyframe of another handle: ORBX_ERR_INVALID.  Bytes equal the packed forms' on the same rows. */
int orbx_keyframe_refresh_map_points(orbx_handle* h, int M, const double* positions, const int* obs_start, const int* obs_kf,
                                     const int* obs_feat, const orbx_keyframe* const* kfs, int T, double scale_range, uint8_t* mp_desc,
                                     double* normals, double* min_distance, double* max_distance, orbx_mp_refresh_record* records);

/* ---- resident map points: store, local-map selection, tracking (tracker.rs:826-867, :1024-1036, :1093-1102) ----------------
 * orbx_map_points keeps map points in device memory, so that a frame's list of map points is made where the tracker reads it.
 * A store has a fixed capacity; a point lives in a SLOT, an int in [0, capacity).  The caller owns the id -> slot assignment (ids
 * are map bookkeeping and stay on the host, as they do for orbx_keyframe).  Per slot: position f64[3], descriptor u8[32] and a
 * live byte — live means map.get_map_point(id) is Some; is_bad is not consulted (neither tracker.rs:864-867 nor :1099-1102 reads
 * it).  A store belongs to its handle; all its work is ordered on the handle's stream.
 *   set: rows i of positions [n][3] / desc [n][32] go to slots[i]; one upload, one launch.  Either array may be NULL: that field
 *     stays as it is (positions only: BA's apply; descriptors only: the refresh).  A slot that is not live becomes live and needs
 *     both.  ORBX_ERR_INVALID before anything is enqueued, the store unchanged: a slot outside [0, capacity), a slot listed twice
 *     in the call, a first set with a field missing.
 *   set_device: the same with the rows in device memory (the outputs of orbx_refresh_map_points_device, BA's point array, the
 *     points of orbx_keyframe_triangulate_from_neighbors), asynchronous.  slots stays a HOST array (copied before the call returns):
 *     the assignment is the caller's, and so every check of set is made here too.  d_desc 4-byte, d_positions 8-byte aligned.
 *   erase: clears live (a slot may repeat; one that is not live stays so).  download: rows of the listed slots (any of the three
 *     outputs may be NULL), synchronous; for tests and debugging.  info: capacity and the number of live slots.
 *   orbx_keyframe_set_map_point_slots: the keyframe's per-feature slot table [n], -1 = None, kept in the keyframe's device block;
 *     NULL clears it (a keyframe without a table counts as all -1).  Values < -1 or >= capacity: ORBX_ERR_INVALID.  The table is
 *     bound to the store it was set against (which must outlive it); orbx_keyframe_set_map_points and the ids are untouched.
 *
 * orbx_map_select_points_device makes, for each of n_frames frames, its list of map points, with no host synchronisation inside.
 *   ORBX_MAP_SOURCE_KEYFRAMES (track_local_map, :826-867): frame b names kfs[kf_offsets[b] .. kf_offsets[b+1]) (host arrays,
 *     copied before the call returns).  Its list is the DISTINCT LIVE slots in FIRST-SEEN order, walking the keyframes in the order
 *     given and each keyframe's features in index order (get_map_point_indices, keyframe.rs:249-254); -1 and slots not live when
 *     the kernels run are skipped.  [spec] the reference collects into a HashSet, whose order is unspecified and changes between
 *     runs; the order matters because it is the order of PnP's correspondences.
 *   ORBX_MAP_SOURCE_SLOTS (track_with_motion_model, :1093-1102): frame b's source is d_src_slots[src_offsets[b] ..
 *     src_offsets[b+1]) (a device array, host offsets), walked in order; -1 and slots not live are skipped; NO de-duplication (the
 *     reference pushes a point once per feature that carries it).
 *   The arguments of the other kind are ignored (NULL).  Outputs, device memory: d_list_offsets [n_frames+1] packed from 0,
 *   d_list_slot, d_positions [.][3], d_mp_desc [.][32] (16-byte aligned) — the last two in the layout orbx_track_frames_device reads.
 *   list_cap is the number of rows the three hold; it must reach the host-known bound: the sum over the frames of their candidates
 *   (features of the frame's keyframes, or entries of its source), per frame at most the capacity where keyframes are the source.
 *   A list is never truncated.  The result is the same bytes on every run and in any batch composition.
 *
 * orbx_map_track_frames_device = that selection, then orbx_track_frames_device's launches on the lists as they lie.  Frames, poses,
 * cfg and the outputs d_offsets .. d_results are those of orbx_track_frames_device, sized by list_cap where that call says M (mp_idx
 * indexes the frame's list).  Added: the lists themselves and d_matched_slot [n_frames][max_feat]: matched mapped through the list
 * to slots, -1 where none.  d_matched_slot of frame t is a valid SLOTS source for frame t+1 (src_offsets[b] = b * max_feat).  Every
 * output equals orbx_track_frames_device's on the same lists, byte for byte.  orbx_map_track_frames: the same with the features,
 * the slot source and every output in host memory (matched / matched_slot packed by feat_offsets), synchronous.
 *
 * orbx_map_track_reference_device = orbx_keyframe_track_reference with kf_positions / kf_valid made on the device from kfs[b]'s slot
 * table and the store: valid[i] = slot[i] >= 0 && live[slot[i]], positions[i] = that slot's position, else zeros.  They are
 * written to d_kf_positions [K][3] / d_kf_valid [K], K = the keyframes' feature counts summed in kfs order (frame b's rows start
 * where the earlier keyframes' end); the other outputs are sized by K as in orbx_track_reference_device.
 *
 * In the four calls above the frame is a grid dimension of the launches: n_frames > 65535 is ORBX_ERR_INVALID before anything is
 * enqueued, with the store, the tables and the outputs untouched. */
typedef struct orbx_map_points orbx_map_points;
enum { ORBX_MAP_SOURCE_KEYFRAMES = 0, ORBX_MAP_SOURCE_SLOTS = 1 };
int orbx_map_points_create(orbx_handle* h, int capacity, orbx_map_points** out);
void orbx_map_points_destroy(orbx_map_points* mp);
int orbx_map_points_info(const orbx_map_points* mp, int* capacity, int* n_live);
int orbx_map_points_set(orbx_map_points* mp, const int* slots, int n, const double* positions, const uint8_t* desc);
int orbx_map_points_set_device(orbx_map_points* mp, const int* slots, int n, const double* d_positions, const uint8_t* d_desc);
int orbx_map_points_erase(orbx_map_points* mp, const int* slots, int n);
int orbx_map_points_download(orbx_map_points* mp, const int* slots, int n, double* positions, uint8_t* desc, uint8_t* live);
int orbx_keyframe_set_map_point_slots(orbx_keyframe* kf, const orbx_map_points* mp, const int* slots);
int orbx_map_select_points_device(orbx_handle* h, orbx_map_points* mp, int source, int n_frames, const orbx_keyframe* const* kfs,
                                  const int* kf_offsets, const int* d_src_slots, const int* src_offsets, int list_cap,
                                  int* d_list_offsets, int* d_list_slot, double* d_positions, uint8_t* d_mp_desc);
int orbx_map_track_frames_device(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                                 orbx_map_points* mp, int source, int n_frames, const orbx_keyframe* const* kfs, const int* kf_offsets,
                                 const int* d_src_slots, const int* src_offsets, const orbx_keypoint* d_kp, const uint8_t* d_desc,
                                 const int* d_feat_start, const int* d_feat_count, int feat_count_stride, int max_feat,
                                 const double* d_search_poses_wc, const double* d_priors_wc, int list_cap, int* d_list_offsets,
                                 int* d_list_slot, double* d_positions, uint8_t* d_mp_desc, int* d_offsets, double* d_pts3d,
                                 float* d_pts2d, int* d_mp_idx, int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out,
                                 double* d_err_out, orbx_pnp_result* d_pnp_results, int* d_matched, int* d_matched_slot,
                                 orbx_track_result* d_results);
int orbx_map_track_frames(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                          orbx_map_points* mp, int source, int n_frames, const orbx_keyframe* const* kfs, const int* kf_offsets,
                          const int* src_slots, const int* src_offsets, const orbx_keypoint* kp, const uint8_t* desc,
                          const int* feat_offsets, const double* search_poses_wc, const double* priors_wc, int list_cap,
                          int* list_offsets, int* list_slot, int* offsets, double* pts3d, float* pts2d, int* mp_idx, int* feat_idx,
                          double* poses_wc_out, uint8_t* inlier_out, double* err_out, orbx_pnp_result* pnp_results, int* matched,
                          int* matched_slot, orbx_track_result* results);
int orbx_map_track_reference_device(orbx_handle* h, const orbx_camera* cam, const orbx_pnp_config* pnp_cfg, int min_correspondences,
                                    orbx_map_points* mp, int n_frames, const orbx_keyframe* const* kfs, const orbx_keypoint* d_kp,
                                    const uint8_t* d_desc, const int* d_feat_start, const int* d_feat_count, int feat_count_stride,
                                    int max_feat, const double* d_priors_wc, double* d_kf_positions, uint8_t* d_kf_valid,
                                    orbx_dmatch* d_matches, int* d_offsets, double* d_pts3d, float* d_pts2d, int* d_kf_idx,
                                    int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                                    orbx_pnp_result* d_pnp_results, orbx_track_ref_result* d_results);

/* ---- covisibility from the resident map: weights, best neighbours, local-map tracking (map.rs:339-386, :476-489; tracker.rs:826-843) ----
 * The covisibility graph, computed where the slot tables lie instead of maintained on the host per association.  kfs [n_kfs] are
 * the keyframes the caller considers (host array, copied before the call returns; is_bad filtering = leaving a keyframe out);
 * every index below is a position in kfs[].  The reference's weight depends on the association history and its order on HashMap
 * iteration, so the library fixes a derived, deterministic definition:
 *   [spec] obs(k) = the DISTINCT slots s of kfs[k]'s slot table with 0 <= s < capacity and live[s] when the kernels run.  A
 *     keyframe without a table observes nothing; a slot listed at two features of one keyframe counts once.
 *   [spec] weight[q][k] = the number of slots in both obs(query[q]) and obs(k), for k != query[q], and weight[q][query[q]] = 0 (no self connection,
 *     keyframe.rs:270-273).  Symmetric by construction; where every shared point is associated once per keyframe it equals
 *     covisibility_weights() (map.rs:361-383).
 *   [spec] best(q, n) = the keyframes with weight > 0 by weight descending, then by position in kfs[] ascending, at most n
 *     (get_best_covisibles / get_local_keyframes_readonly, keyframe.rs:313-345, map.rs:476-489).  The tie order is fixed: a caller
 *     that lists kfs[] by id ascending gets the order include/orbx_map.hpp recommends.
 *   [spec] local keyframes of a frame with reference index r (tracker.rs:826-843): r >= 0: [r] ++ best(r, n_best) in that order
 *     (the reference unions into a HashSet; the order is fixed because the first-seen order of the map-point list, and so PnP's
 *     correspondence order, follows from it); r == -1 (no reference keyframe, :830-834): all of kfs[] in the order given.
 *
 * orbx_map_covisibility_device: query [n_queries] is a host array (copied before the call returns).  Outputs, device memory, each
 * may be NULL: d_weights [n_queries][n_kfs] int32, d_best [n_queries][n_best] int32 (-1 padded), d_n_best [n_queries] int32 (the
 * entries of the row that are not padding).  Asynchronous on the handle's stream, no host synchronisation inside; the store's mark
 * tables are left as they were found, so a call costs what its keyframes cost, not what the map holds.  Every row is the same
 * bytes in any batch composition.  orbx_map_covisibility: the same with host outputs, synchronous.
 * ORBX_ERR_INVALID before anything is enqueued: an index outside [0, n_kfs), n_best < 0, n_queries > 65535, a keyframe of another
 * handle or whose table is bound to another store.  n_kfs = 0 or n_queries = 0: nothing is done, ORBX_OK.
 *
 * orbx_map_track_local_device = orbx_map_track_frames_device (ORBX_MAP_SOURCE_KEYFRAMES) with frame b's keyframe list chosen on the
 * device: the local keyframes of ref_kf[b] (host [n_frames], -1 = all of kfs[]) with n_best neighbours.  Added output d_local_kf
 * [n_frames][1 + n_best] int32 (may be NULL): the list chosen, -1 padded; for ref_kf[b] = -1 the row is all -1 (the list is kfs[]
 * itself).  Every other argument and output is orbx_map_track_frames_device's and equals, byte for byte, that call's on the
 * keyframe lists the specification gives.  list_cap must reach the host-known bound: per frame the reference keyframe's feature
 * count plus the n_best largest of the other keyframes', at most the capacity; for -1 the sum over all keyframes, at most the
 * capacity.  ORBX_ERR_INVALID as above (ref_kf outside [-1, n_kfs); n_frames > 65535: the frame is a grid dimension).
 * orbx_map_track_local: the host form, as orbx_map_track_frames is to its device form (local_kf [n_frames][1 + n_best], may be NULL).
 * Still the caller's: ids, the id -> slot map, is_bad (by leaving keyframes out of kfs[]) and the spanning tree. */
int orbx_map_covisibility_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_queries,
                                 const int* query, int n_best, int* d_weights, int* d_best, int* d_n_best);
int orbx_map_covisibility(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_queries,
                          const int* query, int n_best, int* weights, int* best, int* n_best_out);
int orbx_map_track_local_device(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                                orbx_map_points* mp, int n_frames, int n_kfs, const orbx_keyframe* const* kfs, const int* ref_kf,
                                int n_best, const orbx_keypoint* d_kp, const uint8_t* d_desc, const int* d_feat_start,
                                const int* d_feat_count, int feat_count_stride, int max_feat, const double* d_search_poses_wc,
                                const double* d_priors_wc, int list_cap, int* d_local_kf, int* d_list_offsets, int* d_list_slot,
                                double* d_positions, uint8_t* d_mp_desc, int* d_offsets, double* d_pts3d, float* d_pts2d,
                                int* d_mp_idx, int* d_feat_idx, double* d_poses_wc_out, uint8_t* d_inlier_out, double* d_err_out,
                                orbx_pnp_result* d_pnp_results, int* d_matched, int* d_matched_slot, orbx_track_result* d_results);
int orbx_map_track_local(orbx_handle* h, const orbx_camera* cam, const orbx_track_config* cfg, const orbx_pnp_config* pnp_cfg,
                         orbx_map_points* mp, int n_frames, int n_kfs, const orbx_keyframe* const* kfs, const int* ref_kf, int n_best,
                         const orbx_keypoint* kp, const uint8_t* desc, const int* feat_offsets, const double* search_poses_wc,
                         const double* priors_wc, int list_cap, int* local_kf, int* list_offsets, int* list_slot, int* offsets,
                         double* pts3d, float* pts2d, int* mp_idx, int* feat_idx, double* poses_wc_out, uint8_t* inlier_out,
                         double* err_out, orbx_pnp_result* pnp_results, int* matched, int* matched_slot, orbx_track_result* results);

/* ---- local BA from the resident map: the window collected on the device (local_ba_lm.rs:665-726, :800-897; local_mapper.rs:377-410) ----
 * collect_visual_ba_data walked a host map with hash sets and built one observation per feature for the solver to upload.  Here the
 * window is made where the slot tables, the keypoints and the store lie.  kfs [n_kfs] are the keyframes the caller considers (host
 * array, copied before the call returns; is_bad filtering = leaving a keyframe out); every index below is a position in kfs[].
 *   [spec] local = [cur] ++ best(cur, max_covisible), best as orbx_map_covisibility defines it (collect_local_keyframes, :665-683,
 *     with the covisibility list in the library's fixed order).  local[0] is the anchor and is fixed (:821); local[1..] are the K
 *     optimised keyframes, in that order.
 *   [spec] P = the distinct live slots of local's tables in first-seen order, keyframes in local order and features in index order:
 *     what ORBX_MAP_SOURCE_KEYFRAMES gives for one frame (:686-704).  M = |P|; a point's mp_idx is its position in P.
 *   [spec] c(k), for every keyframe of kfs[] = the number of features i whose table entry s satisfies 0 <= s < capacity, live[s] and
 *     s in P.  Every feature counts, repeats of a slot inside one keyframe included (:863-882 pushes one observation per feature); a
 *     keyframe without a table has c = 0.
 *   [spec] fixed = the keyframes k not in local with c(k) > 0, by ascending position in kfs[].  (The reference finds them through
 *     mp.observations in HashMap order, :707-726; here they are derived from the tables, in a fixed order.  Where every observation
 *     is associated in both directions the set is the reference's.)  F = 1 + their number: fixed index 0 is the anchor, fixed index
 *     1 + j is fixed[j].
 *   [spec] observations: the observers in the order local[0], local[1..], fixed[0..] (:889-890), each observer's counted features in
 *     index order, one orbx_ba_obs32 per counted feature: kf_idx = i - 1 for local[i], i >= 1; -1 for the anchor; -2 - j for fixed[j]
 *     (orbx_ba_obs32's coding of fixed observers); mp_idx as above; u, v = the keypoint's x, y as the f32 they are.  N = their number.
 *   [spec] M = 0 (equivalently N = 0) is ORBX_ERR_EMPTY: the reference's None (:813-815, :884-886).  K = 0 (no covisibles) is a valid
 *     collection; what the solver answers for it is the solver's.
 *
 * orbx_map_collect_ba_window_device: outputs, device memory: d_counts [4] int32 = K, F, M, N; d_local_kf [1 + max_covisible] int32,
 * -1 padded; d_fixed_kf [n_kfs] int32, entries [0, F - 1) then -1; d_list_slot [list_cap] and d_positions [list_cap][3]: P's slots and
 * positions, rows [0, M); d_obs32 [obs_cap] (16-byte aligned), rows [0, N).  list_cap must reach the bound orbx_map_track_local_device
 * states for one frame with reference cur and n_best = max_covisible; obs_cap the sum of the feature counts of kfs[].  Nothing is
 * ever truncated.  Asynchronous on the handle's stream, no host synchronisation inside; the store's tables are left as they were
 * found, and no launch is sized by the capacity: a call costs what its keyframes cost, not what the map holds.  Every output is the
 * same bytes on every run.  ORBX_ERR_INVALID before anything is enqueued: cur outside [0, n_kfs) (so n_kfs = 0: there is no cur),
 * max_covisible < 0, n_kfs > 65535, a cap below its bound, a keyframe of another handle or whose table is bound to another store.
 * orbx_map_collect_ba_window: the same with host outputs, synchronous; ORBX_ERR_EMPTY where the specification says so (counts,
 * local_kf and fixed_kf are then written, the rows are not).  With T_cw = the inverses of the keyframes' poses (optimised:
 * local[1..]; fixed: local[0], then fixed[]) its outputs are orbx_ba_solve_visual_obs32's arguments.
 *
 * orbx_map_local_ba = phases 1-3 of local_bundle_adjustment's visual branch (local_mapper.rs:377-410) on the resident map: the
 * collection with max_covisible = cfg->max_covisible_keyframes; ONE download of counts, local and fixed keyframes, P's slots and
 * positions, the only synchronisation before the solve; T_cw from the keyframes' own pose_wc; orbx_ba_solve_visual_obs32_device on
 * the observations where they lie; then, if the solve iterated (:396), the M optimised positions written to P's slots through
 * orbx_map_points_set's scatter, positions only (the point half of apply_visual_ba_results, :1125-1135).  Outputs, host memory:
 * local_kf_out [1 + max_covisible] (-1 padded), poses_wc_out [max_covisible][7]: the optimised T_wc of local[1..], rows [0, K)
 * (the keyframes are const here: the caller applies them with orbx_keyframe_set_pose, as it applies ids), counts_out [4] = K, F, M,
 * N, and the solver's scalars.  ORBX_ERR_EMPTY where the collection or the solver says so, the store untouched.  Not with an
 * all-reduce hook / communicator installed.
 * Still the caller's: ids, orbx_keyframe_set_pose, the spanning tree.  (The inertial branch: orbx_map_local_inertial_ba below.) */
int orbx_map_collect_ba_window_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int cur,
                                      int max_covisible, int list_cap, int obs_cap, int* d_counts, int* d_local_kf, int* d_fixed_kf,
                                      int* d_list_slot, double* d_positions, orbx_ba_obs32* d_obs32);
int orbx_map_collect_ba_window(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int cur,
                               int max_covisible, int list_cap, int obs_cap, int* counts, int* local_kf, int* fixed_kf, int* list_slot,
                               double* positions, orbx_ba_obs32* obs32);
int orbx_map_local_ba(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, orbx_map_points* mp, int n_kfs,
                      const orbx_keyframe* const* kfs, int cur, orbx_should_stop_fn should_stop, void* user, int* local_kf_out,
                      double* poses_wc_out, int* counts_out, int* iterations, double* initial_error, double* final_error);

/* ---- local INERTIAL BA from the resident map (local_inertial_ba.rs:366-421, :930-1030; local_mapper.rs:343-375) ----
 * Once the IMU is initialised every keyframe's local BA takes the inertial branch: the window is a temporal chain, not a covisibility
 * neighbourhood, and an observation says whether its feature has a stereo point.  kfs [n_kfs] as above (host array, copied before the
 * call returns; is_bad filtering = leaving a keyframe out, which also stands for the existence test of collect_fixed_keyframes,
 * :418-421).  chain [n_chain]: positions in kfs[], OLDEST FIRST — collect_temporal_keyframes' result (:366-384); the caller follows
 * its own prev_kf links, ids and links being the caller's.
 *   [spec] K = n_chain; chain[0] is the anchor: a window keyframe (index 0) whose observations are fixed (:1009-1013).
 *   [spec] P = the distinct live slots of the chain's tables in first-seen order, keyframes in chain order and features in index
 *     order (:387-403): what ORBX_MAP_SOURCE_KEYFRAMES gives for one frame that names the chain.  M = |P|.
 *   [spec] c(k), for every keyframe of kfs[], exactly as for the visual window: every feature counts, repeats included; no table: 0.
 *   [spec] fixed = the keyframes not in the chain with c(k) > 0, by ascending position in kfs[].  F = 1 + their number: fixed index 0
 *     is the anchor (:973-978), fixed index 1 + j is fixed[j].
 *   [spec] observations: the observers in the order chain[0], chain[1..], fixed[0..], each observer's counted features in index
 *     order, one orbx_ba_obs32 each: kf_idx = i for chain[i], i >= 1 (window index 0 never occurs); -1 for chain[0]; -2 - j for
 *     fixed[j].  mp_idx = the position in P, OR ORBX_BA_OBS32_STEREO where the observer's has_point[feature] != 0 (:1006-1007; a
 *     keyframe created without d_has_point never sets it).  u, v = the keypoint's x, y as the f32 they are.  N = their number.
 * orbx_map_collect_inertial_window_device: outputs, device memory: d_counts [4] int32 = K, F, M, N; d_fixed_kf [n_kfs] int32, entries
 * [0, F - 1) then -1; d_list_slot [list_cap], d_positions [list_cap][3]: rows [0, M); d_obs32 [obs_cap] (16-byte aligned): rows
 * [0, N).  list_cap must reach the chain's feature counts summed, at most the capacity; obs_cap the feature counts of kfs[] summed.
 * Asynchronous on the handle's stream; the store's tables are left as found; no launch is sized by the capacity; every output is the
 * same bytes on every run.  ORBX_ERR_EMPTY, before anything is enqueued: n_chain < 2 (:940-942).  ORBX_ERR_INVALID, before anything
 * is enqueued: a chain entry outside [0, n_kfs) or listed twice, n_kfs > 65535, a cap below its bound, a keyframe of another handle
 * or whose table is bound to another store.
 * orbx_map_collect_inertial_window: the same with host outputs, synchronous; M = 0 (:946-948) is ORBX_ERR_EMPTY with counts and
 * fixed_kf written and no rows.  With poses_wc = the chain's poses and fixed T_cw = the inverses of the anchor's and fixed[]'s poses
 * its outputs are orbx_ba_solve_inertial_obs32's arguments.
 *
 * orbx_map_local_inertial_ba = phases 1-3 of the inertial branch (local_mapper.rs:343-375): the collection; ONE download of counts,
 * fixed keyframes, P's slots and positions; poses_wc from kfs[chain[i]]'s pose_wc and the fixed T_cw from the anchor and fixed[];
 * orbx_ba_solve_inertial_obs32_device on the observations where they lie; then, if the solve iterated (:363), the M positions written
 * to P's slots, positions only.  velocities [K][3], biases [K][6], edge_kf [E][2] (window indices = positions in chain[]) and
 * preint [E][11] are the caller's, as for orbx_ba_solve_inertial (build_imu_edges is a loop over preintegrations the host holds);
 * every rule for them holds, and they are checked before anything is enqueued.  Outputs, host memory, for all K keyframes:
 * poses_wc_out [K][7], vel_out [K][3], bias_out [K][6]; fixed_kf_out [n_kfs]; counts_out [4]; the solver's scalars.  The keyframes are
 * const: the caller applies orbx_keyframe_set_pose and keeps velocities and biases.  ORBX_ERR_EMPTY / ORBX_ERR_INVALID as the parts
 * define them (more than 51 keyframes: the solver's), the store untouched.  Not with an all-reduce hook / communicator installed. */
int orbx_map_collect_inertial_window_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs,
                                            int n_chain, const int* chain, int list_cap, int obs_cap, int* d_counts, int* d_fixed_kf,
                                            int* d_list_slot, double* d_positions, orbx_ba_obs32* d_obs32);
int orbx_map_collect_inertial_window(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_chain,
                                     const int* chain, int list_cap, int obs_cap, int* counts, int* fixed_kf, int* list_slot,
                                     double* positions, orbx_ba_obs32* obs32);
int orbx_map_local_inertial_ba(orbx_handle* h, const orbx_camera* cam, const orbx_inertial_ba_config* cfg, orbx_map_points* mp,
                               int n_kfs, const orbx_keyframe* const* kfs, int n_chain, const int* chain, const double* velocities,
                               const double* biases, int E, const int* edge_kf, const double* preint,
                               orbx_should_stop_fn should_stop, void* user, double* poses_wc_out, double* vel_out, double* bias_out,
                               int* fixed_kf_out, int* counts_out, int* iterations, double* initial_error, double* final_error);

/* ---- global BA from the resident map (src/optimizer/global_ba.rs:100-181, :184-418; loop_closer.rs:237-240) ----
 * collect_global_ba_data where the slot tables lie.  kfs [n_kfs] is the caller's list of the map's keyframes in ascending id (host
 * array, copied before the call returns; is_bad filtering = leaving a keyframe out).
 *   [spec] kfs[0] is the anchor (:124); kfs[1..] are the K = n_kfs - 1 optimised keyframes in that order.
 *   [spec] P = the distinct slots s with 0 <= s < capacity and live[s] of all tables in first-seen order, keyframes in list order,
 *     features in index order; M = |P|.  A keyframe without a table observes nothing.
 *   [spec] one orbx_ba_obs32 per feature whose table entry is in P (a slot repeated inside a keyframe: one per feature), keyframes in
 *     list order, features in index order: kf_idx = i - 1 (-1: the anchor), mp_idx = the position in P, u, v = the keypoint's f32.
 *     N is their number.
 * orbx_map_collect_global_device: asynchronous on the handle's stream; outputs in device memory: d_counts [4] = (K, 1, M, N),
 * d_list_slot [list_cap], d_positions [list_cap][3] (rows [0, M)), d_obs32 [obs_cap] (rows [0, N), 16-byte aligned).  Nothing is
 * truncated: list_cap >= min(the keyframes' features summed, capacity) and obs_cap >= the features summed, else ORBX_ERR_INVALID before
 * anything is enqueued, as for n_kfs <= 0, n_kfs > 65535, a keyframe of another handle or whose table is bound to another store.  The
 * same bytes come out on every run; the store and the tables are left as found.
 * orbx_map_collect_global: the same with host outputs, synchronous; M == 0 (:176-178) is ORBX_ERR_EMPTY with counts written and no
 * rows.  With T_cw = the inverses of the keyframes' poses its outputs are orbx_ba_solve_global_map_obs32's arguments.
 * orbx_map_global_ba = run_global_ba's device half: the collection; ONE download of counts, P's slots and positions; T_cw from the
 * keyframes' own pose_wc; orbx_ba_solve_global_map_obs32_device on the observations where they lie; then, if the solve iterated, the M
 * positions written to P's slots, positions only.  poses_wc_out [n_kfs - 1][7] (host), counts_out [4] and the solver's scalars go to
 * the caller, who applies the poses with orbx_keyframe_set_pose: the keyframes are const.  ORBX_ERR_EMPTY for n_kfs < 2 or M == 0,
 * ORBX_ERR_INVALID for more optimised keyframes than orbx_ba_global_map_max_keyframes() (before anything is enqueued) and with an
 * all-reduce hook / communicator installed; the store is then untouched. */
int orbx_map_collect_global_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int list_cap,
                                   int obs_cap, int* d_counts, int* d_list_slot, double* d_positions, orbx_ba_obs32* d_obs32);
int orbx_map_collect_global(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int list_cap, int obs_cap,
                            int* counts, int* list_slot, double* positions, orbx_ba_obs32* obs32);
int orbx_map_global_ba(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, orbx_map_points* mp, int n_kfs,
                       const orbx_keyframe* const* kfs, orbx_should_stop_fn should_stop, void* user, double* poses_wc_out,
                       int* counts_out, int* iterations, double* initial_error, double* final_error);

/* ---- observations from the resident map: lists, refresh, redundancy (map_point.rs:140-156; local_mapper.rs:421-469, :487-583) ----
 * mp.observations — which keyframes see a point, and at which feature — is the inverse of the slot tables.  Like the covisibility
 * graph it is derived from the tables where they lie instead of maintained per association.  kfs [n_kfs] are the keyframes the
 * caller considers (host array, copied before the call returns; is_bad filtering = leaving a keyframe out); every keyframe index
 * below is a position in kfs[].
 *   [spec] obs(k) is covisibility's: the distinct slots s of kfs[k]'s table with 0 <= s < capacity and live[s] when the kernels run.
 *     The feature that observes s in k is the FIRST feature that names it.  (The reference's HashMap<KeyFrameId, usize> holds one
 *     feature per keyframe and the last add_observation wins; here the choice is fixed.  Where every point is associated once per
 *     keyframe the two agree.)  A keyframe without a table observes nothing.
 *   [spec] observations(s) = the pairs (k, feat) with s in obs(k), by ascending k.  (The reference iterates a HashMap;
 *     orbx_refresh_map_points takes "the order as given", and this is the order given.)
 *   [spec] n_observers(s) = |observations(s)|.
 * Every call below has a _device form — asynchronous on the handle's stream, no host synchronisation inside, outputs in device
 * memory — and a host form: synchronous, one download, outputs packed.  The store's tables are left as they were found and no
 * launch is sized by the capacity: a call costs what its keyframes and points cost.  Every output is the same bytes on every run.
 * ORBX_ERR_INVALID before anything is enqueued, the store and the outputs untouched: n_kfs > 65535, a keyframe of another handle or
 * whose table is bound to another store, and what each call adds.
 *
 * orbx_map_observations[_device]: slots [M] are the points asked for, a HOST array in both forms, checked like orbx_map_points_set's:
 * ORBX_ERR_INVALID for a slot outside [0, capacity), a slot listed twice, or a slot that is not live.  Point p owns rows
 * [obs_start[p], obs_start[p+1]) of obs_kf / obs_feat; obs_start [M+1], obs_start[0] = 0.  obs_cap, the rows obs_kf and obs_feat
 * hold, must reach the sum of the feature counts of kfs[] (else ORBX_ERR_INVALID); nothing is ever truncated.  The outputs are the
 * arguments orbx_refresh_map_points_device takes, with T = n_kfs.  The observation test of map-point culling (map_point.rs:140-156,
 * local_mapper.rs:421-469) is obs_start[p+1] - obs_start[p] < min_observations; found_ratio is 1.0 in the reference (nothing
 * increments its counters); the grace period, ids and is_bad stay with the caller.
 *
 * orbx_map_refresh_points[_device] = phase 4 of search_in_neighbors on the resident map: the lists above for slots [M] (HOST array,
 * checked as above); then orbx_refresh_map_points's launches, unchanged, on the resident keyframes' own descriptors, their camera
 * centres (the translation of pose_wc, as orbx_keyframe_refresh_map_points takes them) and the points' positions and current
 * descriptors read from the store; then the chosen descriptors written back into the store's slots through orbx_map_points_set's
 * scatter, descriptors only.  mp_desc [M][32] out, normals [M][3] in/out (the store keeps none), min_distance / max_distance [M],
 * records [M] (device form: mp_desc and normals 8-byte aligned).  Every output equals, byte for byte,
 * orbx_keyframe_refresh_map_points called with the specification's lists and the store's rows; afterwards
 * orbx_map_points_download of slots gives mp_desc.  Positions and live bytes are untouched.  M = 0: ORBX_OK.
 *
 * orbx_map_keyframe_redundancy[_device] = the decision of cull_keyframes (local_mapper.rs:487-583) for n_cand candidates at once; the
 * reference collects to_cull before it removes anything, so every candidate's decision is independent.  cand [n_cand] is a HOST
 * array of positions in kfs[] (an index may repeat); the caller leaves out the current keyframe, roots and bad keyframes (:516-533)
 * and finds "covisible with current" by orbx_map_covisibility's weights > 0.
 *   [spec] total(c) = the features of kfs[c] whose table entry s satisfies 0 <= s < capacity and live[s]; every feature counts,
 *     repeats of a slot included (:539-547 walks map_point_ids).
 *   [spec] redundant(c) = those of them with n_observers(s) - 1 >= min_observations (c itself is one of the observers, :549-555).
 *   [spec] cull(c) = total > 0 && (double)redundant / (double)total > threshold: one IEEE f64 division (:561-565; 0.9, or 0.5).
 *   A candidate without a table gives 0, 0, 0.
 * Outputs total / redundant [n_cand] int32, cull [n_cand] u8.  ORBX_ERR_INVALID also for an index outside [0, n_kfs),
 * min_observations < 0, n_cand > 65535.  n_cand = 0: nothing is done, ORBX_OK.
 * Still the caller's: removal itself (IMU preintegration merging, the spanning tree, ids), normals; of search_in_neighbors the
 * choice of the neighbours (the fuse and merge phases: the next block). */
int orbx_map_observations_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots,
                                 int obs_cap, int* d_obs_start, int* d_obs_kf, int* d_obs_feat);
int orbx_map_observations(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots,
                          int obs_cap, int* obs_start, int* obs_kf, int* obs_feat);
int orbx_map_refresh_points_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots,
                                   double scale_range, uint8_t* d_mp_desc, double* d_normals, double* d_min_distance, double* d_max_distance,
                                   orbx_mp_refresh_record* d_records);
int orbx_map_refresh_points(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* slots,
                            double scale_range, uint8_t* mp_desc, double* normals, double* min_distance, double* max_distance,
                            orbx_mp_refresh_record* records);
int orbx_map_keyframe_redundancy_device(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_cand,
                                        const int* cand, int min_observations, double threshold, int* d_total, int* d_redundant,
                                        uint8_t* d_cull);
int orbx_map_keyframe_redundancy(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n_cand,
                                 const int* cand, int min_observations, double threshold, int* total, int* redundant, uint8_t* cull);

/* ---- fuse and merge on the resident map (search_in_neighbors.rs:240-390, map.rs:770-...: merge_map_points) ------------------------
 * fuse_points_into_keyframes walks points x targets sequentially and mutates as it goes: a match on a feature without a point is
 * associated, a match on a feature with another point merges the two, the point with more observations keeps (the projected one
 * on ties), the goner's observers are re-pointed or erased.  Its outcome depends on orders the reference leaves to HashSet
 * iteration (neighbor_ids, neighbor_only_mps, the goner's observations) and on counts that change during the walk; the library fixes
 * a derived, deterministic definition of ONE PASS fuse(src, tgt).  kfs [n_kfs], src [n_src], tgt [n_tgt] are host arrays (copied
 * before the call returns); src and tgt hold positions in kfs[].  All reads are of the state at entry to the pass; obs(k),
 * n_observers(s) and "live" are those of the observations block, over kfs[].
 *   [spec] L = the distinct live slots of the tables of kfs[src[0..n_src)] in first-seen order: what ORBX_MAP_SOURCE_KEYFRAMES gives
 *     one frame.  P = |L|.
 *   [spec] search: for point j (p = L[j]) and target t, match[j][t] = -1 if p is in obs(tgt[t]) (:272); otherwise the feature that
 *     orbx_keyframe_fuse_search returns for the store's position and descriptor of p against kfs[tgt[t]], or -1 — bit for bit the
 *     existing search, with the same inverse of pose_wc made on the host the same way.
 *   [spec] classes: a match (j, t, f) with e = table(tgt[t])[f], the entry read WITH repeats: if 0 <= e < capacity and live[e], p and
 *     e are the same point; otherwise p CLAIMS (t, f), and all points that claim one feature are the same point.  Classes are the
 *     connected components over slots.
 *   [spec] keeper of a class = the member with the largest n_observers; ties go to the member earliest in L, a tied member that is
 *     not in L comes after all those in L, by ascending slot.  Every other member of a class of two or more is a GONER.
 *   [spec] tables: for every keyframe k of kfs[] and every class C that has a claim or at least two members, G = the features of k
 *     whose entry is a live member of C together with the features of k claimed by members of C.  If a feature of G already names
 *     the keeper, the features naming the keeper stay and all others of G become -1; otherwise the lowest-indexed feature of G gets
 *     the keeper and the others become -1.  Nothing else in any table changes; a keyframe that is not in kfs[] is not touched: the
 *     caller passes every keyframe that may observe the points involved.
 *   [spec] outputs: counts[4] = {P, matches, added, goners} (added: the features whose entry went from "no live point" to a slot),
 *     list_slot [P], match [P][n_tgt], goner[] / keeper[] by ascending goner slot.
 * Deviations from the sequential reference: counts are those at entry (the reference's grow as it associates); a projected point
 * that loses a merge still contributes its later matches to its class (the reference drops them: the point no longer exists); the
 * orders above are fixed.  Where every class has at most two members, no feature is matched twice, every merge keeps the projected
 * point and the two counts of a merged pair differ by more than n_tgt, the pass equals the reference replayed in L order and target
 * order.
 * Liveness: the store keeps a host mirror of its live bytes, so the device form leaves them alone.  After the pass no table of
 * kfs[] names a goner, and the goner list is an output (the caller needs it anyway to retire ids).  Positions, descriptors,
 * d_mp_flag and mp_ids are untouched (merge_map_points changes none of them).  d_mp_uniq of every keyframe whose table changed is
 * made again.  A target without a table is given one, every entry -1, when the call is accepted: to every reader the same thing.
 *
 * orbx_map_fuse_device: asynchronous on the handle's stream, no host synchronisation inside; the store's tables are left as found
 * and no launch is sized by the capacity; the outputs are the same bytes on every run.  list_cap, the rows d_list_slot holds (and
 * d_match rows of n_tgt), must reach L's bound: the features of kfs[src[..]] summed, at most the capacity.  d_goner / d_keeper hold
 * that bound + the sum of the targets' feature counts.  d_counts [4].
 * orbx_map_fuse: the same with host outputs, synchronous, one download; the goners are then erased as orbx_map_points_erase does.
 * ORBX_ERR_INVALID before anything is enqueued, tables, store and outputs untouched: an index outside [0, n_kfs), a target listed
 * twice, a keyframe listed twice in kfs[], n_kfs > 65535, desc_threshold > 256, list_cap below its bound, a keyframe of another
 * handle or bound to another store.  n_src = 0, n_tgt = 0 or P = 0: ORBX_OK, counts written and nothing else.
 *
 * orbx_map_search_in_neighbors = phases 2 to 4 of search_in_neighbors for the current keyframe kfs[cur] and neighbours nb [n_nb]
 * (positions in kfs[], none twice, none of them cur; choosing them — orbx_map_covisibility's best list, the secondaries, the temporal
 * chain — stays with the caller): pass A = fuse([cur], nb); pass B = fuse(nb, [cur]) on the tables as A left them, enqueued behind A
 * with no synchronisation between; ONE download of both passes' counts and goner lists and of the affected list; the erase;
 * orbx_map_refresh_points on the affected list.  The affected list is the distinct live slots of [cur] ++ nb after both passes in
 * first-seen order, made by the selection kernels.  counts [8]: pass A's four, then pass B's; goner_a / keeper_a / goner_b /
 * keeper_b hold goner_cap rows each, at least the larger of the two passes' bounds above; affected_slot and the refresh outputs
 * (mp_desc [..][32], normals [..][3], min_distance, max_distance, records: orbx_map_refresh_points's, in the affected list's order)
 * hold affected_cap rows, at least the features of cur and nb[] summed, at most the capacity.  slot_normals [capacity][3] (NULL:
 * zeros) gives every slot's normal before the call: the store keeps none.  The refusals are those above.
 *
 * orbx_keyframe_get_map_point_slots: the table as it lies in device memory (every entry -1 without one); synchronous.
 * Still the caller's: the choice of the neighbours, ids and the id -> slot map (goner / keeper and the tables read back say what to
 * apply), normals; removal: orbx_map_remove_points, below. */
int orbx_keyframe_get_map_point_slots(const orbx_keyframe* kf, int* slots);
int orbx_map_fuse_device(orbx_handle* h, const orbx_camera* cam, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int n_src,
                         const int* src, int n_tgt, const int* tgt, double radius_scale, unsigned desc_threshold, int list_cap,
                         int* d_counts, int* d_list_slot, int* d_match, int* d_goner, int* d_keeper);
int orbx_map_fuse(orbx_handle* h, const orbx_camera* cam, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int n_src,
                  const int* src, int n_tgt, const int* tgt, double radius_scale, unsigned desc_threshold, int list_cap, int* counts,
                  int* list_slot, int* match, int* goner, int* keeper);
int orbx_map_search_in_neighbors(orbx_handle* h, const orbx_camera* cam, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, int cur,
                                 int n_nb, const int* nb, double radius_scale, unsigned desc_threshold, double scale_range,
                                 const double* slot_normals, int goner_cap, int affected_cap, int* counts, int* goner_a, int* keeper_a,
                                 int* goner_b, int* keeper_b, int* n_affected, int* affected_slot, uint8_t* mp_desc, double* normals,
                                 double* min_distance, double* max_distance, orbx_mp_refresh_record* records);

/* ---- create and cull map points on the resident map (local_mapper.rs:105-142: steps 2, 3, 3b and 5 of process_keyframe) -------------
 * The steps of process_keyframe that WRITE the tables and the store, so that a keyframe goes extractor -> tracking -> insertion ->
 * new points -> fuse -> BA -> cull with its tables never leaving the device.  Conventions are those of the fuse block: kfs / nbs /
 * free_slots / slots / cand are host arrays copied before the call returns, all work is ordered on the handle's stream, a refusal
 * is ORBX_ERR_INVALID before anything is enqueued with tables, store and outputs untouched, the outputs are the same bytes on every
 * run, no launch is sized by the capacity, and "names a live point" means an entry s with 0 <= s < capacity and live[s].
 *
 * orbx_keyframe_set_map_point_slots_device (step 2, associate_matched_points :208-223): orbx_keyframe_set_map_point_slots from a
 * device array d_slots [n] (4-byte aligned), e.g. the tracker's d_matched_slot row; asynchronous, no synchronisation.
 *   [spec] a value outside [-1, capacity) is stored as -1: the host cannot check it without a wait.
 *   d_mp_uniq is made on the device (the first feature that names a slot keeps it); on in-range input the table and d_mp_uniq are
 *   byte for byte the host form's.
 *
 * orbx_map_create_points[_device] (steps 3 and 3b: triangulate_new_points :232-268, triangulate_from_neighbors triangulation.rs:71-308
 * with create_map_point and the associate calls).  phases: ORBX_MAP_CREATE_STEREO | ORBX_MAP_CREATE_NEIGHBOURS.  free_slots [n_free]:
 * the slots the new points take, in creation order (the caller owns the id -> slot map); every list holds n_free rows and only
 * created points are listed.  All reads are of the state at entry unless said.
 *   [spec] flag(k, i) = the table of keyframe k names a live point at feature i.  A keyframe without a table has every flag 0 and is
 *     given a table of -1 when the call is accepted.  d_mp_flag and mp_ids are neither read nor written.
 *   [spec] stereo phase: the candidates are the features i of cur in ascending i with has_point[i] && !flag(cur, i); S is their number.
 *     Candidate r takes free_slots[r] if r < n_free: position pose_wc(cur) * points_cam[i] (rotation matrix, then translation),
 *     descriptor = cur's row i, table(cur)[i] = the slot, listed with new_neighbour = -1 and new_idx2 = -1.  A candidate with
 *     r >= n_free is dropped: no slot, no table write, its flag stays 0.  S' = min(S, n_free).
 *   [spec] neighbour phase: the searches, the pair loop, the ordered compaction and stats [T][4] of
 *     orbx_keyframe_triangulate_from_neighbors(cur, nbs[0..T)), with flag(cur, .) | "given a slot by the stereo phase" and
 *     flag(nbs[t], .) in place of the keyframes' d_mp_flag.  N = the validated pairs, in creation order (neighbour, then the search's
 *     pair order).  Pair e takes free_slots[S' + e] if that exists: the triangulated position, descriptor = cur's row idx1
 *     (triangulation.rs:280), table(nbs[t])[idx2] = the slot, and table(cur)[idx1] = the slot of the LAST created pair with that idx1:
 *     the reference clones the current keyframe's flags before the loop (:94-107), so one feature is matched in several neighbours
 *     and each associate overwrites the one before (:289).
 *   [spec] counts [4] = {S, N, created, dropped}, created = min(S + N, n_free), dropped = S + N - created.
 *   Deviation: the earlier points of a feature matched in several neighbours are created all the same and are observed by their
 *   neighbour only (observations are derived from the tables); the reference's mp.observations still lists the current keyframe.
 *   d_mp_uniq of every keyframe whose table changed is made again.
 *   PRECONDITION (the caller's): no table names a slot handed over as free — orbx_map_remove_points guarantees it.
 * orbx_map_create_points_device: asynchronous, no host synchronisation inside; the epipolar geometry and the node ranges are made on
 *   the host and go up with the other tables.  It leaves the store untouched (positions, descriptors, live bytes, mirror): the
 *   caller makes the points live with orbx_map_points_set_device(mp, free_slots, created, d_new_points, d_new_desc) once it has read
 *   d_counts; until then every reader skips the new entries as not live.  d_new_desc [n_free][32] is 16-byte aligned.
 * orbx_map_create_points: the device form into a workspace, ONE download (counts, lists, stats), then that set_device for the first
 *   `created` slots: orbx_map_points_download of new_slot gives new_points and the descriptor rows byte for byte.
 * Refused: T outside [0, 256], max_descriptor_dist > 256, cur among nbs or a neighbour twice, a keyframe of another handle or bound to
 * another store, phases outside 1..3, n_free < 0, a free slot outside [0, capacity), listed twice or live.  n_free = 0 is accepted:
 * counts and stats are written, nothing else.
 *
 * orbx_map_remove_points (remove_map_point_full, map.rs:609-631, for a list): every entry, repeats included, of d_mp_slot and
 * d_mp_uniq of kfs[] that names a listed slot becomes -1, then the slots are erased as orbx_map_points_erase does.  slots [n] is
 * checked like erase's (repeats allowed); a slot that is not live is accepted and its stale entries are purged too.  n_cleared: the
 * table entries (of d_mp_slot) cleared — NULL: nothing is downloaded and the call does not wait; else one 4-byte download.  A keyframe
 * outside kfs[] is not touched; a keyframe twice in kfs[] is refused.
 *
 * orbx_map_cull_points (cull_map_points :421-469): cand [M] is checked like orbx_map_observations' slots (in range, once, live).
 *   [spec] culled = the candidates with n_observers(s) < min_observations (the observations block's count over kfs[]), in cand order;
 *   then orbx_map_remove_points on them.  Synchronous, one download (the counts: the store's mirror needs the list).
 * found_ratio is 1.0 in the reference and its in-grace rule (:443) can never fire, because nothing increments visible_count; the
 * grace period and is_bad are the caller's, exercised through its choice of cand.
 * Still the caller's: ids and the id -> slot map, the choice of the neighbours, growth of the store, normals, keyframe removal. */
#define ORBX_MAP_CREATE_STEREO 1
#define ORBX_MAP_CREATE_NEIGHBOURS 2
int orbx_keyframe_set_map_point_slots_device(orbx_keyframe* kf, const orbx_map_points* mp, const int* d_slots);
int orbx_map_create_points_device(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                                  orbx_map_points* mp, orbx_keyframe* cur, orbx_keyframe* const* nbs, int T, int phases,
                                  const int* free_slots, int n_free, int* d_counts, int* d_new_slot, int* d_new_neighbour,
                                  int* d_new_idx1, int* d_new_idx2, double* d_new_points, uint8_t* d_new_desc, int* d_stats);
int orbx_map_create_points(orbx_handle* h, const orbx_camera* cam, const orbx_triangulation_config* cfg, int is_inertial,
                           orbx_map_points* mp, orbx_keyframe* cur, orbx_keyframe* const* nbs, int T, int phases, const int* free_slots,
                           int n_free, int* counts, int* new_slot, int* new_neighbour, int* new_idx1, int* new_idx2, double* new_points,
                           int* stats);
int orbx_map_remove_points(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int n, const int* slots,
                           int* n_cleared);
int orbx_map_cull_points(orbx_handle* h, orbx_map_points* mp, int n_kfs, const orbx_keyframe* const* kfs, int M, const int* cand,
                         int min_observations, int* n_culled, int* culled);

/* ---- loop correction on the resident map: rigid correction and fuse (corrector.rs:383-619; loop_closer.rs:155-241, step 5) ------
 * correct_loop — collect_correction_data, compute_correction, apply_correction, fuse_map_points — where the slot tables, the store
 * and the poses lie.  The reference walks host hash maps in their iteration order and merges with counts that change as it goes; the
 * library fixes a derived, deterministic definition.  kfs [n_kfs], parent [n_kfs] and sim3 [8] are host arrays (copied before the
 * call returns); every keyframe index is a position in kfs[].  parent[k] is keyframe k's spanning-tree parent or -1; sim3 is
 * sim3_current_to_loop as orbx_keyframe_verify_loop_candidates writes it (qw, qx, qy, qz, tx, ty, tz, scale), feature_matches that
 * call's [n_matches][2] (current feature, loop feature).  All reads are of the state at entry; obs(k), n_observers(s), "live" and
 * weight are those of the covisibility and observations blocks, over kfs[].
 *   [spec] affected keyframes A (:433-465): arcs k -> c for parent[c] == k (a parent is not reached from its child) and k <-> j for
 *     weight(k, j) >= min_covisibility_weight; A = the keyframes at most max_propagation_depth arcs from cur.  The reference's FIFO
 *     walk gives this set whatever order it visits neighbours in.  (With min_covisibility_weight = 0 every pair is an arc; the
 *     reference walks the keyframes it has weights for.)  affected[k] = 1 for k in A, else 0.
 *   [spec] affected points (:467-480): the distinct live slots of the tables of A's keyframes, keyframes by ascending position and
 *     features in index order — what ORBX_MAP_SOURCE_KEYFRAMES gives one frame — in list_slot; counts[1] of them.
 *   [spec] correction (:493-515, sim3.rs:144-170): C = sim3^-1: q_c = the conjugate of sim3's quaternion, s_c = 1 / scale,
 *     t_c = -(R_c t) * s_c.  Every affected point's position in the store becomes s_c * (R_c p) + t_c, once, however many keyframes
 *     and features name it.  Every affected keyframe's pose becomes rotation q_c * q, translation s_c * (R_c t_wc) + t_c, the scale
 *     dropped (to_se3); the quaternion product is not renormalised and its sign is left as it falls.  poses_wc[k] is that pose for
 *     k in A and the pose as found otherwise.  Bytes of unaffected slots do not change.
 *   [spec] pairs (:168-173): match (fc, fl) gives (a, b) = (table(cur)[fc], table(loop)[fl]); it counts iff both are in range and live
 *     and a != b.  counts[2] = their number.
 *   [spec] fuse (:572-619), order-free like the fuse block: classes are the connected components over the pairs; the keeper of a
 *     class is the member with the largest n_observers at entry, ties to the member that occurs first in the flattened pair list
 *     a0, b0, a1, b1, ... (a two-member tie keeps the current keyframe's point, as :589 does); every other member is a GONER.  In
 *     every table of kfs[] an entry that names a goner becomes its keeper; nothing else changes; d_mp_uniq of the changed keyframes
 *     is made again.  goner[] / keeper[] by ascending goner slot; counts[4] = {|A|, affected points, pairs, goners}.
 * Deviations from the sequential reference: counts are those at entry (the reference's grow as it merges); a goner named at two
 * features of one keyframe is replaced at both (the reference's observations map holds one feature per keyframe); a keyframe that
 * already names the keeper may afterwards name it at two features, as in the reference — every reader of the tables counts such a
 * slot once.  Where no slot occurs in two distinct pairs the result equals the reference replayed in list order.  Keepers' positions
 * are the corrected ones; descriptors, d_mp_flag and mp_ids are untouched.  The pose graph stays out: the reference never solves it.
 *
 * orbx_map_correct_loop_device: asynchronous on the handle's stream, no host synchronisation inside; the N x N weights are counted
 * by the covisibility kernels with every keyframe as a query and never leave the device (int32, at most 64 MB at
 * orbx_map_loop_max_keyframes() = 4096 keyframes); the store's mark / index tables are left as found, no launch is sized by the
 * capacity and the outputs are the same bytes on every run.  d_feature_matches [n_matches][2] is device memory; a match outside its
 * keyframe's features is no pair.  Outputs, device memory: d_counts [4], d_affected [n_kfs] bytes, d_poses_wc [n_kfs][7],
 * d_list_slot [list_cap], list_cap >= min(the features of kfs[] summed, capacity); d_goner / d_keeper [n_matches] (goners <= pairs).
 * The keyframes' own pose_wc and the store's live bytes are left alone: the caller applies poses_wc and erases the goners.
 * orbx_map_correct_loop: the same with host arrays, synchronous: ONE download of the counts, affected bytes, poses, list and goner
 * lists; the poses of A applied as orbx_keyframe_set_pose does; the goners erased as orbx_map_points_erase does.
 * orbx_map_close_loop = orbx_map_correct_loop, then, if ba_cfg is given, orbx_map_global_ba on the same kfs[] by its own rules
 * (kfs[0] the anchor, the list in ascending id; its return value is the call's); poses_wc_out goes to the caller unapplied, as that
 * call leaves it.
 * ORBX_ERR_INVALID before anything is enqueued, store, tables and poses untouched: cur or a parent entry outside its range,
 * parent[k] == k, loop outside [0, n_kfs) ([spec] -1 is accepted where n_matches == 0: no loop keyframe is read), cur == loop,
 * n_kfs > orbx_map_loop_max_keyframes(), a keyframe listed twice, a keyframe of another handle or store, cur or loop without a table
 * while n_matches > 0, a match index outside its keyframe (host form), a sim3 entry that is not finite or a scale <= 0, a negative
 * configuration value, list_cap below its bound, n_matches < 0.  n_kfs = 0: ORBX_OK and nothing is done.
 * Still the caller's: ids and the id -> slot map (goner / keeper say what to retire), the spanning tree, the loop edge. */
typedef struct {
  int min_covisibility_weight, max_propagation_depth;   /* 15, 100: corrector.rs:97-104 */
} orbx_loop_correct_config;
void orbx_default_loop_correct_config(orbx_loop_correct_config* cfg);
int orbx_map_loop_max_keyframes(void);                  /* 4096 */
int orbx_map_correct_loop_device(orbx_handle* h, const orbx_loop_correct_config* cfg, orbx_map_points* mp, int n_kfs,
                                 orbx_keyframe* const* kfs, const int* parent, int cur, int loop, const double* sim3, int n_matches,
                                 const int* d_feature_matches, int list_cap, int* d_counts, uint8_t* d_affected, double* d_poses_wc,
                                 int* d_list_slot, int* d_goner, int* d_keeper);
int orbx_map_correct_loop(orbx_handle* h, const orbx_loop_correct_config* cfg, orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs,
                          const int* parent, int cur, int loop, const double* sim3, int n_matches, const int* feature_matches,
                          int list_cap, int* counts, uint8_t* affected, double* poses_wc, int* list_slot, int* goner, int* keeper);
int orbx_map_close_loop(orbx_handle* h, const orbx_camera* cam, const orbx_loop_correct_config* correct_cfg, const orbx_ba_config* ba_cfg,
                        orbx_map_points* mp, int n_kfs, orbx_keyframe* const* kfs, const int* parent, int cur, int loop,
                        const double* sim3, int n_matches, const int* feature_matches, int list_cap, int* counts, uint8_t* affected,
                        double* poses_wc, int* list_slot, int* goner, int* keeper, orbx_should_stop_fn should_stop, void* user,
                        double* poses_wc_out, int* ba_counts, int* iterations, double* initial_error, double* final_error);

/* ---- keyframe BoW database and loop-candidate search (src/atlas/keyframe_db.rs, src/loop_closing/detector.rs) ------
 * Replaces KeyFrameDatabase (keyframe_db.rs:36-95: add / erase / detect_candidates, the relocalisation query over all maps) and
 * detect_loop_candidates (detector.rs:185-368, called for every keyframe by LoopCloser::process_keyframe, loop_closer.rs:155-170).
 * The BowVectors live in device memory as orbx_bow_vectors[_device] returns them (ascending u32 word ids, f64 weights, at most
 * 8192 words); a call scores one query or a batch of queries against every entry in one launch.  Two scorings
 * (compute_bow_score with and without a vocabulary, detector.rs:371-388):
 *   ORBX_KFDB_SCORE_L1   OrbVocabulary::score (vocabulary/mod.rs:357-374): exactly orbx_bow_score of the pair;
 *   ORBX_KFDB_SCORE_DOT  sum of w1 * w2 over the common words (keyframe_db.rs:73-79, detector.rs:380-386), product then add,
 *                        [spec] in ascending word id (the reference walks a HashMap).
 * Every score is one serial f64 sum per pair, bit for bit the host arithmetic, so that every comparison and ordering below is the
 * restatement's.  [spec] equal scores are ordered by ascending keyframe id (the reference's stable sort leaves them in HashMap
 * order).  An entry also carries its map index and the keyframe's is_bad flag (detector.rs:334).
 * A database belongs to the handle it was made with and works on that handle's stream; it is not thread-safe.  erase / replace
 * leave tombstones that a later query call compacts away once they outnumber the entries (or orbx_kfdb_compact at once). */
typedef struct orbx_kfdb orbx_kfdb;
enum { ORBX_KFDB_SCORE_L1 = 0, ORBX_KFDB_SCORE_DOT = 1 };
/* = LoopDetectorConfig, detector.rs:17-46; orbx_default_loop_detector_config: 0.75, 3, 5, 10, 30.  The integer fields must be
 * >= 0 and min_score_ratio not NaN; other values -> ORBX_ERR_INVALID.  consistency_threshold is the ConsistencyChecker's (host
 * code of the mirrors); the searches do not read it. */
typedef struct {
  double min_score_ratio;
  int consistency_threshold, min_covisibles_for_threshold, max_covisibles_to_check, min_temporal_gap;
} orbx_loop_detector_config;
void orbx_default_loop_detector_config(orbx_loop_detector_config* cfg);

int orbx_kfdb_create(orbx_handle* h, orbx_kfdb** out);
void orbx_kfdb_destroy(orbx_kfdb* db);
/* KeyFrameDatabase::add (keyframe_db.rs:45-47): an id that exists is replaced.  word [n] strictly ascending (else
 * ORBX_ERR_INVALID, as orbx_bow_score), weight [n], 0 <= n <= 8192, map_index >= 0.  Host pointers; synchronous. */
int orbx_kfdb_add(orbx_kfdb* db, uint64_t keyframe_id, int map_index, int is_bad, const uint32_t* word, const double* weight, int n);
/* The same from device memory, with the word count a device value: d_word / d_weight [max_n], n = *d_count clamped to
 * [0, max_n].  The outputs of orbx_bow_vectors_device go straight in (d_bow_word, d_bow_weight, d_counts).  Asynchronous on the
 * handle's stream, no host synchronisation; the word ids are trusted to ascend. */
int orbx_kfdb_add_device(orbx_kfdb* db, uint64_t keyframe_id, int map_index, int is_bad, const uint32_t* d_word, const double* d_weight,
                         const int* d_count, int max_n);
/* KeyFrameDatabase::erase (:50-52): an absent id is not an error. */
int orbx_kfdb_erase(orbx_kfdb* db, uint64_t keyframe_id);
int orbx_kfdb_set_bad(orbx_kfdb* db, uint64_t keyframe_id, int is_bad);
/* n_entries: live entries; n_slots: table rows including tombstones (either may be NULL). */
int orbx_kfdb_size(const orbx_kfdb* db, int* n_entries, int* n_slots);
int orbx_kfdb_compact(orbx_kfdb* db);
/* Reads one entry back (synchronous): *n words into word / weight [cap] (ORBX_ERR_CAPACITY with *n set when cap is too small). */
int orbx_kfdb_download(orbx_kfdb* db, uint64_t keyframe_id, uint32_t* word, double* weight, int cap, int* n, int* map_index, int* is_bad);
/* The scores of one query vector against every entry: ids [cap] in ascending keyframe id and scores [cap], *n_out = entries
 * (ORBX_ERR_CAPACITY when cap is smaller).  Synchronous. */
int orbx_kfdb_score(orbx_kfdb* db, int scoring, const uint32_t* q_word, const double* q_weight, int nq, uint64_t* ids, double* scores, int cap,
                    int* n_out);
/* KeyFrameDatabase::detect_candidates (keyframe_db.rs:58-94): DOT score against every entry, entries of exclude_map skipped
 * (exclude_map < 0: None), kept iff score > 0.0, score descending, truncated to max_results.  ids / scores [max_results],
 * map_indices [max_results] or NULL; *n_out <= max_results. */
int orbx_kfdb_detect_candidates(orbx_kfdb* db, const uint32_t* q_word, const double* q_weight, int nq, int exclude_map, int max_results,
                                uint64_t* ids, int* map_indices, double* scores, int* n_out);
/* detect_loop_candidates (detector.rs:185-368) for a current keyframe that is an entry (an unknown id: *count = 0, :195-204).
 * connected [n_connected]: the ids of get_connected_keyframes (:232-262) in the order the caller iterates them — map bookkeeping
 * that stays on the host.  Threshold (:265-298): connected[] is walked as given (a repeated id counts again), ids that are not
 * entries of the current keyframe's map are skipped, each other one is scored, bad or not, until max_covisibles_to_check are;
 * fewer than min_covisibles_for_threshold scored: threshold 0; else best * min_score_ratio; a threshold < 0.01: no candidates
 * (:212-215).  get_connected_keyframes inserts the current keyframe itself (:234) and compute_min_score does not exclude it: the
 * library scores whatever the caller lists.  Candidates (:301-358): entries of the current keyframe's map, not in
 * connected[], |id - current| >= min_temporal_gap as u64, not bad, score >= threshold; score descending (:361-365).
 * ids / scores [cap]: the first min(*count, cap) candidates; *count: all of them (it may exceed cap). */
int orbx_kfdb_detect_loop_candidates(orbx_kfdb* db, const orbx_loop_detector_config* cfg, int scoring, uint64_t current_id, const uint64_t* connected,
                                     int n_connected, int cap, uint64_t* ids, double* scores, int* count);
/* n_queries current keyframes in one call: query q owns connected [connected_offsets[q], connected_offsets[q+1]) (offsets
 * [n_queries+1], ascending from 0); ids / scores [n_queries][cap], counts [n_queries].  A query's result is the same bytes alone
 * and inside any batch. */
int orbx_kfdb_detect_loop_candidates_batch(orbx_kfdb* db, const orbx_loop_detector_config* cfg, int scoring, int n_queries, const uint64_t* current_ids,
                                           const int* connected_offsets, const uint64_t* connected, int cap, uint64_t* ids, double* scores,
                                           int* counts);

/* Per-kernel device time for bench.py's roofline block.  While profiling is on
 * (orbx_set_profiling), every launch is bracketed by HIP events on the handle's stream;
 * orbx_get_kernel_times synchronises, fills up to `cap` entries with the durations summed
 * over all calls since the previous read (returns the number of kernels seen), and starts a
 * new accumulation window. */
typedef struct {
  char name[48];
  float ms;          /* summed duration of this kernel's launches in the window */
  int launches;
} orbx_kernel_time;
int orbx_set_profiling(orbx_handle* h, int on);
/* The same with the events around the launches of ONE kernel only (its name as orbx_get_kernel_times reports it): what a
 * timed region that needs one kernel's durations pays — two event records per launch of that kernel instead of two per
 * launch of every kernel (about 1.5 % of a 256-pair step).  NULL or "" = every kernel, as orbx_set_profiling(h, 1). */
int orbx_set_profiling_only(orbx_handle* h, const char* kernel_name);
int orbx_get_kernel_times(orbx_handle* h, orbx_kernel_time* out, int cap);

/* ---- stage inspection (tests, debugging) ---------------------------------------------------
 * Read back intermediate results of the LAST extraction call of this handle: one pyramid level
 * (which = 0) or its blurred version (which = 1) of image `image_index` as w_l*h_l tightly
 * packed bytes (out may be NULL to query the size), and the FAST+NMS candidates of a level packed
 * as (score<<24 | y<<12 | x) in no particular order.  Synchronous. */
int orbx_debug_read_level(orbx_handle* h, int image_index, int level, int which, uint8_t* out,
                          int* w_l, int* h_l);
int orbx_debug_read_candidates(orbx_handle* h, int image_index, int level, uint32_t* out, int cap,
                               int* n);

/* The per-observation terms of the BA linearisation at the given parameters, from the same device functions the solver's
 * kernels call: compute_residuals (local_ba_lm.rs:557-588) and the blocks of compute_jacobian (:591-639; jacobian_pose
 * :216-254, jacobian_point :257-288, huber_weight :291-297), in input order.
 *   out [N][20] = residual (2) | A = d r / d pose, row-major 2x6 (rot xyz, trans xyz) | B = d r / d point, row-major 2x3,
 *   all times sqrt(w).  global_mode != 0: the zero-Jacobian rule of solve_global_ba (global_ba.rs:561-563).
 * This is how the reference's Jacobian known answer (test_jacobian_pose_numerical, :1163-1243) is checked on the GPU. */
int orbx_debug_ba_blocks(orbx_handle* h, const orbx_camera* cam, const orbx_ba_config* cfg, int K, const double* poses_cw,
                         int F, const double* fixed_poses_cw, int M, const double* points, int N, const orbx_ba_obs* obs,
                         int global_mode, double* out);

/* compute_imu_residual (src/optimizer/imu_factors.rs:66-103) of every IMU edge at the given keyframe states, from the device
 * function the inertial solver's ba_imu_kernel calls.
 *   poses_wc [K][7] (qw,qx,qy,qz,tx,ty,tz) T_wc, velocities [K][3], edge_kf [E][2] = (i, j), preint [E][11] as orbx_ba_solve_inertial
 *   (delta_rot qw,qx,qy,qz | delta_vel | delta_pos | dt);  out [E][9] = rotation | velocity | position residual.
 * This is how the reference's own known answer for this factor (test_imu_residual_zero_motion, imu_factors.rs:264-276: identical
 * states and an identity preintegration give a zero residual) is checked on the GPU. */
int orbx_debug_imu_residual(orbx_handle* h, int K, const double* poses_wc, const double* velocities, int E, const int* edge_kf,
                            const double* preint, double* out);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
