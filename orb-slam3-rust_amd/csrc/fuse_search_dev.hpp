// fuse_search_dev.hpp — the fuse search of one (map point, target keyframe) pair per thread (search_in_neighbors.rs:273-343,
// keyframe.rs:408-443), shared by fuse_search_kernel (match_kernels.hip: the targets' features side by side in one array) and
// mf_search_kernel (map_store_kernels.hip: every target's features where its resident keyframe keeps them).
// Project, clamp the depth-scaled radius to [10, 50] px, scan the keyframe's keypoints inside the circle, keep the smallest Hamming
// distance below the threshold (lowest index on ties).  The keyframe's keypoint coordinates stream through LDS and every thread
// tests all of them (the reference's linear scan, in f64 so that the <= r^2 gate is exact).
// Device code only, inside an anonymous namespace: each translation unit that includes it gets its own copy.
#pragma once
#include "guided_search_dev.hpp"

#define FUSE_CHUNK 2048
#define FUSE_THREADS 128

namespace {

// LDS of one workgroup of FUSE_THREADS threads
struct FuseLds {
  double2 xy[FUSE_CHUNK];                      // widened once per block: the circle test is f64 (keyframe.rs:435-437)
  unsigned short hits[4][FUSE_THREADS];
};

// Every thread of the workgroup calls it (barriers inside); `valid`: the thread has a point to search.  position / desc: the point's
// rows; q: the keyframe's inverse pose from the host (se3.rs:56-63); kps / descs [n]: the keyframe's features.
// -> (distance << 32 | feature), ~0: no match
__device__ __forceinline__ unsigned long long fuse_search_point(const orbx_camera& cam, bool valid, const double* __restrict__ position,
                                                                const uint8_t* __restrict__ desc, const double* __restrict__ q,
                                                                const orbx_keypoint* __restrict__ kps, const uint8_t* __restrict__ descs, int n,
                                                                double radius_scale, unsigned thr, FuseLds& lds) {
  double u = 0.0, v = 0.0, r2 = -1.0;
  Desc256 dq{};
  if (valid) {
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double px = position[0], py = position[1], pz = position[2];
    const double t0 = 2.0 * (qy * pz - qz * py), t1 = 2.0 * (qz * px - qx * pz), t2 = 2.0 * (qx * py - qy * px);
    const double c0 = qy * t2 - qz * t1, c1 = qz * t0 - qx * t2, c2 = qx * t1 - qy * t0;
    const double x = (t0 * qw + c0 + px) + q[4], y = (t1 * qw + c1 + py) + q[5], z = (t2 * qw + c2 + pz) + q[6];
    valid = !(z <= 0.0);                                                   // :286
    if (valid) {
      u = cam.fx * x / z + cam.cx;                                         // :291-292
      v = cam.fy * y / z + cam.cy;
      const double width = cam.cx * 2.0, height = cam.cy * 2.0;
      valid = !(u < 0.0 || u >= width || v < 0.0 || v >= height);          // :297
      const double radius = radius_scale * z / cam.fx;                     // :303
      const double sr = fmax(fmin(radius, 50.0), 10.0);                    // :304
      r2 = sr * sr;
      dq = load_desc(desc);
    }
  }
  // Hits are rare (about one per query) but each costs a dependent 32-byte global load; they are parked in a
  // 4-entry list (LDS, one column per thread) and scored together so that a wave stalls once per flush instead of
  // once per hit.  The scan itself is unrolled by 8 so that the LDS reads and the f64 chains of 8 tests overlap.
  unsigned long long best = ~0ull;
  int nh = 0, cbase = 0;
  auto flush = [&]() {
    Desc256 dd[4];
    int id[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < nh) { id[k] = cbase + lds.hits[k][threadIdx.x]; dd[k] = load_desc(descs + 32 * (size_t)id[k]); }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < nh) {
        const unsigned d = hamming(dq, dd[k]);
        if (d < thr) {                                                     // :336
          const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)id[k];
          best = key < best ? key : best;
        }
      }
    }
    nh = 0;
  };
  for (int c = 0; c < n; c += FUSE_CHUNK) {
    const int m = min(FUSE_CHUNK, n - c);
    if (nh) flush();                                                       // list entries are relative to cbase
    cbase = c;
    __syncthreads();
    for (int i = threadIdx.x; i < FUSE_CHUNK; i += FUSE_THREADS)
      lds.xy[i] = i < m ? make_double2((double)kps[c + i].x, (double)kps[c + i].y) : make_double2(1e300, 1e300);
    __syncthreads();
    if (valid) {
      for (int i = 0; i < m; i += 8) {                                     // padding entries never pass the gate
        unsigned mask = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const double2 w = lds.xy[i + k];
          const double du = w.x - u, dv = w.y - v;
          mask |= (du * du + dv * dv <= r2 ? 1u : 0u) << k;
        }
        while (mask) {
          const int k = __ffs(mask) - 1;
          mask &= mask - 1;
          lds.hits[nh][threadIdx.x] = (unsigned short)(i + k);
          if (++nh == 4) flush();
        }
      }
    }
  }
  if (nh) flush();
  return best;
}

}  // namespace
