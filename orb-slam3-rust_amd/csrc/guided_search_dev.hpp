// guided_search_dev.hpp — device code shared by the matchers (match_kernels.hip) and the frame tracker (track_kernels.hip):
// 256-bit descriptors, the FeatureGrid of tracking_frame.rs:52-128 as a counting sort, and the tracker's descriptor search
// over the cells around a projected position (tracker.rs:880-923, :1126-1157), one wave per query.
// Device code only, inside an anonymous namespace: each translation unit that includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/orbx.h"
#include "block_dev.hpp"

namespace {

constexpr int kWave = 64;
constexpr unsigned TH_HIGH = 100;  // stereo.rs:10

struct Desc256 {
  unsigned long long w[4];
};

__device__ __forceinline__ Desc256 load_desc(const uint8_t* p) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
  Desc256 d;
  d.w[0] = q[0]; d.w[1] = q[1]; d.w[2] = q[2]; d.w[3] = q[3];
  return d;
}
__device__ __forceinline__ unsigned hamming(const Desc256& a, const Desc256& b) {
  return (unsigned)(__popcll(a.w[0] ^ b.w[0]) + __popcll(a.w[1] ^ b.w[1]) +
                    __popcll(a.w[2] ^ b.w[2]) + __popcll(a.w[3] ^ b.w[3]));
}

// ---- guided matching: FeatureGrid (tracking_frame.rs:52-128) + the tracker's two search rules -----------------
constexpr int GG_COLS = 64, GG_ROWS = 48, GG_CELLS = GG_COLS * GG_ROWS;   // tracking_frame.rs:43-44
constexpr int GG_THREADS = 1024;                                          // three cells per thread in the scan
static_assert(GG_CELLS == 3 * GG_THREADS, "three counters per thread in the scan");

// Rust `f64 as usize`: truncation, negative / NaN -> 0
__device__ __forceinline__ int sat_cell(double v, int last) {
  return (v > 0.0) ? (v >= (double)(last + 1) ? last : (int)v) : 0;
}
// Rust `f64 as i32`: saturating, NaN -> 0
__device__ __forceinline__ int sat_i32(double v) {
  if (v != v) return 0;
  if (v <= -2147483648.0) return INT_MIN;
  if (v >= 2147483647.0) return INT_MAX;
  return (int)v;
}

// One block of GG_THREADS: counting sort of the keypoints by grid cell (CSR: cell_start[GG_CELLS+1], sorted_idx[n]) and the
// cell of every keypoint.  The order inside a cell is irrelevant: ties are broken on (cell, index) explicitly.
__device__ __forceinline__ void grid_build_body(const orbx_keypoint* __restrict__ kp, int n, double winv, double hinv,
                                                int* __restrict__ cell_start, int* __restrict__ sorted_idx,
                                                unsigned short* __restrict__ cell_of) {
  __shared__ int cnt[GG_CELLS];
  __shared__ int wsum[GG_THREADS / 64];
  const int tid = threadIdx.x;
  for (int i = tid; i < GG_CELLS; i += GG_THREADS) cnt[i] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += GG_THREADS) {
    const int cx = sat_cell(((double)kp[i].x - 0.0) * winv, GG_COLS - 1);     // tracking_frame.rs:66-75
    const int cy = sat_cell(((double)kp[i].y - 0.0) * hinv, GG_ROWS - 1);
    const int c = cy * GG_COLS + cx;
    cell_of[i] = (unsigned short)c;
    atomicAdd(&cnt[c], 1);
  }
  __syncthreads();
  const int total = block_counter_scan<GG_THREADS, GG_CELLS / GG_THREADS, false>(cnt, wsum, [&](int i, int start) { cell_start[i] = start; });
  if (tid == GG_THREADS - 1) cell_start[GG_CELLS] = total;                // (round<false>: the last thread holds the total)
  __syncthreads();
  for (int i = tid; i < n; i += GG_THREADS) sorted_idx[atomicAdd(&cnt[cell_of[i]], 1)] = i;
}

// The descriptor search of one query at (x, y) by one wave (every lane calls it with the same arguments and its own `lane`).
// key = (distance << 48 | cell << 32 | index): the minimum key is the smallest distance, and among equal distances the first
// candidate in the reference's visiting order (cells row-major, indices ascending inside a cell).  `second` is the second
// smallest distance of the multiset.  Returns, on every lane, the matched keypoint index or -1, and its distance in *dist.
//   mode 0  track_with_motion_model (tracker.rs:1126-1157): smallest distance < TH_HIGH;
//   mode 1  track_local_map (tracker.rs:880-923): best <= TH_HIGH and, with more than one candidate, !(best > 0.75 second).
__device__ __forceinline__ int guided_search_wave(const uint8_t* __restrict__ desc, const int* __restrict__ cell_start,
                                                  const int* __restrict__ sorted_idx, const unsigned short* __restrict__ cell_of,
                                                  double x, double y, const Desc256& dq, double radius, double winv, double hinv,
                                                  int mode, int lane, unsigned* dist) {
  // tracking_frame.rs:107-117, including `(max as usize).min(cols - 1)`: a negative max wraps -> last cell
  const int mnx = sat_i32(floor((x - 0.0 - radius) * winv)), mxx = sat_i32(ceil((x - 0.0 + radius) * winv));
  const int mny = sat_i32(floor((y - 0.0 - radius) * hinv)), mxy = sat_i32(ceil((y - 0.0 + radius) * hinv));
  const int x0 = max(mnx, 0), y0 = max(mny, 0);
  const int x1 = (mxx < 0 || mxx > GG_COLS - 1) ? GG_COLS - 1 : mxx;
  const int y1 = (mxy < 0 || mxy > GG_ROWS - 1) ? GG_ROWS - 1 : mxy;
  unsigned long long bk = ~0ull;
  unsigned s = 0xffffffffu;
  int total = 0;
  if (x0 <= x1) {
    for (int cy = y0; cy <= y1; ++cy) {
      const int lo = cell_start[cy * GG_COLS + x0], hi = cell_start[cy * GG_COLS + x1 + 1];
      total += hi - lo;
      for (int t = lo + lane; t < hi; t += kWave) {
        const int i = sorted_idx[t];
        const unsigned d = hamming(dq, load_desc(desc + (size_t)i * 32));
        if (mode == 0 && d >= TH_HIGH) continue;                          // tracker.rs:1146
        const unsigned long long key = ((unsigned long long)d << 48) | ((unsigned long long)cell_of[i] << 32) | (unsigned)i;
        if (key < bk) { s = min(s, (unsigned)(bk >> 48)); if (bk == ~0ull) s = 0xffffffffu; bk = key; }
        else s = min(s, d);
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long ok = __shfl_xor(bk, off);
    const unsigned os = __shfl_xor(s, off);
    const unsigned long long mn = ok < bk ? ok : bk, mx = ok < bk ? bk : ok;
    unsigned ns = min(s, os);
    if (mx != ~0ull) ns = min(ns, (unsigned)(mx >> 48));
    bk = mn; s = ns;
  }
  int res = -1;
  unsigned rd = 0;
  if (bk != ~0ull) {
    const unsigned best = (unsigned)(bk >> 48);
    const int bi = (int)(unsigned)(bk & 0xffffffffull);
    if (mode == 0) { res = bi; rd = best; }
    else if (total > 0 && best <= TH_HIGH &&                                        // tracker.rs:884-886, :907-909
             !(total > 1 && (float)best > 0.75f * (float)s)) { res = bi; rd = best; }   // :911-915
  }
  *dist = rd;
  return res;
}

}  // namespace
