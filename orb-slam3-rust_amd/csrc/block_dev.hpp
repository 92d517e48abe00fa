// block_dev.hpp — workgroup primitives shared by the kernels: the fixed-order block sum (int or f64), the ordered append, the
// ordered scan of counts and the counter scan of the counting sorts ("Workgroup primitives").  Every thread of the
// workgroup must reach each call — a call under a condition that is not uniform over the block hangs it; THREADS is the
// workgroup's size, a multiple of 64.
// Device code only, inside an anonymous namespace: each translation unit that includes it gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// Fixed-order sum of NV values (int or double) over the workgroup, in every thread: shuffle tree inside each wave, then every thread
// adds the wave totals in wave order (the same bits in every thread, whatever the batch).  s_w: LDS [THREADS / 64][NV].  One barrier
// before the store (s_w may still be read from an earlier use) and one after.
template <int THREADS, int NV, typename T>
__device__ __forceinline__ void block_sum(T (&v)[NV], T* __restrict__ s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
  }
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) s_w[wave * NV + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    T t = 0;
    for (int w = 0; w < THREADS / 64; ++w) t += s_w[w * NV + k];
    v[k] = t;
  }
}

// The workgroup's sum of one int.  wave_tot: LDS [THREADS / 64].
template <int THREADS>
__device__ __forceinline__ int block_sum(int v, int* wave_tot) {
  int a[1] = {v};
  block_sum<THREADS, 1>(a, wave_tot);
  return a[0];
}

// Ordered append of NF flag sets at once.  Each round every thread passes its flags; at[f] is the number of threads flagged in f
// before this one, in thread order, over this and all earlier rounds, plus whatever total[f] started from — the place of a flagged
// thread's entry.  total[f] is the same in every thread: the count so far, which a caller may set between rounds (a list that
// continues another's).  Two barriers per round; the first also covers an earlier use of the same LDS.
template <int THREADS, int NF>
struct BlockAppend {
  int* wave_tot;      // LDS [THREADS / 64][NF]
  int total[NF];
  __device__ __forceinline__ explicit BlockAppend(int* lds) : wave_tot(lds) {
#pragma unroll
    for (int f = 0; f < NF; ++f) total[f] = 0;
  }
  __device__ __forceinline__ void round(const bool (&flag)[NF], int (&at)[NF]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long m[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) m[f] = __ballot(flag[f]);
    __syncthreads();                                                      // (the previous round's totals are no longer read)
    if (lane == 0) {
#pragma unroll
      for (int f = 0; f < NF; ++f) wave_tot[wave * NF + f] = __popcll(m[f]);
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int before = 0, all = 0;
#pragma unroll
      for (int w = 0; w < THREADS / 64; ++w) { const int t = wave_tot[w * NF + f]; before += w < wave ? t : 0; all += t; }
      at[f] = total[f] + before + __popcll(m[f] & ((1ull << lane) - 1ull));
      total[f] += all;
    }
  }
  __device__ __forceinline__ int round(bool flag) {                       // NF == 1
    const bool fl[1] = {flag};
    int at[1];
    round(fl, at);
    return at[0];
  }
};

// Inclusive scan of v over the 64 lanes of a wave: the one step the scans below share.  No LDS, no barrier.
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// Ordered exclusive scan of counts: BlockAppend from flags to counts.  Each round every thread passes its count and gets the number
// of items of the threads before it, in thread order, over this and all earlier rounds, plus whatever `total` started from (a list
// behind a base) — the place of the thread's first item.  total is the same in every thread: the count so far.  Two barriers per
// round; the first also covers an earlier use of the same LDS.
// round<false> is for a single round whose total only the last thread needs, or nobody (a counting sort's end sentinel): a thread
// adds the waves before it and no more, and total is the block's in thread THREADS - 1 alone.  No round may follow it.  (Sixteen
// wave totals summed in every thread cost a 1024-thread counting sort some 20 VGPRs and 35 instructions, and the one-launch stereo
// matcher a wave of occupancy: profiles/block_scan_codegen.txt.)
template <int THREADS, typename T = int>
struct BlockScan {
  T* wave_tot;        // LDS [THREADS / 64]
  T total;
  __device__ __forceinline__ explicit BlockScan(T* lds, T start = 0) : wave_tot(lds), total(start) {}
  template <bool UNIFORM = true>
  __device__ __forceinline__ T round(T count) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive_scan(count);
    __syncthreads();                                                      // (the previous round's totals are no longer read)
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
    if (UNIFORM) {
#pragma unroll
      for (int w = 0; w < THREADS / 64; ++w) { const T t = wave_tot[w]; before += w < wave ? t : 0; all += t; }
    } else {
      for (int w = 0; w < wave; ++w) before += wave_tot[w];
      all = before + incl;                                                // (the last thread's: the block's)
    }
    const T at = total + before + incl - count;
    total += all;
    return at;
  }
};

struct NoEmit {
  template <typename T>
  __device__ __forceinline__ void operator()(int, T) const {}
};

// In-place exclusive prefix over THREADS x PER counters in LDS (int or unsigned), thread t scanning counters [PER t, PER t + PER):
// the middle of a counting sort.  emit(i, start) is called by that thread with every counter's start as it is produced, from
// registers (a sort writes its cell_start there).  Returns the total, as BlockScan<THREADS>::round<UNIFORM> leaves it: in every
// thread, or with UNIFORM = false in the last thread only — the end sentinel, written by the caller in one place.
// wave_tot: LDS [THREADS / 64].  The caller puts a barrier between the last update of the counters and this call, and one between
// this call and the first read of a start from LDS; inside, BlockScan's two.
template <int THREADS, int PER, bool UNIFORM = true, typename T, typename Emit = NoEmit>
__device__ __forceinline__ T block_counter_scan(T* cnt, T* wave_tot, Emit emit = Emit()) {
  const int i0 = PER * threadIdx.x;
  T c[PER], tot = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) { c[k] = cnt[i0 + k]; tot += c[k]; }
  BlockScan<THREADS, T> scan(wave_tot);
  T run = scan.template round<UNIFORM>(tot);
#pragma unroll
  for (int k = 0; k < PER; ++k) { emit(i0 + k, run); cnt[i0 + k] = run; run += c[k]; }
  return scan.total;
}

}  // namespace
